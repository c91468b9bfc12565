"""Instances of the STAFF family at the smallest shapes where a group's action loop (`for a0 ...; a0 += R` of the
register-blocked kernels in csrc/sdp_staff.hpp) has a second trip, the switch sets that reach every kernel form, and the
geometry read off a launch plan.  Shared by tests/test_staff_plan.py (host arithmetic, no GPU) and
tests/test_gpu_staff_blocks.py (parity against oracle/staffref.c)."""
import numpy as np
from scipy import stats

import staff_cases
from staff_cases import StaffCase, StaffFunctor

SWITCHES = ("SDPGPU_STAFF_R", "SDPGPU_STAFF_BLOCK", "SDPGPU_STAFF_PAIR", "SDPGPU_STAFF_WIN", "SDPGPU_STAFF_LANES",
            "SDPGPU_STAFF_UNI")

# label -> environment ("auto": the launcher's own choice by the size of the staff range); EXPECTED below says what each reaches
SWITCH_SETS = {
    "auto": {},
    "win4": {"SDPGPU_STAFF_PAIR": "1", "SDPGPU_STAFF_WIN": "4"},
    "win2": {"SDPGPU_STAFF_WIN": "2"},
    "win4_staged": {"SDPGPU_STAFF_WIN": "4", "SDPGPU_STAFF_UNI": "0"},
    "pair": {"SDPGPU_STAFF_WIN": "0"},
    "block4": {"SDPGPU_STAFF_PAIR": "0"},
    "block8": {"SDPGPU_STAFF_PAIR": "0", "SDPGPU_STAFF_R": "8"},
    "plain": {"SDPGPU_STAFF_BLOCK": "0"},
}
LANES = {"SDPGPU_STAFF_LANES": "1"}  # on few_states only: one workgroup per state and 64 actions

# (r, s, static LDS?) of a plan -> the form it names
FORM_NAMES = {(64, 1, False): "lanes", (1, 1, False): "plain", (4, 1, False): "block4", (8, 1, False): "block8",
              (4, 2, False): "pair", (4, 2, True): "win2", (4, 4, True): "win4"}
REGISTER_BLOCKED = ("block4", "block8", "pair", "win2", "win4")


def set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def truncated_table(rate, rows, cap, T):
    """Binomial(y, rate) turnover cut to its first min(y + 1, cap) realisations and renormalised: (T, rows, cap) and the
    row lengths.  The rate is small enough that the kept entries carry the mass (mean turnover rows * rate < cap)."""
    y = np.arange(rows)[:, None]
    j = np.arange(cap)[None, :]
    p = stats.binom.pmf(j, y, rate)
    row_len = np.minimum(np.arange(rows) + 1, cap).astype(np.int32)
    p[j >= row_len[:, None]] = 0.0
    p /= p.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(np.broadcast_to(p, (T, rows, cap))), row_len


def ragged_table(rate, rows, cap, T, seed):
    """Every level's length drawn from 1 .. min(y + 1, cap) on its own (neighbouring levels of unequal, non-monotone lengths);
    the caller's array holds NaN behind every row's length -- the reference's rows are jagged arrays, nothing is there."""
    rng = np.random.default_rng(seed)
    row_len = rng.integers(1, np.minimum(np.arange(rows) + 1, cap) + 1).astype(np.int32)
    y = np.arange(rows)[:, None]
    j = np.arange(cap)[None, :]
    p = stats.binom.pmf(j, y, rate)
    beyond = j >= row_len[:, None]
    p[beyond] = 0.0
    p /= p.sum(axis=1, keepdims=True)
    p[beyond] = np.nan
    return np.ascontiguousarray(np.broadcast_to(p, (T, rows, cap))), row_len


def _functor(min_staff, max_hire, max_x=None, costs=(50.0, 2.5, 5.0, 37.0)):
    K, v, salary, pen = costs
    if max_x is None:
        return StaffFunctor(fixCost=K, unitVariCost=v, salary=salary, unitPenalty=pen, minStaffNum=list(min_staff),
                            maxHireNum=max_hire, clampStaff=False, iniStaffNum=0)
    return StaffFunctor(fixCost=K, unitVariCost=v, salary=salary, unitPenalty=pen, minStaffNum=list(min_staff),
                        maxHireNum=max_hire, minX=0, maxX=max_x, clampStaff=True, iniStaffNum=0)


# (the table lengths leave (rows - 1) % 8 = 3: with staff numbers from 0 and groups of 8 actions some window wave then starts below
# the table's last row and ends on or beyond it -- the staged and the scalar path in one loop)
def clamped_wide():
    """8200 staff numbers x 2101 hires: 5 / 3 / 2 trips at tiles of 64 / 128 / 256 states."""
    table, row_len = truncated_table(0.002, 2996, 12, 2)
    return StaffCase("clamped_wide", _functor([900, 941], 2100, 8199), table, row_len)


def clamped_mid():
    """4160 x 1101: the block kernel's smallest shape with two trips (tiles of 64 states)."""
    table, row_len = truncated_table(0.003, 1500, 9, 3)
    return StaffCase("clamped_mid", _functor([873, 900, 958], 1100, 4159), table, row_len)


def few_states():
    """1500 x 5501: two states per lane from the window by the launcher's own choice, two trips."""
    table, row_len = truncated_table(0.006, 700, 10, 2)
    return StaffCase("few_states", _functor([900, 866], 5500, 1499), table, row_len)


def growing():
    """Unclamped from 0: staff ranges of 1, 2101, 4201, 6301 and 8401 numbers."""
    table, row_len = truncated_table(0.0025, 2196, 12, 5)
    return StaffCase("growing", _functor([851, 900, 927, 884, 969], 2100), table, row_len)


def long_rows():
    """Full binomial rows (no row_len): step loops of hundreds of steps under the block kernel's second trip."""
    return StaffCase("long_rows", _functor([900, 1013], 1100, 4159), staff_cases.staff_level_pmf([0.3, 0.3], 396))


def ties_closed_form(c):
    """Last period with K = v = salary = 0: a level y with y - (cap - 1) >= minStaff leaves no realisation below minStaff and
    costs exactly +0.0; the first such action is max(0, minStaff + cap - 1 - x).  -> (that action per state, where the hire
    limit allows it)."""
    cap = c.table.shape[2]
    x = c.functor.minX + np.arange(c.functor.maxX - c.functor.minX + 1)
    want = np.maximum(0, c.functor.minStaffNum[-1] + cap - 1 - x)
    return want, want <= c.functor.maxHireNum


def ties():
    """K = v = salary = 0: every action whose level clears minStaff + cap - 1 costs exactly +0.0 and the strict compare
    keeps the first of them."""
    table, row_len = truncated_table(0.003, 1500, 9, 3)
    return StaffCase("ties", _functor([900, 37, 2500], 1100, 4159, costs=(0.0, 0.0, 0.0, 37.0)), table, row_len)


def ties_wide():
    """ties at clamped_wide's size, where the pair and the window kernels have their second trip too."""
    table, row_len = truncated_table(0.002, 2996, 12, 2)
    return StaffCase("ties_wide", _functor([37, 5000], 2100, 8199, costs=(0.0, 0.0, 0.0, 37.0)), table, row_len)


def ragged_rows():
    table, row_len = ragged_table(0.0015, 2996, 9, 3, seed=20)
    return StaffCase("ragged_rows", _functor([873, 900, 958], 1100, 4159), table, row_len)


def ragged_wide():
    """ragged_rows at clamped_wide's size: rows of unequal lengths under every form's second trip."""
    table, row_len = ragged_table(0.002, 2996, 12, 2, seed=21)
    return StaffCase("ragged_wide", _functor([900, 941], 2100, 8199), table, row_len)


MAIN = [clamped_wide, clamped_mid, few_states, growing, long_rows]
ALL = MAIN + [ties, ties_wide, ragged_rows, ragged_wide]


# The plan every (instance, switch set) is meant to reach: (form, trips of the action loop per group) -- one pair for all
# periods of a clamped instance, one per period of the growing one.  tests/test_staff_plan.py holds the library's own plan
# report against it without a GPU; the GPU tests assert it again before they compare tables.
_WIDE = {"auto": ("win4", 2), "win4": ("win4", 2), "win2": ("win2", 3), "win4_staged": ("win4", 2), "pair": ("pair", 3),
         "block4": ("block4", 5), "block8": ("block8", 3), "plain": ("plain", 20)}
_MID = {"auto": ("win4", 1), "win4": ("win4", 1), "win2": ("win2", 1), "win4_staged": ("win4", 1), "pair": ("pair", 1),
        "block4": ("block4", 2), "block8": ("block8", 1), "plain": ("plain", 8)}
EXPECTED = {
    "clamped_wide": _WIDE, "ragged_wide": _WIDE, "ties_wide": _WIDE,
    "clamped_mid": _MID, "long_rows": _MID, "ties": _MID, "ragged_rows": _MID,
    "few_states": {"auto": ("win2", 2), "win4": ("win4", 1), "win2": ("win2", 2), "win4_staged": ("win4", 1),
                   "pair": ("pair", 2), "block4": ("block4", 3), "block8": ("block8", 2), "plain": ("plain", 12),
                   "lanes": ("lanes", 1)},
    "growing": {
        "auto": [("lanes", 1), ("win4", 1), ("win4", 1), ("win4", 1), ("win4", 2)],
        "win4": [("lanes", 1), ("win4", 1), ("win4", 1), ("win4", 1), ("win4", 2)],
        "win2": [("lanes", 1), ("win2", 1), ("win2", 2), ("win2", 2), ("win2", 3)],
        "win4_staged": [("lanes", 1), ("win4", 1), ("win4", 1), ("win4", 1), ("win4", 2)],
        "pair": [("lanes", 1), ("pair", 1), ("pair", 2), ("pair", 2), ("pair", 3)],
        "block4": [("lanes", 1), ("block4", 2), ("block4", 3), ("block4", 4), ("block4", 5)],
        "block8": [("lanes", 1), ("block8", 1), ("block8", 2), ("block8", 2), ("block8", 3)],
        "plain": [("plain", 4), ("plain", 8), ("plain", 12), ("plain", 16), ("plain", 20)],
    },
}


# slabs of clamped_wide's last period that keep two trips on every rank: (switch set, world size)
SLABS = [("block4", 3), ("win2", 2), ("pair", 2)]


def switch_sets(c):
    sets = dict(SWITCH_SETS)
    if c.name == "few_states":
        sets["lanes"] = LANES
    return sets


def expected(c, label, period):
    e = EXPECTED[c.name][label]
    return e[period - 1] if isinstance(e, list) else e


def engine(sia, c, rank=0, world=1):
    d = c.functor.to_desc(c.T)
    d.rank, d.world_size = rank, world
    return sia.SdpEngine(d, None, [float(m) for m in c.functor.minStaffNum], level_pmf=c.table, level_row_len=c.row_len)


def form_of(pl):
    return FORM_NAMES[(pl.r, pl.s, pl.lds_bytes > 0)]


class Geometry:
    """What a launch of one period walks, from the plan the library reports (never from a restatement of its group
    arithmetic): tiles of `tile_states` states x `chunks` groups of `group_actions` actions in blocks of r."""

    def __init__(self, eng, c, period):
        pl = eng.plan(period)
        self.plan, self.form = pl, form_of(pl)
        self.n_actions = c.functor.maxHireNum + 1
        self.n_rows = c.table.shape[1]
        self.x_lo = int(eng.grid(period)[0])
        _, self.lo, self.hi = eng.slab(period)
        self.states = self.hi - self.lo
        self.r, self.chunk_blocks = pl.r, pl.chunk_blocks
        self.group_actions = pl.r * pl.chunk_blocks
        assert pl.tasks == pl.tiles * pl.chunks and pl.kernel == 1  # KERNEL_GATHER, what stats reports
        assert (pl.chunks - 1) * self.group_actions < self.n_actions <= pl.chunks * self.group_actions
        # states per tile: one for lanes-are-actions, else 64 s (the pair kernel and the window kernel carry s per lane)
        self.tile_states = 1 if self.form == "lanes" else 64 * pl.s
        assert pl.tiles == -(-self.states // self.tile_states)

    def ragged_ends(self):
        """A ragged last group whose last block is partial, on a ragged last tile."""
        return (self.n_actions % self.group_actions != 0 and self.n_actions % self.r != 0 and
                self.states % self.tile_states != 0)

    def mixed_waves(self):
        """Window form: (tile, group) pairs whose first block lies below the table's last row (staged path) while a later
        block of the same loop lies on or beyond it (scalar path): Y0 = lowest level of a block."""
        if self.form not in ("win2", "win4"):
            return 0
        last_row = self.n_rows - 1
        n = 0
        for tile in range(self.plan.tiles):
            x0 = self.x_lo + self.lo + tile * self.tile_states
            for g in range(self.plan.chunks):
                a0 = g * self.group_actions
                a_end = min(self.n_actions, a0 + self.group_actions)
                blocks = range(a0, a_end, self.r)
                if x0 + blocks[0] < last_row and any(x0 + a >= last_row for a in blocks[1:]):
                    n += 1
        return n

    def block_shares(self, pol):
        """Of the states that hire, the share whose best action lies in the first block of its group / in a later one."""
        hires = pol[pol > 0]
        later = np.count_nonzero(hires % self.group_actions >= self.r)
        return (len(hires) - later) / max(1, len(hires)), later / max(1, len(hires)), len(hires)
