"""Tables and parameters shared by tests/test_cash_structure_host.py (the host entry point against the twin) and part c of
tests/test_gpu_cash_structure.py (the device against the host entry point): random tables, tables of special values, and
hand-built tables on which each of the three checks fails at a pinned index.  `expected` is the twin's answer to a whole
request; `compare` holds a CashStructure to it by bits."""
import numpy as np

import cash_structure_twin as tw

ALL = 0x3ff
SLOTS = ("h", "gagb", "fg")

# (min_cash, fix_cost, vari_cost): the drivers' (0, 10, 1); non-integer variCost, where the (int) truncations matter; a negative
# minCash, so that cashIndex < 0 is skipped; K = 0; v = 0 ((cash - K) / 0 saturates the (int), j + Qbound wraps); v < 0; K = NaN
PARAMS = [(0.0, 10.0, 1.0), (0.0, 2.5, 0.7), (-3.0, 1.0, 1.3), (0.0, 0.0, 0.37), (1.0, 3.0, 0.0), (0.0, 4.0, -0.5), (2.0, 2.0, 2.0 / 3.0),
          (0.0, float("nan"), 1.0)]


def random_tables(seed, n_r, n_x, scale=3.0):
    rng = np.random.default_rng(seed)
    return {name: rng.normal(scale=scale, size=(n_r, n_x)) for name in ("g", "ga", "gb", "f")}


def special_tables(seed, n_r, n_x):
    """Random tables salted with NaN, +-inf, -0.0, and -- in every table, hence in H = -K rows, GB - GA - K and F - G alike --
    steps of exactly +-0.1 between neighbours (0.1 and -0.1 themselves sit in the tables too)."""
    rng = np.random.default_rng(seed)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.1, -0.1, 1.0, -1.0, 0.2, 0.30000000000000004, 5e-324, 1e308])
    out = {}
    for name in ("g", "ga", "gb", "f"):
        t = rng.normal(size=(n_r, n_x))
        pick = rng.random((n_r, n_x)) < 0.35
        t[pick] = rng.choice(pool, size=int(pick.sum()))
        out[name] = t
    return out


def threshold_table(n_r, n_x):
    """Entries exactly at -0.1 (fails the single crossing's `> -0.1`) and neighbours exactly 0.1 / -0.1 apart (fail `< 0.1` /
    `> -0.1`): 0.1 * (i + j) has such steps only where the product rounds that way, so the steps are laid down by addition."""
    t = np.zeros((n_r, n_x))
    for i in range(n_r):
        for j in range(n_x):
            t[i, j] = (0.1 if (i + j) % 2 else 0.0) - (0.1 if i % 3 == 2 else 0.0)
    return t


def expected(mask, tables, min_cash, K, v, given=()):
    """The twin's answer: ({name: table}, {key: verdict}).  `given`: names of derived tables taken from `tables` as they are."""
    need = [bool(mask & (1 << s)) or bool(mask & (0x10 << s)) or bool(mask & (0x80 << s)) for s in range(3)]
    need[0] = need[0] or bool(mask & 0x8)
    tabs = {}
    if need[0]:
        if "h" in given:
            tabs["h"] = tables["h"]
        else:
            tabs["h"], tabs["opt_y"] = tw.getH(tables["g"], min_cash, K, v, with_index=True)
    if need[1]:
        tabs["gagb"] = tables["gagb"] if "gagb" in given else tw.getMinusGAGB(tables["ga"], tables["gb"], min_cash, K, v)
    if need[2]:
        tabs["fg"] = tables["fg"] if "fg" in given else tw.getMinusFG(tables["g"], tables["f"], min_cash, K, v)
    ver = {}
    if mask & 0x8:
        ver["single_crossing"] = tw.checkSingleCrossing(tabs["h"])
    for s, name in enumerate(SLOTS):
        if mask & (0x10 << s):
            ver["non_increasing:" + name] = tw.checkNonIncreasing(tabs[name])
        if mask & (0x80 << s):
            ver["non_decreasing:" + name] = tw.checkNonDecreasing(tabs[name])
    return tabs, ver


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_table(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def compare(res, want_tabs, want_ver, what):
    for name, t in want_tabs.items():
        assert same_table(res.tables[name], t), (what, name, res.tables[name], t)
    assert set(res.verdicts) == set(want_ver), (what, sorted(res.verdicts), sorted(want_ver))
    for key, v in want_ver.items():
        assert tw.same_verdict(res.verdicts[key], v), (what, key, res.verdicts[key], v)


# ---- hand-built tables: each check fails, the failing index pinned ----
def crossing_fails():
    """H of 4 x 5.  Row 0 passes up to column 1, so its rectangle is rows 0..3 x columns 0..1: row 2 fails at column 1 (and
    row 3 at column 0, later in loop order).  -> (H, verdict)"""
    H = np.full((4, 5), -1.0)
    H[0, :2] = 0.0
    H[1, :4] = 0.0
    H[2, 0] = 0.0
    H[2, 1] = -0.5
    H[3, 0] = -2.0
    H[3, 1] = 0.0
    return H, (0, 0, 1, 2, 1, -0.5)


def crossing_fails_late():
    """Rows 0 and 1 have no passing entry (lastColumnEnd stays 0), row 2 passes at column 2 only: its rectangle starts at
    column 0 and fails at once, at (2, 0).  Row 3 would fail as well."""
    H = np.full((4, 4), -1.0)
    H[2, 2] = 3.0
    H[3, 3] = np.nan
    return H, (0, 2, 2, 2, 0, -1.0)


def crossing_nan():
    """A NaN inside a rectangle violates: row 0 passes up to column 2, row 1 holds a NaN at column 1."""
    H = np.zeros((3, 4))
    H[:, 3] = -1.0
    H[1, 1] = np.nan
    return H, (0, 0, 2, 1, 1, float("nan"))


def crossing_holds():
    """A staircase: each row passes one column further than the one above, and everything left of the steps passes below."""
    H = np.full((4, 6), -1.0)
    for i in range(4):
        H[i, : i + 2] = 0.0
    return H, tw.HOLDS


def noninc_fails():
    a = np.zeros((3, 5))
    a[0] = [4, 3, 2, 1, 0]
    a[1] = [1, 1.05, 1.0, 1.2, 0]   # +0.05 passes, +0.2 fails at j = 2 (1.2 - 1.0, inexact)
    a[2] = [0, 9, 0, 0, 0]          # fails at (2, 0), later in loop order
    return a, (0, 1, 2, 1, 3, 1.2 - 1.0)


def nondec_fails():
    a = np.zeros((4, 3))
    a[:, 0] = [0, 1, 2, 3]
    a[:, 1] = [0, -0.05, 5, 4.5]    # -0.05 passes, 4.5 - 5 fails at (i, j) = (2, 1)
    a[:, 2] = [9, 0, 0, 0]          # fails at (0, 2), later in loop order (j outer)
    return a, (0, 2, 1, 3, 1, -0.5)


def nondec_holds():
    a = np.add.outer(np.arange(5.0), -np.arange(4.0))
    return a, tw.HOLDS


HAND_BUILT = [("single_crossing", crossing_fails), ("single_crossing", crossing_fails_late), ("single_crossing", crossing_nan),
              ("single_crossing", crossing_holds), ("non_increasing", noninc_fails), ("non_decreasing", nondec_fails),
              ("non_decreasing", nondec_holds)]
TWIN_CHECK = {"single_crossing": tw.checkSingleCrossing, "non_increasing": tw.checkNonIncreasing, "non_decreasing": tw.checkNonDecreasing}


def embed(table, n_r, n_x, check):
    """A hand-built table placed in the top-left corner of an n_r x n_x one whose other entries cannot change the verdict:
    the rows below repeat the last row, the columns to the right repeat the last column (differences 0) -- for the single
    crossing they are -1.0 (never pass)."""
    t = np.asarray(table, dtype=np.float64)
    r, x = t.shape
    if n_r < r or n_x < x:
        return None
    big = np.full((n_r, n_x), -1.0)
    big[:r, :x] = t
    if check != "single_crossing":
        big[:r, x:] = t[:, -1:]
    big[r:, :] = big[r - 1, :]
    return big
