"""Host twin of the batch sampler, written from its DEFINITION in DESIGN.md section 4 ("Batched simulation") in plain
Python integers and numpy -- it shares no code with csrc/sdp_batch_sim.hpp.  The GPU tests hold sdpgpu_batch_sample_demands to
it bit for bit; the host tests check the construction itself (sigma a bijection, one u per stratum, columns uncorrelated).

    uniforms   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (stratum j, period index t, instance i, 0):
               a = (((w0 << 32) | w1) >> 11) * 2^-53,  u = j / n + a / n  (three fp64 operations in this order)
    shuffle    path p takes stratum sigma(p): 8 Feistel rounds over 2h bits (h >= 1 smallest with 4^h >= n), halves of h bits,
               (l, r) -> (r, l ^ (mix32(r + key_q) & mask)), keys = the words of Philox at counters (0, t, i, 1) and (1, t, i, 1);
               a result >= n goes through again (cycle walking)
    demand     k_lo + #{thresholds <= u}  (continuous distributions and pmf tiles) / k_lo + #{thresholds < u} (integer-valued)
"""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _philox_vec(c0, c1, c2, c3, key):
    """The same on numpy uint64 arrays (c0 an array, the rest scalars)."""
    c0 = c0.astype(np.uint64)
    c1 = np.full_like(c0, c1)
    c2 = np.full_like(c0, c2)
    c3 = np.full_like(c0, c3)
    k0, k1 = key
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _key(seed):
    return seed & M32, (seed >> 32) & M32


def _mix32(x):
    m = np.uint64(M32)
    x = x & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def half_bits(n):
    h = 1
    while 4 ** h < n:
        h += 1
    return h


def sigma(n, seed, inst, t):
    """sigma(p) for p = 0 .. n-1 as an int64 array."""
    key = _key(seed)
    rk = list(philox4x32_10((0, t, inst, 1), key)) + list(philox4x32_10((1, t, inst, 1), key))
    h = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(h)) - 1)
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    while todo.any():
        v = x[todo]
        l, r = v >> h, v & mask
        for q in range(8):
            f = _mix32(r + np.uint64(rk[q])) & mask
            l, r = r, l ^ f
        x[todo] = (l << h) | r
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def strata_and_uniforms(n, seed, inst, t):
    """(j[p], u[p]) of column (inst, t)."""
    j = sigma(n, seed, inst, t)
    w0, w1, _, _ = _philox_vec(j, t, inst, 0, _key(seed))
    bits = ((w0 << np.uint64(32)) | w1) >> np.uint64(11)
    a = bits.astype(np.float64) * 2.0 ** -53
    u = j.astype(np.float64) / float(n) + a / float(n)
    return j, u


def demand_of(u, k_lo, thresholds, strict):
    return (k_lo + np.searchsorted(thresholds, u, side="left" if strict else "right")).astype(np.float64)


def tile_table(tile):
    """(k_lo, thresholds, strict) of a pmf tile [[demand, prob], ...]: the running fp64 sum, the last threshold +infinity."""
    thr = np.cumsum(np.asarray(tile)[:, 1], dtype=np.float64)
    thr[-1] = np.inf
    return int(tile[0][0]), thr, False


def sample(n, seed, inst, tables):
    """(demand[n, T], u[n, T]) of one instance: tables[t] = (k_lo, thresholds, strict)."""
    T = len(tables)
    dem = np.empty((n, T))
    uu = np.empty((n, T))
    for t, (k_lo, thr, strict) in enumerate(tables):
        _, u = strata_and_uniforms(n, seed, inst, t)
        uu[:, t] = u
        dem[:, t] = demand_of(u, k_lo, thr, strict)
    return dem, uu
