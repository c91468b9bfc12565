"""Host twin of the workforce rollout on a sampled tree (sdpgpu_staff_simulate), written from its DEFINITION in DESIGN.md
section 4 ("Workforce rollout on a sampled tree") in numpy -- it shares no code with csrc/sdp_staff_sim.hpp.  Philox, sigma and
the uniforms are tests/sampler_twin.py's (the column (inst = parent i, t) with n = K[t] paths).

    tree      K[t] >= 1 children per node of depth t, N = prod K leaves, stride_t = prod_{s > t} K[s]; leaf p passes node
              n_t = p div stride_t, child digit j = n_t mod K[t], parent i = n_t div K[t] (0 at depth 0)
    uniform   of (t, i, j): sampler_twin.strata_and_uniforms(K[t], seed, inst = i, t)[1][j]
    hires     level rule: s = (int) ss[t][0], S = (int) ss[t][1], optQ = S - x if x < s else 0
              table rule: optQ = policy_t[x - x_lo(t)]; x outside the period's box ends the leaf (valid flag clear)
    turnover  hireTo = x + optQ; 0 if hireTo <= 0, else with r = min(hireTo, n_rows - 1) and c = np.cumsum(row r):
              #{q < row_len[r] - 1 : c_q <= u}
    step      fv = fixHire + variHire, n = hireTo - turnover, imm = fv + salary n + penalty(n), the clamp of n when the problem
              clamps; end_0 = imm_0, end_t = end_{t-1} + imm_t

Everything is computed per NODE of the tree (a node's state is shared by the leaves below it) and spread to the leaves at the
end, so the default tree (10, 10, 10, 10, 1, ...) costs 41 110 node steps."""
import numpy as np

import sampler_twin as tw


class Problem:
    """The numbers the rollout reads: a StaffFunctor's fields, the level pmf table (T, rows, stride) and the rows' lengths."""

    def __init__(self, functor, table, row_len=None):
        self.T = table.shape[0]
        self.K, self.v, self.salary, self.pen = float(functor.fixCost), float(functor.unitVariCost), float(functor.salary), float(functor.unitPenalty)
        self.min_staff = [int(m) for m in functor.minStaffNum]
        self.clamp, self.min_x, self.max_x = bool(functor.clampStaff), int(functor.minX), int(functor.maxX)
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        self.n_rows = self.table.shape[1]
        self.row_len = np.arange(1, self.n_rows + 1) if row_len is None else np.asarray(row_len, dtype=np.int64)
        # thresholds: the running fp64 sum of every row, left to right (np.cumsum adds sequentially)
        self.cum = [np.cumsum(self.table[t], axis=1, dtype=np.float64) for t in range(self.T)]


def strides(K):
    """stride_t = prod_{s > t} K[s]."""
    out, s = [], 1
    for k in reversed(list(K)):
        out.append(s)
        s *= int(k)
    return out[::-1]


def leaf_nodes(K):
    """(node[N, T], child[N, T], parent[N, T]) of every leaf: n_t = p div stride_t, j_t = n_t mod K[t], i_t = n_t div K[t]."""
    K = [int(k) for k in K]
    N = int(np.prod(K, dtype=np.int64))
    p = np.arange(N, dtype=np.int64)
    node = np.stack([p // s for s in strides(K)], axis=1)
    kk = np.asarray(K, dtype=np.int64)[None, :]
    return node, node % kk, node // kk


def node_uniforms(k, seed, t, n_parents):
    """u[i, j] of the children j of every parent i at depth t, one column of sampler_twin per parent."""
    return np.stack([tw.strata_and_uniforms(k, seed, i, t)[1] for i in range(n_parents)], axis=0)


def node_uniforms_vec(k, seed, t, n_parents):
    """The same for all parents at once (the parent index rides in Philox's counter word 2 as an array)."""
    key = tw._key(seed)
    inst = np.arange(n_parents, dtype=np.uint64)
    zero = np.zeros(n_parents, dtype=np.uint64)
    rk = list(tw._philox_vec(zero, t, inst, 1, key)) + list(tw._philox_vec(zero + np.uint64(1), t, inst, 1, key))
    h = np.uint64(tw.half_bits(k))
    mask = np.uint64((1 << int(h)) - 1)
    x = np.broadcast_to(np.arange(k, dtype=np.uint64), (n_parents, k)).copy()
    todo = np.ones(x.shape, dtype=bool)
    keys = [np.broadcast_to(w[:, None], x.shape) for w in rk]
    while todo.any():
        v = x[todo]
        l, r = v >> h, v & mask
        for q in range(8):
            f = tw._mix32(r + keys[q][todo]) & mask
            l, r = r, l ^ f
        x[todo] = (l << h) | r
        todo = x >= np.uint64(k)
    j = x.reshape(-1)
    w0, w1, _, _ = tw._philox_vec(j, t, np.repeat(inst, k), 0, key)
    bits = ((w0 << np.uint64(32)) | w1) >> np.uint64(11)
    a = bits.astype(np.float64) * 2.0 ** -53
    u = j.astype(np.float64) / float(k) + a / float(k)
    return u.reshape(n_parents, k)


def turnover(P, t, hire_to, u):
    """#{q < row_len[r] - 1 : c_q <= u}, r = min(hireTo, n_rows - 1); 0 where hireTo <= 0."""
    out = np.zeros(len(hire_to), dtype=np.int64)
    live = np.nonzero(hire_to > 0)[0]
    q = np.arange(P.table.shape[2])[None, :]
    for at in np.array_split(live, max(1, len(live) * P.table.shape[2] // (1 << 22))):
        r = np.minimum(hire_to[at], P.n_rows - 1)
        counted = q < (P.row_len[r] - 1)[:, None]
        out[at] = ((P.cum[t][r] <= u[at][:, None]) & counted).sum(axis=1)
    return out


def trunc_levels(ss):
    """(int) of Java on a double array."""
    return np.trunc(np.asarray(ss, dtype=np.float64)).astype(np.int64)


def simulate(P, K, seed, ini_x, ss=None, policy=None, x_lo=None, uniforms=node_uniforms_vec):
    """-> dict(sum[N], valid[N], demand[N, T] (-1 in the periods an ended leaf did not reach), mean of the sums by fsum).
    ss: (T, 2) levels, or None with policy[t] (int array) and x_lo[t] for the table rule."""
    K = [int(k) for k in K]
    T = P.T
    assert len(K) == T and min(K) >= 1
    levels = None if ss is None else trunc_levels(ss)
    x = np.array([int(ini_x)], dtype=np.int64)
    end = np.zeros(1)
    valid = np.ones(1, dtype=bool)
    st = strides(K)
    dem_leaf = []
    for t in range(T):
        k = K[t]
        n_par = len(x)
        # the parent's decision
        if levels is not None:
            s, S = int(levels[t][0]), int(levels[t][1])
            opt_q = np.where(x < s, S - x, 0)
            ok = valid.copy()
        else:
            idx = x - int(x_lo[t])
            ok = valid & (idx >= 0) & (idx < len(policy[t]))
            opt_q = np.where(ok, np.asarray(policy[t], dtype=np.int64)[np.clip(idx, 0, len(policy[t]) - 1)], 0)
        hire_to = x + opt_q
        # children in the order i * k + j
        u = uniforms(k, seed, t, n_par).reshape(-1)
        xc, qc, hc, okc, endc = (np.repeat(a, k) for a in (x, opt_q, hire_to, ok, end))
        d = turnover(P, t, np.where(okc, hc, 0), u)
        fix_hire = np.where(qc > 0, P.K, 0.0)
        vari_hire = P.v * qc.astype(np.float64)
        fv = fix_hire + vari_hire
        n = hc - d
        salary_cost = P.salary * n.astype(np.float64)
        penalty = np.where(n > P.min_staff[t], 0.0, P.pen * (P.min_staff[t] - n).astype(np.float64))
        imm = fv + salary_cost + penalty
        new_end = imm if t == 0 else endc + imm
        nn = n
        if P.clamp:
            nn = np.where(nn > P.max_x, P.max_x, nn)
            nn = np.where(nn < P.min_x, P.min_x, nn)
        x = np.where(okc, nn, xc)
        end = np.where(okc, new_end, endc)
        valid = okc
        dem_leaf.append(np.repeat(np.where(okc, d, -1), st[t]))
    return {"sum": end, "valid": valid, "demand": np.stack(dem_leaf, axis=1).astype(np.int32)}


def literal(P, K, seed, ini_x, ss):
    """SimulatesS.simulatesS's nested loops restated statement by statement (level rule only; arrays indexed [t][i * K + j]),
    with the uniform of (t, i, j) in place of generateLHSamples: for the indexing self-check."""
    T = P.T
    nxt, endv, dem = [None] * T, [None] * T, [None] * T
    for t in range(T):
        k = K[t]
        tot = int(np.prod(K[:t + 1]))
        endv[t], nxt[t], dem[t] = [0.0] * tot, [0] * tot, [0] * tot
        last = 1 if t == 0 else len(nxt[t - 1])
        for i in range(last):
            x = ini_x if t == 0 else nxt[t - 1][i]
            opt_q = int(ss[t][1]) - x if x < int(ss[t][0]) else 0
            hire_to = x + opt_q
            if hire_to > 0:
                u = tw.strata_and_uniforms(k, seed, i, t)[1]
                r = min(hire_to, P.n_rows - 1)
                c = np.cumsum(P.table[t][r])
                draws = [int(sum(1 for q in range(int(P.row_len[r]) - 1) if c[q] <= u[j])) for j in range(k)]
            else:
                draws = [0] * k
            for j in range(k):
                n = hire_to - draws[j]
                imm = ((P.K if opt_q > 0 else 0.0) + P.v * opt_q) + P.salary * n
                imm = imm + (0.0 if n > P.min_staff[t] else P.pen * (P.min_staff[t] - n))
                if P.clamp:
                    n = P.max_x if n > P.max_x else n
                    n = P.min_x if n < P.min_x else n
                nxt[t][i * k + j] = n
                dem[t][i * k + j] = draws[j]
                endv[t][i * k + j] = endv[t - 1][i] + imm if t > 0 else imm
    return np.array(endv[T - 1]), dem
