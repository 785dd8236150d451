"""Exact host definition of the device graph generators (csrc/eco_graphgen.hip) and of the fields
eco_graphs_prepare derives from a generated graph (csrc/eco_env.hip).

The generators hash a counter RNG (mix64 / rng3 / u01 of csrc/eco_common.h), so for a seed, a slot and a pair or
draw number every edge, sign and float64 weight is an exact function; this module restates that function in Python
integers and numpy uint64, without torch and without a device.  It restates the kernels, not networkx: parity with
networkx is distributional (tests/test_graph_generators_cpu.py), parity of the kernels with this file is bitwise
(tests/test_graphgen_exact_gpu.py).

generate(kind, n, param, seed, g, weights, cap) returns one Graph: the CSR the kernels write into slot g and the
prepared fields, or an empty flagged graph where the kernels report ECO_ERR_GRAPH."""
from collections import namedtuple

import numpy as np

MASK = (1 << 64) - 1
WEIGHT_SALT = 0x5157A3C1           # edge_sign / edge_weight_random key their hash with seed ^ WEIGHT_SALT
REGULAR_MAX_RESTARTS = 256         # ECO_REGULAR_MAX_RESTARTS (include/eco_hip.h)
REGULAR_MAX_STALLS = 64            # kRegularMaxStalls
_GOLD, _M1, _M2, _BMUL = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93

Graph = namedtuple("Graph", "row_ptr edges weights deg max_deg valid meta overflow restarts stalls")
Graph.__doc__ = """row_ptr int32 [n + 1]; edges uint32 [row_ptr[n]], col | (uint8(w) << 24), rows sorted by column;
weights float64 [row_ptr[n]] or None; deg int32 [n]; max_deg, valid ints; meta float64 [4]; overflow: the kernels
leave the slot empty and set ECO_ERR_GRAPH; restarts, stalls: of the pairing algorithm (0 for the other kinds)."""


# ---- RNG and packing -------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + _GOLD) & MASK
    z = ((z ^ (z >> 30)) * _M1) & MASK
    z = ((z ^ (z >> 27)) * _M2) & MASK
    return z ^ (z >> 31)


def rng3(seed, a, b):
    return mix64(mix64(mix64(seed & MASK) ^ (a & MASK)) ^ ((b * _BMUL) & MASK))


def u01(r):
    """The top 24 bits over 2^24: exact in float32, hence in the float64 returned here."""
    return (r >> 40) / 16777216.0


def mix64_np(z):
    """mix64 of a uint64 array (wrapping arithmetic)."""
    z = z + np.uint64(_GOLD)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
    return z ^ (z >> np.uint64(31))


def rng3_np(seed, a, b):
    """rng3 for scalar seed and a and a uint64 array b."""
    head = np.uint64(mix64(mix64(seed & MASK) ^ (a & MASK)))
    return mix64_np(head ^ (np.asarray(b, dtype=np.uint64) * np.uint64(_BMUL)))


def pair_key(i, j, n):
    return min(i, j) * n + max(i, j)


def draw_below(r, rng):
    """Uniform integer in [0, rng) from a 64-bit draw: the high word of the 128-bit product."""
    return (r * rng) >> 64


# ---- structure: the undirected edge list (a[e], b[e]) of slot g ---------------------------------------------------
def er_pairs(n, p, seed, g):
    """{i, j} present iff i != j and u01(rng3(seed, g, pair_key)) < float32(p), over the upper triangle."""
    iu, ju = np.triu_indices(n, 1)
    r = rng3_np(seed, g, iu.astype(np.uint64) * np.uint64(n) + ju.astype(np.uint64))
    u = (r >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = u < np.float32(p)
    return iu[keep], ju[keep]


def ba_pairs(n, m, seed, g):
    """ba_kernel: the first m vertices are the targets of vertex m; every later vertex draws m distinct targets
    rep[rng3(seed, g, ctr++) % nrep] from the repeated-nodes list, duplicates redrawn, kept in draw order."""
    rep, src_l, tgt_l = [], [], []
    targets = list(range(m))
    ctr = 0
    for src in range(m, n):
        src_l.extend([src] * m)
        tgt_l.extend(targets)
        rep.extend(targets)
        rep.extend([src] * m)
        targets = []
        while len(targets) < m:
            x = rep[rng3(seed, g, ctr) % len(rep)]
            ctr += 1
            if x not in targets:
                targets.append(x)
    return np.array(src_l, dtype=np.int64), np.array(tgt_l, dtype=np.int64)


def regular_pairs(n, d, seed, g, max_restarts=REGULAR_MAX_RESTARTS):
    """regular_kernel.  Returns (a, b, restarts, stalls); a is None when all max_restarts + 1 attempts failed.
    restarts: failed attempts before the one that succeeded; stalls: rounds that added no edge, over all attempts.
    The draw counter runs on across rounds and attempts."""
    S = n * d
    ctr = 0
    stalls_total = 0
    for attempt in range(max_restarts + 1):
        adj = [[] for _ in range(n)]
        stubs = [s % n for s in range(S)]
        stalls = 0
        done = False
        while True:
            ns = len(stubs)
            if ns == 0:
                done = True
                break
            pot = [0] * n
            if ns >= 64:     # the round's ns - 1 draws in one vectorised call
                rs = rng3_np(seed, g, np.arange(ctr, ctr + ns - 1, dtype=np.uint64)).tolist()
            else:
                rs = [rng3(seed, g, ctr + t) for t in range(ns - 1)]
            ctr += ns - 1
            for t, i in enumerate(range(ns - 1, 0, -1)):
                j = draw_below(rs[t], i + 1)
                stubs[i], stubs[j] = stubs[j], stubs[i]
            added = 0
            for q in range(0, ns, 2):
                a, b = stubs[q], stubs[q + 1]
                if a == b or b in adj[a]:
                    pot[a] += 1
                    pot[b] += 1
                else:
                    adj[a].append(b)
                    adj[b].append(a)
                    added += 1
            n_pot = sum(1 for c in pot if c > 0)
            if n_pot == 0:
                done = True
                break
            # u can still be joined iff fewer than n_pot - 1 of its neighbours are potential
            suitable = any(pot[u] > 0 and sum(1 for v in adj[u] if pot[v] > 0) < n_pot - 1 for u in range(n))
            if added == 0:
                stalls += 1
                stalls_total += 1
            if not suitable or stalls > REGULAR_MAX_STALLS:
                break
            stubs = [i for i in range(n) for _ in range(pot[i])]   # rebuilt in vertex order
        if done:
            a = np.array([u for u in range(n) for v in adj[u] if u < v], dtype=np.int64)
            b = np.array([v for u in range(n) for v in adj[u] if u < v], dtype=np.int64)
            return a, b, attempt, stalls_total
    return None, None, max_restarts + 1, stalls_total


def ws_pairs(n, k):
    """Ring lattice: i ~ j iff the circular distance min(|i - j|, n - |i - j|) is in [1, k // 2]."""
    iu, ju = np.triu_indices(n, 1)
    dist = np.minimum(ju - iu, n - (ju - iu))
    keep = dist <= k // 2
    return iu[keep], ju[keep]


# ---- weights ----------------------------------------------------------------------------------------------------
def pair_weights(n, a, b, seed, g, weights):
    """Per undirected edge: (int8 byte of the packed word, float64 weight or None).  Keyed by seed ^ WEIGHT_SALT and
    the unordered pair."""
    if weights == "uniform":
        return np.ones(a.size, dtype=np.int8), None
    key = (np.minimum(a, b) * n + np.maximum(a, b)).astype(np.uint64)
    r = rng3_np(seed ^ WEIGHT_SALT, g, key)
    if weights == "discrete":
        return np.where(r >> np.uint64(63), 1, -1).astype(np.int8), None
    if weights != "random":
        raise ValueError(weights)
    w = 2.0 * ((r >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0   # (r >> 11) < 2^53: exact
    w[w == 0.0] = 2.0 ** -53
    return np.where(w > 0.0, 1, -1).astype(np.int8), w


# ---- prepared fields (graphs_prepare_kernel / graphs_prepare_weighted_kernel) ---------------------------------------
def _butterfly(v):
    """wave_sum_d: v += shfl_xor(v, o) for o = 32 .. 1 on 64 lanes; float addition commutes, so every lane ends
    with the sum of the balanced tree that folds the upper half onto the lower."""
    v = np.asarray(v, dtype=np.float64)
    while v.size > 1:
        h = v.size // 2
        v = v[:h] + v[h:]
    return float(v[0])


def prepared(n, row_ptr, sign, wf):
    """deg (nonzero entries per row), max_deg = max(1, .), valid and meta as the comments over the two prepare
    kernels define them: meta = {max over the NONZERO row sums (1 if there is none), max(1, sum of positive weights
    / 2), min(0, sum of negative weights / 2), sum of all weights}, valid = some row sum is nonzero.
    Integer weights: exact integer sums, any order.  Float weights: float64 sums in the kernel's order (lane t of
    the graph's 64 WPG threads sums rows t, t + 64 WPG, ... entry by entry, a wave folds its lanes by the xor
    butterfly, the waves add up in wave order; WPG = 1 up to 512 vertices, 4 above)."""
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    deg = np.bincount(rows, minlength=n).astype(np.int32)   # every stored weight is nonzero
    max_deg = max(1, int(deg.max()) if n else 1)
    if wf is None:
        w = sign.astype(np.int64)
        rs = np.zeros(n, dtype=np.int64)
        np.add.at(rs, rows, w)
        nz = rs[rs != 0]
        pos, neg, tot = int(w[w > 0].sum()), int(w[w < 0].sum()), int(w.sum())
        best = float(nz.max()) if nz.size else 1.0
        valid = int(nz.size > 0)
        q, lb = pos / 2.0, neg / 2.0
        return deg, max_deg, valid, np.array([best, q if q > 1.0 else 1.0, lb if lb < 0.0 else 0.0, float(tot)])
    ntg = 64 if n <= 512 else 256
    pos, neg, tot = [0.0] * ntg, [0.0] * ntg, [0.0] * ntg
    best = [-np.inf] * ntg
    has = 0
    wl = wf.tolist()
    rp = row_ptr.tolist()
    for t in range(ntg):
        for v in range(t, n, ntg):
            rs = 0.0
            for q in range(rp[v], rp[v + 1]):
                x = wl[q]
                rs += x
                if x > 0.0:
                    pos[t] += x
                else:
                    neg[t] += x
            tot[t] += rs
            if rs != 0.0:
                has = 1
                best[t] = max(best[t], rs)
    fold = lambda lanes: sum((_butterfly(lanes[k:k + 64]) for k in range(64, ntg, 64)), _butterfly(lanes[:64]))
    p, m, s = fold(pos), fold(neg), fold(tot)
    q, lb = p / 2.0, m / 2.0
    return deg, max_deg, has, np.array([max(best) if has else 1.0, q if q > 1.0 else 1.0,
                                        lb if lb < 0.0 else 0.0, s])


# ---- one slot ---------------------------------------------------------------------------------------------------
def empty(n, overflow, restarts=0, stalls=0, float_weights=False):
    """What the kernels leave in a slot whose graph has no entries: a zero row_ptr row; prepare then gives degree 0,
    max_deg 1, valid 0 and meta {1, 1, 0, 0}."""
    return Graph(np.zeros(n + 1, np.int32), np.zeros(0, np.uint32), np.zeros(0) if float_weights else None,
                 np.zeros(n, np.int32), 1, 0, np.array([1.0, 1.0, 0.0, 0.0]), overflow, restarts, stalls)


def assemble(n, a, b, seed, g, weights="discrete", restarts=0, stalls=0):
    """The slot's CSR from the undirected edge list: both directions, rows sorted by column, one weight per pair."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    sign, wf = pair_weights(n, a, b, seed, g, weights)
    r, c = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((c, r))
    r, c, sign = r[order], c[order], np.concatenate([sign, sign])[order]
    if wf is not None:
        wf = np.concatenate([wf, wf])[order]
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    edges = c.astype(np.uint32) | (sign.view(np.uint8).astype(np.uint32) << np.uint32(24))
    deg, max_deg, valid, meta = prepared(n, row_ptr, sign, wf)
    return Graph(row_ptr, edges, wf, deg, max_deg, valid, meta, False, restarts, stalls)


def generate(kind, n, param, seed, g, weights="discrete", cap=None):
    """Slot g of eco_graphs_generate(kind, param, weights, seed) on n vertices with edge slots of `cap` entries
    (None: large enough).  Overflow rule: a graph whose entry count exceeds cap comes back empty and flagged: ER
    total > cap, BA 2 m (n - m) > cap, REG restarts exhausted (the host rejects a cap below n d or below the ring
    lattice's entries before any launch)."""
    fw = weights == "random"
    if kind == "ER":
        a, b = er_pairs(n, param, seed, g)
        if cap is not None and 2 * a.size > cap:
            return empty(n, True, float_weights=fw)
        return assemble(n, a, b, seed, g, weights)
    if kind == "BA":
        m = int(param)
        if cap is not None and 2 * m * (n - m) > cap:
            return empty(n, True, float_weights=fw)
        a, b = ba_pairs(n, m, seed, g)
        return assemble(n, a, b, seed, g, weights)
    if kind == "REG":
        a, b, restarts, stalls = regular_pairs(n, int(param), seed, g)
        if a is None:
            return empty(n, True, restarts, stalls, float_weights=fw)
        return assemble(n, a, b, seed, g, weights, restarts, stalls)
    if kind == "WS":
        a, b = ws_pairs(n, int(param))
        return assemble(n, a, b, seed, g, weights)
    raise ValueError(kind)


def dense(n, graph):
    """[n, n] float64 matrix of a Graph (float weights where it has them, the packed bytes otherwise)."""
    m = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(graph.row_ptr))
    cols = (graph.edges & np.uint32(0xFFFFFF)).astype(np.int64)
    m[rows, cols] = graph.weights if graph.weights is not None else \
        (graph.edges >> np.uint32(24)).astype(np.uint8).view(np.int8)
    return m
