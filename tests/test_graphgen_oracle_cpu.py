"""oracle/graphgen_oracle.py pinned on the host, before tests/test_graphgen_exact_gpu.py holds the kernels to it:
its RNG against the suite's other restatements and against literals printed by a host program built on
csrc/eco_common.h (recipe: DESIGN.md section 27), the structure of every graph the GPU cases use, its distributions
against the numpy-stream generators of eco_hip.graphs, and the coverage the REG cases are chosen for."""
import os
import re

import numpy as np
import pytest

import graphgen_cases as gc
import prio_common
from oracle import graphgen_oracle as go

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1

# (seed, a, b, rng3(seed, a, b), u01(rng3), mix64(seed)) printed by the host program of DESIGN.md section 27
RNG_LITERALS = [
    (0x0, 0x0, 0x0, 0x238275BC38FCBE91, 0.13870936632156372, 0xE220A8397B1DCDAF),
    (0x1, 0x2, 0x3, 0x1591EEDBD504C4AD, 0.084257960319519043, 0x910A2DEC89025CC1),
    (0x7, 0x0, 0x1, 0x42E6070CFDA13724, 0.26132243871688843, 0x63CBE1E459320DD7),
    (0x7, 0x1, 0x0, 0x7010C70C013E27EC, 0.4377560019493103, 0x63CBE1E459320DD7),
    (0xB, 0x5, 0x103F, 0xD1641071DA84E474, 0.81793308258056641, 0x50F5647D2380309D),
    (0x5157A3C1, 0x3, 0x40, 0xA69275D42398B08B, 0.65067225694656372, 0x9E4B609CA5C52EB3),
    (0x5157A3C6, 0xF, 0x1080, 0xA633D9B6BADF379A, 0.64922863245010376, 0x23A6C91D7E8F81B6),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xBDE48779173DBC2B, 0.74176830053329468,
     0xE4D971771B652C20),
    (0x21, 0x1FFF, 0x3FFFFFF, 0x14359AD46D5580C5, 0.07894289493560791, 0x2C0E0FEDBE2218A8),
    (0x8000000000000000, 0x100000000, 0x80000000, 0xDD15D89706D2FA49, 0.86361455917358398, 0x481EC0A212A9F3DB),
    (0x7E8, 0xC, 0xFFFFFFFF, 0xDFADFD3E726B8F4F, 0.87374860048294067, 0x9F6D8FECF88EECD5),
    (0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93, 0xBF58476D1CE4E5B9, 0xD26FB35DDED73331, 0.82201689481735229,
     0x6E789E6AA1B965F4),
]


def _act_skip_mix64(z):
    """tests/test_act_skip_gpu.py's _mix64 / _rng3, restated (that module needs a device to import)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _act_skip_rng3(seed, a, b):
    return _act_skip_mix64(_act_skip_mix64(_act_skip_mix64(seed) ^ a) ^ ((b * 0xD6E8FEB86659FD93) & M64))


# ---- RNG --------------------------------------------------------------------------------------------------------
def test_rng3_agrees_with_the_other_restatements():
    rng = np.random.default_rng(0)
    triples = [tuple(int(x) for x in rng.integers(0, 1 << 64, 3, dtype=np.uint64)) for _ in range(200)]
    triples += [tuple(int(x) for x in rng.integers(0, 1 << 20, 3)) for _ in range(200)]
    for s, a, b in triples:
        r = go.rng3(s, a, b)
        assert r == prio_common.rng3(s, a, b) == _act_skip_rng3(s, a, b)
        assert go.mix64(s) == prio_common.mix64(s)
    # the vectorised form, per scalar seed and a
    for s, a, _ in triples[::40]:
        bs = np.array([t[2] for t in triples], dtype=np.uint64)
        assert go.rng3_np(s, a, bs).tolist() == [go.rng3(s, a, int(b)) for b in bs]
        assert go.mix64_np(bs).tolist() == [go.mix64(int(b)) for b in bs]


def test_rng3_u01_mix64_literals_of_the_device_header():
    for s, a, b, r, u, m in RNG_LITERALS:
        assert go.rng3(s, a, b) == r and go.mix64(s) == m
        assert go.u01(r) == u and np.float32(go.u01(r)) == np.float32(u)
        assert int(go.rng3_np(s, a, np.array([b], dtype=np.uint64))[0]) == r


def test_packing_helpers():
    assert go.pair_key(3, 5, 20) == go.pair_key(5, 3, 20) == 65
    assert go.draw_below(M64, 7) == 6 and go.draw_below(0, 7) == 0 and go.draw_below(1 << 63, 7) == 3
    assert [go.draw_below(r, 1) for r in (0, 12345, M64)] == [0, 0, 0]


def test_constants_match_the_headers():
    hdr = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    assert int(re.search(r"ECO_REGULAR_MAX_RESTARTS\s*=\s*(\d+)", hdr).group(1)) == go.REGULAR_MAX_RESTARTS
    src = open(os.path.join(REPO, "eco-dqn_amd", "csrc", "eco_graphgen.hip")).read()
    assert int(re.search(r"kRegularMaxStalls\s*=\s*(\d+)", src).group(1)) == go.REGULAR_MAX_STALLS
    assert f"0x{go.WEIGHT_SALT:X}ull" in src


def test_er_vectorised_equals_the_scalar_definition():
    """er_edge for every ordered pair, in Python integers and one float32 comparison each, against the vectorised
    upper triangle; the weights of both kinds from the scalar hash of the unordered pair."""
    n, p, seed, g = 21, 0.3, 5, 9
    p32 = np.float32(p)
    A = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for j in range(n):
            A[i, j] = i != j and np.float32(go.u01(go.rng3(seed, g, go.pair_key(i, j, n)))) < p32
    a, b = go.er_pairs(n, p, seed, g)
    B = np.zeros((n, n), dtype=bool)
    B[a, b] = B[b, a] = True
    assert np.array_equal(A, B) and A.any()
    sign, _ = go.pair_weights(n, a, b, seed, g, "discrete")
    _, wf = go.pair_weights(n, a, b, seed, g, "random")
    for e in range(a.size):
        r = go.rng3(seed ^ 0x5157A3C1, g, go.pair_key(int(b[e]), int(a[e]), n))
        assert sign[e] == (1 if r >> 63 else -1)
        w = 2.0 * ((r >> 11) * 2.0 ** -53) - 1.0
        assert wf[e] == (w if w != 0.0 else 2.0 ** -53)


# ---- structure of every oracle graph the GPU test uses --------------------------------------------------------------
def _ring(n, k):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    dist = np.minimum(np.abs(i - j), n - np.abs(i - j))
    return ((dist >= 1) & (dist <= k // 2)).astype(float)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_structure_of_the_oracle_graphs(name):
    c = gc.CASES[name]
    graphs = gc.oracle_graphs(name)
    assert sorted(graphs) == list(range(c.first, c.first + c.count))
    for g, gr in graphs.items():
        n = c.n
        assert not gr.overflow
        rp = gr.row_ptr.astype(np.int64)
        assert rp[0] == 0 and np.all(np.diff(rp) >= 0) and gr.edges.size == rp[-1]
        rows = np.repeat(np.arange(n), np.diff(rp))
        cols = (gr.edges & 0xFFFFFF).astype(np.int64)
        byte = (gr.edges >> 24).astype(np.uint8).view(np.int8)
        assert np.all(rows != cols) and (cols.size == 0 or (cols.min() >= 0 and cols.max() < n))
        assert np.all(np.diff(cols)[np.diff(rows) == 0] > 0)              # rows sorted, no duplicate
        t = np.lexsort((rows, cols))                                      # the transpose, in CSR order
        assert np.array_equal(cols[t], rows) and np.array_equal(rows[t], cols) and np.array_equal(byte[t], byte)
        assert np.array_equal(gr.deg, np.diff(rp)) and gr.max_deg == max(1, int(np.diff(rp).max()))
        if c.weights == "uniform":
            assert np.all(byte == 1) and gr.weights is None
        elif c.weights == "discrete":
            assert set(np.unique(byte)) <= {-1, 1} and gr.weights is None
        else:
            w = gr.weights
            assert np.all(w != 0) and np.all(np.abs(w) < 1) and np.array_equal(w[t], w)
            assert np.array_equal(byte, np.sign(w).astype(np.int8))
            J = go.dense(n, gr)                                           # meta against plain numpy, to rounding
            assert abs(gr.meta[3] - J.sum()) <= 1e-12 and abs(gr.meta[1] - max(1, J[J > 0].sum() / 2)) <= 1e-12
            assert abs(gr.meta[2] - min(0, J[J < 0].sum() / 2)) <= 1e-12
            rs = J.sum(1)
            assert abs(gr.meta[0] - rs[rs != 0].max()) <= 1e-12 and gr.valid == 1
        if c.weights != "random" and n <= 600:
            J = go.dense(n, gr)
            rs = J.sum(1)
            nz = rs[rs != 0]
            ref = [nz.max() if nz.size else 1.0, max(1.0, J[J > 0].sum() / 2), min(0.0, J[J < 0].sum() / 2), J.sum()]
            assert gr.meta.tolist() == ref and gr.valid == int(nz.size > 0)
        if c.kind == "BA":
            assert rp[-1] == 2 * c.param * (n - c.param)
        elif c.kind == "REG":
            assert np.all(np.diff(rp) == c.param)
        elif c.kind == "WS":
            if n <= 600:
                assert np.array_equal(np.abs(go.dense(n, gr)) != 0, _ring(n, c.param) != 0)
            else:                                                         # the same definition, row by row
                d = np.abs(rows - cols)
                assert np.all(np.minimum(d, n - d) <= c.param // 2) and np.all(np.diff(rp) == 2 * (c.param // 2))
        elif name == "er65_p0":
            assert rp[-1] == 0 and gr.valid == 0 and gr.meta.tolist() == [1.0, 1.0, 0.0, 0.0]
        elif name == "er65_p1":
            assert rp[-1] == n * (n - 1)
    if c.count > 1 and c.kind != "WS" and name not in ("er65_p0", "er65_p1", "reg8_7"):   # those have one structure
        first = graphs[c.first]
        assert all(not np.array_equal(first.edges & 0xFFFFFF, graphs[g].edges & 0xFFFFFF)
                   for g in range(c.first + 1, c.first + c.count))        # slots differ


@pytest.mark.parametrize("group", gc.WEIGHT_KIND_GROUPS)
def test_structure_does_not_depend_on_the_weight_kind(group):
    base = gc.oracle_graphs(group[0])
    for other in group[1:]:
        for g, gr in gc.oracle_graphs(other).items():
            assert np.array_equal(gr.row_ptr, base[g].row_ptr)
            assert np.array_equal(gr.edges & 0xFFFFFF, base[g].edges & 0xFFFFFF)


def test_er_case_with_p_equal_to_a_draw():
    """er20_p_on_draw: pair {14, 17} of slot 0 draws exactly p, so the strict comparison leaves it out and a
    non-strict one would put it in; the other pairs around it are decided either way."""
    c = gc.CASES["er20_p_on_draw"]
    assert c.param == float(np.float32(c.param)) and 0.2 < c.param < 0.21
    assert go.u01(go.rng3(c.seed, 0, go.pair_key(17, 14, c.n))) == c.param
    J = go.dense(c.n, gc.oracle_graphs("er20_p_on_draw")[0])
    assert J[14, 17] == 0 and J[17, 14] == 0 and np.count_nonzero(J) > 40


def test_overflow_rule():
    er = go.generate("ER", 30, 0.4, 3, 2)
    total = int(er.row_ptr[-1])
    full = go.generate("ER", 30, 0.4, 3, 2, cap=total)
    assert not full.overflow and np.array_equal(full.edges, er.edges)
    over = go.generate("ER", 30, 0.4, 3, 2, cap=total - 1)
    assert over.overflow and not over.row_ptr.any() and over.edges.size == 0 and over.valid == 0
    assert over.max_deg == 1 and not over.deg.any() and over.meta.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert not go.generate("BA", 20, 4, 3, 0, cap=128).overflow
    ba = go.generate("BA", 20, 4, 3, 0, cap=127)
    assert ba.overflow and not ba.row_ptr.any() and ba.valid == 0


# ---- distributions: the restatement is not a private fiction ---------------------------------------------------------
def test_er_edge_count_is_binomial():
    n, p, G = 40, 0.15, 64
    pairs = n * (n - 1) // 2
    edges = sum(go.er_pairs(n, p, 19, g)[0].size for g in range(G))
    se = np.sqrt(G * pairs * p * (1 - p))
    print(f"ER edges {edges}, expected {G * pairs * p:.1f}, binomial sd {se:.1f}")
    assert abs(edges - G * pairs * p) < 5 * se


def _two_triangle_fraction(S):
    """S [G, 6, 6] bool, 2-regular: two triangles iff the two neighbours of vertex 0 are adjacent."""
    nb = np.argsort(~S[:, 0, :], axis=1, kind="stable")[:, :2]
    return S[np.arange(S.shape[0]), nb[:, 0], nb[:, 1]].mean()


def test_regular_two_triangle_fraction_matches_the_numpy_stream():
    from eco_hip.graphs import random_csr
    n, d, G = 6, 2, 2048
    O = np.zeros((G, n, n), dtype=bool)
    for g in range(G):
        a, b, _, _ = go.regular_pairs(n, d, 33, g)
        O[g, a, b] = O[g, b, a] = True
    assert np.all(O.sum(2) == d)
    csr = random_csr("REG", G, n, d, seed=34, weights="uniform")
    cols = (csr[2] & 0xFFFFFF).astype(np.int64).reshape(G, n, d)
    H = np.zeros((G, n, n), dtype=bool)
    H[np.arange(G)[:, None, None], np.arange(n)[None, :, None], cols] = True
    ora, host = _two_triangle_fraction(O), _two_triangle_fraction(H)
    pooled = (ora + host) / 2
    se = np.sqrt(pooled * (1 - pooled) * 2 / G)
    print(f"two-triangle fraction: oracle {ora:.4f}, numpy stream {host:.4f}, se of the difference {se:.4f}")
    assert 0 < host < 1 and abs(ora - host) < 5 * se


def test_ba_degree_sequence_matches_the_numpy_stream():
    """Same mean degree (it is 2 m (n - m) / n whatever the draws) and a maximum degree like the numpy stream's: the
    mean of the per-graph maximum over 64 graphs within 5 standard errors of the difference of two such means, and
    the oracle's median maximum inside the range of the numpy stream's 64 maxima."""
    from eco_hip.graphs import _ba_edges
    n, m, G = 40, 4, 64
    rng = np.random.default_rng(3)
    omax, hmax = [], []
    for g in range(G):
        a, b = go.ba_pairs(n, m, 23, g)
        od = np.bincount(np.concatenate([a, b]), minlength=n)
        iu, ju = _ba_edges(n, m, rng)
        hd = np.bincount(np.concatenate([iu, ju]), minlength=n)
        assert od.sum() == hd.sum() == 2 * m * (n - m) and od.min() >= 1 and od[m:].min() >= m
        assert np.unique(a * n + b).size == a.size and np.all(b < a)      # m distinct earlier targets each
        omax.append(od.max())
        hmax.append(hd.max())
    omax, hmax = np.array(omax), np.array(hmax)
    se = np.sqrt((omax.var(ddof=1) + hmax.var(ddof=1)) / G)
    print(f"BA max degree: oracle mean {omax.mean():.2f}, numpy stream {hmax.mean():.2f} "
          f"[{hmax.min()}, {hmax.max()}], se of the difference {se:.2f}")
    assert abs(omax.mean() - hmax.mean()) < 5 * se
    assert hmax.min() <= np.median(omax) <= hmax.max()


# ---- coverage the REG cases are chosen for ----------------------------------------------------------------------------
def test_regular_cases_cover_restarts_and_stalls():
    restarts = {k: [g.restarts for g in gc.oracle_graphs(k).values()] for k in gc.REG_CASES}
    stalls = {k: [g.stalls for g in gc.oracle_graphs(k).values()] for k in gc.REG_CASES}
    print("restarts", restarts)
    print("stalls", stalls)
    for k in ("reg20_3", "reg9_4", "reg65_6"):
        assert max(restarts[k]) > 0, k
    for k in ("reg20_3", "reg9_4", "reg8_7", "reg12_4_random"):
        assert max(stalls[k]) > 0, k
    assert max(restarts["reg9_4"]) >= 3                  # the draw counter runs on over several attempts
    # d = n - 1: a vertex with a stub left misses an edge to a vertex that has one left too, so an attempt is always
    # suitable and can only fail through kRegularMaxStalls: reg8_7 covers stalls, not restarts
    assert max(restarts["reg8_7"]) == 0 and max(stalls["reg8_7"]) >= 5


def test_no_small_complete_graph_exhausts_the_restarts():
    """(n, n - 1) for n <= 8: no slot of 256 seeds comes near ECO_REGULAR_MAX_RESTARTS + 1 failed attempts (the
    search over 3000 seeds each is in DESIGN.md section 27: none restarts at all, at most 25 stalls).  The exhausted
    branch of regular_kernel is therefore not pinned by a GPU case."""
    for n in range(2, 9):
        if n * (n - 1) % 2:
            continue
        out = [go.regular_pairs(n, n - 1, seed, 0) for seed in range(256)]
        assert all(o[0] is not None and o[0].size == n * (n - 1) // 2 for o in out)
        assert max(o[2] for o in out) == 0 and max(o[3] for o in out) <= go.REGULAR_MAX_STALLS


def test_exhausted_restarts_give_an_empty_flagged_graph():
    """The oracle's own exhausted branch, reached with a lowered limit on the host only: (6, 4) restarts often."""
    hit = [s for s in range(64) if go.regular_pairs(6, 4, s, 0, max_restarts=0)[0] is None]
    assert hit
    a, b, restarts, _ = go.regular_pairs(6, 4, hit[0], 0, max_restarts=0)
    assert a is None and restarts == 1
    assert go.regular_pairs(6, 4, hit[0], 0)[0] is not None
