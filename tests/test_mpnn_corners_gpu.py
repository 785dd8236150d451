"""MPNN saving forward + backward against float64 (oracle.mpnn_oracle.forward_staged and its autograd) at the widths,
weights, block shapes and inputs the rest of the suite leaves out.  Helper and bars: tests/mpnn_corner_common.py.

Which hole each case selects (kernel names: csrc/eco_mpnn.hip mpnn_forward_kernel<MT, SV, NW, WLDS, FW> /
mpnn_backward_kernel<MT, NW, WLDS, FW>, derived from pick_cfg / lds_bytes; "CSR" below):

1. Observable counts (every live column of x nonzero, 1e3 in the dead columns of the 8- / 16-float row):
   w8-er20x37      n_obs 8, dense3 kernels, 6 graphs per block, partial last block (37 % gpb != 0 for gpb 5..10)
   w8-er200x5      n_obs 8, mask 0: dense3, one graph per block, prepared adjbits; DENSE2_FWD: dense2 (bitwise mask 0);
                   NO_DENSE: CSR <1,true,16,true,false> / <2,8,true,false>
   w8-ba300x3      n_obs 8, mask 0: DL kernels (eco_mpnn_dl.h); NO_DL: CSR <4,true,8,false,false> / <4,8,false,false>
   w9-*, w16-*     first / full wide row (PK_W0H, PK_WXH, 16-float rows, xwide): CSR <1,true,16,true,false> /
                   <2,8,true,false>, several graphs per block (er40x9) and one (er200x3)
   w1-er20x8       n_obs 1 (the S2V width), dense3
   test_wide_shared_inference: n_obs 8 / 16 at N = 513, shared-graph kernels and (NO_SHARED) mpnn_forward_large_kernel
2. CSR variants at their boundary, one graph per block (rows_pad = N rounded up to 16):
   forward   rows_pad <= 256 <1,SV,16,true,FW>;  rows_pad = 272 <4,SV,8,true,FW>;  288 <= rows_pad <= 512 <4,SV,8,false,FW>
   backward  rows_pad <= 256 <2,8,true,FW>;  272 <= rows_pad <= 512 <4,8,false,FW>
   (82 rows_pad + 19074 floats of LDS with staged weights against 40960: 256 fits, 272 does not; the forward's
   82 rows_pad + 17477 fits at 272, where 17 tiles on 8 waves need MT = 4.)
   csr256-*  N = 256: the last of <1,..,16,true> / <2,8,true>      csr257-*  N = 257 (rows_pad 272): <4,..,8,true> / <4,8,false>
   csr273-fw16  N = 273 (rows_pad 288): the forward's first <4,..,8,false>      csr512-fw13  BA(512, 4): <4,..,8,false> / <4,8,false>
   flavours: fw7 float weights, 7 observables (FW = true); unit13 weight 1 on every edge, 13 observables (FW = false,
   xwide); fw16 / fw13 float weights and wide rows (FW = true, xwide).
   For N <= 512 no other instantiation is reachable with N >= 3: forward <2,..,8,true>, <4,..,4,true>, <4,..,4,false>,
   <8,..,4,false> and backward <4,8,true>, <4,4,true>, <4,4,false>, <8,4,false> are dead (N = 2 at 104 graphs per block
   reaches the backward's <4,8,false> through the per-graph LDS terms; not run here).
3. int40x6, int200x3: integer weights from {-3, -2, 1, 2}: packed-byte weights with |w| > 1, CSR FW = false.
4. Block shapes, +-1 weights, 7 observables: n3x41 (N < 4: CSR, 42 graphs per block), n4x41 (dense, 32 per block, partial
   last block), n17x25 (every graph straddles a 16-row tile), n104x5 (bitmask built in the kernel), n105x3 (prepared
   adjbits); the last two with an isolated vertex and a hub per graph.  With B <= CU count the heuristic takes the
   fewest graphs per block it considers (one at N = 104: two per block needs B > CU count, far above the row limit of
   these cases; test_dense3_matches_dense2_bitwise runs 104 x 33 the same way).
5. train-*: a store of 12 graphs, graph ids [7, 7, 2, 11, 0, 7, 2, 5, 11], one-hot dq with one all-zero row: dense
   several graphs per block (er20), dense one graph per block (er200), CSR wide (er40, 13 observables), CSR FW (er70).

Measured on an MI355X, worst over the 27 cases and their masks [the fp32 torch oracle on the CPU, same metric]:
   Q scaled error 5.8e-8 [4.6e-8] (bar 5e-7);  gradient tensor relative L2 8.0e-7 (bar 1e-5);
   column of the two narrow Linears 6.2e-7 [7.2e-6 -> bar 2.9e-5];  readout element 8.6e-7 [1.4e-6 -> bar 1e-5];
   saved activations: n17x25 1.2e-7 [1.3e-7 -> bar 5.2e-7], w8-ba300x3 9.7e-8 [1.4e-7 -> bar 5.6e-7],
   train-er70-fw 1.3e-7 [1.2e-7 -> bar 5e-7].
   (The fp32 oracle's figures depend on the host's BLAS threading; the bars are derived from them at run time.)
"""
import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
import mpnn_corner_common as cc

pytestmark = pytest.mark.gpu

NO_DENSE, NO_DL, NO_SHARED, DENSE2_FWD = 1, 2, 4, 16      # ECO_PATH_* of include/eco_hip.h (eco_hip._lib)
TRAIN_GIDS = [7, 7, 2, 11, 0, 7, 2, 5, 11]
ZERO_ROW = 5        # graph 7 also sits in rows 0 and 1: dropping the row leaves the call's norm.max() unchanged


def _er(n, p, seed, weights="discrete"):
    J = og.er_graph(n, p, np.random.default_rng(seed), weights)
    if not J.any():
        J[0, 1] = J[1, 0] = 1.0
    return J


def _fw(J, seed):
    """Float weights (EdgeType.RANDOM style) on the edges of J: uniform magnitudes in [0.05, 1), random signs."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(0.05, 1.0, J.shape) * np.where(rng.random(J.shape) < 0.5, -1.0, 1.0), 1)
    return (J != 0) * (U + U.T)


def _intw(n, p, seed):
    """The construction of test_non_unit_weights_use_the_csr_path, with -3 among the weights."""
    rng = np.random.default_rng(seed)
    a = np.triu((rng.random((n, n)) < p) * rng.choice([-3.0, -2.0, 1.0, 2.0], (n, n)), 1)
    if not a.any():
        a[0, 1] = -3.0
    return a + a.T


def _hub_and_isolated(J, seed):
    """Vertex 0 isolated, vertex 1 joined to every other vertex (+-1 weights)."""
    rng = np.random.default_rng(seed)
    J = J.copy()
    n = J.shape[0]
    J[1, 2:] = J[2:, 1] = 2.0 * rng.integers(0, 2, n - 2) - 1.0
    J[0, :] = J[:, 0] = 0.0
    return J


def _n3(b, seed):
    rng = np.random.default_rng(seed)
    J = np.zeros((3, 3))
    for i, j in ((0, 1), (1, 2)) + (((0, 2),) if b % 2 else ()):     # a path, then a triangle, alternating
        J[i, j] = J[j, i] = 2.0 * rng.integers(0, 2) - 1.0
    return J


def _build():
    C = {}

    def add(name, mats, n_obs, masks=(0,), seed=None, **kw):
        C[name] = (cc.Case(name, mats, n_obs, len(C) + 1 if seed is None else seed, **kw), masks)

    # 1. widths
    add("w8-er20x37", [_er(20, 0.3, 100 + b) for b in range(37)], 8)
    add("w8-er200x5", [_er(200, 0.15, 200 + b) for b in range(5)], 8, masks=(0, DENSE2_FWD, NO_DENSE))
    # seed 103: at the table's own seed (3) one H3 pre-activation of the CSR kernels (NO_DL) sits at 8e-8 of the
    # tensor's max and takes the other side of the ReLU than float64 (a rounding tie; gradients then 3e-3 away)
    add("w8-ba300x3", [og.ba_graph(300, 4, np.random.default_rng(300 + b)) for b in range(3)], 8, masks=(0, NO_DL),
        seed=103)
    for k in (9, 16):
        add(f"w{k}-er40x9", [_er(40, 0.2, 400 + k + b) for b in range(9)], k)
        add(f"w{k}-er200x3", [_er(200, 0.15, 500 + k + b) for b in range(3)], k)
    add("w1-er20x8", [_er(20, 0.3, 600 + b) for b in range(8)], 1)
    # 2. CSR variants at their boundary
    for n in (256, 257):
        add(f"csr{n}-fw7", [_fw(_er(n, 0.03, 700 + n + b), b) for b in range(2)], 7)
        add(f"csr{n}-unit13", [_er(n, 0.03, 800 + n + b, "uniform") for b in range(2)], 13)
        add(f"csr{n}-fw16", [_fw(_er(n, 0.03, 900 + n + b), b + 7) for b in range(2)], 16)
    add("csr273-fw16", [_fw(_er(273, 0.03, 1000 + b), b + 3) for b in range(2)], 16)
    add("csr512-fw13", [_fw(og.ba_graph(512, 4, np.random.default_rng(1100 + b)), b + 5) for b in range(2)], 13)
    # 3. integer weights beyond +-1
    add("int40x6", [_intw(40, 0.2, 1200 + b) for b in range(6)], 7)
    add("int200x3", [_intw(200, 0.1, 1300 + b) for b in range(3)], 7)
    # 4. block shapes
    # seed 119: at the table's own seed (19) one M0 pre-activation sits at 2e-8 of the tensor's max (a rounding tie)
    add("n3x41", [_n3(b, 1400 + b) for b in range(41)], 7, seed=119)
    add("n4x41", [_er(4, 0.6, 1500 + b) for b in range(41)], 7)
    add("n17x25", [_er(17, 0.3, 1600 + b) for b in range(25)], 7)
    # seed 122: at the table's own seed (22) the fp32 oracle itself lands on the other side of a ReLU input within
    # rounding of 0 (its edge-embedding gradient column 1.2e-2 from float64), which alone would set the column bar
    add("n104x5", [_hub_and_isolated(_er(104, 0.1, 1700 + b), b) for b in range(5)], 7, seed=122)
    add("n105x3", [_hub_and_isolated(_er(105, 0.1, 1800 + b), b) for b in range(3)], 7)
    # 5. training-shaped inputs
    tr = dict(gids=TRAIN_GIDS, dq="onehot", zero_row=ZERO_ROW)
    add("train-er20", [_er(20, 0.3, 1900 + g) for g in range(12)], 7, **tr)
    add("train-er200", [_er(200, 0.15, 2000 + g) for g in range(12)], 7, **tr)
    add("train-er40-w13", [_er(40, 0.2, 2100 + g) for g in range(12)], 13, **tr)
    add("train-er70-fw", [_fw(_er(70, 0.15, 2200 + g), g + 9) for g in range(12)], 7, **tr)
    return C


CASES = _build()
PARTIAL = {"w8-er20x37", "n3x41", "n4x41", "n17x25"}      # meant to leave a partly filled last block
SAVED_CASES = ["n17x25", "w8-ba300x3", "train-er70-fw"]   # dense, DL, CSR (float weights, repeated graph ids)


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


@pytest.fixture(scope="module")
def fine_bars():
    """4 x the fp32 oracle's worst figure over every case of the module, never below 1e-5 (the factor allows for
    the kernels' other summation order over up to B N rows)."""
    col = el = 0.0
    for case, _ in CASES.values():
        f = cc.reference(case)["fp32"]
        col, el = max(col, f[0]), max(el, f[1])
    print(f"fp32 oracle, worst over {len(CASES)} cases: column {col:.3e}, readout element {el:.3e}")
    return max(4 * col, 1e-5), max(4 * el, 1e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_match_float64(name, fine_bars):
    case, masks = CASES[name]
    store = cc.make_store(case)
    n = case.N
    if all(np.isin(m, (-1.0, 0.0, 1.0)).all() for m in case.mats):
        assert store.unit_weights and (store.adjbits is not None) == (104 < n <= 512), name
    else:
        assert not store.unit_weights and store.adjbits is None, name
        assert store.float_weights == ("fw" in name), name
    if name in PARTIAL:
        assert case.B % cc.graphs_per_block(n, case.B) != 0, (name, cc.graphs_per_block(n, case.B))
    out = {m: cc.check_case(case, m, fine_bars, store) for m in masks}
    if DENSE2_FWD in out:      # ECO_PATH_DENSE2_FWD: bitwise the default dense kernels (include/eco_hip.h)
        for a, b in zip(out[0], out[DENSE2_FWD]):
            assert torch.equal(a, b), name
    for m in masks:
        if m and m != DENSE2_FWD:  # another kernel family really ran
            assert not torch.equal(out[0][1], out[m][1]), (name, m)
    if case.zero_row is not None:
        # the all-zero dq row contributes exactly nothing: the same call without that row (device against device)
        _, g8, _ = cc.run_device(case.without_row(case.zero_row), 0, store)
        d9, d8 = cc.flat_to_dict(out[0][1], case.n_obs), cc.flat_to_dict(g8, case.n_obs)
        for k in mo.KEYS:
            err = float((d9[k] - d8[k]).double().norm() / max(float(d8[k].double().norm()), 1e-300))
            assert err < cc.GRAD_BAR, (name, k, err)


@pytest.mark.parametrize("name", SAVED_CASES)
def test_saved_activations_match_float64(name):
    """H0..H3, E, EAGG, M0..M2, AGG0..AGG2 and MEAN of the saved buffer against the float64 stages; the bar is 4 x
    the fp32 oracle's own worst intermediate error on the case, never below 5e-7."""
    case, _ = CASES[name]
    _, _, saved = cc.run_device(case, 0)
    dev = cc.saved_tensors(saved, case.B, case.N)
    where = "cuda" if case.N > 300 else "cpu"
    _, st64, _ = cc.stages(case, torch.float64, where)
    _, st32, _ = cc.stages(case, torch.float32, "cpu")
    names = cc.NODE_STAGES + ["MEAN"]
    own = max(cc.scaled_err(st32[k], st64[k]) for k in names)
    bar = max(4 * own, 5e-7)
    errs = {k: cc.scaled_err(dev[k], st64[k]) for k in names + ["P"]}
    worst = max(errs[k] for k in names)
    print(f"{name}: saved tensors worst scaled err {worst:.3e} (fp32 oracle {own:.3e}, bar {bar:.3e}); P {errs['P']:.3e}")
    if not worst <= bar:
        print(cc.stage_report(case, saved))
    assert worst <= bar, (name, errs)


@pytest.mark.parametrize("n_obs", [8, 16])
def test_wide_shared_inference(n_obs):
    """Inference only: one ER(513, 0.02) +-1 graph shared by 3 episodes with a full narrow / full wide row, on the
    shared-graph kernels and (ECO_PATH_NO_SHARED) the per-episode global-memory kernel, against the fp32 oracle at
    the bar of test_wide_large_gpu."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from wide_common import oracle_q, scaled_err, wide_net
    n, B = 513, 3
    J = _er(n, 0.02, 513)
    store = GraphStore.from_dense([J])
    assert store.unit_weights
    w, net, wc = wide_net(513 + n_obs, n_obs)
    case = cc.Case("shared", [J], n_obs, 77, gids=[0] * B)       # for its node rows (sentinels in the dead columns)
    xc = case.x.cuda()
    gids = torch.zeros(B, dtype=torch.int32, device="cuda")
    ref = [oracle_q(wc, xc[b], J, n_obs) for b in range(B)]
    qs = {}
    for mask in (0, NO_SHARED):
        with _lib.kernel_paths(mask):
            qs[mask] = net.forward_graphs(xc, store, gids, norm_scope=_lib.ECO_NORM_PER_GRAPH).clone()
        for b in range(B):
            assert scaled_err(qs[mask][b], ref[b], f"n_obs={n_obs} mask {mask} episode {b}") <= 5e-7
    assert not torch.equal(qs[0], qs[NO_SHARED])     # two different kernels ran
    store.check_errors()
