"""MPNN.grad_wg / eco_mpnn_grad_wg (the gradient on global-memory rows, 2048 < N <= 8192, integer weights) against
float64 autograd.

Bar: relative L2 <= 1e-5 per parameter tensor, the project's backward bar (mpnn_corner_common.GRAD_BAR).

Cases, two graphs each:
  n2049    the first size: rows_pad = 2064, the last 16-row tile holds ONE valid row -- vertex 2048, in graph 1 a hub
           of degree 2048; graph 0 has an isolated vertex.  7 observables, one-hot dq (as eco_dqn_td_loss writes it).
           Reference: the dense float64 autograd on the device, as tests/test_large_grad_gpu.py at 2048.
  n2304    integer weights in {-3, -2, 1, 2}, 13 observables (16-float rows), dense dq; dense reference.
  n4100    a partial last 16-row group, the first size of the env's 32-slot kernels; vertex 4099 isolated in both
           graphs.  Reference: the float64 edge-list restatement of wg_grad_common (pinned by test_wg_grad_cpu.py).
  n8192    the cap.  Graph 0: ER of mean degree 6, +-1 weights.  Graph 1: ER of mean degree 3 whose vertex 0 is
           adjacent to every other vertex, +-1 weights with a few of +127 and -128.  One-hot dq on vertex 8191 in
           graph 0 and on the hub in graph 1.  Edge-list reference.
           Bar of this case only: max(GRAD_BAR, 4 E32g), E32g the worst per-tensor relative L2 of the edge-list
           restatement evaluated in float32 against itself in float64 on this input: what ONE float32 evaluation of
           sums of 8191 terms of magnitude up to 128 costs.  The factor 4 covers another summation order and the
           bf16x3 weight split (the construction of tests/test_wg_gpu.py::test_forward_large_sizes), and is not to grow.
           Recorded on one MI355X: E32g 8.0e-6, bar 3.2e-5, the kernel's worst tensor 7.3e-6 (the other cases: 5.1e-7,
           1.0e-6 and 5.9e-7 against 1e-5).

Every case: the gradient is finite, the NaN-filled output is fully overwritten, a second call on the dirty workspace
and a call on a fresh workspace give the same bytes, and the store's error word is clean.  Each float64 reference is
computed once per case.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
import mpnn_corner_common as cc
import wg_grad_common as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


class Inputs:
    """What one grad_wg call takes, and the float64 reference of its result."""

    def __init__(self, n, n_obs, w, x, dq, store, g64, bar=cc.GRAD_BAR):
        self.n, self.n_obs, self.w, self.x, self.dq, self.store, self.g64, self.bar = n, n_obs, w, x, dq, store, g64, bar
        self.B = x.shape[0]


def _dense_inputs(name, mats, n_obs, seed, dq):
    case = cc.Case(name, mats, n_obs, seed, dq=dq)
    _, g64 = cc._autograd(case, torch.float64, "cuda")
    torch.cuda.empty_cache()
    return Inputs(case.N, n_obs, case.w, case.x, case.dq, cc.make_store(case), g64)


def _n2049():
    n = 2049
    mats = [og.er_graph(n, 8.0 / n, np.random.default_rng(20490 + b), "discrete") for b in range(2)]
    mats[0][7, :] = mats[0][:, 7] = 0.0                                    # an isolated vertex
    hub = 2.0 * np.random.default_rng(20499).integers(0, 2, n) - 1.0
    hub[2048] = 0.0
    mats[1][2048, :] = mats[1][:, 2048] = hub                              # the last tile's one valid row
    assert (mats[0][7] == 0).all() and int((mats[1][2048] != 0).sum()) == n - 1
    return _dense_inputs("n2049", mats, 7, 1, "onehot")


def _n2304():
    n = 2304
    mats = []
    for b in range(2):
        rng = np.random.default_rng(23040 + b)
        a = np.triu((rng.random((n, n)) < 8.0 / n) * rng.choice([-3.0, -2.0, 1.0, 2.0], (n, n)), 1)
        mats.append(a + a.T)
    return _dense_inputs("n2304", mats, 13, 2, "dense")


def _sparse_inputs(n, n_obs, seed, graphs, dq_at, bar_from_f32=False):
    g = torch.Generator().manual_seed(seed)
    w = mo.init_weights(g, std=0.1, n_obs_in=n_obs)
    x = wc.node_rows(2, n, n_obs, g)
    mag = torch.randn(2, generator=g)
    mag = torch.where(mag.abs() < 0.1, torch.full_like(mag, 0.7), mag)
    dq = torch.zeros(2, n)
    dq[torch.arange(2), torch.tensor(dq_at)] = mag
    _, g64 = wc.sparse_autograd(w, x, graphs, dq, n_obs)
    bar = cc.GRAD_BAR
    if bar_from_f32:
        _, g32 = wc.sparse_autograd(w, x, graphs, dq, n_obs, dtype=torch.float32)
        e32g = max(wc.worst_rel_l2(g32, g64).values())
        bar = max(cc.GRAD_BAR, 4 * e32g)
        print(f"n{n}: E32g {e32g:.3e}, bar {bar:.3e}")
    return Inputs(n, n_obs, w, x, dq, wc.store_of(n, graphs), g64, bar)


def _n4100():
    n = 4100
    rng = np.random.default_rng(4100)
    i, j = wc.er_edges(n, 6.0, rng)
    g0 = wc.without_vertex(i, j, rng.choice([-1, 1], i.size), n - 1)
    i, j = wc.er_edges(n, 4.0, rng)
    g1 = wc.without_vertex(i, j, rng.choice([-3, -2, 1, 2], i.size), n - 1)
    for gr in (g0, g1):
        assert np.bincount(np.concatenate([gr[0], gr[1]]), minlength=n)[n - 1] == 0
    at0 = int(g0[1][g0[1] < n - 1].max())                                   # the last vertex with an edge
    assert at0 >= 4096                                                      # in the partial last 16-row group
    return _sparse_inputs(n, 7, 3, [g0, g1], [at0, 1234])


def _n8192():
    n = 8192
    rng = np.random.default_rng(8192)
    i, j = wc.er_edges(n, 6.0, rng)
    g0 = (i, j, rng.choice([-1, 1], i.size))
    i, j = wc.er_edges(n, 3.0, rng)
    w1 = rng.choice([-1, 1], i.size)
    w1[rng.choice(i.size, 4, replace=False)] = [127, -128, 127, -128]
    wh = rng.choice([-1, 1], n - 1)
    wh[[5, 77, 1000, n - 2]] = [-128, 127, -128, 127]
    g1 = wc.with_hub(n, i, j, w1, hub=0, wh=wh)
    assert wc.max_degree(n, *g1) == n - 1 and wc.max_degree(n, *g0) < 40
    return _sparse_inputs(n, 7, 4, [g0, g1], [n - 1, 0], bar_from_f32=True)


BUILDERS = {"n2049": _n2049, "n2304": _n2304, "n4100": _n4100, "n8192": _n8192}
_CACHE = {}


def _inputs(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


def _grad_wg(c, workspace=None):
    from eco_hip.networks.mpnn import MPNN
    net = MPNN(n_obs_in=c.n_obs, device="cuda")
    net.load_state_dict(c.w)
    gids = torch.arange(c.B, dtype=torch.int32, device="cuda")
    grad = torch.full_like(net.flat, float("nan"))                       # the call overwrites every entry
    net.grad_wg(c.x.cuda(), c.store, gids, c.dq.cuda(), grad, workspace=workspace)
    torch.cuda.synchronize()
    c.store.check_errors()
    return grad


@pytest.mark.parametrize("name", list(BUILDERS))
def test_grad_wg_matches_float64_autograd(name):
    from eco_hip.networks.mpnn import MPNN
    c = _inputs(name)
    assert not c.store.float_weights and c.store.n_spins == c.n and (c.n_obs > 8) == (name == "n2304")
    ws = torch.empty(MPNN.grad_wg_bytes(c.n, c.B), dtype=torch.uint8, device="cuda")
    grad = _grad_wg(c, ws)
    assert torch.isfinite(grad).all(), name
    gd = cc.flat_to_dict(grad.cpu(), c.n_obs)
    errs = wc.worst_rel_l2(gd, c.g64)
    print(f"{name}: relative L2 vs float64 autograd per tensor (bar {c.bar:.3e}, worst {max(errs.values()):.3e}): " +
          ", ".join(f"{e:.2e}" for e in errs.values()))
    bad = {k: e for k, e in errs.items() if not e <= c.bar}
    assert not bad, (name, bad)
    # a second call on the same (now dirty) workspace and one on a fresh workspace: byte-identical gradients
    again = _grad_wg(c, ws)
    fresh = _grad_wg(c)
    assert torch.equal(grad.view(torch.int32), again.view(torch.int32)), name
    assert torch.equal(grad.view(torch.int32), fresh.view(torch.int32)), name


def test_boundaries_are_rejected_without_a_launch():
    """N = 2048 and N = 8193, a float-weighted set and a NULL dq: ECO_ERR_ARG naming the range, nothing written."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    lib = _lib.lib
    n, B = 2049, 2
    store = GraphStore.from_edges(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1, np.int64))
    net = MPNN(device="cuda")
    net.init_normal_(0.1, generator=torch.Generator().manual_seed(1))
    net.repack()
    x = torch.zeros(B, n, 8, device="cuda")
    dq = torch.zeros(B, n, device="cuda")
    gids = torch.zeros(B, dtype=torch.int32, device="cuda")
    sentinel = 123.0
    grad = torch.full_like(net.flat, sentinel)
    ws = torch.zeros(lib.eco_mpnn_grad_wg_workspace_bytes(n, B), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0

    def call(gs=store.gs, batch=B, dq_=dq, grad_=grad, ws_=ws):
        return lib.eco_mpnn_grad_wg(_lib.ptr(net.packed), 7, ctypes.byref(gs), _lib.ptr(gids), batch, _lib.ptr(x),
                                    _lib.ptr(dq_), _lib.ptr(grad_), _lib.ptr(ws_), _lib.stream_ptr())

    for n_bad in (2048, 8193):
        bad = _lib.GraphSet.from_buffer_copy(store.gs)
        bad.n_spins = n_bad
        assert call(gs=bad) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error(), n_bad
    fw = _lib.GraphSet.from_buffer_copy(store.gs)       # no store holds float weights above 2048: the fields alone
    weights = torch.ones(2 * (n - 1), dtype=torch.float64, device="cuda")
    fw.edge_weights, fw.unit_weights = weights.data_ptr(), 0
    assert call(gs=fw) == _lib.ECO_ERR_ARG
    assert "2048 < N <= 8192" in _lib.last_error() and "integer weights only" in _lib.last_error()
    assert call(dq_=None) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error()
    assert call(batch=0) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error()
    big = (2 ** 31 - 1) // 64 // n + 1
    assert call(batch=big) == _lib.ECO_ERR_ARG and "32-bit row index" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((grad == sentinel).all()) and not bool(ws.any())
    with pytest.raises(ValueError, match="2048 < N <= 8192"):
        small = GraphStore.random("ER", B, 2048, 0.005, seed=4)
        net.grad_wg(torch.zeros(B, 2048, 8, device="cuda"), small, gids, torch.zeros(B, 2048, device="cuda"), grad)
    assert call() == _lib.ECO_OK
    torch.cuda.synchronize()
    store.check_errors()
    assert bool((grad == 0).all())                      # dq = 0: a zero gradient, every entry overwritten
