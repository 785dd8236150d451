"""MPNN.grad_large / eco_mpnn_grad_large (gradient on global-memory rows, 512 < N <= 2048) against float64 autograd
of the oracle restatement (oracle.mpnn_oracle, through the Case / float64 judge of mpnn_corner_common).

Bar: relative L2 <= 1e-5 per parameter tensor, the project's backward bar (mpnn_corner_common.GRAD_BAR).

Shapes: N = 513 (first size above the limit; rows_pad = 528, the last 16-row tile holds ONE valid row) with three
distinct ER graphs, one with an isolated vertex and one with a hub of degree N - 1; BA(600, 4) with +-1 weights;
N = 528 (a whole number of tiles) with float weights and 10 observables; N = 530 with 13 observables and integer
weights beyond +-1; N = 2048 (the largest), one sparse graph.  dq is one-hot per episode as eco_dqn_td_loss writes
it; one case takes a dense dq.  Each float64 reference is computed once per case and shared.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
import mpnn_corner_common as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _er(n, p, seed, weights="discrete"):
    return og.er_graph(n, p, np.random.default_rng(seed), weights)


def _fw(J, seed):
    """Float weights on the edges of J: uniform magnitudes in [0.05, 1), random signs."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(0.05, 1.0, J.shape) * np.where(rng.random(J.shape) < 0.5, -1.0, 1.0), 1)
    return (J != 0) * (U + U.T)


def _intw(n, p, seed):
    rng = np.random.default_rng(seed)
    a = np.triu((rng.random((n, n)) < p) * rng.choice([-3.0, -2.0, 1.0, 2.0], (n, n)), 1)
    return a + a.T


def _n513_mats():
    n = 513
    mats = [_er(n, 0.02, 5130 + b) for b in range(3)]
    mats[0][7, :] = mats[0][:, 7] = 0.0                                    # an isolated vertex
    rng = np.random.default_rng(5139)
    hub = 2.0 * rng.integers(0, 2, n) - 1.0
    hub[512] = 0.0
    mats[1][512, :] = mats[1][:, 512] = hub                                # the last tile's one valid row: degree N - 1
    assert (mats[0][7] == 0).all() and int((mats[1][512] != 0).sum()) == n - 1
    return mats


def _build():
    m513 = _n513_mats()
    return {
        "n513-er-x3": dict(mats=m513, n_obs=7, seed=1, dq="onehot"),
        "n513-er-x3-dense-dq": dict(mats=m513, n_obs=7, seed=2, dq="dense"),
        "n600-ba4-pm1-x2": dict(mats=[og.ba_graph(600, 4, np.random.default_rng(6000 + b)) for b in range(2)], n_obs=7,
                                seed=3, dq="onehot"),
        "n528-fw-obs10-x2": dict(mats=[_fw(_er(528, 0.02, 5280 + b), b + 1) for b in range(2)], n_obs=10, seed=4,
                                 dq="onehot"),
        "n530-int-obs13-x2": dict(mats=[_intw(530, 0.02, 5300 + b) for b in range(2)], n_obs=13, seed=5, dq="onehot"),
        "n2048-sparse-x1": dict(mats=[_er(2048, 0.005, 20480)], n_obs=7, seed=6, dq="onehot"),
    }


SPECS = _build()
_CACHE = {}


def _case(name):
    """The case, its float64 gradients (computed once, kept unchanged) and its device store."""
    if name not in _CACHE:
        s = SPECS[name]
        case = cc.Case(name, s["mats"], s["n_obs"], s["seed"], dq=s["dq"])
        _, g64 = cc._autograd(case, torch.float64, "cuda")
        _CACHE[name] = (case, g64, cc.make_store(case))
    return _CACHE[name]


def _grad_large(case, store, workspace=None):
    from eco_hip.networks.mpnn import MPNN
    net = MPNN(n_obs_in=case.n_obs, device="cuda")
    net.load_state_dict(case.w)
    gids = torch.tensor(case.gids, dtype=torch.int32, device="cuda")
    grad = torch.full_like(net.flat, float("nan"))                       # the call overwrites every entry
    net.grad_large(case.x.cuda(), store, gids, case.dq.cuda(), grad, workspace=workspace)
    torch.cuda.synchronize()
    store.check_errors()
    return grad


@pytest.mark.parametrize("name", list(SPECS))
def test_grad_large_matches_float64_autograd(name):
    from eco_hip import _lib
    case, g64, store = _case(name)
    assert store.float_weights == ("fw" in name) and (case.n_obs > 8) == ("obs1" in name)
    ws = torch.empty(_lib.lib.eco_mpnn_grad_large_workspace_bytes(case.N, case.B), dtype=torch.uint8, device="cuda")
    grad = _grad_large(case, store, ws)
    assert torch.isfinite(grad).all(), name
    gd = cc.flat_to_dict(grad.cpu(), case.n_obs)
    errs = {}
    for k in mo.KEYS:
        r = g64[k]
        errs[k] = float((gd[k].double() - r).norm() / max(float(r.norm()), 1e-300))
    print(f"{name}: relative L2 vs float64 autograd per tensor: " + ", ".join(f"{e:.2e}" for e in errs.values()))
    bad = {k: e for k, e in errs.items() if not e <= cc.GRAD_BAR}
    assert not bad, (name, bad)
    # a second call on the same (now dirty) workspace and one on a fresh workspace: byte-identical gradients
    again = _grad_large(case, store, ws)
    fresh = _grad_large(case, store)
    assert torch.equal(grad.view(torch.int32), again.view(torch.int32)), name
    assert torch.equal(grad.view(torch.int32), fresh.view(torch.int32)), name


@pytest.mark.parametrize("shared", [False, True])
def test_forward_unaffected_by_interleaved_grad_large(shared):
    """Q of forward_graphs before and after a grad_large call on the same network (which owns the forward
    workspace and, on one shared +-1 graph, the shared-graph tables cached in it) is bitwise the same, and equals a
    fresh network's."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    n, B = 600, 4
    J = _er(n, 0.02, 777)
    store = GraphStore.from_dense([J] if shared else [J] * B)
    gids = (torch.zeros(B, dtype=torch.int32, device="cuda") if shared
            else torch.arange(B, dtype=torch.int32, device="cuda"))
    route = _lib.lib.eco_mpnn_route(ctypes.byref(store.gs), 7, B, 0, 0, 0)
    assert route == (_lib.ECO_ROUTE_SHARED if shared else _lib.ECO_ROUTE_LARGE)
    case = cc.Case("interleave", [J], 7, 9, gids=[0] * B, dq="onehot")
    x, dq = case.x.cuda(), case.dq.cuda()
    net = MPNN(device="cuda")
    net.load_state_dict(case.w)
    q0 = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
    grad = torch.zeros_like(net.flat)
    net.grad_large(x, store, gids, dq, grad)
    q1 = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
    other = MPNN(device="cuda")
    other.load_state_dict(case.w)
    q2 = other.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL)
    torch.cuda.synchronize()
    assert torch.equal(q0, q1) and torch.equal(q0, q2)
    # the gradient does not depend on how the episodes name their graph: one shared graph or B copies of it
    if shared:
        rep = GraphStore.from_dense([J] * B)
        grad_rep = torch.zeros_like(net.flat)
        net.grad_large(x, rep, torch.arange(B, dtype=torch.int32, device="cuda"), dq, grad_rep)
        torch.cuda.synchronize()
        assert torch.equal(grad, grad_rep)


def test_argument_errors_and_bytes_query():
    """Every rejection happens before a launch: ECO_ERR_ARG, nothing written."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    lib = _lib.lib
    for n in (1, 200, 512):
        assert lib.eco_mpnn_grad_large_workspace_bytes(n, 4) == 0
    assert lib.eco_mpnn_grad_large_workspace_bytes(2049, 4) == 0
    assert lib.eco_mpnn_grad_large_workspace_bytes(513, 0) == 0
    n, B = 513, 2
    store = GraphStore.random("ER", B, n, 0.02, seed=3)
    net = MPNN(device="cuda")
    net.init_normal_(0.1, generator=torch.Generator().manual_seed(1))
    net.repack()
    x = torch.zeros(B, n, 8, device="cuda")
    dq = torch.zeros(B, n, device="cuda")
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    sentinel = 123.0
    grad = torch.full_like(net.flat, sentinel)
    ws = torch.zeros(lib.eco_mpnn_grad_large_workspace_bytes(n, B), dtype=torch.uint8, device="cuda")

    def call(gs=store.gs, batch=B, dq_=dq, grad_=grad, ws_=ws):
        return lib.eco_mpnn_grad_large(_lib.ptr(net.packed), 7, ctypes.byref(gs), _lib.ptr(gids), batch, _lib.ptr(x),
                                       _lib.ptr(dq_), _lib.ptr(grad_), _lib.ptr(ws_), _lib.stream_ptr())

    assert call(dq_=None) == _lib.ECO_ERR_ARG
    assert call(grad_=None) == _lib.ECO_ERR_ARG
    assert call(ws_=None) == _lib.ECO_ERR_ARG
    assert call(batch=0) == _lib.ECO_ERR_ARG
    small = GraphStore.random("ER", B, 512, 0.02, seed=4)
    assert call(gs=small.gs) == _lib.ECO_ERR_ARG
    assert "512 < N <= 2048" in _lib.last_error()
    big = _lib.GraphSet.from_buffer_copy(store.gs)      # no store holds more than 2048 vertices: the scalar field alone
    big.n_spins = 2049
    assert call(gs=big) == _lib.ECO_ERR_ARG
    torch.cuda.synchronize()
    assert bool((grad == sentinel).all()) and not bool(ws.any())
    with pytest.raises(ValueError, match="512 < N"):
        net.grad_large(torch.zeros(B, 512, 8, device="cuda"), small, gids, torch.zeros(B, 512, device="cuda"), grad)
    assert call() == _lib.ECO_OK
    torch.cuda.synchronize()
    assert bool((grad == 0).all())                      # dq = 0: a zero gradient, every entry overwritten


def test_saved_training_forward_above_512_keeps_its_message():
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    n, B = 513, 2
    store = GraphStore.random("ER", B, n, 0.02, seed=5)
    net = MPNN(device="cuda")
    x = torch.zeros(B, n, 8, device="cuda")
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    saved = torch.empty(MPNN.saved_bytes(n, B), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"training forward \(saved activations\) supports N <= 512"):
        net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL, saved=saved)
    ws = torch.empty(_lib.lib.eco_mpnn_backward_workspace_bytes(n, B), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="MPNN backward supports N <= 512"):
        net.backward_graphs(x, store, gids, saved, torch.zeros(B, n, device="cuda"), torch.zeros_like(net.flat),
                            workspace=ws)
