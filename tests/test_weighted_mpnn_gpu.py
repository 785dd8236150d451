"""MPNN on float-weighted graphs (EdgeType.RANDOM): the CSR-gather kernels read (float)edge_weights[q].

Forward bar: the existing |q - q_ref| <= 5e-7 (1 + |q_ref|) against the fp32 torch oracle; backward: 1e-5 relative
L2 per parameter tensor against float64 autograd of the oracle on the same f32 inputs (the network sees the
adjacency as f32: obs.float(), dqn.py:282).  Each test prints its worst figure before asserting.
"""
import numpy as np
import pytest
import torch

from oracle import mpnn_oracle as mo

pytestmark = pytest.mark.gpu
RTOL = 5e-7


def _graph(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = rng.uniform(-1.0, 1.0, int(keep.sum()))
    return m + m.T


def _setup(n, B, p, seed):
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    g = torch.Generator().manual_seed(seed)
    w = mo.init_weights(g, std=0.1)
    net = MPNN(device="cuda")
    net.load_state_dict(w)
    Js = [_graph(n, p, 100 * seed + b) for b in range(B)]
    store = GraphStore.from_dense(Js)
    assert store.float_weights and not store.unit_weights and store.adjbits is None
    x = torch.zeros(B, n, 8)
    x[:, :, :7] = torch.rand(B, n, 7, generator=g) * 2 - 1
    x[:, :, 0] = torch.where(x[:, :, 0] > 0, 1.0, -1.0)
    obs = torch.from_numpy(np.stack([np.vstack([x[b, :, :7].numpy().T.astype(np.float64), Js[b]])
                                     for b in range(B)])).float()
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    return w, net, store, x.cuda(), obs, gids


def _close(q, ref, what):
    err = (np.abs(np.asarray(q, np.float64) - np.asarray(ref, np.float64)) / (1.0 + np.abs(ref))).max()
    print(f"{what}: max scaled err {err:.3e} (bar {RTOL:.0e})")
    assert err <= RTOL, (what, err)


@pytest.mark.parametrize("n,B,p", [(20, 4, 0.3), (70, 4, 0.15), (200, 4, 0.1), (600, 2, 0.02)])
def test_forward_act_and_pair_match_oracle(n, B, p):
    from eco_hip._lib import ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL, ActConfig
    from eco_hip.networks.mpnn import MPNN
    w, net, store, x, obs, gids = _setup(n, B, p, n)
    q_call = net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_CALL)
    _close(q_call.cpu().numpy(), mo.forward(w, obs).numpy(), f"N={n} per-call")
    q_graph = net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_GRAPH)
    ref = np.stack([mo.forward(w, obs[b]).numpy() for b in range(B)])
    _close(q_graph.cpu().numpy(), ref, f"N={n} per-graph")
    # fused act = argmax of the returned Q
    q = torch.empty(B, n, device="cuda")
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_GRAPH, q_out=q, act=ActConfig(0.0, 1, 0.0, 7, 0),
                       actions_out=acts)
    assert torch.equal(q, q_graph)
    assert torch.equal(acts.long(), q.argmax(1))
    # eco_mpnn_forward_pair == two forwards
    other = MPNN(device="cuda")
    other.load_state_dict(mo.init_weights(torch.Generator().manual_seed(n + 1), std=0.1))
    for scope in (ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL):
        qa, qb = net.forward_pair_graphs(other, x, store, gids, norm_scope=scope)
        assert torch.equal(qa, net.forward_graphs(x, store, gids, norm_scope=scope))
        assert torch.equal(qb, other.forward_graphs(x, store, gids, norm_scope=scope))
    store.check_errors()


@pytest.mark.parametrize("n,B,p", [(20, 8, 0.3), (200, 8, 0.1)])
def test_backward_matches_float64_autograd(n, B, p):
    from eco_hip._lib import ECO_NORM_PER_CALL
    from eco_hip.networks.mpnn import MPNN, param_layout
    w, net, store, x, obs, gids = _setup(n, B, p, n + 7)
    dq = torch.randn(B, n, generator=torch.Generator().manual_seed(n))
    saved = torch.empty(MPNN.saved_bytes(n, B), dtype=torch.uint8, device="cuda")
    q = net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_CALL, saved=saved)
    grad = torch.zeros_like(net.flat)
    net.backward_graphs(x, store, gids, saved, dq.cuda(), grad)
    wg = {k: v.double().requires_grad_(True) for k, v in w.items()}
    qr = mo.forward(wg, obs.double())
    _close(q.cpu().numpy(), qr.detach().numpy(), f"N={n} saving forward")
    (qr * dq.double()).sum().backward()
    flat, off, worst = grad.cpu().double(), 0, 0.0
    for name, shape in param_layout(7):
        k = int(np.prod(shape))
        got, ref = flat[off:off + k].reshape(shape), wg[name].grad
        off += k
        err = float((got - ref).norm() / max(float(ref.norm()), 1e-12))
        print(f"N={n} {name}: relative L2 {err:.3e}")
        worst = max(worst, err)
    assert worst <= 1e-5, worst
    grad2 = torch.zeros_like(net.flat)
    net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_CALL, saved=saved)
    net.backward_graphs(x, store, gids, saved, dq.cuda(), grad2)
    assert torch.equal(grad, grad2)            # fixed-order reductions
    store.check_errors()


def test_no_kernel_path_bit_reroutes_a_weighted_set():
    from eco_hip import _lib
    w, net, store, x, obs, gids = _setup(24, 4, 0.3, 3)
    q0 = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
    for bit in (_lib.ECO_PATH_NO_DENSE, _lib.ECO_PATH_NO_DL, _lib.ECO_PATH_NO_SHARED, _lib.ECO_PATH_NO_PAIR):
        with _lib.kernel_paths(bit):
            q = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL)
            qa, _ = net.forward_pair_graphs(net, x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL)
        assert torch.equal(q, q0) and torch.equal(qa, q0), bit


def test_single_weighted_graph_above_512_does_not_take_the_shared_kernels():
    """One float-weighted graph of N = 600 shared by every episode: the per-episode global-memory kernel runs
    (the shared-graph kernels are +-1 only) and matches the oracle."""
    from eco_hip._lib import ECO_NORM_PER_GRAPH
    from eco_hip.graphs import GraphStore
    n, B = 600, 3
    w, net, _, x, _, _ = _setup(n, B, 0.02, 11)
    J = _graph(n, 0.02, 12)
    store = GraphStore.from_dense([J])
    gids = torch.zeros(B, dtype=torch.int32, device="cuda")
    q = net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_GRAPH).cpu().numpy()
    xc = x.cpu()
    for b in range(B):
        obs = torch.from_numpy(np.vstack([xc[b, :, :7].numpy().T.astype(np.float64), J])).float()
        _close(q[b], mo.forward(w, obs).numpy(), f"shared N=600 episode {b}")


def test_reference_format_forward_takes_a_float_adjacency():
    w, net, store, x, obs, gids = _setup(20, 4, 0.3, 5)
    q = net(obs.clone().cuda()).cpu().numpy()
    _close(q, mo.forward(w, obs).numpy(), "drop-in forward")


def test_reference_fixture_mpnn_case():
    """tests/golden/weighted.npz: the reference MPNN's own Q on a batch of two float-weighted observations."""
    import os
    from conftest import GOLDEN
    from weighted_common import fixture_weights
    from eco_hip._lib import ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    f = np.load(os.path.join(GOLDEN, "weighted.npz"))
    net = MPNN(n_obs_in=7, device="cuda")
    net.load_state_dict(fixture_weights(f))
    obs = f["mpnn/obs"]
    x = np.zeros((2, obs.shape[2], 8), np.float32)
    x[:, :, :7] = obs[:, :7, :].transpose(0, 2, 1).astype(np.float32)
    x = torch.from_numpy(x).cuda()
    store = GraphStore.from_dense([a for a in obs[:, 7:, :]])
    assert store.float_weights
    gids = torch.arange(2, dtype=torch.int32, device="cuda")
    _close(net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_CALL).cpu().numpy(), f["mpnn/q_b2"], "fixture batch")
    _close(net.forward_graphs(x, store, gids, norm_scope=ECO_NORM_PER_GRAPH).cpu().numpy(), f["mpnn/q_b1"], "fixture B=1")
    _close(net(torch.from_numpy(obs).float().cuda()).cpu().numpy(), f["mpnn/q_b2"], "fixture drop-in forward")
