"""More than 8 observables (16-float node rows) above 512 vertices on the per-episode global-memory kernel
(mpnn_forward_large_kernel's 16-float-row instances, csrc/eco_mpnn.hip): several distinct graphs per call, so no
call takes the shared-graph kernels.

Bar: |q - ref| <= 5e-7 (1 + |ref|) against the fp32 torch oracle (oracle.mpnn_oracle.forward, on the GPU), the bar of
tests/test_large_gpu.py and tests/test_weighted_mpnn_gpu.py for the same kernel's 8-float-row instances."""
import numpy as np
import pytest
import torch

from oracle import graphs as og
from wide_common import N_OBS, oracle_q, scaled_err, wide_net, wide_x

pytestmark = pytest.mark.gpu

BAR = 5e-7


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


@pytest.mark.parametrize("n,p", [(513, 0.02), (600, 0.02)])  # 513: one real row in the last 16-row tile
def test_wide_large_forward_matches_oracle(n, p):
    from eco_hip.graphs import GraphStore
    from eco_hip._lib import ActConfig, ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL
    B = 3
    rng = np.random.default_rng(n)
    mats = [og.er_graph(n, p, rng, weights="uniform" if b % 2 else "discrete") for b in range(B)]
    store = GraphStore.from_dense(mats)
    w, net, wc = wide_net(n)
    x = wide_x(n, B, n)
    xc = x.cuda()
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    q = net.forward_graphs(xc, store, gids, norm_scope=ECO_NORM_PER_GRAPH)
    for b in range(B):
        assert scaled_err(q[b], oracle_q(wc, xc[b], mats[b]), f"N={n} graph {b}") <= BAR
    # per-call norm scope + fused greedy act = argmax of the returned Q
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    qc = torch.empty(B, n, device="cuda")
    net.forward_graphs(xc, store, gids, norm_scope=ECO_NORM_PER_CALL, q_out=qc, act=ActConfig(0.0, 1, 0.0, 1, 0),
                       actions_out=acts)
    assert torch.equal(acts.long(), qc.argmax(1))
    # irreversible act: only vertices whose feature 0 (read with the 16-float stride) equals -1, greedy and random
    for eps in (0.0, 1.0):
        net.forward_graphs(xc, store, gids, norm_scope=ECO_NORM_PER_CALL, act=ActConfig(eps, 0, -1.0, 3, 1),
                           actions_out=acts)
        a = acts.long().cpu()
        assert bool((x[torch.arange(B), a, 0] == -1).all()), (eps, a)
        if eps == 0.0:
            masked = qc.cpu().masked_fill(x[:, :, 0] != -1, float("-inf"))
            assert torch.equal(a, masked.argmax(1))
    store.check_errors()


def test_wide_large_forward_float_weighted_matches_oracle():
    """A float-weighted set (the FW instance) with ten observables: N = 520, B = 2."""
    from eco_hip.graphs import GraphStore
    from eco_hip._lib import ECO_NORM_PER_GRAPH
    n, B, n_obs = 520, 2, 10
    mats = []
    for b in range(B):
        rng = np.random.default_rng(5200 + b)
        iu, ju = np.triu_indices(n, 1)
        keep = rng.random(iu.size) < 0.02
        m = np.zeros((n, n))
        m[iu[keep], ju[keep]] = rng.uniform(-1.0, 1.0, int(keep.sum()))
        mats.append(m + m.T)
    store = GraphStore.from_dense(mats)
    assert store.float_weights and not store.unit_weights
    w, net, wc = wide_net(520, n_obs)
    xc = wide_x(520, B, n, n_obs).cuda()
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    q = net.forward_graphs(xc, store, gids, norm_scope=ECO_NORM_PER_GRAPH)
    for b in range(B):
        assert scaled_err(q[b], oracle_q(wc, xc[b], mats[b], n_obs), f"float-weighted graph {b}") <= BAR
    store.check_errors()


def test_wide_training_forward_above_512_is_still_rejected():
    from eco_hip.graphs import GraphStore
    n = 600
    store = GraphStore.from_dense([og.er_graph(n, 0.01, np.random.default_rng(0))])
    _, net, _ = wide_net(1)
    x = torch.zeros(1, n, 16, device="cuda")
    gids = torch.zeros(1, dtype=torch.int32, device="cuda")
    saved = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        net.forward_graphs(x, store, gids, norm_scope=1, saved=saved)
    assert N_OBS == net.n_obs_in
