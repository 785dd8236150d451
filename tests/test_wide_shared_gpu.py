"""More than 8 observables (16-float node rows) on the shared-graph path (one +-1 graph above 512 vertices, many
episodes: csrc/eco_mpnn_shared.h).  The aggregation launches build U, V and h0 from the rows with four MFMA K-steps
(shared_agg_kernel<1..3, 16>), the first update layer rebuilds h0 with lin16 (shared_lin_kernel<1, 16>), the readout
reads feature 0 with the row stride.

Bar: 5e-5 in |q - ref| / (1 + |ref|) against the fp32 torch oracle (on the GPU) and against the per-episode
global-memory kernel on the graph replicated per episode: the bar tests/test_parity_bench_sizes_gpu.py sets for the
8-float-row instances of the same kernels."""
import numpy as np
import pytest
import torch

from oracle import graphs as og
from wide_common import oracle_q, scaled_err, wide_net, wide_x

pytestmark = pytest.mark.gpu

BAR = 5e-5


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _both(net, xc, J, B):
    """Q of the shared-graph path (one graph, B episodes) and of the per-episode kernel (the graph B times)."""
    from eco_hip.graphs import GraphStore
    from eco_hip._lib import ECO_NORM_PER_CALL
    one = GraphStore.from_dense([J])
    rep = GraphStore.from_dense([J] * B)
    assert one.unit_weights
    q1 = net.forward_graphs(xc, one, torch.zeros(B, dtype=torch.int32, device="cuda"), norm_scope=ECO_NORM_PER_CALL)
    qr = net.forward_graphs(xc, rep, torch.arange(B, dtype=torch.int32, device="cuda"), norm_scope=ECO_NORM_PER_CALL)
    assert torch.isfinite(q1).all()
    return one, q1, qr


@pytest.mark.parametrize("weights", ["uniform", "discrete"])
def test_wide_shared_forward_matches_per_episode_and_oracle(weights):
    """N = 600, B = 37 (full slices and a padded one); "discrete" (+-1) runs the A- / V pass."""
    from eco_hip._lib import ActConfig, ECO_NORM_PER_CALL
    n, B = 600, 37
    J = og.er_graph(n, 0.02, np.random.default_rng(600), weights=weights)
    w, net, wc = wide_net(6)
    x = wide_x(6, B, n)
    xc = x.cuda()
    one, q1, qr = _both(net, xc, J, B)
    assert scaled_err(q1, qr, f"{weights}: shared vs per-episode") <= BAR
    for b in (0, 15, 16, 36):
        assert scaled_err(q1[b], oracle_q(wc, xc[b], J), f"{weights}: episode {b} vs oracle") <= BAR
    gz = torch.zeros(B, dtype=torch.int32, device="cuda")
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    qa = torch.empty(B, n, device="cuda")
    net.forward_graphs(xc, one, gz, norm_scope=ECO_NORM_PER_CALL, q_out=qa, act=ActConfig(0.0, 1, 0.0, 1, 0),
                       actions_out=acts)
    assert torch.equal(acts.long(), qa.argmax(1))
    # irreversible act through shared_readout_kernel: feature 0 read with the 16-float stride
    for eps in (0.0, 1.0):
        net.forward_graphs(xc, one, gz, norm_scope=ECO_NORM_PER_CALL, act=ActConfig(eps, 0, -1.0, 3, 1),
                           actions_out=acts)
        a = acts.long().cpu()
        assert bool((x[torch.arange(B), a, 0] == -1).all())
        if eps == 0.0:
            assert torch.equal(a, qa.cpu().masked_fill(x[:, :, 0] != -1, float("-inf")).argmax(1))


def test_wide_shared_forward_n2048():
    """N = 2048, the largest block: padding words point at row 0 with weight 0 (no zero row behind the block).
    Against the per-episode kernel only (the oracle's edge tensor is about 1 GB at this size)."""
    n, B = 2048, 5
    J = og.er_graph(n, 0.005, np.random.default_rng(2048), weights="discrete")
    _, net, _ = wide_net(20)
    xc = wide_x(20, B, n).cuda()
    _, q1, qr = _both(net, xc, J, B)
    assert scaled_err(q1, qr, "N=2048: shared vs per-episode") <= BAR


def _packed_table_words(J):
    """16-bit words of the shared path's packed edge table (shared_pack_kernel): tiles of 16 nodes ranked by
    decreasing degree, each tile 16 x its longest row rounded up to 4 edges."""
    deg = np.sort((J != 0).sum(1))[::-1]
    return int(16 * ((deg[::16] + 3) // 4 * 4).sum())


def test_wide_shared_forward_edge_table_beside_narrow_weights_only():
    """shared_agg_kernel keeps the packed edge table in LDS when
    (2 N + 2) 16 + (words + 64) 2 + 4 WL <= 160 KB, WL = 576 floats of x-build weights for 8-float rows and 1088 for
    16-float rows.  This graph's table fits beside the 576 but not beside the 1088: the wide x-build launches read
    the table from L2 (in_lds == false) while the two h aggregations of the same call keep it in LDS."""
    n, B = 1000, 9
    J = og.er_graph(n, 0.0622, np.random.default_rng(1002), weights="discrete")
    lds, block = 160 * 1024, (2 * n + 2) * 16
    table = (_packed_table_words(J) + 64) * 2
    assert block + table + 576 * 4 <= lds < block + table + 1088 * 4, (block, table)
    w, net, wc = wide_net(10)
    xc = wide_x(10, B, n).cuda()
    _, q1, qr = _both(net, xc, J, B)
    assert scaled_err(q1, qr, "table in L2: shared vs per-episode") <= BAR
    for b in (0, 8):
        assert scaled_err(q1[b], oracle_q(wc, xc[b], J), f"table in L2: episode {b} vs oracle") <= BAR


def test_wide_shared_forward_hub_and_isolated_nodes():
    """A hub adjacent to every other vertex and two isolated vertices, N = 700, B = 6."""
    n, B = 700, 6
    rng = np.random.default_rng(700)
    J = og.er_graph(n, 0.01, rng, weights="discrete")
    for v in (5, 17):
        J[v, :] = 0
        J[:, v] = 0
    hub = 3
    wv = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    wv[[hub, 5, 17]] = 0
    J[hub, :] = wv
    J[:, hub] = wv
    w, net, wc = wide_net(7)
    xc = wide_x(7, B, n).cuda()
    _, q1, qr = _both(net, xc, J, B)
    assert scaled_err(q1, qr, "hub: shared vs per-episode") <= BAR
    for b in (0, 5):
        assert scaled_err(q1[b], oracle_q(wc, xc[b], J), f"hub: episode {b} vs oracle") <= BAR


def test_wide_no_shared_bit_routes_to_the_per_episode_kernel():
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 600, 20
    J = og.er_graph(n, 0.02, np.random.default_rng(601), weights="discrete")
    one = GraphStore.from_dense([J])
    _, net, _ = wide_net(8)
    xc = wide_x(8, B, n).cuda()
    gz = torch.zeros(B, dtype=torch.int32, device="cuda")
    res = {}
    for mask in (0, _lib.ECO_PATH_NO_SHARED):
        with _lib.kernel_paths(mask):
            q = torch.empty(B, n, device="cuda")
            a = torch.empty(B, dtype=torch.int32, device="cuda")
            net.forward_graphs(xc, one, gz, norm_scope=_lib.ECO_NORM_PER_CALL, q_out=q,
                               act=_lib.ActConfig(0.0, 1, 0.0, 1, 0), actions_out=a)
            torch.cuda.synchronize()
            res[mask] = (q, a)
    (q0, a0), (q1, a1) = res[0], res[_lib.ECO_PATH_NO_SHARED]
    assert not torch.equal(q0, q1)  # two kernel families: other summation orders
    assert scaled_err(q1, q0, "NO_SHARED vs default") <= BAR
    assert torch.equal(a0.long(), q0.argmax(1)) and torch.equal(a1.long(), q1.argmax(1))
