"""On-device generation of float-weighted graphs (eco_graphs_generate weight kind 2: uniform in (-1, 1))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _csr(store):
    rp = store.row_ptr.cpu().numpy()
    eb = store.edge_base.cpu().numpy()
    ed = store.edges.cpu().numpy().view(np.uint32)
    ew = store.edge_weights.cpu().numpy() if store.float_weights else None
    return rp, eb, ed, ew


@pytest.mark.parametrize("kind,param", [("ER", 0.15), ("BA", 4)])
def test_kind2_weights_are_symmetric_uniform_and_reproducible(kind, param):
    from eco_hip.graphs import GraphStore
    n, G = 40, 256
    st = GraphStore.generated(kind, G, n, param, seed=11, weights="random")
    st.check_errors()
    assert st.float_weights and not st.unit_weights
    rp, eb, ed, ew = _csr(st)
    ref = GraphStore.generated(kind, G, n, param, seed=11, weights="discrete")
    rpd, ebd, edd, _ = _csr(ref)
    np.testing.assert_array_equal(rp, rpd)                    # same edge structure as kind 1 for the seed
    allw = []
    for g in range(G):
        m = st.dense(g)
        np.testing.assert_array_equal(m, m.T)
        assert not np.diag(m).any()
        k = rp[g, -1]
        cols, colsd = ed[eb[g]:eb[g] + k] & 0xFFFFFF, edd[ebd[g]:ebd[g] + k] & 0xFFFFFF
        np.testing.assert_array_equal(cols, colsd)
        wg = ew[eb[g]:eb[g] + k]
        assert np.all(wg != 0) and np.all(np.abs(wg) < 1)
        sign = ((ed[eb[g]:eb[g] + k] >> 24).astype(np.uint8)).view(np.int8)
        np.testing.assert_array_equal(sign, np.sign(wg).astype(np.int8))
        assert (m != 0).sum() == k                            # sorted, distinct columns
        allw.append(m[np.triu_indices(n, 1)][m[np.triu_indices(n, 1)] != 0])
    w = np.concatenate(allw)                                  # one draw per undirected edge
    k = w.size
    # uniform(-1, 1): mean 0 (sd 1/sqrt(3)), variance 1/3 (sd of w^2 = sqrt(1/5 - 1/9))
    assert abs(w.mean()) <= 4 * np.sqrt(1 / 3 / k), w.mean()
    assert abs((w ** 2).mean() - 1 / 3) <= 4 * np.sqrt((1 / 5 - 1 / 9) / k), (w ** 2).mean()
    # normalisers of the generated set against numpy, and the same seed gives the same bits
    meta = st.meta.cpu().numpy()
    for g in (0, G - 1):
        J = st.dense(g)
        assert abs(meta[g, 1] - max(1, J[J > 0].sum() / 2)) <= 1e-12 and abs(meta[g, 3] - J.sum()) <= 1e-12
    again = GraphStore.generated(kind, G, n, param, seed=11, weights="random")
    assert torch.equal(again.edges, st.edges) and torch.equal(again.row_ptr, st.row_ptr)
    assert torch.equal(again.edge_weights.view(torch.int64), st.edge_weights.view(torch.int64))
    assert torch.equal(again.meta.view(torch.int64), st.meta.view(torch.int64))
    other = GraphStore.generated(kind, G, n, param, seed=12, weights="random")
    assert not torch.equal(other.edge_weights, st.edge_weights)
