"""Shared pieces of tests/test_wg_grad_cpu.py and tests/test_wg_grad_gpu.py: a float64 torch restatement of the MPNN
forward over the DIRECTED EDGE LIST (index_add instead of the [N, N, 63] edge tensor of mpnn.py:90-100), so autograd
gives the gradient of sum(dq . Q) at N = 8192, where the dense autograd of mpnn_corner_common would need tens of GB.

It restates oracle/mpnn_sparse_oracle.py::forward statement by statement in torch; tests/test_wg_grad_cpu.py pins it
to that oracle (Q) and to the dense autograd (gradients) at sizes where both run.  The two switches `divide_by_degree`
and `norm_scope` are the negative controls of that test, never the reference.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mpnn_oracle as mo

SENTINEL = 1e3          # dead columns of the 8- / 16-float node rows, as mpnn_corner_common.Case


def er_edges(n, mean_deg, rng):
    """About n * mean_deg / 2 distinct undirected pairs (i < j), no dense matrix."""
    k = int(n * mean_deg / 2)
    a, b = rng.integers(0, n, k), rng.integers(0, n, k)
    key = np.unique((np.minimum(a, b) * n + np.maximum(a, b))[a != b])
    return key // n, key % n


def without_vertex(i, j, w, v):
    """The edge list with every edge of vertex v removed (v becomes isolated)."""
    keep = (i != v) & (j != v)
    return i[keep], j[keep], w[keep]


def with_hub(n, i, j, w, hub, wh, skip=()):
    """The edge list with vertex `hub` joined to every other vertex but those of `skip`, weights wh in vertex order;
    hub's own earlier edges are dropped."""
    i, j, w = without_vertex(i, j, w, hub)
    others = np.array([v for v in range(n) if v != hub and v not in skip])
    assert wh.size == others.size
    return (np.concatenate([i, np.minimum(others, hub)]), np.concatenate([j, np.maximum(others, hub)]),
            np.concatenate([w, wh]))


def dense_of(n, i, j, w):
    m = np.zeros((n, n))
    m[i, j] = w
    m[j, i] = w
    return m


def directed(i, j, w, device="cpu", dtype=torch.float64):
    """(u, v, a): both directions of every nonzero edge -- row u, column v, weight a_uv."""
    i, j, w = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(w, np.float64)
    nz = w != 0
    u = torch.from_numpy(np.concatenate([i[nz], j[nz]])).to(device)
    v = torch.from_numpy(np.concatenate([j[nz], i[nz]])).to(device)
    a = torch.from_numpy(np.concatenate([w[nz], w[nz]])).to(device, dtype)
    return u, v, a


def max_degree(n, i, j, w):
    nz = np.asarray(w) != 0
    return max(1, int(np.bincount(np.concatenate([np.asarray(i)[nz], np.asarray(j)[nz]]), minlength=n).max()))


def sparse_forward(w, x, n, u, v, a, norm_max, divide_by_degree=True):
    """MPNN.forward (mpnn.py:40-77) of one graph -> Q [N], in the dtype of x, differentiable in w.
    x [N, n_obs]; (u, v, a) of directed(); norm_max: the norm.max() of :102 (the call's or the graph's)."""
    dt = x.dtype
    W = [w[k] for k in mo.KEYS]
    norm = torch.bincount(u, minlength=n).clamp_min(1).to(dt).unsqueeze(1)        # :36-38
    div = norm if divide_by_degree else torch.ones_like(norm)
    h = F.relu(x @ W[0].T)                                                        # :20-23, :55
    ef = torch.cat([a.unsqueeze(1), x[v]], dim=1)                                 # :90-94, the unmasked entries
    emb = F.relu(ef @ W[1].T)                                                     # :96-99
    emb = torch.zeros(n, emb.shape[1], dtype=dt, device=x.device).index_add(0, u, emb) / div     # :100
    e = F.relu(torch.cat([emb, norm / norm_max], dim=1) @ W[2].T)                 # :102
    for layer in range(3):                                                        # :68-72, :114-120
        agg = torch.zeros(n, 64, dtype=dt, device=x.device).index_add(0, u, a.unsqueeze(1) * h[v]) / div   # :115
        m = F.relu(torch.cat([agg, e], dim=1) @ W[3 + 2 * layer].T)               # :117
        h = F.relu(torch.cat([h, m], dim=1) @ W[4 + 2 * layer].T)                 # :118
    pooled = (h.sum(dim=0) / n) @ W[9].T                                          # :147
    feat = F.relu(torch.cat([pooled.unsqueeze(0).expand(n, pooled.shape[0]), h], dim=1))   # :148-150
    return (feat @ W[10].T + W[11])[:, 0]                                         # :152-153


def sparse_autograd(w, x, graphs, dq, n_obs, dtype=torch.float64, device="cpu", norm_scope="call",
                    divide_by_degree=True):
    """(Q [B, N], {name: d sum(dq . Q) / d w[name]}) for the batch of graphs [(i, j, wt)] * B with node rows
    x [B, N, >= n_obs] and dq [B, N].  norm_scope "call": norm.max() over the whole batch (mpnn.py:102 on a batch,
    ECO_NORM_PER_CALL); "graph": each graph's own."""
    B, n = x.shape[0], x.shape[1]
    wg = {k: t.detach().to(device, dtype).requires_grad_(True) for k, t in w.items()}
    degs = [max_degree(n, *g) for g in graphs]
    qs, total = [], 0.0
    for b, g in enumerate(graphs):
        u, v, a = directed(*g, device=device, dtype=dtype)
        nmax = float(max(degs) if norm_scope == "call" else degs[b])
        q = sparse_forward(wg, x[b, :, :n_obs].to(device, dtype), n, u, v, a, nmax, divide_by_degree)
        total = total + (q * dq[b].to(device, dtype)).sum()
        qs.append(q.detach().cpu())
    total.backward()
    return torch.stack(qs), {k: wg[k].grad.detach().cpu() for k in mo.KEYS}


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def worst_rel_l2(got, ref):
    """Per-tensor relative L2 figures {name: figure} of two gradient dicts."""
    return {k: rel_l2(got[k], ref[k]) for k in mo.KEYS}


def node_rows(B, n, n_obs, gen):
    """Node rows [B, N, 8 | 16] as mpnn_corner_common.Case draws them: live entries in [-1, 1] and nonzero, the
    spin column +-1, SENTINEL in the dead columns."""
    x = torch.full((B, n, 8 if n_obs <= 8 else 16), SENTINEL)
    live = torch.rand(B, n, n_obs, generator=gen) * 2 - 1
    live = torch.where(live.abs() < 1e-3, torch.full_like(live, 0.5), live)
    live[:, :, 0] = torch.where(live[:, :, 0] > 0, 1.0, -1.0)
    x[:, :, :n_obs] = live
    return x


def store_of(n, graphs):
    """A GraphStore of integer-weighted graphs from their edge lists, without a dense matrix."""
    from eco_hip.graphs import CSR, GraphStore, edges_to_csr
    parts = [edges_to_csr(n, *g) for g in graphs]
    assert all(p.weights is None for p in parts)
    base = np.cumsum([0] + [p[2].size for p in parts[:-1]]).astype(np.int64)
    return GraphStore.from_csr(CSR(np.vstack([p[0] for p in parts]), base, np.concatenate([p[2] for p in parts])))
