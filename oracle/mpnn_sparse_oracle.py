"""numpy restatement of the reference MPNN forward over an EDGE LIST (TEST INFRASTRUCTURE ONLY): what
oracle/mpnn_oracle.py::forward_staged computes, statement by statement and with the same citations of
src/networks/mpnn.py, without the [N, N, 63] edge tensor of :90-100 -- so it runs at N = 8192 (a second, a few
MB), where the dense oracle would need 17 GB.

  forward(w, x, n, i, j, wt, n_obs_in=7, norm_max=None) -> Q [N]

x [N, n_obs_in] node features, (i, j, wt) an undirected edge list with every edge given ONCE (no self-loops, no
repeated pair), w the weights under the reference state_dict names (oracle.mpnn_oracle.KEYS; torch tensors or
arrays).  Every operation is float64.  A zero-weight edge is no edge: the dense statements mask it out of the degree
(:36) and of the edge embedding (:94), and it adds nothing to adj @ h (:115).

dtype=np.float32 is the SAME statements in float32 with every row sum accumulated sequentially in edge order (row
u adds its neighbours one after the other).  It is not an oracle: it measures what a float32 evaluation of these
sums costs against the float64 one, which sizes the bar of a float32 kernel on rows of thousands of entries
(tests/test_wg_gpu.py)."""
import numpy as np

from oracle.mpnn_oracle import KEYS


def _relu(a):
    return np.maximum(a, 0)


def _row_sum(rows, vals, n, dt):
    """out[u] = sum of vals[k] over the directed edges k with rows[k] == u.  float64: np.add.at.  Otherwise the
    edges are sorted by row and the t-th entry of every row is added in step t: each row accumulates its entries
    one by one, in edge order, in `dt` (vectorised over the rows, max-degree steps)."""
    out = np.zeros((n, vals.shape[1]), dtype=dt)
    if dt == np.float64:
        np.add.at(out, rows, vals)
        return out
    order = np.argsort(rows, kind="stable")
    r, v = rows[order], vals[order]
    start = np.searchsorted(r, np.arange(n))
    rank = np.arange(r.size) - start[r]            # position of the edge within its row
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2)) if r.size else [0]
    for t in range(len(cuts) - 1):
        k = by_rank[cuts[t]:cuts[t + 1]]           # one entry per row that has a t-th entry: no repeated index
        out[r[k]] += v[k]
    return out


def forward(w, x, n, i, j, wt, n_obs_in=7, norm_max=None, dtype=np.float64, clamp_degree=True):
    """MPNN.forward (:40-77) -> Q [N].  clamp_degree=False leaves out the clamp of :37 (an isolated vertex then
    divides by 0): the negative control of tests/test_mpnn_sparse_oracle_cpu.py, never the oracle."""
    dt = np.dtype(dtype).type
    W = [np.asarray(w[k], dtype=np.float64).astype(dt) for k in KEYS]
    x = np.asarray(x, dtype=np.float64).astype(dt)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    wt = np.asarray(wt, dtype=np.float64)
    assert x.shape == (n, n_obs_in) and i.shape == j.shape == wt.shape and not np.any(i == j)
    key = np.minimum(i, j) * n + np.maximum(i, j)
    assert np.unique(key).size == key.size, "every edge once"
    nz = wt != 0
    u = np.concatenate([i[nz], j[nz]])             # directed: row u, column v, a_uv
    v = np.concatenate([j[nz], i[nz]])
    a = np.concatenate([wt[nz], wt[nz]]).astype(dt)
    norm = np.bincount(u, minlength=n).astype(np.int64)[:, None]      # :36
    if clamp_degree:
        norm[norm == 0] = 1                                           # :37
    norm = norm.astype(dt)                                            # :38
    h = _relu(x @ W[0].T)                                             # :20-23, :55
    # EdgeAndNodeEmbeddingLayer (:89-104)
    ef = np.concatenate([a[:, None], x[v]], axis=1)                   # :90-94, the unmasked entries
    emb = _relu(ef @ W[1].T)                                          # :96-99 (a masked entry embeds to relu(0) = 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        emb = _row_sum(u, emb, n, dt) / norm                          # :100
        nmax = norm.max() if norm_max is None else dt(norm_max)
        e = _relu(np.concatenate([emb, norm / nmax], axis=1) @ W[2].T)    # :102
        for layer in range(3):                                        # :68-72, :114-120
            agg = _row_sum(u, a[:, None] * h[v], n, dt) / norm        # :115
            m = _relu(np.concatenate([agg, e], axis=1) @ W[3 + 2 * layer].T)   # :117
            h = _relu(np.concatenate([h, m], axis=1) @ W[4 + 2 * layer].T)     # :118
    # ReadoutLayer (:143-159)
    if dt == np.float64:
        mean = h.sum(axis=0) / n                                      # :147
    else:
        mean = np.zeros(h.shape[1], dtype=dt)
        for row in h:                                                 # sequential, vertex order
            mean += row
        mean = mean / dt(n)
    pooled = mean @ W[9].T
    feat = _relu(np.concatenate([np.broadcast_to(pooled, (n, pooled.size)), h], axis=1))   # :148-150
    q = feat @ W[10].T + W[11]                                        # :152-153
    return q[:, 0]


def f32_cost(w, x, n, i, j, wt, n_obs_in=7, norm_max=None):
    """(Q64, E32): the float64 Q and the largest |Q32 - Q64| / (1 + |Q64|) of the float32 mode."""
    q64 = forward(w, x, n, i, j, wt, n_obs_in, norm_max)
    q32 = forward(w, x, n, i, j, wt, n_obs_in, norm_max, dtype=np.float32).astype(np.float64)
    return q64, float(np.max(np.abs(q32 - q64) / (1 + np.abs(q64))))
