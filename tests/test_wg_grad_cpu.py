"""Training on 2049 to 8192 vertices without a GPU.

1. The float64 edge-list restatement of tests/wg_grad_common.py, the reference of tests/test_wg_grad_gpu.py above the
   sizes the dense autograd can hold, is pinned where both run: N = 61 and N = 200, two graphs each (graph 0 with a
   hub joined to every vertex but an isolated one, graph 1 with an isolated vertex and short rows), 7 and 13
   observables.  Q within 1e-12 (1 + |q|) of oracle.mpnn_sparse_oracle and every gradient tensor within 1e-10
   relative L2 of mpnn_corner_common._autograd in float64: both figures are float64 rounding in another summation
   order (measured: at most 6e-17 and 1.2e-15).  Two negative controls -- the restatement without the division by the degree,
   and with each graph's own norm.max() instead of the call's -- must move a gradient tensor by more than 1e-6.
2. eco_mpnn_grad_wg and its bytes query are declared in include/eco_hip.h, exported, bound with argtypes, and
   MPNN.grad_wg exists; the query is 0 outside its range and positive and 256 B aligned inside it;
   eco_mpnn_grad_large keeps its range.
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import mpnn_oracle as mo
from oracle import mpnn_sparse_oracle as ms
import mpnn_corner_common as cc
import wg_grad_common as wc

NAMES = ("eco_mpnn_grad_wg", "eco_mpnn_grad_wg_workspace_bytes")


def _graphs(n, rng):
    hub, iso = n - 1, 5
    i, j = wc.er_edges(n, 6.0, rng)
    g0 = wc.without_vertex(i, j, rng.choice([-3, -2, -1, 1, 2], i.size), iso)
    g0 = wc.with_hub(n, *g0, hub=hub, wh=rng.choice([-1, 1], n - 2), skip=(iso,))
    i, j = wc.er_edges(n, 4.0, rng)
    g1 = wc.without_vertex(i, j, rng.choice([-1, 1], i.size), 11)
    return [g0, g1]


_CASES = {}


def _case(n, n_obs):
    """(Case, its edge lists, the restatement's float64 Q and gradients), computed once."""
    if (n, n_obs) not in _CASES:
        graphs = _graphs(n, np.random.default_rng(100 * n + n_obs))
        deg = [np.bincount(np.concatenate([g[0], g[1]]), minlength=n) for g in graphs]
        assert deg[0][n - 1] == n - 2 and deg[0][5] == 0 and deg[1][11] == 0 and deg[1].max() < n // 2
        case = cc.Case(f"n{n}-obs{n_obs}", [wc.dense_of(n, *g) for g in graphs], n_obs, seed=n + n_obs, dq="dense")
        q, g = wc.sparse_autograd(case.w, case.x, graphs, case.dq, n_obs)
        _CASES[(n, n_obs)] = (case, graphs, q, g)
    return _CASES[(n, n_obs)]


SIZES = [(61, 7), (61, 13), (200, 7), (200, 13)]


@pytest.mark.parametrize("n,n_obs", SIZES)
def test_restatement_matches_sparse_oracle_and_dense_autograd(n, n_obs):
    case, graphs, q, g = _case(n, n_obs)
    nmax = max(wc.max_degree(n, *gr) for gr in graphs)
    assert nmax == n - 2
    for b, gr in enumerate(graphs):
        ref = torch.from_numpy(ms.forward(case.w, case.x[b, :, :n_obs].numpy(), n, *gr, n_obs_in=n_obs, norm_max=nmax))
        err = float(((q[b] - ref).abs() / (1 + ref.abs())).max())
        print(f"{case.name} graph {b}: Q against oracle.mpnn_sparse_oracle {err:.2e}")
        assert err <= 1e-12
    q_dense, g_dense = cc._autograd(case, torch.float64, "cpu")
    assert float(((q - q_dense).abs() / (1 + q_dense.abs())).max()) <= 1e-12
    errs = wc.worst_rel_l2(g, g_dense)
    print(f"{case.name}: gradients against the dense float64 autograd: " + ", ".join(f"{e:.1e}" for e in errs.values()))
    assert max(errs.values()) <= 1e-10, errs


@pytest.mark.parametrize("n,n_obs", [(61, 7), (200, 13)])
def test_negative_controls_move_the_gradient(n, n_obs):
    case, graphs, _, g = _case(n, n_obs)
    for name, kw in (("no division by the degree", dict(divide_by_degree=False)),
                     ("per-graph norm.max()", dict(norm_scope="graph"))):
        _, bad = wc.sparse_autograd(case.w, case.x, graphs, case.dq, n_obs, **kw)
        moved = max(wc.worst_rel_l2(bad, g).values())
        print(f"{case.name}: {name} moves a gradient tensor by {moved:.2e}")
        assert moved > 1e-6, name


def test_symbols_declared_exported_and_bound():
    from eco_hip import _lib
    src = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _lib.EXPORTS, name
        assert hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert len(_lib.lib.eco_mpnn_grad_wg.argtypes) == len(_lib.lib.eco_mpnn_grad_large.argtypes) == 10
    from eco_hip.networks.mpnn import MPNN
    assert callable(MPNN.grad_wg) and callable(MPNN.grad_wg_bytes)


def test_workspace_bytes_range():
    from eco_hip import _lib
    from eco_hip.networks.mpnn import MPNN
    q = _lib.lib.eco_mpnn_grad_wg_workspace_bytes
    for n, b in ((2048, 1), (8193, 1), (4100, 0), (8192, 4096), (512, 4), (0, 1), (-1, 1), (4100, -2)):
        assert q(n, b) == 0, (n, b)
    for n, b in ((2049, 1), (4100, 3), (8192, 2), (8192, 4095)):
        v = q(n, b)
        assert v > 0 and v % 256 == 0, (n, b, v)
        assert MPNN.grad_wg_bytes(n, b) == v
        # at least the 12 saved and 11 gradient node tensors, the gather rows and the three forward row buffers
        assert v >= 27 * b * n * 256
    assert q(8192, 2) > q(8192, 1) > q(4100, 1) > q(2049, 1)
    # about 27 x rows_pad x 256 B per sample: 56.6 MB at 8192 vertices
    assert abs((q(8192, 2) - q(8192, 1)) - 56.6e6) < 0.1e6
    assert _lib.lib.eco_mpnn_grad_large_workspace_bytes(2049, 1) == 0
    assert _lib.lib.eco_mpnn_grad_large_workspace_bytes(2048, 1) > 0
