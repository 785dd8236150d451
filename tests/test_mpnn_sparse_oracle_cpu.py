"""oracle.mpnn_sparse_oracle.forward (float64 over an edge list, the judge of tests/test_wg_gpu.py above 2304
vertices) pinned to oracle.mpnn_oracle.forward_staged in float64 on the same graph as a dense matrix.

Bar: 1e-12 absolute.  Both sides are float64 evaluations of the same statements that differ only in the order of
their sums (at most 200 terms of magnitude <= 127 * O(1)), so they agree to a few ulps of values of order 1 -- the
measured difference is 2e-16 to 1e-15 for |Q| up to 2.6; 1e-12 leaves three decimal digits and is six below what
any wrong statement moves Q by (the negative controls at the end: > 1e-6 each).

The graphs: vertex 0 joins every vertex but one, which stays isolated (the longest row the format allows and the
0 -> 1 clamp of mpnn.py:37 in one graph), over a sparse random background; weights from {-1, +1} with a few +-127."""
import numpy as np
import pytest
import torch

from oracle import mpnn_oracle as mo
from oracle import mpnn_sparse_oracle as ms

BAR = 1e-12


def _hub_graph(n, rng):
    """(i, j, wt, iso): hub 0 -- every vertex but `iso`; ER background of mean degree 3 on the others."""
    iso = n - 2
    others = np.array([v for v in range(1, n) if v != iso])
    k = 3 * n // 2
    a, b = rng.choice(others, k), rng.choice(others, k)
    keep = a != b
    key = np.unique(np.minimum(a, b)[keep] * n + np.maximum(a, b)[keep])
    i = np.concatenate([np.zeros(others.size, np.int64), key // n])
    j = np.concatenate([others, key % n])
    wt = rng.choice([-1.0, 1.0], i.size)
    wt[rng.choice(i.size, 6, replace=False)] = [127, -127, 127, -127, 127, -127]
    wt[others.size - 1] = 127.0            # the hub's edge to the last vertex
    return i, j, wt, iso


def _case(n, n_obs, seed=0):
    rng = np.random.default_rng(1000 * n + n_obs + seed)
    i, j, wt, iso = _hub_graph(n, rng)
    g = torch.Generator().manual_seed(n + n_obs)
    w = {k: v.double() for k, v in mo.init_weights(g, std=0.05, n_obs_in=n_obs).items()}
    x = rng.uniform(-1, 1, (n, n_obs))
    return w, x, i, j, wt, iso


def _dense(n, i, j, wt):
    J = np.zeros((n, n))
    J[i, j] = wt
    J[j, i] = wt
    return J


def _staged(w, x, J, n_obs, norm_max):
    q, _ = mo.forward_staged(w, torch.from_numpy(x)[None], torch.from_numpy(J)[None], n_obs, norm_max=norm_max)
    return q.numpy()


@pytest.mark.parametrize("norm_max", [None, "twice"])
@pytest.mark.parametrize("n_obs", [7, 13])
@pytest.mark.parametrize("n", [61, 200])
def test_sparse_float64_equals_forward_staged(n, n_obs, norm_max):
    w, x, i, j, wt, iso = _case(n, n_obs)
    J = _dense(n, i, j, wt)
    assert (J[0] != 0).sum() == n - 2 and not J[iso].any() and J[0, n - 1] == 127 and (np.abs(J) == 127).sum() >= 8
    nm = None if norm_max is None else 2 * (n - 2)      # a call-wide maximum larger than the graph's own n - 2
    want = _staged(w, x, J, n_obs, nm)
    got = ms.forward(w, x, n, i, j, wt, n_obs_in=n_obs, norm_max=nm)
    d = float(np.abs(got - want).max())
    print(f"n {n} n_obs {n_obs} norm_max {nm}: max |sparse - staged| = {d:.2e}, |Q| up to {np.abs(want).max():.3g}")
    assert got.shape == (n,) and got.dtype == np.float64 and np.isfinite(got).all()
    assert d <= BAR
    assert np.ptp(want) > 1e-3                          # Q is no constant: the comparison sees the graph
    # the direction of an edge in the list and the order of the list are immaterial
    p = np.random.default_rng(1).permutation(i.size)
    flip = ms.forward(w, x, n, j[p], i[p], wt[p], n_obs_in=n_obs, norm_max=nm)
    assert np.abs(flip - want).max() <= BAR


def test_zero_weight_edge_is_no_edge():
    n, n_obs = 61, 7
    w, x, i, j, wt, iso = _case(n, n_obs)
    want = ms.forward(w, x, n, i, j, wt)
    got = ms.forward(w, x, n, np.append(i, iso), np.append(j, 5), np.append(wt, 0.0))
    assert np.array_equal(got, want)
    assert np.abs(got - _staged(w, x, _dense(n, i, j, wt), n_obs, None)).max() <= BAR


@pytest.mark.parametrize("n_obs", [7, 13])
def test_float32_mode_is_the_same_forward_at_float32_accuracy(n_obs):
    """The float32 mode (sequential row sums) differs from float64 by float32 rounding and no more: below 1e-4
    (1 + |q|) -- rows of 198 terms of magnitude up to 127, eps32 = 6e-8 -- and above 0."""
    n = 200
    w, x, i, j, wt, _ = _case(n, n_obs)
    q64, e32 = ms.f32_cost(w, x, n, i, j, wt, n_obs_in=n_obs)
    print(f"n_obs {n_obs}: E32 = {e32:.2e}")
    assert 0 < e32 < 1e-4
    assert np.array_equal(q64, ms.forward(w, x, n, i, j, wt, n_obs_in=n_obs))


@pytest.mark.parametrize("n", [61, 200])
def test_negative_controls_move_q(n):
    """What the comparison above must notice, each by more than 1e-6 somewhere (a million bars): one hub edge
    dropped, the degree left unclamped (the isolated vertex divides 0 by 0: a NaN counts as moved), and the
    caller's norm_max ignored."""
    n_obs = 7
    w, x, i, j, wt, iso = _case(n, n_obs)
    nm = 2 * (n - 2)
    want = _staged(w, x, _dense(n, i, j, wt), n_obs, nm)

    def moved(q):
        return bool((~(np.abs(q - want) <= 1e-6)).any())

    assert not moved(ms.forward(w, x, n, i, j, wt, norm_max=nm))
    drop = np.ones(i.size, bool)
    drop[3] = False                                      # the hub's edge to vertex 4, weight +-1
    assert i[3] == 0 and abs(wt[3]) in (1, 127)
    assert moved(ms.forward(w, x, n, i[drop], j[drop], wt[drop], norm_max=nm))
    assert moved(ms.forward(w, x, n, i, j, wt, norm_max=nm, clamp_degree=False))
    assert moved(ms.forward(w, x, n, i, j, wt))          # the graph's own maximum n - 2 in place of norm_max
