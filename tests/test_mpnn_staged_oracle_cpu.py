"""oracle.mpnn_oracle.forward_staged (the float64-clean forward that also returns every intermediate under its
SV_* name) pinned to oracle.mpnn_oracle.forward, the judge of test_dense_gpu / test_weighted_mpnn_gpu:
  fp32: bitwise the same Q (reference fixture tests/golden/mpnn_fwd.npz and n_obs_in = 1, 8, 9, 16);
  float64: Q within the project's bar 5e-7 (1 + |q|) of the fp32 result;
  float64 autograd: every parameter gradient within 1e-12 relative L2 of autograd through forward(w.double(), ...).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import graphs as og
from oracle import mpnn_oracle as mo


def _split(obs, n_obs):
    """x, adj as mpnn.py:44-50 slices them (views of the transposed observation, as forward() takes them)."""
    t = (obs.unsqueeze(0) if obs.dim() == 2 else obs).transpose(-1, -2)     # :41-44
    return t[:, :, :n_obs], t[:, :, n_obs:]


def _random_case(n_obs, n=12, B=3, seed=0, float_weights=False):
    g = torch.Generator().manual_seed(100 + n_obs + seed)
    w = mo.init_weights(g, std=0.1, n_obs_in=n_obs)
    rng = np.random.default_rng(n_obs + seed)
    obs = []
    for b in range(B):
        J = og.er_graph(n, 0.3, rng)
        if float_weights:
            J = J * np.triu(rng.uniform(0.1, 1.0, (n, n)), 1)
            J = J + J.T
        if b == 1:
            J[3, :] = J[:, 3] = 0.0   # an isolated vertex: the 0 -> 1 clamp of :37
        obs.append(np.vstack([rng.uniform(-1, 1, (n_obs, n)), J]))
    return w, torch.from_numpy(np.array(obs)).float()


def _golden_cases():
    f = np.load(os.path.join(GOLDEN, "mpnn_fwd.npz"))
    for p, key in (("er200/", "obs"), ("er200/", "obs_binary"), ("er20/", "obs")):
        w = {k: torch.from_numpy(f[p + k]) for k in mo.KEYS}
        yield p + key, w, torch.from_numpy(f[p + key]).float(), 7


def _cases():
    yield from _golden_cases()
    for n_obs in (1, 8, 9, 16):
        w, obs = _random_case(n_obs, float_weights=n_obs == 9)
        yield f"random n_obs={n_obs}", w, obs, n_obs


def test_fp32_is_bitwise_forward_and_float64_is_within_the_q_bar():
    for name, w, obs, n_obs in _cases():
        ref = mo.forward(w, obs, n_obs_in=n_obs)
        x, adj = _split(obs, n_obs)
        q, st = mo.forward_staged(w, x, adj, n_obs)
        assert q.dtype == torch.float32 and torch.equal(q, ref), name
        assert list(st) and sorted(st) == sorted(mo.STAGES), name
        w64 = {k: v.double() for k, v in w.items()}
        x64, adj64 = _split(obs.double(), n_obs)
        q64, st64 = mo.forward_staged(w64, x64, adj64, n_obs)
        assert q64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in st64.values()), name
        err = float(((q64 - q.double()).abs() / (1 + q64.abs())).max())
        print(f"{name}: float64 vs fp32 scaled err {err:.3e}")
        assert err <= 5e-7, (name, err)
        B, N = adj.shape[0], adj.shape[1]
        for k, v in st64.items():
            assert v.shape == ((B, 64) if k in ("MEAN", "P") else (B, N, 64)), (name, k)


def test_norm_max_argument_matches_forward():
    w, obs = _random_case(7, seed=3)
    x, adj = _split(obs, 7)
    q, _ = mo.forward_staged(w, x[:1], adj[:1], 7, norm_max=9.0)
    assert torch.equal(q, mo.forward(w, obs[:1], norm_max=9.0))


@pytest.mark.parametrize("n_obs,float_weights", [(7, False), (13, True)])
def test_float64_autograd_equals_autograd_through_forward(n_obs, float_weights):
    # forward() in float64 still rounds norm / norm.max() to fp32 (norm.float(), the very thing forward_staged
    # avoids), which alone moves the edge_feature_NN gradient by 1e-8.  The two agree to float64 rounding exactly
    # when those quotients are fp32 numbers, so the case is the first seed whose largest degree is a power of two.
    for seed in range(64):
        w, obs = _random_case(n_obs, seed=seed, float_weights=float_weights)
        nmax = int(mo.batch_norm_max(obs, n_obs))
        if nmax in (4, 8):
            break
    assert nmax in (4, 8)
    dq =torch.randn(obs.shape[0], obs.shape[2], generator=torch.Generator().manual_seed(1)).double()
    wa = {k: v.double().requires_grad_(True) for k, v in w.items()}
    (mo.forward(wa, obs.double(), n_obs_in=n_obs) * dq).sum().backward()
    wb = {k: v.double().requires_grad_(True) for k, v in w.items()}
    x, adj = _split(obs.double(), n_obs)
    q, _ = mo.forward_staged(wb, x, adj, n_obs)
    (q * dq).sum().backward()
    for k in mo.KEYS:
        err = float((wa[k].grad - wb[k].grad).norm() / wa[k].grad.norm())
        print(f"{k}: relative L2 {err:.3e}")
        assert err <= 1e-12, (k, err)
