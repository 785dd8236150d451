"""DQN(loss="huber", max_grad_norm=c) on the device: eco_dqn_td_loss and eco_grad_clip against exact / float64
references, DQN.train_step against the reference's own recorded steps (tests/golden/dqn_step_huber_clip*.npz,
pinned on the CPU by tests/test_huber_clip_golden_cpu.py), and the agent-level behaviour.

Tolerances are stated per test."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from huber_clip_common import clipped_agents, load_golden
from oracle import mpnn_oracle as mo
from test_dqn_gpu import _dqn_for, _flat_to_dict, _split

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ golden parity
@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _run_golden_agent(f, prefix):
    """The recorded agent's three train steps through DQN.train_step; yields (step, loss, agent) after each."""
    from eco_hip.graphs import GraphStore
    n, M, steps = 20, 16, int(f["steps"])
    adj = [a for s in range(steps) for a in f[f"s{s}/states"][:, 7:, :]]
    store = GraphStore.from_dense(adj)
    kw = {} if prefix == "huber/" else {"max_grad_norm": float(f[prefix + "max_grad_norm"])}
    agent = _dqn_for(store, n, B=M, minibatch_size=M, gamma=float(f["gamma"]), loss="huber", **kw)
    agent.network.load_state_dict({k: torch.from_numpy(f["w0/" + k]) for k in mo.KEYS})
    agent.target_network.load_state_dict({k: torch.from_numpy(f["target/" + k]) for k in mo.KEYS})
    for s in range(steps):
        p = f"s{s}/"
        xs, _ = _split(f[p + "states"])
        xn, _ = _split(f[p + "states_next"])
        gid = torch.arange(s * M, (s + 1) * M, dtype=torch.int32, device="cuda")
        act = torch.from_numpy(f[p + "actions"][:, 0].astype(np.int32)).cuda()
        rew = torch.from_numpy(f[p + "rewards"][:, 0]).cuda()
        done = torch.from_numpy(f[p + "dones"][:, 0]).cuda()
        yield s, agent.train_step((xs, act, rew, xn, done, gid)), agent


def _check_loss_and_weights(f, prefix, s, loss, agent):
    """The bars of test_train_step_matches_reference_three_steps."""
    ref_loss = float(f[f"{prefix}s{s}/loss"])
    print(f"{prefix} step {s}: loss {loss!r} ref {ref_loss!r}")
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (s, loss, ref_loss)
    got = _flat_to_dict(agent.network.flat.cpu())
    for k in mo.KEYS:
        np.testing.assert_allclose(got[k].numpy(), f[f"{prefix}s{s}/w/" + k], rtol=0, atol=2e-6,
                                   err_msg=f"{prefix} step {s} {k}")


def test_huber_train_step_matches_reference_three_steps(golden):
    f = golden
    for s, loss, agent in _run_golden_agent(f, "huber/"):
        _check_loss_and_weights(f, "huber/", s, loss, agent)
        assert agent.grad_norm is None


def test_huber_clipped_train_step_matches_reference_three_steps(golden):
    """Adam is nearly invariant to a uniform gradient scale, so besides loss and weights: the norm
    (agent.grad_norm[0]) against the value clip_grad_norm_ returned, to 1e-5 relative (it inherits the gradient's
    own error), the coefficient it implies, and after the first step -- which the fixture clips -- the clipped
    gradient itself, relative L2 per parameter tensor under the 2e-4 of test_backward_matches_autograd."""
    f = golden
    agents = clipped_agents(f)
    assert agents
    for prefix in agents:
        c = float(f[prefix + "max_grad_norm"])
        for s, loss, agent in _run_golden_agent(f, prefix):
            _check_loss_and_weights(f, prefix, s, loss, agent)
            norm, coef = (float(v) for v in agent.grad_norm.cpu())
            ref_norm = float(f[f"{prefix}s{s}/norm"])
            print(f"{prefix} step {s}: norm {norm!r} ref {ref_norm!r} coef {coef!r}")
            assert abs(norm - ref_norm) <= 1e-5 * ref_norm, (s, norm, ref_norm)
            ref_coef = min(1.0, c / (ref_norm + 1e-6))
            assert abs(coef - ref_coef) <= 1e-5 * ref_coef, (s, coef, ref_coef)
            if s == 0:
                got = _flat_to_dict(agent.grad.cpu())
                for k in mo.KEYS:
                    ref = torch.from_numpy(f[f"{prefix}s0/grad/" + k])
                    err = (got[k] - ref).norm() / max(ref.norm(), 1e-12)
                    assert err < 2e-4, (k, float(err), float(ref.norm()))
    if "clip/" in agents:
        assert float(f["clip/s0/norm"]) > float(f["clip/max_grad_norm"])   # the first step's gradient IS clipped


# ------------------------------------------------------------------ eco_dqn_td_loss
def _td_inputs():
    """B = 64, N = 20: q, rewards and target Q multiples of 1/8 in [-4, 4], gamma = 0.5, so td is a multiple of
    1/16 and every intermediate (d, 0.5 d^2, |d| - 0.5, d / 64 and their sums) is exact in fp32.  The first
    samples pin d = 0, +-1, +-15/16 (just inside) and +-7.5 (far outside); a_star has out-of-range entries."""
    B, N = 64, 20
    g = torch.Generator().manual_seed(11)
    eighth = lambda *shape: torch.randint(-32, 33, shape, generator=g).float() / 8   # noqa: E731
    q_s, q_tn, rew = eighth(B, N), eighth(B, N), eighth(B)
    act = torch.randint(0, N, (B,), generator=g, dtype=torch.int32)
    a_star = torch.randint(0, N, (B,), generator=g, dtype=torch.int32)
    done = (torch.rand(B, generator=g) < 0.4).float()
    a_star[8], a_star[9], a_star[10] = -1, N, 1 << 30
    # pinned samples: (d, reward, done, target q at a_star), td = reward + (1 - done) * 0.5 * qt
    pins = [(0.0, 0.5, 1, 0.0), (1.0, 0.5, 1, 0.0), (-1.0, 0.5, 1, 0.0), (15 / 16, 0.5, 0, 1 / 8),
            (-15 / 16, 0.5, 0, 1 / 8), (7.5, -3.5, 1, 0.0), (-7.5, 3.5, 1, 0.0), (0.0, 0.5, 0, 2 / 8)]
    for b, (d, r, dn, qt) in enumerate(pins):
        rew[b], done[b] = r, float(dn)
        q_tn[b, a_star[b]] = qt
        q_s[b, act[b]] = r + (1 - dn) * 0.5 * qt + d
    # a third of the samples inside the quadratic zone: terminal (td = reward), q = reward + k / 8 with |k| <= 7
    for b in range(16, 40):
        done[b] = 1.0
        rew[b] = float(torch.randint(-24, 25, (1,), generator=g)) / 8
        q_s[b, act[b]] = rew[b] + float(torch.randint(-7, 8, (1,), generator=g)) / 8
    for t in (q_s, q_tn, rew):
        assert float((t * 8).frac().abs().max()) == 0 and float(t.abs().max()) <= 4
    return q_s, q_tn, a_star, act, rew, done


def _td_reference(q_s, q_tn, a_star, act, rew, done, gamma, clip):
    """torch CPU float64 smooth_l1_loss and its autograd, cast to fp32 (index guards as the kernel's)."""
    B, N = q_s.shape
    a = a_star.long()
    a = torch.where((a >= 0) & (a < N), a, torch.zeros_like(a))
    qt = q_tn.double().gather(1, a[:, None])
    if clip:
        qt = qt.clamp(min=0)
    td = rew.double()[:, None] + (1 - done.double()[:, None]) * gamma * qt
    q = q_s.double().requires_grad_(True)
    qa = q.gather(1, act.long()[:, None])
    loss = F.smooth_l1_loss(qa, td, reduction="mean")
    loss.backward()
    per = F.smooth_l1_loss(qa, td, reduction="none").detach()[:, 0]
    return q.grad.float(), per.float(), loss.detach().float().reshape(1), (qa - td).detach()[:, 0]


def _td_call(fn, inputs, gamma, clip, kind=None):
    from eco_hip import _lib
    q_s, q_tn, a_star, act, rew, done = (t.cuda() for t in inputs)
    B, N = q_s.shape
    dq = torch.full((B, N), 7.0, device="cuda")
    sq = torch.full((B,), 7.0, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    args = [_lib.ptr(q_s), _lib.ptr(q_tn), _lib.ptr(a_star), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), B, N,
            ctypes.c_float(gamma), int(clip)] + ([] if kind is None else [kind])
    rc = getattr(_lib.lib, fn)(*args, _lib.ptr(dq), _lib.ptr(sq), _lib.ptr(loss), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dq.cpu(), sq.cpu(), loss.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("clip", [0, 1])
def test_td_loss_huber_is_exact(clip):
    from eco_hip import _lib
    inputs = _td_inputs()
    ref_dq, ref_per, ref_loss, d = _td_reference(*inputs, 0.5, clip)
    # both branches, the boundary and the pinned values are present
    assert set([0.0, 1.0, -1.0, 15 / 16, -15 / 16, 7.5, -7.5]) <= set(d.tolist())
    assert 0.25 < float((d.abs() < 1).float().mean()) < 0.75
    rc, dq, sq, loss = _td_call("eco_dqn_td_loss", inputs, 0.5, clip, _lib.ECO_LOSS_HUBER)
    assert rc == _lib.ECO_OK
    assert torch.equal(_bits(dq), _bits(ref_dq))
    assert torch.equal(_bits(sq), _bits(ref_per))
    assert torch.equal(_bits(loss), _bits(ref_loss))


@pytest.mark.parametrize("clip", [0, 1])
def test_td_loss_mse_kind_is_eco_dqn_td_and_bad_kind_is_rejected(clip):
    from eco_hip import _lib
    inputs = _td_inputs()
    rc0, dq0, sq0, loss0 = _td_call("eco_dqn_td", inputs, 0.5, clip)
    rc1, dq1, sq1, loss1 = _td_call("eco_dqn_td_loss", inputs, 0.5, clip, _lib.ECO_LOSS_MSE)
    assert rc0 == rc1 == _lib.ECO_OK
    assert torch.equal(_bits(dq0), _bits(dq1)) and torch.equal(_bits(sq0), _bits(sq1))
    assert torch.equal(_bits(loss0), _bits(loss1))
    assert float(dq0.abs().max()) > 0
    for kind in (2, -1):
        rc, dq, sq, loss = _td_call("eco_dqn_td_loss", inputs, 0.5, clip, kind)
        assert rc == _lib.ECO_ERR_ARG and "loss_kind" in _lib.last_error()
        assert float(dq.min()) == 7.0 and float(sq.min()) == 7.0 and float(loss) == 7.0   # nothing was launched


# ------------------------------------------------------------------ eco_grad_clip
def _clip_call(g, scale, max_norm):
    from eco_hip import _lib
    gd = g.cuda()
    out = torch.full((2,), -3.0, device="cuda")
    rc = _lib.lib.eco_grad_clip(_lib.ptr(gd), gd.numel(), scale, max_norm, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, gd.cpu(), out.cpu()


def _clip_check(g, scale, max_norm):
    """Against float64 numpy on the same fp32 input.  total_norm to 2^-23 relative (the float64 accumulation is
    exact to fp32 rounding; the roundings of the final grad_scale * sqrt follow); elements to 5e-7 relative (coef
    carries at most three fp32 roundings and the product one more: 4 * 2^-24 = 2.4e-7, doubled as the MPNN bars
    are).  Returns (clipped gradient, {norm, coef}, reference coefficient)."""
    from eco_hip import _lib
    g64 = g.numpy().astype(np.float64)
    total = scale * np.sqrt((g64 * g64).sum())
    coef = min(1.0, max_norm / (total + 1e-6))
    rc, got, out = _clip_call(g, scale, max_norm)
    assert rc == _lib.ECO_OK
    assert abs(float(out[0]) - total) <= 2.0 ** -23 * total, (float(out[0]), total)
    assert abs(float(out[1]) - coef) <= 2.0 ** -23 * coef, (float(out[1]), coef)
    ref = g64 * coef
    err = np.abs(got.numpy().astype(np.float64) - ref)
    assert (err <= 5e-7 * np.abs(ref)).all(), float((err / np.maximum(np.abs(ref), 1e-300)).max())
    rc2, got2, out2 = _clip_call(g, scale, max_norm)          # bitwise reproducible run to run
    assert torch.equal(_bits(got), _bits(got2)) and torch.equal(_bits(out), _bits(out2))
    return got, out, coef


# 2,100,152: more than GC_CHUNK * GC_MAX_BLOCKS = 2,097,152 elements, where workgroups take a second chunk
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 58425, 2100152])
def test_grad_clip_matches_float64(n, scale):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.3
    total = scale * float(np.sqrt((g.numpy().astype(np.float64) ** 2).sum()))
    got, out, coef = _clip_check(g, scale, 0.37 * total)       # clips
    assert coef < 0.5 and not torch.equal(got, g)
    got, out, coef = _clip_check(g, scale, 2.0 * total)        # does not clip: coef == 1.0f, grad untouched
    assert coef == 1.0 and float(out[1]) == 1.0
    assert torch.equal(_bits(got), _bits(g))


def test_grad_clip_zero_and_huge_vectors():
    z = torch.zeros(257)
    got, out, coef = _clip_check(z, 1.0, 1.0)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0 and torch.equal(_bits(got), _bits(z))
    h = torch.ones(58425)
    h[12345] = 1e30                                           # its square overflows fp32, not the float64 sum
    got, out, coef = _clip_check(h, 1.0, 1.0)
    assert np.isfinite(float(out[0])) and abs(float(got[12345]) - 1.0) < 1e-6
    got, out, coef = _clip_check(h, 0.5, 1e31)
    assert float(out[1]) == 1.0 and torch.equal(_bits(got), _bits(h))


def test_grad_clip_nonfinite_propagates_as_torch():
    """error_if_nonfinite=False: an infinite norm gives coef 0 (inf * 0 = NaN), a NaN norm makes everything NaN."""
    from eco_hip import _lib
    for bad in (float("inf"), float("nan")):
        g = torch.arange(1, 131, dtype=torch.float32)
        g[7] = bad
        p = torch.nn.Parameter(g.clone())
        p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p], 1.0)
        rc, got, out = _clip_call(g, 1.0, 1.0)
        assert rc == _lib.ECO_OK
        assert torch.equal(torch.isnan(got), torch.isnan(p.grad))
        assert torch.equal(got[~torch.isnan(got)], p.grad[~torch.isnan(p.grad)])


def test_grad_clip_bad_arguments():
    from eco_hip import _lib
    g = torch.ones(64, device="cuda")
    out = torch.full((2,), -3.0, device="cuda")
    call = lambda gp, n, mx, op: _lib.lib.eco_grad_clip(gp, n, 1.0, mx, op, _lib.stream_ptr())   # noqa: E731
    for mx in (0.0, -1.0, float("inf"), float("nan")):
        assert call(_lib.ptr(g), 64, mx, _lib.ptr(out)) == _lib.ECO_ERR_ARG
    assert call(_lib.ptr(g), 0, 1.0, _lib.ptr(out)) == _lib.ECO_ERR_ARG
    assert call(_lib.ptr(g), -5, 1.0, _lib.ptr(out)) == _lib.ECO_ERR_ARG
    assert call(None, 64, 1.0, _lib.ptr(out)) == _lib.ECO_ERR_ARG
    assert call(_lib.ptr(g), 64, 1.0, None) == _lib.ECO_ERR_ARG
    torch.cuda.synchronize()
    assert float(g.min()) == 1.0 and float(out.min()) == -3.0   # nothing was launched
    with pytest.raises(ValueError):
        _lib.check(call(_lib.ptr(g), 64, 0.0, _lib.ptr(out)))


# ------------------------------------------------------------------ agent level
def _learn_agent(timesteps_episodes, **kw):
    from eco_hip.graphs import GraphStore
    n, B = 20, 256
    store = GraphStore.random("ER", 1024, n, 0.15, seed=4)
    agent = _dqn_for(store, n, B=B, replay_start_size=2 * B, train_minibatch=128, update_target_frequency=500, **kw)
    return agent, B * 2 * n * timesteps_episodes


def test_learn_huber_clipped_without_host_sync_and_no_state_leak():
    """A short ER-20 learn() with both options on.  Its steady state -- from the 4th vector step after training is
    ready to the last one, as tests/dist_eval_worker.py brackets it: learn()'s first steps allocate and its end
    reads the loss log back on purpose -- runs under torch's sync-debug mode "error", which raises on any implicit
    host synchronisation.  Around it, two default agents (one run before the clipped agent existed, one after)
    must end with bitwise equal weights: the options leave no state behind in the process."""
    before, t1 = _learn_agent(1)
    before.learn(timesteps=t1)
    assert before.grad_norm is None and before.grad_steps > 0

    agent, t3 = _learn_agent(3, loss="huber", max_grad_norm=1.0)
    steady = {"n": 0, "on": False, "steps": 0}

    def on_step(t):
        if agent._ready:
            steady["n"] += 1
        on = 4 <= steady["n"] and t < t3
        steady["steps"] += on
        if on != steady["on"]:
            torch.cuda.set_sync_debug_mode("error" if on else "default")
            steady["on"] = on
    try:
        agent.learn(timesteps=t3, on_vector_step=on_step)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert steady["steps"] > 50 and agent.grad_steps > 100
    assert torch.isfinite(agent.network.flat).all()
    norm, coef = (float(v) for v in agent.grad_norm.cpu())
    assert np.isfinite(norm) and norm > 0 and 0 < coef <= 1.0

    after, _ = _learn_agent(1)
    after.learn(timesteps=t1)
    assert after.grad_steps == before.grad_steps
    assert torch.equal(_bits(after.network.flat), _bits(before.network.flat))
    assert not torch.equal(after.network.flat, agent.network.flat)


def test_constructor_rejections():
    from eco_hip.graphs import GraphStore
    store = GraphStore.random("ER", 16, 20, 0.15, seed=4)
    with pytest.raises(ValueError, match="loss must be 'huber', 'mse' or a callable"):
        _dqn_for(store, 20, loss="l1")
    with pytest.raises(ValueError, match="loss must be 'huber', 'mse' or a callable"):
        _dqn_for(store, 20, loss=None)
    with pytest.raises(NotImplementedError, match="kernel"):
        _dqn_for(store, 20, loss=F.smooth_l1_loss)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1.0", True, [1.0]):
        with pytest.raises(ValueError, match="max_grad_norm"):
            _dqn_for(store, 20, max_grad_norm=bad)
    for ok in (1, 0.5, np.float32(2.0)):
        agent = _dqn_for(store, 20, loss="huber", max_grad_norm=ok)
        assert agent.max_grad_norm == float(ok) and agent.grad_norm.shape == (2,) and agent.loss == "huber"
    agent = _dqn_for(store, 20)
    assert agent.loss == "mse" and agent.max_grad_norm is None and agent.grad_norm is None
