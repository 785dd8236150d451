"""DQN training on 2049 to 8192 vertices (DQN(..., train_large_graphs=True)): Q(s') from two forwards of
eco_mpnn_forward_wg, Q(s) from a third that reuses the online network's per-call max degree, the gradient from
MPNN.grad_wg.  Small shapes throughout: B = M = 2 episodes, T = 8, a few pushed vector steps.

The train-step comparisons are tests/test_large_train_gpu.py::_check_step on the same sampled minibatch against
oracle.mpnn_oracle.train_step (dqn.py:403-451), with that file's bars: loss within 1e-4 relative; dLoss/dparams 2e-4
relative L2 per tensor; new weights within 2 lr (+ 1e-6) and 99 % of them within 2e-6; with clipping the norm within
2e-4 relative and the coefficient within 2e-4.
"""
import numpy as np
import pytest
import torch

import test_large_train_gpu as lt

pytestmark = pytest.mark.gpu

T = 8


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _pm1_store(n, graphs=2, seed=0):
    from eco_hip.graphs import GraphStore
    return GraphStore.random("ER", graphs, n, 8.0 / n, seed=seed)


def _int_store(n, seed):
    from eco_hip.graphs import GraphStore
    mats = []
    for b in range(2):
        rng = np.random.default_rng(seed + b)
        a = np.triu((rng.random((n, n)) < 8.0 / n) * rng.choice([-3.0, -2.0, 1.0, 2.0], (n, n)), 1)
        mats.append(a + a.T)
    return GraphStore.from_dense(mats)


def test_keyword_opts_in_and_outer_bounds_stay():
    from eco_hip.graphs import GraphStore
    n = 2049
    store = _pm1_store(n, seed=1)
    with pytest.raises(ValueError, match="at most ECO_MAX_SPINS=2048"):
        lt._agent(store, n, 2, T=T)
    with pytest.raises(ValueError, match="at most ECO_MAX_SPINS=2048"):
        lt._agent(store, n, 2, T=T, train_large_graphs=False)
    agent = lt._agent(store, n, 2, T=T, train_large_graphs=True)
    assert agent._wg and agent._large and agent.saved is None and agent.compact_replay
    assert agent.grad_ws.numel() == agent.network.grad_wg_bytes(n, 2) > 0
    # the keyword lifts nothing else: the store's own limits, and regenerate_graphs above 2048
    with pytest.raises(ValueError, match="exceeds ECO_MAX_SPINS_WG=8192"):
        GraphStore.from_edges(8193, [0], [1], [1])
    with pytest.raises(ValueError, match="integer weights only"):
        GraphStore.from_edges(2049, [0], [1], [0.5])
    with pytest.raises(ValueError, match="regenerate_graphs takes graphs of at most ECO_MAX_SPINS=2048"):
        lt._agent(store, n, 2, T=T, train_large_graphs=True, regenerate_graphs=("ER", 8.0 / n))
    # and it changes nothing at a size that trains without it
    small = _pm1_store(600, seed=2)
    a600 = lt._agent(small, 600, 2, T=T, train_large_graphs=True)
    assert a600._large and not a600._wg
    # a minibatch beyond the gradient's 32-bit row index names the bound on train_minibatch
    with pytest.raises(ValueError, match=r"train_minibatch <= 16376"):
        agent._alloc_train_buffers((2 ** 31 - 1) // 64 // n + 1)
    assert agent._train_m == 2 and agent.q_s.shape == (2, n)       # rejected before anything was reallocated


def test_train_step_n2049_pm1_compact_replay_matches_oracle():
    n, M = 2049, 2
    store = _pm1_store(n, seed=3)
    agent = lt._filled_agent(store, n, M, T=T, train_large_graphs=True)
    assert agent.compact_replay and agent._wg
    lt._check_step(agent, store)


def test_train_step_n2100_integer_weights_feature_ring_huber_clipped_matches_oracle():
    """Integer weights beyond +-1: the fp32 feature ring.  Weights of std 0.3 as in the N = 520 test of
    test_large_train_gpu.py (TD errors beyond the quadratic zone of the Huber loss); max_grad_norm = 0.1 lies below
    the gradient norm of this step, printed by _check_step, so the clip acts."""
    n, M = 2100, 2
    store = _int_store(n, seed=2100)
    assert not store.unit_weights and not store.float_weights
    agent = lt._filled_agent(store, n, M, T=T, train_large_graphs=True, loss="huber", max_grad_norm=0.1,
                             init_weight_std=0.3)
    assert not agent.compact_replay and agent._wg
    lt._check_step(agent, store, loss="huber", max_grad_norm=0.1)
    assert float(agent.grad_norm[0]) > 0.1 and float(agent.grad_norm[1]) < 1.0


def test_double_dqn_on_and_off_reuse_the_online_max_degree():
    """Q(s) of train_step runs with ECO_NORM_PER_CALL_REUSE on the online network's workspace: it must equal, bit for
    bit, a fresh ECO_NORM_PER_CALL forward of the same weights -- with the header of that workspace poisoned before
    the step, so a step that reused a value the online forward on s' did not write there would show.  Graphs of
    different max degree; the target network differs from the online one."""
    from eco_hip import _lib
    n, M = 2049, 2
    store = _pm1_store(n, graphs=2, seed=5)
    agent = lt._filled_agent(store, n, M, T=T, train_large_graphs=True)
    net, tgt = agent.network, agent.target_network
    for double in (True, False):
        agent.double_dqn = double
        xs, act, rew, xn, done, gid = [t.clone() for t in agent.replay_buffer.sample(M)]
        q_s = net.forward_graphs(xs, store, gid, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
        q_on = net.forward_graphs(xn, store, gid, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
        q_tn = tgt.forward_graphs(xn, store, gid, norm_scope=_lib.ECO_NORM_PER_CALL).clone()
        torch.cuda.synchronize()
        net._ws[:4].view(torch.int32).fill_(12345)          # the per-call max degree slot of the online workspace
        loss = agent.train_step((xs, act, rew, xn, done, gid))
        assert np.isfinite(loss), double
        assert torch.equal(agent.q_s.view(torch.int32), q_s.view(torch.int32)), double
        assert torch.equal(agent.q_tn.view(torch.int32), q_tn.view(torch.int32)), double
        assert torch.equal(agent.a_star.long(), (q_on if double else q_tn).argmax(1)), double
        assert torch.isfinite(agent.grad).all() and float(agent.grad.abs().max()) > 0
    agent.env.check_errors()


def test_prioritised_replay_step():
    n, M = 2049, 2
    store = _pm1_store(n, seed=6)
    agent = lt._filled_agent(store, n, M, T=T, train_large_graphs=True, prioritised_replay={})
    assert agent._prio is not None and agent._wg
    tr = agent.replay_buffer.sample(M)
    before = agent._prio.mass.clone()
    w0 = agent.network.flat.clone()
    loss = agent.train_step(tr)
    assert np.isfinite(loss)
    idx = agent._prio.last_idx.long()
    assert not torch.equal(agent._prio.mass[idx], before[idx])      # the sampled positions took their |td| priorities
    assert torch.isfinite(agent.network.flat).all() and not torch.equal(agent.network.flat, w0)
    agent.env.check_errors()


def test_learn_n2060(tmp_path):
    from eco_hip.agents.dqn.utils import TestMetric
    n, B = 2060, 2
    store = _pm1_store(n, graphs=4, seed=7)
    agent = lt._agent(store, n, B, T=T, train_large_graphs=True, replay_buffer_size=B * T * 2, replay_start_size=2 * B,
                      update_target_frequency=32 * 10, evaluate=True, test_envs=None, test_episodes=2,
                      test_frequency=B * 20, test_metric=TestMetric.BEST, save_network_frequency=B * 100000,
                      network_save_path=str(tmp_path / "network.pth"))
    syncs = []
    sync = agent.sync_target
    agent.sync_target = lambda: (syncs.append(agent.grad_steps), sync())
    w0 = agent.network.flat.clone()
    t0 = agent.target_network.flat.clone()
    agent.learn(timesteps=B * T * 16)                  # 256 env-steps: sixteen episode batches
    agent.env.check_errors()
    store.check_errors()
    losses = agent.losses()
    assert len(losses) >= 40 and all(np.isfinite(l) for _, l in losses)
    assert agent.grad_steps == len(losses)
    assert torch.isfinite(agent.network.flat).all() and not torch.equal(agent.network.flat, w0)
    assert len(syncs) >= 1 and not torch.equal(agent.target_network.flat, t0)
    assert agent.evaluations_run >= 1 and len(agent.test_scores) >= 1
    assert all(np.isfinite(s) for _, s in agent.test_scores)
