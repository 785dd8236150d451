"""DQN training above 512 vertices: train_step takes Q(s) from an inference forward and the gradient from
MPNN.grad_large.

  (a) one DQN.train_step at N = 520, minibatch 4, against oracle.mpnn_oracle.train_step (dqn.py:403-451) on the same
      sampled minibatch, as test_parity_bench_sizes_gpu.py does at ER-200, with that file's bars: loss within 1e-4
      relative; dLoss/dparams 2e-4 relative L2 per tensor; new weights within 2 lr (+ 1e-6) and 99 % of them within
      2e-6.  Variants: +-1 ER graphs with the compact replay; float-weighted graphs with the feature ring;
      loss="huber" with max_grad_norm=1.0 (the oracle step restated with smooth_l1_loss and clip_grad_norm_,
      dqn.py:172, :446-447).
  (b) learn() at N = 528 with fresh graphs per episode (regenerate_graphs), a few hundred env-steps.
  (c) one shared +-1 graph at N = 600: train_step with and without the shared-graph inference kernels
      (ECO_PATH_NO_SHARED) gives the same loss and gradient at the oracle bars.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import graphs as og
from oracle import mpnn_oracle as mo

pytestmark = pytest.mark.gpu

LR, GAMMA = 1e-4, 0.95


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _flat_to_dict(flat, n_obs=7):
    from eco_hip.networks.mpnn import param_layout
    out, off = {}, 0
    for name, shape in param_layout(n_obs):
        k = int(np.prod(shape))
        out[name] = flat[off:off + k].reshape(shape)
        off += k
    return out


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def _agent(store, n, B, T=None, **kw):
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    env = VecSpinSystem(store, B, 2 * n if T is None else T, observables=DEFAULT_OBSERVABLES,
                        reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                        optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED, norm_rewards=True,
                        basin_reward=1. / n)
    args = dict(init_weight_std=0.01, double_dqn=True, clip_Q_targets=False, replay_start_size=2 * B,
                replay_buffer_size=B * 8, gamma=GAMMA, update_target_frequency=4000, update_learning_rate=False,
                initial_learning_rate=LR, peak_learning_rate=LR, final_learning_rate=LR, update_frequency=32,
                minibatch_size=64, train_minibatch=B, initial_exploration_rate=1, final_exploration_rate=0.05,
                final_exploration_step=800000, adam_epsilon=1e-8, seed=11, evaluate=False, test_save_path=None)
    args.update(kw)
    return DQN(env, lambda: MPNN(device="cuda"), **args)


def _dense(store, gid):
    """float32 [k, N, N] adjacency of graphs gid (the network takes obs.float(), dqn.py:282)."""
    return torch.from_numpy(np.stack([store.dense(int(g)) for g in gid.cpu()])).float().cuda()


def _obs(x, adj, n_obs=7):
    return torch.cat([x[:, :, :n_obs].transpose(1, 2), adj], dim=1)


def _oracle_step(w, tw, tr, store, loss="mse", max_grad_norm=None):
    """(new weights, loss, gradient after clipping, total norm before clipping) of dqn.py:403-451 on minibatch tr.
    loss="mse" without clipping is oracle.mpnn_oracle.train_step itself."""
    xs, act, rew, xn, done, gid = tr
    adj = _dense(store, gid)
    s, sn = _obs(xs, adj), _obs(xn, adj)
    a, r, d = act.long().unsqueeze(1), rew.unsqueeze(1), done.unsqueeze(1)
    if loss == "mse" and max_grad_norm is None:
        st = {"step": 0, "m": {}, "v": {}}
        w1, l = mo.train_step(w, st, s, a, r, sn, d, gamma=GAMMA, lr=LR, eps=1e-8, target_w=tw)
        return w1, l, st["grad"], None
    with torch.no_grad():
        a_star = mo.forward(w, sn).reshape(sn.shape[0], -1).argmax(1, True)
        td = r + (1 - d) * GAMMA * mo.forward(tw, sn).reshape(sn.shape[0], -1).gather(1, a_star)
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    q = mo.forward(wg, s).reshape(s.shape[0], -1).gather(1, a)
    l = F.smooth_l1_loss(q, td) if loss == "huber" else F.mse_loss(q, td)
    l.backward()
    norm = None
    if max_grad_norm is not None:
        norm = float(torch.nn.utils.clip_grad_norm_([wg[k] for k in mo.KEYS], max_grad_norm))
    grads = {k: wg[k].grad.detach().clone() for k in mo.KEYS}
    w1 = {}
    for k in mo.KEYS:                                   # Adam's first step (bias-corrected, eps added to sqrt(v_hat))
        g = grads[k]
        m, v = 0.1 * g, 0.001 * g * g
        w1[k] = w[k] - (LR / 0.1) * m / ((v.sqrt() / (0.001 ** 0.5)) + 1e-8)
    return w1, float(l.detach()), grads, norm


def _filled_agent(store, n, B, steps=3, **kw):
    """An agent whose replay holds `steps` vector steps of random-policy transitions, target != online."""
    agent = _agent(store, n, B, **kw)
    with torch.no_grad():
        agent.target_network.flat.add_(torch.randn(agent.target_network.flat.shape, device="cuda",
                                                   generator=torch.Generator(device="cuda").manual_seed(1)) * 0.01)
    agent.start()
    for _ in range(steps):
        agent.vector_step(False)
    return agent


def _check_step(agent, store, loss="mse", max_grad_norm=None):
    tr = [t.clone() for t in agent.replay_buffer.sample(agent.M)]
    w = _flat_to_dict(agent.network.flat.clone())
    tw = _flat_to_dict(agent.target_network.flat.clone())
    got_loss = agent.train_step(tr)
    grad = _flat_to_dict(agent.grad.clone())
    w1 = _flat_to_dict(agent.network.flat.clone())
    agent.env.check_errors()
    ref_w1, ref_loss, ref_grad, ref_norm = _oracle_step(w, tw, tr, store, loss, max_grad_norm)
    print(f"loss {got_loss!r} oracle {ref_loss!r}; grad rel L2 " +
          ", ".join(f"{_rel(grad[k], ref_grad[k]):.2e}" for k in mo.KEYS))
    assert abs(got_loss - ref_loss) <= 1e-4 * abs(ref_loss), (got_loss, ref_loss)
    for k in mo.KEYS:
        assert _rel(grad[k], ref_grad[k]) < 2e-4, k
        d = (w1[k] - ref_w1[k]).abs()
        assert float(d.max()) <= 2 * LR + 1e-6, k
        assert float((d > 2e-6).float().mean()) <= 0.01, k
    if max_grad_norm is not None:
        norm, coef = (float(v) for v in agent.grad_norm.cpu())
        print(f"gradient norm {norm!r} oracle {ref_norm!r}, clip coefficient {coef!r}")
        assert abs(norm - ref_norm) <= 2e-4 * ref_norm
        assert abs(coef - min(1.0, max_grad_norm / (ref_norm + 1e-6))) <= 2e-4
    return got_loss, agent.grad.clone()


def test_train_step_n520_pm1_compact_replay_matches_oracle():
    from eco_hip.graphs import GraphStore
    n, M = 520, 4
    store = GraphStore.random("ER", M, n, 0.02, seed=52)
    agent = _filled_agent(store, n, M)
    assert agent.compact_replay and agent._large and agent.saved is None
    _check_step(agent, store)


def test_train_step_n520_float_weights_feature_ring_matches_oracle():
    from eco_hip.graphs import GraphStore
    n, M = 520, 4
    store = GraphStore.random("ER", M, n, 0.02, seed=53, weights="random")
    agent = _filled_agent(store, n, M)
    assert store.float_weights and not agent.compact_replay
    _check_step(agent, store)


def test_train_step_n520_huber_clipped_matches_oracle():
    from eco_hip.graphs import GraphStore
    n, M = 520, 4
    store = GraphStore.random("ER", M, n, 0.02, seed=54)
    # weights of std 0.3: TD errors beyond the quadratic zone of the Huber loss and a gradient norm above 1, so
    # both options act on this step (at std 0.01 the norm is 0.014 and nothing is clipped)
    agent = _filled_agent(store, n, M, loss="huber", max_grad_norm=1.0, init_weight_std=0.3)
    _check_step(agent, store, loss="huber", max_grad_norm=1.0)
    assert float(agent.grad_norm[0]) > 1.0 and float(agent.grad_norm[1]) < 1.0


def test_learn_n528_regenerated_graphs(tmp_path):
    from eco_hip.graphs import GraphStore, edge_cap
    from eco_hip.agents.dqn.dqn import graph_slots_needed
    from eco_hip.agents.dqn.utils import TestMetric
    n, B, T = 528, 8, 16
    C = B * T
    st = GraphStore.slots(graph_slots_needed(B, T, C), n, edge_cap("ER", n, 0.02))
    agent = _agent(st, n, B, T=T, replay_buffer_size=C, replay_start_size=2 * B, regenerate_graphs=("ER", 0.02),
                   evaluate=True, test_envs=None, test_episodes=4, test_frequency=B * 20,
                   test_metric=TestMetric.BEST, save_network_frequency=B * 100000, network_save_path=str(tmp_path / "network.pth"))
    w0 = agent.network.flat.clone()
    agent.learn(timesteps=B * T * 3)                   # 384 env-steps: three episode batches
    agent.env.check_errors()
    losses = agent.losses()
    assert len(losses) >= 40 and all(np.isfinite(l) for _, l in losses)
    assert agent.grad_steps == len(losses)
    assert torch.isfinite(agent.network.flat).all() and not torch.equal(agent.network.flat, w0)
    assert agent.graphs_regenerated >= B
    assert agent.evaluations_run >= 1 and len(agent.test_scores) >= 1


def test_train_step_n600_shared_graph_with_and_without_shared_kernels():
    """n_graphs == 1 with +-1 weights: Q(s) and the double-DQN pair run the shared-graph inference kernels; with
    ECO_PATH_NO_SHARED they run the per-episode kernel.  Both train steps match the oracle, the gradients each other
    at the same bar."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, M = 600, 4
    J = og.er_graph(n, 0.02, np.random.default_rng(600), weights="discrete")
    out = []
    for mask in (0, _lib.ECO_PATH_NO_SHARED):
        store = GraphStore.from_dense([J])
        assert store.n_graphs == 1 and store.unit_weights
        with _lib.kernel_paths(mask):
            route = _lib.lib.eco_mpnn_route(ctypes.byref(store.gs), 7, M, 0, 0, 0)
            assert route == (_lib.ECO_ROUTE_LARGE if mask else _lib.ECO_ROUTE_SHARED)
            agent = _filled_agent(store, n, M)
            out.append(_check_step(agent, store))
    (l0, g0), (l1, g1) = out
    assert abs(l0 - l1) <= 1e-4 * abs(l1)
    d0, d1 = _flat_to_dict(g0), _flat_to_dict(g1)
    for k in mo.KEYS:
        assert _rel(d0[k], d1[k]) < 2e-4, k
