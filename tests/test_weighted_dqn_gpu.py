"""DQN training on float-weighted graphs (EdgeType.RANDOM): train_step against the torch oracle at the bars of
tests/test_dqn_gpu.py's three-step test, the replay ring that is selected, and a short learn() with per-episode
on-device graph regeneration."""
import numpy as np
import pytest
import torch

from oracle import mpnn_oracle as mo
from oracle import spinsystem_oracle as so

pytestmark = pytest.mark.gpu


def _graph(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = rng.uniform(-1.0, 1.0, int(keep.sum()))
    return m + m.T


def _dqn_for(store, n, B=16, **kw):
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget, SpinBasis)
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    env = VecSpinSystem(store, B, 2 * n, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                        extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                        spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n)
    args = dict(init_weight_std=0.01, double_dqn=True, clip_Q_targets=False, replay_start_size=500,
                replay_buffer_size=4096, gamma=0.95, update_target_frequency=1000, update_learning_rate=False,
                initial_learning_rate=1e-4, peak_learning_rate=1e-4, final_learning_rate=1e-4,
                update_frequency=32, minibatch_size=64, final_exploration_rate=0.05, final_exploration_step=150000,
                adam_epsilon=1e-8, seed=3, evaluate=False, test_save_path=None)
    args.update(kw)
    return DQN(env, lambda: MPNN(device="cuda"), **args)


def _split(obs):
    obs = np.asarray(obs)
    x = np.zeros((obs.shape[0], obs.shape[2], 8), np.float32)
    x[:, :, :7] = obs[:, :7, :].transpose(0, 2, 1).astype(np.float32)
    return torch.from_numpy(x).cuda()


def test_train_step_matches_oracle_three_steps():
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import param_layout
    n, M, steps = 20, 16, 3
    rng = np.random.default_rng(0)
    Js = [_graph(n, 0.3, 50 + k) for k in range(steps * M)]
    store = GraphStore.from_dense(Js)
    assert store.float_weights
    agent = _dqn_for(store, n, B=M, minibatch_size=M)
    from eco_hip.agents.dqn.utils import ReplayBuffer
    assert not agent.compact_replay and isinstance(agent.replay_buffer, ReplayBuffer)
    w = mo.init_weights(torch.Generator().manual_seed(1), std=0.1)
    tw = mo.init_weights(torch.Generator().manual_seed(2), std=0.1)
    agent.network.load_state_dict(w)
    agent.target_network.load_state_dict(tw)
    adam = dict(step=0, m={}, v={})
    for s in range(steps):
        S, Sn, A, R, D = [], [], [], [], []
        for k in range(M):
            o = so.SpinSystemOracle(Js[s * M + k], 2 * n, basin_reward=1. / n)
            o.reset(spins=2 * rng.integers(0, 2, n) - 1)
            for _ in range(int(rng.integers(0, 5))):
                o.step(int(rng.integers(0, n)))
            S.append(o.get_observation())
            a = int(rng.integers(0, n))
            obs, r, d, _ = o.step(a)
            Sn.append(obs); A.append(a); R.append(r); D.append(float(d or k == 0))
        S, Sn = np.stack(S), np.stack(Sn)
        st, stn = torch.from_numpy(S).float(), torch.from_numpy(Sn).float()
        act = torch.tensor(A).long()[:, None]
        rew = torch.tensor(R, dtype=torch.float32)[:, None]
        done = torch.tensor(D, dtype=torch.float32)[:, None]
        w, ref_loss = mo.train_step(w, adam, st, act, rew, stn, done, gamma=0.95, lr=1e-4, eps=1e-8, target_w=tw)
        gid = torch.arange(s * M, (s + 1) * M, dtype=torch.int32, device="cuda")
        loss = agent.train_step((_split(S), act[:, 0].int().cuda(), rew[:, 0].cuda(), _split(Sn), done[:, 0].cuda(),
                                 gid))
        print(f"step {s}: loss {loss:.9g} oracle {ref_loss:.9g}")
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (s, loss, ref_loss)
        flat, off = agent.network.flat.cpu(), 0
        for name, shape in param_layout(7):
            k = int(np.prod(shape))
            np.testing.assert_allclose(flat[off:off + k].reshape(shape).numpy(), w[name].numpy(), rtol=0, atol=2e-6,
                                       err_msg=f"step {s} {name}")
            off += k


def test_feature_ring_is_selected_and_compact_ring_refused():
    from eco_hip.graphs import GraphStore
    from eco_hip.agents.dqn.utils import ReplayBuffer
    n = 20
    store = GraphStore.from_dense([_graph(n, 0.3, s) for s in range(8)])
    agent = _dqn_for(store, n, B=8)
    assert agent.compact_replay is False and isinstance(agent.replay_buffer, ReplayBuffer)
    with pytest.raises(ValueError, match="compact replay"):
        _dqn_for(store, n, B=8, compact_replay=True)


def test_learn_2000_env_steps_with_per_episode_regeneration():
    from eco_hip.graphs import GraphStore
    from eco_hip.agents.dqn.dqn import graph_slots_needed
    n, B = 20, 50
    T = 2 * n                                   # 2,000 env steps = one episode batch
    C = 1024
    need = graph_slots_needed(B, T, C)
    st = GraphStore.generated("ER", need, n, 0.15, seed=5, weights="random")
    agent = _dqn_for(st, n, B=B, replay_buffer_size=C, replay_start_size=4 * B, train_minibatch=64,
                     regenerate_graphs=("ER", 0.15))
    w0 = agent.network.flat.clone()
    e0 = st.edge_weights.clone()
    losses = agent.learn(timesteps=2000)
    agent.env.check_errors()
    assert agent.grad_steps > 0 and len(losses) > 0 and all(np.isfinite(l) for _, l in losses)
    assert torch.isfinite(agent.network.flat).all() and not torch.equal(w0, agent.network.flat)
    assert agent.graphs_regenerated >= B and not torch.equal(e0, st.edge_weights)
    assert st.float_weights and bool((st.valid[agent.env.graph_ids.long()] == 1).all())
