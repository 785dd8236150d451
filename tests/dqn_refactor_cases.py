"""Whole-agent learn() runs shared by tests/golden/make_dqn_learn_parent.py (which recorded
tests/golden/dqn_learn_parent.npz on an MI355X from the commit before the DQN class was split) and
tests/test_dqn_refactor_parity_gpu.py (which reruns them and compares exactly).

Every case is learn(timesteps=B * 41) at N = 20, B = 64, M = 64, evaluating every 10 vector steps.
The two parameter vectors of a case (final network.flat, the `_best` state dict) are recorded as the
SHA-256 of their bytes: an exact comparison needs no more, and the vectors themselves (234 KB each,
incompressible) would not fit a committed file."""
import hashlib
import os

import numpy as np
import torch

from test_dqn_gpu import _dqn_for, _s2v_dqn, _s2v_env

N, B = 20, 64
T = 2 * N
# test_dqn_gpu._dqn_for's agent settings
DQN_ARGS = dict(init_weight_std=0.01, double_dqn=True, clip_Q_targets=False, replay_buffer_size=4096, gamma=0.95,
                update_target_frequency=1000, update_learning_rate=False, initial_learning_rate=1e-4,
                peak_learning_rate=1e-4, final_learning_rate=1e-4, update_frequency=32, minibatch_size=64,
                final_exploration_rate=0.05, final_exploration_step=150000, adam_epsilon=1e-8, seed=3)
# recorded cases; "mse_explicit" (build() below) is "eco_best" with loss="mse" passed explicitly and is compared
# with that case's entry
CASES = ("eco_best", "stagger_regen", "s2v_final", "cum_reward", "huber_clip_samples", "early_masked")


def _learn_args(tmp, **kw):
    args = dict(replay_start_size=2 * B, train_minibatch=64, evaluate=True, test_episodes=8, test_frequency=B * 10,
                save_network_frequency=B * 20, network_save_path=os.path.join(tmp, "network.pth"),
                test_save_path=os.path.join(tmp, "test_scores.pkl"))
    args.update(kw)
    return args


def _eco(tmp, stopping=None, **kw):
    """The configuration of test_learn_evaluates_saves_and_pickles: lockstep episodes, compact replay, a
    separate test env, overlapped one-fill evaluations (eager, then captured, then replayed)."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis, Stopping)
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    from eco_hip.agents.dqn.utils import TestMetric
    env_args = dict(observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                    optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED, norm_rewards=True,
                    basin_reward=1. / N, stopping=stopping or Stopping.NORMAL)
    env = VecSpinSystem(GraphStore.random("ER", 256, N, 0.15, seed=4), B, T, **env_args)
    test_env = VecSpinSystem(GraphStore.random("ER", 8, N, 0.15, seed=5), 8, T, **env_args)
    args = dict(DQN_ARGS, test_envs=test_env, test_metric=TestMetric.BEST)
    args.update(_learn_args(tmp, **kw))
    return DQN(env, lambda: MPNN(device="cuda"), **args)


def build(name, tmp):
    from eco_hip.graphs import GraphStore, edge_cap
    from eco_hip.agents.dqn.dqn import graph_slots_needed
    from eco_hip.agents.dqn.utils import TestMetric
    if name == "eco_best":
        return _eco(tmp)
    if name == "mse_explicit":
        return _eco(tmp, loss="mse")
    if name == "cum_reward":
        return _eco(tmp, test_metric=TestMetric.CUMULATIVE_REWARD)
    if name == "huber_clip_samples":
        return _eco(tmp, loss="huber", max_grad_norm=1.0, double_dqn=False, target_sync="samples")
    if name == "early_masked":
        # Stopping.EARLY: episodes end at different steps (masked resets from the device dones onto pool
        # graphs), and the evaluation takes the refill loop
        from eco_hip.envs.utils import Stopping
        return _eco(tmp, stopping=Stopping.EARLY, graph_pool_ids=np.arange(100, 228))
    if name == "stagger_regen":
        # staggered episodes on regenerated graph slots, a store of exactly the needed size; the evaluation
        # reads the training store, so it runs synchronously
        st = GraphStore.slots(graph_slots_needed(B, T, 4096), N, edge_cap("ER", N, 0.15))
        agent = _dqn_for(st, N, B=B, **_learn_args(tmp, regenerate_graphs=("ER", 0.15), test_envs=None,
                                                   test_metric=TestMetric.BEST))
        agent.stagger_episodes = True
        return agent
    if name == "s2v_final":
        # irreversible spins: dones read back from the device, feature replay, FINAL metric, and more test
        # episodes than test slots (the refill loop)
        env = _s2v_env(GraphStore.random("ER", 256, N, 0.15, seed=9), N, B, T=T)
        test_env = _s2v_env(GraphStore.random("ER", 8, N, 0.15, seed=5), N, 4, T=T)
        return _s2v_dqn(env, compact_replay=False, **_learn_args(tmp, test_envs=test_env, test_episodes=6,
                                                                 test_metric=TestMetric.FINAL))
    raise KeyError(name)


def _digest(data):
    return np.frombuffer(hashlib.sha256(data).digest(), np.uint8).copy()


def run_case(name, tmp):
    """learn(B * 41) of case `name`, files under `tmp`; returns the recorded fields as arrays."""
    agent = build(name, str(tmp))
    agent.learn(timesteps=B * 41)
    agent.env.check_errors()
    last_scores, last_solutions = agent.last_evaluation
    flat = agent.network.flat.cpu().numpy()
    best = torch.load(os.path.join(str(tmp), "network_best.pth"), map_location="cpu", weights_only=True)
    best_bytes = b"".join(k.encode() + v.contiguous().numpy().tobytes() for k, v in best.items())
    return {
        "losses": np.array(agent.losses(), np.float64).reshape(-1, 2),
        "test_scores": np.array(agent.test_scores, np.float64),
        "test_solutions": np.array(agent.test_solutions, np.float64),
        "last_scores": np.array(last_scores, np.float64),
        "last_solutions": np.array(last_solutions, np.float64),
        "flat_sha256": _digest(flat.tobytes()),
        "flat_sum": np.array([flat.astype(np.float64).sum(), np.abs(flat.astype(np.float64)).sum()]),
        "best_sha256": _digest(best_bytes),
        "schedules": np.array([agent.epsilon, agent.lr], np.float64),
        "counters": np.array([agent.grad_steps, getattr(agent, "graphs_regenerated", 0),
                              getattr(agent, "graphs_reused", 0)], np.int64),
    }
