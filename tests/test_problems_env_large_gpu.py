"""Generic-scorer env kernels (csrc/eco_env_problems.hip) above 512 vertices: N = 528 (9 vertices per lane) and
N = 2048 (the largest template width of ECO_DISPATCH_VPT), every set problem and MIN_CUT, against
oracle/problems_oracle.py.

Bar: rewards, dones, float64 observation rows, scores and greedy actions equal (==) to the oracle's, as
tests/test_problems_gpu.py::test_problem_env_batched_vs_oracle."""
import zlib

import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import problems_oracle as po

pytestmark = pytest.mark.gpu

TARGETS = ["MIN_COVER", "MAX_IND_SET", "MAX_CLIQUE", "MIN_DOM_SET", "MIN_CUT"]


def _env_args(target_name, n):
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, MAIN_OBSERVABLES, ExtraAction, OptimisationTarget,
                                    RewardSignal)
    obs = DEFAULT_OBSERVABLES if target_name == "MIN_CUT" else MAIN_OBSERVABLES
    return dict(observables=obs, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                optimisation_target=OptimisationTarget[target_name], norm_rewards=True, basin_reward=1. / n,
                reversible_spins=True)


def _oracle_kwargs(target_name, n):
    obs = po.DEFAULT_OBSERVABLES if target_name == "MIN_CUT" else po.MAIN_OBSERVABLES
    return dict(target=getattr(po, target_name), observables=obs, reward_signal="BLS", basin_reward=1. / n,
                reversible_spins=True)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("n,p", [(528, 0.02), (2048, 0.004)])
def test_problem_env_above_512_vs_oracle(target, n, p):
    """B = 4 episodes on 2 graphs: 6 random steps, then 4 greedy steps, every step against the oracle."""
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.graphs import GraphStore
    rng = np.random.default_rng(zlib.crc32(f"{target}/{n}".encode()))
    w = "discrete" if target == "MIN_CUT" else "uniform"
    Js = [og.er_graph(n, p, rng, w) for _ in range(2)]
    B, T = 4, 2 * n
    gids = np.array([b % 2 for b in range(B)])
    vec = VecSpinSystem(GraphStore.from_dense(Js), B, T, want_f64=True, **_env_args(target, n))
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    vec.reset(graph_ids=gids, spins=spins)
    vec.check_errors()
    envs = []
    for b in range(B):
        e = po.ProblemSpinSystemOracle(Js[gids[b]], T, init_reset=False, **_oracle_kwargs(target, n))
        e.reset(spins=spins[b])
        envs.append(e)
    np.testing.assert_array_equal(vec.obs_f64.cpu().numpy(), np.stack([e.state_rows() for e in envs]))
    done = np.zeros(B, bool)
    for t in range(10):
        if t < 6:
            acts = rng.integers(0, n, B)
            a_dev = torch.tensor(acts, dtype=torch.int32, device="cuda")
        else:
            a_dev = vec.greedy_actions()
            acts = a_dev.cpu().numpy()
            gacts = [po.greedy_action(e) if not d else None for e, d in zip(envs, done)]
            greedy_stop = np.array([g is None for g in gacts]) & ~done
            for b in range(B):
                if not done[b] and gacts[b] is not None:
                    assert acts[b] == gacts[b], (target, n, b, t, acts[b], gacts[b])
            st = vec.read()
            assert np.array_equal(st["done"].cpu().numpy().astype(bool), done | greedy_stop)
            done |= greedy_stop
        _, rew, dn = vec.step(a_dev)
        vec.check_errors()
        rew, dn = rew.cpu().numpy(), dn.cpu().numpy().astype(bool)
        rows = vec.obs_f64.cpu().numpy()
        for b, e in enumerate(envs):
            if done[b]:
                assert rew[b] == 0.0 and dn[b]
                continue
            _, r, d, _ = e.step(int(acts[b]))
            assert rew[b] == r, (target, n, b, t, rew[b], r)
            assert dn[b] == d
            np.testing.assert_array_equal(rows[b], e.state_rows(), err_msg=f"{target} N={n} b={b} t={t}")
            done[b] |= d
        if done.all():
            break
    st = vec.read()
    for b, e in enumerate(envs):
        assert st["score"][b].item() == e.score and st["normalized_score"][b].item() == e.normalized_score
        assert st["best_score"][b].item() == e.best_score and st["best_solution"][b].item() == e.best_solution
