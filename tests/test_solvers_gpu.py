"""eco_hip.agents.solver (Network, Greedy, Random) on the batched env: free-running Network histories are
self-consistent (every action is the first-index argmax of the recorded Q over allowed vertices) and the CPU
oracles replaying those actions reproduce every other field exactly; Greedy reproduces the reference's
greedy_solver.npz; Random is reproducible under a seeded generator."""
import os

import numpy as np
import pytest
import torch

import solver_history_common as sh
from conftest import GOLDEN
from oracle import graphs as og
from oracle import mpnn_oracle as mo
from oracle import spinsystem_oracle as so

pytestmark = pytest.mark.gpu


def _make(Js, B, T, target="CUT", mode="eco", n_obs_in=7):
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.networks.mpnn import MPNN
    store = GraphStore.from_dense(Js)
    env = VecSpinSystem(store, B, T, **sh.env_kwargs(target, mode, "SIGNED", Js[0].shape[0]))
    env.reset(graph_ids=np.arange(B) % len(Js))   # the reference env's constructor reset
    net = MPNN(n_obs_in=n_obs_in, device="cuda")
    net.load_state_dict(mo.init_weights(torch.Generator().manual_seed(5), std=0.1, n_obs_in=n_obs_in))
    return env, net


def _check_history(solver, Js, T, target, mode, reversible=True):
    h = solver.history
    ln = h.length.cpu().numpy()
    got = {k: getattr(h, k).cpu().numpy() for k in sh.FIELDS}
    total = solver.total_reward.cpu().numpy()
    measure = solver.measure.cpu().numpy()
    for e in range(len(ln)):
        L = int(ln[e])
        acts = got["action"][1:L, e].astype(np.int64)
        for t in range(1, L):
            assert sh.allowed_argmax(got["qs"][t, e], got["spins"][t - 1, e], reversible) == acts[t - 1], (e, t)
        r = sh.replay(Js[e % len(Js)], T, target, mode, "SIGNED", got["spins"][0, e], acts)
        assert len(r["action"]) == L and r["done"][-1], (e, L)
        for k in sh.FIELDS:
            if k != "qs":
                np.testing.assert_array_equal(got[k][:L, e].astype(np.float64), np.asarray(r[k], np.float64),
                                              err_msg=f"episode {e} {k}")
        assert measure[e] == r["solution"][-1]
        assert total[e] == np.cumsum(r["reward"])[-1]   # the same left-to-right float64 sum as solve()
    return ln


@pytest.mark.parametrize("n,start", [(20, "empty"), (20, "full"), (20, "random"), (200, "empty"), (200, "full"),
                                     (200, "random")])
def test_network_free_running(n, start):
    from eco_hip.agents.solver import Network
    rng = np.random.default_rng(n)
    B, T = 4, 2 * n if n == 20 else 30
    Js = [og.er_graph(n, 0.25 if n == 20 else 0.05, rng, "discrete") for _ in range(2)]
    env, net = _make(Js, B, T)
    s = Network(net, env)
    assert Network.epsilon == 0
    s.reset({"empty": -np.ones(n, np.int64), "full": np.ones(n, np.int64)}.get(start))
    s.solve()
    ln = _check_history(s, Js, T, "CUT", "eco")
    assert (ln == T + 1).all()
    if start != "random":
        assert (s.history.spins[0].cpu().numpy() == (-1 if start == "empty" else 1)).all()


def test_network_episodes_of_different_lengths():
    """Irreversible env started with different numbers of -1 spins: an episode ends when its last -1 is flipped,
    its history stops there, and length / measure / total_reward are per episode."""
    from eco_hip.agents.solver import Network
    n, B, T = 20, 4, 40
    rng = np.random.default_rng(8)
    Js = [og.er_graph(n, 0.25, rng, "uniform")]
    env, net = _make(Js, B, T, "MIN_COVER", "s2v", n_obs_in=1)
    spins = -np.ones((B, n), np.int64)
    for e, k in enumerate((0, 5, 12, 17)):
        spins[e, rng.permutation(n)[:k]] = 1
    s = Network(net, env)
    s.reset(spins)
    s.solve()
    ln = _check_history(s, Js, T, "MIN_COVER", "s2v", reversible=False)
    np.testing.assert_array_equal(ln, [21, 16, 9, 4])
    recs = s.history.to_records(3)
    assert len(recs) == 4 and len(recs[0]) == 7


def test_to_records_without_qs():
    from eco_hip.agents.solver import Network
    n, B, T = 20, 2, 6
    rng = np.random.default_rng(9)
    Js = [og.er_graph(n, 0.25, rng, "discrete")]
    env, net = _make(Js, B, T)
    s = Network(net, env)
    s.record_qs = False
    s.reset()
    s.solve()
    recs = s.history.to_records(1)
    assert s.history.qs is None and len(recs) == T + 1
    for r in recs:   # [action, solution, reward, spins, score_mask, valid]
        assert len(r) == 6 and isinstance(r[0], float) and len(r[3]) == n and len(r[4]) == n and isinstance(r[5], bool)
    assert recs[0][0] == 0.0 and recs[0][2] == 0.0


def test_greedy_reproduces_reference():
    from eco_hip.agents.solver import Greedy
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    f = np.load(os.path.join(GOLDEN, "greedy_solver.npz"))
    by_n = {}
    for c in range(int(f["n_cases"])):
        by_n.setdefault(f[f"c{c}_J"].shape[0], []).append(c)
    for n, cases in by_n.items():
        Js = [f[f"c{c}_J"].astype(np.float64) for c in cases]
        B = len(cases)
        env = VecSpinSystem(GraphStore.from_dense(Js), B, 2 * n, **sh.env_kwargs("CUT", "eco", "SIGNED", n))
        env.reset(graph_ids=np.arange(B))
        g = Greedy(env)
        g.reset(np.stack([f[f"c{c}_spins"] for c in cases]).astype(np.int64))
        total = g.solve().cpu().numpy()
        final = env.read(spins=True)["spins"].cpu().numpy()
        for b, c in enumerate(cases):
            s = f[f"c{c}_spins"].astype(np.float64)
            o = so.SpinSystemOracle(Js[b], 2 * n, basin_reward=1. / n)
            o.reset(spins=s.astype(np.int64))
            rew = 0.0
            for a in f[f"c{c}_actions"]:
                s[a] = -s[a]
                rew += o.step(int(a))[1]
            np.testing.assert_array_equal(final[b], s)
            assert float(g.measure[b]) == so.calculate_cut(s, Js[b])
            assert abs(total[b] - rew) <= 1e-12


def test_random_is_reproducible_and_matches_oracle():
    from eco_hip.agents.solver import Random
    n, B, T = 20, 3, 12
    rng = np.random.default_rng(10)
    Js = [og.er_graph(n, 0.25, rng, "uniform")]
    runs = []
    for mode, target in (("eco", "MAX_IND_SET"), ("s2v", "MIN_COVER")):
        for rep in range(2):
            env, _ = _make(Js, B, T, target, mode, n_obs_in=13 if mode == "eco" else 1)
            r = Random(env, generator=torch.Generator(device="cuda").manual_seed(42))
            spins = -np.ones((B, n), np.int64)
            r.reset(spins)
            acts, rews = [], []
            for _ in range(T):
                rew, done = r.step()
                acts.append(r.last_actions.cpu().numpy())
                rews.append(rew.cpu().numpy().copy())
            runs.append(np.array(acts))
            acts, rews = np.array(acts), np.array(rews)
            for e in range(B):
                ref = sh.replay(Js[0], T, target, mode, "SIGNED", spins[e], acts[:, e])
                np.testing.assert_array_equal(rews[:, e], ref["reward"][1:])
                if mode == "s2v":   # drawn among still-flippable vertices: never the same vertex twice
                    assert len(set(acts[:, e])) == T
        np.testing.assert_array_equal(runs[-1], runs[-2])
