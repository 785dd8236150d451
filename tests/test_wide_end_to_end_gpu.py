"""A 13-observable (MAIN_OBSERVABLES) network on a set problem above 512 vertices, end to end: MIN_COVER at
N = 520, the device loop of wide forward + fused greedy act + env.step against CPU oracles, then
experiments.test_network on a 520-vertex graph.

Bars: env rewards and float64 rows equal (==) to the oracle env replaying the device's actions; Q within the
kernel's bar of the MPNN oracle evaluated on the ORACLE env's observation: 5e-5 (1 + |q|) on the shared-graph path
(one graph), 5e-7 on the per-episode kernel (several graphs)."""
import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
from oracle import problems_oracle as po
from wide_common import N_OBS, scaled_err, wide_net

pytestmark = pytest.mark.gpu

N = 520


@pytest.fixture(autouse=True)
def _no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def _env_args():
    from eco_hip.envs.utils import MAIN_OBSERVABLES, ExtraAction, OptimisationTarget, RewardSignal
    return dict(observables=MAIN_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                optimisation_target=OptimisationTarget.MIN_COVER, norm_rewards=True, basin_reward=1. / N,
                reversible_spins=True)


@pytest.mark.parametrize("n_graphs,B,bar", [(1, 5, 5e-5), (3, 3, 5e-7)])
def test_wide_min_cover_rollout_matches_oracles(n_graphs, B, bar):
    from eco_hip import _lib
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.graphs import GraphStore
    rng = np.random.default_rng(520 + n_graphs)
    Js = [og.er_graph(N, 0.02, rng, "uniform") for _ in range(n_graphs)]
    store = GraphStore.from_dense(Js)
    gids = np.arange(B) % n_graphs
    T = 2 * N
    env = VecSpinSystem(store, B, T, want_f64=True, **_env_args())
    assert env.n_obs == N_OBS and env.obs_x.shape[2] == 16
    spins = 2 * rng.integers(0, 2, (B, N)) - 1
    env.reset(graph_ids=gids, spins=spins)
    oracles = []
    for b in range(B):
        o = po.ProblemSpinSystemOracle(Js[gids[b]], T, init_reset=False, target=po.MIN_COVER,
                                       observables=po.MAIN_OBSERVABLES, reward_signal="BLS", basin_reward=1. / N,
                                       reversible_spins=True)
        o.reset(spins=spins[b])
        oracles.append(o)
    w, net, wc = wide_net(52)
    q = torch.empty(B, N, device="cuda")
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    for t in range(8):
        net.forward_graphs(env.obs_x, store, env.graph_ids, norm_scope=_lib.ECO_NORM_PER_GRAPH, q_out=q,
                           act=_lib.ActConfig(0.0, 1, 0.0, 0, 0), actions_out=acts)
        assert torch.equal(acts.long(), q.argmax(1))
        if t in (0, 7):
            for b, o in enumerate(oracles):
                obs = torch.from_numpy(o.get_observation()).float().cuda().unsqueeze(0)
                with torch.no_grad():
                    ref = mo.forward(wc, obs, n_obs_in=N_OBS).reshape(-1)
                assert scaled_err(q[b], ref, f"{n_graphs} graph(s), step {t}, episode {b}") <= bar
        _, rew, _ = env.step(acts)
        env.check_errors()
        rew = rew.cpu().numpy()
        rows = env.obs_f64.cpu().numpy()
        a = acts.cpu().numpy()
        for b, o in enumerate(oracles):
            _, r, _, _ = o.step(int(a[b]))
            assert rew[b] == r, (t, b, rew[b], r)
            np.testing.assert_array_equal(rows[b], o.state_rows(), err_msg=f"step {t} episode {b}")


def test_wide_test_network_on_a_520_vertex_graph():
    from eco_hip import _lib
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.experiments import test_network as run_test_network
    from eco_hip.graphs import GraphStore
    J = og.er_graph(N, 0.02, np.random.default_rng(5200), "uniform")
    _, net, _ = wide_net(53)
    seed, n_attempts = 7, 4
    frame = run_test_network(net, _env_args(), [J], n_attempts=n_attempts, step_factor=0.02, seed=seed)
    assert frame.shape[0] == 1
    # the same attempts, read back independently: test_network draws 2 * randint(2, (attempts, N)) - 1 from
    # RandomState(seed) for its one batch
    spins = 2 * np.random.RandomState(seed).randint(2, size=(n_attempts, N)) - 1
    store = GraphStore.from_dense([J])
    n_steps = int(N * 0.02)
    env = VecSpinSystem(store, n_attempts, n_steps, **_env_args())
    env.reset(graph_ids=np.zeros(n_attempts, dtype=np.int64), spins=spins)
    acts = torch.empty(n_attempts, dtype=torch.int32, device="cuda")
    for _ in range(n_steps):
        net.forward_graphs(env.obs_x, store, env.graph_ids, norm_scope=_lib.ECO_NORM_PER_CALL,
                           act=_lib.ActConfig(0.0, 1, -1.0, 0, 0), actions_out=acts)
        env.step(acts)
    best = env.read()["best_solution"].cpu().numpy()
    print("best_solution per attempt", best, "test_network cut", frame["cut"][0])
    assert frame["cut"][0] == best.max()
    assert frame["mean cut"][0] == float(np.mean(best))
