"""Random-regular (ECO_GRAPH_REGULAR) and ring-lattice (ECO_GRAPH_WS) graphs generated on the device: structure,
determinism, distribution (pair marginals; the two-triangle fraction against the host restatement of the same
pairing algorithm), weights, the host argument checks, and that the graphs drive the env and the training loop."""
import numpy as np
import pytest
import torch

from oracle import spinsystem_oracle as so

pytestmark = pytest.mark.gpu


def _adjacency(store):
    """[G, n, n] float64 weights (signs for a float store) of every graph, checking on the way that every row is
    sorted by column without duplicates; one device read for the whole store."""
    G, n = store.n_graphs, store.n_spins
    rp = store.row_ptr.cpu().numpy().astype(np.int64)
    eb = store.edge_base.cpu().numpy()
    ed = store.edges.cpu().numpy().view(np.uint32)
    A = np.zeros((G, n, n))
    for g in range(G):
        e = ed[eb[g]:eb[g] + rp[g, -1]]
        cols = (e & 0xFFFFFF).astype(np.int64)
        rows = np.repeat(np.arange(n), np.diff(rp[g]))
        step = np.diff(cols)
        assert np.all(step[np.diff(rows) == 0] > 0), g
        assert cols.size == 0 or cols.max() < n
        A[g, rows, cols] = (e >> 24).astype(np.uint8).view(np.int8)
    return A


def _ring(n, k):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    dist = np.minimum(np.abs(i - j), n - np.abs(i - j))
    return ((dist >= 1) & (dist <= k // 2)).astype(float)


@pytest.mark.parametrize("n,d,G", [(20, 3, 512), (9, 4, 512), (65, 6, 64), (600, 3, 4)])
def test_regular_structure_and_determinism(n, d, G):
    from eco_hip.graphs import GraphStore
    st = GraphStore.generated("REG", G, n, d, seed=7)
    st.check_errors()
    assert st.cap == n * d
    A = _adjacency(st)
    assert np.array_equal(A, A.transpose(0, 2, 1)) and not np.einsum("gii->g", np.abs(A)).any()
    assert np.all((A != 0).sum(2) == d)
    assert set(np.unique(A)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(st.row_ptr.cpu().numpy(), np.tile(np.arange(n + 1) * d, (G, 1)))
    assert int(st.valid.sum().item()) == G
    assert np.array_equal(st.deg.cpu().numpy(), np.full((G, n), d))
    S = A != 0
    assert all(not np.array_equal(S[0], S[g]) for g in range(1, min(G, 8)))     # slots differ
    again = GraphStore.generated("REG", G, n, d, seed=7)
    assert torch.equal(again.edges, st.edges) and torch.equal(again.row_ptr, st.row_ptr)
    g = G // 2                                        # one slot regenerated in place: same seed, same graph
    before = st.edges.clone()
    st.edges[g * st.cap:(g + 1) * st.cap] = 0
    st.generate(g, 1, "REG", d, seed=7)
    assert torch.equal(st.edges, before) and int(st.valid.sum().item()) == G
    other = GraphStore.generated("REG", G, n, d, seed=8)
    assert not torch.equal(other.edges, st.edges)


def test_regular_degree_zero_is_an_empty_graph():
    from eco_hip.graphs import GraphStore
    st = GraphStore.generated("REG", 3, 10, 0, seed=1)
    st.check_errors()
    assert not st.row_ptr.any().item() and not st.valid.any().item()


def test_regular_pair_marginals():
    """Every pair is an edge with probability exactly d / (n - 1) (the algorithm treats all labels alike): at (8, 3)
    each of the 28 pair frequencies over 4096 device graphs is within 5 standard errors of 3 / 7."""
    from eco_hip.graphs import GraphStore
    n, d, G = 8, 3, 4096
    st = GraphStore.generated("REG", G, n, d, seed=21, weights="uniform")
    st.check_errors()
    freq = _adjacency(st).mean(0)
    p = d / (n - 1)
    se = np.sqrt(p * (1 - p) / G)
    iu = np.triu_indices(n, 1)
    print("pair frequencies - 3/7, in standard errors:", np.round((freq[iu] - p) / se, 2))
    assert np.all(np.abs(freq[iu] - p) < 5 * se)


def _two_triangle_fraction(S):
    """S [G, 6, 6] bool, 2-regular: the graph is two triangles iff the two neighbours of vertex 0 are adjacent."""
    nb = np.argsort(~S[:, 0, :], axis=1, kind="stable")[:, :2]
    return S[np.arange(S.shape[0]), nb[:, 0], nb[:, 1]].mean()


def test_regular_distribution_matches_host_restatement():
    """(6, 2): a 6-cycle or two triangles.  The device's two-triangle fraction over 8192 graphs against the host
    restatement's (random_csr, numpy stream) over 8192: within 5 standard errors of the difference of two samples."""
    from eco_hip.graphs import GraphStore, random_csr
    n, d, G = 6, 2, 8192
    st = GraphStore.generated("REG", G, n, d, seed=33, weights="uniform")
    st.check_errors()
    dev = _two_triangle_fraction(_adjacency(st) != 0)
    csr = random_csr("REG", G, n, d, seed=34, weights="uniform")
    cols = (csr[2] & 0xFFFFFF).astype(np.int64).reshape(G, n, d)
    H = np.zeros((G, n, n), dtype=bool)
    H[np.arange(G)[:, None, None], np.arange(n)[None, :, None], cols] = True
    host = _two_triangle_fraction(H)
    pooled = (dev + host) / 2
    se = np.sqrt(pooled * (1 - pooled) * 2 / G)
    print(f"two-triangle fraction: device {dev:.4f}, host restatement {host:.4f}, se of the difference {se:.4f}")
    assert 0 < host < 1 and abs(dev - host) < 5 * se


@pytest.mark.parametrize("n,k,G", [(9, 4, 8), (7, 3, 8), (8, 8, 8), (200, 6, 16)])
def test_ring_lattice(n, k, G):
    from eco_hip.graphs import GraphStore
    st = GraphStore.generated("WS", G, n, k, seed=5)
    st.check_errors()
    A = _adjacency(st)
    ref = _ring(n, k)
    assert st.cap == int(ref.sum())
    for g in range(G):
        np.testing.assert_array_equal(np.abs(A[g]), ref)
    assert np.array_equal(A, A.transpose(0, 2, 1)) and int(st.valid.sum().item()) == G
    w = A[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]]
    w = w[w != 0]                                     # one fair sign per undirected edge, pooled over the store
    assert set(np.unique(w)) == {-1.0, 1.0}
    assert abs((w > 0).mean() - 0.5) < 5 * 0.5 / np.sqrt(w.size)
    uni = GraphStore.generated("WS", 2, n, k, seed=5, weights="uniform")
    np.testing.assert_array_equal(uni.dense(1), ref)
    again = GraphStore.generated("WS", G, n, k, seed=5)
    assert torch.equal(again.edges, st.edges)


def test_ring_lattice_k_zero_is_empty():
    from eco_hip.graphs import GraphStore
    st = GraphStore.generated("WS", 2, 10, 0, seed=5)
    st.check_errors()
    assert not st.row_ptr.any().item() and not st.valid.any().item()


@pytest.mark.parametrize("kind,param", [("REG", 4), ("WS", 5)])
def test_float_weights(kind, param):
    from eco_hip.graphs import GraphStore
    n, G = 12, 64
    st = GraphStore.generated(kind, G, n, param, seed=11, weights="random")
    st.check_errors()
    assert st.float_weights and not st.unit_weights
    ref = GraphStore.generated(kind, G, n, param, seed=11, weights="discrete")
    assert torch.equal(st.row_ptr, ref.row_ptr)                 # the structure does not depend on the weight kind
    assert torch.equal(st.edges & 0xFFFFFF, ref.edges & 0xFFFFFF)
    ew = st.edge_weights.cpu().numpy()
    assert np.all(ew != 0) and np.all(np.abs(ew) < 1)
    sign = (st.edges.cpu().numpy().view(np.uint32) >> 24).astype(np.uint8).view(np.int8)
    np.testing.assert_array_equal(sign, np.sign(ew).astype(np.int8))
    for g in (0, G - 1):
        m = st.dense(g)
        np.testing.assert_array_equal(m, m.T)
        assert not np.diag(m).any() and np.all((m != 0).sum(1) == 4)
    assert int(st.valid.sum().item()) == G


@pytest.mark.parametrize("kind,n,param,cap", [("REG", 9, 3, 27),      # n d odd
                                               ("REG", 8, 8, 64),      # d = n
                                               ("REG", 8, 2.5, 64),    # not an integer
                                               ("WS", 8, 9, 64),       # k > n
                                               ("REG", 20, 3, 59),     # edge slot of n d - 1
                                               ("WS", 8, 8, 55),       # complete graph needs 56
                                               ("REG", 2000, 12, 24000)])  # lists beyond one workgroup's LDS
def test_argument_errors_come_from_the_host_check(kind, n, param, cap):
    from eco_hip.graphs import GraphStore
    st = GraphStore.slots(2, n, cap)
    with pytest.raises(ValueError):
        st.generate(0, 2, kind, param, seed=1)
    st.check_errors()                                  # nothing ran: no device error, nothing written
    assert not st.row_ptr.any().item() and not st.edges.any().item()


def test_generated_regular_graphs_drive_env_like_oracle():
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    n, d, B = 20, 3, 32
    st = GraphStore.generated("REG", B, n, d, seed=1)
    env = VecSpinSystem(st, B, 2 * n, want_f64=True, observables=DEFAULT_OBSERVABLES,
                        reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                        optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED,
                        norm_rewards=True, basin_reward=1. / n)
    rng = np.random.default_rng(0)
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    env.reset(graph_ids=np.arange(B), spins=spins)
    o = so.SpinSystemOracle(st.dense(7), 2 * n, basin_reward=1. / n)
    o.reset(spins=spins[7])
    for t in range(2 * n):
        a = rng.integers(0, n, B)
        _, r, _ = env.step(torch.from_numpy(a).to(torch.int32).cuda())
        _, orew, _, _ = o.step(int(a[7]))
        assert r[7].item() == orew
    env.check_errors()
    np.testing.assert_array_equal(env.obs_f64[7].cpu().numpy().view(np.uint64), o.state_rows().view(np.uint64))


@pytest.mark.parametrize("kind,param", [("REG", 3), ("WS", 4)])
def test_learn_with_fresh_graphs_per_episode(kind, param):
    from eco_hip.graphs import GraphStore, edge_cap
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    n, B = 20, 128
    st = GraphStore.slots(2 * B, n, edge_cap(kind, n, param))
    env = VecSpinSystem(st, B, 2 * n, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                        extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                        spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n)
    agent = DQN(env, lambda: MPNN(device="cuda"), init_weight_std=0.01, gamma=0.95, replay_start_size=256,
                replay_buffer_size=B * 2 * n, update_target_frequency=500, update_learning_rate=False,
                initial_learning_rate=1e-4, update_frequency=32, minibatch_size=64, train_minibatch=128,
                regenerate_graphs=(kind, param), seed=2)
    agent.learn(timesteps=B * 2 * n * 3)
    env.check_errors()
    assert agent.graphs_regenerated > 0
    assert agent.grad_steps > 0 and torch.isfinite(agent.network.flat).all()
    deg = st.deg.cpu().numpy()
    assert np.all(deg[st.valid.cpu().numpy() == 1] == (param if kind == "REG" else 2 * (param // 2)))


def test_generator_classes_feed_the_single_env():
    """core.make("SpinSystem", gg, ...) with the three generator classes: the env's adjacency is the generator's
    matrix, and an episode on it follows the oracle (exactly for the integer weights, and for the float weights of
    PerturbedGraphGenerator within 1e-12 on rewards of order 1: a 20-term float64 sum rounds below 1e-14)."""
    from eco_hip.envs import core
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget, SpinBasis,
                                    EdgeType, RandomRegularGraphGenerator, RandomWattsStrogatzGraphGenerator,
                                    PerturbedGraphGenerator)
    n, T = 20, 40
    kw = dict(observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
              optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED, norm_rewards=True,
              basin_reward=1. / n, reversible_spins=True)
    np.random.seed(5)
    base = RandomRegularGraphGenerator(n, 4, EdgeType.DISCRETE).get()
    gens = [(RandomRegularGraphGenerator(n, [3, 0], EdgeType.DISCRETE), 3, 0.0),
            (RandomWattsStrogatzGraphGenerator(n, [4, 0], EdgeType.DISCRETE), 4, 0.0),
            (PerturbedGraphGenerator([base], 0.0, 0.05, ordered=True), 4, 1e-12)]
    rng = np.random.default_rng(2)
    for gg, deg, tol in gens:
        env = core.make("SpinSystem", gg, T, **kw)
        spins = 2 * rng.integers(0, 2, n) - 1
        obs = env.reset(spins=spins)
        M = np.array(obs[7:], dtype=np.float64)
        assert np.array_equal(M, M.T) and not np.diag(M).any() and np.all((M != 0).sum(1) == deg)
        if tol:
            assert np.array_equal(M != 0, base != 0) and np.all(M[M != 0] != np.round(M[M != 0]))
        o = so.SpinSystemOracle(M, T, basin_reward=1. / n)
        o.reset(spins=spins)
        for a in rng.integers(0, n, 12):
            _, r, done, _ = env.step(int(a))
            _, orew, odone, _ = o.step(int(a))
            assert abs(r - orew) <= tol and done == odone
