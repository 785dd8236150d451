"""2048 < N <= 8192: the workgroup-per-episode env kernels (csrc/eco_env_wg.hip), the MPNN forward above 2048
vertices (eco_mpnn_forward_wg, picked by MPNN.forward_graphs) and the solvers on them.

Bars: env rewards, dones, float64 observation rows, spins, best spins and scores bit-exact against
oracle.spinsystem_oracle (exact integer scores, the reference's own float64 operations); Q within 5e-7 (1 + |q|) of
oracle.mpnn_oracle, the project's bar for an f32 forward in another summation order (tests/test_large_gpu.py:5), and
of oracle.mpnn_sparse_oracle (float64 over the edge list); rows of thousands of entries get the bar derived in
test_forward_large_sizes.

Cost.  Up to 4100 the dense CPU oracles are what these tests cost (four dense J @ s products and up to three [N, N]
outer products per env oracle step, 72 oracle steps per env case; an [N, N, 63] tensor, about 1 GB at 2049, per MPNN
oracle call): 2 to 4 s per case.  Above, the oracles run over the edge list -- the env oracle's sparse mode (84 steps
of a few sums over 82,000 directed edges: 0.1 s per episode) and the float64 MPNN oracle (three calls of 0.3 s and
one float32-mode call of 0.5 s per case at 8192) -- and no [N, N] array is formed: under a second per case.  The
sizes are the smallest that put a vertex in slot 8 (2049), a partial last slot and a partial last 64-bit word (4100)
and every slot (8192); 8191 is the largest size with a padded row."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
from oracle import mpnn_sparse_oracle as ms
from oracle import spinsystem_oracle as so

pytestmark = pytest.mark.gpu

BAR = 5e-7


def _scaled_err(a, b):
    e = float(((a - b).abs() / (1 + b.abs())).max())
    print(f"scaled err {e:.3e}")
    return e


def _env_args(**over):
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget, SpinBasis)
    a = dict(observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
             optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED, norm_rewards=True)
    a.update(over)
    return a


def _cut(i, j, w, spins):
    """Cut weight of signed spins on the undirected edge list (i, j, w)."""
    return float(np.sum(w * (spins[i] != spins[j])))


def _edge_list(store, g=0):
    """(i, j, w) with i < j of graph g of a store, from its CSR."""
    rp = store.row_ptr[g].cpu().numpy()
    b = int(store.edge_base[g].item())
    e = store.edges[b:b + int(rp[-1])].cpu().numpy().view(np.uint32)
    rows = np.repeat(np.arange(store.n_spins), np.diff(rp))
    cols = (e & 0xFFFFFF).astype(np.int64)
    w = (e >> 24).astype(np.uint8).view(np.int8).astype(np.int64)
    keep = rows < cols
    return rows[keep], cols[keep], w[keep]


# ---- 1. env against the CPU oracle ----

def _actions(n, B, steps, rng):
    """Injected actions [steps][B]: vertex 0, vertex N - 1, the same vertex twice in a row after them (the second
    flip returns to a state that WAS inserted: a revisit), the last vertex of slot 7 and the first of slot 8, then
    random ones."""
    a = rng.integers(0, n, (steps, B))
    a[0], a[1] = 0, n - 1
    a[2] = a[3] = rng.integers(0, n, B)
    a[4], a[5] = 2047, 2048
    a[6] = a[7] = n - 1     # twice the last vertex: revisits the state after step 6
    if n == 8192:           # each twice in a row (a revisit each): the hub, slots 17, 24 and 31, words 65 and 127, 0
        for t, v in zip(range(8, 22, 2), (HUB, 4400, 6200, 8000, 4170, 8130, 0)):
            a[t] = a[t + 1] = v
        assert [v // 256 for v in (HUB, 4400, 6200, 8000)] == [19, 17, 24, 31] and (4170 // 64, 8130 // 64) == (65, 127)
    return a


HUB = 5000   # the vertex of degree 8191 of the N = 8192 env graph


def _env_graph_8192(rng):
    """(i, j, w): ER of mean degree 8 with +-1 weights plus vertex HUB joined to every other vertex (its flip
    scatters a row of 8191 entries through the LDS delta array, 32 edges per thread)."""
    n = 8192
    i, j = _er_edges(n, 8.0, rng)
    keep = (i != HUB) & (j != HUB)
    others = np.delete(np.arange(n), HUB)
    i, j = np.concatenate([i[keep], np.full(n - 1, HUB)]), np.concatenate([j[keep], others])
    return i, j, rng.choice([-1, 1], i.size)


@pytest.mark.parametrize("n,basis,obs_kind", [(2049, "BINARY", "default"), (4100, "SIGNED", "custom"),
                                              (8192, "SIGNED", "custom"), (8192, "BINARY", "default")])
def test_env_matches_oracle(n, basis, obs_kind):
    """B = 3 episodes on one er_graph(N, 8 / N, uniform), T = 64, BLS reward, norm_rewards, basin_reward = 1 / N, 24
    injected actions: rewards, dones and float64 observation rows bit-exact every step; spins, best spins, best score
    and the visited-set size at the end.  N = 2049: one vertex in slot 8, BINARY basis, DEFAULT_OBSERVABLES (with a
    second env that takes the fp32-only fast write, compared bitwise).  N = 4100: a partial last slot and a partial
    last 64-bit word, a non-default observable list (the general write) and a stagnation punishment, so the revisits
    show in the rewards.  N = 8192 (both observable lists): the 32-slot instantiation with every slot and all 128
    state words in use, on _env_graph_8192 (+-1 weights, a hub of degree 8191) against the oracle's sparse mode, 28
    injected actions that flip and at once re-flip vertex 0, vertex 8191, the hub, a vertex in each of slots 17, 24
    and 31 and in each of words 65 and 127."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import Observable, SpinBasis
    B, T, steps = 3, 64, 28 if n == 8192 else 24
    rng = np.random.default_rng(n)
    if n == 8192:
        edges = _env_graph_8192(rng)
        J = so.SparseMatrix.from_edges(n, *edges)
        store = GraphStore.from_edges(n, *edges)
        assert int(store.max_deg[0]) == n - 1
    else:
        J = og.er_graph(n, 8.0 / n, rng, weights="uniform")
        store = GraphStore.from_dense([J])
    custom = [Observable.SPIN_STATE, Observable.TIME_SINCE_FLIP, Observable.IMMEDIATE_QUALITY_CHANGE,
              Observable.NUMBER_OF_QUALITY_IMPROVEMENTS, Observable.DISTANCE_FROM_BEST_STATE,
              Observable.TERMINATION_IMMANENCY]
    stag = 0.01 if obs_kind == "custom" else None
    over = dict(spin_basis=SpinBasis[basis], basin_reward=1. / n, stag_punishment=stag)
    okw = dict(basin_reward=1. / n, spin_basis=basis, stag_punishment=stag)
    if obs_kind == "custom":
        over["observables"] = custom
        okw["observables"] = [o.value for o in custom]
    env = VecSpinSystem(store, B, T, want_f64=True, **_env_args(**over))
    fast = VecSpinSystem(store, B, T, **_env_args(**over)) if obs_kind == "default" else None
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    gids = np.zeros(B, dtype=np.int64)
    env.reset(graph_ids=gids, spins=spins)
    if fast is not None:
        fast.reset(graph_ids=gids, spins=spins)
        assert torch.equal(fast.obs_x.view(torch.int32), env.obs_x.view(torch.int32))
    oracles = []
    for b in range(B):
        o = so.SpinSystemOracle(J, T, **okw)
        o.reset(spins=(spins[b] + 1) // 2 if basis == "BINARY" else spins[b])
        np.testing.assert_array_equal(env.obs_f64[b].cpu().numpy().view(np.uint64), o.state_rows().view(np.uint64))
        oracles.append(o)
    acts = _actions(n, B, steps, rng)
    act = torch.zeros(B, dtype=torch.int32, device="cuda")
    revisits = 0
    for t in range(steps):
        act.copy_(torch.from_numpy(acts[t]).to(torch.int32))
        _, r, d = env.step(act)
        if fast is not None:
            fast.step(act)
            assert torch.equal(fast.obs_x.view(torch.int32), env.obs_x.view(torch.int32)), t
            assert torch.equal(fast.rewards, env.rewards)
        r = r.cpu().numpy()
        f64 = env.obs_f64.cpu().numpy()
        for b, o in enumerate(oracles):
            before = sum(len(v) for v in o.history.buffer.values())
            _, orew, odone, _ = o.step(int(acts[t, b]))
            revisits += sum(len(v) for v in o.history.buffer.values()) == before
            assert r[b] == orew and bool(d[b]) == odone, (t, b, r[b], orew)
            np.testing.assert_array_equal(f64[b].view(np.uint64), o.state_rows().view(np.uint64))
    assert revisits >= (9 if n == 8192 else 2) * B    # steps 3 and 7 of every episode; 8192: every odd step to 21
    env.check_errors()
    st = env.read(spins=True, best_spins=True)
    for b, o in enumerate(oracles):
        np.testing.assert_array_equal(st["spins"][b].cpu().numpy(), o.state[0].astype(np.int8))
        np.testing.assert_array_equal(st["best_spins"][b].cpu().numpy(), o.best_spins.astype(np.int8))
        assert float(st["best_score"][b]) == o.best_score and float(st["score"][b]) == o.score
        assert float(st["best_solution"][b]) == o.best_solution


# ---- 2. env at the cap ----

def test_env_n8192_ring_lattice():
    """N = 8192 (every slot, 128 words): ring lattice k = 4 with +-1 weights from the host generator, B = 2, 40 random
    flips.  The score is the cut recomputed from the edge list and the returned spins (+ |lower bound|); best_score
    dominates every intermediate score; a masked reset re-initialises only the masked episode."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    n, B, T = 8192, 2, 64
    store = GraphStore.random("WS", 1, n, 4, seed=3, weights="discrete")
    i, j, w = _edge_list(store)
    assert i.size == 2 * n
    lbabs = float(-w[w < 0].sum())
    env = VecSpinSystem(store, B, T, **_env_args(basin_reward=1. / n))
    rng = np.random.default_rng(8192)
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    env.reset(graph_ids=np.zeros(B, dtype=np.int64), spins=spins)
    cur = spins.copy()
    acts = rng.integers(0, n, (40, B))
    acts[0], acts[1], acts[2] = 0, n - 1, n - 256
    act = torch.zeros(B, dtype=torch.int32, device="cuda")
    seen = []
    for t in range(40):
        act.copy_(torch.from_numpy(acts[t]).to(torch.int32))
        env.step(act)
        cur[np.arange(B), acts[t]] *= -1
        st = env.read(spins=True)
        sp = st["spins"].cpu().numpy()
        np.testing.assert_array_equal(sp, cur.astype(np.int8))
        score = st["score"].cpu().numpy()
        for b in range(B):
            assert score[b] == _cut(i, j, w, sp[b]) + lbabs, (t, b)
        seen.append(score.copy())
    env.check_errors()
    st = env.read(spins=True, best_spins=True)
    best = st["best_score"].cpu().numpy()
    init = np.array([_cut(i, j, w, spins[b]) + lbabs for b in range(B)])
    assert (best == np.maximum(np.max(seen, axis=0), init)).all()
    bsp = st["best_spins"].cpu().numpy()
    for b in range(B):
        assert best[b] == _cut(i, j, w, bsp[b]) + lbabs
    # masked reset: episode 1 only
    fresh = 2 * rng.integers(0, 2, (B, n)) - 1
    keep = {k: st[k].cpu().numpy().copy() for k in ("score", "best_score", "current_step", "spins")}
    env.reset(spins=fresh, mask=np.array([0, 1], dtype=np.uint8))
    st = env.read(spins=True)
    sp = st["spins"].cpu().numpy()
    np.testing.assert_array_equal(sp[0], keep["spins"][0])
    np.testing.assert_array_equal(sp[1], fresh[1].astype(np.int8))
    assert float(st["current_step"][0]) == 40 and float(st["current_step"][1]) == 0
    assert float(st["score"][0]) == keep["score"][0] and float(st["best_score"][0]) == keep["best_score"][0]
    assert float(st["score"][1]) == float(st["best_score"][1]) == _cut(i, j, w, fresh[1]) + lbabs
    env.check_errors()


# ---- 3. Greedy ----

def _greedy_matches_oracle(J, store, spins, T, max_distinct):
    """greedy_actions + step on `store` against the oracle's greedy loop (solver.py:100-131) on J (a dense matrix or
    the oracle's sparse form): the same actions, the same final cut; returns the oracles' action lists."""
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import Observable
    B = spins.shape[0]
    obs = [Observable.SPIN_STATE, Observable.IMMEDIATE_QUALITY_CHANGE]
    env = VecSpinSystem(store, B, T, **_env_args(observables=obs))
    env.reset(graph_ids=np.zeros(B, dtype=np.int64), spins=spins)
    got = []
    for _ in range(T):
        a = env.greedy_actions()
        done = env.read()["done"].cpu().numpy() != 0
        if done.all():
            break
        got.append(np.where(done, -1, a.cpu().numpy()))
        env.step(a)
    got = np.array(got)
    st = env.read()
    env.check_errors()
    wants = []
    for b in range(B):
        o = so.SpinSystemOracle(J, T, observables=[o_.value for o_ in obs], basin_reward=None)
        o.reset(spins=spins[b])
        want = so.greedy_solve(o)
        mine = [int(x) for x in got[:, b] if x >= 0]
        assert mine == want, b
        assert len(set(np.round(so.calculate_cut_changes(o.state[0], o.matrix)))) < max_distinct   # few gains: ties
        assert float(st["score"][b]) == o.score
        assert float(st["best_solution"][b]) == o.best_solution
        wants.append(want)
    return wants


def test_greedy_n2049_matches_oracle():
    """greedy_actions + step at N = 2049 on +-1 weights (small integer gains: ties at every step, the lowest index
    must win) against the oracle's greedy loop (solver.py:100-131): the same actions and the same final cut.  T = 40
    bounds the loop (the oracle steps densely)."""
    from eco_hip.graphs import GraphStore
    n, B, T = 2049, 2, 40
    rng = np.random.default_rng(49)
    J = og.er_graph(n, 8.0 / n, rng, weights="discrete")
    store = GraphStore.from_dense([J])
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    spins[1, 1:] = spins[0, 1:]   # nearly the same start: the tie-breaks of both episodes differ by one vertex
    _greedy_matches_oracle(J, store, spins, T, 20)


def test_greedy_n8192_matches_oracle():
    """The same at the cap (32 slots of 256 vertices), against the oracle's sparse mode: ER of mean degree 8, +-1
    weights, T = 40.  A tie across the slots is planted: vertex 3 (slot 0) and vertex 8000 (slot 31) are each the
    centre of a star of 30 private leaves with weight +1 and every spin of both stars +1, so each centre gains
    exactly 30; every other vertex has at most 29 edges of weight +-1 (asserted) and gains at most 29.  The first
    step therefore sees the maximum at exactly these two vertices, and the lower index, in slot 0, must win; the
    second step takes 8000."""
    from eco_hip.graphs import GraphStore
    n, B, T = 8192, 2, 40
    rng = np.random.default_rng(8192 + 49)
    i, j = _er_edges(n, 8.0, rng)
    stars = {3: np.arange(300, 330), 8000: np.arange(7000, 7030)}
    private = np.concatenate([[c] + list(v) for c, v in stars.items()])
    keep = ~np.isin(i, private) & ~np.isin(j, private)
    i, j = i[keep], j[keep]
    w = rng.choice([-1, 1], i.size)
    assert np.bincount(np.concatenate([i, j]), minlength=n).max() <= 29
    for c, leaves in stars.items():
        i, j, w = np.concatenate([i, np.full(30, c)]), np.concatenate([j, leaves]), np.concatenate([w, np.ones(30, int)])
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    spins[1, 1:] = spins[0, 1:]
    spins[:, private] = 1
    model = so.SparseMatrix.from_edges(n, i, j, w)
    g = so.calculate_cut_changes(spins[0].astype(np.float64), model)
    assert g[3] == g[8000] == g.max() == 30 and (g == 30).sum() == 2
    wants = _greedy_matches_oracle(model, GraphStore.from_edges(n, i, j, w), spins, T, 62)
    assert all(want[:2] == [3, 8000] and len(want) == T for want in wants)


# ---- 4. MPNN against the torch oracle ----

def _mpnn_case(n, B, n_obs, seed):
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    rng = np.random.default_rng(seed)
    mats = [og.er_graph(n, 8.0 / n, rng, weights="uniform" if b % 2 else "discrete") for b in range(B)]
    store = GraphStore.from_dense(mats)
    g = torch.Generator().manual_seed(seed)
    w = mo.init_weights(g, std=0.1, n_obs_in=n_obs)
    net = MPNN(n_obs_in=n_obs, device="cuda")
    net.load_state_dict(w)
    x = torch.zeros(B, n, 8 if n_obs <= 8 else 16)
    x[:, :, :n_obs] = torch.rand(B, n, n_obs, generator=g) * 2 - 1
    return mats, store, w, net, x


@pytest.mark.parametrize("n,n_obs", [(2049, 7), (2304, 7), (2049, 13)])
def test_forward_matches_oracle(n, n_obs):
    """B = 2 graphs (one +-1, one unit-weight) under the per-graph norm against the fp32 torch oracle, one oracle call
    per graph; then NORM_PER_CALL with the fused greedy act: actions == argmax of the returned Q.  n_obs = 13: the
    16-float-row instance."""
    from eco_hip._lib import ActConfig, ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL
    B = 2
    mats, store, w, net, x = _mpnn_case(n, B, n_obs, seed=n + n_obs)
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    q = net.forward_graphs(x.cuda(), store, gids, norm_scope=ECO_NORM_PER_GRAPH).cpu()
    edges = []
    for b in range(B):
        obs = torch.from_numpy(np.vstack([x[b, :, :n_obs].numpy().T.astype(np.float64), mats[b]])).float()
        dense = mo.forward(w, obs, n_obs_in=n_obs)
        assert _scaled_err(q[b], dense) <= BAR
        del obs
        # the float64 edge-list oracle, the judge above 2304 vertices, at a size where both oracles run
        i, j = np.nonzero(np.triu(mats[b]))
        edges.append((i, j, mats[b][i, j]))
        sparse = torch.from_numpy(ms.forward(w, x[b, :, :n_obs].numpy(), n, *edges[b], n_obs_in=n_obs))
        assert _scaled_err(q[b].double(), sparse) <= BAR
        assert _scaled_err(dense.double(), sparse) <= BAR
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    qc = torch.empty(B, n, device="cuda")
    net.forward_graphs(x.cuda(), store, gids, norm_scope=ECO_NORM_PER_CALL, q_out=qc,
                       act=ActConfig(0.0, 1, 0.0, 1, 0), actions_out=acts)
    assert torch.equal(acts.long(), qc.argmax(1))
    # the graph whose own norm.max() is the smaller one against the oracle with the call-wide maximum
    degs = [int((m != 0).sum(1).max()) for m in mats]
    b = int(np.argmin(degs))
    obs = torch.from_numpy(np.vstack([x[b, :, :n_obs].numpy().T.astype(np.float64), mats[b]])).float()
    assert _scaled_err(qc[b].cpu(), mo.forward(w, obs, n_obs_in=n_obs, norm_max=max(degs))) <= BAR
    sparse = ms.forward(w, x[b, :, :n_obs].numpy(), n, *edges[b], n_obs_in=n_obs, norm_max=max(degs))
    assert _scaled_err(qc[b].cpu().double(), torch.from_numpy(sparse)) <= BAR


# ---- 5. MPNN at 4100, 8191 and the cap against the float64 edge-list oracle ----

def _er_edges(n, mean_deg, rng):
    """About n * mean_deg / 2 distinct undirected pairs (i < j), no dense matrix."""
    k = int(n * mean_deg / 2)
    a, b = rng.integers(0, n, k), rng.integers(0, n, k)
    key = np.unique((np.minimum(a, b) * n + np.maximum(a, b))[a != b])
    return key // n, key % n


def _large_graphs(n, rng):
    """[(i, j, wt)] * 2.  Graph 0: ER, mean degree 6, +-1 weights (it has isolated vertices: 8192 e^-6 = 20).
    Graph 1: ER, mean degree 3, with vertex 0 a hub -- of every other vertex at 8191 and 8192 (a row of N - 1
    entries, the longest the format allows; edge (0, N - 1) weighs 127), of every vertex but 4099 at 4100, where
    4099 stays isolated in the partial last 16-row group (edge (0, 4098) weighs 127); a few more weights are +-127
    and -128."""
    i0, j0 = _er_edges(n, 6.0, rng)
    g0 = (i0, j0, rng.choice([-1, 1], i0.size))
    i1, j1 = _er_edges(n, 3.0, rng)
    iso = n - 1 if n == 4100 else -1
    keep = (i1 != 0) & (i1 != iso) & (j1 != iso)          # i < j: the hub's edges are the i == 0 ones
    i1, j1 = i1[keep], j1[keep]
    w1 = rng.choice([-1, 1], i1.size)
    w1[rng.choice(i1.size, 6, replace=False)] = [127, -127, -128, 127, -127, -128]
    hub = np.array([v for v in range(1, n) if v != iso])
    wh = rng.choice([-1, 1], hub.size)
    wh[[5, 77, 1000]] = [-128, 127, -127]
    wh[-1] = 127
    g1 = (np.concatenate([np.zeros(hub.size, np.int64), i1]), np.concatenate([hub, j1]), np.concatenate([wh, w1]))
    return [g0, g1], iso


def _two_graph_store(n, graphs):
    from eco_hip.graphs import CSR, GraphStore, edges_to_csr
    parts = [edges_to_csr(n, *g) for g in graphs]
    assert all(p.weights is None for p in parts)
    base = np.cumsum([0] + [p[2].size for p in parts[:-1]]).astype(np.int64)
    return GraphStore.from_csr(CSR(np.vstack([p[0] for p in parts]), base, np.concatenate([p[2] for p in parts])))


@pytest.mark.parametrize("n,n_obs", [pytest.param(4100, 7, id="4100"), pytest.param(8191, 7, id="8191"),
                                     pytest.param(8192, 7, id="8192"), pytest.param(8192, 13, id="8192-13")])
def test_forward_large_sizes(n, n_obs):
    """B = 2 on the graphs of _large_graphs: Q finite, the fused act equals the argmax, Q of episode 0 does not move
    when episode 1 runs another graph under the per-graph norm (an episode offset that overflowed would alias the
    two) -- and Q against oracle.mpnn_sparse_oracle (float64 over the edge list) under ECO_NORM_PER_GRAPH and
    ECO_NORM_PER_CALL; under the latter graph 0 is judged with norm_max = the hub's degree (N - 1 = 8191 at the cap:
    the largest value of the packed row info's norm field; N - 2 at 4100, where the hub leaves 4099 isolated), and
    the fused act at epsilon = 0 must be the oracle's argmax wherever the oracle's two best Q are more than twice the
    bar apart.  N = 4100: rows_pad 4112, a partial last 16-row group; 8191: the largest size with a padded row; 8192:
    the cap, also with the 16-float rows of n_obs = 13.

    Bars.  Graph 0 (rows of a few dozen entries): 5e-7 (1 + |q|), the file's bar.  Graph 1: max(5e-7, 4 E32)
    (1 + |q|), where E32 is the largest scaled error of the oracle's own float32 mode (the same statements in
    np.float32, each row summed entry by entry) against its float64 mode, computed here for the case's own inputs:
    what ONE float32 evaluation of a sum of N - 1 terms of magnitude up to 128 costs; the factor 4 covers the
    kernel's different summation order and its bf16x3 weight split, and is not to grow.
    Recorded on one MI355X (E32 | kernel's scaled error on graph 0 | on graph 1, per-graph norm; the per-call
    figures are the same within 10 %):
      N 4100, n_obs 7:   E32 1.66e-6 | 3.5e-8 | 1.03e-6      N 8191, n_obs 7:   E32 2.76e-6 | 6.1e-8 | 2.60e-6
      N 8192, n_obs 7:   E32 2.93e-6 | 3.6e-8 | 7.13e-6      N 8192, n_obs 13:  E32 2.84e-5 | 4.9e-8 | 3.73e-6"""
    from eco_hip.networks.mpnn import MPNN
    from eco_hip._lib import ActConfig, ECO_NORM_PER_GRAPH, ECO_NORM_PER_CALL
    B = 2
    rng = np.random.default_rng(n + n_obs)
    graphs, iso = _large_graphs(n, rng)
    store = _two_graph_store(n, graphs)
    deg = [np.bincount(np.concatenate([g[0], g[1]]), minlength=n) for g in graphs]
    hub_deg = n - 2 if n == 4100 else n - 1
    assert deg[1][0] == hub_deg == deg[1].max() and deg[0].max() < 40 and (deg[0] == 0).any()
    assert (deg[1][iso] == 0) if n == 4100 else (deg[1].min() >= 1)
    assert store.max_deg.cpu().tolist() == [int(deg[0].max()), hub_deg]
    g = torch.Generator().manual_seed(n + n_obs)
    w = mo.init_weights(g, std=0.1, n_obs_in=n_obs)
    net = MPNN(n_obs_in=n_obs, device="cuda")
    net.load_state_dict(w)
    xw = 8 if n_obs <= 8 else 16
    x = torch.zeros(B, n, xw)
    x[:, :, :n_obs] = torch.rand(B, n, n_obs, generator=g) * 2 - 1
    xd = x.cuda()
    greedy = ActConfig(0.0, 1, 0.0, 1, 0)
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    q0 = torch.empty(B, n, device="cuda")
    net.forward_graphs(xd, store, torch.tensor([0, 0], dtype=torch.int32, device="cuda"),
                       norm_scope=ECO_NORM_PER_GRAPH, q_out=q0, act=greedy, actions_out=acts)
    assert torch.isfinite(q0).all()
    assert torch.equal(acts.long(), q0.argmax(1))
    gids = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    q1 = net.forward_graphs(xd, store, gids, norm_scope=ECO_NORM_PER_GRAPH)
    assert torch.isfinite(q1).all()
    assert torch.equal(q0[0], q1[0])
    assert not torch.equal(q0[1], q1[1])
    assert float(q0.abs().max()) > 0
    acts_c = torch.empty(B, dtype=torch.int32, device="cuda")
    qc = torch.empty(B, n, device="cuda")
    net.forward_graphs(xd, store, gids, norm_scope=ECO_NORM_PER_CALL, q_out=qc, act=greedy, actions_out=acts_c)
    assert torch.isfinite(qc).all()
    assert torch.equal(acts_c.long(), qc.argmax(1))
    q1, qc, acts, acts_c = q1.cpu().double().numpy(), qc.cpu().double().numpy(), acts.cpu().numpy(), acts_c.cpu().numpy()
    # the oracle: float64, and the float32 cost of graph 1's sums
    xs = [x[b, :, :n_obs].numpy() for b in range(B)]
    ref0 = ms.forward(w, xs[0], n, *graphs[0], n_obs_in=n_obs)
    ref0_call = ms.forward(w, xs[0], n, *graphs[0], n_obs_in=n_obs, norm_max=hub_deg)
    ref1, e32 = ms.f32_cost(w, xs[1], n, *graphs[1], n_obs_in=n_obs)
    bar1 = max(BAR, 4 * e32)
    assert np.abs(ref0 - ref0_call).max() > 1e-4           # the call-wide maximum is visible in graph 0's Q
    err = lambda q, ref: float((np.abs(q - ref) / (1 + np.abs(ref))).max())   # noqa: E731
    figures = {"g0 per-graph": err(q1[0], ref0), "g1 per-graph": err(q1[1], ref1),
               "g0 per-call": err(qc[0], ref0_call), "g1 per-call": err(qc[1], ref1)}
    print(f"N {n} n_obs {n_obs}: E32 {e32:.3e} bar1 {bar1:.3e} |q| up to {np.abs(ref1).max():.3g}; " +
          "; ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    assert figures["g0 per-graph"] <= BAR and figures["g0 per-call"] <= BAR
    assert figures["g1 per-graph"] <= bar1 and figures["g1 per-call"] <= bar1
    # the fused act against the oracle's argmax
    checked = 0
    for a, ref, bar in ((acts[0], ref0, BAR), (acts_c[0], ref0_call, BAR), (acts_c[1], ref1, bar1)):
        top = np.sort(ref)[-2:]
        if top[1] - top[0] > 2 * bar * (1 + abs(top[1])):
            assert int(a) == int(ref.argmax())
            checked += 1
    assert checked == 3       # every gap is far above its bar on these inputs (2e-3 against 1e-6 at the least)


# ---- 6. solvers end to end ----

def test_solvers_n2500():
    """Network(...).solve() and test_network(n_attempts=4) on one ER(2500) graph, max_steps = 30: the best cut returned
    equals the cut recomputed from the best spins returned; History rows have their shapes; the recorded actions,
    replayed on the host from the recorded first row, give the recorded spins and cut."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.solver import Greedy, Network, Random
    from eco_hip.experiments import test_network as run_test_network
    n, B, T = 2500, 3, 30
    rng = np.random.default_rng(2500)
    J = og.er_graph(n, 6.0 / n, rng, weights="discrete")
    store = GraphStore.from_dense([J])
    i, j, w = _edge_list(store)
    net = MPNN(device="cuda")
    net.load_state_dict(mo.init_weights(torch.Generator().manual_seed(5), std=0.1))
    env = VecSpinSystem(store, B, T, **_env_args())
    env.reset(graph_ids=np.zeros(B, dtype=np.int64))
    s = Network(net, env)
    s.reset()
    s.solve()
    env.check_errors()
    h = s.history
    ln = h.length.cpu().numpy()
    assert (ln == T + 1).all()
    assert tuple(h.action.shape) == (T + 1, B) and tuple(h.solution.shape) == (T + 1, B)
    assert tuple(h.qs.shape) == (T + 1, B, n) and tuple(h.spins.shape) == (T + 1, B, n)
    assert tuple(h.score_mask.shape) == (T + 1, B, n)
    action, spins, sol = h.action.cpu().numpy(), h.spins.cpu().numpy(), h.solution.cpu().numpy()
    qs = h.qs.cpu().numpy()
    st = env.read(best_spins=True)
    for e in range(B):
        cur = spins[0, e].astype(np.int64)
        assert sol[0, e] == _cut(i, j, w, cur)
        for t in range(1, T + 1):
            a = int(action[t, e])
            assert a == int(qs[t, e].argmax())
            cur[a] *= -1
            np.testing.assert_array_equal(spins[t, e], cur.astype(np.int8))
            assert sol[t, e] == _cut(i, j, w, cur), (e, t)
        assert float(s.measure[e]) == sol[T, e]
        assert float(st["best_solution"][e]) == _cut(i, j, w, st["best_spins"][e].cpu().numpy()) == sol[:, e].max()
    for cls in (Greedy, Random):
        env2 = VecSpinSystem(store, B, T, **_env_args())
        env2.reset(graph_ids=np.zeros(B, dtype=np.int64))
        s2 = cls(env2)
        s2.reset()
        s2.solve()
        env2.check_errors()
        st2 = env2.read(spins=True)
        for e in range(B):
            assert float(s2.measure[e]) == _cut(i, j, w, st2["spins"][e].cpu().numpy())
    args = _env_args(reversible_spins=True, memory_length=None, horizon_length=None, stag_punishment=None,
                     basin_reward=None)
    # step_factor: int(n * step_factor) == T whatever the rounding of the quotient
    res, raw = run_test_network(net, args, [J], step_factor=(T + 0.5) / n, n_attempts=4, return_raw=True, seed=1)
    r = res.iloc[0]
    assert len(raw["cuts"][0]) == 4
    assert float(r["cut"]) == _cut(i, j, w, np.asarray(r["sol"])) == max(raw["cuts"][0])
    assert float(r["greedy (rand init) cut"]) == _cut(i, j, w, np.asarray(r["greedy (rand init) sol"]))
    assert float(r["greedy (+1 init) cut"]) == _cut(i, j, w, np.asarray(r["greedy (+1 init) sol"]))


# ---- 7. boundaries ----

def test_boundaries_are_rejected_without_a_launch():
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem, make_config
    from eco_hip.envs.utils import OptimisationTarget
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    lib = _lib.lib
    with pytest.raises(ValueError, match="exceeds ECO_MAX_SPINS_WG=8192"):
        GraphStore.from_edges(8193, [0], [1], [1])
    with pytest.raises(ValueError, match="integer weights only"):
        GraphStore.from_edges(2049, [0], [1], [0.5])
    n = 2049
    store = GraphStore.from_edges(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1, np.int64))
    with pytest.raises(ValueError, match="OptimisationTarget.CUT only"):
        VecSpinSystem(store, 2, 8, **_env_args(optimisation_target=OptimisationTarget.MIN_COVER))
    env = VecSpinSystem(store, 2, 8, **_env_args())
    env.reset(graph_ids=np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match="at most ECO_MAX_SPINS=2048"):
        DQN(env, lambda: MPNN(device="cuda"))
    # the same rejections at the ABI, outputs pre-filled with a sentinel
    rew = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    dones = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
    obs = torch.full((2, n, 8), -7.0, device="cuda")
    act = torch.full((2,), 5, dtype=torch.int32, device="cuda")
    good = make_config(n, 8, **_env_args())
    for name, change, msg in (("n8193", dict(n_spins=8193), "[1, 8192]"),
                              ("float", dict(float_weights=1), "2048 < N <= 8192 takes integer weights only"),
                              ("cover", dict(optimisation_target=_lib.ECO_TARGET_MIN_COVER),
                               "2048 < N <= 8192 runs OptimisationTarget.CUT only")):
        cfg = _lib.EnvConfig.from_buffer_copy(good)
        for k, v in change.items():
            setattr(cfg, k, v)
        assert lib.eco_env_state_bytes(ctypes.byref(cfg), 2) == 0, name
        assert msg in _lib.last_error(), (name, _lib.last_error())
        rc = lib.eco_env_step(ctypes.byref(cfg), ctypes.byref(store.gs), _lib.ptr(env.state), 2, _lib.ptr(act),
                              _lib.ptr(rew), _lib.ptr(dones), _lib.ptr(obs), None, _lib.stream_ptr())
        assert rc == _lib.ECO_ERR_ARG and msg in _lib.last_error(), name
        rc = lib.eco_env_reset(ctypes.byref(cfg), ctypes.byref(store.gs), _lib.ptr(env.state), 2,
                               _lib.ptr(env.graph_ids), None, None, ctypes.c_uint64(0), _lib.ptr(obs), None,
                               _lib.stream_ptr())
        assert rc == _lib.ECO_ERR_ARG, name
        rc = lib.eco_env_greedy_actions(ctypes.byref(cfg), ctypes.byref(store.gs), _lib.ptr(env.state), 2,
                                        _lib.ptr(act), _lib.stream_ptr())
        assert rc == _lib.ECO_ERR_ARG, name
    torch.cuda.synchronize()
    assert (rew == -7.0).all() and (dones == 9).all() and (obs == -7.0).all() and (act == 5).all()
    # eco_mpnn_forward_wg
    wsb = lib.eco_mpnn_forward_wg_workspace_bytes
    assert wsb(2048, 2, 7) == 0 and wsb(8193, 2, 7) == 0 and wsb(2049, 2, 7) > 0
    net = MPNN(device="cuda")
    net._ensure_packed()
    q = torch.full((2, n), -7.0, device="cuda")
    x = torch.zeros(2, n, 8, device="cuda")
    gids = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.zeros(wsb(n, 2, 7), dtype=torch.uint8, device="cuda")

    def call(gs, batch=2, packed=net.packed, workspace=ws, q_out=q):
        return lib.eco_mpnn_forward_wg(_lib.ptr(packed), 7, ctypes.byref(gs), _lib.ptr(gids), batch, _lib.ptr(x),
                                       _lib.ECO_NORM_PER_GRAPH, _lib.ptr(q_out), None, None, _lib.ptr(workspace),
                                       _lib.stream_ptr())

    for n_bad in (2048, 8193):
        bad = _lib.GraphSet.from_buffer_copy(store.gs)
        bad.n_spins = n_bad
        assert call(bad) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error()
    assert call(store.gs, batch=0) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error()
    assert call(store.gs, packed=None) == _lib.ECO_ERR_ARG and "2048 < N <= 8192" in _lib.last_error()
    assert call(store.gs, workspace=None) == _lib.ECO_ERR_ARG
    assert call(store.gs, q_out=None) == _lib.ECO_ERR_ARG
    big = (2 ** 31 - 1) // 64 // 2064 + 1   # rows_pad(2049) = 2064
    assert call(store.gs, batch=big) == _lib.ECO_ERR_ARG and "32-bit row index" in _lib.last_error()
    torch.cuda.synchronize()
    assert (q == -7.0).all()
    # eco_mpnn_forward keeps its range
    with pytest.raises(ValueError, match="1 <= N <= 2048"):
        _lib.check(lib.eco_mpnn_forward(_lib.ptr(net.packed), 7, ctypes.byref(store.gs), _lib.ptr(gids), 2, _lib.ptr(x),
                                        _lib.ECO_NORM_PER_GRAPH, _lib.ptr(q), None, None, None, _lib.ptr(ws),
                                        _lib.stream_ptr()))
    assert (q == -7.0).all()
    assert call(store.gs) == _lib.ECO_OK   # and the accepted call writes q
    torch.cuda.synchronize()
    assert torch.isfinite(q).all() and not (q == -7.0).any()
