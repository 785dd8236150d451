"""2048 < N <= 8192: the workgroup-per-episode env kernels (csrc/eco_env_wg.hip), the MPNN forward above 2048
vertices (eco_mpnn_forward_wg, picked by MPNN.forward_graphs) and the solvers on them.

Bars: env rewards, dones, float64 observation rows, spins, best spins and scores bit-exact against
oracle.spinsystem_oracle (exact integer scores, the reference's own float64 operations); Q within 5e-7 (1 + |q|) of
oracle.mpnn_oracle, the project's bar for an f32 forward in another summation order (tests/test_large_gpu.py:5).

The dense CPU oracles are what these tests cost (four dense J @ s products and up to three [N, N] outer products per
env oracle step, 72 oracle steps per env case; an [N, N, 63] tensor, about 1 GB at 2049, per MPNN oracle call): 2 to
4 s per case.  The sizes are the smallest that put a vertex in slot 8 (2049), a partial last slot and a partial last
64-bit word (4100) and every slot (8192)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import graphs as og
from oracle import mpnn_oracle as mo
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
    return a


@pytest.mark.parametrize("n,basis,obs_kind", [(2049, "BINARY", "default"), (4100, "SIGNED", "custom")])
def test_env_matches_oracle(n, basis, obs_kind):
    """B = 3 episodes on one er_graph(N, 8 / N, uniform), T = 64, BLS reward, norm_rewards, basin_reward = 1 / N, 24
    injected actions: rewards, dones and float64 observation rows bit-exact every step; spins, best spins, best score
    and the visited-set size at the end.  N = 2049: one vertex in slot 8, BINARY basis, DEFAULT_OBSERVABLES (with a
    second env that takes the fp32-only fast write, compared bitwise).  N = 4100: a partial last slot and a partial
    last 64-bit word, a non-default observable list (the general write) and a stagnation punishment, so the revisits
    show in the rewards."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import Observable, SpinBasis
    B, T, steps = 3, 64, 24
    rng = np.random.default_rng(n)
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
    assert revisits >= 2 * B    # steps 3 and 7 of every episode
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

def test_greedy_n2049_matches_oracle():
    """greedy_actions + step at N = 2049 on +-1 weights (small integer gains: ties at every step, the lowest index
    must win) against the oracle's greedy loop (solver.py:100-131): the same actions and the same final cut.  T = 40
    bounds the loop (the oracle steps densely)."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import Observable
    n, B, T = 2049, 2, 40
    rng = np.random.default_rng(49)
    J = og.er_graph(n, 8.0 / n, rng, weights="discrete")
    store = GraphStore.from_dense([J])
    obs = [Observable.SPIN_STATE, Observable.IMMEDIATE_QUALITY_CHANGE]
    env = VecSpinSystem(store, B, T, **_env_args(observables=obs))
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    spins[1, 1:] = spins[0, 1:]   # nearly the same start: the tie-breaks of both episodes differ by one vertex
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
    for b in range(B):
        o = so.SpinSystemOracle(J, T, observables=[o_.value for o_ in obs], basin_reward=None)
        o.reset(spins=spins[b])
        want = so.greedy_solve(o)
        mine = [int(x) for x in got[:, b] if x >= 0]
        assert mine == want, b
        assert len(set(np.round(so.calculate_cut_changes(o.state[0], J)))) < 20   # few distinct gains: ties
        assert float(st["score"][b]) == o.score
        assert float(st["best_solution"][b]) == o.best_solution


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
    for b in range(B):
        obs = torch.from_numpy(np.vstack([x[b, :, :n_obs].numpy().T.astype(np.float64), mats[b]])).float()
        assert _scaled_err(q[b], mo.forward(w, obs, n_obs_in=n_obs)) <= BAR
        del obs
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


# ---- 5. MPNN at 4100 and at the cap ----

@pytest.mark.parametrize("n", [4100, 8192])
def test_forward_large_sizes(n):
    """B = 2: Q finite, the fused act equals the argmax, and Q of episode 0 does not move when episode 1 runs another
    graph under the per-graph norm (an episode offset that overflowed would alias the two)."""
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    from eco_hip._lib import ActConfig, ECO_NORM_PER_GRAPH
    B = 2
    store = GraphStore.random("ER", 2, n, 6.0 / n, seed=n, weights="discrete")
    g = torch.Generator().manual_seed(n)
    net = MPNN(device="cuda")
    net.load_state_dict(mo.init_weights(g, std=0.1))
    x = torch.zeros(B, n, 8)
    x[:, :, :7] = torch.rand(B, n, 7, generator=g) * 2 - 1
    x = x.cuda()
    acts = torch.empty(B, dtype=torch.int32, device="cuda")
    q0 = torch.empty(B, n, device="cuda")
    net.forward_graphs(x, store, torch.tensor([0, 0], dtype=torch.int32, device="cuda"),
                       norm_scope=ECO_NORM_PER_GRAPH, q_out=q0, act=ActConfig(0.0, 1, 0.0, 1, 0), actions_out=acts)
    assert torch.isfinite(q0).all()
    assert torch.equal(acts.long(), q0.argmax(1))
    q1 = net.forward_graphs(x, store, torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                            norm_scope=ECO_NORM_PER_GRAPH)
    assert torch.isfinite(q1).all()
    assert torch.equal(q0[0], q1[0])
    assert not torch.equal(q0[1], q1[1])
    assert float(q0.abs().max()) > 0


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
