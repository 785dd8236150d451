"""Float-weighted graphs (EdgeType.RANDOM) through the batched MaxCut env, against the CPU oracle.

Discrete outputs (spins, dones, the improvement count, Hamming distance, best spins, greedy actions, the time rows)
must match exactly.  Float64 quantities are held to bars derived from the arithmetic, not measured: with
u = 2^-52, A = max_v sum_j |J_vj|, d = the maximum degree and W = sum |J| / 2,
  field / g rows at step t:                      u (N + d + t) A / |mlr|
  score, best_score, unnormalised rewards:       u (t + 1) (N + d + t + 1) W
  nscore, normalised rewards:                    the score bar / qn
  distance-from-best row:                        2 x the score bar / |mlr|
They cover both sides' rounding: an N-term dot product per step on the oracle, a d-term CSR sum plus t row updates
on the engine, and the t-step running sums of score / nscore.  At these shapes they are <= 1e-7, while an f32
slip on a score of order 10^3 gives >= 1e-4.  Each comparison first asserts, on the oracle's own trajectory, that
every nonzero |g| and every nonzero |score - best_score| is >= 1e-6, so no comparison (g > 0, score > best_score)
can legitimately differ.  ECO_STOP_EARLY is not used: a last-ulp difference on an exact revisit may reset it.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import spinsystem_oracle as so
from weighted_common import U, Bars as _Bars, check_rows as _check_rows, ulp32 as _ulp32, well_separated

pytestmark = pytest.mark.gpu


def _graph(n, p, seed, allneg=False):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    w = rng.uniform(-1.0, 1.0, int(keep.sum()))
    if allneg:
        w = -np.abs(w)
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = w
    return m + m.T


def _actions(n, T, seed):
    """Random actions with an immediate revisit (the same vertex again) forced every seventh step."""
    rng = np.random.default_rng(1000 + seed)
    a = rng.integers(0, n, T)
    a[7::7] = a[6::7][:len(a[7::7])]
    return a


def _env_kwargs(n, basis="SIGNED"):
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget, SpinBasis)
    return dict(observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                optimisation_target=OptimisationTarget.CUT,
                spin_basis=SpinBasis.BINARY if basis == "BINARY" else SpinBasis.SIGNED, norm_rewards=True,
                basin_reward=1. / n, reversible_spins=True)


def _oracle_episode(J, T, spins, acts, basis="SIGNED"):
    """The oracle's trajectory + the precondition that makes every comparison unambiguous."""
    n = J.shape[0]
    o = so.SpinSystemOracle(J, T, basin_reward=1. / n, spin_basis=basis)
    o.reset(spins=(spins + 1) // 2 if basis == "BINARY" else spins)
    out = dict(rows=[o.state_rows().copy()], rew=[], done=[], score=[o.score], nscore=[o.normalized_score],
               best=[o.best_score], best_spins=[o.best_spins.copy()], mlr=o.mlr, qn=o.qn, lb=o.lb)
    gmin, gapmin = np.inf, np.inf
    for a in acts:
        _, r, dn, _ = o.step(int(a))
        g = so.calculate_cut_changes(o.state[0], J)
        nz = np.abs(g[g != 0])
        gmin = min(gmin, nz.min() if nz.size else np.inf)
        gap = abs(o.score - o.best_score)
        if gap != 0:
            gapmin = min(gapmin, gap)
        out["rows"].append(o.state_rows().copy())
        out["rew"].append(r); out["done"].append(dn); out["score"].append(o.score)
        out["nscore"].append(o.normalized_score); out["best"].append(o.best_score)
        out["best_spins"].append(o.best_spins.copy())
        if dn:
            break
    assert gmin >= 1e-6 and gapmin >= 1e-6, ("precondition", gmin, gapmin)
    return out


def _run_batched(n, p, B, T, n_graphs=12, steps=None, basis="SIGNED", graphs=None):
    """B episodes on n_graphs float graphs: general path (f64 rows) and FASTOBS path, every episode on the oracle."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    Js = graphs if graphs is not None else [_graph(n, p, s) for s in range(n_graphs)]
    store = GraphStore.from_dense(Js)
    assert store.float_weights
    steps = T if steps is None else steps
    gen = VecSpinSystem(store, B, T, want_f64=True, **_env_kwargs(n, basis))
    fast = VecSpinSystem(store, B, T, want_f64=False, **_env_kwargs(n, basis))
    assert gen.cfg.float_weights == 1
    rng = np.random.default_rng(77)
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    gids = np.arange(B) % len(Js)
    acts = np.stack([_actions(n, steps, e) for e in range(B)])
    gen.reset(graph_ids=gids, spins=spins)
    fast.reset(graph_ids=gids, spins=spins)
    rows = [gen.obs_f64.cpu().numpy()]
    xf = [fast.obs_x.cpu().numpy()]
    xg = [gen.obs_x.cpu().numpy()]
    rew, done, sc = [], [], [gen.read()]
    sc[0] = {k: v.cpu().numpy().copy() for k, v in sc[0].items()}
    for t in range(steps):
        a = torch.from_numpy(acts[:, t].astype(np.int32)).cuda()
        _, r, d = gen.step(a)
        fast.step(a)
        rows.append(gen.obs_f64.cpu().numpy()); xf.append(fast.obs_x.cpu().numpy()); xg.append(gen.obs_x.cpu().numpy())
        rew.append(r.cpu().numpy().copy()); done.append(d.cpu().numpy().copy())
        sc.append({k: v.cpu().numpy().copy() for k, v in gen.read().items()})
    final = gen.read(spins=True, best_spins=True)
    gen.check_errors()
    meta = store.meta.cpu().numpy()
    worst = 0.0
    for e in range(B):
        J = Js[gids[e]]
        o = _oracle_episode(J, T, spins[e], acts[e], basis)
        bars = _Bars(J, o["mlr"], o["qn"])
        # normalisers (score_solver.py:353-375) against numpy
        assert abs(meta[gids[e], 0] - o["mlr"]) <= U * n * bars.A
        assert abs(meta[gids[e], 1] - o["qn"]) <= U * n * n * bars.W and abs(meta[gids[e], 2] - o["lb"]) <= U * n * n * bars.W
        for t in range(len(o["rows"])):
            tag = f"N={n} episode {e} step {t}"
            _check_rows(rows[t][e], o["rows"][t], bars, t, tag)
            # fp32 rows: the general path is the f64 row rounded once; FASTOBS within 1 f32 ulp of that
            ref32 = o["rows"][t].T.astype(np.float32)
            for x, name in ((xg[t][e], "general"), (xf[t][e], "fastobs")):
                np.testing.assert_array_equal(x[:, [0, 2, 4, 5, 6]], ref32[:, [0, 2, 4, 5, 6]], err_msg=f"{tag} {name}")
                assert (np.abs(x[:, [1, 3]].astype(np.float64) - ref32[:, [1, 3]]) <= _ulp32(ref32[:, [1, 3]])).all(), (tag, name)
                assert not x[:, 7].any()
            np.testing.assert_array_equal(xg[t][e][:, :7], rows[t][e].T.astype(np.float32), err_msg=f"{tag} obs_x = f32(obs_f64)")
            sb = bars.score(t)
            assert abs(sc[t]["score"][e] - o["score"][t]) <= sb, (tag, "score")
            assert abs(sc[t]["best_score"][e] - o["best"][t]) <= sb, (tag, "best_score")
            assert abs(sc[t]["normalized_score"][e] - o["nscore"][t]) <= sb / o["qn"], (tag, "nscore")
            worst = max(worst, abs(sc[t]["score"][e] - o["score"][t]) / sb)
            if t > 0:
                assert abs(rew[t - 1][e] - o["rew"][t - 1]) <= sb / o["qn"], (tag, "reward", rew[t - 1][e], o["rew"][t - 1])
                assert bool(done[t - 1][e]) == bool(o["done"][t - 1]), (tag, "done")
        np.testing.assert_array_equal(final["best_spins"][e].cpu().numpy(), o["best_spins"][-1], err_msg=f"episode {e} best spins")
        # best_solution = best score - |lb| (the cut of the best spins)
        cut = so.calculate_cut(o["best_spins"][-1], J)
        assert abs(final["best_solution"][e].item() - cut) <= 2 * bars.score(len(o["rows"]) - 1)
    print(f"N={n}: worst score error / bar = {worst:.3f}")
    return store


@pytest.mark.parametrize("n,p", [(24, 0.3), (70, 0.15), (130, 0.1)])
def test_batched_env_matches_oracle(n, p):
    """VPT 1, 2, 4; B = 64 episodes over the 12 seeded graphs, T = 2N random actions with forced revisits."""
    _run_batched(n, p, 64, 2 * n)


def test_binary_basis_and_all_negative_weights():
    """BINARY spin basis, and a graph with every weight negative (qn = 1, lb < 0) next to ordinary ones."""
    n = 20
    Js = [_graph(n, 0.3, 40 + s, allneg=(s == 0)) for s in range(4)]
    _run_batched(n, 0.3, 8, 2 * n, basis="BINARY", graphs=Js)


def test_dense_rows_take_the_looped_row_update():
    """N = 130, p = 0.7: rows of > 64 edges (row_update's looped branch)."""
    n = 130
    Js = [_graph(n, 0.7, 3)]
    assert (Js[0] != 0).sum(1).max() > 64
    _run_batched(n, 0.7, 4, 2 * n, steps=60, graphs=Js)


def test_n600_vpt16_and_block_per_graph_prepare():
    """N = 600: 16 vertices per lane, and graphs_prepare's one-workgroup-per-graph branch (N > 512)."""
    n = 600
    Js = [_graph(n, 0.02, 5), _graph(n, 0.02, 6)]
    _run_batched(n, 0.02, 4, 2 * n, steps=8, graphs=Js)


def test_greedy_solver_matches_oracle():
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    n, B = 70, 12
    T = 2 * n
    Js = [_graph(n, 0.15, s) for s in range(B)]
    store = GraphStore.from_dense(Js)
    env = VecSpinSystem(store, B, T, **_env_kwargs(n))
    rng = np.random.default_rng(5)
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    env.reset(graph_ids=np.arange(B), spins=spins)
    ref = []
    for b in range(B):
        o = so.SpinSystemOracle(Js[b], T, basin_reward=1. / n)
        o.reset(spins=spins[b])
        # precondition: the two largest gains of every greedy step differ by >= 1e-6 (argmax is unambiguous)
        acts = []
        done = False
        while not done:
            g = so.calculate_cut_changes(o.state[0], Js[b])
            top = np.sort(g)[-2:]
            assert top[1] - top[0] >= 1e-6 and abs(top[1]) >= 1e-6
            if top[1] < 0:
                break
            acts.append(int(g.argmax()))
            _, _, done, _ = o.step(acts[-1])
        ref.append((acts, o))
    got = [[] for _ in range(B)]
    for _ in range(T):
        a = env.greedy_actions()
        dn = env.read()["done"].cpu().numpy().astype(bool)
        if dn.all():
            break
        for b in np.nonzero(~dn)[0]:
            got[b].append(int(a[b].item()))
        env.step(a)
    st = env.read(best_spins=True)
    for b in range(B):
        assert got[b] == ref[b][0], b
        np.testing.assert_array_equal(st["best_spins"][b].cpu().numpy(), ref[b][1].best_spins)
    env.check_errors()


def test_normalisers_against_numpy_and_reproducible():
    """meta = {max nonzero row sum, max(1, sum_{w>0} w / 2), min(0, sum_{w<0} w / 2), sum w}; deg = nonzeros per row;
    two identical runs give bitwise-equal meta, observations and rewards."""
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    outs = []
    for n, p, G in ((70, 0.15, 9), (600, 0.02, 3)):
        Js = [_graph(n, p, 20 + s) for s in range(G)]
        Js.append(_graph(n, p, 99, allneg=True))
        runs = []
        for _ in range(2):
            store = GraphStore.from_dense(Js)
            env = VecSpinSystem(store, 8, 2 * n, want_f64=True, **_env_kwargs(n))
            env.reset(graph_ids=np.arange(8) % len(Js), seed=3)
            rec = [store.meta.clone(), env.obs_f64.clone(), env.obs_x.clone()]
            for t in range(10):
                a = torch.full((8,), (7 * t) % n, dtype=torch.int32, device="cuda")
                _, r, _ = env.step(a)
                rec += [env.obs_f64.clone(), r.clone()]
            env.check_errors()
            runs.append(rec)
        for x, y in zip(*runs):
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                               y.view(torch.int64) if y.dtype == torch.float64 else y)
        meta = runs[0][0].cpu().numpy()
        deg = store.deg.cpu().numpy()
        for g, J in enumerate(Js):
            rs = J.sum(1)
            A, W = np.abs(J).sum(1).max(), np.abs(J).sum() / 2
            assert abs(meta[g, 0] - rs[rs != 0].max()) <= U * n * A
            assert abs(meta[g, 1] - max(1, J[J > 0].sum() / 2)) <= U * n * n * W
            assert abs(meta[g, 2] - min(0, J[J < 0].sum() / 2)) <= U * n * n * W
            assert abs(meta[g, 3] - J.sum()) <= 2 * U * n * n * W
            np.testing.assert_array_equal(deg[g], (J != 0).sum(1))
            assert store.valid[g].item() == 1
            np.testing.assert_array_equal(store.dense(g), J)
        assert meta[-1, 1] == 1.0 and meta[-1, 0] < 0      # all-negative weights: qn = 1, mlr < 0
        outs.append(meta)


def test_masked_reset_touches_only_masked_episodes():
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    n, B = 24, 8
    Js = [_graph(n, 0.3, s) for s in range(4)]
    store = GraphStore.from_dense(Js)
    env = VecSpinSystem(store, B, 2 * n, want_f64=True, **_env_kwargs(n))
    env.reset(graph_ids=np.arange(B) % 4, seed=1)
    for t in range(5):
        env.step(torch.full((B,), t, dtype=torch.int32, device="cuda"))
    before = env.obs_f64.clone()
    sc0 = env.read()["score"].clone()
    mask = np.array([1, 0, 0, 1, 0, 0, 0, 1], np.uint8)
    spins = -np.ones((B, n), np.int64)
    env.reset(graph_ids=(np.arange(B) + 1) % 4, spins=spins, mask=mask)
    after, sc1 = env.obs_f64, env.read()
    for e in range(B):
        if mask[e]:
            o = so.SpinSystemOracle(Js[(e + 1) % 4], 2 * n, basin_reward=1. / n)
            o.reset(spins=spins[e])
            ok, mins = well_separated(Js[(e + 1) % 4], [o.state[0]], [o.score], [o.best_score])
            assert ok, ("precondition", mins)
            bars = _Bars(Js[(e + 1) % 4], o.mlr, o.qn)
            _check_rows(after[e].cpu().numpy(), o.state_rows(), bars, 0, f"masked reset {e}")
            assert abs(sc1["score"][e].item() - o.score) <= bars.score(0)
            assert sc1["current_step"][e].item() == 0
        else:
            assert torch.equal(after[e], before[e]) and sc1["score"][e].item() == sc0[e].item()
            assert sc1["current_step"][e].item() == 5
    env.check_errors()


def _drop_in_against(env, M, T, spins, acts, basis, records=None):
    """Drive a core.make env (already reset on `spins`) and compare it with the oracle -- or with a recorded
    reference trajectory -- after asserting the precondition on that trajectory."""
    n = M.shape[0]
    o = so.SpinSystemOracle(M, T, basin_reward=1. / n, spin_basis=basis)
    o.reset(spins=spins)
    traj = [dict(rows=o.state_rows().copy(), score=o.score, best=o.best_score, s=o.state[0].copy())]
    for a in acts:
        _, r, d, _ = o.step(int(a))
        traj.append(dict(rows=o.state_rows().copy(), score=o.score, best=o.best_score, s=o.state[0].copy(), rew=r,
                         done=d))
        if d:
            break
    ok, mins = well_separated(M, [x["s"] for x in traj], [x["score"] for x in traj], [x["best"] for x in traj])
    assert ok, ("precondition", mins)
    if records is not None:      # the reference's own rows / scores / rewards instead of the oracle's
        for t, x in enumerate(traj):
            x["rows"], x["score"] = records["obs"][t], records["score"][t]
            if t:
                x["rew"], x["done"] = records["rew"][t - 1], bool(records["done"][t - 1])
    bars = _Bars(M, o.mlr, o.qn)
    _check_rows(env.get_observation()[:7], traj[0]["rows"], bars, 0, "core.make reset")
    for t, x in enumerate(traj[1:], 1):
        obs, r, d, _ = env.step(int(acts[t - 1]))
        _check_rows(obs[:7], x["rows"], bars, t, f"core.make step {t}")
        np.testing.assert_array_equal(obs[7:], M)
        assert abs(r - x["rew"]) <= bars.score(t) / o.qn and d == x["done"]
        assert abs(env.score - x["score"]) <= bars.score(t)
    assert abs(env.best_solution - so.calculate_cut(o.best_spins, M)) <= 2 * bars.score(len(traj))
    np.testing.assert_array_equal(env.best_spins, o.best_spins)


def test_single_env_drop_in_runs_random_and_single_graph_generators():
    """core.make with RandomErdosRenyiGraphGenerator(edge_type=RANDOM) (its graph drawn from the seeded global
    numpy stream, as the reference draws it) and SingleGraphGenerator on a float matrix."""
    from eco_hip.envs import core
    from eco_hip.envs.utils import EdgeType, RandomErdosRenyiGraphGenerator, SingleGraphGenerator
    n = 20
    for gg in (SingleGraphGenerator(_graph(n, 0.3, 8)), RandomErdosRenyiGraphGenerator(n, [0.3, 0], EdgeType.RANDOM)):
        assert gg.edge_type == EdgeType.RANDOM
        np.random.seed(3)
        env = core.make("SpinSystem", gg, 2 * n, **_env_kwargs(n))
        spins = 2 * np.random.default_rng(9).integers(0, 2, n) - 1
        env.reset(spins=spins)
        M = np.asarray(env.matrix, dtype=np.float64)
        assert (M[M != 0] != np.round(M[M != 0])).all()
        _drop_in_against(env, M, 2 * n, spins, _actions(n, 2 * n, 4), "SIGNED")


def _fixture_case(f, c):
    p = f"c{c}_"
    rec = {k: f[p + k] for k in ("obs", "rew", "done", "score", "nscore", "best_score", "best_nscore",
                                 "best_solution")}
    return f[p + "J"], int(f[p + "T"]), str(f[p + "basis"]), f[p + "spins"].astype(np.int64), f[p + "actions"], rec


@pytest.mark.parametrize("case", [0, 1, 2])
def test_reference_fixture_cases_through_vecspinsystem(case):
    """tests/golden/weighted.npz (recorded from the reference): revisits, BINARY basis, all-negative weights."""
    import os
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    f = np.load(os.path.join(GOLDEN, "weighted.npz"))
    J, T, basis, sp, acts, rec = _fixture_case(f, case)
    n = J.shape[0]
    signed = 2 * sp - 1 if basis == "BINARY" else sp
    # precondition, on the reference's trajectory (its spin rows replayed from the recorded actions)
    srows, s = [signed.astype(np.float64)], signed.astype(np.float64).copy()
    for a in acts[:len(rec["rew"])]:
        s = s.copy(); s[a] = -s[a]; srows.append(s)
    ok, mins = well_separated(J, srows, rec["score"], rec["best_score"])
    assert ok, ("precondition", mins)
    bars = _Bars(J, float(f[f"c{case}_mlr"]), float(f[f"c{case}_qn"]))
    qn = float(f[f"c{case}_qn"])
    store = GraphStore.from_dense([J])
    for want_f64 in (True, False):                            # general and FASTOBS step kernels
        env = VecSpinSystem(store, 1, T, want_f64=want_f64, **_env_kwargs(n, basis))
        env.reset(graph_ids=[0], spins=signed[None])
        act = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t in range(len(rec["rew"]) + 1):
            if t:
                act.fill_(int(acts[t - 1]))
                _, r, d = env.step(act)
                assert abs(r.item() - rec["rew"][t - 1]) <= bars.score(t) / qn, (case, t, "reward")
                assert bool(d.item()) == bool(rec["done"][t - 1])
            ref32 = rec["obs"][t].T.astype(np.float32)
            x = env.obs_x[0].cpu().numpy()
            np.testing.assert_array_equal(x[:, [0, 2, 4, 5, 6]], ref32[:, [0, 2, 4, 5, 6]])
            assert (np.abs(x[:, [1, 3]].astype(np.float64) - ref32[:, [1, 3]]) <= _ulp32(ref32[:, [1, 3]])).all()
            st = env.read()
            sb = bars.score(t)
            for key, fk, div in (("score", "score", 1), ("best_score", "best_score", 1), ("normalized_score", "nscore", qn),
                                 ("best_score_normalized", "best_nscore", qn), ("best_solution", "best_solution", 0.5)):
                assert abs(st[key][0].item() - rec[fk][t]) <= sb / div, (case, t, key)
            if want_f64:
                _check_rows(env.obs_f64[0].cpu().numpy(), rec["obs"][t], bars, t, f"fixture case {case} step {t}")
        meta = store.meta[0].cpu().numpy()
        assert abs(meta[0] - f[f"c{case}_mlr"]) <= U * n * bars.A
        assert abs(meta[1] - qn) <= U * n * n * bars.W and abs(meta[2] - f[f"c{case}_lb"]) <= U * n * n * bars.W
        env.check_errors()


def test_reference_fixture_case_through_core_make():
    """The all-negative-weights case (mlr < 0) through the single-env drop-in, against the reference's records."""
    import os
    from eco_hip.envs import core
    from eco_hip.envs.utils import SingleGraphGenerator
    f = np.load(os.path.join(GOLDEN, "weighted.npz"))
    J, T, basis, sp, acts, rec = _fixture_case(f, 2)
    env = core.make("SpinSystem", SingleGraphGenerator(J), T, **_env_kwargs(J.shape[0], basis))
    env.reset(spins=sp)
    assert env.scorer._max_local_reward < 0
    _drop_in_against(env, J, T, sp, acts[:len(rec["rew"])], basis, records=rec)


def test_everything_that_cannot_take_weights_says_so_before_any_launch():
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore, edge_cap
    from eco_hip.envs.batched import VecSpinSystem, make_config
    from eco_hip.envs.utils import ExtraAction, OptimisationTarget, MAIN_OBSERVABLES, RewardSignal
    n, B = 20, 4
    fstore = GraphStore.from_dense([_graph(n, 0.3, 1)])
    istore = GraphStore.random("ER", 1, n, 0.3, seed=1)
    s = _lib.stream_ptr()

    def rc_msg(rc, frag):
        assert rc == _lib.ECO_ERR_ARG and frag in _lib.last_error(), (rc, _lib.last_error())

    # generic-scorer targets
    for t in (OptimisationTarget.MIN_COVER, OptimisationTarget.MIN_CUT, OptimisationTarget.MAX_IND_SET,
              OptimisationTarget.MAX_CLIQUE, OptimisationTarget.MIN_DOM_SET):
        with pytest.raises(ValueError, match="CUT only"):
            VecSpinSystem(fstore, B, 2 * n, extra_action=ExtraAction.NONE, optimisation_target=t,
                          reward_signal=RewardSignal.BLS)
        # through the C ABI: an integer config of that target on the weighted set
        env = VecSpinSystem(istore, B, 2 * n, extra_action=ExtraAction.NONE, optimisation_target=t,
                            reward_signal=RewardSignal.BLS)
        gid = torch.zeros(B, dtype=torch.int32, device="cuda")
        rc_msg(_lib.lib.eco_env_reset(ctypes.byref(env.cfg), ctypes.byref(fstore.gs), _lib.ptr(env.state), B,
                                      _lib.ptr(gid), None, None, 0, _lib.ptr(env.obs_x), None, s), "float")
    # the flag must agree with the set, both ways, in reset, step and greedy
    ienv = VecSpinSystem(istore, B, 2 * n, **_env_kwargs(n))
    fenv = VecSpinSystem(fstore, B, 2 * n, **_env_kwargs(n))
    gid = torch.zeros(B, dtype=torch.int32, device="cuda")
    act = torch.zeros(B, dtype=torch.int32, device="cuda")
    for env, store in ((ienv, fstore), (fenv, istore)):
        rc_msg(_lib.lib.eco_env_reset(ctypes.byref(env.cfg), ctypes.byref(store.gs), _lib.ptr(env.state), B,
                                      _lib.ptr(gid), None, None, 0, _lib.ptr(env.obs_x), None, s), "float")
        rc_msg(_lib.lib.eco_env_step(ctypes.byref(env.cfg), ctypes.byref(store.gs), _lib.ptr(env.state), B,
                                     _lib.ptr(act), _lib.ptr(env.rewards), _lib.ptr(env.dones), _lib.ptr(env.obs_x),
                                     None, s), "float")
        rc_msg(_lib.lib.eco_env_greedy_actions(ctypes.byref(env.cfg), ctypes.byref(store.gs), _lib.ptr(env.state), B,
                                               _lib.ptr(act), s), "float")
    # compact replay ring
    ring = torch.zeros(_lib.lib.eco_replay_compact_bytes(n, 64, B), dtype=torch.uint8, device="cuda")
    fenv.reset(graph_ids=gid, seed=0)
    rc_msg(_lib.lib.eco_replay_compact_snapshot(ctypes.byref(fenv.cfg), _lib.ptr(fenv.state), B, _lib.ptr(ring), 64, 0,
                                                None, s), "compact replay")
    rc_msg(_lib.lib.eco_replay_compact_push(ctypes.byref(fenv.cfg), _lib.ptr(fenv.state), B, _lib.ptr(ring), 64, 0,
                                            _lib.ptr(act), _lib.ptr(fenv.rewards), _lib.ptr(fenv.dones), s),
           "compact replay")
    buf = torch.zeros(B * n * 8, device="cuda")
    for cfg, store in ((fenv.cfg, fstore), (ienv.cfg, fstore)):
        rc_msg(_lib.lib.eco_replay_compact_sample(ctypes.byref(cfg), _lib.ptr(fenv.state), ctypes.byref(store.gs), B,
                                                  _lib.ptr(ring), 64, 4, 8, 2, 0, 0, _lib.ptr(buf), _lib.ptr(buf),
                                                  _lib.ptr(act), _lib.ptr(act), _lib.ptr(buf), _lib.ptr(buf), s),
               "compact replay")
    # edge_weights together with unit_weights
    bad = _lib.GraphSet(*[getattr(fstore.gs, f) for f, _ in _lib.GraphSet._fields_])
    bad.unit_weights = 1
    rc_msg(_lib.lib.eco_graphs_prepare(ctypes.byref(bad), s), "unit_weights")
    # generation: kind 2 needs edge_weights, the integer kinds must not have them, unknown kinds
    slots_i = GraphStore.slots(2, n, edge_cap("ER", n, 0.3))
    slots_f = GraphStore.slots(2, n, edge_cap("ER", n, 0.3), weights="random")
    ws = torch.empty(_lib.lib.eco_graphs_generate_workspace_bytes(n, 2), dtype=torch.uint8, device="cuda")
    for st, kind, frag in ((slots_i, 2, "edge_weights"), (slots_f, 1, "float-weighted"), (slots_i, 3, "weight kind")):
        rc_msg(_lib.lib.eco_graphs_generate(ctypes.byref(st.gs), 0, 2, _lib.ECO_GRAPH_ER, 0.3, kind, 1, st.cap,
                                            _lib.ptr(ws), s), frag)
    with pytest.raises(ValueError):
        slots_i.generate(0, 2, "ER", 0.3, 1, weights="random")
    fenv.check_errors()
    # 9..16 observables are fine on the CSR path: an env with MAIN_OBSERVABLES minus the mask rows runs
    obs = [o for o in MAIN_OBSERVABLES if o.value not in (3, 4, 9)]
    kw = _env_kwargs(n)
    kw["observables"] = obs
    wide = VecSpinSystem(fstore, B, 2 * n, **kw)
    x = wide.reset(graph_ids=gid, seed=1)
    assert x.shape[-1] == 16 and torch.isfinite(x).all()
    wide.check_errors()
