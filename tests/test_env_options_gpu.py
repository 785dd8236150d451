"""The env kernels under every reward / stopping / horizon / stagnation setting of eco_env_config, against the CPU
oracles (tests/env_options_common.py: rows A-I, the scripted actions and the events each row must show;
tests/test_env_options_cpu.py pins both oracles to the reference on the same rows).

Families and bars:
  * integer CUT, general kernels (want_f64): float64 rows bitwise (as uint64), rewards, dones and read() scalars
    equal after every step, every episode on the oracle; the recorded reference cases replayed as well;
  * integer CUT, fp32-only path: rewards, dones, scalars exact, obs_x bitwise equal to the general path's
    (the rule of test_env_gpu.test_fp32_rows_without_f64_match_the_general_path);
  * auto-mask and masked reset of finished episodes, then 20 more steps;
  * float-weighted CUT: discrete outputs exact, float64 quantities within weighted_common.Bars;
  * generic-scorer targets: the rule of tests/test_problems_gpu.py (== on float64 rows, rewards, scores; obs_x the
    rows rounded to float32);
  * workgroup-per-episode kernels at N = 2049 against the oracle's sparse mode, bit-exact;
  * compact replay rings with horizon_length = 7: sample and gather bitwise equal to the feature ring.
"""
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import env_options_common as ec
from conftest import GOLDEN
from oracle import spinsystem_oracle as so
from weighted_common import Bars, check_rows, well_separated

pytestmark = pytest.mark.gpu

B = 8
N_GRAPHS = 3
ALL_ROWS = "ABCDEFGHI"


def _utils():
    import eco_hip.envs.utils as u
    return u


def _T(n, row, t4=False):
    """2 N, and 160 at N = 300 -- except row H there, whose "no spin left" stop at step N needs N < T."""
    if row == "I":
        return 4 if t4 else 3
    return 160 if n == 300 and row != "H" else 2 * n


class Episode:
    """One episode's script and oracle trajectory."""

    def __init__(self, J, gid, T, row, target, spins, acts):
        self.gid, self.spins, self.acts, self.J = gid, np.asarray(spins, dtype=np.int64), acts, J
        o = ec.make_oracle(J, T, row, target)
        self.tr = ec.run_oracle(o, self.spins, acts, ec.ti_index(ec.o_observables(o)))
        self.mlr, self.qn = (o.mlr, o.qn) if target == "CUT" else (o.scorer.mlr, o.scorer.qn)
        self.k = 0     # steps taken

    @property
    def finished(self):
        return self.k == self.tr["steps"] and self.tr["done"][-1]


class Case:
    """B episodes of one (family, N, row, T) on N_GRAPHS graphs, with the row's events asserted on the oracle."""

    def __init__(self, family, target, n, row, T, n_envs=B):
        self.family, self.target, self.n, self.row, self.T, self.B = family, target, n, row, T, n_envs
        base = zlib.crc32(f"{family}/{target}/{n}/{T}".encode()) % 10 ** 6
        last = None
        for attempt in range(16):       # another seed if this one misses an event; the assertion stays
            seed = base + 7919 * attempt
            self._build(seed)
            try:
                self.events = ec.assert_events(row, [e.tr for e in self.eps], T, n)
                return
            except AssertionError as err:
                last = err
        raise last

    def graph(self, seed):
        if self.family == "float":
            return ec.float_graph(self.n, seed)
        if self.family == "wg":
            return so.SparseMatrix.from_dense(ec.cut_graph(self.n, seed))
        if self.target == "CUT":
            return ec.cut_graph(self.n, seed)
        return ec.problem_graph(self.n, seed, self.target)

    def _build(self, seed):
        ng = 1 if self.family == "wg" else N_GRAPHS
        self.Js = [self.graph(seed + g) for g in range(ng)]
        self.eps = []
        for b in range(self.B):
            J = self.Js[b % ng]
            for attempt in range(64):
                s = seed + 1000 * attempt
                if self.family == "wg" and ec.ROWS[self.row]["reversible"]:
                    spins = ec.near_optimum_spins(J, s + 100 + b)
                else:
                    spins = ec.start_spins(self.n, s + 100 + b, self.row)
                acts = ec.script(J, self.T, self.row, spins, s + 200 + b, self.target)
                ep = Episode(J, b % ng, self.T, self.row, self.target, spins, acts)
                # float weights: an exact return to the best state leaves |score - best| at rounding level, where
                # score > best_score is ambiguous; such an episode takes another seed (the test asserts the
                # precondition on the episodes it runs)
                if self.family != "float" or well_separated(J, ep.tr["spins"], ep.tr["score"], ep.tr["best_score"])[0]:
                    break
            self.eps.append(ep)

    def dense(self, g):
        J = self.Js[g]
        if not isinstance(J, so.SparseMatrix):
            return J
        m = np.zeros(J.shape)
        m[J.row, J.col] = J.val
        return m


@functools.lru_cache(maxsize=None)
def _case(family, target, n, row, T, n_envs=B):
    return Case(family, target, n, row, T, n_envs)


def _observables(target):
    u = _utils()
    return u.DEFAULT_OBSERVABLES if target == "CUT" else ec.problem_observables(u, target)


def _make_env(case, want_f64=True, **over):
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.graphs import GraphStore
    store = GraphStore.from_dense([case.dense(g) for g in range(len(case.Js))])
    assert bool(store.float_weights) == (case.family == "float")
    kw = ec.env_kwargs(_utils(), case.row, case.n, case.T, case.target, _observables(case.target), **over)
    return VecSpinSystem(store, case.B, case.T, want_f64=want_f64, **kw)


def _snapshot(env):
    st = env.read()
    out = {k: st[k].cpu().numpy().copy() for k in
           ("current_step", "score", "normalized_score", "best_score", "best_score_normalized", "best_solution", "done")}
    out["rows"] = env.obs_f64.cpu().numpy() if env.obs_f64 is not None else None
    out["x"] = env.obs_x.cpu().numpy()
    out["rew"] = env.rewards.cpu().numpy().copy()
    out["dones"] = env.dones.cpu().numpy().copy()
    return out


# ---- the comparison rules ----

def _cmp_exact(snap, b, ep, t, tag, stepped):
    tr = ep.tr
    if snap["rows"] is not None:
        np.testing.assert_array_equal(snap["rows"][b].view(np.uint64), tr["rows"][t].view(np.uint64), err_msg=str(tag))
        k = tr["rows"][t].shape[0]
        np.testing.assert_array_equal(snap["x"][b][:, :k], tr["rows"][t].T.astype(np.float32), err_msg=str(tag))
        assert not snap["x"][b][:, k:].any(), tag
    for key in ec.SCALARS:
        assert snap[key][b] == tr[key][t], (tag, key, snap[key][b], tr[key][t])
    assert snap["current_step"][b] == t, tag
    if stepped:
        assert snap["rew"][b] == tr["rew"][t - 1], (tag, "reward", snap["rew"][b], tr["rew"][t - 1])
        assert bool(snap["dones"][b]) == tr["done"][t - 1] == bool(snap["done"][b]), (tag, "done")


def _cmp_problems(snap, b, ep, t, tag, stepped):
    """tests/test_problems_gpu.py: rows, rewards and scores equal (==); obs_x = the float64 rows rounded to fp32."""
    tr = ep.tr
    np.testing.assert_array_equal(snap["rows"][b], tr["rows"][t], err_msg=str(tag))
    n_obs = tr["rows"][t].shape[0]
    np.testing.assert_array_equal(snap["x"][b][:, :n_obs], snap["rows"][b].T.astype(np.float32), err_msg=str(tag))
    assert not snap["x"][b][:, n_obs:].any(), tag
    for key in ec.SCALARS:
        assert snap[key][b] == tr[key][t], (tag, key, snap[key][b], tr[key][t])
    if stepped:
        assert snap["rew"][b] == tr["rew"][t - 1], (tag, "reward", snap["rew"][b], tr["rew"][t - 1])
        assert bool(snap["dones"][b]) == tr["done"][t - 1], (tag, "done")


def _cmp_float(norm):
    def cmp(snap, b, ep, t, tag, stepped):
        tr = ep.tr
        bars = Bars(ep.J, ep.mlr, ep.qn)
        check_rows(snap["rows"][b], tr["rows"][t], bars, t, str(tag))
        sb = bars.score(t)
        assert abs(snap["score"][b] - tr["score"][t]) <= sb, (tag, "score")
        assert abs(snap["best_score"][b] - tr["best_score"][t]) <= sb, (tag, "best_score")
        assert abs(snap["normalized_score"][b] - tr["normalized_score"][t]) <= sb / ep.qn, (tag, "nscore")
        assert abs(snap["best_score_normalized"][b] - tr["best_score_normalized"][t]) <= sb / ep.qn, (tag, "best nscore")
        assert abs(snap["best_solution"][b] - tr["best_solution"][t]) <= 2 * sb, (tag, "best_solution")
        assert snap["current_step"][b] == t, tag
        if stepped:
            # the basin reward and the stagnation punishment add exactly representable constants: the score bar holds
            bar = sb / ep.qn if norm else sb
            assert abs(snap["rew"][b] - tr["rew"][t - 1]) <= bar, (tag, "reward", snap["rew"][b], tr["rew"][t - 1])
            assert bool(snap["dones"][b]) == tr["done"][t - 1], (tag, "done")
    return cmp


def _assert_masked(snap, prev, b, tag):
    """A finished episode stepped again: reward 0, done 1, rows and scalars unchanged."""
    assert snap["rew"][b] == 0.0 and snap["dones"][b] == 1 and snap["done"][b] == 1, tag
    for key in ec.SCALARS + ("current_step",):
        assert snap[key][b] == prev[key][b], (tag, key)
    if snap["rows"] is not None:
        np.testing.assert_array_equal(snap["rows"][b].view(np.uint64), prev["rows"][b].view(np.uint64), err_msg=str(tag))
    np.testing.assert_array_equal(snap["x"][b].view(np.uint32), prev["x"][b].view(np.uint32), err_msg=str(tag))


def _step_all(envs, eps, cmp, snap, fast=None):
    """One env step of every episode (a finished or exhausted one replays action 0) and its comparison."""
    env = envs[0]
    acts = np.array([int(e.acts[e.k]) if e.k < e.tr["steps"] else 0 for e in eps], dtype=np.int32)
    a = torch.from_numpy(acts).cuda()
    for v in envs:
        v.step(a)
    new = _snapshot(env)
    if fast is not None:    # the fp32-only path: obs_x, rewards and dones bitwise those of the general path
        assert torch.equal(fast.obs_x.view(torch.int32), env.obs_x.view(torch.int32))
        assert torch.equal(fast.rewards.view(torch.int64), env.rewards.view(torch.int64))
        assert torch.equal(fast.dones, env.dones)
        fs = _snapshot(fast)
    for b, e in enumerate(eps):
        tag = (b, e.k + 1)
        if e.finished:
            _assert_masked(new, snap, b, tag)
            if fast is not None:
                assert fs["rew"][b] == 0.0 and fs["dones"][b] == 1
        elif e.k < e.tr["steps"]:
            e.k += 1
            cmp(new, b, e, e.k, tag, True)
            if fast is not None:
                _cmp_exact(fs, b, e, e.k, tag + ("fast",), True)
    return new


def _run(case, cmp, want_f64=True, with_fast=False):
    """Whole episodes: reset, every step of every episode against its oracle trajectory, finished episodes stepped on
    (auto-mask) until the last one has ended and once more."""
    env = _make_env(case)
    envs = [env]
    fast = None
    if with_fast:
        fast = _make_env(case, want_f64=False)
        envs.append(fast)
    eps = case.eps
    for e in eps:
        e.k = 0
    gids = np.array([e.gid for e in eps])
    spins = np.stack([e.spins for e in eps])
    for v in envs:
        v.reset(graph_ids=gids, spins=spins)
        v.check_errors()
    snap = _snapshot(env)
    for b, e in enumerate(eps):
        cmp(snap, b, e, 0, (b, 0), False)
    if fast is not None:
        assert torch.equal(fast.obs_x.view(torch.int32), env.obs_x.view(torch.int32))
    for _ in range(max(e.tr["steps"] for e in eps) + 1):
        snap = _step_all(envs, eps, cmp, snap, fast)
    assert all(e.finished for e in eps) and snap["dones"].all()
    for v in envs:
        v.check_errors()
    return env


# ---- integer CUT ----

CUT_PARAMS = [(n, r, False) for n in (20, 65, 300) for r in ALL_ROWS] + [(n, "I", True) for n in (20, 65, 300)]


@pytest.mark.parametrize("n,row,t4", CUT_PARAMS)
def test_integer_cut_general_kernel(n, row, t4):
    """N = 20 (1 vertex per lane), 65 (2 per lane, one vertex in the second slot), 300 (8 per lane); B = 8 episodes
    on 3 graphs with their own start spins and scripts."""
    case = _case("cut", "CUT", n, row, _T(n, row, t4))
    print(n, row, case.T, case.events)
    _run(case, _cmp_exact)


@pytest.mark.parametrize("n", [20, 300])
@pytest.mark.parametrize("row", list("ACDEH"))
def test_integer_cut_fp32_path(n, row):
    """want_f64=False with DEFAULT_OBSERVABLES: env_step_fast_kernel<1> at N = 20, env_step_kernel<8, true> at 300."""
    case = _case("cut", "CUT", n, row, _T(n, row))
    _run(case, _cmp_exact, with_fast=True)


F = np.load(os.path.join(GOLDEN, "env_options.npz"))
GOLDEN_CUT = [ci for ci in range(int(F["n_cases"])) if str(F[f"c{ci}_target"]) == "CUT"]


@pytest.mark.parametrize("ci", GOLDEN_CUT)
def test_integer_cut_replays_the_reference(ci):
    """tests/golden/env_options.npz: the reference's own rewards, dones, scalars, row digests and stored rows."""
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.graphs import GraphStore
    p = f"c{ci}_"
    row, T, J = str(F[p + "row"]), int(F[p + "T"]), F[p + "J"].astype(np.float64)
    n = J.shape[0]
    env = VecSpinSystem(GraphStore.from_dense([J]), 1, T, want_f64=True,
                        **ec.env_kwargs(_utils(), row, n, T, "CUT"))
    env.reset(graph_ids=[0], spins=F[p + "spins"].astype(np.int64)[None])
    steps = [int(s) for s in F[p + "obs_steps"]]
    rews = F[p + "rew"]
    act = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in range(len(rews) + 1):
        if t:
            act.fill_(int(F[p + "actions"][t - 1]))
            _, r, d = env.step(act)
            assert r.item() == rews[t - 1] and bool(d.item()) == bool(F[p + "done"][t - 1]), (ci, t)
        rows = env.obs_f64[0].cpu().numpy()
        assert ec.digest(rows) == F[p + "obs_digest"][t], (ci, t)
        if t in steps:
            np.testing.assert_array_equal(rows.view(np.uint64), F[p + "obs_at"][steps.index(t)].view(np.uint64))
        st = env.read()
        for key in ec.SCALARS:
            assert st[key][0].item() == F[p + key][t], (ci, t, key)
    assert bool(F[p + "done"][-1])
    env.check_errors()


# ---- auto-mask and masked reset ----

def _plan_masked_reset(case):
    """(episodes, steps to run before the reset, indices of the episodes finished by then, their replacements)."""
    n, row = case.n, case.row
    eps = [Episode.__new__(Episode) for _ in case.eps]
    for e, src in zip(eps, case.eps):
        e.__dict__.update(src.__dict__)
        e.k = 0
    run = sorted(e.tr["steps"] for e in eps)[case.B // 2 - 1] + 1
    fin = [b for b, e in enumerate(eps) if e.tr["steps"] <= run]
    assert len(fin) >= case.B // 2
    if row == "C":
        assert len(fin) < case.B, "EARLY: some episodes must still be running at the masked reset"
    rev = ec.ROWS[row]["reversible"]
    resets = {}
    # the episode that replays its own start and script: one whose first four steps visit new states only
    replay = next(b for b in fin if not rev or not any(eps[b].tr["revisit"][:4]))
    others = [b for b in fin if b != replay]
    for b in fin:
        old = eps[b]
        g = (old.gid + 1) % N_GRAPHS
        J = case.Js[g]
        if b == replay or not rev:
            resets[b] = Episode(J, g, case.T, row, "CUT", old.spins, old.acts[:20])
        elif b == others[0]:
            for seed in range(16):   # a start in a local optimum that no later state of the tail improves on
                sp = ec.local_optimum(J, ec.start_spins(n, 31 * n + b + 1000 * seed, row))
                e = Episode(J, g, case.T, row, "CUT", sp, ec.random_tail(n, 20, np.random.default_rng(n + b + seed)))
                if not any(e.tr["improved"][:15]):
                    break
            resets[b] = e
        else:
            sp = ec.start_spins(n, 77 * n + b, row)
            resets[b] = Episode(J, g, case.T, row, "CUT", sp, ec.script(J, case.T, row, sp, 55 * n + b, steps=20))
    if row == "C":
        e = resets[others[0]]
        assert e.tr["steps"] == 15 and e.tr["done"][-1] and not any(e.tr["improved"]), "EARLY from a fresh counter"
        assert not any(resets[replay].tr["revisit"][:4])     # new states, unless the visited set was kept
    return eps, run, fin, resets


@pytest.mark.parametrize("n", [20, 65])
@pytest.mark.parametrize("row", list(ALL_ROWS))
def test_auto_mask_and_masked_reset(n, row):
    """Run until half the episodes have finished (all of them under the rows whose episodes end together), step once
    more (the finished ones must not move), reset only the finished ones onto another graph with new spins, then 20
    more steps: the reset episodes against fresh oracles, the others against their continuing ones.  Of the reset
    episodes the first replays its earlier start spins and script on the new graph -- a visited set that was not
    emptied would call those states revisits -- and the second starts in a local optimum and takes the random tail, so
    that 15 steps without an improvement end it under EARLY only if the counter started again from zero."""
    case = _case("cut", "CUT", n, row, _T(n, row))
    eps, run, fin, resets = _plan_masked_reset(case)
    env = _make_env(case)
    env.reset(graph_ids=np.array([e.gid for e in eps]), spins=np.stack([e.spins for e in eps]))
    snap = _snapshot(env)
    for _ in range(run):
        snap = _step_all([env], eps, _cmp_exact, snap)
    assert fin == [b for b, e in enumerate(eps) if e.finished]
    mask = np.zeros(case.B, np.uint8)
    mask[fin] = 1
    gids = np.array([e.gid for e in eps])
    spins = np.stack([e.spins for e in eps])
    for b in fin:
        eps[b] = resets[b]
        gids[b], spins[b] = eps[b].gid, eps[b].spins
    env.reset(graph_ids=gids, spins=spins, mask=mask)
    new = _snapshot(env)
    for b, e in enumerate(eps):
        if mask[b]:
            _cmp_exact(new, b, e, 0, (b, "reset"), False)
            assert new["done"][b] == 0 and new["dones"][b] == 0
        else:
            moved = [k for k in ec.SCALARS + ("current_step", "done") if new[k][b] != snap[k][b]]
            assert not moved, (b, moved)
            np.testing.assert_array_equal(new["rows"][b].view(np.uint64), snap["rows"][b].view(np.uint64))
    snap = new
    for _ in range(20):
        snap = _step_all([env], eps, _cmp_exact, snap)
    assert all(eps[b].k == eps[b].tr["steps"] for b in fin)
    env.check_errors()


# ---- float-weighted CUT ----

@pytest.mark.parametrize("n", [20, 65])
@pytest.mark.parametrize("row", list("ABDEFH"))
def test_float_weighted_cut(n, row):
    """EARLY is left out (a last-ulp difference on an exact revisit may reset its counter, see
    tests/test_weighted_env_gpu.py).  Precondition on every oracle trajectory: nonzero |g| and |score - best| are
    >= 1e-6, so no comparison can legitimately differ."""
    case = _case("float", "CUT", n, row, _T(n, row))
    for e in case.eps:
        ok, mins = well_separated(e.J, e.tr["spins"], e.tr["score"], e.tr["best_score"])
        assert ok, ("precondition", mins)
    _run(case, _cmp_float(ec.ROWS[row]["norm"]))


# ---- generic-scorer targets ----

PROBLEM_PARAMS = ([(t, 20) for t in ("MIN_COVER", "MAX_IND_SET", "MAX_CLIQUE", "MIN_DOM_SET", "MIN_CUT")] +
                  [("MIN_COVER", 65), ("MIN_DOM_SET", 65)])


@pytest.mark.parametrize("target,n", PROBLEM_PARAMS)
@pytest.mark.parametrize("row", list("ABCDE"))
def test_generic_scorer_targets(target, n, row):
    """Rows A-D, and row E so that this family's own horizon_length expression is held to the oracle as well."""
    case = _case("problems", target, n, row, _T(n, row))
    _run(case, _cmp_problems)


# ---- workgroup-per-episode kernels ----

@pytest.mark.parametrize("row", list("ACDE"))
def test_workgroup_per_episode_kernels(row):
    """N = 2049, B = 2, T = 64 on the oracle's sparse mode.  The episodes start three flips away from a local
    optimum, so the greedy phase ends within a few steps and the basin, EARLY and horizon events fit into 64 steps."""
    case = _case("wg", "CUT", 2049, row, 64, 2)
    _run(case, _cmp_exact)


# ---- compact replay rings ----

@pytest.mark.parametrize("target", ["CUT", "MIN_COVER", "MIN_DOM_SET"])
@pytest.mark.parametrize("n", [20, 65])
@pytest.mark.parametrize("row", ["E", "C"])
def test_compact_rings_rebuild_the_horizon_row(target, n, row):
    """horizon_length = 7 under rows E and C: the compact rings recompute TERMINATION_IMMANENCY from it when they
    rebuild s and s'.  Random actions; every finished episode is reset onto a new graph after the step it ended in
    (and the odd episodes once after step 3, so the episodes run out of phase); pushes until the ring has wrapped.
    sample and gather equal the feature ring bitwise (the rule of test_compact_problems_gpu and of
    test_dqn_gpu.test_compact_replay_matches_feature_replay)."""
    from eco_hip import _lib
    from eco_hip.agents.dqn.utils import CompactReplayBuffer, ReplayBuffer
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.graphs import GraphStore
    from test_compact_problems_gpu import _same
    T = 12 if row == "E" else 24
    steps = 20 if row == "E" else 40
    G = 4 * B
    store = (GraphStore.random("ER", G, n, 0.15, seed=n) if target == "CUT" else
             GraphStore.random("ER", G, n, 0.15, seed=n, weights="uniform"))
    env = VecSpinSystem(store, B, T, **ec.env_kwargs(_utils(), row, n, T, target, _observables(target),
                                                     horizon_length=7))
    C = B * T
    feat = ReplayBuffer(C, n, device="cuda", seed=17, n_obs=env.n_obs)
    comp = CompactReplayBuffer(C, env, seed=17)
    env.reset(graph_ids=np.arange(B), seed=3)
    comp.snapshot()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = env.obs_x.clone()
    odd = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
    end_steps = []
    for t in range(steps):
        acts = torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32)
        nxt = x.clone()
        _, rew, done = env.step(acts, obs_out=nxt)
        feat.add_batch(x, nxt, env.graph_ids, acts, rew, done)
        comp.add_step(acts, rew, done)
        x = nxt.clone()
        mask = done.clone()
        if mask.any():
            cur = env.read()["current_step"].cpu().numpy()
            end_steps += [int(c) for c, m in zip(cur, mask.cpu().numpy()) if m]
        if t == 3:
            mask |= odd
        if mask.any():
            env.reset(graph_ids=(np.arange(B) + (t + 1) * B) % G, mask=mask, seed=9 + t)
            comp.snapshot(mask)
            x = env.obs_x.clone()
    env.check_errors()
    assert len(feat) == len(comp) == C and comp._pushed > C + B      # wrapped
    assert len(end_steps) >= B and (row == "E" or min(end_steps) < T)   # EARLY ended episodes before T
    ti = ec.ti_index(_observables(target))
    for m in (C // 2, C):
        a, b = feat.sample(m), comp.sample(m)
        names = ("xs", "act", "rew", "xn", "done", "gid")
        bad = [k for k, u, v in zip(names, a, b) if not _same([u], [v])]
        assert not bad, (bad, m)
    xs, _, _, xn, dn, _ = b
    for rows in (xs, xn):     # the horizon row in both regimes: 0 and strictly between 0 and 1
        col = rows[:, 0, ti]
        assert bool((col == 0).any()) and bool(((col > 0) & (col < 1)).any())
    assert row != "E" or bool((xn[:, 0, ti] == 1).any())     # NORMAL stopping: s' of the last step
    assert bool((dn == 1).any()) and bool((dn == 0).any())
    # with max_steps in place of horizon_length the row would be (t - T) / T + 1 = t / T: never 0 after a step
    idx = torch.from_numpy(np.random.default_rng(n).integers(0, C, 2 * C).astype(np.int32)).cuda()
    fa, cb = feat._buffers(2 * C), comp._buffers(2 * C)
    for tns in fa + cb:
        tns.fill_(-9)
    _lib.check(_lib.lib.eco_replay_gather(ctypes.byref(feat.rb), 2 * C, _lib.ptr(idx), *(_lib.ptr(v) for v in fa),
                                          _lib.stream_ptr()))
    _lib.check(_lib.lib.eco_replay_compact_gather(
        ctypes.byref(env.cfg), _lib.ptr(env.state), ctypes.byref(store.gs), B, _lib.ptr(comp.ring), C, len(comp),
        comp._pushed, 2 * C, _lib.ptr(idx), *(_lib.ptr(v) for v in cb), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert _same(fa, cb) and int(fa[2].min()) >= 0
    env.check_errors()
