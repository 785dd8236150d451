"""Shared cases of the env-option tests (tests/test_env_options_cpu.py, tests/test_env_options_gpu.py and
tests/golden/make_env_options_golden.py): the setting rows, the scripted actions, the oracle trajectories with the
events each row exists for, and the assertions that those events happened.

Rows (ExtraAction.NONE, memory_length None; basin reward 1 / N, stagnation punishment 0.25 where set):

  row  reward      norm   reversible  basin  stag   stopping  horizon
  A    BLS         False  yes         1/N    -      NORMAL    None
  B    BLS         True   yes         -      0.25   NORMAL    None
  C    BLS         True   yes         1/N    0.25   EARLY     None
  D    DENSE       False  yes         -      0.25   QUARTER   None
  E    DENSE       True   yes         -      -      NORMAL    7
  F    SINGLE      True   yes         1/N    -      NORMAL    None
  G    CUSTOM_BLS  True   yes         -      0.25   NORMAL    None
  H    BLS         False  no          -      -      NORMAL    3 T
  I    BLS         True   yes         1/N    -      QUARTER   None   (run with max_steps 3 and 4)

Script of a reversible row: five random steps of which the fifth repeats the fourth (an immediate revisit inside
the first T // 4 steps, which the QUARTER row needs at every size: its episodes end before the random tail), then
greedy steps (argmax of the oracle's score mask) until no change is positive (a local optimum: the basin reward),
then random steps with the previous action repeated at every seventh step (revisits).  Row H starts from all -1
spins and plays a permutation of the vertices ("no spin left" stops the episode at step N < T).
"""
import hashlib

import numpy as np

from oracle import problems_oracle as po
from oracle import spinsystem_oracle as so

STAG = 0.25
ROWS = {
    "A": dict(reward="BLS", norm=False, reversible=True, basin=True, stag=False, stopping="NORMAL", horizon=None),
    "B": dict(reward="BLS", norm=True, reversible=True, basin=False, stag=True, stopping="NORMAL", horizon=None),
    "C": dict(reward="BLS", norm=True, reversible=True, basin=True, stag=True, stopping="EARLY", horizon=None),
    "D": dict(reward="DENSE", norm=False, reversible=True, basin=False, stag=True, stopping="QUARTER", horizon=None),
    "E": dict(reward="DENSE", norm=True, reversible=True, basin=False, stag=False, stopping="NORMAL", horizon=7),
    "F": dict(reward="SINGLE", norm=True, reversible=True, basin=True, stag=False, stopping="NORMAL", horizon=None),
    "G": dict(reward="CUSTOM_BLS", norm=True, reversible=True, basin=False, stag=True, stopping="NORMAL",
              horizon=None),
    "H": dict(reward="BLS", norm=False, reversible=False, basin=False, stag=False, stopping="NORMAL", horizon="3T"),
    "I": dict(reward="BLS", norm=True, reversible=True, basin=True, stag=False, stopping="QUARTER", horizon=None),
}
SCALARS = ("score", "normalized_score", "best_score", "best_score_normalized", "best_solution")


def horizon(row, T):
    h = ROWS[row]["horizon"]
    return 3 * T if h == "3T" else h


def oracle_kwargs(row, n, T, **over):
    """Keyword arguments of SpinSystemOracle / ProblemSpinSystemOracle for a row."""
    r = ROWS[row]
    kw = dict(reward_signal=r["reward"], norm_rewards=r["norm"], reversible_spins=r["reversible"],
              basin_reward=1. / n if r["basin"] else None, stag_punishment=STAG if r["stag"] else None,
              stopping=r["stopping"], horizon_length=horizon(row, T))
    kw.update(over)
    return kw


def env_kwargs(utils, row, n, T, target="CUT", observables=None, **over):
    """env_args of a row in the enums of `utils` (eco_hip.envs.utils, or the reference's module of the same names)."""
    r = ROWS[row]
    kw = dict(observables=observables if observables is not None else utils.DEFAULT_OBSERVABLES,
              reward_signal=utils.RewardSignal[r["reward"]], extra_action=utils.ExtraAction.NONE,
              optimisation_target=utils.OptimisationTarget[target], spin_basis=utils.SpinBasis.SIGNED,
              norm_rewards=r["norm"], memory_length=None, horizon_length=horizon(row, T),
              stag_punishment=STAG if r["stag"] else None, basin_reward=1. / n if r["basin"] else None,
              reversible_spins=r["reversible"], stopping=utils.Stopping[r["stopping"]])
    kw.update(over)
    return kw


def problem_observables(utils, target):
    """MAIN_OBSERVABLES; MIN_CUT has no invalidity mask (TypeError in the reference), so it takes the other ten."""
    if target != "MIN_CUT":
        return list(utils.MAIN_OBSERVABLES)
    return [o for o in utils.MAIN_OBSERVABLES if getattr(o, "value", o) not in po.VALIDITY_MASK_OBSERVABLES]


def make_oracle(J, T, row, target="CUT", **over):
    """The oracle of a family: SpinSystemOracle for CUT (a SparseMatrix selects its sparse mode),
    ProblemSpinSystemOracle (one reset, like a fresh VecSpinSystem) for the generic-scorer targets."""
    n = J.shape[0]
    if target == "CUT":
        return so.SpinSystemOracle(J, T, **oracle_kwargs(row, n, T, **over))
    return po.ProblemSpinSystemOracle(J, T, target=getattr(po, target), observables=problem_observables(po, target),
                                      init_reset=False, **oracle_kwargs(row, n, T, **over))


def score_mask(o):
    """Per-vertex score change of a flip in the oracle's current state."""
    if isinstance(o, so.SpinSystemOracle):
        return so.calculate_cut_changes(o.state[0, :], o.matrix)
    return np.asarray(o.scorer.score_mask(o.state[0, :], o.matrix), dtype=np.float64)


def random_tail(n, length, rng):
    """Random actions with the previous one repeated at every seventh step (test_weighted_env_gpu._actions)."""
    a = rng.integers(0, n, length)
    a[7::7] = a[6::7][:len(a[7::7])]
    return a


def script(J, T, row, spins, seed, target="CUT", steps=None):
    """Actions of one episode, planned on an oracle with NORMAL stopping (the spin trajectory does not depend on the
    reward or stopping settings, so one script serves every reversible row)."""
    n = J.shape[0]
    steps = T if steps is None else steps
    rng = np.random.default_rng(seed)
    if not ROWS[row]["reversible"]:
        return rng.permutation(n)[:steps].astype(np.int64)
    o = make_oracle(J, max(T, steps), "A", target)     # the planner never runs out of steps
    o.reset(spins=spins)
    pre = rng.integers(0, n, 5)
    pre[4] = pre[3]
    acts = []
    for a in pre[:steps]:
        acts.append(int(a))
        o.step(int(a))
    while len(acts) < steps:
        m = score_mask(o)
        a = int(m.argmax())
        if not m[a] > 0:
            break
        acts.append(a)
        o.step(a)
    acts += [int(a) for a in random_tail(n, steps - len(acts), rng)]
    return np.asarray(acts, dtype=np.int64)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], dtype=np.uint64)[0]


def run_oracle(o, spins, actions, ti_index=None):
    """Drive a reset-able oracle over `actions` until done.  Returns the records the tests compare (rows[t],
    scalars[t] for t = 0 .. steps; rew[t], done[t] for the steps) and the per-step event flags."""
    o.reset(spins=spins)
    tr = dict(rows=[o.state_rows().copy()], rew=[], done=[], revisit=[], basin=[], improved=[], ti=[],
              spins=[o.state[0].copy()], **{k: [getattr(o, k)] for k in SCALARS})
    for a in actions:
        visited = None if o.history is None else sum(len(v) for v in o.history.buffer.values())
        best = o.best_score
        _, r, d, _ = o.step(int(a))
        new = o.history is None or sum(len(v) for v in o.history.buffer.values()) > visited
        tr["rows"].append(o.state_rows().copy())
        tr["spins"].append(o.state[0].copy())
        tr["rew"].append(r)
        tr["done"].append(bool(d))
        for k in SCALARS:
            tr[k].append(getattr(o, k))
        tr["revisit"].append(not new)
        tr["basin"].append(bool(o.basin_reward is not None and new and np.all(score_mask(o) <= 0)))
        tr["improved"].append(bool(o.score > best))
        if ti_index is not None:
            tr["ti"].append(float(o.state[ti_index, 0]))
        if d:
            break
    tr["steps"] = len(tr["rew"])
    tr["early_counter"] = o.early_stopping
    return tr


def event_counts(traces):
    """Totals over the episodes of a case."""
    imp_after = 0
    for tr in traces:
        imp = tr["improved"]
        imp_after += sum(1 for t in range(1, len(imp)) if imp[t] and not imp[t - 1])
    return dict(revisits=sum(sum(tr["revisit"]) for tr in traces), basins=sum(sum(tr["basin"]) for tr in traces),
                improvement_after_stall=imp_after,
                ti_between=sum(sum(1 for x in tr["ti"] if 0 < x < 1) for tr in traces),
                ti_zero=sum(sum(1 for x in tr["ti"] if x == 0) for tr in traces),
                end_steps=[tr["steps"] for tr in traces])


def assert_events(row, traces, T, n):
    """The events a row exists for, on the oracle's own trajectories of one case (all its episodes); a case that
    never reaches its branch fails here instead of passing silently."""
    r = ROWS[row]
    ev = event_counts(traces)
    tag = (row, T, n, ev)
    assert all(tr["done"][-1] for tr in traces), tag
    if row == "I":
        # T // 4 == 0 never equals a step >= 1: the episode runs to T; T = 4 stops at step 1
        assert all(tr["steps"] == (1 if T // 4 >= 1 else T) for tr in traces), tag
        return ev
    if r["stag"] or r["basin"]:
        assert ev["revisits"] >= 1, tag
    if r["stag"]:     # a revisit shows in the reward
        assert any(rew < 0 for tr in traces for rew, rv in zip(tr["rew"], tr["revisit"]) if rv), tag
    if r["basin"]:
        assert ev["basins"] >= 1, tag
    if r["stopping"] == "EARLY":
        assert all(tr["steps"] < T and tr["early_counter"] == 15 for tr in traces), tag
        assert ev["improvement_after_stall"] >= 1, tag
    if r["stopping"] == "QUARTER":
        assert all(tr["steps"] == T // 4 < T for tr in traces), tag
    if not r["reversible"]:
        assert all(tr["steps"] == n < T for tr in traces), tag
    if r["stopping"] == "NORMAL" and r["reversible"]:
        assert all(tr["steps"] == T for tr in traces), tag
    if r["horizon"] is not None:
        assert ev["ti_between"] >= 1, tag
        if r["horizon"] == 7:
            assert ev["ti_zero"] >= 1, tag
    return ev


def ti_index(observables):
    vals = [getattr(o, "value", o) for o in observables]
    return vals.index(so.TERMINATION_IMMANENCY) if so.TERMINATION_IMMANENCY in vals else None


def cut_graph(n, seed):
    from oracle import graphs as og
    return og.er_graph(n, min(0.3, 6.0 / n), np.random.default_rng(seed), "discrete")


def start_spins(n, seed, row):
    if not ROWS[row]["reversible"]:
        return -np.ones(n, dtype=np.int64)
    return 2 * np.random.default_rng(seed).integers(0, 2, n) - 1


def float_graph(n, seed):
    """ER(n, min(0.3, 6 / n)) with uniform(-1, 1) weights (EdgeType.RANDOM)."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < min(0.3, 6.0 / n)
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = rng.uniform(-1.0, 1.0, int(keep.sum()))
    return m + m.T


def problem_graph(n, seed, target):
    from oracle import graphs as og
    return og.er_graph(n, min(0.3, 6.0 / n), np.random.default_rng(seed), "discrete" if target == "MIN_CUT" else "uniform")


def local_optimum(J, spins):
    """Greedy MaxCut ascent from `spins` to a state where no single flip gains (J dense or SparseMatrix)."""
    s = np.asarray(spins, dtype=np.float64).copy()
    while True:
        g = so.calculate_cut_changes(s, J)
        a = int(g.argmax())
        if not g[a] > 0:
            return s.astype(np.int64)
        s[a] = -s[a]


def near_optimum_spins(J, seed, flips=3):
    """A local optimum with `flips` random spins flipped: the scripted greedy phase returns to an optimum within a few
    steps, which a graph of thousands of vertices needs for the script's later phases to fit into max_steps."""
    rng = np.random.default_rng(seed)
    n = J.shape[0]
    s = local_optimum(J, 2 * rng.integers(0, 2, n) - 1)
    s[rng.choice(n, flips, replace=False)] *= -1
    return s


# ---- the golden fixture (tests/golden/env_options.npz) ----

GOLDEN_N = 20
GOLDEN_FULL_STEPS = (0, 1, 7)     # observation rows stored in full at these steps, digests at every step
# (target, row, max_steps); row I twice.  Seeds: the first of 0, 1, 2, ... whose script shows the row's events.
GOLDEN_CASES = ([("CUT", r, 2 * GOLDEN_N) for r in "ABCDEFGH"] + [("CUT", "I", 3), ("CUT", "I", 4)] +
                [(t, r, 2 * GOLDEN_N) for t in ("MIN_COVER", "MIN_DOM_SET") for r in "ACD"])


def golden_case_inputs(ci):
    """(target, row, T, J, spins, actions) of golden case ci, chosen so that assert_events holds."""
    target, row, T = GOLDEN_CASES[ci]
    n = GOLDEN_N
    from oracle import graphs as og
    for seed in range(64):
        rng = np.random.default_rng(1000 * ci + seed)
        J = og.er_graph(n, 0.3, rng, "discrete" if target == "CUT" else "uniform")
        spins = start_spins(n, 5000 + 1000 * ci + seed, row)
        acts = script(J, T, row, spins, 9000 + 1000 * ci + seed, target)
        o = make_oracle(J, T, row, target) if target == "CUT" else golden_problem_oracle(J, T, row, target)
        tr = run_oracle(o, spins, acts, ti_index(o_observables(o)))
        try:
            assert_events(row, [tr], T, n)
        except AssertionError:
            continue
        return target, row, T, J, spins, acts
    raise AssertionError(f"no seed shows the events of golden case {ci}")


def golden_problem_oracle(J, T, row, target):
    """The reference constructor resets once before the caller does (spinsystem.py:168), which fixes the invalidity
    normaliser of the first observation: init_reset=True."""
    n = J.shape[0]
    return po.ProblemSpinSystemOracle(J, T, target=getattr(po, target), observables=po.MAIN_OBSERVABLES,
                                      init_reset=True, rng=np.random.RandomState(0), **oracle_kwargs(row, n, T))


def o_observables(o):
    return [obs for _, obs in o.observables]
