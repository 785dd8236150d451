"""Both CPU oracles against the reference under every reward / stopping / horizon / stagnation setting row of
tests/env_options_common.py (fixture tests/golden/env_options.npz, recorded from the reference by
tests/golden/make_env_options_golden.py).

Bar: bitwise equality of rewards, dones, the five per-step scalars, the per-step observation digests and the rows
stored in full.  The negative controls show that the fixture tells the settings apart: no two rows share a
(reward, done) sequence, and an oracle with one setting changed fails the comparison."""
import os

import numpy as np
import pytest

import env_options_common as ec
from conftest import GOLDEN

F = np.load(os.path.join(GOLDEN, "env_options.npz"))
CASES = list(range(int(F["n_cases"])))


def _case(ci):
    p = f"c{ci}_"
    return (str(F[p + "target"]), str(F[p + "row"]), int(F[p + "T"]), F[p + "J"].astype(np.float64),
            F[p + "spins"].astype(np.int64), F[p + "actions"])


def _oracle(target, row, T, J, **over):
    if target == "CUT":
        return ec.make_oracle(J, T, row, target, **over)
    o = ec.golden_problem_oracle(J, T, row, target)
    for k, v in over.items():
        assert hasattr(o, k)
        setattr(o, k, v)
    return o


def _mismatches(ci, o):
    """Names of the recorded quantities the oracle's replay of case ci does not reproduce bitwise."""
    p = f"c{ci}_"
    _, _, _, _, spins, actions = _case(ci)
    tr = ec.run_oracle(o, spins, actions)
    bad = []

    def same(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if not same(tr["rew"], F[p + "rew"]):
        bad.append("rew")
    if not np.array_equal(np.asarray(tr["done"]), F[p + "done"]):
        bad.append("done")
    for k in ec.SCALARS:
        if not same(tr[k], F[p + k]):
            bad.append(k)
    dig = np.array([ec.digest(r) for r in tr["rows"]], dtype=np.uint64)
    if not np.array_equal(dig, F[p + "obs_digest"]):
        bad.append("obs_digest")
    steps = [int(s) for s in F[p + "obs_steps"]]
    if len(tr["rows"]) <= max(steps) or not same(np.stack([tr["rows"][s] for s in steps]), F[p + "obs_at"]):
        bad.append("obs_at")
    return bad


@pytest.mark.parametrize("ci", CASES)
def test_oracle_matches_reference(ci):
    target, row, T, J, _, _ = _case(ci)
    assert (target, row, T) == ec.GOLDEN_CASES[ci]
    assert _mismatches(ci, _oracle(target, row, T, J)) == []


@pytest.mark.parametrize("ci", CASES)
def test_fixture_inputs_are_the_scripted_ones_and_show_the_rows_events(ci):
    """The stored graph, spins and actions are those of env_options_common.golden_case_inputs, and the recorded
    trajectory (replayed on the oracle, equal to it by the test above) contains the events the row exists for."""
    target, row, T, J, spins, actions = _case(ci)
    t2, r2, T2, J2, s2, a2 = ec.golden_case_inputs(ci)
    assert (target, row, T) == (t2, r2, T2)
    np.testing.assert_array_equal(J, J2)
    np.testing.assert_array_equal(spins, s2)
    np.testing.assert_array_equal(actions, a2)
    o = _oracle(target, row, T, J)
    tr = ec.run_oracle(o, spins, actions, ec.ti_index(ec.o_observables(o)))
    ev = ec.assert_events(row, [tr], T, J.shape[0])
    print(target, row, T, ev)
    assert len(F[f"c{ci}_rew"]) == tr["steps"]


def test_no_two_rows_share_a_reward_and_done_sequence():
    for target in ("CUT", "MIN_COVER", "MIN_DOM_SET"):
        seqs = {}
        for ci in CASES:
            if str(F[f"c{ci}_target"]) != target:
                continue
            key = (F[f"c{ci}_rew"].tobytes(), F[f"c{ci}_done"].tobytes())
            assert key not in seqs, (target, ci, seqs[key])
            seqs[key] = ci
        assert len(seqs) == sum(1 for t, _, _ in ec.GOLDEN_CASES if t == target)


def _ci(target, row):
    return next(i for i, (t, r, _) in enumerate(ec.GOLDEN_CASES) if (t, r) == (target, row))


@pytest.mark.parametrize("target,row,attr,value,must_differ", [
    ("CUT", "E", "horizon_length", 40, "obs_digest"),      # horizon_length=None: the horizon is max_steps
    ("CUT", "C", "stopping", "NORMAL", "done"),
    ("CUT", "A", "norm_rewards", True, "rew"),
    ("CUT", "D", "stopping", "NORMAL", "done"),
    ("CUT", "B", "stag_punishment", None, "rew"),
    ("CUT", "F", "reward_signal", "BLS", "rew"),
    ("CUT", "G", "reward_signal", "BLS", "rew"),
    ("CUT", "H", "horizon_length", 40, "obs_digest"),
    ("MIN_COVER", "C", "stopping", "NORMAL", "done"),
    ("MIN_DOM_SET", "A", "norm_rewards", True, "rew"),
])
def test_one_changed_setting_fails_the_comparison(target, row, attr, value, must_differ):
    ci = _ci(target, row)
    _, _, T, J, _, _ = _case(ci)
    assert value != getattr(_oracle(target, row, T, J), attr)
    if attr == "stag_punishment":   # the oracle reads it in reset as well (whether to keep a visited set)
        o = ec.make_oracle(J, T, row, target, stag_punishment=None)
    else:
        o = _oracle(target, row, T, J, **{attr: value})
    assert must_differ in _mismatches(ci, o)
