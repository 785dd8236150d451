"""tests/golden/solver_history.npz (recorded by the reference's own Network solver and test_network) against
the CPU helper that the GPU tests use as their reference: tests/solver_history_common.replay on the recorded
actions reproduces every history field."""
import numpy as np
import pytest

import solver_history_common as sh
from weighted_common import Bars

N_CASES = 9
RTOL_Q = 5e-7   # test_oracle_golden.py's bar for mpnn_fwd.npz: |q - ref| <= 5e-7 (1 + |ref|)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_replay_reproduces_reference_history(ci):
    c = sh.case(ci)
    assert int(sh.fixture()["n_cases"]) == N_CASES
    acts = c["action"][1:].astype(np.int64)
    r = sh.replay(c["J"], c["T"], c["target"], c["mode"], c["basis"], c["init_spins"], acts,
                  w=sh.weights(c["n_obs_in"]), n_obs_in=c["n_obs_in"])
    L = len(c["action"])
    assert len(r["action"]) == L and r["done"][-1] and not r["done"][:-1].any()
    np.testing.assert_array_equal(r["action"], c["action"])
    np.testing.assert_array_equal(r["spins"], c["spins"])
    np.testing.assert_array_equal(r["valid"], c["valid"])
    np.testing.assert_array_equal(r["spins"][0], c["init_spins"])   # state[0] is signed in either basis
    if c["J"].dtype == np.float64 and not np.array_equal(c["J"], np.rint(c["J"])):
        o = sh.make_oracle(c["J"], c["T"], c["target"], c["mode"], c["basis"], c["init_spins"])
        b = Bars(c["J"], o.scorer.mlr, o.scorer.qn)
        for t in range(L):   # field bar x |mlr| for g, score bar for the cut, / qn for rewards
            assert np.abs(r["score_mask"][t] - c["score_mask"][t]).max() <= b.field(t) * b.mlr
            assert abs(r["solution"][t] - c["solution"][t]) <= b.score(t)
            assert abs(r["reward"][t] - c["reward"][t]) <= b.score(t) / b.qn
    else:
        for k in ("solution", "reward", "score_mask"):
            np.testing.assert_array_equal(r[k], c[k], err_msg=k)
    err = np.abs(r["qs"].astype(np.float64) - c["qs"]) / (1 + np.abs(c["qs"]))
    assert err.max() <= RTOL_Q, err.max()
    # the recorded action is the first-index argmax of the recorded Q over allowed vertices
    rev = c["mode"] != "s2v"
    for t in range(1, L):
        assert sh.allowed_argmax(c["qs"][t], c["spins"][t - 1], rev) == int(c["action"][t])
    assert c["measure"] == c["solution"][-1]


def test_margin_condition_recorded():
    f = sh.fixture()
    for ci in range(N_CASES):
        assert float(f[f"c{ci}/min_margin"]) >= 1e-4


def test_test_network_history_frame_is_replayable():
    """The reference's test_network history (fixture case tn): scores are scorer.get_score per step, rewards and
    actions one per step, and the attempts' initial spins are the global numpy stream this repository's
    test_network draws (after the N draws of the reference env constructor's own reset)."""
    f = sh.fixture()
    J = f["tn/J"].astype(np.float64)
    n = J.shape[0]
    T = n * int(f["tn/step_factor"])
    assert list(f["tn/columns"]) == ["actions", "scores", "rewards"]
    assert f["tn/actions"].shape == (3, T) and f["tn/scores"].shape == (3, T + 1) and f["tn/rewards"].shape == (3, T)
    rs = np.random.RandomState(int(f["tn/seed"]))
    rs.randint(2, size=n)
    np.testing.assert_array_equal(2 * rs.randint(2, size=(3, n)) - 1, f["tn/init_spins"])
    for e in range(3):
        r = sh.replay(J, T, "CUT", "eco", "SIGNED", f["tn/init_spins"][e], f["tn/actions"][e])
        np.testing.assert_array_equal(r["score"], f["tn/scores"][e])
        np.testing.assert_array_equal(r["reward"][1:], f["tn/rewards"][e])
