"""eco_hip.experiments.test_network(return_history=True) against the reference's own history frame
(tests/golden/solver_history.npz, case tn: one ER-20 graph, 3 attempts, 2 N steps), and
return_history=False against the frames the parent commit returned for the same seed
(tests/golden/test_network_parent.npz, recorded once on an MI355X before this feature existed)."""
import os

import numpy as np
import pytest

import solver_history_common as sh
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _setup():
    from eco_hip.networks.mpnn import MPNN
    f = sh.fixture()
    J = f["tn/J"].astype(np.float64)
    net = MPNN(n_obs_in=7, device="cuda")
    net.load_state_dict(sh.weights(7))
    return f, J, net, sh.env_kwargs("CUT", "eco", "SIGNED", J.shape[0])


def test_history_frame_matches_reference():
    from eco_hip.experiments import test_network
    f, J, net, kw = _setup()
    n = J.shape[0]
    # the reference run's numpy stream: seeded, then the N draws of its env constructor's own reset
    np.random.seed(int(f["tn/seed"]))
    np.random.randint(2, size=n)
    ret = test_network(net, kw, [J], step_factor=int(f["tn/step_factor"]), n_attempts=3, return_raw=True,
                       return_history=True)
    assert len(ret) == 3
    res, raw, hist = ret
    assert list(hist.columns) == list(f["tn/columns"]) == ["actions", "scores", "rewards"] and len(hist) == 1
    np.testing.assert_array_equal(np.array(raw["init spins"][0]), f["tn/init_spins"])
    acts, scores, rews = hist["actions"][0], hist["scores"][0], hist["rewards"][0]
    assert len(acts) == len(scores) == len(rews) == 3
    for e in range(3):
        assert acts[e][0] is None and rews[e][0] is None
        assert all(isinstance(a, int) for a in acts[e][1:])
        np.testing.assert_array_equal(acts[e][1:], f["tn/actions"][e])
        np.testing.assert_array_equal(np.array(scores[e], dtype=np.float64), f["tn/scores"][e])
        np.testing.assert_array_equal(np.array(rews[e][1:], dtype=np.float64), f["tn/rewards"][e])
    assert float(res["cut"][0]) == float(f["tn/cut"]) and float(res["mean cut"][0]) == float(f["tn/mean_cut"])
    # only the history frame: the reference's position in the returned list
    np.random.seed(int(f["tn/seed"]))
    np.random.randint(2, size=n)
    ret2 = test_network(net, kw, [J], step_factor=int(f["tn/step_factor"]), n_attempts=3, return_history=True)
    assert len(ret2) == 2 and ret2[1]["actions"][0] == acts


def test_frames_without_history_equal_the_parent_commit():
    from eco_hip.experiments import test_network
    f, J, net, kw = _setup()
    p = np.load(os.path.join(GOLDEN, "test_network_parent.npz"))
    res, raw = test_network(net, kw, [J], step_factor=int(f["tn/step_factor"]), n_attempts=3, return_raw=True,
                            seed=int(f["tn/seed"]))
    for c in res.columns:
        if c != "time":
            np.testing.assert_array_equal(np.asarray(res[c][0], dtype=np.float64), p["res/" + c], err_msg=c)
    for c in raw.columns:
        np.testing.assert_array_equal(np.asarray(raw[c][0], dtype=np.float64), p["raw/" + c], err_msg=c)
    assert isinstance(test_network(net, kw, [J], step_factor=1, n_attempts=2, seed=1), type(res))
