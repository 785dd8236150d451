"""Pin the CPU oracle to the reference on float-weighted (EdgeType.RANDOM) graphs: tests/golden/weighted.npz was
recorded by running the reference itself (tests/golden/make_weighted_golden.py).

BLAS summation order differs between CPUs, so float64 quantities are held to the derived bars of
tests/weighted_common.py (both sides sum an N-term dot product per step), not bitwise; discrete outputs (spins,
dones, improvement count, Hamming distance, time rows) must be equal.  MPNN Q: 5e-7 (1 + |q|).
"""
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import mpnn_oracle as mo
from oracle import spinsystem_oracle as so
from weighted_common import Bars, check_rows, fixture_weights, well_separated


def _fixture():
    return np.load(os.path.join(GOLDEN, "weighted.npz"))


def test_fixture_holds_the_three_cases_and_is_small():
    f = _fixture()
    assert int(f["n_cases"]) == 3
    assert os.path.getsize(os.path.join(GOLDEN, "weighted.npz")) <= os.path.getsize(os.path.join(GOLDEN, "env_er20.npz"))
    for c in range(3):
        J = f[f"c{c}_J"]
        assert J.dtype == np.float64 and J.shape == (20, 20) and int(f[f"c{c}_T"]) == 40
        w = J[J != 0]
        assert np.array_equal(J, J.T) and not np.diag(J).any() and (w != np.round(w)).all()   # EdgeType.RANDOM
    a = f["c0_actions"]
    assert np.array_equal(a[0::2], a[1::2])                     # revisits
    assert str(f["c1_basis"]) == "BINARY"
    assert (f["c2_J"] <= 0).all() and f["c2_mlr"] < 0 and f["c2_qn"] == 1.0 and f["c2_lb"] < 0


def test_oracle_reproduces_the_reference_trajectories():
    f = _fixture()
    for c in range(3):
        p = f"c{c}_"
        J, T, basis = f[p + "J"], int(f[p + "T"]), str(f[p + "basis"])
        n = J.shape[0]
        o = so.SpinSystemOracle(J, T, basin_reward=1. / n, spin_basis=basis)
        o.reset(spins=f[p + "spins"].astype(np.int64))
        bars = Bars(J, float(f[p + "mlr"]), float(f[p + "qn"]))
        A, W = bars.A, bars.W
        u = 2.0 ** -52
        assert abs(o.mlr - f[p + "mlr"]) <= u * n * A
        assert abs(o.qn - f[p + "qn"]) <= u * n * n * W and abs(o.lb - f[p + "lb"]) <= u * n * n * W
        ref = f[p + "obs"]
        signed = [o.state[0].copy()]
        check_rows(o.state_rows(), ref[0], bars, 0, f"{p} reset")
        assert abs(o.score - f[p + "score"][0]) <= bars.score(0)
        for t, a in enumerate(f[p + "actions"][:len(f[p + "rew"])]):
            _, rew, done, _ = o.step(int(a))
            signed.append(o.state[0].copy())
            sb = bars.score(t + 1)
            check_rows(o.state_rows(), ref[t + 1], bars, t + 1, f"{p} step {t}")
            assert abs(rew - f[p + "rew"][t]) <= sb / o.qn, (p, t, rew, f[p + "rew"][t])
            assert done == f[p + "done"][t]
            assert abs(o.score - f[p + "score"][t + 1]) <= sb and abs(o.best_score - f[p + "best_score"][t + 1]) <= sb
            assert abs(o.normalized_score - f[p + "nscore"][t + 1]) <= sb / o.qn
            assert abs(o.best_score_normalized - f[p + "best_nscore"][t + 1]) <= sb / o.qn
            assert abs(o.best_solution - f[p + "best_solution"][t + 1]) <= 2 * sb
        # the precondition the engine tests rely on holds on the reference's own trajectory
        ok, mins = well_separated(J, signed, f[p + "score"], f[p + "best_score"])
        assert ok, (p, mins)


def test_oracle_reproduces_the_reference_mpnn_forward():
    f = _fixture()
    w = fixture_weights(f)
    obs = torch.from_numpy(f["mpnn/obs"]).float()
    adj = f["mpnn/obs"][:, 7:, :]
    assert (adj[adj != 0] != np.round(adj[adj != 0])).all()
    for q, ref in ((mo.forward(w, obs).numpy(), f["mpnn/q_b2"]),
                   (np.stack([mo.forward(w, o).numpy() for o in obs]), f["mpnn/q_b1"])):
        err = (np.abs(q.astype(np.float64) - ref) / (1 + np.abs(ref))).max()
        print(f"max scaled err {err:.3e}")
        assert err <= 5e-7, err
