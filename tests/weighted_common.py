"""Shared pieces of the float-weighted (EdgeType.RANDOM) tests: the derived float64 bars, the row comparison, the
precondition that makes every comparison of a trajectory unambiguous, and the seeded network of
tests/golden/weighted.npz."""
import hashlib

import numpy as np

from oracle import mpnn_oracle as mo
from oracle import spinsystem_oracle as so

U = 2.0 ** -52


class Bars:
    def __init__(self, J, mlr, qn):
        self.N = J.shape[0]
        self.A = np.abs(J).sum(1).max()
        self.d = int((J != 0).sum(1).max())
        self.W = np.abs(J).sum() / 2
        self.mlr, self.qn = abs(mlr), qn

    def field(self, t):
        return U * (self.N + self.d + t) * self.A / self.mlr

    def score(self, t):
        return U * (t + 1) * (self.N + self.d + t + 1) * self.W


def check_rows(rows, ref, bars, t, tag):
    """rows / ref: [7, N] float64 DEFAULT_OBSERVABLES rows (engine / oracle)."""
    n = bars.N
    np.testing.assert_array_equal(rows[0], ref[0], err_msg=f"{tag} spins")
    assert np.abs(rows[1] - ref[1]).max() <= bars.field(t), (tag, "g row", np.abs(rows[1] - ref[1]).max(), bars.field(t))
    np.testing.assert_array_equal(rows[2], ref[2], err_msg=f"{tag} time since flip")
    assert np.abs(rows[3] - ref[3]).max() <= 2 * bars.score(t) / bars.mlr, (tag, "distance from best solution")
    np.testing.assert_array_equal(rows[4], ref[4], err_msg=f"{tag} hamming")
    np.testing.assert_array_equal(np.rint(rows[5] * n), np.rint(ref[5] * n), err_msg=f"{tag} improvements x N")
    np.testing.assert_array_equal(rows[5], ref[5], err_msg=f"{tag} improvements row")
    np.testing.assert_array_equal(rows[6], ref[6], err_msg=f"{tag} termination")


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)




def well_separated(J, spin_rows, scores, best_scores):
    """Precondition on an oracle / reference trajectory: every nonzero |g| and every nonzero |score - best_score|
    is >= 1e-6 (so g > 0 and score > best_score cannot differ between two sides that agree to rounding)."""
    gmin = gapmin = np.inf
    for s in spin_rows:
        g = np.abs(so.calculate_cut_changes(np.asarray(s, dtype=np.float64), J))
        if (g != 0).any():
            gmin = min(gmin, g[g != 0].min())
    gap = np.abs(np.asarray(scores) - np.asarray(best_scores))
    if (gap != 0).any():
        gapmin = gap[gap != 0].min()
    return gmin >= 1e-6 and gapmin >= 1e-6, (gmin, gapmin)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], dtype=np.uint64)[0]


def fixture_weights(f, seed=4321):
    """The network of weighted.npz, rebuilt from its seed as tests/golden/make_weighted_golden.py builds it (every
    state_dict tensor in order: 0.1 x standard normal of numpy's default_rng(seed), as float32), checked against the
    digest the fixture records."""
    import torch
    rng = np.random.default_rng(seed)
    w = {k: (0.1 * rng.standard_normal(shape)).astype(np.float32) for k, shape in zip(mo.KEYS, mo.shapes(7))}
    assert digest(np.concatenate([w[k].ravel() for k in mo.KEYS])) == f["mpnn/weights_digest"], \
        "seeded fixture weights differ from the recorded ones"
    return {k: torch.from_numpy(v) for k, v in w.items()}
