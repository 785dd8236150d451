"""The greedy kernels' tie rule (solver.py:100-131: the first index of the largest immediate change) through the one
compare they share (GreedyArgmax of csrc/eco_env_dev.h), at the smallest sizes where the two tied vertices are
combined by the wave butterfly (N = 65, wave per episode) and by the workgroup's four LDS words (N = 2049).

The graph plants the tie: two star centres, each joined to 20 private leaves by weight +1; the first star's spins
are all +1 and the second's all -1, so s * (J s) is exactly 20 at both centres.  Every other vertex has fewer than 20
edges of weight +-1 (asserted), so the maximum is at these two vertices alone (asserted on the oracle's mask).  The
expected action is numpy's first argmax of the oracle's s * (J @ s) over the allowed vertices: the smaller centre
in a reversible env; in an irreversible one the smaller centre is already +1 and not allowed, so the larger one.
Exact integers: the bar is equality."""
import numpy as np
import pytest
import torch

from oracle import spinsystem_oracle as so

pytestmark = pytest.mark.gpu

LEAVES = 20


def _tied_case(n, c_lo, c_hi, leaves_lo, leaves_hi, seed):
    """(J, spins): stars at c_lo (all +1) and c_hi (all -1), +-1 edges of degree < 20 among the other vertices."""
    rng = np.random.default_rng(seed)
    J = np.zeros((n, n))
    star = np.concatenate([[c_lo, c_hi], leaves_lo, leaves_hi])
    assert len(set(star)) == 2 + 2 * LEAVES
    rest = np.setdiff1d(np.arange(n), star)
    m = 2 * rest.size                                    # mean degree 4
    i, j = rng.choice(rest, m), rng.choice(rest, m)
    pairs = np.unique(np.minimum(i, j)[i != j] * n + np.maximum(i, j)[i != j])   # each undirected edge once
    i, j = pairs // n, pairs % n
    J[i, j] = J[j, i] = rng.choice([-1.0, 1.0], pairs.size)
    assert (J == J.T).all()
    assert (J != 0).sum(1).max() < LEAVES
    for c, leaves in ((c_lo, leaves_lo), (c_hi, leaves_hi)):
        J[c, leaves] = J[leaves, c] = 1.0
    spins = 2 * rng.integers(0, 2, n) - 1
    spins[np.concatenate([[c_lo], leaves_lo])] = 1
    spins[np.concatenate([[c_hi], leaves_hi])] = -1
    return J, spins


# N = 65: vertex 5 is lane 5 of slot 0, vertex 64 lane 0 of slot 1 (two slots per lane).
# N = 2049: vertex 70 is thread 70 (wave 1) of slot 0, vertex 2048 thread 0 (wave 0) of slot 8.
CASES = {65: (5, 64, np.arange(10, 30), np.arange(30, 50)),
         2049: (70, 2048, np.arange(300, 320), np.arange(1000, 1020))}


@pytest.mark.parametrize("n", sorted(CASES))
def test_tie_takes_the_smaller_allowed_index(n):
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import Observable, RewardSignal, ExtraAction, OptimisationTarget, SpinBasis
    c_lo, c_hi = CASES[n][:2]
    J, spins = _tied_case(n, *CASES[n], seed=n)
    g = so.calculate_cut_changes(spins.astype(np.float64), J)
    assert g[c_lo] == g[c_hi] == LEAVES and list(np.flatnonzero(g == g.max())) == [c_lo, c_hi]   # the tie, and no third
    if n == 65:
        assert c_lo % 64 != c_hi % 64                                  # different lanes
    else:
        assert (c_lo % 256) // 64 != (c_hi % 256) // 64                # different waves of the workgroup
    store = GraphStore.from_dense([J])
    for reversible in (True, False):
        allowed = np.ones(n, bool) if reversible else spins < 0
        want = int(np.argmax(np.where(allowed, g, -np.inf)))           # first index of the maximum
        assert want == (c_lo if reversible else c_hi)
        env = VecSpinSystem(store, 1, 8, observables=[Observable.SPIN_STATE, Observable.IMMEDIATE_QUALITY_CHANGE],
                            reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                            optimisation_target=OptimisationTarget.CUT, spin_basis=SpinBasis.SIGNED,
                            norm_rewards=True, reversible_spins=reversible)
        env.reset(graph_ids=np.zeros(1, dtype=np.int64), spins=spins[None])
        got = int(env.greedy_actions().to(torch.int64).cpu()[0])
        env.check_errors()
        assert got == want, (n, reversible, got, want)
        assert int(env.read()["done"][0]) == 0
