"""Generate tests/golden/weighted.npz by running the REFERENCE itself on float-weighted (EdgeType.RANDOM) graphs.

Run in the build container only (needs the reference tree; never on the GPU box):
    python tests/golden/make_weighted_golden.py
The reference is imported exactly as make_golden.py imports it (identity numba.jit shim); the fixture is data
only: inputs and the reference's outputs.

Contents (env cases with the env_er20.npz keys, J stored as float64):
  c0  ER-20 uniform(-1, 1) weights, T = 40, every action taken twice in a row (revisits);
  c1  the same kind of graph in the BINARY spin basis;
  c2  every weight negative, so max_local_reward < 0, quality normaliser 1 and lower bound < 0;
  mpnn/  one seeded MPNN (seeded_weights below; a digest of the weights is recorded, not the weights) on a batch
         of two float-weighted observations.
Each env case is drawn until the reference's own trajectory has every nonzero |g| and every nonzero
|score - best_score| >= 1e-6, the precondition under which an engine within rounding of the reference must
reproduce every comparison (g > 0, score > best_score) exactly.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (MPNN, digest, obs_after_random_steps, pack_env_cases, run_episode,  # noqa: E402
                         state_dict_np)

MPNN_SEED = 4321


def seeded_weights(shapes, seed=MPNN_SEED):
    """The fixture's network, rebuilt from a seed instead of stored (58,425 floats would not fit the size limit):
    every tensor of the state_dict, in its order, 0.1 x standard normal draws of numpy's default_rng(seed) rounded to
    float32.  `shapes`: {name: array or shape}.  The fixture records a digest of the result."""
    rng = np.random.default_rng(seed)
    return {k: (0.1 * rng.standard_normal(np.shape(v) if hasattr(v, "shape") else v)).astype(np.float32)
            for k, v in shapes.items()}


def random_graph(n, p, rng, allneg=False):
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    w = rng.uniform(-1.0, 1.0, int(keep.sum()))
    if allneg:
        w = -np.abs(w)
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = w
    return m + m.T


def well_separated(J, rec):
    """every nonzero |g| (= |row 1| * |mlr|) and nonzero |score - best_score| of the trajectory >= 1e-6"""
    g = np.abs(np.stack(rec["obs"])[:, 1, :] * rec["mlr"])
    gap = np.abs(np.asarray(rec["score"]) - np.asarray(rec["best_score"]))
    return (g[g != 0].min() >= 1e-6) and (gap[gap != 0].size == 0 or gap[gap != 0].min() >= 1e-6)


def make_weighted():
    n, T = 20, 40
    cases = []
    for ci, (basis, allneg, revisit) in enumerate((("SIGNED", False, True), ("BINARY", False, False),
                                                   ("SIGNED", True, False))):
        for attempt in range(100):
            rng = np.random.default_rng(1000 * (ci + 1) + attempt)
            J = random_graph(n, 0.3, rng, allneg)
            spins = 2 * rng.integers(0, 2, n) - 1
            actions = (np.array([int(a) for a in rng.integers(0, n, T // 2) for _ in (0, 1)]) if revisit
                       else rng.integers(0, n, T))
            sp = (1 - spins) // 2 if basis == "BINARY" else spins
            rec = run_episode(J, T, "eco", sp, actions, basis)
            if well_separated(J, rec):
                break
        else:
            raise RuntimeError("no well-separated trajectory found")
        print(f"case {ci}: attempt {attempt}, mlr {rec['mlr']:.6g} qn {rec['qn']:.6g} lb {rec['lb']:.6g}")
        cases.append(dict(J=J, T=T, mode="eco", basis=basis, spins=sp, actions=actions, rec=rec))
    out = pack_env_cases(cases)
    for ci, c in enumerate(cases):
        out[f"c{ci}_J"] = c["J"].astype(np.float64)       # pack_env_cases stores int8 adjacencies
    assert out["c2_mlr"] < 0 and out["c2_qn"] == 1.0 and out["c2_lb"] < 0
    rng = np.random.default_rng(77)
    net = MPNN(n_obs_in=7, n_layers=3, n_features=64, n_hid_readout=[], tied_weights=False)
    w = seeded_weights(state_dict_np(net))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    net.eval()
    out["mpnn/weights_digest"] = digest(np.concatenate([w[k].ravel() for k in w]))
    obs = np.array([obs_after_random_steps(random_graph(n, 0.3, rng), T, 9, rng) for _ in range(2)])
    with torch.no_grad():
        out["mpnn/q_b2"] = net(torch.FloatTensor(obs.copy())).numpy()
        out["mpnn/q_b1"] = np.array([net(torch.FloatTensor(o.copy())).numpy() for o in obs])
    out["mpnn/obs"] = obs
    path = os.path.join(HERE, "weighted.npz")
    np.savez_compressed(path, **out)
    print("weighted.npz", os.path.getsize(path), "env_er20.npz", os.path.getsize(os.path.join(HERE, "env_er20.npz")))


if __name__ == "__main__":
    import random
    random.seed(0)
    np.random.seed(0)
    make_weighted()
