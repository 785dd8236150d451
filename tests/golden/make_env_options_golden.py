"""Generate tests/golden/env_options.npz by running the REFERENCE env under the setting rows of
tests/env_options_common.py (reward signal, normalisation, reversibility, basin reward, stagnation punishment,
stopping mode and horizon length).

Run where the reference is available, like make_golden.py (whose import set-up -- the reference on sys.path behind
the identity numba.jit shim -- this script reuses):
    python tests/golden/make_env_options_golden.py

Rows A-I for CUT and rows A, C, D for MIN_COVER and MIN_DOM_SET, each on one ER(20, 0.3) graph.  Per case: the graph,
the start spins, the scripted actions, T, the reference's rewards, dones and per-step score, normalised score, best
score, normalised best score and best solution, an 8-byte SHA-256 digest of the float64 observation rows of every
step, and the full rows at three steps.  The archive is written with fixed zip timestamps, so a rerun reproduces the
file byte for byte.  Data only -- no reference source.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import make_golden as mg                                  # noqa: E402  (puts the reference and the repo on sys.path)
import src.envs.utils as ref_utils                        # noqa: E402
import env_options_common as ec                           # noqa: E402


def run_reference(target, row, T, J, spins, actions):
    n = J.shape[0]
    obs_list = ref_utils.DEFAULT_OBSERVABLES if target == "CUT" else mg.MAIN_OBS
    env = mg.ising_env.make("SpinSystem", ref_utils.SingleGraphGenerator(J), T,
                            **ec.env_kwargs(ref_utils, row, n, T, target, obs_list))
    n_obs = len(env.observables)
    obs = env.reset(spins=spins)

    def scalars():
        return (env.score, env.normalized_score, env.best_score, env.best_score_normalized, env.best_solution)
    rec = dict(obs=[obs[:n_obs].copy()], rew=[], done=[], scal=[scalars()])
    for a in actions:
        obs, rew, done, _ = env.step(int(a))
        rec["obs"].append(obs[:n_obs].copy())
        rec["rew"].append(float(rew))
        rec["done"].append(bool(done))
        rec["scal"].append(scalars())
        if done:
            break
    return rec


def save_deterministic(path, arrays):
    """An .npz (np.load reads it) whose bytes depend on the arrays alone: fixed member timestamps and order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    np.random.seed(0)
    out = {"n_cases": np.int64(len(ec.GOLDEN_CASES))}
    for ci in range(len(ec.GOLDEN_CASES)):
        target, row, T, J, spins, actions = ec.golden_case_inputs(ci)
        rec = run_reference(target, row, T, J, spins, actions)
        p = f"c{ci}_"
        out[p + "target"] = np.array(target)
        out[p + "row"] = np.array(row)
        out[p + "T"] = np.int64(T)
        out[p + "J"] = J.astype(np.int8)
        out[p + "spins"] = np.asarray(spins, dtype=np.int8)
        out[p + "actions"] = np.asarray(actions, dtype=np.int32)
        out[p + "rew"] = np.asarray(rec["rew"], dtype=np.float64)
        out[p + "done"] = np.asarray(rec["done"], dtype=bool)
        scal = np.asarray(rec["scal"], dtype=np.float64)
        for k, name in enumerate(ec.SCALARS):
            out[p + name] = scal[:, k]
        obs = np.stack(rec["obs"])
        out[p + "obs_digest"] = np.array([ec.digest(o) for o in obs], dtype=np.uint64)
        steps = [s for s in ec.GOLDEN_FULL_STEPS if s < len(obs)]
        out[p + "obs_steps"] = np.asarray(steps, dtype=np.int64)
        out[p + "obs_at"] = obs[steps]
    path = os.path.join(HERE, "env_options.npz")
    save_deterministic(path, out)
    print("env_options.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
