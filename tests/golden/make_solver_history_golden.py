"""Generate tests/golden/solver_history.npz by running the REFERENCE's own `Network` solver class
(src/agents/solver.py:161-267), so that ITS history code is what gets recorded, and the reference's
`test_network(..., return_history=True)` (experiments/utils.py:22-303).

Run in the build container only (needs the reference tree; never on the GPU box):
    python tests/golden/make_solver_history_golden.py
The reference is imported as make_golden.py imports it.  solver.py imports docplex (not installed): an empty
stand-in module for `docplex.mp.model` (with a placeholder `Model` name) is put into sys.modules first; none of
the recorded classes touches it.  The fixture is data only: weights, graphs, initial spins and every history field.

Cases (all N = 20):
  c0  CUT, SIGNED, DEFAULT_OBSERVABLES          c5  MAX_CLIQUE, MAIN_OBSERVABLES, empty start
  c1  CUT, BINARY                               c6  MIN_DOM_SET, MAIN_OBSERVABLES, full start
  c2  MIN_CUT (+-1 weights)                     c7  S2V: irreversible, DENSE, SPIN_STATE only, MIN_COVER
  c3  MIN_COVER, MAIN_OBSERVABLES, empty start  c8  CUT with EdgeType.RANDOM (float64 uniform(-1, 1)) weights
  c4  MAX_IND_SET, MAIN_OBSERVABLES, full start tn  test_network(return_history=True), one ER-20 graph, 3 attempts
Networks: mpnn_oracle.init_weights(seed, std = STD) rounded to float16 (stored as float16: the float32 values
the reference ran are exactly the stored ones), one per n_obs_in (7, 13, 1).
Condition, asserted here: in every recorded step the reference's top-two Q margin among allowed actions is at
least 1e-4 (the margin tests/test_mpnn_gpu.py uses for teacher-forced rollouts), so an engine within the fp32
bars of the reference picks the same action at every step; no step is excluded from any comparison.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference and the repository on sys.path)
from make_weighted_golden import random_graph  # noqa: E402

for _name in ("docplex", "docplex.mp", "docplex.mp.model"):
    sys.modules.setdefault(_name, types.ModuleType(_name))
sys.modules["docplex.mp.model"].Model = None

from src.agents.solver import Network  # noqa: E402
from src.envs.utils import SpinBasis  # noqa: E402
import experiments.utils as ref_utils  # noqa: E402
from oracle import graphs, mpnn_oracle as mo  # noqa: E402

N, T = 20, 40
STD = 0.1
MARGIN = 1e-4
NET_SEEDS = {7: 11, 13: 12, 1: 13}


def make_network(n_obs_in):
    w = mo.init_weights(torch.Generator().manual_seed(NET_SEEDS[n_obs_in]), std=STD, n_obs_in=n_obs_in)
    w = {k: v.half().float() for k, v in w.items()}
    net = mg.MPNN(n_obs_in=n_obs_in, n_layers=3, n_features=64, n_hid_readout=[], tied_weights=False)
    net.load_state_dict(w)
    net.eval()
    return net, w


def margins(qs, spins, reversible):
    """top-two Q margin among allowed actions of every step row r >= 1 (chosen on the spins of row r - 1)"""
    out = []
    for r in range(1, len(qs)):
        q = np.asarray(qs[r], dtype=np.float64)
        if not reversible:
            q = q[np.asarray(spins[r - 1]) == -1]
        if q.size >= 2:
            top = np.sort(q)[-2:]
            out.append(top[1] - top[0])
    return np.array(out)


def run_case(J, args, n_obs_in, spins, net):
    env = mg.ising_env.make("SpinSystem", mg.SingleGraphGenerator(J), T, **args)
    solver = Network(net, env)
    basis_spins = (spins + 1) // 2 if args["spin_basis"] == SpinBasis.BINARY else spins   # reset's input basis
    solver.reset(basis_spins)
    total = solver.solve()
    h = solver.history
    rec = dict(action=np.array([r[0] for r in h], dtype=np.float64),
               solution=np.array([r[1] for r in h], dtype=np.float64),
               reward=np.array([r[2] for r in h], dtype=np.float64),
               qs=np.array([np.asarray(r[3], dtype=np.float32).reshape(-1) for r in h], dtype=np.float32),
               spins=np.array([r[4] for r in h], dtype=np.float64),
               score_mask=np.array([r[5] for r in h], dtype=np.float64),
               valid=np.array([bool(r[6]) for r in h]),
               total_reward=np.float64(total), measure=np.float64(solver.measure))
    assert len(h[0]) == 7 and all(len(r) == 7 for r in h)
    return rec


def main():
    import random
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    out = {}
    nets = {k: make_network(k) for k in NET_SEEDS}
    for k, (_, w) in nets.items():
        for name, v in w.items():
            out[f"w{k}/{name}"] = v.numpy().astype(np.float16)
    rng = np.random.default_rng(2024)
    empty, full = -np.ones(N, dtype=np.int64), np.ones(N, dtype=np.int64)
    specs = [  # (target, mode, basis, graph weights, start)
        ("CUT", "eco", "SIGNED", "discrete", "random"),
        ("CUT", "eco", "BINARY", "discrete", "random"),
        ("MIN_CUT", "eco", "SIGNED", "discrete", "random"),
        ("MIN_COVER", "eco", "SIGNED", "uniform", "empty"),
        ("MAX_IND_SET", "eco", "SIGNED", "uniform", "full"),
        ("MAX_CLIQUE", "eco", "SIGNED", "uniform", "empty"),
        ("MIN_DOM_SET", "eco", "SIGNED", "uniform", "full"),
        ("MIN_COVER", "s2v", "SIGNED", "uniform", "empty"),
        ("CUT", "eco", "SIGNED", "random", "random"),
    ]
    for ci, (target, mode, basis, wk, start) in enumerate(specs):
        args = mg.problem_args(target, mode, N)
        args["spin_basis"] = SpinBasis[basis]
        n_obs_in = len(args["observables"])
        for attempt in range(50):
            J = random_graph(N, 0.3, rng) if wk == "random" else graphs.er_graph(N, 0.25, rng, wk)
            spins = {"empty": empty, "full": full}.get(start)
            if spins is None:
                spins = 2 * rng.integers(0, 2, N) - 1
            rec = run_case(J, args, n_obs_in, spins, nets[n_obs_in][0])
            m = margins(rec["qs"], rec["spins"], args["reversible_spins"])
            if m.min() >= MARGIN:
                break
        else:
            raise RuntimeError(f"case {ci}: no trajectory with every Q margin >= {MARGIN}")
        print(f"c{ci} {target}/{mode}/{basis}: attempt {attempt}, rows {len(rec['action'])}, min margin {m.min():.3g}, "
              f"measure {rec['measure']}, valid rows {int(rec['valid'].sum())}")
        p = f"c{ci}/"
        out[p + "J"] = J.astype(np.float64) if wk == "random" else J.astype(np.int8)
        out[p + "init_spins"] = spins.astype(np.int8)
        out[p + "target"] = np.array(target)
        out[p + "mode"] = np.array(mode)
        out[p + "basis"] = np.array(basis)
        out[p + "n_obs_in"] = np.int64(n_obs_in)
        out[p + "min_margin"] = np.float64(m.min())
        for k, v in rec.items():
            out[p + k] = v
    out["n_cases"] = np.int64(len(specs))
    out["T"] = np.int64(T)

    # test_network(return_history=True): one ER-20 graph, 3 attempts (reference's batched rollout)
    args = mg.env_args("eco", N)
    for attempt in range(50):
        J = graphs.er_graph(N, 0.25, rng, "discrete")
        seed = 100 + attempt
        np.random.seed(seed)
        res, raw, hist = ref_utils.test_network(nets[7][0], args, [J], device="cpu", step_factor=2, n_attempts=3,
                                                return_raw=True, return_history=True)
        acts = np.array([a[1:] for a in hist["actions"][0]], dtype=np.int64)           # [attempts][steps]
        scores = np.array(hist["scores"][0], dtype=np.float64)                          # [attempts][steps + 1]
        rews = np.array([r[1:] for r in hist["rewards"][0]], dtype=np.float64)
        init = np.array(raw["init spins"][0], dtype=np.int64)
        # the attempts' initial spins in the order this repository's test_network draws them: the global numpy
        # stream after the N draws of the reference env constructor's own reset
        np.random.seed(seed)
        np.random.randint(2, size=N)
        assert np.array_equal(2 * np.random.randint(2, size=(3, N)) - 1, init)
        # margins: re-run the batched forward on the reference env along the recorded actions
        ok = True
        for e in range(3):
            env = mg.ising_env.make("SpinSystem", mg.SingleGraphGenerator(J), 2 * N, **args)
            obs = env.reset(init[e])
            for a in acts[e]:
                with torch.no_grad():
                    q = np.sort(nets[7][0](torch.FloatTensor(obs)).numpy().astype(np.float64))
                ok = ok and (q[-1] - q[-2] >= MARGIN)
                obs, _, _, _ = env.step(int(a))
        if ok:
            break
    else:
        raise RuntimeError("test_network case: no run with every Q margin >= 1e-4")
    print(f"tn: attempt {attempt}, seed {seed}, frame columns {list(hist.columns)}, shapes {acts.shape} {scores.shape}")
    out["tn/J"] = J.astype(np.int8)
    out["tn/seed"] = np.int64(seed)
    out["tn/step_factor"] = np.int64(2)
    out["tn/init_spins"] = init.astype(np.int8)
    out["tn/actions"] = acts
    out["tn/scores"] = scores
    out["tn/rewards"] = rews
    out["tn/columns"] = np.array(list(hist.columns))
    out["tn/cut"] = np.float64(res["cut"][0])
    out["tn/mean_cut"] = np.float64(res["mean cut"][0])
    path = os.path.join(HERE, "solver_history.npz")
    np.savez_compressed(path, **out)
    print("solver_history.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
