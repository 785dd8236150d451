"""Shared pieces of the solver / trajectory-history tests: the cases of tests/golden/solver_history.npz, the env
arguments they ran with, and `replay`, which rebuilds a Network-solver history (src/agents/solver.py:198-265)
from an action sequence with the CPU oracles -- ProblemSpinSystemOracle for the env and its scorer,
mpnn_oracle.forward for the Q-values."""
import os

import numpy as np
import torch

from oracle import mpnn_oracle as mo
from oracle import problems_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("action", "solution", "reward", "qs", "spins", "score_mask", "valid")
_cache = {}


def fixture():
    if "f" not in _cache:
        _cache["f"] = np.load(os.path.join(GOLDEN, "solver_history.npz"))
    return _cache["f"]


def weights(n_obs_in):
    """The fixture's network for n_obs_in observables (stored as float16, exactly the float32 values run)."""
    f = fixture()
    return {k: torch.from_numpy(f[f"w{n_obs_in}/{k}"].astype(np.float32)) for k in mo.KEYS}


def case(ci):
    f = fixture()
    p = f"c{ci}/"
    c = {k: f[p + k] for k in FIELDS + ("J", "init_spins", "total_reward", "measure")}
    c.update(target=str(f[p + "target"]), mode=str(f[p + "mode"]), basis=str(f[p + "basis"]),
             n_obs_in=int(f[p + "n_obs_in"]), T=int(f["T"]), J=c["J"].astype(np.float64))
    return c


def oracle_kwargs(target, mode, basis, n):
    """The env arguments of the fixture cases (experiments/train_eco.py:244-315, as tests/golden/make_golden.py's
    problem_args) for ProblemSpinSystemOracle."""
    kw = dict(target=getattr(po, target), reward_signal="BLS", norm_rewards=True, basin_reward=1. / n,
              reversible_spins=True, spin_basis=basis,
              observables=po.DEFAULT_OBSERVABLES if target in ("CUT", "MIN_CUT") else po.MAIN_OBSERVABLES)
    if mode == "s2v":
        kw.update(observables=[po.SPIN_STATE], reversible_spins=False, basin_reward=None, reward_signal="DENSE")
    return kw


def env_kwargs(target, mode, basis, n):
    """The same arguments for eco_hip's VecSpinSystem."""
    from eco_hip.envs import utils as u
    ok = oracle_kwargs(target, mode, basis, n)
    return dict(observables=[u.Observable(o) for o in ok["observables"]],
                reward_signal=u.RewardSignal[ok["reward_signal"]], extra_action=u.ExtraAction.NONE,
                optimisation_target=u.OptimisationTarget[target], spin_basis=u.SpinBasis[basis],
                norm_rewards=True, basin_reward=ok["basin_reward"], reversible_spins=ok["reversible_spins"])


def make_oracle(J, T, target, mode, basis, init_spins):
    """The oracle env as the fixture maker builds the reference's: constructed on J (one reset, which leaves J's
    invalidity normaliser behind), then reset onto the signed init_spins."""
    o = po.ProblemSpinSystemOracle(J, T, rng=np.random.RandomState(0), **oracle_kwargs(target, mode, basis, J.shape[0]))
    s = np.asarray(init_spins, dtype=np.int64)
    o.reset(spins=(s + 1) // 2 if basis == "BINARY" else s)
    return o


def replay(J, T, target, mode, basis, init_spins, actions, w=None, n_obs_in=None):
    """History rows of the episode that starts at init_spins ([N], signed) and takes `actions` (row r >= 1 is the
    state after actions[r - 1]), stopping after the step that reports done.  w: network weights for the qs column
    (the Q-values of the observation each action was taken on); None leaves qs out.  Also returns the per-row
    scorer.get_score and the done flag after each row."""
    o = make_oracle(J, T, target, mode, basis, init_spins)
    n = J.shape[0]
    sc = o.scorer

    def row(action, reward, q):
        s = o.state[0, :].copy()
        return dict(action=float(action), solution=float(sc.solution(s, o.matrix)), reward=float(reward), qs=q,
                    spins=s, score_mask=np.asarray(sc.score_mask(s, o.matrix), dtype=np.float64),
                    valid=bool(sc.valid(s, o.matrix)), score=float(sc.score(s, o.matrix)))

    rows = [row(0, 0, np.zeros(n, np.float32))]
    dones = [False]
    for a in actions:
        q = np.zeros(n, np.float32)
        if w is not None:
            with torch.no_grad():
                q = mo.forward(w, torch.from_numpy(o.get_observation()).float(), n_obs_in).numpy()
        _, rew, done, _ = o.step(int(a))
        rows.append(row(a, rew, q))
        dones.append(done)
        if done:
            break
    out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    out["done"] = np.array(dones)
    return out


def allowed_argmax(q, prev_spins, reversible):
    """first-index argmax of q over allowed vertices (irreversible: spins still at -1)"""
    q = np.asarray(q, dtype=np.float64)
    if not reversible:
        q = np.where(np.asarray(prev_spins) == -1, q, -np.inf)
    return int(q.argmax())
