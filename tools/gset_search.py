"""configs[4] best-cut search (VERDICT r04 missing #4): the reference's pretrained-agent harness
(experiments/pretrained_agent/test_eco.py:20-112 -> experiments/utils.py:22-303 `test_network`: step_factor 2,
BINARY basis, BLS reward, reversible spins, no basin reward) run to completion with the reference's pretrained
ER-200 network on the G22-like stand-in of bench.py's gset workload (seeded ER(2000, 0.01), unit weights: G22 itself
is absent from the reference, .MISSING_LARGE_BLOBS:1), one GPU's share of configs[4] (1024 attempts in one batch),
beside the Greedy solver (src/agents/solver.py:88-131) from the all -1 state and from each attempt's random start.
No best-known value exists for the stand-in ("parity unpinned"); G22's own best-known cut, 13359
(_graphs/benchmarks/opts/cuts_gset_2000spin.pkl[0]), is a same-size, same-density reference point only.
usage: python tools/gset_search.py [attempts] [seed] [n] [p] [weights]  -> one JSON line"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "eco-dqn_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def cut_of(adj, sol):
    """Cut weight of a 0/1 or +-1 assignment: sum over i < j of w_ij [s_i != s_j]."""
    s = np.where(np.asarray(sol[:adj.shape[0]]) > 0, 1.0, -1.0)
    return float(0.25 * (adj.sum() - s @ adj @ s))


def pretrained_er200(device="cuda"):
    """The reference's network_best_ER_200spin weights as recorded in tests/golden/mpnn_fwd.npz (weights only)."""
    from eco_hip.networks.mpnn import MPNN
    f = np.load(os.path.join(REPO, "tests", "golden", "mpnn_fwd.npz"))
    net = MPNN(device=device)
    net.load_state_dict({k: torch.from_numpy(f["er200/" + k]) for k in net._names})
    return net


def env_args():
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    return {'observables': DEFAULT_OBSERVABLES, 'reward_signal': RewardSignal.BLS,
            'extra_action': ExtraAction.NONE, 'optimisation_target': OptimisationTarget.CUT,
            'spin_basis': SpinBasis.BINARY, 'norm_rewards': True, 'memory_length': None,
            'horizon_length': None, 'stag_punishment': None, 'basin_reward': None, 'reversible_spins': True}


def search(attempts=1024, seed=0, n=2000, p=0.01, graph_seed=1234, weights="uniform"):
    """weights: "uniform" (G22-like) or "discrete" (+-1, as the G-set's toroidal and +-1 random instances); n up to
    ECO_MAX_SPINS_WG = 8192."""
    from eco_hip.graphs import GraphStore
    from eco_hip.experiments import test_network
    adj = GraphStore.random("ER", 1, n, p, seed=graph_seed, weights=weights).dense(0)
    net = pretrained_er200()
    t0 = time.perf_counter()
    res, raw = test_network(net, env_args(), [adj], step_factor=2, n_attempts=attempts, return_raw=True, seed=seed)
    wall = time.perf_counter() - t0
    r = res.iloc[0]
    cuts = np.asarray(raw["cuts"][0])
    return {
        "workload": f"configs[4] G22-like stand-in ER({n}, {p}) {weights} weights, graph seed {graph_seed}: "
                    f"{attempts} attempts x T = {2 * n} (step_factor 2), pretrained ER-200 network",
        "edges": int((adj != 0).sum() // 2),
        "cut": float(r["cut"]), "cut_recomputed_from_sol": cut_of(adj, r["sol"]),
        "mean_cut": float(r["mean cut"]), "median_cut": float(np.median(cuts)),
        "greedy_all_minus1": float(r["greedy (+1 init) cut"]),
        "greedy_random_best": float(r["greedy (rand init) cut"]),
        "greedy_random_mean": float(r["greedy (rand init) mean cut"]),
        "network_s_per_attempt_batched": float(r["time"]), "wall_s": wall,
        "g22_best_known_for_context": 13359,
    }


if __name__ == "__main__":
    a = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    s = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    kw = {}
    if len(sys.argv) > 3:   # [n] [p] [weights]: another stand-in, e.g. 3000 0.001334 discrete (about 6000 +-1 edges)
        kw["n"] = int(sys.argv[3])
    if len(sys.argv) > 4:
        kw["p"] = float(sys.argv[4])
    if len(sys.argv) > 5:
        kw["weights"] = sys.argv[5]
    print(json.dumps(search(a, s, **kw)), flush=True)
