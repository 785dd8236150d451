"""Recorder of tests/golden/graph_slots_parent.npz.  Run at commit fbddfea (the parent of the commit
that split the DQN class): it drives that commit's unbound DQN._take_graph_slots, which touches no
device, on a stub object whose graphs.generate logs (first, count, seed).

    python tests/golden/make_graph_slots_parent.py

Per scenario of tests/graph_slots_scenarios.py and per start / reset call i the file holds
  <scenario>/<i>/ids          the returned graph ids
  <scenario>/<i>/generate     the (first, count, seed) rows of the generate calls, in order
  <scenario>/<i>/counts       graphs_regenerated, graphs_reused after the call, and whether it warned
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "eco-dqn_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from eco_hip.agents.dqn.dqn import DQN  # noqa: E402
from graph_slots_scenarios import SCENARIOS, drive  # noqa: E402


def record(sc):
    log = []
    graphs = SimpleNamespace(float_weights=False,
                             generate=lambda first, count, kind, param, seed, weights, check:
                             log.append((first, count, seed)))
    stub = SimpleNamespace(B=sc["B"], graphs=graphs, replay_buffer_size=sc["replay"], _pushed=0,
                           _rng=np.random.default_rng(sc["seed"]), _started=False, _host_graph_ids=None,
                           graph_pool_ids=sc.get("pool"), regenerate_graphs=None)
    if sc["n_slots"] is not None:
        stub.regenerate_graphs = ("ER", 0.15)
        stub._slot_users = np.zeros(sc["n_slots"], np.int64)
        stub._slot_free_at = np.full(sc["n_slots"], -(1 << 62), np.int64)
        stub._slot_cursor = 0
        stub._slot_warned = False
        stub.graphs_regenerated = stub.graphs_reused = 0

    def take(mask):
        ids = DQN._take_graph_slots(stub, mask)
        stub._started = True
        return ids

    out = {}
    for i, (mask, ids, warned) in enumerate(drive(sc["ops"], stub, take)):
        out[f"{i}/ids"] = ids
        out[f"{i}/generate"] = np.array(log, np.int64).reshape(-1, 3)
        out[f"{i}/counts"] = np.array([getattr(stub, "graphs_regenerated", 0), getattr(stub, "graphs_reused", 0),
                                       int(warned)], np.int64)
        log.clear()
    return out


if __name__ == "__main__":
    data = {f"{name}/{k}": v for name, sc in SCENARIOS.items() for k, v in record(sc).items()}
    np.savez_compressed(os.path.join(HERE, "graph_slots_parent.npz"), **data)
    print("recorded", len(data), "arrays")
