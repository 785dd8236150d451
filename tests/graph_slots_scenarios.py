"""Scripted graph-slot scenarios shared by tests/golden/make_graph_slots_parent.py (which recorded
tests/golden/graph_slots_parent.npz from the commit before the DQN class was split) and
tests/test_graph_slots_cpu.py (which replays them on GraphSlotRing and DQN._take_graph_slots).

A scenario is a list of operations on an agent of B episodes:
  ("start",)        DQN.start(): every episode reset (a second one after pushes = a second learn())
  ("reset", mask)   the episodes of `mask` (bool, B-long; None = all) end and are reset
  ("push", n)       n transitions are pushed to the replay buffer
"""
import numpy as np


def _full(batches, per_batch):
    ops = [("start",)]
    for _ in range(batches):
        ops += [("push", per_batch), ("reset", None)]
    return ops


def _masked(B, steps, seed):
    rng = np.random.default_rng(seed)
    ops = [("start",)]
    for _ in range(steps):
        mask = rng.random(B) < 0.4
        if not mask.any():
            mask[int(rng.integers(B))] = True
        ops += [("push", B), ("reset", mask)]
    return ops


B, T, REPLAY = 4, 3, 24   # graph_slots_needed(4, 3, 24) == 12

SCENARIOS = {
    # (a) full resets, ring exactly graph_slots_needed long: no reuse
    "a_exact": dict(B=B, replay=REPLAY, n_slots=12, seed=11, ops=_full(8, B * T)),
    # (b) one batch too few: reuse and one warning
    "b_short": dict(B=B, replay=REPLAY, n_slots=8, seed=12, ops=_full(8, B * T)),
    # (c) irregular masked resets: a step with no safe slot and a step whose safe slots form two runs
    "c_masked": dict(B=B, replay=8, n_slots=9, seed=13, ops=_masked(B, 24, 0)),
    # (d) the cursor wraps inside one request: its fresh slots straddle the end of the ring
    "d_wrap": dict(B=B, replay=4, n_slots=10, seed=14, ops=_full(6, B)),
    # (e) a second start() after pushes: the live episodes' slots are released once
    "e_restart": dict(B=B, replay=REPLAY, n_slots=12, seed=15,
                      ops=_full(3, B * T) + [("push", 5)] + _full(3, B * T) + [("push", 7)] + _masked(B, 6, 3)),
    # (f) no regeneration: random graphs of the pool, full and masked
    "f_pool": dict(B=B, replay=REPLAY, n_slots=None, seed=16, pool=np.arange(100, 120),
                   ops=_full(3, B * T) + _masked(B, 6, 4)[1:]),
}


def drive(ops, stub, take):
    """Run `ops` with take(mask) -> graph ids, keeping the host mirror of DQN._reset_env
    (stub._host_graph_ids) and the push count (stub._pushed) as the agent does.  Yields
    (mask, ids, warned) per start / reset."""
    import warnings
    for op in ops:
        if op[0] == "push":
            stub._pushed += op[1]
            continue
        mask = None if op[0] == "start" else op[1]
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            ids = take(mask)
        ids = np.asarray(ids, np.int64)
        if mask is None or stub._host_graph_ids is None:
            stub._host_graph_ids = ids.copy()
        else:
            stub._host_graph_ids[mask] = ids[mask]
        yield mask, ids, any(issubclass(x.category, RuntimeWarning) for x in w)
