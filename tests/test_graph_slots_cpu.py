"""Graph-slot bookkeeping of DQN(regenerate_graphs=...) on the CPU, against the values recorded from the commit
before the DQN class was split (tests/golden/graph_slots_parent.npz, recorder beside it): for every scripted
scenario of tests/graph_slots_scenarios.py the returned ids, the generate calls with their seeds (which pins the
order of the draws from the agent's rng) and the regenerated / reused counts and the warning are reproduced
exactly, both by GraphSlotRing driven directly and by the unbound DQN._take_graph_slots on a stub agent."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from graph_slots_scenarios import SCENARIOS, drive


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "graph_slots_parent.npz"))


def _ring(sc, log):
    from eco_hip.agents.dqn.graph_slots import GraphSlotRing
    return GraphSlotRing(sc["n_slots"], sc["replay"], np.random.default_rng(sc["seed"]),
                         lambda first, count, seed: log.append((first, count, seed)))


def _check(parent, name, calls, log, ring):
    """calls: drive()'s generator.  Compares every call with the recording and asserts the ring's invariants."""
    n = 0
    for i, (mask, ids, warned) in enumerate(calls):
        np.testing.assert_array_equal(ids, parent[f"{name}/{i}/ids"], err_msg=f"{name} call {i}")
        np.testing.assert_array_equal(np.array(log, np.int64).reshape(-1, 3), parent[f"{name}/{i}/generate"],
                                      err_msg=f"{name} call {i}")
        counts = [ring.regenerated, ring.reused] if ring is not None else [0, 0]
        assert counts + [int(warned)] == parent[f"{name}/{i}/counts"].tolist(), (name, i)
        if ring is not None:
            assert (ring.users >= 0).all(), (name, i)
            assert ring.users.sum() == SCENARIOS[name]["B"]   # one slot use per live episode
        log.clear()
        n += 1
    assert f"{name}/{n}/ids" not in parent.files and n > 0   # every recorded call was replayed


@pytest.mark.parametrize("name", [k for k, sc in SCENARIOS.items() if sc["n_slots"] is not None])
def test_ring_reproduces_parent(parent, name):
    sc, log = SCENARIOS[name], []
    ring = _ring(sc, log)
    stub = SimpleNamespace(_pushed=0, _host_graph_ids=None)
    released = []   # (slot, push count) of every release that left the slot without a user
    generate = ring._generate

    def checked_generate(first, count, seed):
        # a regenerated slot has no user and was released at least `replay` pushes ago
        for s in range(first, first + count):
            assert ring.users[s] == 0
            assert stub._pushed - ring.free_at[s] >= sc["replay"]
        generate(first, count, seed)
    ring._generate = checked_generate

    def take(mask):
        k = sc["B"] if mask is None else int(mask.sum())
        if stub._host_graph_ids is not None:
            old = stub._host_graph_ids if mask is None else stub._host_graph_ids[mask]
            ring.release(old, stub._pushed)
            released.extend(old.tolist())
        ids = ring.take(k, stub._pushed)
        if mask is None:
            return ids
        out = np.zeros(sc["B"], np.int64)
        out[mask] = ids
        return out
    _check(parent, name, drive(sc["ops"], stub, take), log, ring)
    assert released


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_take_graph_slots_reproduces_parent(parent, name):
    """DQN._take_graph_slots (pool or ring, then one scatter) on a stub agent: the method touches no device."""
    from eco_hip.agents.dqn.dqn import DQN
    sc, log = SCENARIOS[name], []
    ring = _ring(sc, log) if sc["n_slots"] is not None else None
    rng = ring._rng if ring is not None else np.random.default_rng(sc["seed"])
    stub = SimpleNamespace(B=sc["B"], _pushed=0, _host_graph_ids=None, _slots=ring, _rng=rng,
                           graph_pool_ids=sc.get("pool"))
    _check(parent, name, drive(sc["ops"], stub, lambda mask: DQN._take_graph_slots(stub, mask)), log, ring)


def test_recorded_scenarios_hold_what_they_are_for(parent):
    """The fixture itself: (a) never reuses; (b) reuses and warns once; (c) has a call with no safe slot and a
    call whose safe slots form two runs without a wrap; (d) has a call whose fresh slots straddle the ring's end."""
    def calls(name):
        i = 0
        while f"{name}/{i}/ids" in parent.files:
            yield parent[f"{name}/{i}/ids"], parent[f"{name}/{i}/generate"], parent[f"{name}/{i}/counts"]
            i += 1
    assert all(c[1] == 0 and c[2] == 0 for _, _, c in calls("a_exact"))
    b = list(calls("b_short"))
    assert b[-1][2][1] > 0 and sum(c[2] for _, _, c in b) == 1
    c = list(calls("c_masked"))
    assert any(len(g) == 0 for _, g, _ in c[1:])
    assert any(len(g) == 2 and g[1, 0] > g[0, 0] + g[0, 1] for _, g, _ in c)
    assert any(len(g) == 2 and g[1, 0] == 0 and g[0, 0] + g[0, 1] == SCENARIOS["d_wrap"]["n_slots"]
               for _, g, _ in calls("d_wrap"))
