"""Device prioritised replay without a GPU: the new entries are declared and exported, the integer oracle
(tests/prio_common.py) has the properties the sampler is specified by, and bad arguments are rejected before any
launch (so these calls need no device, as in tests/test_abi_cpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import prio_common as pc
from conftest import REPO

NEW_EXPORTS = ["eco_prio_workspace_bytes", "eco_prio_push", "eco_prio_sample", "eco_prio_update",
               "eco_dqn_td_weighted", "eco_replay_compact_gather"]


def test_new_entries_are_declared_bound_and_exported():
    from eco_hip import _lib
    src = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(eco_[a-z0-9_]+)\s*\(", src))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.eco_prio_workspace_bytes(0) == 0
    # header + two uint64 and one uint32 per 1024-entry block, each array rounded up to 256 B
    assert _lib.lib.eco_prio_workspace_bytes(5000) == 256 * 4
    nb = (3280000 + 1023) // 1024
    assert _lib.lib.eco_prio_workspace_bytes(3280000) >= 256 + 20 * nb


@pytest.mark.parametrize("S,m", [(0, 1), (1, 1), (3, 4), (4, 4), (1000, 7), ((1 << 31) - 1, 257),
                                 (5000 * ((1 << 31) - 1), 65536), ((1 << 62) + 12345, 65536)])
def test_strata_tile_the_total_mass_exactly(S, m):
    lo = pc.strata(S, m)
    assert len(lo) == m + 1 and lo[0] == 0 and lo[-1] == S
    widths = [b - a for a, b in zip(lo[:-1], lo[1:])]
    assert min(widths) >= 0 and sum(widths) == S and max(widths) - min(widths) <= 1
    # lo_k = q k + (r k) // m fits a uint64 for m <= 65536 (r < m, so r k < 2^32)
    q, r = divmod(S, m)
    assert q * m + r * m // m < 1 << 64 and r * m < 1 << 32
    for k, u in enumerate(pc.draws(S, m, seed=5, counter=9)):
        assert lo[k] <= u < max(lo[k + 1], lo[k] + 1)


def test_zero_mass_and_positions_beyond_size_are_never_drawn():
    rng = np.random.default_rng(0)
    cap, size = 300, 211
    mass = rng.integers(1, 1 << 20, cap)
    mass[rng.random(cap) < 0.3] = 0
    mass[5] = 7
    for counter in range(20):
        idx = pc.sample(mass, size, 64, seed=1, counter=counter)
        assert idx.min() >= 0 and idx.max() < size
        assert (mass[idx] > 0).all()
    # every positive position can be drawn: m = S single-unit strata draw each unit of mass once
    small = np.array([0, 2, 0, 1, 3, 0])
    idx = pc.sample(small, 5, 6, seed=3, counter=1)
    assert idx.tolist() == [1, 1, 3, 4, 4, 4]


@pytest.mark.parametrize("seed", [0, 1, 12345, (1 << 64) - 1])
def test_masses_one_and_three_give_position_one_three_times_of_four(seed):
    for counter in range(8):
        idx = pc.sample([1, 3], 2, 4, seed, counter)
        assert sorted(idx.tolist()) == [0, 1, 1, 1]


def test_push_mass_and_weights_of_the_oracle():
    mass = [0] * 10
    assert pc.push(mass, 8, 4, 0) == pc.PRIO_ONE          # empty buffer: the mass of p = 1, wrapping
    assert mass == [pc.PRIO_ONE] * 2 + [0] * 6 + [pc.PRIO_ONE] * 2
    mass[9] = 99999
    mass[1] = 5
    assert pc.push(mass, 2, 3, 2) == pc.PRIO_ONE          # the maximum over the first size_before = 2 only
    assert pc.push(mass, 5, 1, 10) == 99999
    # the mass formula: alpha = 0 is 2^16 whatever |td|; clamps at td_max and at [1, 2^31 - 1]
    td = np.array([0, 1e-6, 0.5, 1.0, 10.0, np.nan], np.float32)
    assert pc.mass_of(td, 0.0, 1e-3, 1.0).tolist() == [65536] * 6
    m1 = pc.mass_of(td, 1.0, 1e-3, 1.0)
    assert m1[0] == 66 and m1[3] == m1[4] == m1[5] == round(1.001 * 65536) and m1[2] == round(0.501 * 65536)
    assert pc.mass_of([0.0], 0.6, 0.0, 1.0).tolist() == [1]
    assert pc.mass_of([1e9], 2.0, 0.0, 1e9).tolist() == [pc.PRIO_MAX]
    # weights: equal masses give exactly 1; beta = 0 gives exactly 1; otherwise the rarest sample has weight 1
    eq = pc.weights([7] * 8, 8, [0, 3, 3, 7], 0.4)
    assert eq.tolist() == [1.0] * 4
    assert pc.weights([1, 3, 9], 3, [0, 1, 2], 0.0).tolist() == [1.0] * 3
    w = pc.weights([1, 3, 9], 3, [2, 0, 1], 0.5)
    assert w[1] == 1.0 and w[0] == np.float32(1 / 3) and abs(float(w[2]) - 3 ** -0.5) < 1e-7


@pytest.mark.parametrize("size", [1, 37, 1024, 1025, 5000])
@pytest.mark.parametrize("pattern", ["equal", "random", "zeros30", "giant"])
def test_fast_paths_equal_the_python_int_oracle(pattern, size):
    """sample_fast / weights_fast (uint64 cumsum + searchsorted, what the large-ring GPU tests are judged by) against
    sample / weights (Python ints) on the 5000-entry patterns of tests/test_prio_gpu.py: exactly equal."""
    mass = pc.mass_pattern(pattern, size)
    for m in (1, 64, 257):
        for counter in (3, 4):
            ref = pc.sample(mass, size, m, 0xC0FFEE, counter)
            fast = pc.sample_fast(mass, size, m, 0xC0FFEE, counter)
            assert fast.dtype == ref.dtype and np.array_equal(fast, ref), (pattern, size, m)
            w, wf = pc.weights(mass, size, ref, 0.4), pc.weights_fast(mass, size, ref, 0.4)
            assert wf.dtype == np.float32 and np.array_equal(w.view(np.int32), wf.view(np.int32))
    with pytest.raises(AssertionError, match="2\\^63"):
        pc.sample_fast(np.broadcast_to(np.int8(1), (1 << 32,)), 4, 1, 1, 1)   # capacity * 2^31 reaches 2^63


def _sample_without_cross_wave_term(mass, size, m, seed, counter):
    """sample_fast with the defect the 65,537-entry case guards against: prio_scan_kernel without its cross-wave
    term `for k < w: acc += ws[k]`, so that the prefix restarts at block 64 (the first block of the second wave at
    chunk = 1).  The total S is right: the kernel sums it separately."""
    v = np.asarray(mass[:size]).astype(np.uint64)
    prefix = np.cumsum(v, dtype=np.uint64)
    S = int(prefix[-1])
    cut = 64 * pc.PRIO_BLOCK
    if size > cut:
        prefix[cut:] -= prefix[cut - 1]
    u = np.array(pc.draws(S, m, seed, counter), dtype=np.uint64)
    return np.searchsorted(prefix, u, side="right").astype(np.int64)


def test_oracle_notices_a_prefix_that_restarts_at_block_64():
    cap = 3280000
    for size, differs in ((65536, False), (65537, True)):
        mass = pc.large_ring_pattern("tail", size, cap)
        ref = pc.sample_fast(mass, size, 2048, 0xC0FFEE, 3)
        bad = _sample_without_cross_wave_term(mass, size, 2048, 0xC0FFEE, 3)
        # 65,537: position 65,536 holds 1 / 700 of the mass, 2.9 of the 2048 strata: the true sampler draws it, the
        # restarted prefix (2^31 - 1 there, below every such draw) cannot
        assert np.array_equal(ref, bad) != differs, size
        if differs:
            assert (ref == size - 1).sum() >= 2 and not (bad == size - 1).any()
    assert ref.max() < size and (mass[ref] > 0).all()


def test_large_ring_patterns():
    cap = 3280000
    for size in (65537, cap):
        for pattern in ("tail", "head"):
            mass = pc.large_ring_pattern(pattern, size, cap)
            big = np.flatnonzero(mass == pc.PRIO_MAX)
            assert big.size == 700 and (mass != pc.PRIO_MAX).sum() == cap - 700 and mass.min() == 1
            assert (big[0], big[-1]) == ((size - 700, size - 1) if pattern == "tail" else (0, 699))
        z = pc.large_ring_pattern("zeros30", size, cap)
        assert 0.25 < (z == 0).mean() < 0.35 and z.max() <= 1 << 20


def test_bad_arguments_are_rejected_before_any_launch():
    from eco_hip import _lib
    buf = (ctypes.c_uint32 * 64)()          # host memory: never touched, the checks come first
    a16 = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(a16)
    sample = lambda cap, size, m, beta=0.4: _lib.lib.eco_prio_sample(   # noqa: E731
        p, cap, size, m, ctypes.c_uint64(1), ctypes.c_uint64(1), beta, p, p, p, None)
    for cap, size, m in [(16, 0, 4), (16, -1, 4), (16, 8, 0), (16, 8, -3), (16, 8, 65537), (16, 17, 4)]:
        assert sample(cap, size, m) == _lib.ECO_ERR_ARG, (cap, size, m)
        assert "prio sample: need 1 <= size <= capacity and 1 <= m <= 65536" in _lib.last_error()
    for beta in (-0.1, float("nan"), float("inf")):
        assert sample(16, 8, 4, beta) == _lib.ECO_ERR_ARG and "beta" in _lib.last_error()
    assert _lib.lib.eco_prio_sample(None, 16, 8, 4, ctypes.c_uint64(1), ctypes.c_uint64(1), 0.4, p, p, p,
                                    None) == _lib.ECO_ERR_ARG
    assert _lib.lib.eco_prio_sample(ctypes.c_void_p(a16 + 4), 16, 8, 4, ctypes.c_uint64(1), ctypes.c_uint64(1), 0.4,
                                    p, p, p, None) == _lib.ECO_ERR_ARG and "aligned" in _lib.last_error()
    push = lambda cap, pos, batch, size: _lib.lib.eco_prio_push(p, cap, pos, batch, size, p, None)   # noqa: E731
    for cap, pos, batch, size in [(0, 0, 1, 0), (16, 0, 0, 0), (16, 0, 17, 0), (16, 16, 1, 0), (16, -1, 1, 0),
                                  (16, 0, 1, 17), (16, 0, 1, -1)]:
        assert push(cap, pos, batch, size) == _lib.ECO_ERR_ARG, (cap, pos, batch, size)
    update = lambda m, alpha, eps, td_max: _lib.lib.eco_prio_update(p, 16, m, p, p, alpha, eps, td_max, None)   # noqa: E731
    for m, alpha, eps, td_max in [(0, 0.6, 1e-3, 1.0), (4, -0.1, 1e-3, 1.0), (4, 0.6, -1.0, 1.0), (4, 0.6, 1e-3, 0.0),
                                  (4, float("nan"), 1e-3, 1.0), (4, 0.6, 1e-3, float("inf"))]:
        assert update(m, alpha, eps, td_max) == _lib.ECO_ERR_ARG, (m, alpha, eps, td_max)
    with pytest.raises(ValueError):
        _lib.check(sample(16, 0, 4))


def test_prioritised_config_fills_defaults_and_rejects_unknown_keys():
    from eco_hip.agents.dqn.prioritised import PRIORITISED_DEFAULTS, prioritised_config
    assert PRIORITISED_DEFAULTS["alpha"] == 0.6 and PRIORITISED_DEFAULTS["beta0"] == 0.4
    assert PRIORITISED_DEFAULTS["eps"] == 1e-3 and PRIORITISED_DEFAULTS["td_max"] == 1.0
    assert prioritised_config({}) == PRIORITISED_DEFAULTS
    assert prioritised_config({"alpha": 0.0, "beta_steps": 10})["beta_steps"] == 10
    with pytest.raises(ValueError, match="unknown keys"):
        prioritised_config({"alpha": 0.5, "gamma": 1})
    with pytest.raises(ValueError):
        prioritised_config(True)
