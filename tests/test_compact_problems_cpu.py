"""Compact replay ring for the set-problem targets without a GPU: the bytes query that takes the env config is
declared, bound and exported, agrees with the old query for OptimisationTarget.CUT, grows by the wider scalars only
for the five generic-scorer targets, and is 0 for every config the ring rejects; the ring's entry points reject
those configs before any launch (so these calls need no device, as in tests/test_abi_cpu.py)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

SET_TARGETS = ["MIN_COVER", "MIN_CUT", "MAX_IND_SET", "MAX_CLIQUE", "MIN_DOM_SET"]


def _cfg(n, T, target="CUT", **over):
    from eco_hip.envs.batched import make_config
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, MAIN_OBSERVABLES, RewardSignal, ExtraAction,
                                    OptimisationTarget)
    obs = DEFAULT_OBSERVABLES if target in ("CUT", "MIN_CUT") else MAIN_OBSERVABLES
    args = dict(observables=obs, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                optimisation_target=OptimisationTarget[target])
    args.update(over)
    return make_config(n, T, **args)


def test_bytes_cfg_is_declared_bound_and_exported():
    from eco_hip import _lib
    src = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"size_t\s+eco_replay_compact_bytes_cfg\s*\(\s*const\s+eco_env_config\s*\*", src)
    assert re.search(r"size_t\s+eco_replay_compact_bytes\s*\(\s*int32_t\s+n_spins", src)   # the old query stays
    assert "eco_replay_compact_bytes_cfg" in _lib.EXPORTS
    assert hasattr(_lib.lib, "eco_replay_compact_bytes_cfg")


@pytest.mark.parametrize("n,cap,B", [(20, 320, 64), (200, 3280000, 8192), (8192, 1000, 3)])
def test_cut_config_sizes_the_ring_as_before(n, cap, B):
    from eco_hip import _lib
    old = _lib.lib.eco_replay_compact_bytes(n, cap, B)
    assert old > 0
    assert _lib.lib.eco_replay_compact_bytes_cfg(ctypes.byref(_cfg(n, 2 * n)), cap, B) == old


@pytest.mark.parametrize("target", SET_TARGETS)
@pytest.mark.parametrize("n,cap,B", [(20, 320, 64), (200, 3280000, 8192), (2048, 1000, 3)])
def test_set_targets_add_the_wider_scalars_only(target, n, cap, B):
    from eco_hip import _lib
    al = lambda x: (x + 255) // 256 * 256   # noqa: E731
    P = cap + B
    old = _lib.lib.eco_replay_compact_bytes(n, cap, B)
    new = _lib.lib.eco_replay_compact_bytes_cfg(ctypes.byref(_cfg(n, 2 * n, target)), cap, B)
    # six f64 scalars for s and for s' instead of four, each array rounded up to 256 B
    assert new - old == 2 * (al(P * 6 * 8) - al(P * 4 * 8))
    # the bound of the layout: at most 12 doubles per state
    assert 0 < new - old <= 2 * 8 * (12 - 4) * P + 2 * 256
    assert new / P <= 4 * n + 2 * 8 * 12 + 16 + 7 * 256 / P


def test_rejected_configs_size_to_zero_with_a_message():
    from eco_hip import _lib
    q = _lib.lib.eco_replay_compact_bytes_cfg
    assert q(None, 64, 8) == 0
    for target in ["CUT"] + SET_TARGETS:
        cfg = _cfg(20, 40, target)
        assert q(ctypes.byref(cfg), 64, 8) > 0
        assert q(ctypes.byref(cfg), 0, 8) == 0 and q(ctypes.byref(cfg), 64, 0) == 0
        cfg.max_steps = 32768
        assert q(ctypes.byref(cfg), 64, 8) == 0 and "max_steps must be < 32768" in _lib.last_error()
        cfg.max_steps = 40
        cfg.float_weights = 1
        assert q(ctypes.byref(cfg), 64, 8) == 0 and "integer weights only" in _lib.last_error()
        cfg.float_weights = 0
        cfg.n_spins = 2049
        if target == "CUT":
            assert q(ctypes.byref(cfg), 64, 8) == _lib.lib.eco_replay_compact_bytes(2049, 64, 8) > 0
        else:
            assert q(ctypes.byref(cfg), 64, 8) == 0 and "n_spins <= 2048" in _lib.last_error()
        cfg.n_spins = 8193
        assert q(ctypes.byref(cfg), 64, 8) == 0
    cfg = _cfg(20, 40)
    cfg.optimisation_target = _lib.ECO_TARGET_ENERGY
    assert q(ctypes.byref(cfg), 64, 8) == 0 and "OptimisationTarget" in _lib.last_error()


@pytest.mark.parametrize("target", SET_TARGETS)
def test_entry_points_reject_before_any_launch(target):
    """Host memory stands in for every buffer: the checks come first, so nothing is read or written."""
    from eco_hip import _lib
    buf = (ctypes.c_uint8 * 256)(*([0xAB] * 256))
    p = ctypes.c_void_p(ctypes.addressof(buf))
    gs = _lib.GraphSet()
    gs.n_spins = 20

    def reads(cfg):
        c = ctypes.byref(cfg)
        return [_lib.lib.eco_replay_compact_sample(c, p, ctypes.byref(gs), 8, p, 64, 8, 8, 4, ctypes.c_uint64(1),
                                                   ctypes.c_uint64(1), p, p, p, p, p, p, None),
                _lib.lib.eco_replay_compact_gather(c, p, ctypes.byref(gs), 8, p, 64, 8, 8, 4, p, p, p, p, p, p, p,
                                                   None)]

    def calls(cfg):
        c = ctypes.byref(cfg)
        return [_lib.lib.eco_replay_compact_snapshot(c, p, 8, p, 64, 0, None, None),
                _lib.lib.eco_replay_compact_push(c, p, 8, p, 64, 0, p, p, p, None)] + reads(cfg)

    cfg = _cfg(20, 40, target)
    cfg.max_steps = 32768
    assert calls(cfg) == [_lib.ECO_ERR_ARG] * 4 and "max_steps" in _lib.last_error()
    cfg.max_steps = 40
    cfg.float_weights = 1
    assert calls(cfg) == [_lib.ECO_ERR_ARG] * 4 and "integer weights only" in _lib.last_error()
    cfg.float_weights = 0
    cfg.n_spins = gs.n_spins = 2049
    assert calls(cfg) == [_lib.ECO_ERR_ARG] * 4 and "n_spins <= 2048" in _lib.last_error()
    # a float-weighted graph set under an integer config: the two calls that read the graph refuse it
    cfg.n_spins = gs.n_spins = 20
    gs.edge_weights = ctypes.addressof(buf)
    assert reads(cfg) == [_lib.ECO_ERR_ARG] * 2 and "float-weighted graph set" in _lib.last_error()
    assert bytes(buf) == b"\xab" * 256
