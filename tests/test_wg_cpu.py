"""Host-side contract of the 2048 < N <= 8192 range (no GPU): the new exports are declared in include/eco_hip.h and
bound in eco_hip/_lib.py, the byte queries are monotone in the batch and zero outside their range, and the env state
layout is unchanged up to ECO_MAX_SPINS."""
import ctypes
import os
import re

from conftest import REPO

NEW_EXPORTS = ("eco_mpnn_forward_wg", "eco_mpnn_forward_wg_workspace_bytes")


def _cfg(n, T, **over):
    from eco_hip.envs.batched import make_config
    from eco_hip.envs.utils import DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget
    args = dict(observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS, extra_action=ExtraAction.NONE,
                optimisation_target=OptimisationTarget.CUT)
    args.update(over)
    return make_config(n, T, **args)


def test_new_exports_are_declared_and_bound():
    from eco_hip import _lib
    src = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    assert re.search(r"#define\s+ECO_MAX_SPINS\s+2048\b", src)
    assert re.search(r"#define\s+ECO_MAX_SPINS_WG\s+8192\b", src)
    assert _lib.ECO_MAX_SPINS == 2048 and _lib.ECO_MAX_SPINS_WG == 8192
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.lib.eco_mpnn_forward_wg_workspace_bytes.restype is ctypes.c_size_t
    assert len(_lib.lib.eco_mpnn_forward_wg.argtypes) == 12    # eco_mpnn_forward's 13 without `saved`


def test_forward_wg_workspace_bytes():
    from eco_hip import _lib
    q = _lib.lib.eco_mpnn_forward_wg_workspace_bytes
    for n in (-1, 0, 1, 512, 2000, 2048, 8193, 20000):
        assert q(n, 4, 7) == 0, n
    assert q(2049, 0, 7) == 0 and q(2049, -3, 7) == 0
    assert q(2049, 4, 0) == 0 and q(2049, 4, 17) == 0
    for n in (2049, 2064, 2065, 3000, 4100, 8191, 8192):
        rows_pad = (n + 15) // 16 * 16
        prev = 0
        for b in (1, 2, 3, 7, 64):
            got = q(n, b, 7)
            assert got == 256 + b * rows_pad * 64 * 3 * 4, (n, b)   # header + three f32 row buffers per episode
            assert got > prev
            prev = got
        assert q(n, 2, 13) == q(n, 2, 7)
    limit = (2 ** 31 - 1) // 64
    assert q(8192, limit // 8192, 7) > 0
    assert q(8192, limit // 8192 + 1, 7) == 0      # batch * rows beyond the 32-bit row index


def _layout_bytes(n, T, B, field_bytes=4):
    """EnvLayout of csrc/eco_common.h restated: 256-byte aligned sections."""
    up = lambda x: (x + 255) // 256 * 256
    words = (n + 63) // 64
    cap = 16
    while cap < 2 * (T + 1):
        cap <<= 1
    o = up(256 + 8 * (T + 1))
    o = up(o + 128 * B)               # EpScal: 10 doubles, the hash, 10 int32
    o = up(o + B * n)                 # spins
    o = up(o + B * n * field_bytes)   # local field
    o = up(o + B * n * 2)             # time since flip
    o = up(o + B * n)                 # best spins
    o = up(o + B * cap * 4)
    o = up(o + B * cap * 8)
    o = up(o + B * (T + 1) * words * 8)
    return o


def test_env_state_bytes():
    """Up to ECO_MAX_SPINS the values of the previous version, recorded there for three (N, B, T); above it the same
    formula, monotone in the batch, and 0 with a message for what the range rejects."""
    from eco_hip import _lib
    sb = _lib.lib.eco_env_state_bytes
    for (n, B, T), want in (((20, 4, 40), 10240), ((200, 8192, 400), 219942400), ((2048, 3, 4096), 3819264)):
        assert sb(ctypes.byref(_cfg(n, T)), B) == want == _layout_bytes(n, T, B), (n, B, T)
    for n, T in ((2049, 64), (4100, 64), (8192, 16384)):
        prev = 0
        for B in (1, 2, 3, 16):
            got = sb(ctypes.byref(_cfg(n, T)), B)
            assert got == _layout_bytes(n, T, B) and got > prev, (n, T, B)
            prev = got
    # the memory note of INTEGRATION.md: the visited set of one episode at N = 8192, T = 2 N
    assert (16384 + 1) * 128 * 8 == 16778240
    cfg = _cfg(2048, 8)
    cfg.n_spins = 8193
    assert sb(ctypes.byref(cfg), 1) == 0 and "[1, 8192]" in _lib.last_error()
    cfg.n_spins = 2049
    cfg.float_weights = 1
    assert sb(ctypes.byref(cfg), 1) == 0 and "2048 < N <= 8192 takes integer weights only" in _lib.last_error()
    cfg.float_weights = 0
    cfg.optimisation_target = _lib.ECO_TARGET_MIN_COVER
    assert sb(ctypes.byref(cfg), 1) == 0 and "2048 < N <= 8192 runs OptimisationTarget.CUT only" in _lib.last_error()
    cfg.n_spins = 2048
    assert sb(ctypes.byref(cfg), 1) > 0    # the generic scorers keep their range


def test_python_surface_names_the_limits():
    import pytest
    from eco_hip.envs.utils import OptimisationTarget
    with pytest.raises(ValueError, match="exceeds ECO_MAX_SPINS_WG=8192"):
        _cfg(8193, 8)
    with pytest.raises(ValueError, match="integer weights only"):
        _cfg(2049, 8, float_weights=True)
    with pytest.raises(ValueError, match="OptimisationTarget.CUT only"):
        _cfg(2049, 8, optimisation_target=OptimisationTarget.MIN_COVER)
    assert _cfg(8192, 8).n_spins == 8192
    assert _cfg(2048, 8, optimisation_target=OptimisationTarget.MIN_COVER).n_spins == 2048
