"""eco_mpnn_grad_large (training above 512 vertices) without a GPU: the two symbols are declared in
include/eco_hip.h, exported by the library and bound by eco_hip._lib, and the workspace query is positive and
non-decreasing over 512 < N <= 2048 and zero outside (host arithmetic only)."""
import os
import re

from conftest import REPO

NAMES = ("eco_mpnn_grad_large", "eco_mpnn_grad_large_workspace_bytes")


def test_symbols_declared_exported_and_bound():
    from eco_hip import _lib
    src = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(_lib.lib, name), name
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert len(_lib.lib.eco_mpnn_grad_large.argtypes) == 10
    from eco_hip.networks.mpnn import MPNN
    assert callable(MPNN.grad_large)


def test_workspace_bytes_range_and_monotonic():
    from eco_hip import _lib
    q = _lib.lib.eco_mpnn_grad_large_workspace_bytes
    for n in (-1, 0, 1, 200, 511, 512, 2049, 4096):
        for b in (1, 4, 64):
            assert q(n, b) == 0, (n, b)
    for n in (513, 2048):
        for b in (0, -3):
            assert q(n, b) == 0, (n, b)
    assert q(2048, (2 ** 31 - 1) // 64 // 2048 + 1) == 0      # batch * n_spins beyond the 32-bit row index
    sizes = (513, 514, 528, 529, 600, 800, 1024, 2000, 2047, 2048)
    batches = (1, 2, 3, 8, 64, 65)
    for b in batches:
        prev = 0
        for n in sizes:
            v = q(n, b)
            assert v > 0 and v >= prev, (n, b, v, prev)
            prev = v
    for n in sizes:
        prev = 0
        for b in batches:
            v = q(n, b)
            assert v >= prev, (n, b, v, prev)
            prev = v
    # at least the 12 saved and 11 gradient node tensors, the gather rows and the three forward row buffers
    n, b = 2000, 64
    assert q(n, b) >= (23 * n * b + 4 * b * n) * 64 * 4
