"""What the global-row entries reject, on real device buffers: eco_mpnn_grad_large (512 < N <= 2048),
eco_mpnn_grad_wg and eco_mpnn_forward_wg (2048 < N <= 8192).

One path graph at the first size of the entry's range (N = 513 or 2049), batch 2.  Every rejected call returns
ECO_ERR_ARG with the name of the entry that was called and its range in last_error(), and launches nothing: the
sentinel-filled output and the zeroed workspace are untouched afterwards.  One valid call follows; it returns ECO_OK
and leaves the error word clean.

NEWLY REJECTED marks the rows that eco_mpnn_grad_large accepted (and launched on) before the three entries came to
share one check: a graph set with a NULL row_ptr, edge_base, edges, deg or max_deg.  Every GraphStore constructor
fills all five, so no caller of the package is affected.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
SENTINEL = 123.0
ENTRIES = {"eco_mpnn_grad_large": (513, 512, 2048), "eco_mpnn_grad_wg": (2049, 2048, 8192),
           "eco_mpnn_forward_wg": (2049, 2048, 8192)}
GRAPH_SET_POINTERS = ("row_ptr", "edge_base", "edges", "deg", "max_deg")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_rejections_name_the_entry_and_launch_nothing(entry):
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    lib = _lib.lib
    n, lo, hi = ENTRIES[entry]
    grad_entry = "grad" in entry
    store = GraphStore.from_edges(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1, np.int64))
    net = MPNN(device="cuda")
    net.init_normal_(0.1, generator=torch.Generator().manual_seed(1))
    net.repack()
    x = torch.zeros(B, n, 8, device="cuda")
    dq = torch.zeros(B, n, device="cuda")
    gids = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.full_like(net.flat, SENTINEL) if grad_entry else torch.full((B, n), SENTINEL, device="cuda")
    nbytes = (getattr(lib, entry + "_workspace_bytes")(n, B) if grad_entry
              else lib.eco_mpnn_forward_wg_workspace_bytes(n, B, 7))
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    good = dict(packed=net.packed, n_obs=7, gs=store.gs, gids=gids, batch=B, x=x, dq=dq, out=out, ws=ws)

    def call(**change):
        a = dict(good, **change)
        gs = ctypes.byref(a["gs"]) if a["gs"] is not None else None
        if grad_entry:
            return getattr(lib, entry)(_lib.ptr(a["packed"]), a["n_obs"], gs, _lib.ptr(a["gids"]), a["batch"],
                                       _lib.ptr(a["x"]), _lib.ptr(a["dq"]), _lib.ptr(a["out"]), _lib.ptr(a["ws"]),
                                       _lib.stream_ptr())
        return lib.eco_mpnn_forward_wg(_lib.ptr(a["packed"]), a["n_obs"], gs, _lib.ptr(a["gids"]), a["batch"],
                                       _lib.ptr(a["x"]), _lib.ECO_NORM_PER_CALL, _lib.ptr(a["out"]), None, None,
                                       _lib.ptr(a["ws"]), _lib.stream_ptr())

    def graph_set(**fields):
        gs = _lib.GraphSet.from_buffer_copy(store.gs)
        for k, v in fields.items():
            setattr(gs, k, v)
        return gs

    def rejected(what, also=None, **change):
        rc, msg = call(**change), _lib.last_error()
        assert rc == _lib.ECO_ERR_ARG, (entry, what, rc)
        assert entry + " takes" in msg and f"{lo} < N <= {hi}" in msg, (entry, what, msg)
        assert also is None or also in msg, (entry, what, msg)

    for name in ("packed", "gs", "gids", "x", "ws") + (("dq", "out") if grad_entry else ()):
        rejected("NULL " + name, **{name: None})
    if not grad_entry:                                   # q is optional, but a call must compute something
        assert call(out=None) == _lib.ECO_ERR_ARG
    rejected("batch 0", batch=0)
    for n_bad in (lo, hi + 1):
        rejected(f"N = {n_bad}", gs=graph_set(n_spins=n_bad))
    for n_obs in (0, 17):
        rejected(f"n_obs_in = {n_obs}", also="n_obs_in out of range [1, 16]", n_obs=n_obs)
    if hi == 8192:                                       # no store holds float weights above 2048: the fields alone
        weights = torch.ones(2 * (n - 1), dtype=torch.float64, device="cuda")
        rejected("float weights", also="integer weights only",
                 gs=graph_set(edge_weights=weights.data_ptr(), unit_weights=0))
    rows = n if grad_entry else (n + 15) // 16 * 16      # the gradient indexes batch * N rows, the forward batch * rows_pad
    rejected("row index", also="32-bit row index", batch=(2 ** 31 - 1) // 64 // rows + 1)
    for name in GRAPH_SET_POINTERS:                      # NEWLY REJECTED by eco_mpnn_grad_large
        rejected("graph set without " + name, gs=graph_set(**{name: None}))
    rejected("empty graph set", gs=graph_set(n_graphs=0))   # NEWLY REJECTED by eco_mpnn_grad_large
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and not bool(ws.any()), entry

    assert call() == _lib.ECO_OK
    torch.cuda.synchronize()
    store.check_errors()
    if grad_entry:
        assert bool((out == 0).all())                    # dq = 0: a zero gradient, every entry overwritten
    else:
        assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())
