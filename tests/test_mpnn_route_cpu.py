"""eco_mpnn_route (include/eco_hip.h) names the kernel family the MPNN dispatcher picks, without a GPU.

The oracle below restates the `if` chains that eco_mpnn_forward, eco_mpnn_forward_pair and mpnn_backward_launch each
carried before they shared one route function (csrc/eco_mpnn.hip with dense_eligible of eco_mpnn_dense.h and
dl_eligible of eco_mpnn_dl.h, as of the commit before the router): three separate chains, compared with the library
over the full grid of shapes, weights, path masks and call kinds.  The route is a pure function of its arguments, so
combinations graphs_per_block() would never produce (several 500-vertex graphs in a block, say) are compared too;
none is skipped."""
import ctypes
import itertools

NO_DENSE, NO_DL, NO_SHARED, NO_PAIR, DENSE2_FWD = 1, 2, 4, 8, 16
NONE, DENSE3, DENSE2, DL, SHARED, LARGE, CSR = range(7)
PAIR_FUSED = 16

NS = (3, 4, 20, 200, 208, 224, 225, 500, 512, 513, 2000)
GPBS = (1, 2, 9)
WEIGHTS = ("unit", "integer", "float")


def _dense_eligible(unit, N, gpb):
    rows_pad = (gpb * N + 15) & ~15
    return unit and rows_pad <= 224 and N >= 4


def _dl_eligible(unit, adjbits, N, gpb):
    rows_pad = (N + 15) & ~15
    return unit and adjbits and gpb == 1 and 224 < rows_pad <= 512


def _forward(N, gpb, unit, adjbits, n_graphs, xw, saved, paths):
    if xw == 8 and _dense_eligible(unit, N, gpb) and not paths & NO_DENSE:
        return DENSE2 if paths & DENSE2_FWD else DENSE3
    if xw == 8 and _dl_eligible(unit, adjbits, N, gpb) and not paths & (NO_DL | NO_DENSE):
        return DL
    if N > 512:
        if saved:
            return NONE           # "training forward (saved activations) supports N <= 512"
        if n_graphs == 1 and unit and not paths & NO_SHARED:
            return SHARED
        return LARGE
    return CSR


def _backward(N, gpb, unit, adjbits, xw, paths):
    if N > 512:
        return NONE               # "MPNN backward supports N <= 512"
    if xw == 8 and _dense_eligible(unit, N, gpb) and not paths & NO_DENSE:
        return DENSE2 if paths & DENSE2_FWD else DENSE3
    if xw == 8 and _dl_eligible(unit, adjbits, N, gpb) and not paths & (NO_DL | NO_DENSE):
        return DL
    return CSR


def _pair(N, gpb, unit, adjbits, n_graphs, xw, paths):
    if paths & (NO_PAIR | NO_DENSE) or not (xw == 8 and _dense_eligible(unit, N, gpb) and gpb == 1 and adjbits):
        return _forward(N, gpb, unit, adjbits, n_graphs, xw, False, paths)   # two single forwards
    return (DENSE2 if paths & DENSE2_FWD else DENSE3) | PAIR_FUSED


def test_route_matches_the_three_dispatch_chains_on_the_full_grid():
    from eco_hip import _lib
    assert (_lib.ECO_ROUTE_NONE, _lib.ECO_ROUTE_DENSE3, _lib.ECO_ROUTE_DENSE2, _lib.ECO_ROUTE_DL,
            _lib.ECO_ROUTE_SHARED, _lib.ECO_ROUTE_LARGE, _lib.ECO_ROUTE_CSR, _lib.ECO_ROUTE_PAIR_FUSED) == \
        (NONE, DENSE3, DENSE2, DL, SHARED, LARGE, CSR, PAIR_FUSED)
    route = _lib.lib.eco_mpnn_route
    dummy = 0x1000                # never dereferenced: the route reads pointer null-ness only
    shapes = []
    for N, gpb, wt, adjbits, n_graphs, n_obs in itertools.product(NS, GPBS, WEIGHTS, (False, True), (1, 2), (7, 13)):
        gs = _lib.GraphSet(n_graphs=n_graphs, n_spins=N, row_ptr=dummy, edge_base=dummy, edges=dummy, deg=dummy,
                           max_deg=dummy, meta=dummy, valid=dummy, unit_weights=int(wt == "unit"),
                           adjbits=dummy if adjbits else None, edge_weights=dummy if wt == "float" else None)
        shapes.append((N, gpb, wt == "unit", adjbits, n_graphs, n_obs, gs))
    total = skipped = 0
    families = set()
    for paths in range(32):
        with _lib.kernel_paths(paths):
            for N, gpb, unit, adjbits, n_graphs, n_obs, gs in shapes:
                xw = _lib.obs_x_stride(n_obs)
                for training, pair in itertools.product((0, 1), (0, 1)):
                    total += 1
                    if pair:      # eco_mpnn_forward_pair never saves: `training` does not apply
                        want = _pair(N, gpb, unit, adjbits, n_graphs, xw, paths)
                    elif training:
                        want = _forward(N, gpb, unit, adjbits, n_graphs, xw, True, paths)
                        # the backward must read `saved` with the family the forward wrote it with
                        assert want == _backward(N, gpb, unit, adjbits, xw, paths), (N, gpb, unit, adjbits, paths)
                    else:
                        want = _forward(N, gpb, unit, adjbits, n_graphs, xw, False, paths)
                    got = route(ctypes.byref(gs), n_obs, 64, gpb, training, pair)
                    assert got == want, (N, gpb, unit, adjbits, n_graphs, n_obs, training, pair, paths, got, want)
                    families.add(got)
    assert total == len(NS) * len(GPBS) * len(WEIGHTS) * 2 * 2 * 2 * 2 * 2 * 32
    assert skipped / total <= 0.25
    assert families == {NONE, DENSE3, DENSE2, DL, SHARED, LARGE, CSR, DENSE3 | PAIR_FUSED, DENSE2 | PAIR_FUSED}


def test_route_rejects_what_the_forward_rejects_and_computes_graphs_per_block():
    from eco_hip import _lib
    route = _lib.lib.eco_mpnn_route
    dummy = 0x1000

    def gs(N, unit=1, fw=False, adjbits=False):
        return _lib.GraphSet(n_graphs=4, n_spins=N, row_ptr=dummy, edge_base=dummy, edges=dummy, deg=dummy,
                             max_deg=dummy, meta=dummy, valid=dummy, unit_weights=unit,
                             adjbits=dummy if adjbits else None, edge_weights=dummy if fw else None)
    with _lib.kernel_paths(0):
        assert route(None, 7, 64, 1, 0, 0) == NONE
        assert route(ctypes.byref(gs(20)), 0, 64, 1, 0, 0) == NONE        # n_obs_in out of range [1, 16]
        assert route(ctypes.byref(gs(20)), 17, 64, 1, 0, 0) == NONE
        assert route(ctypes.byref(gs(20)), 7, 0, 1, 0, 0) == NONE         # batch must be >= 1
        assert route(ctypes.byref(gs(0)), 7, 64, 1, 0, 0) == NONE         # 1 <= N <= 2048
        assert route(ctypes.byref(gs(2049)), 7, 64, 1, 0, 0) == NONE
        assert route(ctypes.byref(gs(20, unit=1, fw=True)), 7, 64, 1, 0, 0) == NONE   # float weights and unit flag
        # graphs_per_block <= 0: the library's own choice -- one graph per block from 105 vertices up, several of 20
        assert route(ctypes.byref(gs(300, adjbits=True)), 7, 64, 0, 1, 0) == DL
        assert route(ctypes.byref(gs(200, adjbits=True)), 7, 64, -1, 0, 1) == DENSE3 | PAIR_FUSED
        assert route(ctypes.byref(gs(20, adjbits=True)), 7, 4096, 0, 0, 1) == DENSE3   # several graphs per block
