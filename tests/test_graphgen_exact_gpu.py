"""eco_graphs_generate against oracle/graphgen_oracle.py, byte for byte: row_ptr, the edge words, the float64
weights, and the fields eco_graphs_prepare derives (deg, max_deg, valid, meta), for ER, BA, REG and WS at the shapes
of tests/graphgen_cases.py; every slot outside the generated range, and the unused tail of every generated slot,
keeps a sentinel pattern.  Then the slot-overflow paths: ER total above the slot size, ER row degree above it (the
fill kernel must write nothing for a graph the scan kernel marked), BA.  No tolerances."""
import numpy as np
import pytest
import torch

import graphgen_cases as gc
from oracle import graphgen_oracle as go

pytestmark = pytest.mark.gpu

EDGE_SENTINEL = 0x5A5A5A5A
WEIGHT_SENTINEL = -7.25
ROW_SENTINEL = -3


def _sentinel_store(G, n, cap, weights):
    """Slot store with the sentinel in every edge word, weight and row pointer."""
    from eco_hip.graphs import GraphStore
    st = GraphStore.slots(G, n, cap, weights=weights)
    st.edges.fill_(EDGE_SENTINEL)
    st.row_ptr.fill_(ROW_SENTINEL)
    if st.float_weights:
        st.edge_weights.fill_(WEIGHT_SENTINEL)
    return st


def _host(st):
    ew = st.edge_weights.cpu().numpy().view(np.int64) if st.float_weights else None
    return dict(rp=st.row_ptr.cpu().numpy(), ed=st.edges.cpu().numpy().view(np.uint32), ew=ew,
                deg=st.deg.cpu().numpy(), max_deg=st.max_deg.cpu().numpy(), valid=st.valid.cpu().numpy(),
                meta=st.meta.cpu().numpy().view(np.int64))


def _assert_slots(h, n, cap, G, graphs):
    """graphs {slot: oracle Graph}: those slots equal the oracle bit for bit and keep the sentinel behind their
    row_ptr[n] entries; every other slot is sentinel throughout."""
    wsent = np.array([WEIGHT_SENTINEL]).view(np.int64)[0]
    for g in range(G):
        ed = h["ed"][g * cap:(g + 1) * cap]
        ew = h["ew"][g * cap:(g + 1) * cap] if h["ew"] is not None else None
        if g not in graphs:
            assert np.all(h["rp"][g] == ROW_SENTINEL), g
            assert np.all(ed == EDGE_SENTINEL), g
            assert ew is None or np.all(ew == wsent), g
            continue
        o = graphs[g]
        k = int(o.row_ptr[-1])
        assert k <= cap
        assert np.array_equal(h["rp"][g], o.row_ptr), g
        assert np.array_equal(ed[:k], o.edges), g
        assert np.all(ed[k:] == EDGE_SENTINEL), g
        if ew is not None:
            assert np.array_equal(ew[:k], o.weights.view(np.int64)), g
            assert np.all(ew[k:] == wsent), g
        assert np.array_equal(h["deg"][g], o.deg), g
        assert h["max_deg"][g] == o.max_deg and h["valid"][g] == o.valid, g
        assert np.array_equal(h["meta"][g], o.meta.view(np.int64)), (g, h["meta"][g].view(np.float64), o.meta)


def _run(name, cap=None):
    from eco_hip.graphs import edge_cap
    c = gc.CASES[name]
    cap = edge_cap(c.kind, c.n, c.param) if cap is None else cap
    st = _sentinel_store(c.G, c.n, cap, c.weights)
    st.generate(c.first, c.count, c.kind, c.param, c.seed, c.weights)
    st.check_errors()
    return st, cap


@pytest.mark.parametrize("name", list(gc.CASES))
def test_generated_slots_equal_the_oracle(name):
    c = gc.CASES[name]
    st, cap = _run(name)
    _assert_slots(_host(st), c.n, cap, c.G, gc.oracle_graphs(name))
    st.check_errors()


def test_er_empty_and_complete():
    """p = 0: empty graphs, valid = 0, and no error (an empty graph is not an overflow); p = 1: all n (n - 1)."""
    st, _ = _run("er65_p0")
    assert not st.row_ptr.any().item() and not st.valid.any().item()
    st.check_errors()
    st, _ = _run("er65_p1")
    assert np.all(st.row_ptr.cpu().numpy()[:, -1] == 65 * 64) and np.all(st.deg.cpu().numpy() == 64)
    st.check_errors()


@pytest.mark.parametrize("group", gc.WEIGHT_KIND_GROUPS)
def test_structure_identical_across_weight_kinds(group):
    base, _ = _run(group[0])
    n_edges = gc.CASES[group[0]].G * base.cap
    for other in group[1:]:
        st, cap = _run(other)
        assert cap == base.cap and torch.equal(st.row_ptr, base.row_ptr)
        assert torch.equal(st.edges[:n_edges] & 0xFFFFFF, base.edges[:n_edges] & 0xFFFFFF)
        assert torch.equal(st.deg, base.deg)


def _clear_error_word(st):
    try:
        st.check_errors()
    except ValueError:
        pass


def test_er_total_above_the_slot_size():
    """Eight ER(65, 0.5) graphs into slots of the median of their totals: the oracle says which overflow.  Those come
    back empty and untouched, the others equal the oracle; the error is reported once per call."""
    n, p, G, seed = 65, 0.5, 8, 13
    free = [go.generate("ER", n, p, seed, g) for g in range(G)]
    totals = [int(o.row_ptr[-1]) for o in free]
    cap = int(np.median(totals))
    graphs = {g: go.generate("ER", n, p, seed, g, cap=cap) for g in range(G)}
    over = [g for g in range(G) if graphs[g].overflow]
    print("totals", totals, "cap", cap, "overflowing slots", over)
    assert 0 < len(over) < G and over == [g for g in range(G) if totals[g] > cap]
    st = _sentinel_store(G, n, cap, "discrete")
    try:
        with pytest.raises(ValueError):
            st.generate(0, G, "ER", p, seed, check=True)
        st.check_errors()                                   # raised once, then cleared
        h = _host(st)
        _assert_slots(h, n, cap, G, graphs)                 # overflowing: zero row_ptr row, valid 0, sentinel edges
        for g in over:
            assert not h["rp"][g].any() and h["valid"][g] == 0
        st2 = _sentinel_store(G, n, cap, "discrete")
        st2.generate(0, G, "ER", p, seed, check=False)      # no synchronisation, no exception
        with pytest.raises(ValueError):
            st2.check_errors()
        st2.check_errors()
        _assert_slots(_host(st2), n, cap, G, graphs)
    finally:
        _clear_error_word(st)


@pytest.mark.parametrize("weights", ["discrete", "random"])
def test_er_row_degree_above_the_slot_size(weights):
    """ER(65, 1.0) into slot 1 of four 40-entry slots: every row has 64 entries, more than a slot.  The scan kernel
    marks the graph (zero row_ptr row); the fill kernel must then write nothing: not into its own slot, and not
    into slots 2 and 3 behind it, which belong to graphs the call does not regenerate.  (A fill that went on would
    write entries 40 .. 103 of a 160-entry allocation: inside the buffer, outside the slot.)"""
    n, G, cap, seed = 65, 4, 40, 3
    st = _sentinel_store(G, n, cap, weights)
    try:
        with pytest.raises(ValueError):
            st.generate(1, 1, "ER", 1.0, seed, weights, check=True)
        st.check_errors()
        o = go.generate("ER", n, 1.0, seed, 1, weights, cap=cap)
        assert o.overflow
        _assert_slots(_host(st), n, cap, G, {1: o})
    finally:
        _clear_error_word(st)


def test_ba_total_above_the_slot_size():
    n, m, G, seed = 20, 4, 4, 7
    cap = 2 * m * (n - m) - 1
    st = _sentinel_store(G, n, cap, "discrete")
    try:
        with pytest.raises(ValueError):
            st.generate(0, G, "BA", m, seed, check=True)
        st.check_errors()
        graphs = {g: go.generate("BA", n, m, seed, g, cap=cap) for g in range(G)}
        assert all(o.overflow for o in graphs.values())
        h = _host(st)
        _assert_slots(h, n, cap, G, graphs)                 # every slot empty, every edge word still the sentinel
        assert not h["rp"].any() and not h["valid"].any()
    finally:
        _clear_error_word(st)
