"""Host-side CSR construction for float-weighted graphs (EdgeType.RANDOM): float input round-trips to the dense
matrix, integer input takes exactly the integer path (packed words unchanged, no weights array), and the packed
byte of a float-weighted set holds sign(w)."""
import numpy as np
import pytest


def _dense(n, row_ptr, edges, weights, g=0, base=0):
    m = np.zeros((n, n))
    rp = row_ptr[g]
    e = edges[base:base + rp[-1]]
    rows = np.repeat(np.arange(n), np.diff(rp))
    m[rows, e & 0xFFFFFF] = weights[base:base + rp[-1]] if weights is not None \
        else ((e >> 24).astype(np.uint8)).view(np.int8)
    return m


def _sym(n, p, rng, draw):
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    m = np.zeros((n, n))
    m[iu[keep], ju[keep]] = draw(int(keep.sum()))
    return m + m.T


def test_dense_to_csr_float_roundtrip_and_sign_byte():
    from eco_hip.graphs import dense_to_csr
    rng = np.random.default_rng(0)
    mats = [_sym(17, 0.4, rng, lambda k: rng.uniform(-1, 1, k)) for _ in range(3)]
    csr = dense_to_csr(mats)
    rp, eb, ed = csr[0], csr[1], csr[2]
    with pytest.raises(TypeError, match="from_csr"):      # unpacking would drop the weights
        _ = tuple(csr)
    with pytest.raises(TypeError, match="from_csr"):
        _a, _b, _c = csr
    assert csr.weights is not None and csr.weights.dtype == np.float64 and csr.weights.size == ed.size
    for g, m in enumerate(mats):
        np.testing.assert_array_equal(_dense(17, rp, ed, csr.weights, g, int(eb[g])), m)
    sign = ((ed >> 24).astype(np.uint8)).view(np.int8)
    np.testing.assert_array_equal(sign, np.sign(csr.weights).astype(np.int8))
    assert set(np.unique(sign)) <= {-1, 1}


def test_edges_to_csr_float_roundtrip():
    from eco_hip.graphs import edges_to_csr
    rng = np.random.default_rng(1)
    n = 23
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < 0.3
    i, j = iu[keep], ju[keep]
    w = rng.normal(size=i.size)
    w[0] = 0.0                       # zero weights are dropped
    csr = edges_to_csr(n, i, j, w)
    m = np.zeros((n, n))
    m[i, j] = w
    m[j, i] = w
    assert csr.weights is not None and np.all(csr.weights != 0)
    np.testing.assert_array_equal(_dense(n, csr[0], csr[2], csr.weights), m)


def test_random_csr_float_roundtrip_symmetric():
    from eco_hip.graphs import random_csr
    csr = random_csr("ER", 4, 30, 0.3, seed=5, weights="random")
    rp, eb, ed = csr[0], csr[1], csr[2]
    assert csr.weights is not None
    for g in range(4):
        m = _dense(30, rp, ed, csr.weights, g, int(eb[g]))
        np.testing.assert_array_equal(m, m.T)
        assert not np.diag(m).any()
        nz = m[m != 0]
        assert nz.size and np.all(np.abs(nz) < 1)
    ba = random_csr("BA", 2, 30, 4, seed=5, weights="random")
    assert ba.weights is not None and ba.weights.size == ba[2].size


def test_integer_input_takes_the_integer_path_unchanged():
    """Packed words as the integer-only code produced them: column | (uint8 weight << 24); no weights array."""
    from eco_hip.graphs import dense_to_csr, edges_to_csr, random_csr
    rng = np.random.default_rng(2)
    m = _sym(19, 0.4, rng, lambda k: rng.integers(-128, 128, k).astype(np.float64))
    csr = dense_to_csr([m])
    assert csr.weights is None and len(csr) == 3
    r, c = np.nonzero(m)
    expect = (c.astype(np.uint32) | ((m[r, c].astype(np.int64) & 0xFF).astype(np.uint32) << 24)).astype(np.uint32)
    np.testing.assert_array_equal(csr[2], expect)
    assert csr[2].dtype == np.uint32
    np.testing.assert_array_equal(csr[0][0, 1:], np.cumsum(np.bincount(r, minlength=19)))
    i, j = np.nonzero(np.triu(m))
    e = edges_to_csr(19, i, j, m[i, j].astype(np.int64))
    assert e.weights is None
    np.testing.assert_array_equal(e[2], expect)
    for kind in ("discrete", "uniform"):
        assert random_csr("ER", 2, 20, 0.3, seed=1, weights=kind).weights is None


@pytest.mark.parametrize("w", [200.0, 0.5, -129.0])
def test_out_of_range_and_fractional_weights_select_the_float_path(w):
    from eco_hip.graphs import dense_to_csr
    m = np.zeros((5, 5))
    m[0, 1] = m[1, 0] = w
    m[2, 3] = m[3, 2] = -1.0
    csr = dense_to_csr([m])
    assert csr.weights is not None
    np.testing.assert_array_equal(csr.weights, [w, w, -1.0, -1.0])
    sign = ((csr[2] >> 24).astype(np.uint8)).view(np.int8)
    np.testing.assert_array_equal(sign, np.sign([w, w, -1, -1]).astype(np.int8))


def test_abi_structs_have_the_trailing_fields_and_integer_layout_is_unchanged():
    """edge_weights / float_weights are trailing fields (positional construction keeps working) and a config with
    float_weights = 0 sizes the state exactly as before; the f64 field adds 4 B per vertex (rounded to 256)."""
    import ctypes
    from eco_hip import _lib
    from eco_hip.envs.batched import make_config
    from eco_hip.envs.utils import ExtraAction, OptimisationTarget
    assert _lib.GraphSet._fields_[-1][0] == "edge_weights"
    assert _lib.EnvConfig._fields_[-1][0] == "float_weights"
    gs = _lib.GraphSet(1, 2, None, None, None, None, None, None, None, 1, None)   # the 11 original fields
    assert gs.edge_weights is None
    kw = dict(extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT)
    n, T, B = 200, 400, 64
    c0 = make_config(n, T, **kw)
    c1 = make_config(n, T, float_weights=True, **kw)
    assert c0.float_weights == 0 and c1.float_weights == 1
    b0 = _lib.lib.eco_env_state_bytes(ctypes.byref(c0), B)
    b1 = _lib.lib.eco_env_state_bytes(ctypes.byref(c1), B)
    assert b1 - b0 == B * n * 4          # 51,200: a multiple of the 256 B section alignment
    # integer layout, section by section (eco_common.h env_layout): unchanged
    al = lambda x: (x + 255) // 256 * 256
    cap = 16
    while cap < 2 * (T + 1):
        cap <<= 1
    words = (n + 63) // 64
    o = al(256 + 8 * (T + 1))
    o = al(o + 128 * B)             # sizeof(EpScal)
    for per in (n, 4 * n, 2 * n, n, cap * 4, cap * 8, (T + 1) * words * 8):
        o = al(o + B * per)
    assert b0 == o
    # float weights with a generic-scorer target: rejected (the query returns 0), in Python with a message
    with pytest.raises(ValueError, match="CUT only"):
        make_config(n, T, float_weights=True, extra_action=ExtraAction.NONE,
                    optimisation_target=OptimisationTarget.MIN_COVER)
    c1.optimisation_target = OptimisationTarget.MIN_COVER.value
    assert _lib.lib.eco_env_state_bytes(ctypes.byref(c1), B) == 0
    assert "CUT only" in _lib.last_error()


def test_read_mc_real_weights(tmp_path):
    from eco_hip.experiments import read_mc
    from eco_hip.graphs import edges_to_csr
    p = tmp_path / "w.mc"
    p.write_text("4 3\n1 2 0.25\n2 3 -1.5\n3 4 2\n")
    n, m, i, j, w = read_mc(str(p))
    assert (n, m) == (4, 3) and w.dtype == np.float64
    np.testing.assert_array_equal(w, [0.25, -1.5, 2.0])
    assert edges_to_csr(n, i, j, w).weights is not None
    p.write_text("4 2\n1 2 1\n2 3 -1\n")
    assert read_mc(str(p))[4].dtype == np.int64
