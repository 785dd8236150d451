"""Random-regular and ring-lattice graphs on the host: random_csr("REG" / "WS"), the exact edge_cap of both, and the
generator classes RandomRegularGraphGenerator, RandomWattsStrogatzGraphGenerator and PerturbedGraphGenerator
(the reference's src/envs/utils.py:238-314, :385-436)."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(csr, g, n):
    """[n, n] weight matrix of graph g of an integer-weighted CSR, checking that rows are sorted without duplicates."""
    rp, base, edges = csr[0][g], int(csr[1][g]), csr[2]
    J = np.zeros((n, n))
    for i in range(n):
        e = edges[base + rp[i]:base + rp[i + 1]]
        cols = (e & 0xFFFFFF).astype(np.int64)
        assert np.all(np.diff(cols) > 0)
        J[i, cols] = (e >> 24).astype(np.uint8).view(np.int8)
    return J


def _ring(n, k):
    """The circular-distance definition: i ~ j iff 1 <= min(|i - j|, n - |i - j|) <= k // 2."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    dist = np.minimum(np.abs(i - j), n - np.abs(i - j))
    return ((dist >= 1) & (dist <= k // 2)).astype(float)


@pytest.mark.parametrize("n,d", [(20, 3), (9, 4), (64, 4)])
def test_regular_structure(n, d):
    from eco_hip.graphs import random_csr, edge_cap
    G = 16
    csr = random_csr("REG", G, n, d, seed=5)
    assert edge_cap("REG", n, d) == n * d
    assert np.array_equal(csr[0][:, -1], np.full(G, n * d)) and csr[2].size == G * n * d
    mats = [_dense(csr, g, n) for g in range(G)]
    for J in mats:
        assert np.array_equal(J, J.T) and not np.diag(J).any()
        assert np.all((J != 0).sum(1) == d) and set(np.unique(J)) <= {-1.0, 0.0, 1.0}
    assert any(not np.array_equal(mats[0] != 0, J != 0) for J in mats[1:])
    again = random_csr("REG", G, n, d, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(csr, again))


def test_regular_degree_zero_and_bad_arguments():
    from eco_hip.graphs import random_csr, edge_cap
    csr = random_csr("REG", 3, 7, 0, seed=1)
    assert not csr[0].any() and csr[2].size == 0 and edge_cap("REG", 7, 0) == 0
    for n, d in [(9, 3), (8, 8), (8, 9), (8, -1), (8, 2.5)]:   # odd n d, d >= n, negative, not an integer
        with pytest.raises(ValueError):
            random_csr("REG", 1, n, d, seed=1)
        with pytest.raises(ValueError):
            edge_cap("REG", n, d)


def test_regular_pair_marginals():
    """The pairing algorithm treats all labels alike, so every pair is an edge with probability exactly d / (n - 1):
    at (8, 3) each of the 28 pair frequencies over 4096 graphs is within 5 standard errors of 3 / 7."""
    from eco_hip.graphs import random_csr
    n, d, G = 8, 3, 4096
    csr = random_csr("REG", G, n, d, seed=11, weights="uniform")
    cols = (csr[2] & 0xFFFFFF).astype(np.int64).reshape(G, n, d)      # every row has exactly d entries
    freq = np.zeros((n, n))
    np.add.at(freq, (np.repeat(np.arange(n), d)[None].repeat(G, 0).ravel(), cols.ravel()), 1.0)
    freq /= G
    p = d / (n - 1)
    se = np.sqrt(p * (1 - p) / G)
    iu = np.triu_indices(n, 1)
    print("pair frequencies - 3/7, in standard errors:", np.round((freq[iu] - p) / se, 2))
    assert np.array_equal(freq, freq.T) and np.all(np.abs(freq[iu] - p) < 5 * se)


def test_regular_restart_cap_raises():
    """(12, 10) restarts often (the complement is a perfect-matching-like 1-regular graph): with no restart allowed
    some seed among a few fails; with the default 256 all of them succeed."""
    from eco_hip.graphs import random_csr
    failed = []
    for seed in range(32):
        try:
            random_csr("REG", 1, 12, 10, seed=seed, max_restarts=0)
        except ValueError:
            failed.append(seed)
    assert failed
    csr = random_csr("REG", 1, 12, 10, seed=failed[0])
    assert np.all(np.diff(csr[0][0]) == 10)


@pytest.mark.parametrize("n,k", [(9, 4), (7, 3), (8, 8), (10, 0)])
def test_ring_lattice_is_the_circular_distance_definition(n, k):
    from eco_hip.graphs import random_csr, edge_cap
    csr = random_csr("WS", 3, n, k, seed=2, weights="uniform")
    ref = _ring(n, k)
    for g in range(3):
        np.testing.assert_array_equal(_dense(csr, g, n), ref)
    assert edge_cap("WS", n, k) == int(ref.sum()) == int(csr[0][0, -1])
    with pytest.raises(ValueError):
        random_csr("WS", 1, n, n + 1, seed=2)
    with pytest.raises(ValueError):
        edge_cap("WS", n, n + 1)


@pytest.mark.parametrize("n,k", [(8, 7), (8, 6), (6, 6), (5, 5), (2, 2), (12, 1)])
def test_ring_lattice_edge_cap_near_the_antipode(n, k):
    """k // 2 = n / 2 (n even) reaches the antipode from both sides: one neighbour, not two."""
    from eco_hip.graphs import random_csr, edge_cap
    csr = random_csr("WS", 1, n, k, seed=0)
    assert edge_cap("WS", n, k) == int(_ring(n, k).sum()) == int(csr[0][0, -1])


@pytest.mark.parametrize("cls,arg", [("RandomRegularGraphGenerator", 3), ("RandomWattsStrogatzGraphGenerator", 4)])
def test_generator_classes_shapes_and_weights(cls, arg):
    from eco_hip.envs import utils
    from eco_hip.envs.utils import EdgeType
    n = 20
    for edge_type in (EdgeType.UNIFORM, EdgeType.DISCRETE, EdgeType.RANDOM):
        np.random.seed(3)
        gen = getattr(utils, cls)(n, arg, edge_type)      # a scalar parameter means [value, 0]
        assert gen.n_spins == n and gen.edge_type == edge_type and not gen.biased
        J = gen.get()
        assert J.shape == (n, n) and J.dtype == np.float64
        assert np.array_equal(J, J.T) and not np.diag(J).any()
        deg = (J != 0).sum(1)
        assert np.all(deg == (arg if cls == "RandomRegularGraphGenerator" else 2 * (arg // 2)))
        w = J[J != 0]
        if edge_type == EdgeType.UNIFORM:
            assert set(w) == {1.0}
        elif edge_type == EdgeType.DISCRETE:
            assert set(w) == {-1.0, 1.0}
        else:
            assert np.all(np.abs(w) < 1) and np.unique(np.abs(w)).size == w.size // 2
    with pytest.raises(NotImplementedError):
        getattr(utils, cls)(n, arg, EdgeType.DISCRETE, biased=True)
    with pytest.raises(AssertionError):
        getattr(utils, cls)(n, [1, 2, 3])


def test_ring_generator_matches_definition_and_regular_generator_rejects_odd():
    from eco_hip.envs.utils import RandomRegularGraphGenerator, RandomWattsStrogatzGraphGenerator, EdgeType
    np.testing.assert_array_equal(RandomWattsStrogatzGraphGenerator(9, [5, 0], EdgeType.UNIFORM).get(), _ring(9, 5))
    np.testing.assert_array_equal(RandomWattsStrogatzGraphGenerator(8, [30, 0], EdgeType.UNIFORM).get(),
                                  _ring(8, 8))                                       # k is clipped to n
    with pytest.raises(ValueError):
        RandomRegularGraphGenerator(9, [3, 0]).get()                                 # n d odd, as networkx raises


def test_degree_spread_varies_between_calls():
    from eco_hip.envs.utils import RandomRegularGraphGenerator, RandomWattsStrogatzGraphGenerator, EdgeType
    np.random.seed(7)
    gen = RandomRegularGraphGenerator(20, [6, 2], EdgeType.UNIFORM)
    degs = []
    for _ in range(12):
        deg = (gen.get() != 0).sum(1)
        assert np.all(deg == deg[0])
        degs.append(int(deg[0]))
    assert len(set(degs)) > 1
    np.random.seed(7)
    assert degs == [int((gen.get() != 0).sum(1)[0]) for _ in range(12)]
    np.random.seed(7)
    ring = RandomWattsStrogatzGraphGenerator(20, [8, 3], EdgeType.UNIFORM)
    assert len({int((ring.get() != 0).sum()) for _ in range(12)}) > 1


def test_perturbed_graph_generator():
    from eco_hip.envs.utils import PerturbedGraphGenerator, EdgeType
    rng = np.random.default_rng(4)
    mats = []
    for _ in range(3):
        J = np.triu((rng.random((10, 10)) < 0.4) * rng.choice([-1.0, 1.0], size=(10, 10)), 1)
        mats.append(J + J.T)
    gen = PerturbedGraphGenerator(mats, perturb_mean=0.0, perturb_std=0.05, ordered=True)
    assert gen.edge_type == EdgeType.RANDOM and gen.n_spins == 10 and not gen.biased
    np.random.seed(1)
    for i in range(7):                                    # ordered: cycles through the graphs
        base = mats[i % 3]
        P = gen.get()
        noise = P - base
        assert P.shape == (10, 10) and np.array_equal(P, P.T) and not np.diag(P).any()
        assert not noise[base == 0].any() and np.all(noise[base != 0] != 0)
        assert np.abs(noise).max() < 0.05 * 6
    shifted = PerturbedGraphGenerator(mats[:1], perturb_mean=0.5, perturb_std=0.0).get()
    np.testing.assert_array_equal(shifted, mats[0] + 0.5 * (mats[0] != 0))
    with pytest.raises(NotImplementedError):
        PerturbedGraphGenerator(mats, biases=[np.zeros(11)] * 3)
    with pytest.raises(NotImplementedError):
        PerturbedGraphGenerator([np.zeros((4, 4)), np.zeros((5, 5))])


def test_header_enum_values_match_lib_constants():
    from eco_hip import _lib
    text = open(os.path.join(REPO, "include", "eco_hip.h")).read()
    for name in ("ECO_GRAPH_ER", "ECO_GRAPH_BA", "ECO_GRAPH_REGULAR", "ECO_GRAPH_WS", "ECO_REGULAR_MAX_RESTARTS"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert (_lib.ECO_GRAPH_REGULAR, _lib.ECO_GRAPH_WS) == (3, 4)
