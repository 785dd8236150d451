"""Device graph store: G graphs of N vertices as CSR (eco_graph_set, include/eco_hip.h).

Replaces the dense `GraphGenerator.get() -> ndarray[N,N] f64` adjacency that the
reference stacks under every observation (spinsystem.py:561-574): on the device a
graph is CSR, shared by every episode that references its id: integer weights in [-128, 127] packed into
the edge word, or (EdgeType.RANDOM, any other weight) a parallel float64 weights array with the weight's sign
in the word.
Host-side construction is numpy (input preparation, not the hot path); the
normalisers (mlr, qn, lb, degrees) are computed on the device by
eco_graphs_prepare.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _is_float_weights(weights):
    """True when the weights need the float64 path: any non-integer value or one outside [-128, 127]
    (EdgeType.RANDOM, src/envs/utils.py:137-148,323-330)."""
    w = np.asarray(weights)
    return bool(w.size) and (not np.all(np.equal(np.mod(w, 1), 0)) or w.min() < -128 or w.max() > 127)


def _pack_edges(cols, weights, as_float=False):
    """Packed edge words column | (uint8 weight << 24).  as_float: the byte holds sign(w) (the float64 weights
    travel in a parallel array)."""
    w = np.asarray(weights)
    if as_float:
        w = np.sign(w)
    elif _is_float_weights(w):
        raise ValueError("non-integer edge weights need the float-weights path (as_float=True)")
    return (np.asarray(cols, dtype=np.uint32) | ((w.astype(np.int64) & 0xFF).astype(np.uint32) << 24)).astype(np.uint32)


class CSR(tuple):
    """(row_ptr, edge_base, edges) with the float64 weights of a float-weighted set in `.weights` (None for
    integer weights).  An integer CSR is a plain 3-tuple to every caller that unpacks it.  A float-weighted one
    refuses to be unpacked or iterated (indexing still works): `GraphStore(*csr)` or `tuple(csr)` would drop the
    weights and leave an integer graph of their signs.  Build a store with GraphStore.from_csr(csr)."""

    def __new__(cls, row_ptr, edge_base, edges, weights=None):
        t = super().__new__(cls, (row_ptr, edge_base, edges))
        t.weights = weights
        return t

    def __iter__(self):
        if self.weights is not None:
            raise TypeError("a float-weighted CSR cannot be unpacked into (row_ptr, edge_base, edges): its weights "
                            "would be lost; use GraphStore.from_csr(csr), or csr[0..2] and csr.weights")
        return super().__iter__()


def dense_to_csr(matrices):
    """list of [N,N] symmetric zero-diagonal matrices -> CSR (row_ptr [G][N+1], edge_base [G], edges); float
    weights (any non-integer or outside [-128, 127], in any matrix) also give .weights [total edges] f64."""
    mats = [np.asarray(m) for m in matrices]
    fw = any(_is_float_weights(m) for m in mats)
    wchunks = []
    n = mats[0].shape[0]
    row_ptr = np.zeros((len(mats), n + 1), dtype=np.int32)
    bases = np.zeros(len(mats), dtype=np.int64)
    chunks = []
    off = 0
    for g, m in enumerate(mats):
        if m.shape != (n, n):
            raise ValueError("all graphs in a store must have the same N")
        if np.any(np.diag(m) != 0):
            raise ValueError("adjacency must have a zero diagonal (src/envs/utils.py:198-199)")
        if not np.array_equal(m, m.T):
            raise ValueError("adjacency must be symmetric (unbiased MaxCut)")
        r, c = np.nonzero(m)
        row_ptr[g, 1:] = np.cumsum(np.bincount(r, minlength=n))
        bases[g] = off
        chunks.append(_pack_edges(c, m[r, c], fw))
        if fw:
            wchunks.append(np.asarray(m[r, c], dtype=np.float64))
        off += r.size
    edges = np.concatenate(chunks) if chunks else np.zeros(0, np.uint32)
    return CSR(row_ptr, bases, edges, np.concatenate(wchunks) if fw else None)


def edges_to_csr(n, i, j, w):
    """One graph from an undirected edge list (each edge once, 0-based) -> CSR (row_ptr [1][N+1], edge_base [1],
    edges): the CSR of the symmetric matrix load_graph builds (matrix[[i,j],[j,i]] = w), without the dense
    N x N array (GSet graphs, N = 800 .. 20,000).  A repeated pair keeps its last weight, as the reference.
    Real-valued weights (or integers outside [-128, 127]) give a float-weighted CSR (.weights)."""
    i, j = (np.asarray(v, dtype=np.int64) for v in (i, j))
    w = np.asarray(w)
    fw = _is_float_weights(w)
    w = w.astype(np.float64) if fw else w.astype(np.int64)
    if i.size and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) >= n):
        raise ValueError("edge endpoint out of range")
    if np.any(i == j):
        raise ValueError("self-loops are not allowed (zero diagonal)")
    key = np.minimum(i, j) * n + np.maximum(i, j)
    _, last = np.unique(key[::-1], return_index=True)   # last occurrence of every pair
    keep = np.sort(key.size - 1 - last)
    i, j, w = i[keep], j[keep], w[keep]
    nz = w != 0
    i, j, w = i[nz], j[nz], w[nz]
    r = np.concatenate([i, j])
    c = np.concatenate([j, i])
    ww = np.concatenate([w, w])
    order = np.lexsort((c, r))
    r, c, ww = r[order], c[order], ww[order]
    row_ptr = np.zeros((1, n + 1), dtype=np.int32)
    row_ptr[0, 1:] = np.cumsum(np.bincount(r, minlength=n))
    return CSR(row_ptr, np.zeros(1, dtype=np.int64), _pack_edges(c, ww, fw), ww if fw else None)


def random_csr(kind, n_graphs, n, param, seed, weights="discrete", chunk=512, max_restarts=None):
    """Seeded synthetic graph pool built directly as CSR (no dense N x N per graph).
    kind 'ER': G(n, p=param); 'BA': preferential attachment with m=param; 'REG': random d-regular with d=param
    (max_restarts: see _regular_edges); 'WS': ring lattice with k=param.
    weights 'discrete' = fair +-1 per edge (EdgeType.DISCRETE), 'uniform' = 1, 'random' = float64 uniform in
    (-1, 1) (EdgeType.RANDOM; a float-weighted CSR with .weights)."""
    if kind not in ("ER", "BA", "REG", "WS"):
        raise ValueError(kind)
    if kind in ("REG", "WS"):
        param = _integer_param(kind, n, param)
    if max_restarts is None:
        max_restarts = _lib.ECO_REGULAR_MAX_RESTARTS
    rng = np.random.default_rng(seed)
    fw = weights == "random"
    wparts = []
    row_ptr = np.zeros((n_graphs, n + 1), dtype=np.int32)
    bases = np.zeros(n_graphs, dtype=np.int64)
    parts = []
    off = 0
    iu_all, ju_all = np.triu_indices(n, 1)
    for g0 in range(0, n_graphs, chunk):
        g1 = min(n_graphs, g0 + chunk)
        for g in range(g0, g1):
            if kind == "ER":
                keep = rng.random(iu_all.size) < param
                iu, ju = iu_all[keep], ju_all[keep]
            elif kind == "BA":
                iu, ju = _ba_edges(n, int(param), rng)
            elif kind == "REG":
                iu, ju = _regular_edges(n, param, rng, max_restarts)
            else:
                iu, ju = _ring_edges(n, param)
            if fw:
                w = rng.uniform(-1.0, 1.0, iu.size)
                w[w == 0.0] = 2.0 ** -53   # stored weights are nonzero
            else:
                w = (2 * rng.integers(0, 2, iu.size) - 1) if weights == "discrete" else np.ones(iu.size, np.int64)
            r = np.concatenate([iu, ju])
            c = np.concatenate([ju, iu])
            ww = np.concatenate([w, w])
            order = np.lexsort((c, r))
            r, c, ww = r[order], c[order], ww[order]
            row_ptr[g, 1:] = np.cumsum(np.bincount(r, minlength=n))
            bases[g] = off
            parts.append(_pack_edges(c, ww, fw))
            if fw:
                wparts.append(ww)
            off += r.size
    return CSR(row_ptr, bases, np.concatenate(parts), np.concatenate(wparts) if fw else None)


def _ba_edges(n, m, rng):
    targets = list(range(m))
    repeated = []
    iu, ju = [], []
    for src in range(m, n):
        iu.extend(targets)
        ju.extend([src] * m)
        repeated.extend(targets)
        repeated.extend([src] * m)
        chosen = set()
        while len(chosen) < m:
            chosen.add(repeated[int(rng.integers(0, len(repeated)))])
        targets = sorted(chosen)
    return np.array(iu, dtype=np.int64), np.array(ju, dtype=np.int64)


def _integer_param(kind, n, param):
    """The degree d of 'REG' (0 <= d < n, n d even) or the k of 'WS' (0 <= k <= n) as an int; ValueError otherwise
    (the checks eco_graphs_generate makes before a launch)."""
    p = int(param)
    if p != param:
        raise ValueError(f"{kind} needs an integer parameter, got {param!r}")
    if kind == "REG":
        if not 0 <= p < n:
            raise ValueError(f"regular-graph degree d={p} must be in [0, n={n})")
        if (n * p) % 2:
            raise ValueError(f"no {p}-regular graph on {n} vertices: n d must be even")
    elif not 0 <= p <= n:
        raise ValueError(f"ring-lattice k={p} must be in [0, n={n}]")
    return p


REGULAR_MAX_STALLS = 64   # kRegularMaxStalls of csrc/eco_graphgen.hip


def _regular_edges(n, d, rng, max_restarts=_lib.ECO_REGULAR_MAX_RESTARTS):
    """Edges (iu < ju) of a random simple d-regular graph: the pairing algorithm of networkx.random_regular_graph
    (Steger and Wormald) restated, the algorithm of regular_kernel (csrc/eco_graphgen.hip) on numpy's stream.
    An attempt starts from the stub list (every vertex d times) and runs rounds: shuffle the stubs, pair
    consecutive ones, accept a pair that is neither a loop nor an edge already (this round's included), count the
    stubs of a rejected pair as potential.  When no two distinct potential vertices are left that are not joined,
    the attempt has failed and restarts from scratch; otherwise the next round runs on the potential stubs, until
    none is left.  A round that adds no edge is a stall; an attempt with more than REGULAR_MAX_STALLS of them
    fails too, which bounds the rounds of an attempt by n d / 2 + REGULAR_MAX_STALLS + 1.  More than max_restarts
    restarts raise ValueError (likely only for d close to n - 1)."""
    for _ in range(max_restarts + 1):
        edges = set()
        stubs = np.tile(np.arange(n, dtype=np.int64), d)
        stalls = 0
        while stubs.size:
            rng.shuffle(stubs)
            pot = np.zeros(n, dtype=np.int64)
            before = len(edges)
            for a, b in zip(stubs[0::2].tolist(), stubs[1::2].tolist()):
                key = min(a, b) * n + max(a, b)
                if a != b and key not in edges:
                    edges.add(key)
                else:
                    pot[a] += 1
                    pot[b] += 1
            pv = np.flatnonzero(pot)
            if pv.size == 0:
                break
            # a joinable pair is left iff some potential vertex is joined to fewer than all other potential ones
            if not any(min(u, v) * n + max(u, v) not in edges
                       for x, u in enumerate(pv.tolist()) for v in pv[:x].tolist()):
                stubs = None
                break
            stalls += len(edges) == before
            if stalls > REGULAR_MAX_STALLS:
                stubs = None
                break
            stubs = np.repeat(pv, pot[pv])
        if stubs is not None:
            keys = np.fromiter(sorted(edges), dtype=np.int64, count=len(edges))
            return keys // n, keys % n
    raise ValueError(f"no {d}-regular graph on {n} vertices after {max_restarts} restarts of the pairing algorithm")


def _ring_edges(n, k):
    """Edges (iu < ju) of the ring lattice networkx.watts_strogatz_graph(n, k, 0): i ~ j iff their circular
    distance min(|i - j|, n - |i - j|) is in [1, k // 2]."""
    iu, ju = np.triu_indices(n, 1)
    dist = np.minimum(ju - iu, n - (ju - iu))
    keep = dist <= k // 2
    return iu[keep], ju[keep]


def edge_cap(kind, n, param, slack_sd=10.0):
    """Edge-slot size per graph for on-device generation: exact for BA (2 m (N - m)), REG (N d) and WS
    (N min(2 (k // 2), N - 1): k // 2 = N / 2 reaches the antipode from both sides, one neighbour), mean +
    slack_sd standard deviations for ER."""
    if kind == "BA":
        return 2 * int(param) * (n - int(param))
    if kind == "REG":
        return n * _integer_param(kind, n, param)
    if kind == "WS":
        return n * min(2 * (_integer_param(kind, n, param) // 2), n - 1)
    pairs = n * (n - 1) / 2.0
    mean, sd = 2.0 * pairs * param, 2.0 * np.sqrt(pairs * param * (1 - param))
    return int(mean + slack_sd * sd + 64)


class GraphStore:
    """G graphs of N vertices resident on the device (eco_graph_set).  edge_weights: float64 [total edges]
    parallel to `edges` for a float-weighted store (EdgeType.RANDOM), None for integer weights; a store holds one
    kind (`float_weights`)."""

    def __init__(self, row_ptr, edge_base, edges, device="cuda", stream=None, unit_weights=None,
                 edge_weights=None):
        dev = torch.device(device)
        self.device = dev
        self.float_weights = edge_weights is not None
        if self.float_weights:
            if unit_weights:
                raise ValueError("a float-weighted store cannot have unit_weights")
            unit_weights = False
            if isinstance(edge_weights, torch.Tensor):
                self.edge_weights = edge_weights
            else:
                ew = np.ascontiguousarray(edge_weights, dtype=np.float64)
                self.edge_weights = torch.from_numpy(ew if ew.size else np.zeros(1, np.float64)).to(dev)
        else:
            self.edge_weights = None
        if isinstance(row_ptr, torch.Tensor):
            self.row_ptr, self.edge_base, self.edges = row_ptr, edge_base, edges
            self.n_graphs, n1 = row_ptr.shape
        else:
            row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
            self.n_graphs, n1 = row_ptr.shape
            self.row_ptr = torch.from_numpy(row_ptr).to(dev)
            self.edge_base = torch.from_numpy(np.ascontiguousarray(edge_base, dtype=np.int64)).to(dev)
            e = np.ascontiguousarray(edges, dtype=np.uint32).view(np.int32)
            self.edges = torch.from_numpy(e if e.size else np.zeros(1, np.int32)).to(dev)
        self.n_spins = n1 - 1
        if self.n_spins > _lib.ECO_MAX_SPINS_WG:
            raise ValueError(f"N={self.n_spins} exceeds ECO_MAX_SPINS_WG={_lib.ECO_MAX_SPINS_WG}")
        if self.n_spins > _lib.ECO_MAX_SPINS and self.float_weights:
            raise ValueError(f"a float-weighted store holds at most ECO_MAX_SPINS={_lib.ECO_MAX_SPINS} vertices, got "
                             f"N={self.n_spins}: {_lib.ECO_MAX_SPINS} < N <= {_lib.ECO_MAX_SPINS_WG} takes integer "
                             "weights only")
        self.deg = torch.zeros(self.n_graphs, self.n_spins, dtype=torch.int32, device=dev)
        self.max_deg = torch.zeros(self.n_graphs, dtype=torch.int32, device=dev)
        self.meta = torch.zeros(self.n_graphs, 4, dtype=torch.float64, device=dev)
        self.valid = torch.zeros(self.n_graphs, dtype=torch.int32, device=dev)
        if unit_weights is None:  # every stored weight +-1: the dense-aggregation MPNN path applies
            w = (self.edges.view(torch.int32) >> 24).to(torch.int8)
            unit_weights = bool((w.abs() == 1).all().item()) if self.edges.numel() > 1 else True
        self.unit_weights = bool(unit_weights)
        # dense-MPNN bitmask operand, built by eco_graphs_prepare (one graph per workgroup sizes only)
        nb = _lib.lib.eco_graphs_adjbits_bytes(self.n_spins, self.n_graphs) if self.unit_weights else 0
        self.adjbits = torch.zeros(nb // 4, dtype=torch.int32, device=dev) if nb else None
        self.gs = _lib.GraphSet(self.n_graphs, self.n_spins, self.row_ptr.data_ptr(), self.edge_base.data_ptr(),
                                self.edges.data_ptr(), self.deg.data_ptr(), self.max_deg.data_ptr(),
                                self.meta.data_ptr(), self.valid.data_ptr(), int(self.unit_weights),
                                self.adjbits.data_ptr() if nb else None,
                                self.edge_weights.data_ptr() if self.float_weights else None)
        _lib.check(_lib.lib.eco_graphs_prepare(ctypes.byref(self.gs), _lib.stream_ptr(stream)))

    @classmethod
    def slots(cls, n_graphs, n, cap, device="cuda", weights="discrete"):
        """Empty store with fixed edge slots (edge_base[g] = g * cap) for eco_graphs_generate;
        weights="random": a float-weighted store (float64 weight slots next to the edge words)."""
        dev = torch.device(device)
        rp = torch.zeros(n_graphs, n + 1, dtype=torch.int32, device=dev)
        eb = torch.arange(n_graphs, dtype=torch.int64, device=dev) * int(cap)
        ed = torch.zeros(max(1, n_graphs * int(cap)), dtype=torch.int32, device=dev)
        if weights == "random":
            st = cls(rp, eb, ed, device=dev,
                     edge_weights=torch.zeros(max(1, n_graphs * int(cap)), dtype=torch.float64, device=dev))
        else:
            st = cls(rp, eb, ed, device=dev, unit_weights=True)  # eco_graphs_generate writes +-1 / 1 weights
        st.cap = int(cap)
        return st

    @classmethod
    def generated(cls, kind, n_graphs, n, param, seed=0, weights="discrete", device="cuda"):
        """Pool of n_graphs ER(n, p=param) / BA(n, m=param) / REG(n, d=param) / WS(n, k=param) graphs generated
        on the device."""
        st = cls.slots(n_graphs, n, edge_cap(kind, n, param), device=device, weights=weights)
        st.generate(0, n_graphs, kind, param, seed, weights)
        return st

    def generate(self, first, count, kind, param, seed, weights="discrete", stream=None, check=True):
        """Regenerate graphs [first, first+count) in place on the device (eco_graphs_generate);
        check=True synchronises and raises on an edge-slot overflow (or a 'REG' graph out of restarts).
        kind 'ER' (param p), 'BA' (m), 'REG' (random d-regular, d) or 'WS' (ring lattice, k)."""
        if not hasattr(self, "cap"):
            raise ValueError("generate() needs a store created with GraphStore.slots()")
        ws = torch.empty(_lib.lib.eco_graphs_generate_workspace_bytes(self.n_spins, count), dtype=torch.uint8,
                         device=self.device)
        k = {"ER": _lib.ECO_GRAPH_ER, "BA": _lib.ECO_GRAPH_BA, "REG": _lib.ECO_GRAPH_REGULAR,
             "WS": _lib.ECO_GRAPH_WS}[kind]
        wk = {"uniform": _lib.ECO_WEIGHTS_UNIFORM, "discrete": _lib.ECO_WEIGHTS_DISCRETE,
              "random": _lib.ECO_WEIGHTS_RANDOM}[weights]
        if (weights == "random") != self.float_weights:
            raise ValueError("a store holds one weight kind: weights='random' needs a store made with "
                             "weights='random', and the integer kinds one made without")
        _lib.check(_lib.lib.eco_graphs_generate(ctypes.byref(self.gs), first, count, k, float(param),
                                                wk, ctypes.c_uint64(seed), self.cap,
                                                _lib.ptr(ws), _lib.stream_ptr(stream)))
        if check:  # an edge-slot overflow leaves an empty graph and sets the device error word
            self.check_errors(stream)

    def check_errors(self, stream=None):
        """Synchronise `stream` and raise the first device-side error (eco_check_errors)."""
        _lib.check(_lib.lib.eco_check_errors(_lib.stream_ptr(stream)))

    @classmethod
    def from_csr(cls, csr, device="cuda"):
        """Store from a CSR of dense_to_csr / edges_to_csr / random_csr, float weights included."""
        return cls(csr[0], csr[1], csr[2], device=device, edge_weights=csr.weights)

    @classmethod
    def from_dense(cls, matrices, device="cuda"):
        return cls.from_csr(dense_to_csr(matrices), device=device)

    @classmethod
    def from_edges(cls, n, i, j, w, device="cuda"):
        """Single-graph store from an undirected edge list (GSet .mc instances, load_gset)."""
        return cls.from_csr(edges_to_csr(n, i, j, w), device=device)

    @classmethod
    def random(cls, kind, n_graphs, n, param, seed=0, weights="discrete", device="cuda"):
        return cls.from_csr(random_csr(kind, n_graphs, n, param, seed, weights), device=device)

    def dense(self, g):
        """Host dense adjacency of graph g (for the reference-format observation); the float64 weights of a
        float-weighted store."""
        rp = self.row_ptr[g].cpu().numpy()
        b = int(self.edge_base[g].item())
        e = self.edges[b:b + int(rp[-1])].cpu().numpy().view(np.uint32)
        m = np.zeros((self.n_spins, self.n_spins))
        rows = np.repeat(np.arange(self.n_spins), np.diff(rp))
        if self.float_weights:
            m[rows, e & 0xFFFFFF] = self.edge_weights[b:b + int(rp[-1])].cpu().numpy()
        else:
            m[rows, e & 0xFFFFFF] = ((e >> 24).astype(np.uint8)).view(np.int8)
        return m
