"""Cases shared by tests/test_graphgen_oracle_cpu.py (structure and coverage of the oracle's graphs) and
tests/test_graphgen_exact_gpu.py (device against oracle, byte for byte).  The shapes are the smallest at which
csrc/eco_graphgen.hip changes behaviour: the 64-lane ballot tail, more than one 64-block per row, a generated range
inside a larger store, the workgroup-per-graph prepare kernel above 512 vertices, the BA LDS and targets[] limits.
Above 512 vertices a case generates one graph (slot 1 of a 3-slot store)."""
import functools
from collections import namedtuple

from oracle import graphgen_oracle as go

Case = namedtuple("Case", "kind n param G first count seed weights")


def _c(kind, n, param, G, first=0, count=None, seed=7, weights="discrete"):
    return Case(kind, n, param, G, first, G - first if count is None else count, seed, weights)


ER_CASES = {
    "er20": _c("ER", 20, 0.15, 16),
    "er63": _c("ER", 63, 0.3, 8),
    "er64": _c("ER", 64, 0.3, 8),                         # ballot with no tail; lane 63's prefix mask
    "er65": _c("ER", 65, 0.3, 8),                         # a second 64-block of one column
    "er129_range": _c("ER", 129, 0.5, 8, first=3, count=2),   # row_cnt by relative graph, row_ptr by absolute
    "er513": _c("ER", 513, 0.02, 3, first=1, count=1),    # prepare: one workgroup per graph
    "er2049": _c("ER", 2049, 0.005, 3, first=1, count=1),
    "er65_p0": _c("ER", 65, 0.0, 4),
    "er65_p1": _c("ER", 65, 1.0, 4),
    "er65_p01": _c("ER", 65, 0.1, 8),                     # 0.1 is not a float32 number
    # p = the draw of pair {14, 17} of slot 0 itself (a multiple of 2^-24, about 0.2014): u < p leaves that edge out
    "er20_p_on_draw": _c("ER", 20, go.u01(go.rng3(7, 0, go.pair_key(14, 17, 20))), 8),
    "er65_uniform": _c("ER", 65, 0.3, 8, weights="uniform"),
    "er65_random": _c("ER", 65, 0.3, 8, weights="random"),
}
BA_CASES = {
    "ba20_4": _c("BA", 20, 4, 16),
    "ba65_1": _c("BA", 65, 1, 8),
    "ba130_64": _c("BA", 130, 64, 4),                     # targets[64] full
    "ba500_4": _c("BA", 500, 4, 4),
    "ba2049_4": _c("BA", 2049, 4, 3, first=1, count=1),   # 147,272 B of the 160 KB of dynamic LDS the host allows
    "ba20_4_range": _c("BA", 20, 4, 8, first=5, count=3),
    "ba65_4": _c("BA", 65, 4, 8),
    "ba65_4_uniform": _c("BA", 65, 4, 8, weights="uniform"),
    "ba65_4_random": _c("BA", 65, 4, 8, weights="random"),
}
REG_CASES = {
    "reg20_3": _c("REG", 20, 3, 16),
    "reg9_4": _c("REG", 9, 4, 16),
    "reg65_6": _c("REG", 65, 6, 8),
    "reg600_3": _c("REG", 600, 3, 3, first=1, count=1),
    "reg8_7": _c("REG", 8, 7, 16),                        # complete graph: stalls, never a restart
    "reg12_4_random": _c("REG", 12, 4, 8, seed=11, weights="random"),
}
WS_CASES = {
    "ws9_4": _c("WS", 9, 4, 4),
    "ws8_8": _c("WS", 8, 8, 4),                           # k / 2 = n / 2: the antipode is one neighbour
    "ws65_6_random": _c("WS", 65, 6, 4, weights="random"),
    "ws2049_6": _c("WS", 2049, 6, 3, first=1, count=1),
    "ws9_4_range": _c("WS", 9, 4, 8, first=2, count=3),
}
CASES = {**ER_CASES, **BA_CASES, **REG_CASES, **WS_CASES}
# the three weight kinds on one structure
WEIGHT_KIND_GROUPS = [("er65", "er65_uniform", "er65_random"), ("ba65_4", "ba65_4_uniform", "ba65_4_random")]


@functools.lru_cache(maxsize=None)
def oracle_graphs(name):
    """{slot: Graph} of the case's generated range, computed once for every test that needs it (read-only)."""
    c = CASES[name]
    return {g: go.generate(c.kind, c.n, c.param, c.seed, g, c.weights) for g in range(c.first, c.first + c.count)}
