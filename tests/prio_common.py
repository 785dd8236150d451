"""Exact restatement of the device prioritised replay (csrc/eco_prio.hip, include/eco_hip.h eco_prio_*) in Python
integers and numpy float64: the counter RNG, the mass formula, push, the stratified proportional sampler and the
importance weights.  Every sum is a Python int, so nothing here depends on an order of operations; the only
floating-point steps are one float64 pow each in `mass_of` and `weights`."""
import numpy as np

MASK = (1 << 64) - 1
PRIO_ONE = 1 << 16          # the mass of priority p = 1
PRIO_MAX = (1 << 31) - 1
PRIO_BLOCK = 1024           # entries per block sum of the kernels (the tests choose sizes around it)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def rng3(seed, a, b):
    """csrc/eco_common.h rng3."""
    return mix64(mix64(mix64(seed & MASK) ^ (a & MASK)) ^ ((b * 0xD6E8FEB86659FD93) & MASK))


def mass_of(abs_td, alpha, eps, td_max):
    """clamp(rint((min(|td|, td_max) + eps)^alpha * 2^16), 1, 2^31 - 1) of float32 |td| values, in float64 (a NaN
    counts as td_max); returns int64."""
    t = np.asarray(abs_td, np.float32).astype(np.float64)
    p = np.where(t < td_max, t, np.float64(td_max)) + np.float64(eps)
    v = np.rint(np.power(p, np.float64(alpha)) * 65536.0)
    return np.clip(v, 1.0, float(PRIO_MAX)).astype(np.int64)


def push(mass, pos, batch, size_before):
    """eco_prio_push on a list / array of ints, in place: the `batch` positions from pos (wrapping) take the largest
    mass of the first size_before positions, or PRIO_ONE for an empty buffer."""
    cap = len(mass)
    mx = max((int(v) for v in mass[:size_before]), default=0) or PRIO_ONE
    for i in range(batch):
        mass[(pos + i) % cap] = mx
    return mx


def strata(S, m):
    """[lo_0, ..., lo_m]: lo_k = q k + (r k) // m with q, r = divmod(S, m); lo_0 = 0 and lo_m = S."""
    q, r = divmod(int(S), m)
    return [q * k + (r * k) // m for k in range(m + 1)]


def draws(S, m, seed, counter):
    """u_k = lo_k + rng3(seed, counter, k) % max(1, lo_{k+1} - lo_k)."""
    lo = strata(S, m)
    return [lo[k] + rng3(seed, counter, k) % max(1, lo[k + 1] - lo[k]) for k in range(m)]


def sample(mass, size, m, seed, counter):
    """idx[k] = the smallest x < size whose inclusive prefix sum exceeds u_k (int64 array)."""
    vals = [int(v) for v in mass[:size]]
    prefix = np.cumsum(np.array(vals, dtype=object)) if vals else np.array([], dtype=object)
    S = int(prefix[-1])
    assert S > 0, "no stored mass"
    pre = [int(p) for p in prefix]
    out = np.empty(m, np.int64)
    import bisect
    for k, u in enumerate(draws(S, m, seed, counter)):
        out[k] = bisect.bisect_right(pre, u)     # first position with prefix > u
    return out


def _u64(mass, size):
    """mass[:size] as uint64, with the bound that keeps every prefix sum inside a uint64 (the kernels' own bound)."""
    assert len(mass) * (1 << 31) < (1 << 63), "capacity * 2^31 must stay below 2^63"
    v = np.asarray(mass[:size])
    assert v.size == 0 or (int(v.min()) >= 0 and int(v.max()) <= PRIO_MAX)
    return v.astype(np.uint64)


def sample_fast(mass, size, m, seed, counter):
    """sample() for rings of millions of entries: the prefix sums as one uint64 np.cumsum (exact: no sum reaches
    2^63) and the search as np.searchsorted(side="right"), the array form of bisect_right.  Equal to sample()
    entry for entry (tests/test_prio_cpu.py)."""
    prefix = np.cumsum(_u64(mass, size), dtype=np.uint64)
    S = int(prefix[-1])
    assert S > 0, "no stored mass"
    u = np.array(draws(S, m, seed, counter), dtype=np.uint64)
    return np.searchsorted(prefix, u, side="right").astype(np.int64)


def weights_fast(mass, size, idx, beta):
    """weights() with the total as one uint64 sum: the same integer S, then the same float64 statements."""
    S = np.float64(int(_u64(mass, size).sum(dtype=np.uint64)))
    mk = np.asarray(mass)[np.asarray(idx, dtype=np.int64)].astype(np.float64)
    w = np.power(np.float64(size) * mk / S, -np.float64(beta))
    return (w / w.max()).astype(np.float32)


def mass_pattern(pattern, size, capacity=5000):
    """The mass patterns of tests/test_prio_gpu.py::test_sampler_is_exact (int64 array of `capacity` entries)."""
    rng = np.random.default_rng(1000 * size + len(pattern))
    if pattern == "equal":
        mass = np.full(capacity, 777, np.int64)
    elif pattern == "random":
        mass = rng.integers(1, (1 << 20) + 1, capacity)
    elif pattern == "zeros30":
        mass = rng.integers(1, (1 << 20) + 1, capacity)
        mass[rng.random(capacity) < 0.3] = 0
        if mass[:size].sum() == 0:
            mass[0] = 1          # a stored transition has mass >= 1: S = 0 is outside the contract
    else:
        mass = np.ones(capacity, np.int64)
        mass[size // 2] = (1 << 31) - 1
    return mass                  # positions >= size hold mass too: they must never be drawn


def large_ring_pattern(pattern, size, capacity):
    """Mass of a ring of `capacity` positions for the samplers' large-size tests (int64 array).  Positions >= size
    hold mass too: they must never be drawn.
      random   uniform in [1, 2^20]
      zeros30  the same with 30 % of the positions at 0
      tail     1 everywhere but the last 700 positions of [0, size), which hold 2^31 - 1: all but about 1 / 458,000
               of the mass (size = 3,280,000; less below) sits there, so nearly every draw resolves in the last full
               block and the final partial one
      head     the mirror image: the first 700 positions"""
    rng = np.random.default_rng(size + 7 * len(pattern))
    if pattern in ("random", "zeros30"):
        mass = rng.integers(1, (1 << 20) + 1, capacity)
        if pattern == "zeros30":
            mass[rng.random(capacity) < 0.3] = 0
            mass[0] = max(int(mass[0]), 1)
    elif pattern in ("tail", "head"):
        mass = np.ones(capacity, np.int64)
        if pattern == "tail":
            mass[size - 700:size] = PRIO_MAX
        else:
            mass[:700] = PRIO_MAX
    else:
        raise ValueError(pattern)
    return mass.astype(np.int64)


def weights(mass, size, idx, beta):
    """w_k = (size * mass[x_k] / S)^(-beta) in float64 -- the product, then the quotient, then one pow, as the
    kernel orders them -- divided by the largest w of the minibatch, as float32."""
    S = np.float64(sum(int(v) for v in mass[:size]))
    mk = np.array([int(mass[int(x)]) for x in idx], np.float64)
    w = np.power(np.float64(size) * mk / S, -np.float64(beta))
    return (w / w.max()).astype(np.float32)
