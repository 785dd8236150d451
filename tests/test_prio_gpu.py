"""Device prioritised replay (csrc/eco_prio.hip, eco_dqn_td_weighted, eco_replay_compact_gather,
agents/dqn/prioritised.py) against the exact integer oracle tests/prio_common.py.

Tolerances: sampled positions are exact.  Importance weights: 4 float32 ulps (both sides do one float64 pow and a
divide before rounding to float32: 1 ulp for the pow implementations, 3 spare).  Masses written by update: +-1 unit
(the float64 pow of the device and of numpy may round differently just below a half; nothing else may).  Weighted TD:
bitwise, the bar tests/test_huber_clip_gpu.py applies to the unweighted kernel -- its inputs are short binary
fractions, so every product is exact in float32 and the one division by B is correctly rounded on both sides (the
float64 reference, rounded again to float32, cannot differ: 53 >= 2 * 24 + 2 bits)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prio_common as pc

pytestmark = pytest.mark.gpu

CAP = 5000     # five 1024-entry blocks, the last one partial


def _u32(a):
    """int values < 2^31 as the int32 tensor that carries the uint32 mass bits."""
    return torch.from_numpy(np.asarray(a, np.int64).astype(np.int32)).cuda()


def _mass_pattern(pattern, size):
    return pc.mass_pattern(pattern, size, CAP)   # shared with tests/test_prio_cpu.py


def _sample(mass_dev, size, m, seed, counter, beta, ws):
    from eco_hip import _lib
    idx = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((m,), -7.0, device="cuda")
    rc = _lib.lib.eco_prio_sample(_lib.ptr(mass_dev), mass_dev.numel(), size, m, ctypes.c_uint64(seed),
                                  ctypes.c_uint64(counter), beta, _lib.ptr(idx), _lib.ptr(w), _lib.ptr(ws),
                                  _lib.stream_ptr())
    assert rc == _lib.ECO_OK, _lib.last_error()
    torch.cuda.synchronize()
    return idx.cpu().numpy(), w.cpu().numpy()


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("size", [1, 37, 1024, 1025, 5000])
@pytest.mark.parametrize("pattern", ["equal", "random", "zeros30", "giant"])
def test_sampler_is_exact(pattern, size):
    from eco_hip import _lib
    mass = _mass_pattern(pattern, size)
    md = _u32(mass)
    ws = torch.zeros(_lib.lib.eco_prio_workspace_bytes(CAP), dtype=torch.uint8, device="cuda")
    seed, beta = 0xC0FFEE, 0.4
    for m in (1, 64, 257):
        idx, w = _sample(md, size, m, seed, 3, beta, ws)
        ref = pc.sample(mass, size, m, seed, 3)
        np.testing.assert_array_equal(idx, ref, err_msg=f"{pattern} size {size} m {m}")
        wref = pc.weights(mass, size, ref, beta)
        d = _ulps(w, wref)
        print(f"{pattern} size {size} m {m}: max weight distance {int(d.max())} ulp, duplicates {m - len(set(idx))}")
        assert d.max() <= 4, (pattern, size, m, int(d.max()))
        assert w.max() == 1.0 and w.min() > 0
        idx2, w2 = _sample(md, size, m, seed, 3, beta, ws)          # same key: the same draw, bit for bit
        assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.int32), w2.view(np.int32))
        if pattern == "giant" and m > 1:
            # the ones weigh < 5000 in all, a stratum > 8e6: at most the first and the last stratum can miss the giant
            assert (idx == size // 2).sum() >= m - 2
    if pattern == "random" and size >= 37:
        a, _ = _sample(md, size, 257, seed, 3, beta, ws)
        b, _ = _sample(md, size, 257, seed, 4, beta, ws)
        assert not np.array_equal(a, b)                              # another counter: another draw
        np.testing.assert_array_equal(b, pc.sample(mass, size, 257, seed, 4))
    assert np.array_equal(md.cpu().numpy(), mass.astype(np.int32))   # the sampler writes no mass


BIG_CAP = 3280000   # the ring of the training recipe: 3204 block sums, four per scan thread


@pytest.mark.parametrize("size", [65536, 65537, 1048576, 1048577, BIG_CAP])
@pytest.mark.parametrize("pattern", ["random", "zeros30", "tail", "head"])
def test_sampler_is_exact_on_large_rings(pattern, size):
    """Capacity 3,280,000.  nb = ceil(size / 1024) block sums: 64 (the last size one wave of prio_scan_kernel
    covers), 65 (the first block whose prefix needs the cross-wave term `acc += ws[k]`), 1024 (chunk 1, every scan
    thread busy), 1025 (chunk 2, threads 513 and up own nothing), 3204 (chunk 4); the draw's binary search runs over
    up to 3204 prefixes.  Positions exact, weights within 4 ulp (the bar and the reasoning of the file docstring), the
    mass unmodified, a repeated call bitwise equal, no position >= size drawn although those hold mass.

    What 65,537 can and cannot show: the draw never READS the prefix of the last block (its search falls back on the
    last block and subtracts bpre[nb - 2]), so a wrong bpre[64] alone passes there; blocks 64 and up of the three
    larger sizes are read.  The oracle's own draws must reach them (asserted below, on the reference alone, for
    "random" at m = 2048): at 1,048,576 a position in each of the 16 wave ranges of the scan and 1000 distinct
    blocks; at the two larger sizes every wave range that owns a full block (8 and 13) and 1000 distinct blocks; and
    "tail" at m = 2048 draws position size - 1, the lone entry of the last block at 65,537 and 1,048,577."""
    from eco_hip import _lib
    mass = pc.large_ring_pattern(pattern, size, BIG_CAP)
    md = _u32(mass)
    ws = torch.zeros(_lib.lib.eco_prio_workspace_bytes(BIG_CAP), dtype=torch.uint8, device="cuda")
    seed, beta = 0xC0FFEE, 0.4
    nb = (size + pc.PRIO_BLOCK - 1) // pc.PRIO_BLOCK
    chunk = (nb + 1023) // 1024
    for m in (1, 257, 2048):
        idx, w = _sample(md, size, m, seed, 3, beta, ws)
        ref = pc.sample_fast(mass, size, m, seed, 3)
        assert ref.min() >= 0 and ref.max() < size and (mass[ref] > 0).all()
        np.testing.assert_array_equal(idx, ref, err_msg=f"{pattern} size {size} m {m}")
        wref = pc.weights_fast(mass, size, ref, beta)
        d = _ulps(w, wref)
        blocks = np.unique(ref // pc.PRIO_BLOCK)
        waves = np.unique(blocks // chunk // 64)
        print(f"{pattern} size {size} m {m}: max weight distance {int(d.max())} ulp, {len(blocks)} distinct blocks, "
              f"{len(waves)} scan waves, {len(np.unique(ref))} distinct positions")
        assert d.max() <= 4, (pattern, size, m, int(d.max()))
        assert w.max() == 1.0 and w.min() > 0
        idx2, w2 = _sample(md, size, m, seed, 3, beta, ws)
        assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.int32), w2.view(np.int32))
        if pattern == "random" and m == 2048:
            # wave ranges that own at least one full block (at 65 and 1025 blocks the last wave range owns one
            # entry, which "tail" reaches below)
            full = {64: 1, 65: 1, 1024: 16, 1025: 8, 3204: 13}[nb]
            assert len(waves) >= full
            assert len(blocks) >= (1000 if nb >= 1024 else 64)
        if pattern == "tail" and m == 2048:
            assert ref.max() == size - 1      # the last position, alone in its block at 65,537 and 1,048,577
        if pattern in ("tail", "head") and m > 1:
            # the 700 giants hold all but size / (700 * 2^31) < 3e-6 of the mass: at most the first and the last
            # stratum can reach a one
            giants = (ref >= size - 700) if pattern == "tail" else (ref < 700)
            assert giants.sum() >= m - 2
    assert np.array_equal(md.cpu().numpy(), mass.astype(np.int32))   # the sampler writes no mass


def test_push_takes_the_maximum_of_more_than_256_blocks():
    """prio_push_kernel's strided `b += 256` maximum over the block maxima: the single largest mass sits in block
    292 (position 299,999 of 300,000 stored) and in block 2929 (position 3,000,000 of a full ring), both beyond the
    first 256 block maxima that one pass of the 256 threads reads; then a larger mass beyond size_before, which must be
    ignored.  The whole ring against pc.push."""
    from eco_hip import _lib
    ws = torch.zeros(_lib.lib.eco_prio_workspace_bytes(BIG_CAP), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(11)
    base = rng.integers(1, 1 << 24, BIG_CAP)
    giant = (1 << 30) + 12345
    for size_before, at, pos, batch in ((300000, 299999, 300000, 48), (BIG_CAP, 3000000, BIG_CAP - 20, 48),
                                        (300000, 300100, 300000, 48)):
        mass = base.copy()
        mass[at] = giant
        md = _u32(mass)
        rc = _lib.lib.eco_prio_push(_lib.ptr(md), BIG_CAP, pos, batch, size_before, _lib.ptr(ws), _lib.stream_ptr())
        assert rc == _lib.ECO_OK, _lib.last_error()
        torch.cuda.synchronize()
        ref = mass.copy()
        mx = pc.push(ref, pos, batch, size_before)
        got = md.cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(got, ref)
        written = (np.arange(BIG_CAP) - pos) % BIG_CAP < batch
        assert written.sum() == batch and (got[written] == mx).all()
        if at < size_before:
            assert mx == giant and at // pc.PRIO_BLOCK >= 256
        else:
            assert mx == mass[:size_before].max() < (1 << 24) and got[at] == giant   # not stored yet: ignored, kept
        # the maximum is one entry, outside the first 256 blocks: a maximum over those alone is another value
        assert mass[:256 * pc.PRIO_BLOCK].max() != mx or at >= size_before


def test_push_wraps_and_takes_the_current_maximum():
    from eco_hip import _lib
    cap = 100
    ws = torch.zeros(_lib.lib.eco_prio_workspace_bytes(cap), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(7)
    mass = rng.integers(1, 1 << 24, cap)
    mass[55] = (1 << 30) + 12345

    def push(m, pos, batch, size_before):
        md = _u32(m)
        rc = _lib.lib.eco_prio_push(_lib.ptr(md), cap, pos, batch, size_before, _lib.ptr(ws), _lib.stream_ptr())
        assert rc == _lib.ECO_OK, _lib.last_error()
        torch.cuda.synchronize()
        ref = [int(v) for v in m]
        pc.push(ref, pos, batch, size_before)
        return md.cpu().numpy().astype(np.int64), np.array(ref)

    got, ref = push(mass, 80, 48, cap)                   # full ring: positions 80..99 and 0..27
    np.testing.assert_array_equal(got, ref)
    written = np.zeros(cap, bool)
    written[80:] = written[:28] = True
    assert (got[written] == (1 << 30) + 12345).all() and np.array_equal(got[~written], mass[~written])
    got, ref = push(mass, 40, 10, 40)                    # the maximum of the first 40 only (55 is not stored yet)
    np.testing.assert_array_equal(got, ref)
    assert (got[40:50] == mass[:40].max()).all() and got[55] == mass[55]
    got, ref = push(np.zeros(cap, np.int64), 80, 48, 0)  # empty buffer: the mass of p = 1
    np.testing.assert_array_equal(got, ref)
    assert (got[written] == 1 << 16).all() and (got[~written] == 0).all()


@pytest.mark.parametrize("alpha", [0.0, 0.6, 1.0])
def test_update_writes_the_mass_formula(alpha):
    from eco_hip import _lib
    cap, eps, td_max = 64, 1e-3, 2.0
    base = np.array([0.0, 1e-6, 0.5, td_max, 10 * td_max], np.float32)
    rng = np.random.default_rng(3)
    extra = rng.random(20).astype(np.float32) * 3
    # two entries per value: duplicates of an index carry the same |td|
    idx = np.concatenate([np.arange(5), np.arange(5), 10 + np.arange(20), [63, 63]]).astype(np.int32)
    td = np.concatenate([base, base, extra, np.float32([1.25, 1.25])]).astype(np.float32)
    md = torch.full((cap,), 123, dtype=torch.int32, device="cuda")
    idx_d, td_d = torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda()
    rc = _lib.lib.eco_prio_update(_lib.ptr(md), cap, len(idx), _lib.ptr(idx_d), _lib.ptr(td_d), alpha, eps, td_max,
                                  _lib.stream_ptr())
    assert rc == _lib.ECO_OK, _lib.last_error()
    torch.cuda.synchronize()
    got = md.cpu().numpy().astype(np.int64)
    ref = pc.mass_of(td, alpha, eps, td_max)
    d = np.abs(got[idx] - ref)
    print(f"alpha {alpha}: max |mass - oracle| = {int(d.max())}, masses {got[:5].tolist()}")
    assert d.max() <= 1
    untouched = np.setdiff1d(np.arange(cap), idx)
    assert (got[untouched] == 123).all()
    assert got[3] == got[4]                       # |td| clamps at td_max
    if alpha == 0.0:
        assert (got[idx] == 1 << 16).all()
    assert got.min() >= 1


# ------------------------------------------------------------------ weighted TD
def _td_inputs():
    """B = 5, N = 7: q, rewards and target Q multiples of 1/8 in [-4, 4], gamma = 0.5 (td a multiple of 1/16),
    weights multiples of 1/8 in (0, 1]: every product below is exact in float32.  d = 0, 1 (the Huber boundary),
    -7.5 (far outside), 15/16 (just inside) and one random value; a_star has an out-of-range entry."""
    B, N = 5, 7
    g = torch.Generator().manual_seed(5)
    eighth = lambda *shape: torch.randint(-32, 33, shape, generator=g).float() / 8   # noqa: E731
    q_s, q_tn, rew = eighth(B, N), eighth(B, N), eighth(B)
    act = torch.tensor([0, 6, 3, 3, 2], dtype=torch.int32)
    a_star = torch.tensor([1, 5, -1, 2, 4], dtype=torch.int32)
    done = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0])
    pins = [(0.0, 0.5, 0.0), (1.0, 0.5, 0.0), (-7.5, 3.5, 0.0), (15 / 16, 0.5, 1 / 8)]
    for b, (d, r, qt) in enumerate(pins):
        rew[b] = r
        q_tn[b, max(int(a_star[b]), 0)] = qt
        q_s[b, act[b]] = r + (1 - float(done[b])) * 0.5 * qt + d
    w = torch.tensor([1.0, 0.5, 0.25, 0.75, 0.125])
    return (q_s, q_tn, a_star, act, rew, done), w


def _td_reference(inputs, w, gamma, huber):
    q_s, q_tn, a_star, act, rew, done = inputs
    B, N = q_s.shape
    a = a_star.long()
    a = torch.where((a >= 0) & (a < N), a, torch.zeros_like(a))
    qt = q_tn.double().gather(1, a[:, None])
    td = rew.double()[:, None] + (1 - done.double()[:, None]) * gamma * qt
    q = q_s.double().requires_grad_(True)
    qa = q.gather(1, act.long()[:, None])
    per = (F.smooth_l1_loss(qa, td, reduction="none") if huber else F.mse_loss(qa, td, reduction="none"))[:, 0]
    loss = (w.double() * per).mean()
    loss.backward()
    # |q - td| recomputed in float32 (every term is exact there)
    td32 = rew + (1 - done) * gamma * q_tn.gather(1, a[:, None])[:, 0]
    abs32 = (q_s.gather(1, act.long()[:, None])[:, 0] - td32).abs()
    return q.grad.float(), (w.double() * per.detach()).float(), loss.detach().float().reshape(1), abs32


def _td_call(fn, inputs, gamma, kind, w=None, want_abs=False):
    from eco_hip import _lib
    q_s, q_tn, a_star, act, rew, done = (t.cuda() for t in inputs)
    B, N = q_s.shape
    dq = torch.full((B, N), 7.0, device="cuda")
    sq = torch.full((B,), 7.0, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    abs_td = torch.full((B,), 7.0, device="cuda") if want_abs else None
    wd = None if w is None else w.cuda()
    args = [_lib.ptr(q_s), _lib.ptr(q_tn), _lib.ptr(a_star), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), B, N,
            ctypes.c_float(gamma), 0, kind, _lib.ptr(dq), _lib.ptr(sq), _lib.ptr(loss)]
    if fn == "eco_dqn_td_weighted":
        args += [_lib.ptr(wd), _lib.ptr(abs_td)]
    rc = getattr(_lib.lib, fn)(*args, _lib.stream_ptr())
    assert rc == _lib.ECO_OK, _lib.last_error()
    torch.cuda.synchronize()
    return dq.cpu(), sq.cpu(), loss.cpu(), None if abs_td is None else abs_td.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("huber", [False, True])
def test_weighted_td_matches_float64_autograd_and_plain_td_without_weights(huber):
    from eco_hip import _lib
    kind = _lib.ECO_LOSS_HUBER if huber else _lib.ECO_LOSS_MSE
    inputs, w = _td_inputs()
    # both NULL: eco_dqn_td_loss, bit for bit
    dq0, sq0, loss0, _ = _td_call("eco_dqn_td_loss", inputs, 0.5, kind)
    dq1, sq1, loss1, _ = _td_call("eco_dqn_td_weighted", inputs, 0.5, kind)
    assert torch.equal(_bits(dq0), _bits(dq1)) and torch.equal(_bits(sq0), _bits(sq1))
    assert torch.equal(_bits(loss0), _bits(loss1)) and float(dq0.abs().max()) > 0
    # weights and |td|
    ref_dq, ref_per, ref_loss, ref_abs = _td_reference(inputs, w, 0.5, huber)
    assert sorted(ref_abs.tolist())[:1] == [0.0] and 1.0 in ref_abs.tolist() and 7.5 in ref_abs.tolist()
    dq, sq, loss, abs_td = _td_call("eco_dqn_td_weighted", inputs, 0.5, kind, w=w, want_abs=True)
    print(f"huber {huber}: loss {float(loss)!r} ref {float(ref_loss)!r}; abs_td {abs_td.tolist()}")
    assert torch.equal(_bits(dq), _bits(ref_dq))
    assert torch.equal(_bits(sq), _bits(ref_per))
    assert torch.equal(_bits(loss), _bits(ref_loss))
    assert torch.equal(_bits(abs_td), _bits(ref_abs))
    assert not torch.equal(dq, dq0)
    # |td| alone (no weights): the unweighted values, and the same |td|
    dq2, sq2, loss2, abs2 = _td_call("eco_dqn_td_weighted", inputs, 0.5, kind, want_abs=True)
    assert torch.equal(_bits(dq2), _bits(dq0)) and torch.equal(_bits(sq2), _bits(sq0))
    assert torch.equal(_bits(loss2), _bits(loss0)) and torch.equal(_bits(abs2), _bits(ref_abs))


# ------------------------------------------------------------------ the two rings
def _er20_env(B, n_graphs=64, seed=20):
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    n = 20
    store = GraphStore.random("ER", n_graphs, n, 0.15, seed=seed)
    env = VecSpinSystem(store, B, 2 * n, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                        extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                        spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n)
    return store, env


def _same(a, b):
    return all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                           v.view(torch.int32) if v.dtype == torch.float32 else v) for u, v in zip(a, b))


def test_both_rings_give_one_minibatch_for_one_idx():
    from eco_hip import _lib
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    n, B, C = 20, 8, 64
    store, env = _er20_env(B)
    feat = ReplayBuffer(C, n, device="cuda", seed=17)
    comp = CompactReplayBuffer(C, env, seed=17)
    env.reset(graph_ids=np.arange(B), seed=3)
    comp.snapshot()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = env.obs_x.clone()
    rng = np.random.default_rng(2)

    def gather_both(m):
        idx = torch.from_numpy(rng.integers(0, len(feat), m).astype(np.int32)).cuda()   # duplicates included
        a, b = feat._buffers(m), comp._buffers(m)
        for t in a + b:
            t.fill_(-9)
        _lib.check(_lib.lib.eco_replay_gather(ctypes.byref(feat.rb), m, _lib.ptr(idx), *(_lib.ptr(t) for t in a),
                                              _lib.stream_ptr()))
        _lib.check(_lib.lib.eco_replay_compact_gather(
            ctypes.byref(env.cfg), _lib.ptr(env.state), ctypes.byref(store.gs), B, _lib.ptr(comp.ring), C, len(comp),
            comp._pushed, m, _lib.ptr(idx), *(_lib.ptr(t) for t in b), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert _same(a, b)
        assert float(a[0].abs().max()) > 0 and int(a[2].min()) >= 0
        return idx, a

    for t in range(13):            # 104 transitions into a ring of 64: wraps, not at a batch boundary of the ring
        acts = torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32)
        nxt = torch.empty_like(x)
        _, rew, done = env.step(acts, obs_out=nxt)
        feat.add_batch(x, nxt, env.graph_ids, acts, rew, done)
        comp.add_step(acts, rew, done)
        x = nxt.clone()
        if t == 4:                 # before the ring is full: positions [0, 40)
            assert len(feat) == len(comp) == 40
            gather_both(50)
            mask = (torch.arange(B, device="cuda") % 2).to(torch.uint8)   # masked reset onto new graphs
            env.reset(graph_ids=np.arange(B) + B, mask=mask, seed=9)
            comp.snapshot(mask)
            x = env.obs_x.clone()
    env.check_errors()
    assert len(feat) == len(comp) == C
    idx, a = gather_both(100)
    # the gathered rows are the ring's rows at those positions
    assert torch.equal(a[0], feat.xs[idx.long()]) and torch.equal(a[3], feat.act[idx.long()])
    # the uniform sampler of the compact ring still returns what the feature ring returns under equal keys
    for m in (C // 2, C):
        assert _same(feat.sample(m), comp.sample(m))
    # an out-of-range position leaves its rows untouched
    bad = torch.tensor([3, -1, C, 5], dtype=torch.int32, device="cuda")
    b = comp._buffers(4)
    for t in b:
        t.fill_(-9)
    _lib.check(_lib.lib.eco_replay_compact_gather(
        ctypes.byref(env.cfg), _lib.ptr(env.state), ctypes.byref(store.gs), B, _lib.ptr(comp.ring), C, len(comp),
        comp._pushed, 4, _lib.ptr(bad), *(_lib.ptr(t) for t in b), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert b[2].tolist()[1:3] == [-9, -9] and float(b[0][1].max()) == -9 and b[2].tolist()[0] >= 0


def test_cut_gather_on_the_128_thread_path():
    """eco_replay_compact_gather on a MaxCut ring above 256 vertices (128 threads, several vertices per thread;
    the test above stays on the 64-thread path): for positions drawn with duplicates, across a masked reset and a
    ring wrap, the rows equal the feature ring's eco_replay_gather bit for bit, and the rows of the two positions
    outside [0, len(ring)) keep what they held."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    n, B, m = 257, 12, 40
    C = 5 * B
    store = GraphStore.random("ER", 2 * B, n, 0.15, seed=n)
    env = VecSpinSystem(store, B, 2 * n, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                        extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                        spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n)
    feat = ReplayBuffer(C, n, device="cuda", seed=17)
    comp = CompactReplayBuffer(C, env, seed=17)
    env.reset(graph_ids=np.arange(B), seed=3)
    comp.snapshot()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = env.obs_x.clone()
    for t in range(8):             # 96 transitions into a ring of 60: wraps
        acts = torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32)
        nxt = torch.empty_like(x)
        _, rew, done = env.step(acts, obs_out=nxt)
        feat.add_batch(x, nxt, env.graph_ids, acts, rew, done)
        comp.add_step(acts, rew, done)
        x = nxt.clone()
        if t == 3:                 # masked reset of half the episodes onto new graphs
            mask = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
            env.reset(graph_ids=np.arange(B) + B, mask=mask, seed=9)
            comp.snapshot(mask)
            x = env.obs_x.clone()
    env.check_errors()
    assert len(feat) == len(comp) == C
    pos = np.random.default_rng(11).integers(0, C, m).astype(np.int32)   # duplicates included
    assert len(set(pos.tolist())) < m
    pos[7], pos[23] = -1, C
    keep = np.flatnonzero((pos >= 0) & (pos < C))
    assert len(keep) == m - 2
    idx, idx_in = torch.from_numpy(pos).cuda(), torch.from_numpy(pos[keep]).cuda()
    a, b = feat._buffers(len(keep)), comp._buffers(m)
    for t in a + b:
        t.fill_(-9)
    _lib.check(_lib.lib.eco_replay_gather(ctypes.byref(feat.rb), len(keep), _lib.ptr(idx_in),
                                          *(_lib.ptr(t) for t in a), _lib.stream_ptr()))
    _lib.check(_lib.lib.eco_replay_compact_gather(
        ctypes.byref(env.cfg), _lib.ptr(env.state), ctypes.byref(store.gs), B, _lib.ptr(comp.ring), C, len(comp),
        comp._pushed, m, _lib.ptr(idx), *(_lib.ptr(t) for t in b), _lib.stream_ptr()))
    torch.cuda.synchronize()
    kd = torch.from_numpy(keep).cuda()
    assert _same(a, [t[kd] for t in b])    # features of s and s', graph id, action, reward, done
    assert float(a[0].abs().max()) > 0 and int(a[2].min()) >= 0
    for t in b:
        assert bool((t[[7, 23]] == -9).all())


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("alpha", [0.6, 0.0])
@pytest.mark.parametrize("compact", [True, False])
def test_dqn_learns_with_prioritised_replay_without_host_sync(compact, alpha):
    """DQN(prioritised_replay=...) on ER-20, B = 16, M = 32, two gradient steps per vector step (so the prefetch of
    minibatch k + 1 follows the priority update of minibatch k), about 40 vector steps past replay_start_size, the
    steady state under torch's sync-debug mode "error".  Every push and every update is logged on the device (clones,
    no host read) and the final mass is explained position by position: a position sampled since its last push
    carries the mass of its last |td| (+-1), a stored position never sampled since carries the maximum pushed into it,
    an unwritten position 0.  alpha = 0: every stored mass is 2^16 and every weight exactly 1."""
    from test_dqn_gpu import _dqn_for
    from eco_hip.graphs import GraphStore
    from eco_hip.agents.dqn.prioritised import DevicePrioritisedReplay
    n, B, M, cap = 20, 16, 32, 4096
    store = GraphStore.random("ER", 256, n, 0.15, seed=4)
    cfg = {"alpha": alpha, "beta0": 0.4, "beta_steps": 50, "eps": 1e-3}
    agent = _dqn_for(store, n, B=B, replay_start_size=8 * B, replay_buffer_size=cap, train_minibatch=M,
                     minibatch_size=64, update_frequency=16, compact_replay=compact, prioritised_replay=cfg)
    prio = agent.replay_buffer
    assert isinstance(prio, DevicePrioritisedReplay) and prio is agent._prio and prio.compact == compact
    assert prio.td_max == 1.0 and prio.alpha == alpha
    log = []
    push0, update0 = prio._push, prio.update

    def push(pos, batch, size_before, stream=None):
        push0(pos, batch, size_before, stream)
        log.append(("push", pos, batch, size_before, prio.mass[pos:pos + 1].clone()))

    def update(abs_td, stream=None):
        update0(abs_td, stream)
        log.append(("update", prio.last_idx.clone(), abs_td.clone(), prio.last_weights.clone()))
    prio._push, prio.update = push, update

    total = (8 + 40) * B
    steady = {"n": 0, "on": False, "steps": 0}

    def on_step(t):
        if agent._ready:
            steady["n"] += 1
        on = 4 <= steady["n"] and t < total
        steady["steps"] += on
        if on != steady["on"]:
            torch.cuda.set_sync_debug_mode("error" if on else "default")
            steady["on"] = on
    try:
        agent.learn(timesteps=total, on_vector_step=on_step)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert steady["steps"] >= 30 and agent.grad_steps >= 70 and agent._k_per_vec == 2
    losses = np.array(agent.losses())[:, 1]
    assert len(losses) == agent.grad_steps and np.isfinite(losses).all()
    assert torch.isfinite(agent.network.flat).all()
    assert abs(prio.beta - 1.0) < 1e-12 and prio._counter >= 50

    mass = prio.mass.cpu().numpy().astype(np.int64)
    model = np.zeros(cap, np.int64)       # the expected mass, updates through the oracle
    last = [None] * cap                   # ("push", value) / ("update", |td|)
    n_up = 0
    for ev in log:
        if ev[0] == "push":
            _, pos, batch, size_before, val = ev
            val = int(val.item())
            want = int(model[:size_before].max()) if size_before else pc.PRIO_ONE
            assert abs(val - want) <= 1, (pos, val, want)       # the current maximum (itself +-1 when an update's)
            for i in range(batch):
                model[(pos + i) % cap] = val
                last[(pos + i) % cap] = ("push", val)
        else:
            _, idx, abs_td, w = ev
            idx, abs_td, w = idx.cpu().numpy(), abs_td.cpu().numpy(), w.cpu().numpy()
            assert idx.min() >= 0 and np.isfinite(abs_td).all() and w.max() == 1.0 and w.min() > 0
            assert all(last[x] is not None for x in idx)         # only stored positions are drawn
            if alpha == 0.0:
                assert (w == 1.0).all()
            ms = pc.mass_of(abs_td, alpha, prio.eps, prio.td_max)
            for x, t, mv in zip(idx, abs_td, ms):
                model[x] = mv
                last[x] = ("update", float(t))
            n_up += 1
    assert n_up == agent.grad_steps
    stored = np.array([e is not None for e in last])
    assert stored.sum() == len(prio) == total and (mass[~stored] == 0).all()
    kinds = np.array([e[0] if e else "" for e in last])
    assert (kinds == "update").sum() > 100 and (kinds == "push").sum() >= 1
    assert (mass[kinds == "push"] == model[kinds == "push"]).all()
    d = np.abs(mass[kinds == "update"] - model[kinds == "update"])
    print(f"compact {compact} alpha {alpha}: {int((kinds == 'update').sum())} sampled positions, max |mass - oracle| "
          f"{int(d.max())}, distinct masses {len(np.unique(mass[stored]))}")
    assert d.max() <= 1
    if alpha == 0.0:
        assert (mass[stored] == pc.PRIO_ONE).all()
    else:
        assert len(np.unique(mass[stored])) > 50


def test_dqn_prioritised_constructor():
    from test_dqn_gpu import _dqn_for
    from eco_hip.graphs import GraphStore
    from eco_hip.agents.dqn.utils import CompactReplayBuffer, ReplayBuffer
    store = GraphStore.random("ER", 16, 20, 0.15, seed=4)
    agent = _dqn_for(store, 20)
    assert agent._prio is None and isinstance(agent.replay_buffer, CompactReplayBuffer)
    assert not hasattr(agent, "abs_td")
    agent = _dqn_for(store, 20, compact_replay=False, prioritised_replay={})
    assert isinstance(agent.replay_buffer.inner, ReplayBuffer) and agent.replay_buffer.alpha == 0.6
    assert agent.replay_buffer.beta0 == 0.4 and agent.replay_buffer.eps == 1e-3
    with pytest.raises(ValueError, match="unknown keys"):
        _dqn_for(store, 20, prioritised_replay={"alhpa": 0.5})
    with pytest.raises(ValueError):
        _dqn_for(store, 20, prioritised_replay={"alpha": -1.0})
