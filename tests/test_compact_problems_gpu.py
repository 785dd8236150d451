"""Compact replay ring for the five set-problem targets (MIN_COVER, MIN_CUT, MAX_IND_SET, MAX_CLIQUE, MIN_DOM_SET;
csrc/eco_replay.hip, ProbRing).

The oracle is the fp32 feature ring fed by the same pushes: its rows are the env's own, and the env is pinned to the
reference in tests/test_problems_gpu.py.  Every comparison is bitwise (float32 viewed as int32), so there is no
tolerance to state."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SET_TARGETS = ["MIN_COVER", "MIN_CUT", "MAX_IND_SET", "MAX_CLIQUE", "MIN_DOM_SET"]


def _observables(target, which="main"):
    """All 13 MAIN_OBSERVABLES; MIN_CUT has no invalidity, and the env rejects the three validity-mask observables
    for it (ECO_ERR_OBSERVABLE), so it takes the other ten (still 16-float rows).  "default": the 7-observable subset
    of MAIN_OBSERVABLES the reference trains half its problems with (train_eco.py: DEFAULT_OBSERVABLES, 8-float
    rows)."""
    from eco_hip.envs.utils import DEFAULT_OBSERVABLES, MAIN_OBSERVABLES, Observable
    if which == "default":
        return DEFAULT_OBSERVABLES
    if target == "MIN_CUT":
        masks = (Observable.IMMEDIATE_VALIDITY_DIFFERENCE, Observable.IMMEDIATE_VALIDITY_CHANGE,
                 Observable.NUMBER_OF_VALIDITY_IMPROVEMENTS)
        return [o for o in MAIN_OBSERVABLES if o not in masks]
    return MAIN_OBSERVABLES


def _store(kind, n_graphs, n, target, seed):
    from eco_hip.graphs import GraphStore
    # +-1 weights for MIN_CUT (negative neighbour sums), unit weights for the set problems (train_eco.py: UNIFORM)
    return GraphStore.random(kind, n_graphs, n, 0.15 if kind == "ER" else 4, seed=seed,
                             weights="discrete" if target == "MIN_CUT" else "uniform")


def _env(store, B, T, target, basis="SIGNED", which="main"):
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import ExtraAction, OptimisationTarget, RewardSignal, SpinBasis
    return VecSpinSystem(store, B, T, observables=_observables(target, which), reward_signal=RewardSignal.BLS,
                         extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget[target],
                         spin_basis=SpinBasis[basis], norm_rewards=True, basin_reward=1. / store.n_spins,
                         reversible_spins=True)


def _same(a, b):
    return all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u,
                           v.view(torch.int32) if v.dtype == torch.float32 else v) for u, v in zip(a, b))


def _fill(env, feat, comp, steps, reset_after, on_step=None):
    """`steps` random-action steps pushed into both rings, with a masked reset of the odd episodes onto new graphs
    after step `reset_after`.  A finished episode is stepped on (the env returns its state unchanged and writes no
    rows), so the feature ring's s' of such a transition is its s: nxt starts as a copy of x.  Returns the number of
    these no-flip transitions."""
    B, n = env.n_envs, env.n_spins
    env.reset(graph_ids=np.arange(B), seed=3)
    comp.snapshot()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = env.obs_x.clone()
    noflip = 0
    for t in range(steps):
        acts = torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32)
        noflip += int(env.dones.sum())
        nxt = x.clone()
        _, rew, done = env.step(acts, obs_out=nxt)
        feat.add_batch(x, nxt, env.graph_ids, acts, rew, done)
        comp.add_step(acts, rew, done)
        x = nxt.clone()
        if on_step is not None:
            on_step(t)
        if t == reset_after:
            mask = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
            env.reset(graph_ids=np.arange(B) + B, mask=mask, seed=9)
            comp.snapshot(mask)
            x = env.obs_x.clone()
    env.check_errors()
    return noflip


CASES = [(t, "ER", 20, 64, "SIGNED", "main") for t in SET_TARGETS] + [
    ("MIN_COVER", "ER", 20, 64, "BINARY", "default"),
    ("MIN_DOM_SET", "ER", 257, 12, "SIGNED", "main"),
    ("MAX_CLIQUE", "ER", 257, 12, "SIGNED", "main"),
    ("MIN_CUT", "BA", 130, 16, "SIGNED", "main"),
]


@pytest.mark.parametrize("target,kind,n,B,basis,which", CASES)
def test_compact_ring_matches_feature_ring(target, kind, n, B, basis, which):
    """The compact ring returns exactly the transitions the fp32 feature ring returns for the same pushes and the
    same sampling keys: node features bitwise, actions, rewards, dones, graph ids -- across a masked reset (rows
    written with the previous reset's invalidity normaliser), a ring wrap (8 B pushes into 5 B slots) and episodes
    that finish inside the run (max_steps = 6: the even episodes are stepped twice after their end, which stores
    no-flip transitions).  N = 257 takes the 128-thread path with a vertex in the second slot of a thread; BA-130
    with +-1 weights gives MIN_CUT negative neighbour sums and -0.0 quality changes."""
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    store = _store(kind, 2 * B, n, target, seed=n)
    env = _env(store, B, 6, target, basis, which)
    C = B * 5
    feat = ReplayBuffer(C, n, device="cuda", seed=17, n_obs=env.n_obs)
    comp = CompactReplayBuffer(C, env, seed=17)
    noflip = _fill(env, feat, comp, steps=8, reset_after=3)
    assert noflip >= B // 2                      # the even episodes ended at step 6 and were stepped twice more
    assert len(feat) == len(comp) == C
    for m in (C // 2, C):
        a = feat.sample(m)
        b = comp.sample(m)
        names = ("xs", "act", "rew", "xn", "done", "gid")
        bad = [k for k, u, v in zip(names, a, b) if not _same([u], [v])]
        assert not bad, (bad, m)
        assert float(a[0].abs().max()) > 0
    if target == "MIN_CUT" and kind == "BA":
        xs = comp.sample(C)[0]
        assert bool((xs[:, :, 1].view(torch.int32) == -2 ** 31).any())      # a -0.0 quality change was rebuilt
        assert bool((xs[:, :, 1] > 0).any()) and bool((xs[:, :, 1] < 0).any())


def test_gather_by_explicit_position_min_dom_set():
    """eco_replay_compact_gather on a MIN_DOM_SET ring = eco_replay_gather on the feature ring for the same idx
    (duplicates, m > size), before the ring is full and after it wrapped; an index outside [0, size) leaves its
    sentinel-filled output rows untouched."""
    from eco_hip import _lib
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    n, B, C = 20, 8, 64
    store = _store("ER", 2 * B, n, "MIN_DOM_SET", seed=20)
    env = _env(store, B, 2 * n, "MIN_DOM_SET")
    feat = ReplayBuffer(C, n, device="cuda", seed=17, n_obs=env.n_obs)
    comp = CompactReplayBuffer(C, env, seed=17)
    rng = np.random.default_rng(2)

    def gather(idx):
        m = idx.numel()
        a, b = feat._buffers(m), comp._buffers(m)
        for t in a + b:
            t.fill_(-9)
        _lib.check(_lib.lib.eco_replay_gather(ctypes.byref(feat.rb), m, _lib.ptr(idx), *(_lib.ptr(t) for t in a),
                                              _lib.stream_ptr()))
        _lib.check(_lib.lib.eco_replay_compact_gather(
            ctypes.byref(env.cfg), _lib.ptr(env.state), ctypes.byref(store.gs), B, _lib.ptr(comp.ring), C, len(comp),
            comp._pushed, m, _lib.ptr(idx), *(_lib.ptr(t) for t in b), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return a, b

    def check(m):
        idx = torch.from_numpy(rng.integers(0, len(feat), m).astype(np.int32)).cuda()   # duplicates included
        a, b = gather(idx)
        assert _same(a, b)
        assert float(a[0].abs().max()) > 0 and int(a[2].min()) >= 0

    def on_step(t):
        if t == 4:                       # 40 of 64 positions written
            assert len(feat) == len(comp) == 40
            check(50)

    _fill(env, feat, comp, steps=13, reset_after=4, on_step=on_step)   # 104 pushes: wraps inside a batch
    assert len(feat) == len(comp) == C
    check(100)
    bad = torch.tensor([3, -1, C, 5], dtype=torch.int32, device="cuda")
    a, b = gather(bad)
    for k in (1, 2):
        assert all(bool((t[k] == -9).all()) for t in b)
    for k in (0, 3):
        assert _same([t[k] for t in a], [t[k] for t in b]) and int(b[2][k]) >= 0


def _set_dqn(env, **kw):
    from eco_hip.networks.mpnn import MPNN
    from eco_hip.agents.dqn.dqn import DQN
    n_obs = env.n_obs
    args = dict(init_weight_std=0.01, double_dqn=True, clip_Q_targets=False, replay_start_size=64,
                replay_buffer_size=1024, gamma=0.95, update_target_frequency=100, update_learning_rate=False,
                initial_learning_rate=1e-4, peak_learning_rate=1e-4, final_learning_rate=1e-4, update_frequency=16,
                minibatch_size=16, final_exploration_rate=0.05, final_exploration_step=2000, adam_epsilon=1e-8,
                seed=3, evaluate=False, test_save_path=None, train_minibatch=16)
    args.update(kw)
    return DQN(env, lambda: MPNN(n_obs_in=n_obs, device="cuda"), **args)


def test_training_is_identical_on_either_ring():
    """Two DQNs of one seed on MIN_COVER (N = 20, B = 16, M = 16), one on the compact ring and one on the feature
    ring: after 25 vector steps (400 env-steps, about 20 gradient steps, max_steps = 10 so that every episode is reset
    twice inside the run) of learn() the parameters, both Adam moments and the recorded losses are byte-identical --
    the rings draw the same positions from the same keys and hand the network the same bits."""
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    n, B = 20, 16
    out = []
    for compact in (True, False):
        store = _store("ER", 256, n, "MIN_COVER", seed=4)
        agent = _set_dqn(_env(store, B, 10, "MIN_COVER"), compact_replay=compact)
        assert isinstance(agent.replay_buffer, CompactReplayBuffer if compact else ReplayBuffer)
        w0 = agent.network.flat.clone()
        losses = agent.learn(timesteps=B * 25)
        agent.env.check_errors()
        assert agent.grad_steps > 0 and len(losses) > 0 and not torch.equal(w0, agent.network.flat)
        out.append((agent.network.flat.clone(), agent.exp_avg.clone(), agent.exp_avg_sq.clone(), losses,
                    agent.grad_steps))
    (w1, m1, v1, l1, g1), (w2, m2, v2, l2, g2) = out
    print("grad steps", g1, g2, "first losses", l1[:3], l2[:3])
    assert g1 == g2 and l1 == l2
    assert _same([w1, m1, v1], [w2, m2, v2])


def test_prioritised_replay_on_the_compact_ring_of_a_set_problem():
    """DQN(compact_replay=True, prioritised_replay={}) on MAX_IND_SET: DevicePrioritisedReplay gathers through
    eco_replay_compact_gather unchanged; a few hundred steps of learn() leave no device error, finite losses and
    moved parameters."""
    from eco_hip.agents.dqn.prioritised import DevicePrioritisedReplay
    from eco_hip.agents.dqn.utils import CompactReplayBuffer
    n, B = 20, 16
    store = _store("ER", 256, n, "MAX_IND_SET", seed=4)
    agent = _set_dqn(_env(store, B, 10, "MAX_IND_SET"), compact_replay=True, prioritised_replay={})
    prio = agent.replay_buffer
    assert isinstance(prio, DevicePrioritisedReplay) and isinstance(prio.inner, CompactReplayBuffer)
    w0 = agent.network.flat.clone()
    losses = agent.learn(timesteps=B * 25)
    agent.env.check_errors()
    assert agent.grad_steps > 0 and len(losses) > 0
    assert all(np.isfinite(l) for _, l in losses)
    assert torch.isfinite(agent.network.flat).all() and not torch.equal(w0, agent.network.flat)
    assert 0 < len(prio) <= B * 25 and int((prio.mass > 0).sum()) == len(prio)   # every stored position has mass


def test_rejected_configs_leave_the_outputs_untouched():
    """A float-weighted config or graph set, max_steps = 32768 and a generic target above 2048 vertices: the bytes
    query is 0 and sample / gather return ECO_ERR_ARG with sentinel-filled outputs untouched; DQN refuses
    compact_replay=True for weights that are not +-1 and keeps the feature ring for compact_replay=None."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    from eco_hip.agents.dqn.utils import ReplayBuffer, CompactReplayBuffer
    n, B, C = 20, 8, 64
    store = _store("ER", 2 * B, n, "MIN_COVER", seed=20)
    env = _env(store, B, 2 * n, "MIN_COVER")
    feat = ReplayBuffer(C, n, device="cuda", seed=17, n_obs=env.n_obs)
    comp = CompactReplayBuffer(C, env, seed=17)
    _fill(env, feat, comp, steps=4, reset_after=-1)
    fstore = GraphStore.random("ER", 2 * B, n, 0.15, seed=20, weights="random")
    assert fstore.float_weights
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    out = comp._buffers(4)

    def refused(cfg, gs):
        for t in out:
            t.fill_(-9)
        rcs = [_lib.lib.eco_replay_compact_sample(
                   ctypes.byref(cfg), _lib.ptr(env.state), ctypes.byref(gs), B, _lib.ptr(comp.ring), C, len(comp),
                   comp._pushed, 4, ctypes.c_uint64(1), ctypes.c_uint64(1), *(_lib.ptr(t) for t in out),
                   _lib.stream_ptr()),
               _lib.lib.eco_replay_compact_gather(
                   ctypes.byref(cfg), _lib.ptr(env.state), ctypes.byref(gs), B, _lib.ptr(comp.ring), C, len(comp),
                   comp._pushed, 4, _lib.ptr(idx), *(_lib.ptr(t) for t in out), _lib.stream_ptr())]
        msg = _lib.last_error()
        torch.cuda.synchronize()
        assert rcs == [_lib.ECO_ERR_ARG] * 2, rcs
        assert all(bool((t == -9).all()) for t in out)
        return msg

    copy = lambda: _lib.EnvConfig.from_buffer_copy(env.cfg)   # noqa: E731
    cfg = copy()
    cfg.float_weights = 1
    assert _lib.lib.eco_replay_compact_bytes_cfg(ctypes.byref(cfg), C, B) == 0
    assert "integer weights only" in refused(cfg, store.gs)
    assert "float-weighted graph set" in refused(copy(), fstore.gs)
    cfg = copy()
    cfg.max_steps = 32768
    assert _lib.lib.eco_replay_compact_bytes_cfg(ctypes.byref(cfg), C, B) == 0
    assert "max_steps must be < 32768" in refused(cfg, store.gs)
    cfg = copy()
    cfg.n_spins = 2049
    assert _lib.lib.eco_replay_compact_bytes_cfg(ctypes.byref(cfg), C, B) == 0
    assert "n_spins <= 2048" in refused(cfg, store.gs)
    # the accepted config still samples (the refusals above changed nothing)
    assert _same(feat.sample(16), comp.sample(16))
    # DQN: weights 2 are integer but not +-1
    rng = np.random.default_rng(0)
    mats = []
    for _ in range(2 * B):
        a = np.triu((rng.random((n, n)) < 0.2).astype(np.int64) * 2, 1)
        mats.append(a + a.T)
    heavy = GraphStore.from_dense(mats)
    assert not heavy.unit_weights and not heavy.float_weights
    with pytest.raises(ValueError, match="compact replay needs"):
        _set_dqn(_env(heavy, B, 2 * n, "MIN_COVER"), compact_replay=True)
    agent = _set_dqn(_env(store, B, 2 * n, "MIN_COVER"))
    assert agent.compact_replay is False and isinstance(agent.replay_buffer, ReplayBuffer)


@pytest.mark.parametrize("target", SET_TARGETS)
def test_ring_size(target):
    """4 B per vertex, at most 12 f64 scalars for s and for s', 16 B of graph id / action / reward / done (+ the
    256-B alignment of the 7 arrays); at N = 200 at most 1/20 of the 128 N bytes of two 16-float feature rows."""
    from eco_hip.agents.dqn.utils import CompactReplayBuffer
    n, B, C = 200, 4, 60
    env = _env(_store("ER", B, n, target, seed=1), B, 2 * n, target)
    assert env.obs_x.shape[2] == 16
    comp = CompactReplayBuffer(C, env)
    assert comp.bytes_per_transition <= 4 * n + 2 * 8 * 12 + 16 + 7 * 256 / (C + B)
    assert comp.bytes_per_transition <= 128 * n / 20
