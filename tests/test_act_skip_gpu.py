"""The epsilon-greedy act launch skips the forward of a workgroup whose episodes all drew "explore"
(act_skip_block, csrc/eco_mpnn_dev.h; the reference runs no network for a random action, dqn.py:282).  The draw is a
function of the act config's seed and counter, the episode index and the allowed-vertex count, never of Q, so the
actions must be bit-identical with the skip on (default) and off (ECO_PATH_NO_ACT_SKIP): every test runs the same
seeds both ways and compares the actions, and the env state, observations, rewards and dones after one env.step on
them, exactly.  The draw is restated on the host (mix64 / rng3 / u01 of csrc/eco_common.h) to show that the cases
hold all-explore blocks, mixed blocks and greedy episodes, and to pin the exploring episodes' actions."""
import ctypes

import numpy as np
import pytest
import torch

from mpnn_corner_common import graphs_per_block
from oracle import mpnn_oracle as mo

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SEED, COUNTER = 4, 1       # ER-20 x 64 at epsilon 0.5: all-explore and mixed blocks both occur (asserted below)


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _rng3(seed, a, b):
    return _mix64(_mix64(_mix64(seed) ^ a) ^ ((b * 0xD6E8FEB86659FD93) & M64))


def _explores(seed, counter, e, eps, n_allowed):
    """graph_act's explore decision: u01(rng3(seed, counter, e)) < epsilon && n_allowed > 0 (u01: the top 24 bits
    times 2^-24, exact in fp32; epsilon as the fp32 the act config carries)."""
    return (_rng3(seed, counter, e) >> 40) / 16777216.0 < float(np.float32(eps)) and n_allowed > 0


def _random_rank(seed, counter, e, n_allowed):
    """which of the allowed vertices (in index order) an exploring episode takes"""
    return _rng3(seed ^ 0xA5A5A5A5, counter, e) % n_allowed


def _net(seed=3):
    from eco_hip.networks.mpnn import MPNN
    net = MPNN(device="cuda")
    net.load_state_dict(mo.init_weights(torch.Generator().manual_seed(seed), std=0.1))
    return net


def _env(store, B, reversible=True):
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    n = store.n_spins
    return VecSpinSystem(store, B, 2 * n, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                         extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                         spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n,
                         reversible_spins=reversible)


def _route(store, B):
    from eco_hip import _lib
    return _lib.lib.eco_mpnn_route(ctypes.byref(store.gs), 7, B, 0, 0, 0)


def _act_and_step(store, B, eps, skip, reversible=True, spins=None, want_q=False, family_bit=0):
    """One act launch (under the kernel-family bit given) and one env.step on its actions, with the skip on or off
    -> every array the step leaves."""
    from eco_hip import _lib
    env = _env(store, B, reversible)
    x = env.reset(graph_ids=np.arange(B), spins=spins, seed=5)
    gids = torch.arange(B, dtype=torch.int32, device="cuda")
    actions = torch.full((B,), -7, dtype=torch.int32, device="cuda")    # every episode must be written
    q = torch.full((B, store.n_spins), float("nan"), device="cuda") if want_q else None
    x0 = x.clone()
    with _lib.kernel_paths(family_bit | (0 if skip else _lib.ECO_PATH_NO_ACT_SKIP)):
        _net().forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_GRAPH, q_out=q,
                              act=_lib.ActConfig(float(eps), int(reversible), float(env.allowed_action_value()),
                                                 SEED, COUNTER), actions_out=actions)
    nxt = torch.zeros_like(x)
    obs, rew, done = env.step(actions, obs_out=nxt)
    torch.cuda.synchronize()
    out = dict(actions=actions.cpu().numpy(), state=env.state.cpu().numpy(), obs=obs.cpu().numpy(),
               rewards=rew.cpu().numpy().copy(), dones=done.cpu().numpy().copy(), x0=x0.cpu().numpy())
    if want_q:
        out["q"] = q.cpu().numpy()
    return out


def _same(a, b):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def _on_off(store, B, eps, **kw):
    on = _act_and_step(store, B, eps, True, **kw)
    off = _act_and_step(store, B, eps, False, **kw)
    _same(on, off)
    n = store.n_spins
    assert ((on["actions"] >= 0) & (on["actions"] < n)).all()
    return on


def _check_explorers(res, n, eps, reversible=True, allowed_value=-1.0):
    """Every episode the host draw sends exploring took the vertex the host draw names; -> the explore flags."""
    B = len(res["actions"])
    flags = np.zeros(B, bool)
    for e in range(B):
        allowed = np.arange(n) if reversible else np.flatnonzero(res["x0"][e, :, 0] == allowed_value)
        flags[e] = _explores(SEED, COUNTER, e, eps, len(allowed))
        if flags[e]:
            assert res["actions"][e] == allowed[_random_rank(SEED, COUNTER, e, len(allowed))], e
    return flags


@pytest.mark.parametrize("eps", [0.0, 0.5, 1.0])
def test_er20_several_graphs_per_block(eps):
    """ER-20 x 64: several graphs per workgroup.  epsilon 0.5 must give blocks whose graphs all explore (skipped) and
    mixed blocks (forward run for all their graphs); 0 none that skips; 1 only skipped blocks."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 20, 64
    store = GraphStore.random("ER", B, n, 0.15, seed=20)
    assert _route(store, B) == _lib.ECO_ROUTE_DENSE3
    gpb = graphs_per_block(n, B)
    assert gpb > 1
    res = _on_off(store, B, eps)
    flags = _check_explorers(res, n, eps)
    blocks = [flags[b:b + gpb] for b in range(0, B, gpb)]
    n_all = sum(bool(f.all()) for f in blocks)
    n_mixed = sum(bool(f.any() and not f.all()) for f in blocks)
    print(f"gpb {gpb}: {len(blocks)} blocks, {n_all} all-explore, {n_mixed} mixed, {int(flags.sum())} exploring episodes")
    if eps == 0.5:
        assert n_all >= 1 and n_mixed >= 1, (gpb, n_all, n_mixed)
    elif eps == 0.0:
        assert not flags.any()
    else:
        assert n_all == len(blocks)


@pytest.mark.parametrize("eps", [0.5, 1.0])
def test_er200_one_graph_per_block(eps):
    """ER-200 x 16, the flagship shape: one graph per workgroup on the prepared-bitmask dense kernel."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 200, 16
    store = GraphStore.random("ER", B, n, 0.15, seed=200)
    assert _route(store, B) == _lib.ECO_ROUTE_DENSE3 and graphs_per_block(n, B) == 1
    flags = _check_explorers(_on_off(store, B, eps), n, eps)
    print(f"{int(flags.sum())} of {B} episodes explore")
    assert flags.all() if eps == 1.0 else (flags.any() and not flags.all())


@pytest.mark.parametrize("n", [208, 224])
@pytest.mark.parametrize("eps", [0.5, 1.0])
def test_dense_block_size_edges(n, eps):
    """ER-208 and ER-224 x 8: the first one-graph block size and the dense path's last."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    B = 8
    store = GraphStore.random("ER", B, n, 0.1, seed=n)
    assert _route(store, B) == _lib.ECO_ROUTE_DENSE3
    flags = _check_explorers(_on_off(store, B, eps), n, eps)
    assert flags.all() if eps == 1.0 else (flags.any() and not flags.all())


def test_ba240_dl_kernel():
    """BA-240 x 8 at epsilon 1: one graph of 224 < N <= 512 per workgroup (eco_mpnn_dl.h)."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 240, 8
    store = GraphStore.random("BA", B, n, 4, seed=240)
    assert _route(store, B) == _lib.ECO_ROUTE_DL
    assert _check_explorers(_on_off(store, B, 1.0), n, 1.0).all()


@pytest.mark.parametrize("eps", [0.5, 1.0])
def test_er520_large_kernel(eps):
    """ER-520 x 8 on distinct graphs: the per-episode global-memory kernel above 512 vertices."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 520, 8
    store = GraphStore.random("ER", B, n, 0.02, seed=520)
    assert _route(store, B) == _lib.ECO_ROUTE_LARGE
    flags = _check_explorers(_on_off(store, B, eps), n, eps)
    assert flags.all() if eps == 1.0 else (flags.any() and not flags.all())


@pytest.mark.parametrize("mask_name", ["NO_DENSE", "DENSE2_FWD"])
def test_er20_other_families(mask_name):
    """The same ER-20 x 64 act at epsilon 0.5 on the CSR-gather kernels (shared readout) and the 16-wave dense ones."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 20, 64
    store = GraphStore.random("ER", B, n, 0.15, seed=20)
    flags = _check_explorers(_on_off(store, B, 0.5, family_bit=getattr(_lib, "ECO_PATH_" + mask_name)), n, 0.5)
    assert flags.any() and not flags.all()


def test_irreversible_spins_allowed_vertices():
    """Irreversible spins (allowed: feature 0 == -1) at epsilon 1, ER-20 x 64.  Episode 0 has every vertex flipped:
    n_allowed == 0 keeps it greedy, its block runs the forward, and its action is 0 (the argmax of an all-masked
    row).  Episode 1 has exactly one allowed vertex, which every draw must pick."""
    from eco_hip import _lib
    from eco_hip.graphs import GraphStore
    n, B = 20, 64
    store = GraphStore.random("ER", B, n, 0.15, seed=21)
    rng = np.random.default_rng(7)
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    spins[0, :] = 1
    spins[1, :] = 1
    spins[1, 13] = -1
    spins[2:, 0] = -1       # every other episode keeps an allowed vertex
    res = _on_off(store, B, 1.0, reversible=False, spins=spins)
    np.testing.assert_array_equal(res["x0"][:, :, 0], spins.astype(np.float32))
    flags = _check_explorers(res, n, 1.0, reversible=False)
    assert not flags[0] and flags[1:].all()
    assert res["actions"][0] == 0 and res["actions"][1] == 13
    assert (spins[np.arange(1, B), res["actions"][1:]] == -1).all()    # only allowed vertices


def test_q_output_is_never_skipped():
    """A launch that also writes Q runs every forward at epsilon 1: Q is complete and bitwise the skip-off Q."""
    from eco_hip.graphs import GraphStore
    n, B = 20, 64
    store = GraphStore.random("ER", B, n, 0.15, seed=20)
    res = _on_off(store, B, 1.0, want_q=True)
    assert np.isfinite(res["q"]).all()
    ref = _act_and_step(store, B, 0.0, False, want_q=True)
    np.testing.assert_array_equal(res["q"].view(np.uint32), ref["q"].view(np.uint32))   # the forward's own Q
    assert _check_explorers(res, n, 1.0).all()


def test_vector_steps_advance_the_counter_alike():
    """5 x DQN.vector_step at ER-20, epsilon 0.5, with and without the skip: the same action sequence (each act call
    draws under its own counter) and the same env state at the end."""
    from eco_hip import _lib
    from eco_hip.agents.dqn.dqn import DQN
    from eco_hip.graphs import GraphStore
    from eco_hip.networks.mpnn import MPNN
    n, B = 20, 64
    runs = {}
    for skip in (True, False):
        store = GraphStore.random("ER", 256, n, 0.15, seed=22)
        agent = DQN(_env(store, B), lambda: MPNN(device="cuda"), init_weight_std=0.1, double_dqn=True,
                    clip_Q_targets=False, replay_start_size=500, replay_buffer_size=4096, gamma=0.95,
                    update_target_frequency=1000, update_learning_rate=False, initial_learning_rate=1e-4,
                    peak_learning_rate=1e-4, final_learning_rate=1e-4, update_frequency=32, minibatch_size=64,
                    final_exploration_rate=0.05, final_exploration_step=150000, adam_epsilon=1e-8, seed=3,
                    evaluate=False, test_save_path=None)
        agent.start()
        agent.epsilon = 0.5
        seq, c0 = [], agent._act_counter
        with _lib.kernel_paths(0 if skip else _lib.ECO_PATH_NO_ACT_SKIP):
            for _ in range(5):
                agent.vector_step(True)
                seq.append(agent._actions.cpu().numpy().copy())
        torch.cuda.synchronize()
        assert agent._act_counter == c0 + 5
        runs[skip] = (np.stack(seq), agent.env.state.cpu().numpy(), agent.env.obs_x.cpu().numpy())
    for a, b in zip(runs[True], runs[False]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert len({s.tobytes() for s in runs[True][0]}) == 5     # five different draws
