"""eco_env_record (one history row per episode and launch) against the reference's own Network.history
(tests/golden/solver_history.npz, teacher-forced) and against the CPU oracles replaying the GPU's own random
actions at the shapes where the kernel can go wrong.

Bars: action, spins, valid, length exact; solution, score mask and reward exact on integer graphs and at the
DESIGN.md section 14 float64 bars on the float-weighted case; Q-values within tests/test_mpnn_gpu.py's RTOL."""
import ctypes

import numpy as np
import pytest
import torch

import solver_history_common as sh
from oracle import graphs as og
from weighted_common import Bars

pytestmark = pytest.mark.gpu
RTOL = 5e-7   # tests/test_mpnn_gpu.py


def _env(Js, B, T, target, mode="eco", basis="SIGNED", graph_ids=None, spins=None):
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    store = GraphStore.from_dense([np.asarray(J, dtype=np.float64) for J in Js])
    env = VecSpinSystem(store, B, T, **sh.env_kwargs(target, mode, basis, Js[0].shape[0]))
    gids = np.arange(B) % len(Js) if graph_ids is None else graph_ids
    # twice: the reference env is constructed (one reset) and then reset, so the first observation already
    # carries the graph's invalidity normaliser
    env.reset(graph_ids=gids, spins=spins)
    env.reset(graph_ids=gids, spins=spins)
    return env, store


@pytest.mark.parametrize("ci", range(9))
def test_teacher_forced_history_matches_reference(ci):
    from eco_hip import _lib
    from eco_hip.envs.history import History
    from eco_hip.networks.mpnn import MPNN
    c = sh.case(ci)
    n, T, L = c["J"].shape[0], c["T"], len(c["action"])
    env, store = _env([c["J"]], 1, T, c["target"], c["mode"], c["basis"], spins=c["init_spins"][None].astype(np.int64))
    net = MPNN(n_obs_in=c["n_obs_in"], device="cuda")
    net.load_state_dict(sh.weights(c["n_obs_in"]))
    hist = History(env, T + 1)
    hist.record(0)
    q = torch.zeros(1, n, dtype=torch.float32, device="cuda")
    fused = torch.zeros(1, dtype=torch.int32, device="cuda")
    act = _lib.ActConfig(0.0, int(env.reversible_spins), env.allowed_action_value(), 0, 0)
    fused_all = []
    for t in range(1, L):
        net.forward_graphs(env.obs_x, store, env.graph_ids, q_out=q, act=act, actions_out=fused)
        fused_all.append(int(fused[0]))
        a = torch.tensor([int(c["action"][t])], dtype=torch.int32, device="cuda")
        skip = env.dones.clone()
        _, rew, _ = env.step(a)
        hist.record(t, skip=skip, actions=a, rewards=rew, q=q)
    env.check_errors()
    assert int(hist.length[0]) == L
    got = {k: getattr(hist, k)[:L, 0].cpu().numpy() for k in sh.FIELDS}
    np.testing.assert_array_equal(fused_all, c["action"][1:].astype(np.int64))   # the margin condition's promise
    np.testing.assert_array_equal(got["action"], c["action"])
    np.testing.assert_array_equal(got["spins"], c["spins"])
    np.testing.assert_array_equal(got["valid"].astype(bool), c["valid"])
    if ci == 8:   # EdgeType.RANDOM
        o = sh.make_oracle(c["J"], T, c["target"], c["mode"], c["basis"], c["init_spins"])
        b = Bars(c["J"], o.scorer.mlr, o.scorer.qn)
        for t in range(L):
            e = (np.abs(got["score_mask"][t] - c["score_mask"][t]).max() / (b.field(t) * b.mlr),
                 abs(got["solution"][t] - c["solution"][t]) / b.score(t),
                 abs(got["reward"][t] - c["reward"][t]) / (b.score(t) / b.qn))
            assert max(e) <= 1.0, (t, e)
    else:
        for k in ("solution", "score_mask", "reward"):
            np.testing.assert_array_equal(got[k], c[k], err_msg=k)
    err = np.abs(got["qs"].astype(np.float64) - c["qs"]) / (1 + np.abs(c["qs"]))
    print(f"case {ci}: max scaled q err {err.max():.3e} (bar {RTOL:.0e})")
    assert err.max() <= RTOL
    assert not hist.qs[0].any()
    # to_records: the reference's nesting
    recs = hist.to_records(0)
    assert len(recs) == L and all(len(r) == 7 for r in recs)
    assert recs[3][0] == c["action"][3] and recs[3][4] == list(c["spins"][3]) and recs[3][6] == bool(c["valid"][3])
    assert recs[0][3] == [0] * n and isinstance(recs[3][5], list) and len(recs[3][5]) == n


def _hub(n):
    J = np.zeros((n, n))
    J[0, 1:] = J[1:, 0] = 1
    J[1, 2] = J[2, 1] = 1
    return J


SHAPES = [  # (id, target, n, B, graph kind, steps)
    ("n65_cut", "CUT", 65, 3, "er", 6), ("n130_cover", "MIN_COVER", 130, 3, "er", 6),
    ("n130_clique", "MAX_CLIQUE", 130, 3, "er", 6), ("n65_mis", "MAX_IND_SET", 65, 3, "er", 6),
    ("n65_mincut", "MIN_CUT", 65, 3, "er", 6),
    ("n513_cut", "CUT", 513, 3, "er", 6), ("n513_mds", "MIN_DOM_SET", 513, 3, "er", 6),
    ("n2048_cut", "CUT", 2048, 3, "er", 6), ("n2048_mds", "MIN_DOM_SET", 2048, 3, "er", 6),
    ("b5_mds", "MIN_DOM_SET", 40, 5, "er", 8), ("hub_mds", "MIN_DOM_SET", 70, 2, "hub", 8),
]


@pytest.mark.parametrize("tag,target,n,B,kind,steps", SHAPES, ids=[s[0] for s in SHAPES])
def test_random_actions_match_oracle(tag, target, n, B, kind, steps):
    """Exact on the GPU's own random actions: lanes past N in the last 64-group (65, 130), the above-512
    layout (513, 2048), a partly filled last workgroup (B = 5), a hub vertex adjacent to all others."""
    from eco_hip.envs.history import History
    rng = np.random.default_rng(n * 7 + B)
    w = "discrete" if target in ("CUT", "MIN_CUT") else "uniform"
    Js = [_hub(n)] if kind == "hub" else [og.er_graph(n, min(0.3, 6.0 / n), rng, w) for _ in range(min(B, 2))]
    T = 2 * n
    spins = 2 * rng.integers(0, 2, (B, n)) - 1
    env, store = _env(Js, B, T, target, spins=spins)
    hist = History(env, steps + 1, record_qs=False)
    hist.record(0)
    gen = torch.Generator(device="cuda").manual_seed(n + B)
    acts = []
    for t in range(1, steps + 1):
        a = torch.randint(0, n, (B,), generator=gen, device="cuda", dtype=torch.int32)
        if kind == "hub" and t in (1, 3):
            a[0] = 0   # flip the hub itself
        acts.append(a.cpu().numpy())
        skip = env.dones.clone()
        _, rew, _ = env.step(a)
        hist.record(t, skip=skip, actions=a, rewards=rew)
    env.check_errors()
    acts = np.array(acts)
    assert (hist.length.cpu().numpy() == steps + 1).all()
    got = {k: getattr(hist, k).cpu().numpy() for k in sh.FIELDS if k != "qs"}
    for e in range(B):
        r = sh.replay(Js[e % len(Js)], T, target, "eco", "SIGNED", spins[e], acts[:, e])
        for k in got:
            np.testing.assert_array_equal(got[k][:, e].astype(np.float64), np.asarray(r[k], dtype=np.float64),
                                          err_msg=f"{tag} episode {e} {k}")


def test_skip_null_fields_and_sentinels():
    """Skipped episodes keep the sentinel in every row and in `length`; NULL fields are not written; rows past
    length[e] keep the sentinel."""
    from eco_hip.envs.history import History
    n, B, T = 20, 5, 40
    rng = np.random.default_rng(3)
    Js = [og.er_graph(n, 0.25, rng, "uniform")]
    env, _ = _env(Js, B, T, "MIN_COVER", spins=2 * rng.integers(0, 2, (B, n)) - 1)
    hist = History(env, 4, record_solution=False)
    assert hist.solution is None and hist.hist.solution is None and hist.score is None
    names = ("action", "reward", "qs", "spins", "score_mask", "valid", "length")
    for k in names:
        getattr(hist, k).fill_(77)
    skip = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8, device="cuda")
    hist.record(0, skip=skip)
    a = torch.arange(B, dtype=torch.int32, device="cuda")
    _, rew, _ = env.step(a)
    q = torch.rand(B, n, device="cuda")
    hist.record(1, skip=skip, actions=a, rewards=rew, q=q)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.length.cpu().numpy(), [2, 77, 2, 2, 77])
    for k in names[:-1]:
        t = getattr(hist, k).cpu().numpy().astype(np.float64)
        assert (t[:, [1, 4]] == 77).all(), k          # skipped episodes: untouched
        assert (t[2:] == 77).all(), k                 # rows past length: untouched
        assert not (t[:2][:, [0, 2, 3]] == 77).all(), k
    np.testing.assert_array_equal(hist.qs[1, [0, 2, 3]].cpu().numpy(), q[[0, 2, 3]].cpu().numpy())
    np.testing.assert_array_equal(hist.action[1, [0, 2, 3]].cpu().numpy(), [0., 2., 3.])
    assert not hist.qs[0, 0].any() and float(hist.action[0, 0]) == 0.0 and float(hist.reward[0, 2]) == 0.0
    recs = hist.to_records(0)   # record_solution=False drops element 1
    assert len(recs) == 2 and len(recs[1]) == 6 and recs[1][1] == float(rew[0])


def test_argument_errors_raise_value_error():
    from eco_hip import _lib
    from eco_hip.envs.history import History
    from eco_hip.graphs import GraphStore
    n, B, T = 20, 2, 40
    rng = np.random.default_rng(4)
    env, _ = _env([og.er_graph(n, 0.25, rng, "discrete")], B, T, "CUT", spins=2 * rng.integers(0, 2, (B, n)) - 1)
    hist = History(env, 3)
    for row in (-1, 3):
        with pytest.raises(ValueError):
            hist.record(row)

    def call(cfg, gs, batch, h):
        return _lib.lib.eco_env_record(ctypes.byref(cfg), ctypes.byref(gs), _lib.ptr(env.state), batch, 0, None, None,
                                       None, None, h, env._s())
    with pytest.raises(ValueError):
        _lib.check(call(env.cfg, env.graphs.gs, B, None))                       # NULL hist
    with pytest.raises(ValueError):
        _lib.check(call(env.cfg, env.graphs.gs, 0, ctypes.byref(hist.hist)))    # B < 1
    m = np.zeros((n, n))
    m[0, 1] = m[1, 0] = 0.37
    fstore = GraphStore.from_dense([m])
    assert fstore.float_weights
    cfg = _lib.EnvConfig.from_buffer_copy(env.cfg)
    cfg.optimisation_target = _lib.ECO_TARGET_MIN_COVER
    with pytest.raises(ValueError):
        _lib.check(call(cfg, fstore.gs, B, ctypes.byref(hist.hist)))            # float weights, non-CUT target
    hist.record(0)                                                              # and a valid call still goes through
    torch.cuda.synchronize()
    assert (hist.length.cpu().numpy() == 1).all()
