"""Generate tests/golden/dqn_step_huber_clip*.npz by running the REFERENCE's own DQN.train_step with
loss="huber" (dqn.py:172) and max_grad_norm (dqn.py:446-447).

Run in the build container only (needs the reference tree; never on the GPU box):
    python tests/golden/make_huber_clip_golden.py
The reference is imported exactly as make_golden.py imports it; the fixture is data only: inputs and the
reference's outputs.

Three consecutive train steps on ER-20 transitions (M = 16, drawn as make_dqn_step draws them) for agents that
start from the same online and target weights and see the same transitions:
  huber/       loss="huber", max_grad_norm=None
  clip/        loss="huber", max_grad_norm=c
  clip_wide/   only if no single c had a clipped and an unclipped step: loss="huber", a large c that never clips
Per step: the loss and the weights after it; for the clipped agents also the value clip_grad_norm_ returned
(`norm`), and for their first step the gradient as clip_grad_norm_ left it (`s0/grad/<name>`).

Both Huber branches must be exercised.  With weights of std 0.01 every Q is a few 1e-2, so d = q - td is the
reward to within that, and a BLS reward is either 0 or a small positive number.  The recorder therefore draws the
transitions so that 10, 8 and 6 of the 16 samples of steps 0, 1 and 2 carry a nonzero reward and the others a zero
reward, and multiplies every recorded reward by one factor (REWARD_TARGET / the smallest nonzero reward), which puts
every nonzero reward at >= REWARD_TARGET = 1.5.  Every linear-branch sample then has d < -1 and moves the readout
bias gradient by -1/16, which dominates the norm: about 0.625, 0.5 and 0.375 over the three steps, so one c between
them clips the first step (whose clipped gradient is recorded) and leaves the last alone.  The recorder asserts that in every step between 25 % and 75 % of the
samples have |d| >= 1, and that over the clipped agents at least one step has total_norm > c and one
total_norm < c; tests/test_huber_clip_golden_cpu.py re-asserts both from the files.

Files: dqn_step_huber_clip.npz holds everything but the weights after each step, which go to
dqn_step_huber_clip_w_<agent>.npz, one file per agent (tests/huber_clip_common.py loads them as one mapping).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (DQN, MPNN, SingleGraphGenerator, env_args, graphs, ising_env,  # noqa: E402
                         state_dict_np)

REWARD_TARGET = 1.5
N, M, STEPS, GAMMA = 20, 16, 3, 0.95
NONZERO = (10, 8, 6)   # samples with a nonzero reward (|d| >= 1) per step: 62.5 %, 50 %, 37.5 %


def draw_transitions(rng):
    """STEPS minibatches of M transitions as make_dqn_step draws them, redrawn until the first NONZERO[s] samples
    of step s carry a nonzero reward and the others a zero reward."""
    steps = []
    for s in range(STEPS):
        sts, acts, rews, nxt, dns = [], [], [], [], []
        for i in range(M):
            while True:
                Jg = graphs.er_graph(N, 0.15, rng)
                e = ising_env.make("SpinSystem", SingleGraphGenerator(Jg), 2 * N, **env_args("eco", N))
                o = e.reset(spins=2 * rng.integers(0, 2, N) - 1)
                for a in rng.integers(0, N, int(rng.integers(0, 2 * N - 1))):
                    o, _, _, _ = e.step(int(a))
                a = int(rng.integers(0, N))
                o2, r, d, _ = e.step(a)
                if (r != 0) == (i < NONZERO[s]):
                    break
            sts.append(o); acts.append([a]); rews.append([r]); nxt.append(o2); dns.append([float(d)])
        steps.append(dict(states=np.array(sts), actions=np.array(acts), rewards=np.array(rews, dtype=np.float64),
                          states_next=np.array(nxt), dones=np.array(dns, dtype=np.float32)))
    nz = np.concatenate([np.abs(s["rewards"][s["rewards"] != 0]) for s in steps])
    scale = REWARD_TARGET / nz.min()
    for s in steps:
        s["rewards"] = (s["rewards"] * scale).astype(np.float32)
    return steps, scale


def make_agent(env, max_grad_norm, w0=None, target=None):
    net_fn = lambda: MPNN(n_obs_in=7, n_layers=3, n_features=64, n_hid_readout=[], tied_weights=False)  # noqa: E731
    agent = DQN([env], net_fn, init_weight_std=0.01, double_dqn=True, clip_Q_targets=False,
                replay_start_size=10, replay_buffer_size=100, gamma=GAMMA, update_target_frequency=1000,
                update_learning_rate=False, initial_learning_rate=1e-4, peak_learning_rate=1e-4,
                final_learning_rate=1e-4, update_frequency=32, minibatch_size=M, max_grad_norm=max_grad_norm,
                weight_decay=0, update_exploration=True, initial_exploration_rate=1,
                final_exploration_rate=0.05, final_exploration_step=150000, adam_epsilon=1e-8,
                logging=False, loss="huber", save_network_frequency=10**9, network_save_path="/tmp/n.pth",
                evaluate=False, test_envs=None, test_episodes=1, test_frequency=10**9,
                test_save_path="/tmp/ts.pkl", seed=5)
    if w0 is None:
        # perturb the target net so double-DQN's argmax(online) != argmax(target) matters
        with torch.no_grad():
            for p in agent.target_network.parameters():
                p.add_(torch.randn_like(p) * 0.01)
    else:
        agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in w0.items()})
        agent.target_network.load_state_dict({k: torch.from_numpy(v) for k, v in target.items()})
    return agent


def td_errors(agent, tr):
    """d = q(s, a) - td of dqn.py:409-437 for the agent's current weights (reversible env, double DQN)."""
    states, actions, rewards, states_next, dones = tr
    with torch.no_grad():
        a_star = agent.network(states_next.float()).argmax(1, True)
        q_t = agent.target_network(states_next.float()).gather(1, a_star)
        td = rewards + (1 - dones) * GAMMA * q_t
        return (agent.network(states.float()).gather(1, actions) - td)[:, 0].numpy()


def run_agent(agent, steps, out, prefix):
    """STEPS train steps; records loss, weights, |d| >= 1 fraction, and (clipped agents) the norm that
    clip_grad_norm_ returned and the first step's clipped gradient.  Returns the norm of every step: what
    clip_grad_norm_ returned, or for an unclipped agent the norm of the gradient train_step left (for choosing c)."""
    norms = []
    real_clip = torch.nn.utils.clip_grad_norm_
    returned = []

    def spy(parameters, max_norm, *a, **kw):
        r = real_clip(parameters, max_norm, *a, **kw)
        returned.append(float(r))
        return r

    torch.nn.utils.clip_grad_norm_ = spy
    try:
        for s, st in enumerate(steps):
            tr = [torch.as_tensor(st["states"]), torch.as_tensor(st["actions"], dtype=torch.long),
                  torch.as_tensor(st["rewards"], dtype=torch.float), torch.as_tensor(st["states_next"]),
                  torch.as_tensor(st["dones"], dtype=torch.float)]
            d = td_errors(agent, tr)
            frac = float((np.abs(d) >= 1).mean())
            assert 0.25 <= frac <= 0.75, (prefix, s, frac)
            loss = agent.train_step(tr)
            if out is not None:
                out[f"{prefix}s{s}/loss"] = np.float64(loss)
                out[f"{prefix}s{s}/frac_linear"] = np.float64(frac)
                for k, v in state_dict_np(agent.network).items():
                    out[f"{prefix}s{s}/w/" + k] = v
            if agent.max_grad_norm is not None:
                assert len(returned) == s + 1
                norms.append(returned[-1])
                if out is not None:
                    out[f"{prefix}s{s}/norm"] = np.float64(returned[-1])
                    if s == 0:
                        for k, p in agent.network.named_parameters():
                            out[f"{prefix}s0/grad/" + k] = p.grad.detach().numpy().copy()
            else:
                norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum()
                                                  for p in agent.network.parameters()))))
    finally:
        torch.nn.utils.clip_grad_norm_ = real_clip
    return norms


def make_huber_clip():
    rng = np.random.default_rng(2024)
    J = graphs.er_graph(N, 0.15, rng)
    env = ising_env.make("SpinSystem", SingleGraphGenerator(J), 2 * N, **env_args("eco", N))
    steps, scale = draw_transitions(rng)
    out = {"steps": np.int64(STEPS), "reward_scale": np.float64(scale), "gamma": np.float64(GAMMA)}
    for s, st in enumerate(steps):
        for k, v in st.items():
            out[f"s{s}/{k}"] = v
    first = make_agent(env, None)
    w0, target = state_dict_np(first.network), state_dict_np(first.target_network)
    for k, v in w0.items():
        out["w0/" + k] = v
    for k, v in target.items():
        out["target/" + k] = v
    free = run_agent(first, steps, out, "huber/")
    # c between the unclipped norms, so that a clipped agent sees both sides (its first step is the unclipped one)
    lo, hi = min(free), max(free)
    c = float(np.format_float_positional(np.sqrt(lo * hi), precision=3, fractional=False))
    clipped = run_agent(make_agent(env, c, w0, target), steps, out, "clip/")
    out["clip/max_grad_norm"] = np.float64(c)
    above, below = any(v > c for v in clipped), any(v < c for v in clipped)
    if not (above and below):
        wide = 100.0 * hi
        norms = run_agent(make_agent(env, wide, w0, target), steps, out, "clip_wide/")
        out["clip_wide/max_grad_norm"] = np.float64(wide)
        above, below = above or any(v > wide for v in norms), below or any(v < wide for v in norms)
    assert above and below, (c, clipped)
    # one file per agent for the weights after each step (58,425 random floats do not compress: six sets would
    # not fit the size limit of a committed file); everything else in the main file
    sizes = {}
    for agent in sorted({k.split("/")[0] for k in out if "/w/" in k}):
        part = {k: out.pop(k) for k in [k for k in out if k.startswith(agent + "/") and "/w/" in k]}
        path = os.path.join(HERE, f"dqn_step_huber_clip_w_{agent}.npz")
        np.savez_compressed(path, **part)
        sizes[os.path.basename(path)] = os.path.getsize(path)
    path = os.path.join(HERE, "dqn_step_huber_clip.npz")
    np.savez_compressed(path, **out)
    sizes[os.path.basename(path)] = os.path.getsize(path)
    assert max(sizes.values()) < (1 << 20), sizes
    print("unclipped norms", free, "c", c, "clipped agent's norms", clipped, "bytes", sizes)


if __name__ == "__main__":
    import random
    random.seed(0)
    np.random.seed(0)
    make_huber_clip()
