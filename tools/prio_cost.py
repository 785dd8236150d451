"""Cost of the device prioritised replay against the uniform sampler, at the benched shape: compact ring, ER-200,
B = 8192 episodes, capacity B x 400 = 3,276,800 transitions (one episode's worth, bench.py build_train_agent),
minibatch M = 2048.

The ring is filled by one whole episode of random actions (400 vector steps through the wrapper, so every push also
ran eco_prio_push), priorities are then set by updates with random |td| until most positions carry their own mass.
Timed with HIP events after a warm-up, `--reps` windows of `--calls` calls each, the two samplers alternating:
  uniform     CompactReplayBuffer.sample(M)                       (eco_replay_compact_sample)
  prioritised DevicePrioritisedReplay.sample(M) + update(|td|)    (eco_prio_sample + eco_replay_compact_gather +
                                                                   eco_prio_update)
  push        eco_prio_push of B positions into the full ring     (once per vector step)
Prints one JSON line: median / min / max microseconds per call of each, their ratio, and the prioritised cost of the
8 samples + 1 push of a vector step as a share of --vector-step-ms.

    python tools/prio_cost.py [--reps 20] [--calls 500]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "eco-dqn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--minibatch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--samples-per-step", type=int, default=8)
    ap.add_argument("--vector-step-ms", type=float, default=19.19, help="the recorded vector step of the benched recipe")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prio_cost: needs the GPU (timings on anything else mean nothing)")
    from eco_hip.graphs import GraphStore
    from eco_hip.envs.batched import VecSpinSystem
    from eco_hip.envs.utils import (DEFAULT_OBSERVABLES, RewardSignal, ExtraAction, OptimisationTarget,
                                    SpinBasis)
    from eco_hip.agents.dqn.utils import CompactReplayBuffer
    from eco_hip.agents.dqn.prioritised import DevicePrioritisedReplay
    n, B, M = args.n, args.batch, args.minibatch
    T = 2 * n
    cap = B * T
    store = GraphStore.random("ER", B, n, 0.15, seed=1234, device="cuda:0")
    env = VecSpinSystem(store, B, T, observables=DEFAULT_OBSERVABLES, reward_signal=RewardSignal.BLS,
                        extra_action=ExtraAction.NONE, optimisation_target=OptimisationTarget.CUT,
                        spin_basis=SpinBasis.SIGNED, norm_rewards=True, basin_reward=1. / n)
    ring = CompactReplayBuffer(cap, env, seed=1)
    prio = DevicePrioritisedReplay(ring)
    env.reset(graph_ids=np.arange(B), seed=3)
    prio.snapshot()
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = [env.obs_x, torch.zeros_like(env.obs_x)]
    for t in range(T):
        acts = torch.randint(0, n, (B,), generator=g, device="cuda", dtype=torch.int32)
        _, rew, done = env.step(acts, obs_out=obs[(t + 1) & 1])
        prio.add_step(acts, rew, done)
    env.check_errors()
    assert len(prio) == cap
    abs_td = torch.rand(M, generator=g, device="cuda")
    for _ in range(1500):                 # spread priorities over the ring (and warm every kernel up)
        prio.sample(M)
        abs_td.uniform_(0, 1.5, generator=g)
        prio.update(abs_td)
    for _ in range(20):
        ring.sample(M)
    torch.cuda.synchronize()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.calls      # microseconds per call

    def prio_call():
        prio.sample(M)
        prio.update(abs_td)

    def push_call():
        prio._push(0, B, cap)

    times = {"uniform": [], "prioritised": [], "push": []}
    for _ in range(args.reps):
        times["uniform"].append(window(lambda: ring.sample(M)))
        times["prioritised"].append(window(prio_call))
        times["push"].append(window(push_call))
    out = {"shape": {"n_spins": n, "batch": B, "capacity": cap, "minibatch": M, "ring": "compact"},
           "reps": args.reps, "calls_per_window": args.calls, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v = np.array(v)
        out[k + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(v.min()), 2),
                          "max": round(float(v.max()), 2)}
    out["ratio_prioritised_over_uniform"] = round(out["prioritised_us"]["median"] / out["uniform_us"]["median"], 2)
    per_step = args.samples_per_step * out["prioritised_us"]["median"] + out["push_us"]["median"]
    out["prioritised_us_per_vector_step"] = round(per_step, 1)
    out["share_of_vector_step"] = round(per_step * 1e-3 / args.vector_step_ms, 4)
    out["uniform_share_of_vector_step"] = round(args.samples_per_step * out["uniform_us"]["median"] * 1e-3
                                                / args.vector_step_ms, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
