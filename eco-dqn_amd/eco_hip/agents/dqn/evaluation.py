"""DQN.evaluate_agent (dqn.py:514-602) on the HIP engine: greedy rollouts of the agent's test episodes on a
test VecSpinSystem.  Three ways to run one evaluation, all with the same resets, predictions and steps:
the refill loop (any env), the one-fill rollout with no host synchronisation (every test episode fits the
slots at once and ends exactly at max_steps; replayed from a HIP graph from the second evaluation on), and
that rollout on a side stream on a snapshot of the weights while training goes on (learn()).

The Evaluator reads test_envs, test_episodes, test_metric, eval_graphs and overlap_evaluation from the agent
at call time (callers reassign them between calls) and writes agent.last_evaluation."""
from dataclasses import dataclass

import numpy as np
import torch

from ... import _lib
from .utils import TestMetric


@dataclass
class Launched:
    """A one-fill evaluation whose launches are issued: its results land in pinned memory (`st`, `cum`) behind
    `done` (None: issued on the current stream, Evaluator.finish records the event itself)."""
    env: object
    k: int
    cum: torch.Tensor
    st: dict
    metric: TestMetric
    done: object = None


def final_solution(env, st, i):
    """scorer.get_solution of the episode's current spins (score_solver.py:263-271, 377-381,
    463-467, 537-544, 649-656, 776-783) from the env's integer state."""
    t = env.cfg.optimisation_target
    score, lb, qn = float(st["score"][i]), float(st["lower_bound"][i]), float(st["quality_normalizer"][i])
    invalid = float(st["invalidity"][i]) != 0
    size = float(st["set_size"][i])
    if t == _lib.ECO_TARGET_CUT:
        return score - abs(min(0.0, lb))
    if t == _lib.ECO_TARGET_MIN_CUT:
        return max(0.0, qn) - score
    if t in (_lib.ECO_TARGET_MIN_COVER, _lib.ECO_TARGET_MIN_DOM_SET):
        return float(env.n_spins) if invalid else size
    return 0.0 if invalid else size


def episode_result(metric, env, st, cum, i):
    """(score, solution) of the finished episode in slot i under `metric` (dqn.py:560-583); st: the env's scalar
    fields, cum: the cumulative rewards."""
    if metric == TestMetric.BEST:
        return float(st["best_score"][i]), float(st["best_solution"][i])
    if metric == TestMetric.FINAL:
        return float(st["score"][i]), final_solution(env, st, i)
    if metric == TestMetric.CUMULATIVE_REWARD:
        return float(cum[i]), 0.0
    return 0.0, 0.0


def rollout_key(env, act_cfg, net, k, keep_cum):
    """Everything the captured rollout's kernel arguments depend on: the buffers' device addresses (a
    reallocated workspace or feature buffer needs a new capture) and the act / env configuration."""
    ws = net._workspace(env.n_spins, k)
    ptrs = tuple(int(t.data_ptr()) if t is not None else 0 for t in
                 (env.obs_x, env.obs_f64, env.state, env.rewards, env.dones, env.graph_ids, net.packed, ws))
    return (ptrs, bytes(env.graphs.gs), bytes(env.cfg), env.n_envs, k, keep_cum, float(act_cfg.epsilon),
            int(act_cfg.reversible), float(act_cfg.allowed_value), int(act_cfg.seed))


def rollout(env, act_cfg, net, k, rec):
    """The one-fill evaluation's max_steps greedy steps: forward + fused greedy act over the k episodes, then
    the env step of every slot (dqn.py:536-558 without the host round trips)."""
    acts, cum = rec["acts"], rec["cum"]
    sub = acts[:k]
    scope = _lib.ECO_NORM_PER_CALL  # the batch obs_x[:k] never changes: its max degree once, then reused
    for _ in range(env.max_steps):
        net.forward_graphs(env.obs_x[:k], env.graphs, env.graph_ids[:k], norm_scope=scope,
                           act=act_cfg, actions_out=sub)
        _, rew, _ = env.step(acts)
        scope = _lib.ECO_NORM_PER_CALL_REUSE
        if rec["keep_cum"]:  # only the cumulative-reward metric reads it: one elementwise launch fewer per step
            cum += rew


class Evaluator:
    def __init__(self, agent):
        self.agent = agent
        self.net = None       # the snapshot network of overlapped evaluations
        self.stream = None    # their side stream
        self.rollouts = {}    # (id(env), id(net)) -> rollout record

    def test_env(self, test_env=None, batch_size=None):
        """The test VecSpinSystem; its `_eval_next_graph` (the next test graph, continuing across evaluations)
        starts at 0."""
        a = self.agent
        env = test_env or a.test_envs
        if env is None:
            # dqn.py:225-227: test on the training environment(s) -- here a separate batch of episodes
            # over the training graph pool (the training episodes keep running untouched)
            from ...envs.batched import VecSpinSystem
            env = a.test_envs = VecSpinSystem(a.graphs, max(1, int(batch_size or a.minibatch_size)),
                                              a.env.max_steps, **a.env.env_args)
        if isinstance(env, (list, tuple)):
            env = env[0]
        if not hasattr(env, "_eval_next_graph"):
            env._eval_next_graph = 0
        return env

    def act_config(self, env):
        """The greedy act configuration on `env` (which may differ from the training env in reversibility)."""
        cfg = self.agent._act_config(0.0)
        cfg.reversible = int(env.reversible_spins)
        cfg.allowed_value = float(env.allowed_action_value())
        return cfg

    def one_fill_ok(self, env, batch_size):
        """Every test episode fits the slots at once and ends exactly at max_steps (reversible spins,
        Stopping.NORMAL, spinsystem.py:539-554)."""
        slots = min(int(batch_size or self.agent.minibatch_size), env.n_envs)
        return self.agent.test_episodes <= slots and env.reversible_spins and env.cfg.stopping == 1

    def overlap_ok(self, env):
        """learn() overlaps an evaluation with training (side stream, weight snapshot) when it takes the one-fill
        path, the test env runs on the default stream (its kernels are then ordered by the side stream alone), and
        training cannot rewrite the test env's graphs meanwhile (regenerate_graphs on the store the test env reads,
        i.e. test_envs=None): otherwise the evaluation runs synchronously."""
        a = self.agent
        if not (a.overlap_evaluation and self.one_fill_ok(env, None)):
            return False
        if getattr(env, "stream", None) is not None:
            return False
        return not (a.regenerate_graphs is not None and env.graphs is a.graphs)

    def result(self, metric, scores, solutions):
        """An evaluation's return value from its episodes' results (listed in completion order)."""
        if metric == TestMetric.ENERGY_ERROR:
            print("\n{}/{} graphs solved optimally".format(np.count_nonzero(np.array(scores) == 0),
                                                          self.agent.test_episodes), end="")
        self.agent.last_evaluation = (scores, solutions)
        return float(np.mean(scores)), float(np.mean(solutions))

    @torch.no_grad()
    def evaluate(self, batch_size=None, test_env=None):
        """DQN.evaluate_agent."""
        a = self.agent
        env = self.test_env(test_env, batch_size)
        slots = min(int(batch_size or a.minibatch_size), env.n_envs)
        dev = a.device
        act_cfg = self.act_config(env)
        if self.one_fill_ok(env, batch_size):
            return self.finish(self.launch(env, act_cfg, a.network))
        n_graphs = env.graphs.n_graphs
        # every slot holds a valid episode (unused ones run to their end and stay masked)
        env.reset(graph_ids=np.arange(env.n_envs) % n_graphs, seed=a.eval_seed)
        active = torch.zeros(env.n_envs, dtype=torch.bool, device=dev)
        cum = torch.zeros(env.n_envs, dtype=torch.float64, device=dev)
        acts = torch.zeros(env.n_envs, dtype=torch.int32, device=dev)
        scores, solutions = [], []
        started = 0
        metric = a.test_metric
        while len(scores) < a.test_episodes:
            free = (~active[:slots]).nonzero().flatten().cpu().numpy()
            take = free[:max(0, a.test_episodes - started)]
            if len(take):
                mask = np.zeros(env.n_envs, dtype=np.uint8)
                mask[take] = 1
                gids = np.zeros(env.n_envs, dtype=np.int64)
                gids[take] = (env._eval_next_graph + np.arange(len(take))) % n_graphs
                env._eval_next_graph = (env._eval_next_graph + len(take)) % n_graphs
                env.reset(graph_ids=gids, mask=mask, seed=a.eval_seed + started)
                active[torch.as_tensor(take, device=dev)] = True
                cum[torch.as_tensor(take, device=dev)] = 0.0
                started += len(take)
            idx = active.nonzero().flatten()
            act_cfg.counter = 0
            if len(idx) == env.n_envs:
                a.network.forward_graphs(env.obs_x, env.graphs, env.graph_ids, norm_scope=_lib.ECO_NORM_PER_CALL,
                                         act=act_cfg, actions_out=acts)
            else:
                sub = torch.empty(len(idx), dtype=torch.int32, device=dev)
                a.network.forward_graphs(env.obs_x[idx].contiguous(), env.graphs, env.graph_ids[idx],
                                         norm_scope=_lib.ECO_NORM_PER_CALL, act=act_cfg, actions_out=sub)
                acts.zero_()
                acts[idx] = sub
            _, rew, done = env.step(acts)
            cum[active] += rew[active]
            fin = active & done.bool()
            if bool(fin.any()):
                st = env.read()
                for i in fin.nonzero().flatten().cpu().tolist():
                    sc, so = episode_result(metric, env, st, cum, i)
                    scores.append(sc)
                    solutions.append(so)
                active &= ~fin
        return self.result(metric, scores, solutions)  # per episode, in completion order

    def launch(self, env, act_cfg, net):
        """evaluate() when every test episode fits the slots at once (the reference's 50 ER-200 test graphs
        in 64 slots) and every episode ends exactly at max_steps: the same resets, predictions and steps as the
        refill loop, issued with no host synchronisation (on the current stream).  The k episodes take slots
        0..k-1, so each prediction's batch (its norm.max() coupling, dqn.py:546-547) is the contiguous prefix
        obs_x[:k] -- all of them are active until the last step, as in the refill loop."""
        a = self.agent
        k = a.test_episodes
        n_graphs = env.graphs.n_graphs
        keep_cum = a.test_metric == TestMetric.CUMULATIVE_REWARD
        act_cfg.counter = 0
        net._ensure_packed()
        rec = self.rollout_record(env, act_cfg, net, k, keep_cum)
        # the resets' graph ids and mask are formed on the device (no host upload, no synchronisation): every slot
        # holds a valid episode (unused ones run to their end and stay masked), as evaluate(), then slots
        # 0..k-1 take the next k test graphs
        env.reset(graph_ids=rec["slot"] % n_graphs, seed=a.eval_seed)
        env.reset(graph_ids=(rec["slot"] + env._eval_next_graph) % n_graphs, mask=rec["mask"], seed=a.eval_seed)
        env._eval_next_graph = (env._eval_next_graph + k) % n_graphs
        if keep_cum:
            rec["cum"].zero_()
        if rec["graph"] is not None:
            rec["graph"].replay()
        else:
            rollout(env, act_cfg, net, k, rec)
            rec["eager_runs"] += 1
            if a.eval_graphs and net.timer is None:
                self.capture(env, act_cfg, net, k, rec)
        env.read()
        # the results into pinned host memory behind the rollout (read by finish() once the stream's event has
        # fired: no device read on the training stream)
        rec["host_scalars"].copy_(env.scalars, non_blocking=True)
        if keep_cum:
            rec["host_cum"].copy_(rec["cum"], non_blocking=True)
        return Launched(env=env, k=k, cum=rec["host_cum"], st=env.scalar_fields(rec["host_scalars"]),
                        metric=a.test_metric)

    def rollout_record(self, env, act_cfg, net, k, keep_cum):
        """The (env, network) pair's rollout record: persistent action / cumulative-reward buffers, pinned result
        buffers and, from the second evaluation on, the HIP graph of the rollout's 2 x max_steps launches.  The
        record holds the env and the network (so every address the graph names stays allocated); a changed key
        drops the old graph."""
        key = rollout_key(env, act_cfg, net, k, keep_cum)
        pair = (id(env), id(net))
        rec = self.rollouts.get(pair)
        if rec is None or rec["key"] != key:
            dev = self.agent.device
            slot = torch.arange(env.n_envs, dtype=torch.int32, device=dev)
            rec = {"key": key, "env": env, "net": net, "graph": None, "eager_runs": 0, "keep_cum": keep_cum,
                   "acts": torch.zeros(env.n_envs, dtype=torch.int32, device=dev),
                   "cum": torch.zeros(env.n_envs, dtype=torch.float64, device=dev),
                   "slot": slot, "mask": (slot < k).to(torch.uint8),
                   "host_scalars": torch.zeros(env.scalars.shape, dtype=torch.float64).pin_memory(),
                   "host_cum": torch.zeros(env.n_envs, dtype=torch.float64).pin_memory()}
            self.rollouts[pair] = rec
        return rec

    def capture(self, env, act_cfg, net, k, rec):
        """Capture the rollout (2 x max_steps launches) into a HIP graph, replayed by the next evaluations of this
        (env, network) pair: one graph launch instead of ~800 host launches of ~20-30 us each, which otherwise
        leave the training stream without queued work while an overlapped evaluation is issued.  Captured after an
        eager run (workspaces allocated, kernels loaded); the capture itself executes nothing."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rollout(env, act_cfg, net, k, rec)
        rec["graph"] = g

    def finish(self, p):
        """Scores of a launched one-fill evaluation, listed in completion order (end step, then slot), as the
        refill loop appends them."""
        if p.done is None:  # a synchronous evaluation: its copies were issued on the current stream
            p.done = torch.cuda.Event()
            p.done.record()
        p.done.synchronize()  # the host copies have landed (the side stream's work only)
        ends = p.st["current_step"][:p.k].numpy()
        order = np.lexsort((np.arange(p.k), ends))
        scores, solutions = [], []
        for i in order.tolist():
            sc, so = episode_result(p.metric, p.env, p.st, p.cum, i)
            scores.append(sc)
            solutions.append(so)
        return self.result(p.metric, scores, solutions)

    @torch.no_grad()
    def evaluate_overlapped(self, tk):
        """learn()'s evaluation at timestep tk without stopping training: the online weights are copied into a
        snapshot network on the training stream, and the one-fill evaluation runs on a side stream that waits
        for that copy only; training kernels keep going.  The evaluation's kernels and inputs are those of
        evaluate() at tk, so its scores are identical; learn() records them (and saves the snapshot as
        `_best`) once the side stream's completion event has fired, or at the next evaluation / the end."""
        a = self.agent
        if self.net is None:
            self.net = a._network_factory()
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=a.device)
        main = torch.cuda.current_stream(a.device)
        self.net.flat.copy_(a.network.flat)
        snap = torch.cuda.Event()
        snap.record(main)
        env = self.test_env()
        act_cfg = self.act_config(env)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(snap)
            p = self.launch(env, act_cfg, self.net)
            p.done = torch.cuda.Event()
            p.done.record(self.stream)
        return p
