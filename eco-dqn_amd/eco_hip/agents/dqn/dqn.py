"""Batched DQN agent (src/agents/dqn/dqn.py) on the HIP engine.

Same constructor keywords and public methods as the reference DQN
(`learn`, `train_step`, `act`, `predict`, `update_epsilon`, `update_lr`,
`evaluate_agent`, `save`, `load`), but `envs` is a VecSpinSystem: every call
advances B episodes.  Everything on the step path runs in libecohip:
  act       -> MPNN forward with the fused epsilon-greedy argmax (dqn.py:453-465)
  env.step  -> batched SpinSystem kernel (spinsystem.py:355-559)
  replay    -> device ring push / distinct-index sample (dqn/utils.py:28-83)
  train     -> online(s') argmax, target(s') gather, online(s) forward with saved
               activations, TD + MSE / Huber gradient, MPNN backward, optional gradient-norm clipping,
               Adam (dqn.py:403-451); above 512 vertices online(s) is an inference forward and the
               gradient one self-contained call that recomputes it (MPNN.grad_rows; 2049 to 8192 vertices
               with train_large_graphs=True)
Schedules are per env-step as in the reference; a vector step advances the
counter by B.  The replay ratio of the reference (minibatch_size/update_frequency
samples per env-step, 64/32 = 2 in train_eco.py:136-137) is kept by running
K = B*ratio/M gradient steps of minibatch M per vector step.  Multi-GPU: one
process per GPU, episodes sharded, gradients summed over RCCL (torch.distributed)
and averaged inside the Adam kernel; parameters stay bit-identical across ranks.

This class is the training step.  The graph-slot bookkeeping of regenerate_graphs is graph_slots.GraphSlotRing,
evaluate_agent and its overlapped form are evaluation.Evaluator, and learn()'s evaluations in flight, score
all-reduces and deferred checkpoints are learn_pipeline.LearnPipeline.
"""
import ctypes
import math
import numbers
import os
import random

import numpy as np
import torch

from ... import _lib
from ...parallel import allreduce_gradients_async, broadcast_parameters
from .evaluation import Evaluator
from .graph_slots import GraphSlotRing, graph_slots_needed  # noqa: F401  (graph_slots_needed: imported from here)
from .learn_pipeline import LearnPipeline
from .prioritised import DevicePrioritisedReplay, prioritised_config
from .utils import CompactReplayBuffer, ReplayBuffer, TestMetric, set_global_seed


class DQN:
    def __init__(self, envs, network, init_network_params=None, init_weight_std=None, double_dqn=True,
                 update_target_frequency=10000, gamma=0.99, clip_Q_targets=False, replay_start_size=50000,
                 replay_buffer_size=1000000, minibatch_size=32, update_frequency=1, update_learning_rate=True,
                 initial_learning_rate=0, peak_learning_rate=1e-3, peak_learning_rate_step=10000,
                 final_learning_rate=5e-5, final_learning_rate_step=200000, max_grad_norm=None, weight_decay=0,
                 update_exploration=True, initial_exploration_rate=1, final_exploration_rate=0.1,
                 final_exploration_step=1000000, adam_epsilon=1e-8, loss="mse", save_network_frequency=10000,
                 network_save_path='network', evaluate=True, test_envs=None, test_episodes=20,
                 test_frequency=10000, test_save_path='test_scores', test_metric=TestMetric.ENERGY_ERROR,
                 logging=True, seed=None, train_minibatch=None, graph_pool_ids=None, regenerate_graphs=None,
                 compact_replay=None, target_sync="grad_steps", overlap_evaluation=True, prioritised_replay=None,
                 train_large_graphs=False):
        if isinstance(envs, (list, tuple)):
            if len(envs) != 1:
                raise NotImplementedError("pass one VecSpinSystem (it already holds B episodes)")
            envs = envs[0]
        if callable(loss):
            raise NotImplementedError("a callable loss cannot run inside the TD kernel (eco_dqn_td_loss computes the "
                                      "loss and its gradient on the device): pass 'mse' or 'huber'")
        if not isinstance(loss, str) or loss not in ("mse", "huber"):
            raise ValueError("loss must be 'huber', 'mse' or a callable")  # dqn.py:174
        if max_grad_norm is not None:
            if (isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, numbers.Real)
                    or not math.isfinite(max_grad_norm) or max_grad_norm <= 0):
                raise ValueError("max_grad_norm must be None or a finite positive number")
            max_grad_norm = float(max_grad_norm)
        if envs.graphs.n_spins > _lib.ECO_MAX_SPINS:
            # eco_mpnn_grad_large and eco_mpnn_forward_pair stop at ECO_MAX_SPINS.  train_large_graphs=True opts in to
            # the gradient of 2049 to ECO_MAX_SPINS_WG vertices (MPNN.grad_wg; MaxCut on integer weights, which is
            # what the env and the store take there); the default keeps such a store to inference and search
            if not train_large_graphs:
                raise ValueError(f"DQN trains on graphs of at most ECO_MAX_SPINS={_lib.ECO_MAX_SPINS} vertices, got N "
                                 f"= {envs.graphs.n_spins}: {_lib.ECO_MAX_SPINS} < N <= {_lib.ECO_MAX_SPINS_WG} is "
                                 "inference and search only unless train_large_graphs=True is passed")
            if regenerate_graphs is not None:
                raise ValueError(f"regenerate_graphs takes graphs of at most ECO_MAX_SPINS={_lib.ECO_MAX_SPINS} "
                                 f"vertices (the device generators are not run above it), got N = "
                                 f"{envs.graphs.n_spins}: train on a fixed pool there")
        self.loss = loss
        self._loss_kind = _lib.ECO_LOSS_HUBER if loss == "huber" else _lib.ECO_LOSS_MSE
        self.max_grad_norm = max_grad_norm
        self.env = envs
        self.graphs = envs.graphs
        self.device = envs.graphs.device
        self.double_dqn = double_dqn
        self.replay_start_size = replay_start_size
        self.replay_buffer_size = replay_buffer_size
        self.gamma = gamma
        self.clip_Q_targets = clip_Q_targets
        self.update_target_frequency = update_target_frequency
        self.minibatch_size = minibatch_size
        self.update_learning_rate = update_learning_rate
        self.initial_learning_rate = initial_learning_rate
        self.peak_learning_rate = peak_learning_rate
        self.peak_learning_rate_step = peak_learning_rate_step
        self.final_learning_rate = final_learning_rate
        self.final_learning_rate_step = final_learning_rate_step
        self.weight_decay = weight_decay
        self.update_frequency = update_frequency
        # dqn.py:161 stores a one-tuple (`self.update_exploration = update_exploration,`), which is always
        # truthy: the reference decays epsilon whatever is passed, and so does this class
        self.update_exploration = update_exploration,
        self.initial_exploration_rate = initial_exploration_rate
        self.epsilon = initial_exploration_rate
        self.final_exploration_rate = final_exploration_rate
        self.final_exploration_step = final_exploration_step
        self.adam_epsilon = adam_epsilon
        self.lr = initial_learning_rate
        self.logging = logging
        self.seed = random.randint(0, 10 ** 6) if seed is None else seed
        set_global_seed(self.seed)
        self.acting_in_reversible_spin_env = envs.reversible_spins
        self.allowed_value = envs.allowed_action_value()

        self.network = network()
        self.target_network = network()
        self._network_factory = network
        if init_network_params is not None:
            self.load(init_network_params)
        elif init_weight_std is not None:
            self.network.init_normal_(init_weight_std, generator=torch.Generator().manual_seed(self.seed))
        self.dist = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.world = torch.distributed.get_world_size() if self.dist else 1
        broadcast_parameters(self.network.flat)  # every rank starts from rank 0's weights
        # evaluations use rank 0's seed on every rank (learn() runs each evaluation of the job on one rank: its
        # episodes' initial spins must not depend on which rank that is); = seed in one process
        self.eval_seed = self.seed
        if self.dist and self.world > 1:
            t = torch.tensor([self.seed], dtype=torch.int64,
                             device=self.device if torch.distributed.get_backend() == "nccl" else "cpu")
            torch.distributed.broadcast(t, src=0)
            self.eval_seed = int(t.item())
        self.target_network.load_state_dict(self.network.state_dict())
        n = self.network.flat.numel()
        self.grad = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        # max_grad_norm: {total_norm, clip coefficient} of the last train_step, written by eco_grad_clip
        self.grad_norm = (torch.zeros(2, dtype=torch.float32, device=self.device) if max_grad_norm is not None
                          else None)
        self.adam_step = 0
        self.grad_steps = 0

        self.B = envs.n_envs
        self.N = envs.n_spins
        self.M = int(train_minibatch or minibatch_size)
        # compact replay (one integer env state per transition, 4 B per vertex) for MaxCut envs on +-1
        # graphs; else fp32 features (always for a float-weighted store: the ring's local field is an int16)
        # The set-problem targets take the compact ring (N <= ECO_MAX_SPINS) only on request: None keeps their
        # feature ring, so no existing run changes its ring.
        target = envs.cfg.optimisation_target
        set_problem = _lib.ECO_TARGET_MIN_COVER <= target <= _lib.ECO_TARGET_MIN_DOM_SET
        fits = (envs.graphs.unit_weights and not envs.graphs.float_weights and envs.max_steps < 32768)
        eligible = fits and target == _lib.ECO_TARGET_CUT and self.N <= _lib.ECO_COMPACT_MAX_SPINS
        allowed = eligible or (fits and set_problem and self.N <= _lib.ECO_MAX_SPINS)
        self.compact_replay = eligible if compact_replay is None else bool(compact_replay)
        if self.compact_replay and not allowed:
            raise ValueError("compact replay needs +-1 (integer) weights, max_steps < 32768 and OptimisationTarget.CUT "
                             f"with n_spins <= {_lib.ECO_COMPACT_MAX_SPINS}, or MIN_COVER / MIN_CUT / MAX_IND_SET / "
                             f"MAX_CLIQUE / MIN_DOM_SET with n_spins <= {_lib.ECO_MAX_SPINS}")
        if self.compact_replay:
            self.replay_buffer = CompactReplayBuffer(replay_buffer_size, envs, seed=self.seed)
        else:
            self.replay_buffer = ReplayBuffer(replay_buffer_size, self.N, device=self.device, seed=self.seed,
                                              n_obs=envs.n_obs)
        # prioritised_replay: None keeps the uniform ring above and today's train_step; a dict (alpha, beta0,
        # beta_steps, eps, td_max; prioritised.PRIORITISED_DEFAULTS for missing keys) wraps whichever ring was chosen
        # in proportional priorities on the device (prioritised.DevicePrioritisedReplay): importance-weighted TD
        # loss, priorities updated from |td| right after it, no host read
        self._prio = None
        if prioritised_replay is not None:
            self._prio = self.replay_buffer = DevicePrioritisedReplay(self.replay_buffer,
                                                                      **prioritised_config(prioritised_replay))
        self.replay_ratio = minibatch_size / float(update_frequency)
        # reference (dqn.py:332-347): one train_step every update_frequency env-steps and one target sync every
        # update_target_frequency env-steps, i.e. a sync every update_target_frequency / update_frequency gradient
        # steps.  target_sync="grad_steps" (default) keeps that count of optimiser steps between syncs whatever
        # the minibatch ("count sync in gradient steps"); "samples" syncs every
        # update_target_frequency env-steps' worth of replayed samples instead (the two agree at M = minibatch_size).
        if target_sync not in ("grad_steps", "samples"):
            raise ValueError("target_sync must be 'grad_steps' or 'samples'")
        self.target_sync = target_sync
        self.target_sync_grad_steps = max(1, int(round(update_target_frequency / float(update_frequency))))
        self.target_sync_samples = update_target_frequency * self.replay_ratio
        self._samples_since_sync = 0.0
        self.graph_pool_ids = (np.arange(self.graphs.n_graphs) if graph_pool_ids is None
                               else np.asarray(graph_pool_ids))
        # fresh graphs per episode like the reference's generators (utils.py:165-236): graph_slots.py
        self.regenerate_graphs = regenerate_graphs
        self._rng = np.random.default_rng(self.seed)
        self._pushed = 0
        self._host_graph_ids = None   # the live episodes' graph ids (_reset_env's host mirror); None: none yet
        self._slots = None
        if regenerate_graphs is not None:
            if not hasattr(self.graphs, "cap"):
                raise ValueError("regenerate_graphs needs a GraphStore.slots(...) store")
            need = graph_slots_needed(envs.n_envs, envs.max_steps, replay_buffer_size)
            if envs.reversible_spins and envs.cfg.stopping == 1 and self.graphs.n_graphs < need:
                # lockstep episodes (every one ends at max_steps): B * max_steps pushes per episode batch,
                # so ceil(capacity / (B * max_steps)) + 1 batches of B slots must rotate
                raise ValueError(f"regenerate_graphs with n_envs={envs.n_envs}, max_steps={envs.max_steps} and "
                                 f"replay_buffer_size={replay_buffer_size} needs GraphStore.slots(>= {need}, ...) "
                                 f"(has {self.graphs.n_graphs}): a slot may only be regenerated once no stored "
                                 "transition references it")
            self._slots = GraphSlotRing(self.graphs.n_graphs, replay_buffer_size, self._rng, self._regenerate)

        self.evaluate = evaluate
        self.test_envs = test_envs
        self.test_episodes = int(test_episodes)
        self.test_frequency = test_frequency
        self.test_save_path = test_save_path
        self.test_metric = test_metric
        self.save_network_frequency = save_network_frequency
        self.network_save_path = network_save_path
        # learn(): evaluations that take the one-fill path run on a side stream on a snapshot of the weights while
        # training continues (same results: the snapshot is the network at the evaluation's timestep)
        self.overlap_evaluation = overlap_evaluation
        # one-fill evaluations replay their rollout from a HIP graph captured at the second evaluation of an
        # (env, network) pair (Evaluator.capture); False keeps every evaluation's launches eager
        self.eval_graphs = True
        self._evaluator = Evaluator(self)
        # learn(): spread the B lockstep episodes over the T phases of an episode (start(); False: all B episodes
        # start together and end together every T vector steps)
        self.stagger_episodes = False

        self._act_counter = 0
        # every gradient step's loss, kept on the device (dqn.py:339); the device buffer is allocated by start()
        self._loss_buf = None
        self._loss_t = np.zeros(4096, np.int64)
        self._loss_n = 0
        self._loss_start = 0
        self._alloc_train_buffers(self.M)

    # ---------------------------------------------------------------- buffers
    def _alloc_train_buffers(self, m):
        dev = self.device
        self._wg = self.N > _lib.ECO_MAX_SPINS   # 2049 to ECO_MAX_SPINS_WG vertices: no pair forward
        if self._wg and self.network.grad_rows_bytes(self.N, m) == 0:   # before anything is reallocated
            raise ValueError(f"train_minibatch = {m} samples of N = {self.N} vertices exceed the gradient's row "
                             f"index: train_minibatch * N must be at most (2^31 - 1) / 64 = {(2 ** 31 - 1) // 64} "
                             f"(train_minibatch <= {(2 ** 31 - 1) // 64 // self.N})")
        self.q_s = torch.empty(m, self.N, device=dev)
        self.q_tn = torch.empty(m, self.N, device=dev)
        self.a_star = torch.empty(m, dtype=torch.int32, device=dev)
        self.dq = torch.empty(m, self.N, device=dev)
        self.sqerr = torch.empty(m, device=dev)
        self.loss_dev = torch.zeros(1, device=dev)
        if self._prio is not None:
            self.abs_td = torch.empty(m, device=dev)
        # above 512 vertices the gradient is one self-contained call (MPNN.grad_rows) with one workspace; there is
        # no saved-activation buffer between a forward and a backward
        self._large = self.N > _lib.MPNN_MAX_SPINS
        if self._large:
            self.saved = self.bw_ws = None
            self.grad_ws = torch.empty(self.network.grad_rows_bytes(self.N, m), dtype=torch.uint8, device=dev)
        else:
            self.saved = torch.empty(self.network.saved_bytes(self.N, m), dtype=torch.uint8, device=dev)
            self.bw_ws = torch.empty(_lib.lib.eco_mpnn_backward_workspace_bytes(self.N, m), dtype=torch.uint8,
                                     device=dev)
        self._train_m = m
        self._actions = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self._obs = [self.env.obs_x, torch.zeros_like(self.env.obs_x)]

    # -------------------------------------------------------------- schedules
    def update_epsilon(self, timestep):
        """dqn.py:467-471"""
        eps = self.initial_exploration_rate - (self.initial_exploration_rate - self.final_exploration_rate) * (
            timestep / self.final_exploration_step)
        self.epsilon = max(eps, self.final_exploration_rate)

    def update_lr(self, timestep):
        """dqn.py:473-488"""
        if timestep <= self.peak_learning_rate_step:
            lr = self.initial_learning_rate - (self.initial_learning_rate - self.peak_learning_rate) * (
                timestep / self.peak_learning_rate_step)
        elif timestep <= self.final_learning_rate_step:
            lr = self.peak_learning_rate - (self.peak_learning_rate - self.final_learning_rate) * (
                (timestep - self.peak_learning_rate_step) /
                (self.final_learning_rate_step - self.peak_learning_rate_step))
        else:
            lr = None
        if lr is not None:
            self.lr = lr

    # ------------------------------------------------------------------- act
    def _act_config(self, epsilon):
        self._act_counter += 1
        return _lib.ActConfig(float(epsilon), int(self.acting_in_reversible_spin_env), float(self.allowed_value),
                              self.seed, self._act_counter)

    def act(self, obs_x, graph_ids, is_training_ready=True, actions_out=None):
        """dqn.py:453-465 for every episode: epsilon-greedy over the MPNN (B=1 norm semantics, :282)."""
        eps = self.epsilon if is_training_ready else 1.0
        out = actions_out if actions_out is not None else torch.empty(obs_x.shape[0], dtype=torch.int32,
                                                                       device=self.device)
        self.network.forward_graphs(obs_x, self.graphs, graph_ids, norm_scope=_lib.ECO_NORM_PER_GRAPH,
                                    act=self._act_config(eps), actions_out=out)
        return out

    @torch.no_grad()
    def predict(self, obs_x, graph_ids, graphs=None, norm_scope=_lib.ECO_NORM_PER_CALL):
        """dqn.py:490-512: greedy actions (allowed vertices only for irreversible envs)."""
        out = torch.empty(obs_x.shape[0], dtype=torch.int32, device=self.device)
        self.network.forward_graphs(obs_x, graphs or self.graphs, graph_ids, norm_scope=norm_scope,
                                    act=self._act_config(0.0), actions_out=out)
        return out

    # ----------------------------------------------------------------- train
    def train_step(self, transitions, sync_loss=True, loss_out=None, overlap=None):
        """dqn.py:403-451.  transitions = (states_x, actions, rewards, states_next_x, dones, graph_ids)
        as returned by ReplayBuffer.sample.  Returns the loss: a float if sync_loss, else the one-element
        device tensor it was written to (`loss_out`, or a copy of the agent's loss slot).
        overlap: optional callable issued while the gradient all-reduce is in flight (multi-GPU): work that does
        not read the gradient or the online weights, e.g. the next minibatch's replay sample."""
        xs, act, rew, xn, done, gid = transitions
        loss_dev = self.loss_dev if loss_out is None else loss_out
        m = xs.shape[0]
        if m != self._train_m:
            self._alloc_train_buffers(m)
        net, tgt = self.network, self.target_network
        greedy = _lib.ActConfig(0.0, int(self.acting_in_reversible_spin_env), float(self.allowed_value), 0, 0)
        if self.double_dqn and self._wg:
            # eco_mpnn_forward_pair stops at ECO_MAX_SPINS: the pair is two forwards.  The online one runs second, so
            # the per-call max degree Q(s) reuses below is the one it left in its own workspace
            tgt.forward_graphs(xn, self.graphs, gid, norm_scope=_lib.ECO_NORM_PER_CALL, q_out=self.q_tn)
            net.forward_graphs(xn, self.graphs, gid, norm_scope=_lib.ECO_NORM_PER_CALL, act=greedy,
                               actions_out=self.a_star)
            scope_s = _lib.ECO_NORM_PER_CALL_REUSE
        elif self.double_dqn:
            # greedy_actions = network(s').argmax (masked for irreversible envs), q_t = target(s')[a*]
            net.forward_pair_graphs(tgt, xn, self.graphs, gid, norm_scope=_lib.ECO_NORM_PER_CALL, act=greedy,
                                    actions_out=self.a_star, q_out_other=self.q_tn)
            # same graph ids, same workspace: the per-call max degree the pair left there
            scope_s = _lib.ECO_NORM_PER_CALL_REUSE
        else:
            tgt.forward_graphs(xn, self.graphs, gid, norm_scope=_lib.ECO_NORM_PER_CALL, q_out=self.q_tn,
                               act=greedy, actions_out=self.a_star)
            scope_s = _lib.ECO_NORM_PER_CALL
        net.forward_graphs(xs, self.graphs, gid, norm_scope=scope_s, q_out=self.q_s, saved=self.saved)
        # TD error with the MSE or smooth-L1 (loss="huber", dqn.py:172) loss and its gradient
        if self._prio is None:
            _lib.check(_lib.lib.eco_dqn_td_loss(_lib.ptr(self.q_s), _lib.ptr(self.q_tn), _lib.ptr(self.a_star),
                                                _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), m, self.N,
                                                ctypes.c_float(self.gamma), int(bool(self.clip_Q_targets)),
                                                self._loss_kind, _lib.ptr(self.dq), _lib.ptr(self.sqerr),
                                                _lib.ptr(loss_dev), _lib.stream_ptr()))
        else:
            # prioritised replay: `transitions` is the buffer's last sample; its importance weights scale the loss
            # and the gradient, and its |td| become the new priorities right here, before `overlap` prefetches the
            # next minibatch: stream order makes minibatch k + 1 see minibatch k's priorities
            w = self._prio.last_weights
            if w is None or w.shape[0] != m:
                raise ValueError("prioritised replay: train_step takes the replay buffer's last sample()")
            _lib.check(_lib.lib.eco_dqn_td_weighted(_lib.ptr(self.q_s), _lib.ptr(self.q_tn), _lib.ptr(self.a_star),
                                                    _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), m, self.N,
                                                    ctypes.c_float(self.gamma), int(bool(self.clip_Q_targets)),
                                                    self._loss_kind, _lib.ptr(self.dq), _lib.ptr(self.sqerr),
                                                    _lib.ptr(loss_dev), _lib.ptr(w), _lib.ptr(self.abs_td),
                                                    _lib.stream_ptr()))
            self._prio.update(self.abs_td)
        if self._large:
            net.grad_rows(xs, self.graphs, gid, self.dq, self.grad, workspace=self.grad_ws)
        else:
            net.backward_graphs(xs, self.graphs, gid, self.saved, self.dq, self.grad, workspace=self.bw_ws)
        # RCCL sum over xGMI (233.7 KB) on the collective's stream, the mean folded into Adam; independent work
        # (the caller's `overlap`) is issued on this stream meanwhile
        work, scale = allreduce_gradients_async(self.grad)
        if overlap is not None:
            overlap()
        if work is not None:
            work.wait()
        if self.max_grad_norm is not None:
            # clip_grad_norm_ (dqn.py:446-447) on the summed gradient: `scale` (1/world) enters the norm only, so the
            # norm is the mean gradient's and Adam's own scale still applies to the clipped sum
            _lib.check(_lib.lib.eco_grad_clip(_lib.ptr(self.grad), self.grad.numel(), scale, self.max_grad_norm,
                                              _lib.ptr(self.grad_norm), _lib.stream_ptr()))
        self.adam_step += 1
        _lib.check(_lib.lib.eco_adam(_lib.ptr(net.flat), _lib.ptr(self.grad), _lib.ptr(self.exp_avg),
                                     _lib.ptr(self.exp_avg_sq), net.flat.numel(), self.lr, 0.9, 0.999,
                                     self.adam_epsilon, float(self.weight_decay), scale, self.adam_step,
                                     _lib.stream_ptr()))
        net.repack()
        self.grad_steps += 1
        self._samples_since_sync += m * self.world
        if sync_loss:
            return loss_dev.item()
        return loss_dev if loss_out is not None else loss_dev.clone()

    def sync_target(self):
        """dqn.py:346-347: target <- online."""
        self.target_network.flat.copy_(self.network.flat)

    def _take_graph_slots(self, episodes):
        """Graph ids for the episodes being reset (a bool mask over B, or None = all).  Without
        regenerate_graphs: random graphs of the pool.  With it: the next slots of the store in ring
        order, each regenerated on the device when it is safe (no live user, `replay_buffer_size`
        pushes since its last episode ended), reused otherwise (warned once)."""
        k = self.B if episodes is None else int(episodes.sum())
        if self._slots is None:
            ids = self.graph_pool_ids[self._rng.integers(0, len(self.graph_pool_ids), k)]
        else:
            if self._host_graph_ids is not None:   # the episodes being reset leave their slots (no device read)
                old = self._host_graph_ids
                self._slots.release(old if episodes is None else old[episodes], self._pushed)
            ids = self._slots.take(k, self._pushed)
        if episodes is None:
            return ids
        out = np.zeros(self.B, np.int64)   # VecSpinSystem.reset reads graph_ids[mask]: B-long
        out[episodes] = ids
        return out

    def _regenerate(self, first, count, seed):
        kind, param = self.regenerate_graphs[:2]
        weights = (self.regenerate_graphs[2] if len(self.regenerate_graphs) > 2
                   else "random" if self.graphs.float_weights else "discrete")
        self.graphs.generate(first, count, kind, param, seed=seed, weights=weights, check=False)

    # slots regenerated so far (fresh graphs handed out) / handed out without regeneration (not yet safe)
    graphs_regenerated = property(lambda self: self._slots.regenerated if self._slots is not None else 0)
    graphs_reused = property(lambda self: self._slots.reused if self._slots is not None else 0)

    def vector_step(self, is_training_ready):
        """One act -> env.step -> replay.add over all B episodes; returns the new obs buffer.
        Every episode is live here: finished ones are reset by iteration() right after the step
        that ended them (the reference resets on done, dqn.py:306-327)."""
        x = self.env.obs_x
        nxt = self._obs[1] if x.data_ptr() == self._obs[0].data_ptr() else self._obs[0]
        self.act(x, self.env.graph_ids, is_training_ready, actions_out=self._actions)
        _, rew, done = self.env.step(self._actions, obs_out=nxt)
        if self.compact_replay:
            self.replay_buffer.add_step(self._actions, rew, done)
        else:
            self.replay_buffer.add_batch(x, nxt, self.env.graph_ids, self._actions, rew, done)
        self._pushed += self.B
        return nxt

    def _reset_env(self, graph_ids, seed, mask=None):
        """env.reset (all episodes, or the masked ones) and, for the compact replay, record the new states.
        The episodes' graph ids are mirrored on the host for the slot bookkeeping of _take_graph_slots."""
        ids = np.asarray(graph_ids, np.int64)
        if mask is None or self._host_graph_ids is None:
            self._host_graph_ids = ids.copy()
        else:
            m = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).astype(bool)
            self._host_graph_ids[m] = ids[m]
            mask = self.env._upload(mask, torch.uint8)  # one non-blocking upload for the env and the replay
        self.env.reset(graph_ids=graph_ids, mask=mask, seed=seed)
        if self.compact_replay:
            self.replay_buffer.snapshot(mask)

    def start(self):
        """Reset every episode on fresh pool graphs (start of learn).  The replay buffer and the push
        count persist across learn() calls (as the reference's replay buffer does), so graph slots that
        stored transitions reference are not regenerated by a second learn()."""
        self._reset_env(self._take_graph_slots(None), self.seed)
        self._steps_in_episode = 0
        self._timestep = 0
        self._ready = False
        self._k_per_vec = max(1, int(round(self.B * self.replay_ratio / self.M)))
        self._last_loss = None
        if self._loss_buf is None:
            self._loss_buf = torch.zeros(len(self._loss_t), dtype=torch.float32, device=self.device)
        # the reference's `losses` list is local to one learn() call (dqn.py:269): report from here on
        self._loss_start = self._loss_n
        # every episode ends exactly at max_steps only for reversible spins with Stopping.NORMAL
        # (spinsystem.py:539-554); otherwise dones are read back after each vector step
        self._lockstep = self.env.reversible_spins and self.env.cfg.stopping == 1
        # staggered episodes (stagger_episodes, lockstep envs only): episode b's first episode is cut after
        # T - (b T // B) steps (its last transition stored with the env's done = 0: a truncation, not a terminal),
        # so from then on the B episodes sit at B / T evenly spread phases and ~B / T of them end and are reset on
        # fresh graphs every vector step, as a single reference env's consecutive episodes pass through every phase
        self._stagger = bool(self.stagger_episodes and self._lockstep)
        if self._stagger:
            T = self.env.max_steps
            self._ep_left = T - (np.arange(self.B, dtype=np.int64) * T) // self.B

    def iteration(self):
        """One vector step of DQN.learn (dqn.py:273-347): act/step/add for all B episodes, reset
        finished episodes, then K gradient steps (replay ratio preserved) with target syncs.
        Schedules count global env-steps: B per rank per vector step, times the world size."""
        B, T = self.B, self.env.max_steps
        if not self._ready and len(self.replay_buffer) >= max(self.replay_start_size, self.M):
            self._ready = True
        self.vector_step(self._ready)
        self._timestep += B * self.world
        self._steps_in_episode += 1
        # dqn.py:284-290 run after each act with that env-step's 0-based index: a vector step ends with
        # the index of its last env-step (B = 1 reproduces the reference's sequence exactly)
        if self.update_exploration:
            self.update_epsilon(self._timestep - 1)
        if self.update_learning_rate:
            self.update_lr(self._timestep - 1)
        if self._stagger:
            self._ep_left -= 1
            ending = self._ep_left == 0
            if ending.any():
                self._reset_env(self._take_graph_slots(ending), self.seed + self._timestep, mask=ending)
                self._ep_left[ending] = T
        elif self._lockstep:
            if self._steps_in_episode == T:
                self._reset_env(self._take_graph_slots(None), self.seed + self._timestep)
                self._steps_in_episode = 0
        else:
            done = self.env.dones.bool()
            n_done = int(done.sum())
            if n_done == B:
                self._reset_env(self._take_graph_slots(None), self.seed + self._timestep)
                self._steps_in_episode = 0
            elif n_done:
                mask = done.cpu().numpy()
                self._reset_env(self._take_graph_slots(mask), self.seed + self._timestep, mask=done)
        if self._ready:
            # gradient step k's all-reduce overlaps step k+1's replay sample (stream order: the sample rewrites
            # the minibatch buffers after step k's forwards and backward have read them)
            nxt = [self.replay_buffer.sample(self.M)]
            for k in range(self._k_per_vec):
                tr = nxt.pop()
                more = k + 1 < self._k_per_vec

                def prefetch():
                    nxt.append(self.replay_buffer.sample(self.M))
                self._last_loss = self.train_step(tr, sync_loss=False, loss_out=self._loss_slot(self._timestep),
                                                  overlap=prefetch if more else None)
                if (self.grad_steps % self.target_sync_grad_steps == 0 if self.target_sync == "grad_steps"
                        else self._samples_since_sync >= self.target_sync_samples):
                    self.sync_target()
                    self._samples_since_sync = 0.0
        return self._last_loss

    def _loss_slot(self, timestep):
        """One-element view of the device loss log for the next gradient step (grown by doubling, so
        the log costs no allocation per step and one host copy in losses())."""
        if self._loss_n == len(self._loss_t):
            self._loss_buf = torch.cat([self._loss_buf, torch.zeros_like(self._loss_buf)])
            self._loss_t = np.concatenate([self._loss_t, np.zeros_like(self._loss_t)])
        self._loss_t[self._loss_n] = timestep
        self._loss_n += 1
        return self._loss_buf[self._loss_n - 1:self._loss_n]

    def learn(self, timesteps, verbose=False, on_vector_step=None):
        """dqn.py:256-395 with B episodes per vector step on each rank (timesteps counts global
        env-steps).  As in the reference, once training is ready: every `test_frequency` env-steps
        evaluate_agent() and save `<network_save_path>_best` when the score beats every earlier one
        (:349-364); every `save_network_frequency` env-steps save `<network_save_path><t>` (:366-372);
        at the end pickle test_scores / losses / solutions (:377-394).  A vector step that crosses
        k * frequency counts as reaching timestep k * frequency.  Files are written by rank 0.

        Multi-GPU: each crossing is ONE evaluation of the job, run by one rank (evaluation e by rank e mod world,
        on its test env: the same episodes and test graphs as a single-process evaluation at that timestep); its
        scores reach every rank through a small all-reduce to which only the owner contributes, issued by every
        rank at the same point (when evaluation e + world starts, or at the end of learn()), so the evaluation
        work per rank per vector step does not grow with the world size.  Nothing here waits for the training
        stream (learn_pipeline.LearnPipeline).  Returns the last 100 (timestep, loss) pairs."""
        import pickle
        self.start()
        pipe = LearnPipeline(self, verbose)
        while self._timestep < timesteps:
            t_prev = self._timestep
            self.iteration()
            t = self._timestep
            if on_vector_step is not None:
                on_vector_step(t)
            if not self._ready:
                continue
            crossed_test = t // self.test_frequency > t_prev // self.test_frequency
            if crossed_test and self.regenerate_graphs is not None:
                pipe.queue_error_peek()
            pipe.poll()
            if self.evaluate and crossed_test:
                pipe.launch((t // self.test_frequency) * self.test_frequency)
            if t // self.save_network_frequency > t_prev // self.save_network_frequency and pipe.rank == 0:
                tk = (t // self.save_network_frequency) * self.save_network_frequency
                main, ext = os.path.splitext(self.network_save_path)
                pipe.save_deferred(main + str(tk) + (ext or ".pth"), False)
        pipe.drain()
        losses = self.losses()
        if pipe.rank == 0 and self.test_save_path is not None:
            path = self.test_save_path
            if os.path.splitext(path)[-1] == '':
                path += '.pkl'
            folder = os.path.split(self.test_save_path)[0]
            for p_, arr in ((path, pipe.test_scores), (os.path.join(folder, "losses.pkl"), losses),
                            (os.path.join(folder, "solution.pkl"), pipe.test_solutions)):
                with open(p_, 'wb+') as output:
                    pickle.dump(np.array(arr), output, pickle.HIGHEST_PROTOCOL)
                if verbose:
                    print('saved to {}'.format(p_))
        self.test_scores, self.test_solutions = pipe.test_scores, pipe.test_solutions
        self.evaluations_run = sum(1 for i in range(pipe.n_eval) if i % pipe.world == pipe.rank)  # by this rank
        return losses[-100:]

    def losses(self):
        """[[timestep, loss], ...] of every gradient step of the current (or last) learn() call
        (dqn.py:269,339; one host copy)."""
        n, s = self._loss_n, self._loss_start
        if n <= s:
            return []
        vals = self._loss_buf[s:n].cpu().tolist()
        return [[int(t), v] for t, v in zip(self._loss_t[s:n], vals)]

    # ------------------------------------------------------------------ eval
    def evaluate_agent(self, batch_size=None, test_env=None):
        """dqn.py:514-602: greedy rollouts of `test_episodes` episodes, at most `batch_size`
        (default minibatch_size) at a time, on the test VecSpinSystem whose n_envs slots hold the
        concurrent episodes.  Episodes take the test graphs in order, continuing across calls (the
        ordered SetGraphGenerator of train_eco.py:69).  A finished episode's slot is refilled before
        the next prediction, and each prediction couples norm.max() over the active episodes only
        (predict on obs_batch, :546-547).  test_metric:
          BEST              -> (best_score, best_solution)  (:564-566)
          FINAL             -> (score, solution) of the final spins (:567-569)
          CUMULATIVE_REWARD -> (sum of rewards, 0)          (:560-561, :580-581)
          ENERGY_ERROR      -> (0, 0), as in the reference whose branch is commented out (:571-583)
        Returns (mean score, mean solution)."""
        return self._evaluator.evaluate(batch_size, test_env)

    # names the benchmark, the tests and the distributed workers use
    def _test_env(self, test_env=None, batch_size=None):
        return self._evaluator.test_env(test_env, batch_size)

    def _one_fill_ok(self, env, batch_size):
        return self._evaluator.one_fill_ok(env, batch_size)

    def _overlap_ok(self, env):
        return self._evaluator.overlap_ok(env)

    def _evaluate_overlapped(self, tk):
        return self._evaluator.evaluate_overlapped(tk)

    def _eval_one_fill_finish(self, p):
        return self._evaluator.finish(p)

    # the snapshot network of overlapped evaluations (None until one ran); (id(env), id(net)) -> rollout record
    _eval_net = property(lambda self: self._evaluator.net)
    _eval_graphs = property(lambda self: self._evaluator.rollouts)

    # ------------------------------------------------------------ checkpoint
    def _save_flat(self, path, flat):
        """save() of a parameter vector in state_dict order (a host copy of MPNN.flat): the same keys and
        tensors as the network's state_dict (mpnn.MPNN.flat views)."""
        from ...networks.mpnn import param_layout
        sd, off = {}, 0
        for name, shape in param_layout(self.network.n_obs_in):
            cnt = int(np.prod(shape))
            sd[name] = flat[off:off + cnt].view(shape).clone()
            off += cnt
        assert off == flat.numel()
        torch.save(sd, path)

    def save(self, path='network.pth', network=None):
        """dqn.py:604-607: torch.save(state_dict) -- loadable by the reference MPNN.  The reference's
        extension fix-up is a no-op expression (`path + '.pth'`, :606), so `path` is used as given.
        network: another network to save (learn()'s evaluation snapshot); default the online network."""
        net = self.network if network is None else network
        torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, path)

    def load(self, path):
        """dqn.py:609-610 (weights_only: state_dicts are plain tensors)."""
        self.network.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
