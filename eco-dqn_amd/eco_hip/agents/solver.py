"""Spin solvers on the batched env (src/agents/solver.py:11-267): `Network`, `Greedy` and `Random`.

The reference's names and call shapes -- set_env / reset(spins) / solve() / .measure, and Network.history --
batched over the B episodes of ONE VecSpinSystem: total_reward and measure are [B] float64 device tensors,
and Network.history is a `History` (eco_hip.envs.history) whose `to_records(e)` gives episode e's rows in the
reference's nesting.  Every step is device work (MPNN forward with the fused act, env step, one record launch);
solve() reads the done flags back once per step to know when every episode has finished.

Not provided: the reference's CoverMatching, CplexSolver and NetworkXSolver (solver.py:270-) are host-side
baselines built on networkx / docplex with no device path; they stay in the reference.
"""
import ctypes
from abc import ABC, abstractmethod

import numpy as np
import torch

from .. import _lib
from ..envs.history import History
from ..envs.utils import SpinBasis


class SpinSolver(ABC):
    """Abstract base of the solvers (solver.py:11-86).  env: one VecSpinSystem; its graph ids are kept."""

    def __init__(self, env, record_cut=False, record_rewards=False, record_qs=False, verbose=False, name=None):
        self.env = env
        self.verbose = verbose
        self.record_solution = record_cut
        self.record_rewards = record_rewards
        self.record_qs = record_qs
        self.name = name
        self.measure = 0
        self.total_reward = 0
        self._seed = 0

    def set_env(self, env):
        self.env = env

    def _reset_env(self, spins):
        env = self.env
        if spins is not None:
            s = torch.as_tensor(np.asarray(spins.cpu() if isinstance(spins, torch.Tensor) else spins))
            if env.spin_basis == SpinBasis.BINARY:   # _format_spins_to_signed (spinsystem.py:595-606)
                s = 2 * s - 1
            s = s.to(torch.int8)
            if s.dim() == 1:
                s = s.unsqueeze(0).expand(env.n_envs, -1)
            if tuple(s.shape) != (env.n_envs, env.n_spins):
                raise ValueError(f"spins must be [{env.n_spins}] or [{env.n_envs}, {env.n_spins}]")
            spins = s.contiguous()
        self._seed += 1
        obs = env.reset(spins=spins, seed=self._seed)
        self.total_reward = torch.zeros(env.n_envs, dtype=torch.float64, device=env.graphs.device)
        return obs

    def reset(self, spins=None):
        """spins: [N] (every episode) or [B, N], in the env's spin basis; None: the env's own random reset."""
        self._reset_env(spins)

    def _solution(self):
        """scorer.get_solution of every episode's current state: eco_env_record with only `solution` set."""
        env = self.env
        out = torch.empty(1, env.n_envs, dtype=torch.float64, device=env.graphs.device)
        h = _lib.EnvHistory()
        h.rows = 1
        h.solution = out.data_ptr()
        _lib.check(_lib.lib.eco_env_record(ctypes.byref(env.cfg), ctypes.byref(env.graphs.gs), _lib.ptr(env.state),
                                           env.n_envs, 0, None, None, None, None, ctypes.byref(h), env._s()))
        return out[0]

    def solve(self, *args):
        """Step until every episode is done.  Returns total_reward [B]; sets measure [B] to get_solution of each
        episode's LAST state (solver.py:59-67)."""
        for _ in range(self.env.max_steps + 1):
            reward, done = self.step(*args)
            self.total_reward += reward
            if bool(done.all()):
                break
        self.measure = self._solution()
        return self.total_reward

    @abstractmethod
    def step(self, *args):
        raise NotImplementedError()


class Greedy(SpinSolver):
    """solver.py:88-131: the action maximising the immediate score change.  An episode whose best change is
    negative stops without a step (eco_env_greedy_actions marks it done; the step then leaves it unchanged)."""

    def step(self):
        a = self.env.greedy_actions()
        _, reward, done = self.env.step(a)
        return reward, done


class Random(SpinSolver):
    """solver.py:133-159: a uniform action per episode from a torch.Generator on the env's device
    (`generator`, seeded 0 when None).  Irreversible envs draw among the still-flippable vertices."""

    def __init__(self, *args, generator=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.generator = generator
        if generator is None:
            self.generator = torch.Generator(device=self.env.graphs.device)
            self.generator.manual_seed(0)

    def step(self):
        env = self.env
        dev = env.graphs.device
        if env.reversible_spins:
            a = torch.randint(0, env.n_spins, (env.n_envs,), generator=self.generator, device=dev, dtype=torch.int32)
        else:
            u = torch.rand(env.n_envs, env.n_spins, generator=self.generator, device=dev)
            spins = env.read(spins=True)["spins"]
            a = torch.where(spins < 0, u, torch.full_like(u, -1.0)).argmax(1).to(torch.int32)
        self.last_actions = a
        _, reward, done = env.step(a)
        return reward, done


class Network(SpinSolver):
    """solver.py:161-267: act greedily on the network's Q-values and record every step in `.history`.

    Each step is the MPNN forward with the fused act (first-index argmax over allowed vertices), the env step
    and one History.record launch.  The norm scope is per graph: the reference calls the network on ONE
    observation, so its norm.max() is that graph's.  `epsilon` is honoured through ActConfig, but the random
    draws are the device generator's, not numpy's: parity with the reference is claimed for epsilon = 0 only."""

    epsilon = 0

    def __init__(self, network, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.network = network
        self.record_solution = True
        self.record_qs = True
        self.record_rewards = True
        self.record_spins = True
        self.history = None
        self._row = 0
        self._counter = 0

    def set_env(self, env):
        self.env = env
        self.history = None

    def _make_history(self):
        env = self.env
        dev = env.graphs.device
        self.history = History(env, env.max_steps + 1, record_solution=self.record_solution,
                               record_rewards=self.record_rewards, record_qs=self.record_qs,
                               record_spins=self.record_spins)
        self._q = torch.zeros(env.n_envs, env.n_spins, dtype=torch.float32, device=dev)
        self._a = torch.zeros(env.n_envs, dtype=torch.int32, device=dev)
        self._skip = torch.zeros(env.n_envs, dtype=torch.uint8, device=dev)

    def reset(self, spins=None, clear_history=True):
        self._reset_env(spins)
        if self.history is None or self.history.env is not self.env:
            self._make_history()
            clear_history = True
        if clear_history:
            self.history.clear()
            self._row = 0
            self.history.record(0)

    def step(self):
        env = self.env
        if self.history is None:
            raise RuntimeError("Network.step before reset")
        act = _lib.ActConfig(float(self.epsilon), int(env.reversible_spins), env.allowed_action_value(), self._seed,
                             self._counter)
        self._counter += 1
        self.network.forward_graphs(env.obs_x, env.graphs, env.graph_ids, norm_scope=_lib.ECO_NORM_PER_GRAPH,
                                    q_out=self._q, act=act, actions_out=self._a)
        self._skip.copy_(env.dones)   # the dones held before the step: an episode's last row is its last step
        _, reward, done = env.step(self._a)
        self._row += 1
        # a history kept across resets (clear_history=False) holds max_steps + 1 rows in all: past that the
        # export rejects the row (ValueError) rather than dropping it
        self.history.record(self._row, skip=self._skip, actions=self._a, rewards=reward, q=self._q)
        return reward, done
