"""Proportional prioritised replay on the device (Schaul et al. 2016) around the agent's replay rings.

The host `utils.PrioritisedReplayBuffer` keeps the reference's rank-based heap and API; it reads TD errors back to
numpy on every call, so DQN.learn() -- which makes no host read -- cannot drive it.  DevicePrioritisedReplay is the
one the training step uses: one integer priority (`mass`, uint32) per logical ring position, integer sums, a
stratified sampler keyed by (seed, counter), all of it kernels of csrc/eco_prio.hip (include/eco_hip.h eco_prio_*)
with no host read anywhere.  tests/prio_common.py restates the arithmetic exactly.
"""
import ctypes

import torch

from ... import _lib
from .utils import CompactReplayBuffer

PRIORITISED_DEFAULTS = {"alpha": 0.6, "beta0": 0.4, "beta_steps": 100000, "eps": 1e-3, "td_max": 1.0}


def prioritised_config(cfg):
    """DQN(prioritised_replay=...): the dict with the defaults filled in; unknown keys are rejected."""
    if not isinstance(cfg, dict):
        raise ValueError("prioritised_replay must be None or a dict of " + ", ".join(PRIORITISED_DEFAULTS))
    unknown = sorted(set(cfg) - set(PRIORITISED_DEFAULTS))
    if unknown:
        raise ValueError(f"prioritised_replay: unknown keys {unknown} (known: {sorted(PRIORITISED_DEFAULTS)})")
    out = dict(PRIORITISED_DEFAULTS)
    out.update(cfg)
    return out


class DevicePrioritisedReplay:
    """A ReplayBuffer or CompactReplayBuffer with proportional priorities.

    mass[x] belongs to the logical ring position x = k % capacity of transition k (the slot of the feature ring; the
    compact ring resolves it to its own slot).  add_batch / add_step / snapshot forward to the wrapped ring, and
    each push gives the new transitions the current maximum mass.  sample(M) draws M positions in proportion to
    mass (with replacement), gathers them through the ring and returns the usual 6-tuple; the positions and their
    importance weights stay on the device in last_idx / last_weights for the TD kernel, and update(abs_td) writes
    the new priorities of exactly those positions.  beta rises linearly from beta0 to 1 over beta_steps sample()
    calls (computed on the host, as configure_beta_anneal_time does, dqn/utils.py:252, :274-275)."""

    def __init__(self, inner, alpha=0.6, beta0=0.4, beta_steps=100000, eps=1e-3, td_max=1.0, seed=None):
        if not (alpha >= 0 and eps >= 0 and td_max > 0 and 0 <= beta0 <= 1 and beta_steps >= 1):
            raise ValueError("prioritised replay: need alpha >= 0, eps >= 0, td_max > 0, 0 <= beta0 <= 1, beta_steps >= 1")
        self.inner = inner
        self.compact = isinstance(inner, CompactReplayBuffer)
        self._capacity = inner._capacity
        self.device = inner.device
        self.alpha, self.beta0, self.beta_steps = float(alpha), float(beta0), int(beta_steps)
        self.eps, self.td_max = float(eps), float(td_max)
        self.beta = self.beta0
        self.seed = (inner.seed if seed is None else seed) ^ 0x9E3779B9
        self._counter = 0
        self.mass = torch.zeros(self._capacity, dtype=torch.int32, device=self.device)   # uint32 bits, all < 2^31
        self.workspace = torch.zeros(_lib.lib.eco_prio_workspace_bytes(self._capacity), dtype=torch.uint8,
                                     device=self.device)
        self.last_idx = None
        self.last_weights = None
        self._draw = {}

    # ------------------------------------------------------------------ push
    def _push(self, pos, batch, size_before, stream=None):
        _lib.check(_lib.lib.eco_prio_push(_lib.ptr(self.mass), self._capacity, pos, batch, size_before,
                                          _lib.ptr(self.workspace), _lib.stream_ptr(stream)))

    def add_batch(self, xs, *args, stream=None):
        pos, size = self.inner._position, len(self.inner)
        self.inner.add_batch(xs, *args, stream=stream)
        self._push(pos, xs.shape[0], size, stream)

    def add_step(self, actions, rewards, dones, stream=None):
        pos, size = self.inner._pushed % self._capacity, len(self.inner)
        self.inner.add_step(actions, rewards, dones, stream=stream)
        self._push(pos, self.inner.env.n_envs, size, stream)

    def snapshot(self, mask=None, stream=None):
        self.inner.snapshot(mask, stream=stream)

    # ---------------------------------------------------------------- sample
    def sample(self, batch_size, device=None, stream=None):
        """(states_x, actions, rewards, states_next_x, dones, graph_ids) of `batch_size` transitions drawn in
        proportion to their mass; last_idx (int32) and last_weights (float32) describe the draw."""
        m, rb = int(batch_size), self.inner
        if m not in self._draw:
            self._draw[m] = (torch.empty(m, dtype=torch.int32, device=self.device),
                             torch.empty(m, dtype=torch.float32, device=self.device))
        idx, w = self._draw[m]
        self._counter += 1
        self.beta = min(1.0, self.beta0 + (1.0 - self.beta0) * self._counter / self.beta_steps)
        st = _lib.stream_ptr(stream)
        _lib.check(_lib.lib.eco_prio_sample(_lib.ptr(self.mass), self._capacity, len(rb), m,
                                            ctypes.c_uint64(self.seed), ctypes.c_uint64(self._counter), self.beta,
                                            _lib.ptr(idx), _lib.ptr(w), _lib.ptr(self.workspace), st))
        xs, xn, gid, act, rew, done = rb._buffers(m)
        if self.compact:
            _lib.check(_lib.lib.eco_replay_compact_gather(
                ctypes.byref(rb.env.cfg), _lib.ptr(rb.env.state), ctypes.byref(rb.env.graphs.gs), rb.env.n_envs,
                _lib.ptr(rb.ring), self._capacity, len(rb), rb._pushed, m, _lib.ptr(idx), _lib.ptr(xs), _lib.ptr(xn),
                _lib.ptr(gid), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), st))
        else:
            _lib.check(_lib.lib.eco_replay_gather(ctypes.byref(rb.rb), m, _lib.ptr(idx), _lib.ptr(xs), _lib.ptr(xn),
                                                  _lib.ptr(gid), _lib.ptr(act), _lib.ptr(rew), _lib.ptr(done), st))
        self.last_idx, self.last_weights = idx, w
        return xs, act, rew, xn, done, gid

    def update(self, abs_td, stream=None):
        """New priorities of the last sample's positions from their |TD errors| (device float32 [M])."""
        if self.last_idx is None or abs_td.shape[0] != self.last_idx.shape[0]:
            raise ValueError("prioritised replay: update() takes one |td| per position of the last sample()")
        _lib.check(_lib.lib.eco_prio_update(_lib.ptr(self.mass), self._capacity, self.last_idx.shape[0],
                                            _lib.ptr(self.last_idx), _lib.ptr(abs_td), self.alpha, self.eps,
                                            self.td_max, _lib.stream_ptr(stream)))

    def __len__(self):
        return len(self.inner)

    def __getattr__(self, name):   # bytes_per_transition, n_spins, ... of the wrapped ring
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)
