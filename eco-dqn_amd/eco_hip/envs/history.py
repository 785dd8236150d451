"""On-device trajectory histories of a VecSpinSystem (Network.history, src/agents/solver.py:189-265).

The reference appends one python list per step -- [action, solution, reward, qs, spins, score_mask, valid] --
from the env's numpy state.  `History` owns one device tensor per field, [rows, B(, N)], and `record` appends
one row for every episode with ONE kernel launch (eco_env_record): nothing is read back until `to_records`.

Memory: with everything on a history takes rows x B x N x 13 bytes (qs 4 + spins 1 + score_mask 8 per vertex)
plus rows x B x 33 bytes of per-episode scalars: 2 MB for 50 episodes of 200 steps on 200 vertices, but
5.4 GB per 256 rows at B = 8192 -- histories are for tens of episodes, not for a training batch.
"""
import ctypes

import torch

from .. import _lib


class History:
    """Device buffers of `rows` history rows for the B episodes of `env`.

    record_solution / record_rewards / record_qs / record_spins are the reference's flags (solver.py:184-187):
    a dropped field is neither allocated nor written, and `to_records` drops the same list element the
    reference drops.  The score mask and the validity bit are always recorded, as in the reference.
    record_score adds scorer.get_score per row (the per-step column of test_network(return_history=True));
    record_mask=False drops the score mask and validity (that rollout records neither)."""

    def __init__(self, env, rows, record_solution=True, record_rewards=True, record_qs=True, record_spins=True,
                 record_score=False, record_mask=True, record_action=True):
        self.env = env
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError("a history needs at least one row")
        B, N, dev = env.n_envs, env.n_spins, env.graphs.device
        self.record_solution, self.record_rewards = bool(record_solution), bool(record_rewards)
        self.record_qs, self.record_spins = bool(record_qs), bool(record_spins)

        def buf(on, shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=dev) if on else None

        R = self.rows
        self.action = buf(record_action, (R, B), torch.float64)
        self.solution = buf(record_solution, (R, B), torch.float64)
        self.reward = buf(record_rewards, (R, B), torch.float64)
        self.qs = buf(record_qs, (R, B, N), torch.float32)
        self.spins = buf(record_spins, (R, B, N), torch.int8)
        self.score_mask = buf(record_mask, (R, B, N), torch.float64)
        self.valid = buf(record_mask, (R, B), torch.uint8)
        self.score = buf(record_score, (R, B), torch.float64)
        self.length = torch.zeros(B, dtype=torch.int32, device=dev)
        self.hist = _lib.EnvHistory()
        self.hist.rows = R
        for name in ("action", "solution", "reward", "qs", "spins", "score_mask", "valid", "length", "score"):
            t = getattr(self, name)
            setattr(self.hist, name, t.data_ptr() if t is not None else None)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.action, self.solution, self.reward, self.qs,
                                                          self.spins, self.score_mask, self.valid, self.score,
                                                          self.length) if t is not None)

    def clear(self):
        """Forget every row (Network.reset(clear_history=True)); the buffers are reused."""
        self.length.zero_()

    def record(self, row, skip=None, actions=None, rewards=None, q=None):
        """Append row `row` for every episode with skip[e] == 0: row 0 after a reset, row >= 1 after a step with
        the int32 actions [B] stepped, the float64 rewards [B] it returned and the float32 q [B, N] the actions
        came from.  `skip` is the uint8 dones held BEFORE the step."""
        env = self.env
        for t, dt in ((skip, torch.uint8), (actions, torch.int32), (rewards, torch.float64), (q, torch.float32)):
            if t is not None and (t.dtype != dt or not t.is_contiguous()):
                raise ValueError(f"History.record takes contiguous {dt} device tensors")
        _lib.check(_lib.lib.eco_env_record(ctypes.byref(env.cfg), ctypes.byref(env.graphs.gs), _lib.ptr(env.state),
                                           env.n_envs, int(row), _lib.ptr(skip), _lib.ptr(actions),
                                           _lib.ptr(rewards), _lib.ptr(q), ctypes.byref(self.hist), env._s()))

    def to_records(self, e):
        """Episode e's rows as the reference's nested lists (solver.py:200-216, :249-265), length[e] of them:
        [action, solution, reward, qs, spins, score_mask, valid] with the elements of dropped record_* flags
        left out, and the bare [action, score_mask, valid] (integer action on the reset row) when neither
        solutions nor rewards are recorded.  Synchronises: one device-to-host copy per field."""
        n = int(self.length[e])
        col = lambda t: None if t is None else t[:n, e].cpu().numpy()
        action, solution, reward = col(self.action), col(self.solution), col(self.reward)
        qs, spins, mask, valid = col(self.qs), col(self.spins), col(self.score_mask), col(self.valid)
        out = []
        for r in range(n):
            if not self.record_solution and not self.record_rewards:
                rec = [0 if r == 0 else int(action[r])]
            else:
                rec = [float(action[r])]
                if self.record_solution:
                    rec += [float(solution[r])]
                if self.record_rewards:
                    rec += [float(reward[r])]
                if self.record_qs:
                    rec += [[0] * qs.shape[1] if r == 0 else qs[r].tolist()]
                if self.record_spins:
                    rec += [list(spins[r].astype("float64"))]
            if mask is not None:
                rec += [list(mask[r])]
                rec += [bool(valid[r])]
            out.append(rec)
        return out
