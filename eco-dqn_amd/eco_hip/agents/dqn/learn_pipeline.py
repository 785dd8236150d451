"""The host pipeline of DQN.learn(): evaluations in flight, their scores' all-reduce, the `_best` snapshots,
deferred checkpoints and the peeks at the device error word.  Nothing here waits for the training stream.

Multi-GPU: each test_frequency crossing is ONE evaluation of the job, run by one rank (evaluation e by rank
e mod world, on its test env: the same episodes and test graphs as a single-process evaluation at that
timestep); its scores reach every rank through a small all-reduce to which only the owner contributes,
issued by every rank at the same point (when evaluation e + world starts, or at the end of learn()), so the
evaluation work per rank per vector step does not grow with the world size.  The all-reduce is asynchronous
and its result is read back into pinned memory behind an event, recorded (scores, `_best`) once that event has
fired -- a few vector steps later -- or at the end; the owner's scores come from pinned copies behind the side
stream's event.  Rank 0 snapshots the weights of every evaluation into pinned host memory at its timestep for
`_best` (the parameters are bit-identical across ranks)."""
import os
from collections import deque
from dataclasses import dataclass

import numpy as np
import torch

from ... import _lib


@dataclass
class Evaluation:
    tk: int                  # the timestep it evaluates
    owner: int               # the rank that runs it
    idx: int                 # its index in the job
    snap: object = None      # rank 0: the weights at tk in pinned memory, behind snap_ev
    snap_ev: object = None
    launched: object = None  # owner: the overlapped evaluation (evaluation.Launched) ...
    result: tuple = None     # ... or the synchronous evaluation's (score, solution)
    red: tuple = None        # (pinned source, reduced tensor, work) of the scores' all-reduce
    res: object = None       # nccl: the reduced scores in pinned memory, behind res_ev
    res_ev: object = None


class LearnPipeline:
    def __init__(self, agent, verbose):
        self.agent = agent
        self.verbose = verbose
        self.rank = torch.distributed.get_rank() if agent.dist else 0
        self.world = agent.world
        self.nccl = self.world > 1 and torch.distributed.get_backend() == "nccl"
        self.test_scores, self.test_solutions = [], []
        self.inflight = deque()    # evaluations launched, scores not yet taken (index order)
        self.reducing = deque()    # scores taken, all-reduce / read-back in flight, not yet recorded (index order)
        self.err_checks = deque()  # (event, pinned word) peeks at the device error word
        self.saves = deque()       # (event, pinned weights, path) periodic checkpoints not yet written
        self.n_eval = 0            # evaluations launched by the job so far (every rank counts the same)
        self.cursor0 = agent._test_env()._eval_next_graph if agent.evaluate else 0
        # rank 0's weight snapshots for _best, one pinned slot per evaluation that can be unrecorded at once
        self.depth = 3 * self.world
        self.snaps = ([torch.empty(agent.network.flat.numel(), dtype=torch.float32).pin_memory()
                       for _ in range(self.depth)] if self.rank == 0 and agent.evaluate else None)

    def record(self, e, test_score, test_solution):
        a = self.agent
        if self.verbose and self.rank == 0:
            print('\nTest score: {}\nTest solution: {}\n'.format(np.round(test_score, 3),
                                                                np.round(test_solution, 3)))
        if all(test_score > sc for _, sc in self.test_scores) and self.rank == 0:
            main, ext = os.path.splitext(a.network_save_path)
            e.snap_ev.synchronize()  # the snapshot copy (issued at the evaluation's timestep) has landed
            a._save_flat(main + "_best" + (ext or ".pth"), e.snap)
        self.test_scores.append([e.tk, test_score])
        self.test_solutions.append([e.tk, test_solution])

    def take(self, e):
        """Evaluation e's scores on every rank (the same call order everywhere: the all-reduce is collective):
        the owner's from its pinned results, all-reduced without waiting; recorded by flush()."""
        if e.owner == self.rank:
            sc, so = self.agent._eval_one_fill_finish(e.launched) if e.launched is not None else e.result
        else:
            sc, so = 0.0, 0.0
        if self.world == 1:
            self.record(e, sc, so)
            return
        src = torch.tensor([sc, so], dtype=torch.float64).pin_memory()
        if self.nccl:
            t = torch.empty(2, dtype=torch.float64, device=self.agent.device)
            t.copy_(src, non_blocking=True)
        else:
            t = src
        work = torch.distributed.all_reduce(t, async_op=True)  # only the owner contributes: the sum is its result
        e.red = (src, t, work)
        if self.nccl:
            work.wait()  # the current stream waits for the collective; the host does not
            e.res = torch.empty(2, dtype=torch.float64).pin_memory()
            e.res.copy_(t, non_blocking=True)
            e.res_ev = torch.cuda.Event()
            e.res_ev.record()
        self.reducing.append(e)

    def flush(self, upto):
        """Record, in order, the reduced evaluations whose results have arrived, waiting for those with
        index <= upto (None: wait for none)."""
        while self.reducing:
            e = self.reducing[0]
            src, t, work = e.red
            must = upto is not None and e.idx <= upto
            if self.nccl:
                if not (must or e.res_ev.query()):
                    return
                e.res_ev.synchronize()
                res = e.res
            else:
                if not (must or work.is_completed()):
                    return
                work.wait()
                res = t
            self.reducing.popleft()
            self.record(e, float(res[0]), float(res[1]))

    def save_deferred(self, path, block):
        """Periodic checkpoints: the weights copied into pinned memory at their timestep, written once the
        copy has landed (no wait on the training stream)."""
        a = self.agent
        if path is not None:
            host = torch.empty(a.network.flat.numel(), dtype=torch.float32).pin_memory()
            host.copy_(a.network.flat, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.saves.append((ev, host, path))
        while self.saves and (block or self.saves[0][0].query()):
            ev, host, p_ = self.saves.popleft()
            ev.synchronize()
            a._save_flat(p_, host)

    def queue_error_peek(self):
        """Graphs regenerated with check=False since the last peek: an edge-slot overflow sets the device error
        word (the slot becomes an empty graph); copied out without waiting (eco_error_word_copy), raised by
        peek_errors() when seen."""
        word = torch.zeros(1, dtype=torch.int32).pin_memory()
        _lib.check(_lib.lib.eco_error_word_copy(_lib.ptr(word), _lib.stream_ptr()))
        ev = torch.cuda.Event()
        ev.record()
        self.err_checks.append((ev, word))

    def peek_errors(self, block):
        """Raise a device error flagged since the last peek (regenerated graphs: edge-slot overflow)."""
        while self.err_checks and (block or self.err_checks[0][0].query()):
            ev, word = self.err_checks.popleft()
            ev.synchronize()
            if int(word[0]) != 0:
                self.agent.graphs.check_errors()

    def poll(self):
        """After a vector step: whatever has arrived, without waiting."""
        self.peek_errors(False)
        self.flush(None)
        self.save_deferred(None, False)
        if (self.world == 1 and self.inflight and self.inflight[0].launched is not None
                and self.inflight[0].launched.done.query()):
            self.take(self.inflight.popleft())  # finished early (one process: no collective to keep in step)

    def launch(self, tk):
        """Start the job's next evaluation, of the weights at timestep tk."""
        a = self.agent
        while len(self.inflight) >= self.world:  # this evaluation's owner runs one evaluation at a time
            self.take(self.inflight.popleft())
        e = Evaluation(tk=tk, owner=self.n_eval % self.world, idx=self.n_eval)
        self.n_eval += 1
        if self.rank == 0:
            # slot idx % depth is free once evaluation idx - depth is recorded (launched >= 2 world earlier)
            self.flush(e.idx - self.depth)
            e.snap = self.snaps[e.idx % self.depth]
            e.snap.copy_(a.network.flat, non_blocking=True)  # the weights at tk, for _best
            e.snap_ev = torch.cuda.Event()
            e.snap_ev.record()
        if e.owner == self.rank:
            env = a._test_env()
            n_graphs = env.graphs.n_graphs
            env._eval_next_graph = (self.cursor0 + e.idx * a.test_episodes) % n_graphs  # job-wide order
            if a._overlap_ok(env):
                e.launched = a._evaluate_overlapped(tk)
            else:
                e.result = a.evaluate_agent()
        self.inflight.append(e)

    def drain(self):
        """End of learn(): take, reduce and record every evaluation, write every checkpoint, raise any error."""
        while self.inflight:
            self.take(self.inflight.popleft())
        self.flush(self.n_eval)
        self.peek_errors(True)
        self.save_deferred(None, True)
        if self.agent.regenerate_graphs is not None:
            self.agent.graphs.check_errors()
