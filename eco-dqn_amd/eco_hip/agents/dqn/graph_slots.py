"""Graph-slot bookkeeping of DQN(regenerate_graphs=...): which slots of a GraphStore.slots store may be
regenerated.  Host-only (numpy), so it runs without a device.

Fresh graphs per episode like the reference's generators (utils.py:165-236): every reset takes the next
slots of the store in ring order and regenerates them on the device first.  Replay entries reference
graph ids, so a slot is only regenerated once no live episode uses it and `replay_buffer_size` pushes
have passed since its last episode ended (every entry that could reference it has been overwritten);
otherwise its graph is reused as it is (still correct, not fresh) and a warning is issued once."""
import warnings

import numpy as np


def graph_slots_needed(n_envs, max_steps, replay_buffer_size):
    """GraphStore slots for fresh graphs per episode with lockstep episodes (each ends at max_steps):
    a batch of n_envs episodes pushes n_envs * max_steps transitions, and a batch's slots may only be
    regenerated once replay_buffer_size pushes have passed since it ended, so
    ceil(replay_buffer_size / (n_envs * max_steps)) + 1 batches of n_envs slots rotate."""
    per_batch = n_envs * max_steps
    return n_envs * (-(-int(replay_buffer_size) // per_batch) + 1)


class GraphSlotRing:
    """rng: the agent's numpy Generator (the regeneration seeds are drawn from it, one per generate call);
    generate(first, count, seed): regenerate slots first .. first + count - 1."""

    def __init__(self, n_slots, replay_buffer_size, rng, generate):
        self.users = np.zeros(n_slots, np.int64)              # live episodes on each slot
        self.free_at = np.full(n_slots, -(1 << 62), np.int64)  # push count when its last episode ended
        self.cursor = 0
        self.regenerated = 0      # slots regenerated so far (fresh graphs handed out)
        self.reused = 0           # slots handed out without regeneration (not yet safe)
        self.replay_buffer_size = replay_buffer_size
        self._rng = rng
        self._generate = generate
        self._warned = False

    def release(self, old, pushed):
        """The episodes on slots `old` have ended at push count `pushed`."""
        np.subtract.at(self.users, old, 1)
        self.free_at[old[self.users[old] == 0]] = pushed

    def take(self, k, pushed):
        """The next k slots in ring order for episodes starting at push count `pushed`; the safe ones are
        regenerated first, in maximal runs of consecutive slots."""
        n_slots = len(self.users)
        ids = (self.cursor + np.arange(k)) % n_slots
        self.cursor = int((self.cursor + k) % n_slots)
        safe = (self.users[ids] == 0) & (pushed - self.free_at[ids] >= self.replay_buffer_size)
        fresh = ids[safe]
        for run in np.split(fresh, np.nonzero(np.diff(fresh) != 1)[0] + 1) if len(fresh) else []:
            self._generate(int(run[0]), len(run), int(self._rng.integers(1 << 62)))
        self.regenerated += len(fresh)
        self.reused += k - len(fresh)
        if len(fresh) < k and not self._warned:
            warnings.warn(f"regenerate_graphs: {k - len(fresh)} of {k} episodes reset onto graphs that stored "
                          f"transitions may still reference (store of {n_slots} slots); they reuse those graphs. "
                          "Allocate more GraphStore.slots for a fresh graph per episode.", RuntimeWarning)
            self._warned = True
        np.add.at(self.users, ids, 1)
        return ids
