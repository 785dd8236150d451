"""Shared by the Huber-loss / gradient-clipping tests: the reference's recorded train steps
(tests/golden/make_huber_clip_golden.py) as one mapping."""
import glob
import os

import numpy as np

from conftest import GOLDEN


def load_golden():
    """dqn_step_huber_clip.npz plus the per-agent files of the weights after each step."""
    out = dict(np.load(os.path.join(GOLDEN, "dqn_step_huber_clip.npz")))
    parts = sorted(glob.glob(os.path.join(GOLDEN, "dqn_step_huber_clip_w_*.npz")))
    assert parts
    for p in parts:
        out.update(np.load(p))
    return out


def clipped_agents(f):
    """Prefixes of the recorded agents that ran with max_grad_norm."""
    return [a for a in ("clip/", "clip_wide/") if a + "max_grad_norm" in f]
