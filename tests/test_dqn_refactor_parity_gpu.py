"""Whole-agent learn() runs against the commit before the DQN class was split into the training step,
graph_slots.GraphSlotRing, evaluation.Evaluator and learn_pipeline.LearnPipeline.  The fixture
tests/golden/dqn_learn_parent.npz was recorded on an MI355X from that commit (recorder beside it; cases in
tests/dqn_refactor_cases.py).  Training is deterministic run to run (two recordings of the parent were identical
in every field), so every field is compared exactly: each [timestep, loss], the test scores and solutions, the
last evaluation's per-episode results, the final parameters and the `_best` state dict (by the SHA-256 of their
bytes), grad_steps, epsilon, lr and the regenerated / reused graph counts."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dqn_refactor_cases import CASES, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "dqn_learn_parent.npz"))


# "mse_explicit": loss="mse" passed explicitly must equal the parent's default eco_dqn_td path bit for bit
@pytest.mark.parametrize("name,entry", [(c, c) for c in CASES] + [("mse_explicit", "eco_best")])
def test_learn_matches_parent(parent, tmp_path, name, entry):
    got = run_case(name, tmp_path)
    fields = sorted(k.split("/", 1)[1] for k in parent.files if k.startswith(entry + "/"))
    assert fields == sorted(got)
    for k in fields:
        ref = parent[f"{entry}/{k}"]
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (name, k, got[k].shape, ref.shape)
        assert np.array_equal(got[k], ref), (name, k, got[k], ref)
    assert len(got["losses"]) == got["counters"][0] > 0 and len(got["test_scores"]) == 4
