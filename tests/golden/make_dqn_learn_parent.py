"""Recorder of tests/golden/dqn_learn_parent.npz.  Run on an MI355X at commit fbddfea (the parent of the
commit that split the DQN class) with the cases of tests/dqn_refactor_cases.py:

    python tests/golden/make_dqn_learn_parent.py [OUT.npz]

Training is deterministic run to run: two recordings at that commit were identical array for array."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "eco-dqn_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from dqn_refactor_cases import CASES, run_case  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dqn_learn_parent.npz")
    data = {}
    for name in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            for k, v in run_case(name, tmp).items():
                data[f"{name}/{k}"] = v
        print(name, "losses", len(data[f"{name}/losses"]), "scores", data[f"{name}/test_scores"].tolist(),
              "counters", data[f"{name}/counters"].tolist(), flush=True)
    np.savez_compressed(out, **data)
    print("recorded", len(data), "arrays to", out)
