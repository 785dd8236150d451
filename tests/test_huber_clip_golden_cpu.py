"""The reference's own Huber / clipped train steps (tests/golden/dqn_step_huber_clip*.npz) against a float64
restatement: oracle.mpnn_oracle.forward on float64 weights, torch autograd, F.smooth_l1_loss and
clip_grad_norm_ (dqn.py:403-447).  Each step starts from the weights the reference recorded before it, so the
restatement needs no optimiser.  The fixture pins the restatement; the GPU tests lean on the fixture.

Bars are those of tests/test_oracle_golden.py for its restated train step: loss (and here the norm, a scalar of the
same kind) within 1e-6 * max(1, |x|), gradients within rtol 1e-4 / atol 1e-7.  The recorder's two conditions are
re-asserted from the files: 25-75 % of every step's samples on the linear branch, and over the clipped agents a step
with total_norm > c and one with total_norm < c."""
import numpy as np
import torch
import torch.nn.functional as F

from huber_clip_common import clipped_agents, load_golden
from oracle import mpnn_oracle as mo


def _step(f, w, tw, s, max_norm):
    """One restated train step up to (and including) clip_grad_norm_: loss, d, total norm, gradients."""
    p = f"s{s}/"
    dbl = lambda a: torch.from_numpy(a).float().double()   # noqa: E731  (the reference's .float() cast first)
    states, nxt = dbl(f[p + "states"]), dbl(f[p + "states_next"])
    actions = torch.from_numpy(f[p + "actions"])
    rewards, dones = dbl(f[p + "rewards"]), dbl(f[p + "dones"])
    with torch.no_grad():
        a_star = mo.forward(w, nxt).argmax(1, True)
        q_t = mo.forward(tw, nxt).gather(1, a_star)
    td = rewards + (1 - dones) * float(f["gamma"]) * q_t
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    q = mo.forward(wg, states).gather(1, actions)
    loss = F.smooth_l1_loss(q, td, reduction="mean")
    loss.backward()
    norm = None
    if max_norm is not None:
        norm = float(torch.nn.utils.clip_grad_norm_([wg[k] for k in mo.KEYS], max_norm))
    return float(loss.detach()), (q - td).detach()[:, 0].numpy(), norm, {k: wg[k].grad for k in mo.KEYS}


def _close(got, ref):
    return abs(got - ref) <= 1e-6 * max(1.0, abs(ref))


def test_restatement_reproduces_reference_huber_and_clip_steps():
    f = load_golden()
    steps = int(f["steps"])
    tw = {k: torch.from_numpy(f["target/" + k]).double() for k in mo.KEYS}
    agents = ["huber/"] + clipped_agents(f)
    assert len(agents) >= 2
    norms = []
    for a in agents:
        c = float(f[a + "max_grad_norm"]) if a != "huber/" else None
        for s in range(steps):
            prev = "w0/" if s == 0 else f"{a}s{s - 1}/w/"
            w = {k: torch.from_numpy(f[prev + k]).double() for k in mo.KEYS}
            loss, d, norm, grad = _step(f, w, tw, s, c)
            assert _close(loss, float(f[f"{a}s{s}/loss"])), (a, s, loss, float(f[f"{a}s{s}/loss"]))
            frac = float((np.abs(d) >= 1).mean())
            assert 0.25 <= frac <= 0.75 and frac == float(f[f"{a}s{s}/frac_linear"]), (a, s, frac)
            if c is None:
                continue
            ref_norm = float(f[f"{a}s{s}/norm"])
            assert _close(norm, ref_norm), (a, s, norm, ref_norm)
            norms.append((ref_norm, c))
            if s == 0:
                for k in mo.KEYS:
                    torch.testing.assert_close(grad[k].float(), torch.from_numpy(f[f"{a}s0/grad/" + k]),
                                               rtol=1e-4, atol=1e-7, msg=lambda m: f"{a} {k}: {m}")
    assert any(n > c for n, c in norms) and any(n < c for n, c in norms), norms


def test_fixture_files_fit_the_size_limit():
    import glob
    import os
    from conftest import GOLDEN
    files = glob.glob(os.path.join(GOLDEN, "dqn_step_huber_clip*.npz"))
    assert len(files) >= 3
    assert all(os.path.getsize(p) < (1 << 20) for p in files), {p: os.path.getsize(p) for p in files}
