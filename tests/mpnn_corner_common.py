"""Shared pieces of tests/test_mpnn_corners_gpu.py: a case (graphs of a store, observables, weights, node rows, graph
ids, dq), its float64 judge (oracle.mpnn_oracle.forward_staged and its autograd), the fp32 oracle's own error in the
same metrics (which sets the derived bars), the device run, and the stage print-out of a failing case.

Bars: Q |q - q64| <= 5e-7 (1 + |q64|) and relative L2 < 1e-5 per gradient tensor (the project's bars); per input
column of the two narrow Linears and per element of the two readout tensors 4 x the fp32 oracle's worst figure over
the module's cases, never below 1e-5; saved activations 4 x the fp32 oracle's worst on that case, never below 5e-7.
"""
import numpy as np
import torch

from oracle import mpnn_oracle as mo

Q_BAR = 5e-7
GRAD_BAR = 1e-5
SENTINEL = 1e3          # in the dead columns of the 8- / 16-float node rows: a kernel that reads one shows
W0, WE, WR, BR = mo.KEYS[0], mo.KEYS[1], mo.KEYS[10], mo.KEYS[11]
NODE_STAGES = ["H0", "H1", "H2", "H3", "E", "EAGG", "M0", "M1", "M2", "AGG0", "AGG1", "AGG2"]  # SV_* order
RELU_STAGES = ["H0", "H1", "H2", "H3", "E", "M0", "M1", "M2"]


def graphs_per_block(N, B, cus=None):
    """eco::graphs_per_block of csrc/eco_mpnn.h restated (a change there must find this test)."""
    if cus is None:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    gmax = 1 if N >= 208 else 208 // N
    best, best_cost = gmax, 1e300
    g = gmax
    while g >= 1 and 2 * g >= gmax:
        tiles = (g * N + 15) // 16
        blocks = (B + g - 1) // g
        cost = float((blocks + cus - 1) // cus) * ((tiles + 3) // 4 + 1)
        if cost < best_cost:
            best_cost, best = cost, g
        g -= 1
    return best


class Case:
    """mats: the store's graphs (dense, symmetric); gids: the batch's graph ids into it (default: every graph
    once); dq: "dense" (Gaussian) or "onehot" (one nonzero per row, as eco_dqn_td writes it; zero_row: a row
    left entirely zero)."""

    def __init__(self, name, mats, n_obs, seed, gids=None, dq="dense", zero_row=None):
        self.name, self.mats, self.n_obs, self.seed = name, [np.asarray(m, np.float64) for m in mats], n_obs, seed
        self.gids = list(range(len(mats))) if gids is None else list(gids)
        self.B, self.N = len(self.gids), self.mats[0].shape[0]
        assert all((m != 0).any() and (m == m.T).all() for m in self.mats), "every graph needs an edge"
        g = torch.Generator().manual_seed(seed)
        self.w = mo.init_weights(g, std=0.1, n_obs_in=n_obs)
        W = 8 if n_obs <= 8 else 16
        x = torch.full((self.B, self.N, W), SENTINEL)
        live = torch.rand(self.B, self.N, n_obs, generator=g) * 2 - 1
        live = torch.where(live.abs() < 1e-3, torch.full_like(live, 0.5), live)   # every live entry nonzero
        live[:, :, 0] = torch.where(live[:, :, 0] > 0, 1.0, -1.0)
        x[:, :, :n_obs] = live
        self.x = x
        if dq == "dense":
            self.dq = torch.randn(self.B, self.N, generator=g)
        else:
            col = torch.randint(0, self.N, (self.B,), generator=g)
            mag = torch.randn(self.B, generator=g)
            mag = torch.where(mag.abs() < 0.1, torch.full_like(mag, 0.7), mag)
            self.dq = torch.zeros(self.B, self.N)
            self.dq[torch.arange(self.B), col] = mag
            if zero_row is not None:
                self.dq[zero_row] = 0.0
        self.zero_row = zero_row
        self._ref = None

    def without_row(self, r):
        """The same case with batch row r removed (same weights, node rows and dq of the other rows)."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        keep = [i for i in range(self.B) if i != r]
        c.name, c.gids, c.B = self.name + f" without row {r}", [self.gids[i] for i in keep], self.B - 1
        c.x, c.dq, c.zero_row, c._ref = self.x[keep].contiguous(), self.dq[keep].contiguous(), None, None
        return c

    def adj(self):
        """float64 [B, N, N] of the batch, on the f32-rounded weights: the kernels read (float)edge_weights[q] and
        the network takes obs.float() (dqn.py:282), as test_weighted_mpnn_gpu's judge does.  Exact for integers."""
        return torch.from_numpy(np.stack([self.mats[g] for g in self.gids])).float().double()


def _autograd(case, dtype, device):
    w = {k: v.to(device, dtype).requires_grad_(True) for k, v in case.w.items()}
    x = case.x[:, :, :case.n_obs].to(device, dtype)
    q, _ = mo.forward_staged(w, x, case.adj().to(device, dtype), case.n_obs)
    (q.reshape(case.B, case.N) * case.dq.to(device, dtype)).sum().backward()
    return q.detach().reshape(case.B, case.N).cpu(), {k: w[k].grad.detach().cpu() for k in mo.KEYS}


def stages(case, dtype, device="cpu"):
    """Q and the SV_*-named intermediates plus the pre-activations Z_* of the ReLU stages."""
    with torch.no_grad():
        w = {k: v.to(device, dtype) for k, v in case.w.items()}
        x = case.x[:, :, :case.n_obs].to(device, dtype)
        q, st = mo.forward_staged(w, x, case.adj().to(device, dtype), case.n_obs)
        z = {"H0": x @ w[mo.KEYS[0]].T, "E": st["EAGG"] @ w[mo.KEYS[2]].T}
        for i in range(3):
            z[f"M{i}"] = torch.cat([st[f"AGG{i}"], st["E"]], -1) @ w[mo.KEYS[3 + 2 * i]].T
            z[f"H{i + 1}"] = torch.cat([st[f"H{i}"], st[f"M{i}"]], -1) @ w[mo.KEYS[4 + 2 * i]].T
    return q.reshape(case.B, case.N).cpu(), {k: v.cpu() for k, v in st.items()}, {k: v.cpu() for k, v in z.items()}


def column_err(got, ref):
    """Worst relative L2 of one input column (one feature) of a narrow Linear's gradient; columns whose float64
    norm is below 1e-6 of the tensor's are skipped."""
    got, ref = got.double(), ref.double()
    total, worst = float(ref.norm()), 0.0
    for j in range(ref.shape[1]):
        nj = float(ref[:, j].norm())
        if nj < 1e-6 * total:
            continue
        worst = max(worst, float((got[:, j] - ref[:, j]).norm()) / nj)
    return worst


def element_err(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def scaled_err(got, ref):
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (1 + ref.abs())).max())


def fine_figures(grads, ref):
    """(worst column figure of the two narrow Linears, worst element figure of the two readout tensors)."""
    return (max(column_err(grads[W0], ref[W0]), column_err(grads[WE], ref[WE])),
            max(element_err(grads[WR], ref[WR]), element_err(grads[BR], ref[BR])))


def reference(case, device=None):
    """float64 Q and gradients of (q * dq).sum() (cached on the case), and the fp32 CPU oracle's figures in the
    two fine metrics.  float64 runs on the GPU above 300 vertices, as test_dense_large_matches_csr_and_oracle."""
    if case._ref is None:
        if device is None:
            device = "cuda" if case.N > 300 else "cpu"
        q64, g64 = _autograd(case, torch.float64, device)
        q32, g32 = _autograd(case, torch.float32, "cpu")
        case._ref = {"q": q64, "grad": g64, "fp32": fine_figures(g32, g64), "fp32_q": scaled_err(q32, q64)}
    return case._ref


def flat_to_dict(flat, n_obs):
    from eco_hip.networks.mpnn import param_layout
    out, off = {}, 0
    for name, shape in param_layout(n_obs):
        k = int(np.prod(shape))
        out[name] = flat[off:off + k].reshape(shape)
        off += k
    assert off == flat.numel()
    return out


def make_store(case):
    from eco_hip.graphs import GraphStore
    return GraphStore.from_dense(case.mats)


def run_device(case, mask=0, store=None):
    """Saving forward (ECO_NORM_PER_CALL) + backward with a caller-owned workspace, twice: the two gradients must
    be bitwise equal.  Returns Q, the flat gradient and the saved buffer of the first forward (host tensors)."""
    from eco_hip import _lib
    from eco_hip.networks.mpnn import MPNN
    store = make_store(case) if store is None else store
    net = MPNN(n_obs_in=case.n_obs, device="cuda")
    net.load_state_dict(case.w)
    x, dq = case.x.cuda(), case.dq.cuda()
    gids = torch.tensor(case.gids, dtype=torch.int32, device="cuda")
    B, N = case.B, case.N
    ws = torch.empty(_lib.lib.eco_mpnn_backward_workspace_bytes(N, B), dtype=torch.uint8, device="cuda")
    with _lib.kernel_paths(mask):
        saved = torch.zeros(MPNN.saved_bytes(N, B), dtype=torch.uint8, device="cuda")
        q = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL, saved=saved).clone()
        grad = torch.zeros_like(net.flat)
        net.backward_graphs(x, store, gids, saved, dq, grad, workspace=ws)
        saved1 = saved.clone()
        q2 = net.forward_graphs(x, store, gids, norm_scope=_lib.ECO_NORM_PER_CALL, saved=saved)
        grad2 = torch.zeros_like(net.flat)
        net.backward_graphs(x, store, gids, saved, dq, grad2, workspace=ws)
        torch.cuda.synchronize()
    store.check_errors()
    assert torch.equal(q, q2) and torch.equal(saved, saved1), case.name
    assert torch.equal(grad, grad2), case.name + ": the backward is not bitwise reproducible"
    assert torch.isfinite(q).all() and torch.isfinite(grad).all(), case.name
    return q.cpu(), grad.cpu(), saved1.cpu()


def saved_tensors(saved, B, N):
    """The f32 rows of the saved-activation buffer by name.  Layout: SV_* and sv_mask_offset_floats of
    csrc/eco_mpnn.h -- [SV_NODE_TENSORS][B * N][64] floats in SV_* order, then MEAN [B][64], then P [B][64]
    (the ReLU masks of the dense path follow and are not read here)."""
    RT = B * N
    f = saved.view(torch.float32)
    n_node = len(NODE_STAGES)                         # SV_NODE_TENSORS
    assert f.numel() >= n_node * RT * 64 + 2 * B * 64     # sv_mask_offset_floats(RT, B)
    out = {k: f[i * RT * 64:(i + 1) * RT * 64].reshape(B, N, 64) for i, k in enumerate(NODE_STAGES)}
    base = n_node * RT * 64
    out["MEAN"] = f[base:base + B * 64].reshape(B, 64)
    out["P"] = f[base + B * 64:base + 2 * B * 64].reshape(B, 64)
    return out


def stage_report(case, saved):
    """Per saved tensor: the scaled error of the device's f32 rows against float64, the number of ReLU outputs
    whose sign disagrees with float64 and the smallest / largest |z64| among those relative to the tensor's max
    (a disagreement only below 1e-6 of the max is a rounding tie: another seed; anything else is a kernel bug)."""
    _, st64, z64 = stages(case, torch.float64, "cuda" if case.N > 300 else "cpu")
    dev = saved_tensors(saved, case.B, case.N)
    lines, only_ties = [], True
    for k in NODE_STAGES + ["MEAN", "P"]:
        line = f"  {k:5s} scaled err {scaled_err(dev[k], st64[k]):.3e}"
        if k in RELU_STAGES:
            bad = (dev[k] > 0) != (z64[k] > 0)
            n_bad = int(bad.sum())
            line += f"  ReLU sign disagreements {n_bad}"
            if n_bad:
                zmax = float(z64[k].abs().max())
                zb = z64[k].abs()[bad]
                line += f", |z64| / max in [{float(zb.min()) / zmax:.2e}, {float(zb.max()) / zmax:.2e}]"
                only_ties = only_ties and float(zb.max()) < 1e-6 * zmax
        lines.append(line)
    lines.append("  every sign disagreement is a rounding tie (|z64| < 1e-6 max): " + str(only_ties))
    return "\n".join(lines)


def check_case(case, mask=0, fine_bars=None, store=None):
    """Run the case on the device and judge it against float64.  fine_bars: (column bar, readout element bar).
    Returns (q, flat grad, saved) of the device for cross-checks between kernel-path masks."""
    ref = reference(case)
    q, grad, saved = run_device(case, mask, store)
    gd = flat_to_dict(grad, case.n_obs)
    fails = []
    qe = scaled_err(q, ref["q"])
    print(f"{case.name} [mask {mask}]: Q scaled err {qe:.3e} (fp32 oracle {ref['fp32_q']:.3e}, bar {Q_BAR:.0e})")
    if not qe <= Q_BAR:
        fails.append(("Q", qe))
    worst = 0.0
    for k in mo.KEYS:
        r = ref["grad"][k]
        err = float((gd[k].double() - r).norm() / max(float(r.norm()), 1e-300))
        worst = max(worst, err)
        if not err < GRAD_BAR:
            fails.append((k, err))
    col, el = fine_figures(gd, ref["grad"])
    print(f"  gradients: worst relative L2 {worst:.3e} (bar {GRAD_BAR:.0e}); worst column {col:.3e} (fp32 oracle "
          f"{ref['fp32'][0]:.3e}); worst readout element {el:.3e} (fp32 oracle {ref['fp32'][1]:.3e})")
    if fine_bars is not None:
        print(f"  derived bars: column {fine_bars[0]:.3e}, readout element {fine_bars[1]:.3e}")
        if not col <= fine_bars[0]:
            fails.append(("column", col))
        if not el <= fine_bars[1]:
            fails.append(("readout element", el))
    if fails:
        print(f"{case.name} [mask {mask}] FAILED {fails}; device rows against the float64 stages:")
        print(stage_report(case, saved))
    assert not fails, (case.name, mask, fails)
    return q, grad, saved
