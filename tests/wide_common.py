"""Shared pieces of the wide-row (more than 8 observables, 16-float node rows) N > 512 tests."""
import numpy as np
import torch

from oracle import mpnn_oracle as mo

N_OBS = 13  # MAIN_OBSERVABLES


def wide_net(seed, n_obs=N_OBS):
    """(weights dict on the host, MPNN(n_obs) on the GPU, the same weights on the GPU) from init_weights(std=0.1)."""
    from eco_hip.networks.mpnn import MPNN
    w = mo.init_weights(torch.Generator().manual_seed(seed), std=0.1, n_obs_in=n_obs)
    net = MPNN(n_obs_in=n_obs, device="cuda")
    net.load_state_dict(w)
    return w, net, {k: v.cuda() for k, v in w.items()}


def wide_x(seed, B, n, n_obs=N_OBS):
    """x [B, n, 16]: n_obs random columns in (-1, 1), column 0 set to +-1, the rest zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, n, 16)
    x[:, :, :n_obs] = torch.rand(B, n, n_obs, generator=g) * 2 - 1
    x[:, :, 0] = torch.where(x[:, :, 0] > 0, 1.0, -1.0)
    return x


def oracle_q(wc, xb, J, n_obs=N_OBS):
    """The fp32 torch oracle on the GPU for ONE episode: node rows xb [n, 16] (device), dense adjacency J (numpy)."""
    adj = torch.from_numpy(np.asarray(J)).float().cuda().unsqueeze(0)
    obs = torch.cat([xb[None, :, :n_obs].transpose(1, 2), adj], dim=1)
    with torch.no_grad():
        return mo.forward(wc, obs, n_obs_in=n_obs).reshape(-1)


def scaled_err(q, ref, what):
    e = float(((q - ref).abs() / (1 + ref.abs())).max())
    print(f"{what}: scaled err {e:.3e}")
    return e
