"""float64 restatements of torchmetrics.functional.ssim as the reference calls it (loss_metric/metric.py:74-81; torchmetrics
0.6.2 defaults: 11 x 11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03, reflect padding by 5, 5-pixel border crop before the
mean).  Shared by tests/test_ssim_cpu.py and tests/test_gpu_ssim.py."""
import numpy as np
import torch

K, R, SIGMA = 11, 5, 1.5


def gauss(dtype=torch.float64):
    """torchmetrics _gaussian(11, 1.5): exp(-((i - 5) / 1.5)^2 / 2), normalised to sum 1"""
    d = (torch.arange(K, dtype=torch.float64) - R) / SIGMA
    g = torch.exp(-0.5 * d * d)
    return (g / g.sum()).to(dtype)


def band(n: int, device="cpu") -> torch.Tensor:
    """(n - 10, n): row i holds the window at columns i .. i + 10 -- the filter over the valid windows as a matrix"""
    G = torch.zeros(n - 2 * R, n, dtype=torch.float64, device=device)
    g = gauss().to(device)
    for i in range(n - 2 * R):
        G[i, i: i + K] = g
    return G


def _ssim_map(filt, p, t, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mp, mt = filt(p), filt(t)
    vp, vt, cpt = filt(p * p) - mp * mp, filt(t * t) - mt * mt, filt(p * t) - mp * mt
    return ((2 * mp * mt + c1) * (2 * cpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))


def ssim_planes_banded(pred: torch.Tensor, target: torch.Tensor, data_range: float) -> torch.Tensor:
    """(P, H, W) -> (P,) float64 on the inputs' device: every filtered map is Gh X Gw^T over the valid windows"""
    p, t = pred.to(torch.float64), target.to(torch.float64)
    Gh, Gw = band(p.shape[-2], p.device), band(p.shape[-1], p.device)
    return _ssim_map(lambda x: Gh @ x @ Gw.T, p, t, data_range).mean((-2, -1))


def ssim_planes_padded_conv(pred: torch.Tensor, target: torch.Tensor, data_range: float) -> torch.Tensor:
    """torchmetrics' own form: reflect-pad by 5, 2-D convolution with the 11 x 11 window, crop 5 per border, mean"""
    p, t = pred.to(torch.float64)[:, None], target.to(torch.float64)[:, None]
    g = gauss()
    w = (g[:, None] * g[None, :])[None, None].to(p.device)

    def filt(x):
        y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (R, R, R, R), mode="reflect"), w)
        return y[..., R:-R, R:-R]
    return _ssim_map(filt, p, t, data_range).mean((-3, -2, -1))


def ssim_plane_direct(pred: np.ndarray, target: np.ndarray, data_range: float) -> float:
    """sliding 11 x 11 windows in numpy float64, one at a time (small images only)"""
    g = gauss().numpy()
    w = np.outer(g, g)
    p, t = pred.astype(np.float64), target.astype(np.float64)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    H, W = p.shape
    vals = []
    for y in range(H - 2 * R):
        for x in range(W - 2 * R):
            a, b = p[y: y + K, x: x + K], t[y: y + K, x: x + K]
            mp, mt = (w * a).sum(), (w * b).sum()
            vp, vt, cpt = (w * a * a).sum() - mp * mp, (w * b * b).sum() - mt * mt, (w * a * b).sum() - mp * mt
            vals.append(((2 * mp * mt + c1) * (2 * cpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2)))
    return float(np.mean(vals))
