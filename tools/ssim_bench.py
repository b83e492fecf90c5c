"""SSIM of the evaluation epochs (csrc/ren_metrics.hip, ops.ssim_planes) against a torch fp32 restatement of torchmetrics'
form (reflect pad, F.conv2d with the 11 x 11 window, crop, mean), at the evaluation sizes of the reference's datasets:

    260 x 346 x 50 views (DAVIS346 synthetic), 480 x 640 x 1 view, 800 x 800 x 3 channels x 200 views (Bayer, 800^2)

Prints ms per call (median of --iters, HIP events) for both, and the largest deviation of each from the float64
restatement (tests/ssim_reference.py).  GPU only.

    python tools/ssim_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ssim_reference as ref
from robust_e_nerf_amd import ops

DEV = "cuda:0"
CASES = [("260x346x50", 50, 260, 346), ("480x640x1", 1, 480, 640), ("800x800x3x200", 600, 800, 800)]


def torch_fp32(pred, target, data_range, w):
    p, t = pred[:, None], target[:, None]

    def filt(x):
        return torch.nn.functional.conv2d(torch.nn.functional.pad(x, (5, 5, 5, 5), mode="reflect"), w)[..., 5:-5, 5:-5]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mp, mt = filt(p), filt(t)
    vp, vt, cpt = filt(p * p) - mp * mp, filt(t * t) - mt * mt, filt(p * t) - mp * mt
    return (((2 * mp * mt + c1) * (2 * cpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))).mean((-3, -2, -1))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    g = ref.gauss()
    w = (g[:, None] * g[None, :]).float()[None, None].to(DEV)
    for name, P, H, W in CASES:
        gen = torch.Generator(device=DEV).manual_seed(P + H)
        t = torch.rand(P, H, W, generator=gen, device=DEV) * 0.9 + 1e-3
        p = (t + 0.05 * torch.randn(P, H, W, generator=gen, device=DEV)).clamp_min(1e-3)
        R = float(t.max())
        hip = ops.ssim_planes(p, t, R)
        f32 = torch_fp32(p, t, R, w)
        f64 = torch.cat([ref.ssim_planes_banded(p[i: i + 50], t[i: i + 50], R) for i in range(0, P, 50)])
        ms_hip = timed(lambda: ops.ssim_planes(p, t, R), args.iters)
        ms_f32 = timed(lambda: torch_fp32(p, t, R, w), args.iters)
        print(json.dumps(dict(case=name, planes=P, hip_ms=round(ms_hip, 4), torch_fp32_conv2d_ms=round(ms_f32, 4),
                              hip_max_dev_f64=float((hip - f64).abs().max()),
                              torch_fp32_max_dev_f64=float((f32.double() - f64).abs().max()))), flush=True)


if __name__ == "__main__":
    main()
