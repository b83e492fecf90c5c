"""Times of the encoder's input-gradient kernel and of a normal-map render.

    python tools/normals_bench.py [--n 1048576] [--out profiles/normals_bench.json]

In one process, on the same 2^20 points (a trained-like table of order 1, points uniform in the unit cube, so the fine levels
miss every cache): ren_hashgrid_bwd_input, ren_hashgrid_fwd and the three-launch JVP construction of tcnn_api; then
render_normal_image beside render_image at 640 x 480 on the synthetic benchmark field.  Each figure is the median of 20
timed launches after 5 warm-up launches, timed with device events around each launch."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out")
    args = ap.parse_args()
    from robust_e_nerf_amd import engine, evaluation, ops, tcnn_api
    dev = "cuda:0"
    n = args.n
    g = torch.Generator(device=dev).manual_seed(0)
    grid, n_table = ops.make_grid_desc()
    table = torch.rand(n_table, device=dev, generator=g) * 2 - 1
    x = torch.rand(n, 3, device=dev, generator=g)
    dfeat = torch.randn(ops.n_blocks32(n) * 1024, device=dev, generator=g)
    rows = tcnn_api._to_rows(dfeat, n).contiguous()
    out = torch.empty(n, 3, device=dev)
    feat = torch.empty(ops.n_blocks32(n) * 1024, device=dev)
    mod = types.SimpleNamespace(grid=grid, unit_scene=ops.make_scene_desc([0, 0, 0, 1, 1, 1], ops.AABB))
    units = []
    for k in range(3):
        e = torch.zeros_like(x)
        e[:, k] = 1.0
        units.append(e)

    def jvp3():
        return torch.stack([(tcnn_api._encode_with_tangent(mod, table, x, e)[1] * rows).sum(-1) for e in units], -1)

    res = dict(n=n)
    res["bwd_input_ms"] = timed(lambda: ops.hashgrid_bwd_input(grid, table, dfeat, x_unit=x, n=n, layout=1, out=out))
    res["bwd_input_rows_ms"] = timed(lambda: ops.hashgrid_bwd_input(grid, table, rows, x_unit=x, n=n, layout=0, out=out))
    res["fwd_ms"] = timed(lambda: ops.hashgrid_fwd(grid, table, x_unit=x, n=n, layout=1, out=feat))
    res["jvp3_ms"] = timed(jvp3)
    # compulsory bytes: 128 B of dfeat + 12 B of position in, 12 B out per sample, plus the table entries touched at least once
    # (at most the whole table, 128 corner entries of 8 B per sample)
    touched = min(n_table * 4, n * 128 * 8)
    res["compulsory_bytes"] = n * (128 + 12 + 12) + touched
    res["gather_bytes_requested"] = n * 128 * 8
    res["bwd_input_GBps_compulsory"] = res["compulsory_bytes"] / res["bwd_input_ms"][0] / 1e6

    # the scene of tools/render_bench.py: a ball of occupied cells seen from 4 units away, 640 x 480, one chunk
    import math
    import numpy as np
    import bench
    H, W = 480, 640
    gen = torch.Generator().manual_seed(0)

    def lin(o, i):
        b = 1 / math.sqrt(i)
        return (torch.rand(o, i, generator=gen) * 2 - 1) * b, (torch.rand(o, generator=gen) * 2 - 1) * b
    p = {}
    p["base.w0"], p["base.b0"] = lin(64, 32); p["base.wo"], p["base.bo"] = lin(16, 64)
    p["head.w0"], p["head.b0"] = lin(64, 31); p["head.w1"], p["head.b1"] = lin(64, 64); p["head.wo"], p["head.bo"] = lin(1, 64)
    p["hash"] = (torch.rand(n_table, generator=gen) * 2 - 1) * 0.1
    fld = engine.NGPField(dev)
    fld.load(p)
    aabb = (-1.5,) * 3 + (1.5,) * 3
    r = engine.Renderer(fld, engine.RenderCfg(aabb=aabb, sampler="occgrid"))
    r.binary.copy_(torch.from_numpy(bench.ball_binary(128, 0.42, aabb)).to(dev))
    K = np.array([[480.0 * W / 346, 0, W / 2 - 0.5], [0, 480.0 * W / 346, H / 2 - 0.5], [0, 0, 1]])
    Kinv = torch.from_numpy(np.linalg.inv(K)).float().to(dev)
    pos = torch.tensor([4.0, 0.0, 0.3], device=dev)
    z = -pos / pos.norm()
    xa = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], device=dev), z)
    xa = xa / xa.norm()
    rot = torch.stack([xa, torch.linalg.cross(z, xa), z], 1).contiguous()
    res["render_image_ms"] = timed(lambda: evaluation.render_image(r, Kinv, pos, rot, H, W), warm=3, reps=10)
    res["render_normal_image_ms"] = timed(lambda: evaluation.render_normal_image(r, Kinv, pos, rot, H, W), warm=3, reps=10)
    ops.profile_start()
    evaluation.render_normal_image(r, Kinv, pos, rot, H, W)
    res["render_normal_image_kernels_ms"] = {k: round(v[1], 4) for k, v in ops.profile_stop().items()}
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
