"""Cost of fusing depth maps into a truncated signed distance lattice (csrc/ren_tsdf.hip, ops.tsdf_integrate).

  - ren_tsdf_integrate for lattices of --resolutions points a side (default 128, 256) over [-0.5, 0.5]^3 and --views (default 16,
    64) synthetic views of --size (default 480 x 640) of a sphere of radius 0.3: cameras on two rings at distance 1.5 looking
    at the centre, f = 500, analytic z-depth, +inf off the sphere.  Device events around the call, --repeats warm runs: median,
    min, max, and projections (lattice points x views) per second.  Before anything is timed the result is compared with a
    second call (`torch.equal`).
  - the same views in calls of 16 (what tsdf.fuse_renders does): the depth maps one call gathers from stay smaller, at the price
    of reading and writing the lattice once a call.
  - the same call with the depth maps shrunk to 15 x 20 pixels and the intrinsics scaled with them: the same arithmetic per
    projection, but a gather that stays in the nearest cache.  The difference between the two times is what the depth gather
    costs beyond its instructions; what is left is arithmetic, the divisions and the loop.
  - a torch restatement of the same function on the GPU, one view at a time, every step a torch operation over the whole
    lattice: none of the new code.  Its sum and count are compared with the kernel's.
Nothing is fixed in advance; the file records what was measured.  GPU only.

    python tools/tsdf_bench.py [--resolutions 128 256] [--views 16 64] [--repeats 7]
"""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from robust_e_nerf_amd import mesh, ops, tsdf
from mesh_bench import DEV, HI, LO, RADIUS, device_ms, stats

DISTANCE, FOCAL, Z_MIN = 1.5, 500.0, 1e-6


def ring_cameras(n):
    """n cameras on two rings at DISTANCE from the origin looking at it -> cam_pos (n, 3), cam_rot (n, 3, 3) float64 on the host"""
    pos, rot = [], []
    for k in range(n):
        h = 0.5 if k % 2 == 0 else -0.5
        phi = 2.0 * math.pi * k / n
        c = torch.tensor([math.sqrt(1 - h * h) * math.cos(phi), math.sqrt(1 - h * h) * math.sin(phi), h], dtype=torch.float64) * DISTANCE
        fwd = -c / c.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        right = right / right.norm()
        pos.append(c)
        rot.append(torch.stack([right, torch.linalg.cross(fwd, right), fwd], dim=1))
    return torch.stack(pos), torch.stack(rot)


def pinhole(height, width, focal):
    return torch.tensor([[focal, 0.0, (width - 1) / 2.0], [0.0, focal, (height - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float32)


def sphere_depth(cam_pos, cam_rot, K, height, width):
    """(V, H, W) float32 on the device: z-depth of the sphere through every pixel centre, +inf off it (float64 geometry)"""
    K = K.to(DEV, torch.float64)
    ys, xs = torch.meshgrid(torch.arange(height, device=DEV, dtype=torch.float64), torch.arange(width, device=DEV, dtype=torch.float64),
                            indexing="ij")
    yn = (ys - K[1, 2]) / K[1, 1]
    xn = (xs - K[0, 2] - K[0, 1] * yn) / K[0, 0]
    cam = torch.stack([xn, yn, torch.ones_like(xn)], dim=-1)
    out = []
    for c, R in zip(cam_pos.to(DEV), cam_rot.to(DEV)):
        d = cam @ R.t()
        a, b, cc = (d * d).sum(-1), 2.0 * (d @ c), c @ c - RADIUS * RADIUS
        disc = b * b - 4.0 * a * cc
        tt = (-b - torch.sqrt(disc.clamp_min(0.0))) / (2.0 * a)
        out.append(torch.where((disc >= 0) & (tt > 0), tt, torch.full_like(tt, math.inf)).to(torch.float32))
    return torch.stack(out).contiguous()


def torch_integrate(depth, cams, K, pts, trunc, z_min, total, count):
    """the header's steps 2 - 11 as torch operations over all lattice points, one view at a time; pts (n, 3) float32"""
    k00, k01, k02, k11, k12 = float(K[0, 0]), float(K[0, 1]), float(K[0, 2]), float(K[1, 1]), float(K[1, 2])
    height, width = depth.shape[1:]
    for v in range(depth.shape[0]):
        c, R = cams[v, :3], cams[v, 3:].view(3, 3)
        d = pts - c
        q = [(R[0, a] * d[:, 0] + R[1, a] * d[:, 1]) + R[2, a] * d[:, 2] for a in range(3)]
        z = q[2]
        xn, yn = q[0] / z, q[1] / z
        fu = torch.floor(((k00 * xn + k01 * yn) + k02) + 0.5)
        fv = torch.floor((k11 * yn + k12) + 0.5)
        ok = (z > z_min) & (fu >= 0) & (fu < width) & (fv >= 0) & (fv < height)
        pix = torch.where(ok, fv, torch.zeros_like(fv)).long() * width + torch.where(ok, fu, torch.zeros_like(fu)).long()
        D = depth[v].reshape(-1)[pix]
        s = D - z
        ok &= (D > 0) & ~(s < -trunc)
        term = torch.where(s >= trunc, torch.ones_like(s), s / torch.full_like(s, trunc))   # by a tensor: torch multiplies by the
        #                                                                                      reciprocal of a host scalar
        total += torch.where(ok, term, torch.zeros_like(term))
        count += ok.to(torch.int32)


def bench_case(res, n_views, height, width, warmup, repeats):
    cam_pos, cam_rot = ring_cameras(n_views)
    K = pinhole(height, width, FOCAL)
    depth = sphere_depth(cam_pos, cam_rot, K, height, width)
    cams = tsdf.pack_cameras(cam_pos, cam_rot).to(DEV)
    grid = (res, res, res)
    trunc = tsdf.default_trunc(LO, HI, grid)
    zeros = lambda: (torch.zeros(grid, device=DEV), torch.zeros(grid, device=DEV, dtype=torch.int32))
    run = lambda dm, k, st: ops.tsdf_integrate(dm, cams, k, LO, HI, grid, trunc, Z_MIN, *st)
    first, second = zeros(), zeros()
    run(depth, K, first)
    run(depth, K, second)
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1])
    projections = res ** 3 * n_views
    rate = lambda st: round(projections / (1e-3 * st["median_ms"]) / 1e9, 3)
    scratch = zeros()
    kernel = stats(device_ms(lambda: run(depth, K, scratch), warmup, repeats))
    per_call = ops.TSDF_VIEW_BATCH

    def in_calls():                                                                 # what tsdf.fuse_renders does: views_per_call at a time
        for v0 in range(0, n_views, per_call):
            ops.tsdf_integrate(depth[v0: v0 + per_call], cams[v0: v0 + per_call], K, LO, HI, grid, trunc, Z_MIN, *scratch)
    split = stats(device_ms(in_calls, warmup, repeats))
    small_h, small_w = max(1, height // 32), max(1, width // 32)
    small_K = pinhole(small_h, small_w, FOCAL / 32.0)
    small = sphere_depth(cam_pos, cam_rot, small_K, small_h, small_w)
    cached = stats(device_ms(lambda: run(small, small_K, scratch), warmup, repeats))
    pts = mesh.lattice_points(LO, HI, grid, 0, res ** 3, DEV)
    t_state = zeros()
    torch_integrate(depth, cams, K, pts, trunc, Z_MIN, t_state[0].view(-1), t_state[1].view(-1))
    t_scratch = zeros()
    restated = stats(device_ms(lambda: torch_integrate(depth, cams, K, pts, trunc, Z_MIN, t_scratch[0].view(-1), t_scratch[1].view(-1)),
                               1, max(3, repeats // 2)))
    out = dict(resolution=res, views=n_views, image=[height, width], trunc=trunc, projections=projections,
               observed_points=int((first[1] > 0).sum()), mean_views_per_point=float(first[1].double().mean()),
               depth_bytes=int(depth.numel() * 4), lattice_bytes_read_and_written=int(res ** 3 * 16),
               kernel=kernel, gprojections_per_s=rate(kernel),
               kernel_in_calls_of_16_views=split, gprojections_per_s_in_calls_of_16_views=rate(split),
               kernel_depth_maps_of_15x20=cached, gprojections_per_s_depth_maps_of_15x20=rate(cached),
               torch_restatement=restated, gprojections_per_s_torch=rate(restated),
               speedup_over_torch=round(restated["median_ms"] / kernel["median_ms"], 2),
               torch_count_equal=bool(torch.equal(t_state[1], first[1])),
               torch_sum_bits_equal=bool(torch.equal(t_state[0].view(torch.int32), first[0].view(torch.int32))),
               torch_sum_max_abs_difference=float((t_state[0] - first[0]).abs().max()))
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_bench needs the GPU"
    torch.cuda.set_device(0)
    results = dict(device=torch.cuda.get_device_name(0), view_batch=ops.TSDF_VIEW_BATCH, cases={},
                   not_measured="kernel times from a profiler trace (device events around the call instead, which include the "
                                "launch); hardware counters; depth maps of a trained field (these are of an analytic sphere); "
                                "cameras inside the lattice; sizes other than those listed")
    for res in args.resolutions:
        for n_views in args.views:
            results["cases"][f"{res}_v{n_views}"] = bench_case(res, n_views, args.size[0], args.size[1], args.warmup, args.repeats)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
