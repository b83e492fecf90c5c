"""Cost of the exact nearest-neighbour search behind the mesh distances (csrc/ren_mesh_distance.hip, mesh_distance.nearest), and
the geometric error of mesh.simplify measured with it.

  - `nearest` at --sizes points a side (default 2^16, 2^18, 2^20): samples of two icospheres (five subdivisions, radius 1 and
    1.01), each direction's result compared with a second call (`torch.equal`) before anything is timed; the whole call (host
    clock around a call that ends in a device synchronise: the sorts, the grouping, the search, one read-back) and the search
    kernel alone on the grouped input (device events), over --repeats warm runs: median, min, max.  The grid and the number of
    its cells that hold a reference are recorded with them.
  - the baseline at 2^16 x 2^16: a chunked torch brute force, |q|^2 - 2 q.p^T + |p|^2 and argmin per chunk of queries: none
    of the new code.  Its distances are another rounding of the same numbers, so its indices are compared as a share.
  - mesh.simplification_error (the scores export's simplify_error reports, with the floor the sampling sets) at k = --k
    (default 1.5, 2, 4) on the mesh mesh.extract makes of tools/mesh_bench.py's analytic sphere at --resolution (default 256),
    for each of --samples (default 10^6 and 1.6 10^7) points a surface.
Nothing is fixed in advance; the file records what was measured.  GPU only.

    python tools/mesh_distance_bench.py [--sizes 65536 262144 1048576] [--k 1.5 2 4] [--repeats 7]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from robust_e_nerf_amd import mesh, mesh_distance, ops
from mesh_bench import DEV, HI, LO, device_ms, sphere, stats, wall_s


def icosphere(level, radius):
    t = (1 + math.sqrt(5)) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []
        for a, b, c in f:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in mid:
                    s = v[i] + v[j]
                    v.append(s / np.linalg.norm(s))
                    mid[key] = len(v) - 1
                m.append(mid[key])
            nf += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = nf
    return torch.from_numpy((radius * np.array(v)).astype(np.float32)).to(DEV), torch.from_numpy(np.array(f, np.int32)).to(DEV)


def wall_ms(fn, warmup, repeats):
    return [1e3 * t for t in wall_s(fn, warmup, repeats)]


def brute(q, p, chunk=4096):
    d2 = torch.empty(q.shape[0], device=q.device)
    idx = torch.empty(q.shape[0], device=q.device, dtype=torch.int64)
    pp = (p * p).sum(-1)
    for s in range(0, q.shape[0], chunk):
        c = q[s: s + chunk]
        d = (c * c).sum(-1, keepdim=True) - 2.0 * (c @ p.t()) + pp
        d2[s: s + chunk], idx[s: s + chunk] = torch.min(d, dim=1)
    return d2, idx


def grouped(q, p):
    """the inputs of the search kernel as nearest builds them, and the records a query reads on average"""
    lo, hi = torch.aminmax(p, dim=0)
    lo = lo.tolist()
    h, grid = mesh_distance.nn_grid(lo, hi.tolist(), p.shape[0])
    cells, order = torch.sort(ops.nn_cells(p, lo, h, grid), stable=True)
    n_cells = grid[0] * grid[1] * grid[2]
    start = torch.searchsorted(cells, torch.arange(n_cells + 1, device=DEV, dtype=torch.int32), out_int32=True)
    rec = torch.cat([p[order].view(torch.int32), order.to(torch.int32)[:, None]], dim=1).contiguous().view(torch.float32)
    qs = q[torch.sort(ops.nn_cells(q, lo, h, grid), stable=True).indices].contiguous()
    return qs, rec, start, lo, h, grid, int((start[1:] != start[:-1]).sum())


def bench_nearest(n, warmup, repeats):
    a, b = icosphere(5, 1.0), icosphere(5, 1.01)
    q, p = mesh_distance.sample_surface(*a, n, 0), mesh_distance.sample_surface(*b, n, 1)
    first, second = mesh_distance.nearest(q, p), mesh_distance.nearest(q, p)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    qs, rec, start, lo, h, grid, occupied = grouped(q, p)
    out = dict(points_a_side=n, grid=list(grid), h=h, occupied_cells=occupied, mean_distance=float(first[0].double().sqrt().mean()),
               nearest_wall=stats(wall_ms(lambda: mesh_distance.nearest(q, p), warmup, repeats)),
               search_kernel=stats(device_ms(lambda: ops.nn_search(qs, rec, start, lo, h, grid), warmup, repeats)))
    print(n, out, flush=True)
    return out, (q, p, first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2 ** 16, 2 ** 18, 2 ** 20])
    ap.add_argument("--brute-size", type=int, default=2 ** 16)
    ap.add_argument("--k", type=float, nargs="+", default=[1.5, 2, 4])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--samples", type=int, nargs="+", default=[1_000_000, 16_000_000],
                    help="samples a surface for the simplification error: the distances are between samples, so the first (the command "
                         "lines' default) shows the floor a user meets and the second resolves the error under it")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_distance_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_distance_bench needs the GPU"
    torch.cuda.set_device(0)
    results = dict(device=torch.cuda.get_device_name(0), nearest={}, simplify_error={},
                   not_measured="kernel times from a profiler trace (device events around the call instead); point sets that fill a "
                                "volume (these lie on a sphere: most cells of the grid are empty and the occupied ones hold more "
                                "than four references); queries far from every reference; sizes other than those listed")
    for n in args.sizes:
        case, (q, p, got) = bench_nearest(n, args.warmup, args.repeats)
        results["nearest"][str(n)] = case
        if n == args.brute_size:
            want = brute(q, p)
            base = stats(wall_ms(lambda: brute(q, p), 1, args.repeats))
            results["brute_force"] = dict(points_a_side=n, chunk=4096, wall=base,
                                          same_index_share=float((want[1] == got[1]).double().mean()),
                                          max_abs_d2_difference=float((want[0] - got[0]).abs().max()),
                                          nearest_over_brute=round(case["nearest_wall"]["median_ms"] / base["median_ms"], 5),
                                          speedup=round(base["median_ms"] / case["nearest_wall"]["median_ms"], 2))
            print("brute force", results["brute_force"], flush=True)
        del q, p, got
    verts, faces = mesh.extract(sphere(args.resolution), 0.0, LO, HI)
    for k in args.k:
        grid = mesh.cluster_grid(args.resolution, k)
        v2, f2, counts = mesh.simplify(verts, faces, LO, HI, grid)
        for n in args.samples:
            err = mesh.simplification_error(v2, f2, verts, faces, LO, HI, args.resolution, n)
            wall = stats(wall_ms(lambda: mesh.simplification_error(v2, f2, verts, faces, LO, HI, args.resolution, n), 1, 3))
            key = f"{args.resolution}_k{k:g}_n{n}"
            results["simplify_error"][key] = dict(
                resolution=args.resolution, k=k, samples=n, cluster_grid=list(grid), verts_in=int(verts.shape[0]),
                faces_in=int(faces.shape[0]), verts_out=int(v2.shape[0]), faces_out=int(f2.shape[0]),
                face_reduction=round(faces.shape[0] / max(1, f2.shape[0]), 2), **counts, scores=err, wall=wall)
            print(key, results["simplify_error"][key], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
