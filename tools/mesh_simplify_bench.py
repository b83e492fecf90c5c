"""Cost of the mesh simplification by vertex clustering (csrc/ren_mesh_simplify.hip, mesh.simplify), stage by stage, on the
mesh that mesh.extract makes of the analytic sphere of tools/mesh_bench.py.

Per resolution (default 256^3 and 512^3) and cluster size k (default 2 and 4 lattice spacings; grid = mesh.cluster_grid):
  - the result is compared with a second call (`torch.equal` on vertices and faces, the counts) before anything is timed;
  - every stage -- the six kernels, the three prefix sums, and the ordering of the faces by their key (two stable torch.sort
    calls and two gathers) -- timed with device events over --repeats warm launches: median, min, max;
  - mesh.simplify as a whole (host clock around a call that ends in a device synchronise): it adds the allocations, the
    clearing of the per-cell arrays and the two read-backs of totals;
  - the bytes each stage needs, counted from the shapes (gathers at the bytes they use, an atomic add at its operand), over its
    time, and that rate as a share of --hbm-gbs;
  - mesh.extract's device total at the same resolution, from profiles/mesh_bench.json when it is there: the reference point.
Nothing is fixed in advance; the file records what was measured.  Results are merged into --out by case.  GPU only.

    python tools/mesh_simplify_bench.py [--resolutions 256 512] [--k 2 4] [--repeats 7]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from robust_e_nerf_amd import mesh, ops
from mesh_bench import HI, LO, device_ms, sphere, stats, wall_s


def order_by_key(key_a, key_b):
    by_b = torch.sort(key_b, stable=True).indices
    return by_b[torch.sort(key_a[by_b], stable=True).indices]


def bench(verts, faces, res, k, warmup, repeats, hbm_gbs):
    grid = mesh.cluster_grid(res, k)
    cells = grid[0] * grid[1] * grid[2]
    V, F = verts.shape[0], faces.shape[0]
    first, second = mesh.simplify(verts, faces, LO, HI, grid), mesh.simplify(verts, faces, LO, HI, grid)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and first[2] == second[2]
    out_v, out_f, counts = first
    V2, F2 = out_v.shape[0], out_f.shape[0]
    print(f"{res}^3 k = {k}: grid {grid}, {V} -> {V2} vertices, {F} -> {F2} faces, {counts}", flush=True)
    # the stages, each on the inputs the call gives it
    cell, sums, count = ops.mesh_simplify_cells(verts, LO, HI, grid)
    flag = ops.mesh_simplify_flags(count)
    coff, total = ops.exclusive_scan(flag)
    clusters = int(total)
    ids, key_a, key_b, _ = ops.mesh_simplify_faces(faces, V, cell, coff, clusters)
    order = order_by_key(key_a, key_b)
    keep, used = ops.mesh_simplify_heads(order, key_a, key_b, ids, clusters)
    foff, _ = ops.exclusive_scan(keep)
    uoff, _ = ops.exclusive_scan(used)
    run = {"cells": lambda: ops.mesh_simplify_cells(verts, LO, HI, grid),      # with the clearing of sums and count
           "flags": lambda: ops.mesh_simplify_flags(count),
           "scan_cells": lambda: ops.exclusive_scan(flag),
           "faces": lambda: ops.mesh_simplify_faces(faces, V, cell, coff, clusters),
           "order_by_key": lambda: order_by_key(key_a, key_b),
           "heads": lambda: ops.mesh_simplify_heads(order, key_a, key_b, ids, clusters),
           "scan_faces": lambda: ops.exclusive_scan(keep),
           "scan_clusters": lambda: ops.exclusive_scan(used),
           "vertices": lambda: ops.mesh_simplify_vertices(sums, count, coff, used, uoff, LO, HI, grid, V2),
           "compact_faces": lambda: ops.mesh_simplify_compact_faces(ids, keep, foff, uoff, F2)}
    # bytes the algorithm needs.  cells: the vertex, its cell id, four atomic operands (28 B), and the clearing of 28 B per
    # cell.  faces: the face, three cell ids and three offsets gathered, ids + both keys written.  order_by_key: each sort at
    # one read and one write of key and index (a radix sort makes several passes: a lower bound), the two gathers.  heads: the
    # order, both keys of the face and of the one before, keep; the ids and marks of the kept faces.  vertices: count of every
    # cell; per cluster its offset and mark; per written vertex sums, offset and the row.  compact_faces: keep of every face;
    # per kept face its offset, ids, three gathered offsets and the row.
    need = {"cells": 12 * V + 4 * V + 28 * V + 28 * cells, "flags": 8 * cells, "scan_cells": 12 * cells,
            "faces": 12 * F + 3 * 4 * F + 3 * 8 * F + 12 * F + 12 * F,
            "order_by_key": 2 * (8 + 8) * F + 2 * (4 + 8) * F + (8 + 4 + 4) * F + (8 + 8 + 8) * F,
            "heads": 8 * F + 2 * 12 * F + 4 * F + F2 * (12 + 12) + 4 * clusters,
            "scan_faces": 12 * F, "scan_clusters": 12 * clusters,
            "vertices": 4 * cells + clusters * (8 + 4) + V2 * (24 + 8 + 12),
            "compact_faces": 4 * F + F2 * (8 + 12 + 24 + 12)}
    out = dict(resolution=res, k=k, cluster_grid=list(grid), cells=cells, verts_in=V, faces_in=F, verts_out=V2, faces_out=F2,
               **counts, dense_bytes=40 * cells, hbm_gbs_assumed=hbm_gbs, stages={})
    for name, fn in run.items():
        st = stats(device_ms(fn, warmup, repeats))
        gbs = need[name] / (st["median_ms"] * 1e-3) / 1e9
        out["stages"][name] = dict(st, bytes_needed=need[name], gb_per_s=round(gbs, 1), share_of_hbm=round(gbs / hbm_gbs, 4))
        print(f"  {name} {st}", flush=True)
    out["device_total_median_ms"] = round(sum(s["median_ms"] for s in out["stages"].values()), 4)
    out["simplify_wall"] = stats(wall_s(lambda: mesh.simplify(verts, faces, LO, HI, grid), 1, repeats), "s")
    print(f"  device total {out['device_total_median_ms']} ms, simplify {out['simplify_wall']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--k", type=float, nargs="+", default=[2, 4])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak memory bandwidth the rates are set against (GB/s)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_simplify_bench.json"))
    ap.add_argument("--extract-bench", default=os.path.join(REPO, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_simplify_bench needs the GPU"
    torch.cuda.set_device(0)
    results = json.load(open(args.out)) if os.path.exists(args.out) else {}
    extract = json.load(open(args.extract_bench)) if os.path.exists(args.extract_bench) else {}
    results["device"] = torch.cuda.get_device_name(0)
    results["not_measured"] = ("kernel times from a profiler trace (device events around each call instead); a trained field's mesh "
                               "(the sphere's vertices fill the cells of one thin shell evenly); wave-aggregated atomic adds in "
                               "the cells kernel; a sort of the faces that are not degenerate only; resolutions and k other than "
                               "those listed")
    for res in args.resolutions:
        verts, faces = mesh.extract(sphere(res), 0.0, LO, HI)
        for k in args.k:
            case = bench(verts, faces, res, k, args.warmup, args.repeats, args.hbm_gbs)
            if str(res) in extract:
                case["extract_device_total_median_ms"] = extract[str(res)].get("device_total_median_ms")
                case["extract_wall"] = extract[str(res)].get("extract_wall")
            results[f"{res}_k{k:g}"] = case
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            json.dump(results, open(args.out, "w"), indent=1)
    print(json.dumps({k: v.get("device_total_median_ms") for k, v in results.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
