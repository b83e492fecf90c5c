"""Cost of the level-set mesh extraction (csrc/ren_mesh.hip, robust_e_nerf_amd/mesh.py) on an analytic sphere field, stage by
stage, against the cost of sampling the density lattice it works on.

Per resolution (default 256^3 and 512^3; sigma = 0.3 - |x| over the box [-0.5, 0.5]^3, level 0):
  - classify, the two prefix sums and write, each timed with device events over --repeats warm launches: median, min, max;
  - mesh.extract as a whole (host clock around a call that ends in a device synchronise): it adds the read-back of the totals
    and the allocations;
  - the bytes each kernel needs, counted from the shapes (the sigma read at 4 B per lattice point is the read bound; gathers at
    the bytes they use), over its time, and that rate as a share of --hbm-gbs;
  - mesh.sample_density of a randomly initialised default field (arch ngp, configs/synthetic_smoke.yaml) at the same
    resolution: what producing the lattice costs.
Nothing is fixed in advance; the file records what was measured.  Results are merged into --out by resolution.  GPU only.

    python tools/mesh_bench.py [--resolutions 256 512] [--repeats 7]
"""
import argparse
import json
import os
import sys
import time

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from robust_e_nerf_amd import config, mesh, ops

DEV = "cuda:0"
LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
RADIUS = 0.3


def sphere(res):
    ax = torch.linspace(LO[0], HI[0], res, device=DEV)
    return (RADIUS - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).contiguous()


def stats(ts, unit="ms", digits=4):
    ts = sorted(ts)
    return {f"median_{unit}": round(ts[len(ts) // 2], digits), f"min_{unit}": round(ts[0], digits), f"max_{unit}": round(ts[-1], digits),
            "repeats": len(ts)}


def device_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall_s(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def default_field():
    cfg = yaml.safe_load(open(os.path.join(REPO, "configs", "synthetic_smoke.yaml")))
    ncfg = cfg["model"]["nerf"]
    ncfg["occ_grid"]["resolution"] = 16
    fld, r = config.make_renderer(ncfg, config.render_cfg(cfg, None), 1, DEV)
    config.init_field(fld, "ngp", 1, torch.Generator().manual_seed(0))
    return r


def bench(res, warmup, repeats, hbm_gbs, r):
    n, cubes = res ** 3, (res - 1) ** 3
    sigma = sphere(res)
    level = 0.0
    mask, vcount, fcount = ops.mesh_classify(sigma, level)
    voff, v_total = ops.exclusive_scan(vcount)
    foff, f_total = ops.exclusive_scan(fcount)
    n_verts, n_faces = int(v_total), int(f_total)
    verts, faces = ops.mesh_write(sigma, level, mask, voff, foff, LO, HI, n_verts, n_faces)
    v2, f2 = mesh.extract(sigma, level, LO, HI)
    assert torch.equal(verts, v2) and torch.equal(faces, f2)
    surface = int((mask != 0).sum())
    print(f"{res}^3: {n_verts} vertices, {n_faces} faces, {surface} lattice points with a crossed edge", flush=True)
    ms = {"classify": device_ms(lambda: ops.mesh_classify(sigma, level), warmup, repeats)}
    print(f"  classify {stats(ms['classify'])}", flush=True)
    ms["scan_vertices"] = device_ms(lambda: ops.exclusive_scan(vcount), warmup, repeats)
    ms["scan_faces"] = device_ms(lambda: ops.exclusive_scan(fcount), warmup, repeats)
    print(f"  scans {stats(ms['scan_vertices'])} {stats(ms['scan_faces'])}", flush=True)
    ms["write"] = device_ms(lambda: ops.mesh_write(sigma, level, mask, voff, foff, LO, HI, n_verts, n_faces), warmup, repeats)
    print(f"  write {stats(ms['write'])}", flush=True)
    whole = wall_s(lambda: mesh.extract(sigma, level, LO, HI), 1, repeats)
    # bytes the algorithm needs.  classify: sigma once (its neighbours are other lanes' words), mask + vcount per point, fcount
    # per cube.  write: the mask of every point; per surface point its sigma, the neighbours' sigma of its crossed edges
    # (counted with the vertices: 4 B each), voff, six owners' mask and voff, foff; the outputs.
    need = {"classify": 4 * n + 5 * n + 4 * cubes,
            "scan_vertices": 12 * n, "scan_faces": 12 * cubes,
            "write": n + surface * (4 + 8 + 6 * 9 + 8) + 4 * n_verts + 12 * n_verts + 12 * n_faces}
    out = dict(resolution=res, lattice_points=n, verts=n_verts, faces=n_faces, surface_points=surface,
               sigma_read_bound_bytes=4 * n, output_bytes=12 * n_verts + 12 * n_faces, hbm_gbs_assumed=hbm_gbs, stages={})
    for k, v in ms.items():
        st = stats(v)
        gbs = need[k] / (st["median_ms"] * 1e-3) / 1e9
        out["stages"][k] = dict(st, bytes_needed=need[k], gb_per_s=round(gbs, 1), share_of_hbm=round(gbs / hbm_gbs, 4))
    out["device_total_median_ms"] = round(sum(out["stages"][k]["median_ms"] for k in ms), 4)
    out["sigma_read_bound_ms"] = round(4 * n / (hbm_gbs * 1e9) * 1e3, 4)
    out["extract_wall"] = stats(whole, "s")
    del sigma, mask, vcount, fcount, voff, foff, verts, faces, v2, f2
    aabb = [float(v) for v in r.cfg.aabb]
    sample = wall_s(lambda: mesh.sample_density(r, aabb[:3], aabb[3:], res), 1, max(3, repeats // 2))
    out["sample_density_default_field_wall"] = stats(sample, "s")
    print(f"  device total {out['device_total_median_ms']} ms, extract {out['extract_wall']}, sampling {out['sample_density_default_field_wall']}",
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak memory bandwidth the rates are set against (GB/s)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_bench needs the GPU"
    torch.cuda.set_device(0)
    r = default_field()
    results = {}
    if os.path.exists(args.out):
        results = json.load(open(args.out))
    results["device"] = torch.cuda.get_device_name(0)
    results["not_measured"] = ("kernel times from a profiler trace (device events around each call instead); resolutions other "
                               "than those listed; a trained field's surface (the sphere's is smooth and has about 6 n^2 / 4 "
                               "crossed points); arch mlp sampling")
    for res in args.resolutions:
        results[str(res)] = bench(res, args.warmup, args.repeats, args.hbm_gbs, r)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)
    print(json.dumps({k: v.get("device_total_median_ms") for k, v in results.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
