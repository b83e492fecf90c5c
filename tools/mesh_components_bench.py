"""Cost of the lattice components (csrc/ren_mesh_components.hip) beside the memory pass of the same lattice.

Per resolution (default 256^3 and 512^3) and field:
  (a) sphere: tools/mesh_bench.py's sigma = 0.3 - |x| over [-0.5, 0.5]^3 at level 0: ONE giant component, every union ends on one
      root -- the worst contention;
  (b) noise: the same sphere, and outside it seeded uniform noise of which --noise-share lies above the level: the sphere plus a
      great many small components;
ops.mesh_components (its three launches together), with outside = 0 and 1, and ops.mesh_component_apply, each timed with device
events over --repeats launches after --warmup warm ones: median, min, max.  Before timing, every result is compared with a
second run by torch.equal.  Beside each number: ops.mesh_classify on the same lattice (the memory-pass yardstick: components
reads 4 B and writes 9 B per point at the least) and, where scipy imports, scipy.ndimage.label on the host with the same
14-neighbourhood (context; one run).  Nothing is fixed in advance; the file records what was measured.  GPU only.

    python tools/mesh_components_bench.py [--resolutions 256 512] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from mesh_bench import DEV, device_ms, sphere, stats
from robust_e_nerf_amd import ops

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def fields(res, share, seed):
    s = sphere(res)
    yield "sphere", s
    noise = torch.rand(s.shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)
    yield "noise", torch.maximum(s, noise - (1.0 - share)).contiguous()


def scipy_label(sigma, level):
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        return None
    structure = np.zeros((3, 3, 3), dtype=bool)
    structure[1, 1, 1] = True
    for d in DIRS:
        structure[1 + d[0], 1 + d[1], 1 + d[2]] = structure[1 - d[0], 1 - d[1], 1 - d[2]] = True
    inside = sigma.cpu().numpy() >= level
    t0 = time.perf_counter()
    _, count = ndimage.label(inside, structure=structure)
    return dict(seconds=round(time.perf_counter() - t0, 3), components=int(count), repeats=1)


def bench(res, name, sigma, warmup, repeats, with_scipy):
    n, level = res ** 3, 0.0
    out = dict(resolution=res, lattice_points=n, field=name, min_bytes=13 * n)
    for outside in (0, 1):
        a, b = ops.mesh_components(sigma, level, bool(outside)), ops.mesh_components(sigma, level, bool(outside))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "two runs of mesh_components differ"
        label, size, border = a
        roots = torch.nonzero(size).reshape(-1)
        assert int(size.sum()) == int((label >= 0).sum()) and int(roots.numel()) == int((label.reshape(-1)[roots] == roots).sum())
        key = "outside" if outside else "inside"
        out[key] = dict(components=int(roots.numel()), points=int(size.sum()), largest=int(size.max()),
                        on_border=int(border.sum()),
                        **stats(device_ms(lambda: ops.mesh_components(sigma, level, bool(outside)), warmup, repeats)))
        print(f"  {res}^3 {name} {key}: {out[key]}", flush=True)
        if not outside:
            drop = torch.zeros(n, device=DEV, dtype=torch.uint8)
            drop[roots[size[roots] < int(size.max())]] = 1
            x, y = (ops.mesh_component_apply(sigma, label, drop, float("-inf")) for _ in range(2))
            assert torch.equal(x, y)
            out["apply"] = stats(device_ms(lambda: ops.mesh_component_apply(sigma, label, drop, float("-inf")), warmup, repeats))
            del x, y, drop
        del a, b, label, size, border
    out["classify"] = stats(device_ms(lambda: ops.mesh_classify(sigma, level), warmup, repeats))
    for key in ("inside", "outside"):
        out[key]["times_classify"] = round(out[key]["median_ms"] / out["classify"]["median_ms"], 2)
        out[key]["gb_per_s_of_min_bytes"] = round(13 * n / (out[key]["median_ms"] * 1e-3) / 1e9, 1)
    print(f"  {res}^3 {name} apply {out['apply']} classify {out['classify']}", flush=True)
    if with_scipy:
        out["scipy_ndimage_label_host"] = scipy_label(sigma, level)
        print(f"  {res}^3 {name} scipy {out['scipy_ndimage_label_host']}", flush=True)
        if out["scipy_ndimage_label_host"] is not None:
            assert out["scipy_ndimage_label_host"]["components"] == out["inside"]["components"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--noise-share", type=float, default=0.1, help="share of the points outside the sphere that the noise puts inside")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_components_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_components_bench needs the GPU"
    torch.cuda.set_device(0)
    results = json.load(open(args.out)) if os.path.exists(args.out) else {}
    results["device"] = torch.cuda.get_device_name(0)
    results["method"] = (f"{args.warmup} warm launches, then {args.repeats} timed with device events around each call (the three "
                         "launches of mesh_components together); every result compared with a second run by torch.equal first")
    results["not_measured"] = ("kernel times from a profiler trace or per launch; hardware counters; resolutions and noise shares "
                               "other than those listed; a trained field")
    for res in args.resolutions:
        for name, sigma in fields(res, args.noise_share, args.seed):
            results[f"{res}_{name}"] = bench(res, name, sigma, args.warmup, args.repeats, not args.no_scipy)
            del sigma
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            json.dump(results, open(args.out, "w"), indent=1)
    print(json.dumps({k: (v["inside"]["median_ms"], v["classify"]["median_ms"]) for k, v in results.items() if isinstance(v, dict)}))


if __name__ == "__main__":
    main()
