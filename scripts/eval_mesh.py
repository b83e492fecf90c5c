"""Score a triangle mesh against a ground-truth mesh: accuracy, completeness, Chamfer, Hausdorff, precision / recall / F-score.

    python scripts/eval_mesh.py --mesh A.ply --gt B.ply [--samples N] [--seed S] [--threshold D ...] [--out scores.json]

Both files are PLY (ASCII or binary little-endian; polygons are triangulated: mesh_distance.read_ply), for instance what
scripts/export_mesh.py writes.  --samples points (default 1 000 000) are drawn uniformly by area on each surface and every one
gets its nearest sample of the other surface, exactly, on the GPU (robust_e_nerf_amd/mesh_distance.py).  accuracy is the
distance from the mesh to the ground truth, completeness from the ground truth to the mesh; per --threshold, precision is the
share of the mesh's samples within it, recall the share of the ground truth's.  Distances are in the files' units and between
samples: each exceeds the distance to the surface by at most the other set's sampling radius.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", required=True, help="the PLY file to score")
    ap.add_argument("--gt", required=True, help="the ground-truth PLY file")
    ap.add_argument("--samples", type=int, default=1_000_000, help="points drawn on each surface (default 1000000)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the sampling (default 0): the same seed gives the same scores")
    ap.add_argument("--threshold", type=float, nargs="+", default=[], metavar="D",
                    help="distances at which precision, recall and F-score are reported (default: none)")
    ap.add_argument("--out", help="write the scores to this JSON file as well")
    args = ap.parse_args(argv)
    if args.samples < 1:
        ap.error("--samples takes an integer >= 1")
    if any(not t >= 0 for t in args.threshold):
        ap.error("--threshold takes distances >= 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    from robust_e_nerf_amd import mesh_distance
    torch.cuda.set_device(0)
    dev = "cuda:0"
    meshes, counts = [], {}
    for key, path in (("mesh", args.mesh), ("gt", args.gt)):
        verts, faces = mesh_distance.read_ply(path)
        counts[key] = dict(path=path, verts=int(verts.shape[0]), faces=int(faces.shape[0]))
        meshes += [torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)]
    out = dict(mesh_distance.compare(*meshes, samples=args.samples, seed=args.seed, thresholds=args.threshold), **counts)
    for key in ("mesh", "gt"):
        print(f"{key}: {counts[key]['verts']} vertices, {counts[key]['faces']} faces ({counts[key]['path']})")
    for key, what in (("accuracy", "mesh -> gt"), ("completeness", "gt -> mesh")):
        print(f"{key} ({what}): mean {out[key]['mean']:.6g}, rms {out[key]['rms']:.6g}, max {out[key]['max']:.6g}")
    print(f"Chamfer {out['chamfer']:.6g}, Hausdorff {out['hausdorff']:.6g} ({out['samples']} samples a surface, seed {out['seed']})")
    for t in out["thresholds"]:
        print(f"at {t['threshold']:g}: precision {t['precision']:.4f}, recall {t['recall']:.4f}, F-score {t['fscore']:.4f}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
