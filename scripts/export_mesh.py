"""Export the density level set of a checkpoint as a triangle mesh (binary PLY, per-vertex normals for arch ngp).

    python scripts/export_mesh.py --config <YAML> --ckpt runs/train/last.ckpt --out mesh.ply \
        [--resolution N | --resolution NX NY NZ] [--level L] [--aabb x0 y0 z0 x1 y1 z1] [--no-normals]
        [--min-component N] [--largest K] [--fill-cavities] [--simplify K [--simplify-error [N]]]
        [--tsdf [--tsdf-views N] [--tsdf-trunc T] [--tsdf-min-opacity A] [--tsdf-carve]]

The field is loaded as scripts/render.py loads it.  The density is sampled on a regular lattice of --resolution points per
axis over --aabb (default: the model's box), the surface sigma = --level is extracted on the GPU (robust_e_nerf_amd/mesh.py)
and every vertex gets the direction of -grad sigma as its normal, the convention of `render.py --normals`.  Arch mlp has no
density gradient: its mesh is written without normals.  --min-component / --largest drop floaters (connected pieces of the
solid, counted in lattice points) and --fill-cavities closes the voids inside objects before the extraction (mesh.clean).
--simplify K merges the vertices within each cell of K lattice spacings into one (vertex clustering, mesh.simplify): sample
finely for the geometry, simplify for a file a viewer can hold; --simplify-error scores the simplified mesh against the extracted
one (N samples a surface, default 1 000 000: mesh_distance.compare) in world units and in lattice spacings.  `model.nerf.aabb: auto` spans the camera positions, so it needs
--dataset-dir, --synthetic or an explicit --aabb.
--tsdf meshes what the field renders instead of a density level: --tsdf-views poses evenly spaced in time along the trajectory
(the dataset's, or the synthetic orbit) are rendered at the calibration's intrinsics and size, their z-depth maps are fused into
a truncated signed distance lattice on the GPU and its zero set is extracted (robust_e_nerf_amd/tsdf.py); everything after the
extraction is the same.  Points farther than the truncation behind every surface are never seen, so a closed object carries an
inner shell at about that depth; it is a cavity, and --fill-cavities removes it.
"""
import argparse
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--ckpt", help="checkpoint to load (default: the YAML's model.checkpoint_filepath)")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    ap.add_argument("--resolution", type=int, nargs="+", default=[256],
                    help="lattice points per axis: one value for all three axes or NX NY NZ (default 256)")
    ap.add_argument("--level", type=float, default=10.0,
                    help="density of the extracted surface (default 10.0: a parameter for the user to choose per scene, not a "
                         "value measured on any field)")
    ap.add_argument("--aabb", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="world box of the lattice (default: the model's box)")
    ap.add_argument("--no-normals", action="store_true", help="write the mesh without per-vertex normals")
    ap.add_argument("--min-component", type=int, default=1, metavar="N",
                    help="drop the connected pieces of the solid with fewer than N lattice points: floaters (default 1: keep all)")
    ap.add_argument("--largest", type=int, metavar="K", help="keep only the K largest connected pieces of the solid")
    ap.add_argument("--fill-cavities", action="store_true",
                    help="fill the voids that reach no face of the lattice: no inner surface of a hollow object")
    ap.add_argument("--simplify", type=float, metavar="K",
                    help="simplify the mesh by vertex clustering: one vertex per cell of K lattice spacings, K >= 1 (default: off)")
    ap.add_argument("--simplify-error", type=int, nargs="?", const=1_000_000, metavar="N",
                    help="with --simplify: the distance between the simplified and the extracted mesh from N samples a surface "
                         "(default 1000000) (default: off)")
    ap.add_argument("--dataset-dir", help="camera poses for `aabb: auto` (default: the YAML's data.dataset_directory)")
    ap.add_argument("--synthetic", action="store_true",
                    help="`aabb: auto` from the synthetic benchmark orbit; with --tsdf also the views' poses and intrinsics")
    ap.add_argument("--tsdf", action="store_true",
                    help="mesh what the field RENDERS instead of a density level: z-depth maps of --tsdf-views posed views are fused "
                         "into a truncated signed distance lattice and its zero set is extracted (robust_e_nerf_amd/tsdf.py); "
                         "--level is ignored.  Points farther than the truncation behind every surface are never seen, so a closed "
                         "object carries an inner shell at about that depth: --fill-cavities removes it")
    ap.add_argument("--tsdf-views", type=int, default=64, metavar="N",
                    help="with --tsdf: N poses evenly spaced in time along the trajectory, at the calibration's intrinsics and size "
                         "(default 64)")
    ap.add_argument("--tsdf-trunc", type=float, metavar="T",
                    help="with --tsdf: the truncation distance in world units (default: three times the largest lattice spacing)")
    ap.add_argument("--tsdf-min-opacity", type=float, default=0.5, metavar="A",
                    help="with --tsdf: a pixel whose rendered opacity is below A has no depth (default 0.5)")
    ap.add_argument("--tsdf-carve", action="store_true",
                    help="with --tsdf: a pixel below --tsdf-min-opacity met nothing, so the points along its ray are free space "
                         "(default: it says nothing about them)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one value or three")
    if args.min_component < 1 or (args.largest is not None and args.largest < 1):
        ap.error("--min-component and --largest take integers >= 1")
    if args.simplify is not None and not (math.isfinite(args.simplify) and args.simplify >= 1):
        ap.error("--simplify takes a finite number >= 1")
    if args.simplify_error is not None and (args.simplify is None or args.simplify_error < 1):
        ap.error("--simplify-error takes a number of samples >= 1 and needs --simplify")
    if args.tsdf_views < 1:
        ap.error("--tsdf-views takes an integer >= 1")
    if args.tsdf_trunc is not None and not (math.isfinite(args.tsdf_trunc) and args.tsdf_trunc > 0):
        ap.error("--tsdf-trunc takes a finite number > 0")
    if not 0.0 <= args.tsdf_min_opacity <= 1.0:
        ap.error("--tsdf-min-opacity takes a number in [0, 1]")
    if args.tsdf and args.level != ap.get_default("level"):
        print("warning: --level is ignored with --tsdf (the fused field is extracted at its zero set)", file=sys.stderr, flush=True)
    args.resolution = tuple(args.resolution * 3 if len(args.resolution) == 1 else args.resolution)
    return args


def main(argv=None):
    args = parse_args(argv)
    from robust_e_nerf_amd import checkpoint, config, data, mesh
    from render import load_config
    cfg, ckpt = load_config(args.config, args.ckpt)
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ncfg = cfg["model"]["nerf"]
    tab_pos = None
    if ncfg["aabb"] == "auto":
        if args.synthetic:
            import bench
            tab_pos = torch.from_numpy(bench.synthetic_scene()[1])
        else:
            tab_pos = data.load_camera_poses(args.dataset_dir or cfg["data"]["dataset_directory"])[1]
    rcfg = config.render_cfg(cfg, tab_pos)
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    arch = ncfg.get("arch", "ngp")
    fld, r = config.make_renderer(ncfg, rcfg, checkpoint.radiance_dim(sd, arch), dev)
    bkgd = checkpoint.load_render_state(sd, fld, r, arch)
    normals = not args.no_normals
    if normals and arch != "ngp":
        print(f"arch {arch} has no density gradient: the mesh is written without normals", flush=True)
        normals = False
    lo, hi = (args.aabb[:3], args.aabb[3:]) if args.aabb else (None, None)
    common = dict(normals=normals, min_points=args.min_component, largest=args.largest, fill_cavities=args.fill_cavities,
                  simplify=args.simplify, **({} if args.simplify_error is None else dict(simplify_error=args.simplify_error)))
    t0 = time.perf_counter()
    if args.tsdf:
        from robust_e_nerf_amd import ops, tsdf
        if args.synthetic:
            import bench
            cam = data.load_trajectory_camera(None, bench.synthetic_scene())
        else:
            cam = data.load_trajectory_camera(args.dataset_dir or cfg["data"]["dataset_directory"])
        tab_ts, tab_p, tab_q, Kinv, height, width = cam
        ts = data.even_view_times(tab_ts, args.tsdf_views).to(dev)
        cam_pos, cam_rot = ops.trajectory(ts, tab_ts.to(dev), tab_p.to(dev), tab_q.to(dev))
        K = torch.linalg.inv(Kinv.double()).float()
        stats = tsdf.export(r, args.out, K, Kinv.to(dev, torch.float32), cam_pos, cam_rot, height, width, args.resolution, lo, hi,
                            trunc=args.tsdf_trunc, min_opacity=args.tsdf_min_opacity, carve=args.tsdf_carve, bkgd=bkgd, **common)
        what = f"the zero set of {stats['views']} fused views of {height} x {width} (truncation {stats['trunc']:.6g})"
    else:
        stats = mesh.export(r, args.out, args.resolution, args.level, lo, hi, **common)
        what = f"level {args.level:g}"
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{stats['verts']} vertices, {stats['faces']} faces ({'with' if normals else 'no'} normals) at resolution "
          f"{' x '.join(str(v) for v in stats['resolution'])}, {what}: {args.out} written in {dt:.2f} s", flush=True)
    if args.tsdf:
        n_points = stats["resolution"][0] * stats["resolution"][1] * stats["resolution"][2]
        print(f"{stats['observed']} of {n_points} lattice points were seen by a view", flush=True)
        if not args.fill_cavities:
            print("hint: a closed object carries an inner shell at a depth of about the truncation (what lies deeper is never "
                  "seen); --fill-cavities removes it", flush=True)
    if "components" in stats:
        print(f"{stats['components']} connected pieces, {stats['kept']} kept ({stats['dropped_points']} lattice points dropped); "
              f"{stats['cavities']} cavities filled ({stats['filled_points']} lattice points)", flush=True)
    if "clusters" in stats:
        print(f"simplified from {stats['extracted_verts']} vertices, {stats['extracted_faces']} faces on a cluster grid of "
              f"{' x '.join(str(v) for v in stats['cluster_grid'])}: {stats['clusters']} clusters, {stats['degenerate']} collapsed and "
              f"{stats['duplicate']} repeated faces dropped, {stats['orphans']} unreferenced vertices removed", flush=True)
    err = stats.get("simplify_error")
    if err:
        u = err["in_spacings"]
        print(f"simplification error from {err['samples']} samples a surface, in lattice spacings of {err['spacing']:.6g} (world units): "
              f"simplified -> extracted mean {u['accuracy']['mean']:.4f} ({err['accuracy']['mean']:.6g}), max {u['accuracy']['max']:.4f}; "
              f"extracted -> simplified mean {u['completeness']['mean']:.4f} ({err['completeness']['mean']:.6g}), "
              f"max {u['completeness']['max']:.4f}; Chamfer {u['chamfer']:.4f}, Hausdorff {u['hausdorff']:.4f} ({err['hausdorff']:.6g}); "
              f"the extracted mesh against itself from the same samples: Chamfer {err['sampling_floor']['in_spacings']['chamfer']:.4f}, "
              f"Hausdorff {err['sampling_floor']['in_spacings']['hausdorff']:.4f} (the floor the sampling sets: more samples lower it)",
              flush=True)


if __name__ == "__main__":
    main()
