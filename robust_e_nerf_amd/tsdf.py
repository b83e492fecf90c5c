"""Triangle mesh of the surface a trained field RENDERS: posed z-depth maps fused into a truncated signed distance lattice.

    from robust_e_nerf_amd import tsdf
    stats = tsdf.export(renderer, "mesh.ply", K, Kinv, cam_pos, cam_rot, height, width, res=256, fill_cavities=True)

mesh.export extracts the level set sigma = L of the stored density: L is a free parameter, and the half-transparent haze that
the renders integrate away becomes skin at a low L and holes at a high one.  Here the depth maps of posed views
(evaluation.render_image: expected z-depth and opacity) are fused into a lattice (`fuse`, ops.tsdf_integrate -- include/ren_amd.h
"tsdf" fixes every operation, so the field repeats bit for bit and does not depend on how the views are split into calls) and
the zero set of that lattice is extracted by the unchanged tail of mesh.export.  No threshold, and the surface is the one the
training loss saw.

The field: per lattice point the mean over the views that saw it of clamp((D - z) / trunc, ., 1), D the depth at the nearest
pixel and z the point's own depth in that view, NEGATED: inside is positive (mesh.extract's convention, inside = field >= 0,
triangles facing along -grad), free space and never-seen points are -1.  A view does not see a point that lies more than trunc
behind the surface it saw.

Known property -- the inner shell.  Points farther than trunc behind every surface are never seen, so they count as outside:
a closed object gets a second, inward-facing surface at a depth of about trunc.  That shell bounds a cavity in mesh.clean's
sense (an outside component that reaches no face of the lattice), and fill_cavities=True removes it.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import evaluation, mesh, ops


def pack_cameras(cam_pos: torch.Tensor, cam_rot: torch.Tensor) -> torch.Tensor:
    """cam_pos (V, 3), cam_rot (V, 3, 3) camera-to-world (ops.trajectory's pos / rot) -> (V, 12) float32: centre, then R row-major"""
    if cam_pos.dim() != 2 or cam_pos.shape[1] != 3 or cam_rot.shape != (cam_pos.shape[0], 3, 3):
        raise ValueError(f"tsdf.pack_cameras: cam_pos (V, 3) and cam_rot (V, 3, 3) expected; got {tuple(cam_pos.shape)}, "
                         f"{tuple(cam_rot.shape)}")
    return torch.cat([cam_pos.to(torch.float32), cam_rot.to(torch.float32).reshape(-1, 9)], dim=1).contiguous()


def mask_depth(depth: torch.Tensor, opacity: torch.Tensor, min_opacity: float, carve: bool) -> torch.Tensor:
    """rendered z-depth and opacity -> the depth `fuse` takes: where opacity < min_opacity the ray met nothing (+inf: the
    points along it are free space) if `carve`, else it says nothing (NaN); a depth that is not finite and positive elsewhere
    says nothing (NaN)"""
    nan = torch.full_like(depth, math.nan)
    out = torch.where(torch.isfinite(depth) & (depth > 0), depth, nan)
    return torch.where(opacity < min_opacity, torch.full_like(depth, math.inf) if carve else nan, out)


def default_trunc(lo: Sequence[float], hi: Sequence[float], res) -> float:
    """three times the largest lattice spacing"""
    return 3.0 * max((float(b) - float(a)) / (n - 1) for a, b, n in zip(lo, hi, mesh._resolution(res)))


def fuse(depth: torch.Tensor, K, cam_pos: torch.Tensor, cam_rot: torch.Tensor, lo: Sequence[float], hi: Sequence[float], res,
         trunc: float, z_min: float = 1e-6, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """depth (V, H, W) float32 on the device (+inf: nothing met; NaN or <= 0: no information), K the 3 x 3 pinhole matrix,
    cam_pos (V, 3), cam_rot (V, 3, 3) -> (field, count, state) over the lattice of `res` points in [lo, hi]:
    field (nx, ny, nz) float32 = -(sum / count) where count > 0, else -1: positive inside, the surface at level 0 of
    mesh.extract; count (nx, ny, nz) int32: the views that saw each point; state = (sum, count), to be handed back in with
    further views.  The result does not depend on how the views are split into calls as long as their order is kept."""
    res = mesh._resolution(res)
    if state is None:
        state = (torch.zeros(res, device=depth.device, dtype=torch.float32), torch.zeros(res, device=depth.device, dtype=torch.int32))
    total, count = state
    ops.tsdf_integrate(depth, pack_cameras(cam_pos, cam_rot).to(depth.device), K, lo, hi, res, trunc, z_min, total, count)
    field = torch.where(count > 0, -(total / count.to(torch.float32)), torch.full_like(total, -1.0))
    return field, count, state


@torch.no_grad()
def fuse_renders(r, K, Kinv: torch.Tensor, cam_pos: torch.Tensor, cam_rot: torch.Tensor, height: int, width: int,
                 lo: Sequence[float], hi: Sequence[float], res, trunc: float, min_opacity: float = 0.5, carve: bool = False,
                 views_per_call: int = 16, bkgd: Optional[torch.Tensor] = None):
    """render the V poses with evaluation.render_image, `views_per_call` depth maps at a time, mask them (`mask_depth`) and
    integrate them before the next batch is rendered: the V depth maps never exist at once -> fuse's (field, count, state)"""
    if views_per_call < 1 or cam_pos.shape[0] < 1:
        raise ValueError("tsdf.fuse_renders: at least one view, and views_per_call >= 1")
    out = None
    for v0 in range(0, cam_pos.shape[0], views_per_call):
        v1 = min(v0 + views_per_call, cam_pos.shape[0])
        maps = []
        for v in range(v0, v1):
            _, opacity, depth = evaluation.render_image(r, Kinv, cam_pos[v], cam_rot[v], height, width, bkgd=bkgd)
            maps.append(mask_depth(depth, opacity, min_opacity, carve))
        out = fuse(torch.stack(maps).contiguous(), K, cam_pos[v0:v1], cam_rot[v0:v1], lo, hi, res, trunc,
                   state=None if out is None else out[2])
    return out


def export(r, path: str, K, Kinv: torch.Tensor, cam_pos: torch.Tensor, cam_rot: torch.Tensor, height: int, width: int, res,
           lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None, trunc: Optional[float] = None,
           min_opacity: float = 0.5, carve: bool = False, views_per_call: int = 16, bkgd: Optional[torch.Tensor] = None,
           normals: bool = True, min_points: int = 1, largest: Optional[int] = None, fill_cavities: bool = False,
           simplify: Optional[float] = None, simplify_error: Optional[int] = None) -> dict:
    """`fuse_renders` over the given views, then the tail of mesh.export on the fused field at level 0: (clean,) extract,
    (simplify,) (normals,) write `path`; the box defaults to the renderer's cfg.aabb, trunc=None to three times the largest
    lattice spacing.  -> mesh.export's dict plus views, trunc, observed (the lattice points some view saw) and tsdf=True.
    A closed object carries an inner shell at a depth of about trunc (the points behind it are never seen, so they are
    outside); it bounds a cavity in mesh.clean's sense, and fill_cavities=True removes it."""
    grid = mesh.export_options(res, min_points, largest, simplify, simplify_error)
    aabb = [float(v) for v in r.cfg.aabb]
    lo = aabb[:3] if lo is None else lo
    hi = aabb[3:] if hi is None else hi
    res = mesh._resolution(res)
    trunc = default_trunc(lo, hi, res) if trunc is None else float(trunc)
    field, count, _ = fuse_renders(r, K, Kinv, cam_pos, cam_rot, height, width, lo, hi, res, trunc, min_opacity, carve,
                                   views_per_call, bkgd)
    observed = int((count > 0).sum())
    del count
    stats = mesh.export_lattice(r, path, field, 0.0, lo, hi, normals, min_points, largest, fill_cavities, grid, simplify_error)
    return dict(stats, views=int(cam_pos.shape[0]), trunc=trunc, observed=observed, tsdf=True)
