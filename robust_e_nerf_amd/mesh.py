"""Triangle mesh of a trained field's density level set, written as a binary PLY with per-vertex normals.

    from robust_e_nerf_amd import mesh
    stats = mesh.export(renderer, "mesh.ply", res=256, level=10.0)        # box: the renderer's cfg.aabb

The density is sampled on a regular lattice over a world box (`sample_density`, through `Renderer.query_density`, both
architectures), the level set sigma = level is extracted by marching tetrahedra on the GPU (`extract`: ops.mesh_classify, two
ops.exclusive_scan, ops.mesh_write -- include/ren_amd.h "mesh" fixes every index, so the result repeats bit for bit), and the
vertices get the direction of -grad sigma as their normal (`vertex_normals`, through `Renderer.density_gradient`: arch ngp),
the convention of the normal maps.  Triangles of zero area (sigma == level exactly at lattice points) are kept; the caller may
drop them.  The whole lattice lives in device memory at once.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops

Res = Union[int, Sequence[int]]


def _resolution(res: Res) -> Tuple[int, int, int]:
    r = tuple(res) if isinstance(res, (tuple, list)) else (res,)
    if len(r) == 1:
        r = r * 3
    if len(r) != 3 or any(int(v) != v or v < 2 for v in r):
        raise ValueError(f"mesh: the resolution is one or three integers >= 2; got {res!r}")
    r = tuple(int(v) for v in r)
    if r[0] * r[1] * r[2] > ops.MESH_MAX_POINTS:
        raise ValueError(f"mesh: a lattice of {r} has more than 2^30 points")
    return r


def _box(lo: Sequence[float], hi: Sequence[float]):
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"mesh: the box needs finite lo < hi on every axis; got {lo}, {hi}")
    return lo, hi


def lattice_points(lo: Sequence[float], hi: Sequence[float], res: Res, start: int, stop: int, device="cuda:0") -> torch.Tensor:
    """world positions (stop - start, 3) float32 of the lattice indices start .. stop - 1, index (i * ny + j) * nz + k at
    lo + (i, j, k) * (hi - lo) / (res - 1), formed in float64 and rounded once"""
    nx, ny, nz = _resolution(res)
    lo, hi = _box(lo, hi)
    if not 0 <= start <= stop <= nx * ny * nz:
        raise ValueError(f"lattice_points: [{start}, {stop}) is not a range of the {nx * ny * nz} lattice indices")
    p = torch.arange(start, stop, device=device, dtype=torch.int64)
    ijk = torch.stack([p // (ny * nz), (p // nz) % ny, p % nz], dim=-1).to(torch.float64)
    lo_t = torch.tensor(lo, device=device, dtype=torch.float64)
    h = (torch.tensor(hi, device=device, dtype=torch.float64) - lo_t) / torch.tensor([nx - 1, ny - 1, nz - 1], device=device,
                                                                                   dtype=torch.float64)
    return (lo_t + ijk * h).to(torch.float32).contiguous()


def sample_density(r, lo: Sequence[float], hi: Sequence[float], res: Res, chunk: int = 1 << 21) -> torch.Tensor:
    """sigma (nx, ny, nz) float32 on the renderer's device: r.query_density at every lattice point, `chunk` points a call"""
    nx, ny, nz = _resolution(res)
    lo, hi = _box(lo, hi)
    if chunk < 1:
        raise ValueError("sample_density: chunk < 1")
    dev = r.field.flat.device
    n = nx * ny * nz
    out = torch.empty(n, device=dev, dtype=torch.float32)
    for s0 in range(0, n, chunk):
        s1 = min(n, s0 + chunk)
        out[s0:s1] = r.query_density(lattice_points(lo, hi, (nx, ny, nz), s0, s1, dev)).reshape(-1)
    return out.view(nx, ny, nz)


def extract(sigma: torch.Tensor, level: float, lo: Sequence[float], hi: Sequence[float]):
    """sigma (nx, ny, nz) float32 on the device over the world box [lo, hi] -> verts (V, 3) float32, faces (F, 3) int32:
    the level set sigma = level (inside: sigma >= level), triangles oriented along -grad sigma.  One host synchronisation
    (the two totals).  ValueError for more than 2^30 lattice points or 2^31 vertices and beyond."""
    lo, hi = _box(lo, hi)
    mask, vcount, fcount = ops.mesh_classify(sigma, level)
    voff, v_total = ops.exclusive_scan(vcount)
    foff, f_total = ops.exclusive_scan(fcount)
    n_verts, n_faces = torch.cat([v_total, f_total]).tolist()
    if n_verts >= ops.MESH_MAX_VERTS:
        raise ValueError(f"mesh.extract: {n_verts} vertices; the total must stay below 2^31 (lower the resolution)")
    return ops.mesh_write(sigma, level, mask, voff, foff, lo, hi, n_verts, n_faces)


def vertex_normals(r, verts: torch.Tensor, chunk: int = 1 << 20) -> torch.Tensor:
    """(V, 3) float32: -grad sigma / |grad sigma| at the vertices (r.density_gradient: arch ngp; arch mlp raises
    NotImplementedError); a zero gradient gives a zero normal"""
    out = torch.empty(verts.shape[0], 3, device=verts.device, dtype=torch.float32)
    if verts.shape[0] == 0:
        r.density_gradient(verts)                                     # the architecture's refusal does not depend on the mesh
    for s0 in range(0, verts.shape[0], chunk):
        _, g = r.density_gradient(verts[s0: s0 + chunk].contiguous())
        norm = g.norm(dim=-1, keepdim=True)
        out[s0: s0 + chunk] = torch.where(norm > 0, -g / norm.clamp_min(1e-30), torch.zeros_like(g))
    return out


def write_ply(path: str, verts, faces, normals=None) -> None:
    """binary little-endian PLY: vertex x y z [nx ny nz] float, face `list uchar int vertex_indices`"""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    if normals is not None:
        nrm = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
        if nrm.shape != v.shape:
            raise ValueError(f"write_ply: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        v = np.concatenate([v, nrm], axis=1)
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property float {name}" for name in names]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def export(r, path: str, res: Res, level: float, lo: Optional[Sequence[float]] = None, hi: Optional[Sequence[float]] = None,
           normals: bool = True) -> dict:
    """sample, extract, (normals,) write `path`; the box defaults to the renderer's cfg.aabb.
    -> dict(verts=V, faces=F, resolution=(nx, ny, nz), normals=bool)"""
    aabb = [float(v) for v in r.cfg.aabb]
    lo = aabb[:3] if lo is None else lo
    hi = aabb[3:] if hi is None else hi
    res = _resolution(res)
    if math.isnan(float(level)):
        raise ValueError("mesh.export: level is NaN")
    sigma = sample_density(r, lo, hi, res)
    verts, faces = extract(sigma, level, lo, hi)
    del sigma
    nrm = vertex_normals(r, verts) if normals else None
    write_ply(path, verts, faces, nrm)
    return dict(verts=int(verts.shape[0]), faces=int(faces.shape[0]), resolution=res, normals=bool(normals))
