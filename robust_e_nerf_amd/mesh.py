"""Triangle mesh of a trained field's density level set, written as a binary PLY with per-vertex normals.

    from robust_e_nerf_amd import mesh
    stats = mesh.export(renderer, "mesh.ply", res=256, level=10.0)        # box: the renderer's cfg.aabb

The density is sampled on a regular lattice over a world box (`sample_density`, through `Renderer.query_density`, both
architectures), the level set sigma = level is extracted by marching tetrahedra on the GPU (`extract`: ops.mesh_classify, two
ops.exclusive_scan, ops.mesh_write -- include/ren_amd.h "mesh" fixes every index, so the result repeats bit for bit), and the
vertices get the direction of -grad sigma as their normal (`vertex_normals`, through `Renderer.density_gradient`: arch ngp),
the convention of the normal maps.  Triangles of zero area (sigma == level exactly at lattice points) are kept; the caller may
drop them.  The whole lattice lives in device memory at once.

`clean` (export's min_points / largest / fill_cavities) rewrites the lattice before the extraction: floaters -- small connected
components of the inside points -- are dropped and cavities -- outside components that reach no face of the lattice -- are
filled, with the components labelled on the GPU (`components`: ops.mesh_components, include/ren_amd.h "mesh components").

`simplify` (export's simplify=k) reduces the extracted mesh by vertex clustering: one vertex per occupied cell of a grid of k
lattice spacings (`cluster_grid`), collapsed and repeated faces dropped (ops.mesh_simplify_*, include/ren_amd.h "mesh
simplify").  The lattice resolution then sets the fidelity of the sampling and k the size of the file; what k costs in geometry
is measured on request (`simplification_error`, export's simplify_error=n: the scores of mesh_distance.compare between the
simplified and the extracted mesh).
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


def components(sigma: torch.Tensor, level: float, outside: bool = False):
    """connected components of the inside points (sigma >= level; with `outside` of their complement, NaN included) under the
    marching-tetrahedra edges (include/ren_amd.h "mesh components") -> label (nx, ny, nz) int32: the smallest linear index of
    the point's component, -1 where not selected; roots (C,) int64 ascending: those smallest indices; sizes (C,) int32: the
    points of each; border (C,) uint8: 1 where the component touches a face of the lattice.  One host synchronisation (C)."""
    label, size, border = ops.mesh_components(sigma, level, outside)
    roots = torch.nonzero(size).reshape(-1)
    return label, roots, size[roots], border[roots]


def _rule(min_points, largest):
    if int(min_points) != min_points or min_points < 1 or (largest is not None and (int(largest) != largest or largest < 1)):
        raise ValueError(f"mesh: min_points and largest are integers >= 1 (largest may be None); got {min_points}, {largest}")


def kept_components(sizes: torch.Tensor, min_points: int = 1, largest: Optional[int] = None) -> torch.Tensor:
    """`clean`'s rule on the sizes of the components in ascending order of their roots -> bool per component: kept iff
    size >= min_points and (largest is None or rank < largest), the rank by (size descending, root ascending)"""
    _rule(min_points, largest)
    keep = sizes >= min_points
    if largest is not None:
        order = torch.argsort(sizes, descending=True, stable=True)               # stable: a tie goes to the smaller root
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=order.device)
        keep = keep & (rank < largest)
    return keep


def _mark(n: int, roots: torch.Tensor) -> torch.Tensor:
    drop = torch.zeros(n, device=roots.device, dtype=torch.uint8)
    drop[roots] = 1
    return drop


def clean(sigma: torch.Tensor, level: float, min_points: int = 1, largest: Optional[int] = None, fill_cavities: bool = False):
    """sigma (nx, ny, nz) float32 -> (sigma', stats): the lattice without its floaters and, with `fill_cavities`, without its
    cavities, for the unchanged `extract`.
    1. Drop.  The inside components are ranked by (size descending, root ascending); one is kept iff size >= min_points and
       (largest is None or rank < largest); the points of the others become -inf.
    2. Fill, if fill_cavities.  The outside components OF THE RESULT OF STEP 1 that touch no face of the lattice are cavities
       (a dropped floater inside one is part of it by now); their points become +inf.
    stats: components (inside, before), kept, dropped_points, cavities, filled_points.  Nothing to drop or fill returns the
    input tensor itself.  ValueError for min_points < 1, largest < 1 or a level that is not finite.
    Why +-inf is safe and `extract` needs no change: a component is maximal, so every neighbour of a dropped point is outside
    or dropped with it, and every neighbour of a filled point is inside.  No marching-tetrahedra edge at a rewritten point is
    crossed, no interpolation ever reads the +-inf, and every surviving vertex lies on an edge whose two sigma values are
    untouched: the vertices of extract(clean(sigma)) are, bit for bit, a subset of those of extract(sigma)."""
    _rule(min_points, largest)
    if not math.isfinite(float(level)):
        raise ValueError(f"mesh.clean: the level must be finite (a rewritten point is +-inf); got {level}")
    n = sigma.numel()
    label, roots, sizes, _ = components(sigma, level)
    keep = kept_components(sizes, min_points, largest)
    stats = dict(components=int(roots.numel()), kept=int(keep.sum()), dropped_points=int(sizes[~keep].sum()), cavities=0,
                 filled_points=0)
    if stats["kept"] < stats["components"]:
        sigma = ops.mesh_component_apply(sigma, label, _mark(n, roots[~keep]), -math.inf)
    if fill_cavities:
        label, roots, sizes, border = components(sigma, level, outside=True)
        closed = border == 0
        stats.update(cavities=int(closed.sum()), filled_points=int(sizes[closed].sum()))
        if stats["cavities"]:
            sigma = ops.mesh_component_apply(sigma, label, _mark(n, roots[closed]), math.inf)
    return sigma, stats


def cluster_grid(res: Res, k: float) -> Tuple[int, int, int]:
    """the cluster grid of `simplify` for a lattice of `res` points per axis and clusters of k lattice spacings (k >= 1, not
    necessarily whole): g_a = max(1, ceil((n_a - 1) / k)).  k = 1 gives one cell per cube of the lattice."""
    try:
        k = float(k)
    except (TypeError, ValueError):
        raise ValueError(f"mesh.cluster_grid: k is a number >= 1; got {k!r}") from None
    if not math.isfinite(k) or k < 1:
        raise ValueError(f"mesh.cluster_grid: k is a finite number >= 1; got {k!r}")
    return tuple(max(1, math.ceil((n - 1) / k)) for n in _resolution(res))


def simplify(verts: torch.Tensor, faces: torch.Tensor, lo: Sequence[float], hi: Sequence[float], grid: Sequence[int]):
    """verts (V, 3) float32, faces (F, 3) int32 (any triangle list) -> (verts', faces', stats): vertex clustering over the
    `grid` = (gx, gy, gz) cells of the world box [lo, hi] (include/ren_amd.h "mesh simplify").  Every occupied cell becomes
    one vertex at the mean of its members (integer sums: bit-identical from run to run); faces with two corners in one cell
    or a corner index outside [0, V) are dropped as degenerate, faces that repeat an earlier one's cells in the same
    orientation as duplicates, vertices no kept face references as orphans.  Kept faces stay in input order.
    stats: clusters (occupied cells), degenerate, duplicate, orphans.  Two host synchronisations (the number of clusters; the
    other totals); two stable torch.sort calls order the faces by their key, everything else is the library's kernels.
    ValueError before any launch for a wrong dtype, layout or device, a box that is not finite with lo < hi, a grid extent
    below 1 or more than 2^30 cells."""
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or not faces.is_cuda or not faces.is_contiguous():
        raise ValueError(f"mesh.simplify: faces must be a contiguous (F, 3) int32 device tensor; got {tuple(faces.shape)} "
                         f"{faces.dtype} on {faces.device}")
    if faces.shape[0] >= ops.MESH_MAX_VERTS:
        raise ValueError(f"mesh.simplify: {faces.shape[0]} faces; the count must stay below 2^31")
    cell, sums, count = ops.mesh_simplify_cells(verts, lo, hi, grid)              # checks verts, the box and the grid
    n_verts, n_faces, dev = int(verts.shape[0]), int(faces.shape[0]), verts.device
    empty = (torch.empty(0, 3, device=dev, dtype=torch.float32), torch.empty(0, 3, device=dev, dtype=torch.int32))
    stats = dict(clusters=0, degenerate=n_faces, duplicate=0, orphans=0)
    if n_verts == 0:                                                  # no cell is occupied: every face is out of range
        return (*empty, stats)
    coff, total = ops.exclusive_scan(ops.mesh_simplify_flags(count))
    clusters = int(total)
    stats.update(clusters=clusters, orphans=clusters)
    if n_faces == 0:
        return (*empty, stats)
    ids, key_a, key_b, degenerate = ops.mesh_simplify_faces(faces, n_verts, cell, coff, clusters)
    # lexicographic by (key_a, key_b): stable by the minor word, then stable by the major one
    by_b = torch.sort(key_b, stable=True).indices
    order = by_b[torch.sort(key_a[by_b], stable=True).indices]
    keep, used = ops.mesh_simplify_heads(order, key_a, key_b, ids, clusters)
    del order, by_b, key_a, key_b
    foff, f_total = ops.exclusive_scan(keep)
    uoff, u_total = ops.exclusive_scan(used)
    n_degenerate, f_out, v_out = torch.cat([degenerate.to(torch.int64), f_total, u_total]).tolist()
    stats.update(degenerate=n_degenerate, duplicate=n_faces - n_degenerate - f_out, orphans=clusters - v_out)
    if f_out == 0:
        return (*empty, stats)
    new_verts = ops.mesh_simplify_vertices(sums, count, coff, used, uoff, lo, hi, grid, v_out)
    return new_verts, ops.mesh_simplify_compact_faces(ids, keep, foff, uoff, f_out), stats


_simplify = simplify                     # `export` has a parameter of the function's name


def simplification_error(verts: torch.Tensor, faces: torch.Tensor, verts_0: torch.Tensor, faces_0: torch.Tensor,
                         lo: Sequence[float], hi: Sequence[float], res: Res, samples: int, seed: int = 0) -> Optional[dict]:
    """the simplified mesh (verts, faces) against the extracted one (verts_0, faces_0) it was made of, a lattice of `res` points
    over [lo, hi]: mesh_distance.compare with the simplified mesh as A -- accuracy: simplified -> extracted, completeness:
    extracted -> simplified -- thresholds of half a lattice spacing and one, in world units; plus spacing (the largest of the
    three axes') and, under in_spacings, the distances divided by it.  The distances are between samples, so they do not fall
    below the spacing of the samples themselves: sampling_floor holds chamfer and hausdorff of the extracted mesh against ITSELF
    from the same two sets of `samples` points (world units, and in_spacings) -- what a simplification without any error would
    score.  None when either mesh has no face."""
    from . import mesh_distance
    if faces.shape[0] == 0 or faces_0.shape[0] == 0:
        return None
    lo, hi = _box(lo, hi)
    spacing = max((b - a) / (n - 1) for a, b, n in zip(lo, hi, _resolution(res)))
    out = mesh_distance.compare(verts, faces, verts_0, faces_0, samples, seed, (0.5 * spacing, spacing))
    floor = mesh_distance.compare(verts_0, faces_0, verts_0, faces_0, samples, seed)
    per = lambda d: {k: v / spacing for k, v in d.items()}
    out.update(spacing=spacing, in_spacings=dict(accuracy=per(out["accuracy"]), completeness=per(out["completeness"]),
                                                 chamfer=out["chamfer"] / spacing, hausdorff=out["hausdorff"] / spacing),
               sampling_floor=dict(chamfer=floor["chamfer"], hausdorff=floor["hausdorff"],
                                   in_spacings=dict(chamfer=floor["chamfer"] / spacing, hausdorff=floor["hausdorff"] / spacing)))
    return out


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
           normals: bool = True, min_points: int = 1, largest: Optional[int] = None, fill_cavities: bool = False,
           simplify: Optional[float] = None, simplify_error: Optional[int] = None) -> dict:
    """sample, (clean,) extract, (simplify,) (normals,) write `path`; the box defaults to the renderer's cfg.aabb.
    -> dict(verts=V, faces=F, resolution=(nx, ny, nz), normals=bool); with min_points > 1, largest or fill_cavities the lattice
    goes through `clean` first and the dict carries its stats as well.  With `simplify` = k >= 1 the extracted mesh goes
    through `simplify` on the grid `cluster_grid(res, k)` -- clusters of k lattice spacings -- before the normals are taken
    at the new positions; the dict then carries its stats (clusters, degenerate, duplicate, orphans), cluster_grid, and the
    counts before the simplification as extracted_verts / extracted_faces.  With `simplify_error` = n as well the simplified
    mesh is scored against the extracted one, n samples a surface (`simplification_error`), under the key simplify_error."""
    grid = export_options(res, min_points, largest, simplify, simplify_error)
    aabb = [float(v) for v in r.cfg.aabb]
    lo = aabb[:3] if lo is None else lo
    hi = aabb[3:] if hi is None else hi
    res = _resolution(res)
    if math.isnan(float(level)):
        raise ValueError("mesh.export: level is NaN")
    return export_lattice(r, path, sample_density(r, lo, hi, res), level, lo, hi, normals, min_points, largest, fill_cavities,
                          grid, simplify_error)


def export_options(res: Res, min_points: int, largest: Optional[int], simplify: Optional[float], simplify_error: Optional[int]):
    """`export`'s checks that need no lattice, before anything is sampled or rendered -> the cluster grid of `simplify`, or None"""
    _rule(min_points, largest)
    grid = None if simplify is None else cluster_grid(res, simplify)
    if simplify_error is not None and (grid is None or int(simplify_error) != simplify_error or simplify_error < 1):
        raise ValueError(f"mesh.export: simplify_error is a number of samples >= 1 and needs simplify; got {simplify_error!r}")
    return grid


def export_lattice(r, path: str, sigma: torch.Tensor, level: float, lo: Sequence[float], hi: Sequence[float], normals: bool = True,
                   min_points: int = 1, largest: Optional[int] = None, fill_cavities: bool = False,
                   grid: Optional[Tuple[int, int, int]] = None, simplify_error: Optional[int] = None) -> dict:
    """the tail of `export` for any lattice sigma (nx, ny, nz) float32 over [lo, hi] -- the sampled density, or the fused field
    of tsdf.export at level 0: (clean,) extract at `level`, (simplify on the cluster grid `grid`,) (normals from r,) write
    `path` -> `export`'s dict"""
    res = tuple(int(n) for n in sigma.shape)
    cleaned = {}
    if min_points > 1 or largest is not None or fill_cavities:
        sigma, cleaned = clean(sigma, level, min_points, largest, fill_cavities)
    verts, faces = extract(sigma, level, lo, hi)
    del sigma
    simplified = {}
    if grid is not None:
        extracted = dict(extracted_verts=int(verts.shape[0]), extracted_faces=int(faces.shape[0]))
        before = verts, faces
        verts, faces, simplified = _simplify(verts, faces, lo, hi, grid)
        simplified = dict(simplified, cluster_grid=grid, **extracted)
        if simplify_error is not None:
            simplified["simplify_error"] = simplification_error(verts, faces, *before, lo, hi, res, int(simplify_error))
        del before
    nrm = vertex_normals(r, verts) if normals else None
    write_ply(path, verts, faces, nrm)
    return dict(verts=int(verts.shape[0]), faces=int(faces.shape[0]), resolution=res, normals=bool(normals), **cleaned, **simplified)
