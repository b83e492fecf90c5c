"""Distance between two triangle meshes: accuracy, completeness, Chamfer, Hausdorff on samples, precision / recall / F-score.

    from robust_e_nerf_amd import mesh_distance as md
    verts_a, faces_a = md.read_ply("reconstruction.ply")
    verts_b, faces_b = md.read_ply("ground_truth.ply")
    s = md.compare(torch.from_numpy(verts_a).cuda(), torch.from_numpy(faces_a).cuda(),
                   torch.from_numpy(verts_b).cuda(), torch.from_numpy(faces_b).cuda(), samples=1_000_000, seed=0, thresholds=(0.01,))

Both surfaces are sampled uniformly by area (`sample_surface`), every sample of one gets its nearest sample of the other
(`nearest`), and `scores` turns the two arrays of distances into the numbers.  `nearest` is exact -- the minimum of the float32
squared distance and, among equal minima, the smallest index, whatever grid it searched on (include/ren_amd.h "mesh
distance"): references grouped by the cells of a uniform grid (`nn_grid`, ops.nn_cells, one stable sort), one
query per lane walking shells of cells until nothing outside them can be as near (ops.nn_search).  The distances are between
SAMPLES: each is larger than the distance to the surface by at most the sampling radius of the other set.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch

from . import ops

H_MIN, H_MAX = 2.0 ** -120, 2.0 ** 124            # the cell edge and its reciprocal stay normal float32 numbers


def nn_grid(lo: Sequence[float], hi: Sequence[float], n_refs: int, per_cell: float = 4.0) -> Tuple[float, Tuple[int, int, int]]:
    """the search grid for n_refs references in the box [lo, hi] -> (h, (gx, gy, gz)): cubic cells of edge h with about
    `per_cell` references per cell were they spread evenly over the box -- over its volume, or its area or length when one or
    two axes have no extent -- and g_a = floor((hi_a - lo_a) / h) + 1, so that hi lies inside.  An axis without extent gets
    one cell; h is raised to (largest extent) / 512 where the extents would pass ops.NN_MAX_EXTENT, and each g_a is capped
    there (a point beyond belongs to the border cell anyway).  Pure Python; more references never give fewer cells."""
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a <= b for a, b in zip(lo, hi)):
        raise ValueError(f"nn_grid: the box needs finite lo <= hi on every axis; got {lo}, {hi}")
    if int(n_refs) != n_refs or n_refs < 1 or not (math.isfinite(per_cell) and per_cell > 0):
        raise ValueError(f"nn_grid: n_refs is an integer >= 1 and per_cell a positive number; got {n_refs!r}, {per_cell!r}")
    ext = [b - a for a, b in zip(lo, hi)]
    pos = [e for e in ext if e > 0]
    if not pos:
        return 1.0, (1, 1, 1)
    log_h = (sum(math.log(e) for e in pos) + math.log(per_cell / n_refs)) / len(pos)       # (volume * per_cell / n)^(1 / dims)
    h = math.exp(min(max(log_h, math.log(H_MIN)), math.log(H_MAX)))
    h = min(max(h, max(pos) / ops.NN_MAX_EXTENT, H_MIN), H_MAX)
    return h, tuple(min(ops.NN_MAX_EXTENT, int(e // h) + 1) if e > 0 else 1 for e in ext)


def _points(t, what: str) -> int:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise ValueError(f"{what} must be an (n, 3) float32 tensor; got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} "
                         f"{getattr(t, 'dtype', '')}")
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous device tensor; got one on {t.device}, contiguous: {t.is_contiguous()}")
    if t.shape[0] >= ops.MESH_MAX_VERTS:
        raise ValueError(f"{what}: {t.shape[0]} points; the count must stay below 2^31")
    return int(t.shape[0])


def nearest_on_grid(queries: torch.Tensor, refs: torch.Tensor, lo: Sequence[float], h: float, grid: Sequence[int]):
    """`nearest` on a grid of the caller's choice (cells of edge h from the corner lo, `grid` extents): the same result for
    every choice.  No host synchronisation.  The references are grouped by cell with one stable sort and packed as 16-byte
    records; the queries are sorted by cell as well, so that the lanes of a wave walk the same cells, and the outputs are put
    back in the caller's order."""
    nq, nr = _points(queries, "nearest: queries"), _points(refs, "nearest: refs")
    dev = refs.device
    cells = ops.nn_cells(refs, lo, h, grid)                                       # checks lo, h and the grid
    n_cells = int(grid[0]) * int(grid[1]) * int(grid[2])
    cells, order = torch.sort(cells, stable=True)
    cell_start = torch.searchsorted(cells, torch.arange(n_cells + 1, device=dev, dtype=torch.int32), out_int32=True)
    records = torch.empty(nr, 4, device=dev, dtype=torch.int32)
    records[:, :3] = refs[order].view(torch.int32)
    records[:, 3] = order.to(torch.int32)
    d2 = torch.empty(nq, device=dev, dtype=torch.float32)
    idx = torch.empty(nq, device=dev, dtype=torch.int32)
    if nq == 0:
        return d2, idx
    q_order = torch.sort(ops.nn_cells(queries, lo, h, grid), stable=True).indices
    d2_sorted, idx_sorted = ops.nn_search(queries[q_order].contiguous(), records.view(torch.float32), cell_start, lo, h, grid)
    d2[q_order] = d2_sorted
    idx[q_order] = idx_sorted
    return d2, idx


def nearest(queries: torch.Tensor, refs: torch.Tensor):
    """queries (nq, 3), refs (nr, 3): contiguous float32 device tensors -> d2 (nq,) float32, idx (nq,) int32: per query the
    smallest squared distance to a reference -- dx = q.x - p.x, ..., d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded to
    float32 -- and the smallest index of a reference at that distance.  Exact: equal, bit for bit, to the brute force over all
    pairs.  The grid is `nn_grid` of the references' bounding box.  One host synchronisation (the box and the finiteness of
    the coordinates).  ValueError for no references, a coordinate that is not finite, a wrong dtype, shape or device."""
    _points(queries, "nearest: queries")
    if _points(refs, "nearest: refs") == 0:
        raise ValueError("nearest: there are no reference points")
    lo, hi = torch.aminmax(refs, dim=0)
    finite = torch.isfinite(refs).all() & torch.isfinite(queries).all()
    *box, ok = torch.cat([lo.double(), hi.double(), finite.double().reshape(1)]).tolist()
    if not ok:
        raise ValueError("nearest: a coordinate of the queries or the references is not finite")
    h, grid = nn_grid(box[:3], box[3:], refs.shape[0])
    return nearest_on_grid(queries, refs, box[:3], h, grid)


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, n: int, seed: int) -> torch.Tensor:
    """n points (n, 3) float32, uniform by area over the triangles faces (F, 3) of verts (V, 3), on the tensors' device: the
    triangle by inversion of the cumulative areas (float64; a triangle of zero area is never chosen), the point by uniform
    barycentric coordinates (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2).  A generator seeded with `seed` on that device: the
    same seed gives the same points there.  ValueError for a total area of zero (no faces included), a corner index outside
    [0, V), n < 0."""
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sample_surface: verts (V, 3) and integer faces (F, 3) expected; got {tuple(verts.shape)}, "
                         f"{tuple(faces.shape)} {faces.dtype}")
    if faces.device != verts.device or int(n) != n or n < 0:
        raise ValueError("sample_surface: verts and faces live on one device and n is an integer >= 0")
    if faces.shape[0] == 0 or verts.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces: its area is zero")
    f = faces.to(torch.int64)
    lowest, highest = torch.aminmax(f)
    if int(lowest) < 0 or int(highest) >= verts.shape[0]:
        raise ValueError(f"sample_surface: a corner index is outside [0, {verts.shape[0]})")
    v = verts.to(torch.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cum = torch.cumsum(0.5 * torch.linalg.cross(b - a, c - a).norm(dim=-1), dim=0)
    total = float(cum[-1])
    if not (total > 0 and math.isfinite(total)):
        raise ValueError(f"sample_surface: the total area is {total}")
    gen = torch.Generator(device=verts.device).manual_seed(int(seed))
    r = torch.rand(int(n), 3, generator=gen, device=verts.device, dtype=torch.float64)
    # the first triangle whose cumulative share exceeds r0 in [0, 1): one of zero area shares its value with the one before
    t = torch.searchsorted(cum / cum[-1], r[:, 0].contiguous(), right=True).clamp_(max=f.shape[0] - 1)
    s = torch.sqrt(r[:, 1:2])
    return ((1 - s) * a[t] + s * (1 - r[:, 2:3]) * b[t] + s * r[:, 2:3] * c[t]).to(torch.float32).contiguous()


def _direction(d: torch.Tensor) -> dict:
    return dict(mean=float(d.mean()), rms=float(d.square().mean().sqrt()), max=float(d.max()))


def scores(d_ab, d_ba, thresholds: Sequence[float] = ()) -> dict:
    """d_ab: the distance of every sample of mesh A to B, d_ba: of every sample of B to A (B the ground truth; both non-empty,
    taken as float64) -> dict(accuracy = A -> B and completeness = B -> A, each dict(mean, rms, max); chamfer = the mean of
    the two means; hausdorff = the larger of the two maxima; thresholds = [dict(threshold, precision = the share of d_ab <= t,
    recall = the share of d_ba <= t, fscore = 2 P R / (P + R), 0 when P + R = 0) per t])."""
    d_ab, d_ba = (torch.as_tensor(d).to(torch.float64).reshape(-1) for d in (d_ab, d_ba))
    if d_ab.numel() == 0 or d_ba.numel() == 0:
        raise ValueError("scores: both directions need at least one distance")
    acc, comp = _direction(d_ab), _direction(d_ba)
    out = dict(accuracy=acc, completeness=comp, chamfer=0.5 * (acc["mean"] + comp["mean"]), hausdorff=max(acc["max"], comp["max"]),
               thresholds=[])
    for t in thresholds:
        p, r = float((d_ab <= float(t)).double().mean()), float((d_ba <= float(t)).double().mean())
        out["thresholds"].append(dict(threshold=float(t), precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0))
    return out


def compare(verts_a: torch.Tensor, faces_a: torch.Tensor, verts_b: torch.Tensor, faces_b: torch.Tensor, samples: int = 1_000_000,
            seed: int = 0, thresholds: Sequence[float] = ()) -> dict:
    """mesh A (the reconstruction) against mesh B (the ground truth), device tensors: `samples` points on each (seeds `seed`
    and `seed + 1`), the nearest sample of the other for each, `scores` of the two sets of distances plus samples and seed.
    Repeats exactly for a given seed."""
    if int(samples) != samples or samples < 1:
        raise ValueError(f"compare: samples is an integer >= 1; got {samples!r}")
    pa, pb = sample_surface(verts_a, faces_a, samples, seed), sample_surface(verts_b, faces_b, samples, int(seed) + 1)
    d_ab, d_ba = nearest(pa, pb)[0].double().sqrt(), nearest(pb, pa)[0].double().sqrt()
    return dict(scores(d_ab, d_ba, thresholds), samples=int(samples), seed=int(seed))


# ---------------------------------------------------------------------------------------------------- PLY
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("read_ply: not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("read_ply: the header has no end_header")
        w = line.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "end_header":
            break
        if w[0] == "format" and len(w) == 3:
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3:
            elements.append(dict(name=w[1], count=int(w[2]), props=[]))
        elif w[0] == "property" and elements and len(w) == 3 and w[1] in _PLY_TYPES:
            elements[-1]["props"].append((w[2], _PLY_TYPES[w[1]], None))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list" and w[2] in _PLY_TYPES and w[3] in _PLY_TYPES:
            if _PLY_TYPES[w[2]][0] == "f" or _PLY_TYPES[w[3]][0] == "f":
                raise ValueError(f"read_ply: a list of real counts or indices: {' '.join(w)}")
            elements[-1]["props"].append((w[4], _PLY_TYPES[w[3]], _PLY_TYPES[w[2]]))
        else:
            raise ValueError(f"read_ply: header line not understood: {line!r}")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"read_ply: format {fmt!r}; ascii and binary_little_endian are read")
    return fmt, elements


def _ply_faces(el, read_scalars, read_list):
    """the polygons of the face element -> list of corner lists; read_scalars(dtype code) -> one value, read_list(count code,
    item code) -> the items"""
    lists = [p for p in el["props"] if p[2] is not None]
    if len(lists) != 1 or lists[0][0] not in ("vertex_indices", "vertex_index"):
        raise ValueError("read_ply: the face element needs exactly one list property, vertex_indices")
    polys = []
    for _ in range(el["count"]):
        for name, item, count in el["props"]:
            if count is None:
                read_scalars(item)
            else:
                polys.append(read_list(count, item))
    return polys


def read_ply(path: str):
    """-> verts (V, 3) float32, faces (F, 3) int32 as numpy arrays.  ASCII and binary little-endian; the vertex properties x,
    y, z are float or double and its other scalar properties (normals, colours) are skipped; the face element has one list
    property vertex_indices (or vertex_index) of any integer count and index type beside scalar properties; a polygon
    (v0, v1, ..., vk) becomes the fan (v0, v1, v2), (v0, v2, v3), ..., one of fewer than three corners nothing; other elements
    are skipped when all their properties are scalar.  A file without a face element has F = 0.  ValueError for everything
    else: big-endian, a list property on a vertex, a missing x, y or z, a corner index outside [0, V), a truncated file."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        body = f.read()
    verts, polys, pos = None, [], 0
    tokens = body.split() if fmt == "ascii" else None
    for el in elements:
        scalar = all(p[2] is None for p in el["props"])
        if el["name"] == "vertex" or (scalar and el["name"] != "face"):
            if not scalar:
                raise ValueError("read_ply: a list property on the vertex element")
            names = [p[0] for p in el["props"]]
            if fmt == "ascii":
                n = el["count"] * len(names)
                if pos + n > len(tokens):
                    raise ValueError("read_ply: the file ends inside an element")
                rows = np.array(tokens[pos: pos + n], dtype=np.float64).reshape(el["count"], len(names)) if el["name"] == "vertex" else None
                table = None if rows is None else {name: rows[:, k] for k, name in enumerate(names)}
                pos += n
            else:
                dt = np.dtype([(f"{k}:{name}", "<" + code) for k, (name, code, _) in enumerate(el["props"])])
                if pos + dt.itemsize * el["count"] > len(body):
                    raise ValueError("read_ply: the file ends inside an element")
                rows = np.frombuffer(body, dtype=dt, count=el["count"], offset=pos)
                table = {name: rows[f"{k}:{name}"] for k, name in enumerate(names)}
                pos += dt.itemsize * el["count"]
            if el["name"] == "vertex":
                for axis in "xyz":
                    code = dict((p[0], p[1]) for p in el["props"]).get(axis)
                    if code not in ("f4", "f8"):
                        raise ValueError(f"read_ply: the vertex element needs a float or double property {axis}")
                verts = np.stack([table[a] for a in "xyz"], axis=-1).astype(np.float32)
        elif el["name"] == "face":
            if fmt == "ascii":
                def scalars(code):
                    nonlocal pos
                    pos += 1

                def items(count, item):
                    nonlocal pos
                    if pos >= len(tokens) or pos + 1 + int(tokens[pos]) > len(tokens):
                        raise ValueError("read_ply: the file ends inside the face element")
                    k = int(tokens[pos])
                    out = [int(t) for t in tokens[pos + 1: pos + 1 + k]]
                    pos += 1 + k
                    return out
            else:
                def scalars(code):
                    nonlocal pos
                    pos += np.dtype(code).itemsize

                def items(count, item):
                    nonlocal pos
                    cs, it = np.dtype(count).itemsize, np.dtype(item).itemsize
                    if pos + cs > len(body):
                        raise ValueError("read_ply: the file ends inside the face element")
                    k = int(np.frombuffer(body, dtype="<" + count, count=1, offset=pos)[0])
                    if k < 0 or pos + cs + k * it > len(body):
                        raise ValueError("read_ply: the file ends inside the face element")
                    out = np.frombuffer(body, dtype="<" + item, count=k, offset=pos + cs)
                    pos += cs + k * it
                    return out
                fast = _ply_uniform_faces(el, body, pos)
                if fast is not None:
                    polys, pos = fast
                    continue
            polys = _ply_faces(el, scalars, items)
        else:
            raise ValueError(f"read_ply: element {el['name']} has a list property")
    if verts is None:
        raise ValueError("read_ply: no vertex element")
    if isinstance(polys, np.ndarray):
        k = polys.shape[1]
        tris = np.stack([polys[:, [0, i, i + 1]] for i in range(1, k - 1)], axis=1).reshape(-1, 3) if k >= 3 else np.empty((0, 3), np.int64)
    else:
        tris = np.array([(p[0], p[i], p[i + 1]) for p in polys for i in range(1, len(p) - 1)], dtype=np.int64).reshape(-1, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError(f"read_ply: a corner index is outside [0, {len(verts)})")
    return np.ascontiguousarray(verts), np.ascontiguousarray(tris.astype(np.int32))


def _ply_uniform_faces(el, body, pos):
    """binary faces that all have the count of the first one, as one fixed-size record array -> ((F, k) int64, end) or None"""
    if el["count"] == 0:
        return None
    before = 0
    for name, item, count in el["props"]:
        if count is not None:
            break
        before += np.dtype(item).itemsize
    if pos + before + np.dtype(count).itemsize > len(body):
        return None
    k = int(np.frombuffer(body, dtype="<" + count, count=1, offset=pos + before)[0])
    if k < 0 or k > 255:
        return None
    fields = []
    for j, (name, item, count) in enumerate(el["props"]):
        if count is None:
            fields.append((f"{j}", "<" + item))
        else:
            fields += [("n", "<" + count), ("idx", "<" + item, (k,))]
    dt = np.dtype(fields)
    if pos + dt.itemsize * el["count"] > len(body):
        return None
    rows = np.frombuffer(body, dtype=dt, count=el["count"], offset=pos)
    if not (rows["n"] == k).all():
        return None
    return rows["idx"].astype(np.int64).reshape(el["count"], k), pos + dt.itemsize * el["count"]
