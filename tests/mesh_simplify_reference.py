"""numpy restatement of the mesh simplification by vertex clustering (include/ren_amd.h "mesh simplify"), written from the
specification and not from the kernels: explicit float64 operations in the specification's order, integer sums through
`np.add.at`, and a plain loop over a dict for the duplicates.  The GPU tests hold the kernels to it with exact equality.

The conditionals are written out (`np.where` on the stated comparison) and never `np.clip`, which passes NaN through: a
comparison with NaN is false, and the specification sends "not fl >= 0" to cell 0 and "not frac >= 0" to 0.
"""
import numpy as np

import mesh_reference as ref

MAX_CELLS = 2 ** 30
Q_ONE = 1048576.0                       # 2^20 quantisation steps across one cell
LO, HI = (-1.5, 0.25, 2.0), (2.5, 1.75, 3.5)


def box_constants(lo, hi, grid):
    """-> lo, inv, cw as float64 arrays: inv_a = g_a / (hi_a - lo_a), cw_a = (hi_a - lo_a) / g_a, each rounded once"""
    lo64, hi64 = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    g = np.array(grid, dtype=np.float64)
    ext = hi64 - lo64
    return lo64, g / ext, ext / g


def cells(verts, lo, hi, grid):
    """-> c (V, 3) int64: the cell coordinates of every vertex, q (V, 3) uint64: its quantised position within the cell"""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    lo64, inv, _ = box_constants(lo, hi, grid)
    g = np.array(grid, dtype=np.int64)
    with np.errstate(all="ignore"):
        r = (verts.astype(np.float64) - lo64) * inv
        fl = np.floor(r)
        low = ~(fl >= 0.0)                                                         # NaN lands here
        high = fl >= g.astype(np.float64)
        c = np.where(low, 0, np.where(high, g - 1, np.where(low | high, 0.0, fl).astype(np.int64)))
        frac = r - c.astype(np.float64)
        frac = np.where(~(frac >= 0.0), 0.0, frac)
        frac = np.where(frac > 1.0, 1.0, frac)
        q = np.floor(frac * Q_ONE + 0.5).astype(np.uint64)
    return c.astype(np.int64), q


def simplify(verts, faces, lo, hi, grid):
    """-> verts' (V', 3) float32, faces' (F', 3) int32, stats dict(clusters, degenerate, duplicate, orphans)"""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    gx, gy, gz = (int(v) for v in grid)
    assert min(gx, gy, gz) >= 1 and gx * gy * gz <= MAX_CELLS
    n_cells, V = gx * gy * gz, verts.shape[0]
    lo64, _, cw = box_constants(lo, hi, grid)
    c, q = cells(verts, lo, hi, grid)
    cell = (c[:, 0] * gy + c[:, 1]) * gz + c[:, 2]
    # ---- representatives by integer sums
    sums = np.zeros((n_cells, 3), dtype=np.uint64)
    count = np.zeros(n_cells, dtype=np.uint32)
    np.add.at(sums, cell, q)
    np.add.at(count, cell, np.uint32(1))
    occupied = np.flatnonzero(count)                                               # ascending cell id: the provisional ids
    prov = np.full(n_cells, -1, dtype=np.int64)
    prov[occupied] = np.arange(occupied.size)
    cc = np.stack([occupied // (gy * gz), (occupied // gz) % gy, occupied % gz], axis=-1).astype(np.float64)
    mean = sums[occupied].astype(np.float64) / count[occupied].astype(np.float64)[:, None]
    mean = mean / Q_ONE
    pos = (lo64 + (cc + mean) * cw).astype(np.float32)
    # ---- faces
    keep, seen = [], {}
    degenerate = duplicate = 0
    for f, (a, b, d) in enumerate(faces.tolist()):
        if not (0 <= a < V and 0 <= b < V and 0 <= d < V):
            degenerate += 1
            continue
        ids = (int(prov[cell[a]]), int(prov[cell[b]]), int(prov[cell[d]]))
        if ids[0] == ids[1] or ids[1] == ids[2] or ids[0] == ids[2]:
            degenerate += 1
            continue
        m = ids.index(min(ids))
        key = ids[m:] + ids[:m]                                                    # a rotation: the orientation stays
        if key in seen:
            duplicate += 1
            continue
        seen[key] = f
        keep.append(ids)
    kept = np.array(keep, dtype=np.int64).reshape(-1, 3)
    # ---- orphans
    used = np.zeros(occupied.size, dtype=bool)
    used[kept.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    stats = dict(clusters=int(occupied.size), degenerate=degenerate, duplicate=duplicate, orphans=int((~used).sum()))
    return pos[used].reshape(-1, 3), renumber[kept].astype(np.int32).reshape(-1, 3), stats


# ---- the inputs of the specification's table ---------------------------------------------------------------------------------
def random_field():
    return np.random.default_rng(5).standard_normal((13, 11, 9)).astype(np.float32), 0.8


def soup():
    rng = np.random.default_rng(11)
    lo, hi = np.array(LO), np.array(HI)
    verts = (lo - 0.1 + rng.random((5000, 3)) * (hi - lo + 0.2)).astype(np.float32)
    faces = rng.integers(0, 5000, (20000, 3)).astype(np.int32)
    return verts, faces


_MESH = {}


def mesh_of(name):
    """verts, faces of a table input (read-only, computed once)"""
    if name not in _MESH:
        if name == "soup":
            v, f = soup()
        else:
            sigma, level = random_field() if name == "standard_normal" else ref.field(name)
            v, f = ref.extract(sigma, level, LO, HI)[:2]
        v.setflags(write=False)
        f.setflags(write=False)
        _MESH[name] = (v, f)
    return _MESH[name]


# input, grid -> V, F in; V', F' out; degenerate, duplicate, orphans
TABLE = [("two_spheres", (8, 8, 8), 890, 1772, 84, 160, 1612, 0, 0),
         ("two_spheres", (16, 16, 16), 890, 1772, 304, 600, 1172, 0, 0),
         ("sphere", (4, 4, 4), 400, 796, 38, 72, 724, 0, 0),
         ("plane", (2, 2, 1), 45, 62, 0, 0, 62, 0, 3),
         ("standard_normal", (6, 5, 4), 2658, 4778, 117, 370, 4408, 0, 3),
         ("standard_normal", (3, 3, 2), 2658, 4778, 18, 46, 4725, 7, 0),
         ("standard_normal", (12, 10, 8), 2658, 4778, 832, 1680, 3098, 0, 11),
         ("soup", (3, 3, 2), 5000, 20000, 18, 1632, 3091, 15277, 0),
         ("soup", (5, 4, 3), 5000, 20000, 60, 16399, 1008, 2593, 0),
         ("soup", (1, 1, 1), 5000, 20000, 0, 0, 20000, 0, 1)]

_OUT = {}


def table_result(name, grid):
    """the restatement of one table row, computed once and handed out read-only"""
    key = (name, tuple(grid))
    if key not in _OUT:
        v, f, stats = simplify(*mesh_of(name), LO, HI, grid)
        v.setflags(write=False)
        f.setflags(write=False)
        _OUT[key] = (v, f, stats)
    return _OUT[key]
