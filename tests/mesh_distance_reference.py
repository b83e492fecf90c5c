"""numpy restatement of the exact nearest-neighbour search (include/ren_amd.h "mesh distance"), written from the header's
definition: `brute` is the definition itself, `grid_search` the kernel's algorithm shell by shell -- cells, grouping, shells,
the stopping margin -- so that its logic can be held to `brute` without a GPU.  Plus the inputs both test files use."""
import numpy as np

F32 = np.float32


def brute(q, p):
    """q (nq, 3), p (nr, 3) float32 -> d2 (nq,) float32, idx (nq,) int32: d2 = (dx*dx + dy*dy) + dz*dz with every operation
    rounded to float32, the minimum over p and the smallest index that attains it (np.argmin takes the first)"""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    d2 = np.empty(len(q), F32)
    idx = np.empty(len(q), np.int32)
    for s in range(0, len(q), 512):
        d = q[s: s + 512, None, :] - p[None, :, :]
        m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert m.dtype == F32
        a = np.argmin(m, axis=1)
        idx[s: s + 512] = a
        d2[s: s + 512] = m[np.arange(len(a)), a]
    return d2, idx


def inv_of(h):
    return F32(1.0 / float(F32(h)))                                    # what ops.nn_cells / nn_search hand the kernels


def cell_coords(pts, lo, h, grid):
    """(n, 3) int32 per-axis cells: clamp(floor((p - lo) * inv_h), 0, g - 1) in float32, NaN to 0"""
    pts, lo = np.asarray(pts, F32).reshape(-1, 3), np.asarray(lo, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        fl = np.floor((pts - lo) * inv_of(h))
    assert fl.dtype == F32
    g = np.asarray(grid, np.int64)
    gf = g.astype(F32)
    inside = np.where((fl >= 0) & (fl < gf), fl, F32(0)).astype(np.int64)          # NaN compares false: cell 0
    return np.where(fl >= gf, g - 1, inside).astype(np.int32)


def cells(pts, lo, h, grid):
    """linear ids (z * gy + y) * gx + x, int32"""
    c = cell_coords(pts, lo, h, grid).astype(np.int64)
    return ((c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0]).astype(np.int32)


def auto_grid(p):
    """the grid mesh_distance.nearest searches on"""
    from robust_e_nerf_amd import mesh_distance
    p = np.asarray(p, F32)
    lo, hi = p.min(axis=0), p.max(axis=0)
    h, grid = mesh_distance.nn_grid(lo.tolist(), hi.tolist(), len(p))
    return [float(v) for v in lo], h, grid


def grid_search(q, p, lo=None, h=None, grid=None):
    """the kernel's search, one query at a time: the references grouped by cell (stable, so ascending index within a cell), the
    shells r = 0, 1, ... of the query's clamped cell clipped to the grid -- a row on a y or z face of the shell as one range
    of the grouped references, another row as its two end cells -- and after shell r >= 1 the stop when
    best < ((r - 2^-6) * h)^2 in float32, after any shell when the block covers the grid.  Default grid: `auto_grid(p)`."""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    if lo is None:
        lo, h, grid = auto_grid(p)
    gx, gy, gz = (int(v) for v in grid)
    h32 = F32(h)
    ids = cells(p, lo, h, grid)
    order = np.argsort(ids, kind="stable")
    ps = p[order]
    start = np.searchsorted(ids[order], np.arange(gx * gy * gz + 1)).tolist()
    cq = cell_coords(q, lo, h, grid).tolist()
    d2 = np.empty(len(q), F32)
    idx = np.empty(len(q), np.int32)
    for n, (cx, cy, cz) in enumerate(cq):
        best, best_i = F32(np.inf), None
        cover = max(cx, gx - 1 - cx, cy, gy - 1 - cy, cz, gz - 1 - cz)
        for r in range(max(gx, gy, gz)):
            ranges = []
            x0, x1 = max(cx - r, 0), min(cx + r, gx - 1)
            for z in range(max(cz - r, 0), min(cz + r, gz - 1) + 1):
                for y in range(max(cy - r, 0), min(cy + r, gy - 1) + 1):
                    row = (z * gy + y) * gx
                    if abs(z - cz) == r or abs(y - cy) == r:
                        ranges.append((start[row + x0], start[row + x1 + 1]))
                    else:
                        ranges += [(start[row + x], start[row + x + 1]) for x in (cx - r, cx + r) if 0 <= x < gx]
            for a, b in ranges:
                if a == b:
                    continue
                with np.errstate(over="ignore"):
                    d = q[n] - ps[a:b]
                    m = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                for k in np.flatnonzero(m <= best):                    # the candidates that can change the answer
                    i = int(order[a + k])
                    if m[k] < best or (m[k] == best and (best_i is None or i < best_i)):
                        best, best_i = m[k], i
            if r >= cover:
                break
            if r >= 1:
                b = F32(F32(r) - F32(0.015625)) * h32
                assert b.dtype == F32
                if best < b * b:
                    break
        d2[n], idx[n] = best, best_i
    return d2, idx


# ---------------------------------------------------------------------------------------------------- inputs
SIZES = [(1, 1), (65, 1), (1, 65), (63, 64), (1000, 4097), (4097, 1000)]
INPUTS = ["uniform", "cluster_far_queries", "plane", "line", "cell_faces", "ties"]


def make(name, nq, nr, seed=0):
    """(q, p) float32 for one of INPUTS at the given sizes"""
    rng = np.random.default_rng([seed, nq, nr, INPUTS.index(name)])
    if name == "uniform":                                              # a box that is no cube and does not start at 0
        lo, ext = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 1.0, 2.0])
        return (lo + ext * rng.random((nq, 3))).astype(F32), (lo + ext * rng.random((nr, 3))).astype(F32)
    if name == "cluster_far_queries":                                  # queries 100 box widths away, on every side of the box
        p = (np.array([5.0, -3.0, 1.0]) + 1e-3 * rng.random((nr, 3))).astype(F32)
        side = rng.integers(-1, 2, (nq, 3))
        side[side.any(axis=1) == 0] = (1, 0, -1)
        side[:min(nq, 6)] = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])[:min(nq, 6)]
        return (np.array([5.0, -3.0, 1.0]) + 0.1 * side + 1e-3 * rng.random((nq, 3))).astype(F32), p
    if name == "plane":                                                # z has no extent: gz = 1
        p = np.concatenate([rng.random((nr, 2)), np.full((nr, 1), 0.25)], axis=1).astype(F32)
        return (rng.random((nq, 3)) * [1.2, 1.2, 0.5] - [0.1, 0.1, 0.0]).astype(F32), p
    if name == "line":                                                 # x and z have no extent
        p = np.stack([np.full(nr, -2.0), 4 * rng.random(nr), np.full(nr, 7.0)], axis=1).astype(F32)
        return (np.array([-2.0, 0.0, 7.0]) + rng.random((nq, 3)) * [1.0, 4.0, 1.0] - [0.5, 0.0, 0.5]).astype(F32), p
    if name == "cell_faces":                                           # references exactly on cell faces of the grid they get
        corner = np.array([0.0, 0.0, 0.0], F32)
        box_hi = np.array([1.0, 1.0, 1.0], F32)
        from robust_e_nerf_amd import mesh_distance
        h, grid = mesh_distance.nn_grid(corner.tolist(), box_hi.tolist(), nr)
        h32 = F32(h)
        k = np.stack([rng.integers(0, g + 1, nr) for g in grid], axis=1)
        p = np.minimum(corner + k.astype(F32) * h32, box_hi).astype(F32)
        if nr >= 2:
            p[0], p[1] = corner, box_hi                                # the box, and with it the grid, is the one above
        kq = np.stack([rng.integers(0, g, nq) for g in grid], axis=1).astype(F32)
        on_face = rng.random((nq, 3)) < 0.5                            # per axis: on a face, or at the centre of a cell
        return (corner + (kq + np.where(on_face, F32(0), F32(0.5))) * h32).astype(F32), p
    if name == "ties":                                                 # duplicates, and queries midway between two references
        base = rng.integers(-4, 5, (max(1, (nr + 2) // 3), 3)).astype(F32) * F32(0.25)
        p = base[rng.integers(0, len(base), nr)]                       # every point several times over, in no order
        pick = rng.integers(0, nr, (nq, 2))
        return ((p[pick[:, 0]] + p[pick[:, 1]]) * F32(0.5)).astype(F32), p
    raise KeyError(name)


def corner_case(nq=65):
    """one reference in a corner cell of a 16^3 grid that is otherwise empty, the queries in the opposite corner cell: the walk
    over the whole grid.  -> q, p, lo, h, grid"""
    rng = np.random.default_rng(11)
    lo, h, grid = [0.0, 0.0, 0.0], 0.0625, (16, 16, 16)
    p = np.array([[0.01, 0.02, 0.03]], F32)
    return (0.9375 + 0.0625 * rng.random((nq, 3))).astype(F32), p, lo, h, grid


def one_cell_cluster(nq=65, nr=64):
    """all references in one cell of an 8^3 grid, the queries 100 grid widths away on every side -> q, p, lo, h, grid"""
    rng = np.random.default_rng(12)
    lo, h, grid = [-1.0, -1.0, -1.0], 0.25, (8, 8, 8)
    p = (np.array([0.30, -0.70, 0.55]) + 0.2 * rng.random((nr, 3))).astype(F32)
    side = rng.integers(-1, 2, (nq, 3))
    side[side.any(axis=1) == 0] = (-1, 1, 0)
    return (200.0 * side + rng.random((nq, 3))).astype(F32), p, lo, h, grid
