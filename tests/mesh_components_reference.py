"""numpy restatement of the lattice components (include/ren_amd.h "mesh components") and of mesh.clean's rules, written from
the specification: a flood fill over the 14-neighbourhood of the marching-tetrahedra edges, lattice point by lattice point.

A point p = (i * ny + j) * nz + k is inside when sigma >= level (NaN outside).  S is the set of inside points, with `outside`
its complement.  The neighbours of p are p + e and p - e for the seven directions DIRS, where they lie in the lattice.
label[p] = the smallest linear index of p's component (-1 outside S); size[r] = the points of the component whose smallest
index is r (0 elsewhere); border[r] = 1 when it has a point on a face of the lattice (0 elsewhere).
"""
import numpy as np

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
NEIGHBOURS = DIRS + tuple(tuple(-c for c in d) for d in DIRS)


def selected(sigma, level, outside=False):
    inside = np.asarray(sigma, dtype=np.float32) >= np.float32(level)             # NaN compares false: outside
    return ~inside if outside else inside


def components(sigma, level, outside=False):
    """-> label (nx, ny, nz) int32, size (n,) int32, border (n,) uint8"""
    sel = selected(sigma, level, outside)
    nx, ny, nz = sel.shape
    n = nx * ny * nz
    label = np.full(n, -1, dtype=np.int32)
    size = np.zeros(n, dtype=np.int32)
    border = np.zeros(n, dtype=np.uint8)
    flat = sel.reshape(-1)
    for root in range(n):                                                         # ascending: the first point met is the smallest
        if not flat[root] or label[root] >= 0:
            continue
        label[root] = root
        stack = [root]
        while stack:
            p = stack.pop()
            i, j, k = p // (ny * nz), p // nz % ny, p % nz
            size[root] += 1
            if i in (0, nx - 1) or j in (0, ny - 1) or k in (0, nz - 1):
                border[root] = 1
            for di, dj, dk in NEIGHBOURS:
                a, b, c = i + di, j + dj, k + dk
                if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz:
                    q = (a * ny + b) * nz + c
                    if flat[q] and label[q] < 0:
                        label[q] = root
                        stack.append(q)
    return label.reshape(nx, ny, nz), size, border


def kept(sizes, min_points=1, largest=None):
    """sizes of the components in ascending order of their roots -> bool per component: size >= min_points and (largest is None
    or rank < largest), ranked by (size descending, root ascending)"""
    sizes = [int(s) for s in sizes]
    order = sorted(range(len(sizes)), key=lambda c: (-sizes[c], c))
    rank = {c: r for r, c in enumerate(order)}
    return np.array([sizes[c] >= min_points and (largest is None or rank[c] < largest) for c in range(len(sizes))], dtype=bool)


def clean(sigma, level, min_points=1, largest=None, fill_cavities=False):
    """-> (sigma', stats): 1. the inside components that are not kept become -inf; 2. with fill_cavities the outside components
    of THAT lattice without a point on a face of the lattice become +inf"""
    out = np.array(sigma, dtype=np.float32, copy=True)
    label, size, _ = components(out, level)
    roots = np.flatnonzero(size)
    keep = kept(size[roots], min_points, largest)
    stats = dict(components=len(roots), kept=int(keep.sum()), dropped_points=int(size[roots[~keep]].sum()), cavities=0,
                 filled_points=0)
    out[np.isin(label, roots[~keep])] = -np.inf
    if fill_cavities:
        label, size, border = components(out, level, outside=True)
        roots = np.flatnonzero(size)
        closed = roots[border[roots] == 0]
        stats.update(cavities=len(closed), filled_points=int(size[closed].sum()))
        out[np.isin(label, closed)] = np.inf
    return out, stats


def ball(res, centre, radius):
    """sigma = radius - |x - centre| on the lattice, coordinates = lattice indices, float32"""
    i, j, k = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in res), indexing="ij")
    c = [np.float32(v) for v in centre]
    return (np.float32(radius) - np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2, dtype=np.float32)).astype(np.float32)


def random_lattice(res, share, seed=7):
    """seeded uniform float32 in [0, 1) and the level above which about `share` of the points lie -> sigma, level"""
    sigma = np.random.default_rng(seed).random(res, dtype=np.float32)
    return sigma, float(np.float32(1.0 - share))
