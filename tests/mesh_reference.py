"""numpy restatement of the level-set mesh extraction (include/ren_amd.h "mesh"), written from the specification and not from
the kernel: plain loops over lattice points, cubes and tetrahedra.  The GPU tests hold the kernels to it index for index.

Lattice nx x ny x nz over the box [lo, hi], point (i, j, k) at linear index (i * ny + j) * nz + k.  A point is inside when
sigma >= level (NaN outside).  Every cube is split into the six Kuhn tetrahedra v0 = base, v1 = v0 + e_a, v2 = v1 + e_b,
v3 = v2 + e_c, the permutations (a, b, c) in lexicographic order.  Every tetrahedron edge leaves its lower-numbered end in one
of the seven directions DIRS; that end owns it.  One vertex per owned edge whose ends differ, ordered by owner index, then
direction; faces ordered by cube index, tetrahedron, triangle.

The orientation of a triangle is decided HERE from integer geometry: the edge MIDPOINTS of the tetrahedron (never the
interpolated positions) give a normal, and the triangle's last two corners are swapped when it points from the outside
vertices to the inside ones.  The kernel carries the same decision as a 16-entry table and the parity of the permutation;
`flip_by_table` restates that form, and tests/test_mesh_cpu.py holds the two to each other for all 6 x 14 cases.
"""
import itertools

import numpy as np

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
E_OF = {d: e for e, d in enumerate(DIRS)}
PERMS = tuple(sorted(itertools.permutations(range(3))))
UNIT = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
MAX_POINTS = 2 ** 30
FLIP_TABLE = 0x4D24                     # bit s: an even-permutation tetrahedron with inside set s swaps its triangles' last two corners
ODD_PERMS = 0b100110                    # bit t: permutation t is odd


def tet_vertices(t):
    """the four corner offsets (within the cube) of tetrahedron t"""
    v = [(0, 0, 0)]
    for axis in PERMS[t]:
        v.append(tuple(a + b for a, b in zip(v[-1], UNIT[axis])))
    return v


def tet_triangles(s):
    """triangles of a tetrahedron whose inside set is the 4-bit s (bit m = v_m inside), before orientation: each corner is a
    tetrahedron edge (m, n), m < n"""
    ins = [m for m in range(4) if s >> m & 1]
    out = [m for m in range(4) if not s >> m & 1]
    edge = lambda p, q: (min(p, q), max(p, q))
    if len(ins) == 1:
        return [[edge(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[edge(out[0], i) for i in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        ac, ad, bd, bc = edge(a, c), edge(a, d), edge(b, d), edge(b, c)
        return [[ac, ad, bd], [ac, bd, bc]]
    return []


def flip_by_midpoints(t, s):
    """True when the triangles of tet_triangles(s) in tetrahedron t point from outside to inside as listed"""
    v = np.array(tet_vertices(t), dtype=np.int64)
    ins = [m for m in range(4) if s >> m & 1]
    out = [m for m in range(4) if not s >> m & 1]
    towards_outside = len(ins) * v[out].sum(0) - len(out) * v[ins].sum(0)          # (mean of outside - mean of inside) x |ins| |out|
    flips = []
    for tri in tet_triangles(s):
        m = [v[p] + v[q] for p, q in tri]                                          # twice the edge midpoints
        dot = int(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), towards_outside))
        assert dot != 0
        flips.append(dot < 0)
    assert len(set(flips)) == 1
    return flips[0]


def flip_by_table(t, s):
    """the kernel's form of the same decision"""
    return bool((FLIP_TABLE >> s ^ ODD_PERMS >> t) & 1)


_TETS = [tet_vertices(t) for t in range(6)]
_FLIP = {(t, s): flip_by_midpoints(t, s) for t in range(6) for s in range(1, 15)}


def spacing(lo, hi, res):
    """h per axis: computed in float64, rounded to float32"""
    return tuple(np.float32((float(hi[a]) - float(lo[a])) / (res[a] - 1)) for a in range(3))


def extract(sigma, level, lo, hi, dtype=np.float32):
    """-> verts (V, 3) `dtype`, faces (F, 3) int32, mask (nx, ny, nz) uint8, fcount (cubes,) int32.
    dtype float32: every operation rounded on its own, as the kernel; float64: the same expressions on the same float32 inputs
    (sigma, level, lo, hi and h are float32 values either way)."""
    sigma = np.asarray(sigma, dtype=np.float32)
    nx, ny, nz = sigma.shape
    assert min(nx, ny, nz) >= 2 and nx * ny * nz <= MAX_POINTS
    F = dtype
    level32 = np.float32(level)
    h32 = spacing(lo, hi, (nx, ny, nz))
    lo32, hi32 = [np.float32(v) for v in lo], [np.float32(v) for v in hi]
    inside = (sigma >= level32).tolist()                                           # NaN compares false: outside
    n = (nx, ny, nz)
    mask = np.zeros(n, dtype=np.uint8)
    verts = []
    voff = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    voff[i, j, k] = len(verts)
                    for e, (di, dj, dk) in enumerate(DIRS):
                        qi, qj, qk = i + di, j + dj, k + dk
                        if qi >= nx or qj >= ny or qk >= nz or inside[i][j][k] == inside[qi][qj][qk]:
                            continue
                        mask[i, j, k] |= 1 << e
                        sp, sq = F(sigma[i, j, k]), F(sigma[qi, qj, qk])
                        t = (F(level32) - sp) / (sq - sp)
                        if not np.isfinite(t):
                            t = F(0.5)
                        x = []
                        for a, (idx, d) in enumerate(((i, di), (j, dj), (k, dk))):
                            u = F(idx) + t * F(d)
                            x.append(min(F(lo32[a]) + u * F(h32[a]), F(hi32[a])))  # the one step past lo + u h: never past hi
                        verts.append(x)
    pop = lambda m: bin(int(m)).count("1")

    def vid(p, q):
        d = tuple(b - a for a, b in zip(p, q))
        return int(voff[p]) + pop(mask[p] & ((1 << E_OF[d]) - 1))

    faces, fcount = [], []
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                before = len(faces)
                for t in range(6):
                    c = [(i + a, j + b, k + d) for a, b, d in _TETS[t]]
                    s = sum(1 << m for m in range(4) if inside[c[m][0]][c[m][1]][c[m][2]])
                    for tri in tet_triangles(s):
                        ids = [vid(c[p], c[q]) for p, q in tri]
                        if _FLIP[t, s]:
                            ids = [ids[0], ids[2], ids[1]]
                        faces.append(ids)
                fcount.append(len(faces) - before)
    return (np.array(verts, dtype=dtype).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3), mask,
            np.array(fcount, dtype=np.int32))


def topology(verts, faces):
    """-> dict(closed: every directed edge occurs once and its reverse once; euler: V - E + F; boundary: the undirected edges
    used by exactly one face, as (lo id, hi id) pairs; n_boundary: their number)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    directed = {}
    for f in faces:
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            directed[(int(a), int(b))] = directed.get((int(a), int(b)), 0) + 1
    closed = all(c == 1 and directed.get((b, a), 0) == 1 for (a, b), c in directed.items())
    undirected = {}
    for (a, b), c in directed.items():
        key = (min(a, b), max(a, b))
        undirected[key] = undirected.get(key, 0) + c
    boundary = sorted(e for e, c in undirected.items() if c == 1)
    return dict(closed=closed, euler=len(verts) - len(undirected) + len(faces), boundary=boundary, n_boundary=len(boundary))


def zero_area(verts, faces):
    """number of triangles whose corners are collinear or coincide (float64 cross product exactly zero)"""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return int((np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) == 0).all(axis=1).sum())


# ---- the four fields of the specification's table (coordinates are lattice indices; sigma and the distances float32) ------
def _grid(res):
    return np.meshgrid(*(np.arange(n, dtype=np.float32) for n in res), indexing="ij")


def sphere_field(res, centre, radius):
    i, j, k = _grid(res)
    c = [np.float32(v) for v in centre]
    d = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2, dtype=np.float32)
    return (np.float32(radius) - d).astype(np.float32)


def field(name):
    """-> sigma (float32), level"""
    if name == "sphere":
        return sphere_field((9, 9, 9), (4.1, 3.9, 4.2), 2.7), 0.0
    if name == "two_spheres":
        return np.maximum(sphere_field((17,) * 3, (4.1, 4.2, 3.9), 2.6), sphere_field((17,) * 3, (11.7, 12.1, 11.9), 3.1)), 0.0
    if name == "plane":
        # 1.3, 0.2 and 0.1 are not float32 (or float64) numbers, and the plane passes through lattice points -- (2, 2, 1) for
        # one -- so the classification there depends on how the expression is evaluated.  The specification's counts (45, 62,
        # 26 boundary edges) are those of the expression evaluated in float64 and then stored as float32 (sigma(2, 2, 1) =
        # 2.8e-17: inside); evaluated left to right in float32 the same point is -5.2e-8 and the counts are 43, 60, 24.
        i, j, k = (a.astype(np.float64) for a in _grid((5, 4, 3)))
        return (1.3 - 0.5 * i - 0.2 * j + 0.1 * k).astype(np.float32), 0.0
    if name == "octahedron":
        i, j, k = _grid((7, 7, 7))
        return (2 - np.abs(i - 3) - np.abs(j - 3) - np.abs(k - 3)).astype(np.float32), 0.0
    raise KeyError(name)


# what the specification's table states for each: V, F, closed, Euler number
TABLE = {"sphere": (400, 796, True, 2), "two_spheres": (890, 1772, True, 4), "plane": (45, 62, False, 1),
         "octahedron": (194, 384, True, 2)}
