"""Mesh distance on the GPU (csrc/ren_mesh_distance.hip, robust_e_nerf_amd/mesh_distance.py): the grid nearest-neighbour search
against the numpy brute force of tests/mesh_distance_reference.py with exact equality of the squared distances and the indices,
every case -- the result is a function of the two point sets alone, so there is no tolerance on it anywhere in this file; then
the scores of two spheres, and the simplification error of mesh.export."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import mesh_distance_reference as dref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, mesh, mesh_distance, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, mesh_distance, mesh


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def case(name, nq, nr):
    q, p = dref.make(name, nq, nr)
    want = dref.brute(q, p)
    for a in (q, p, *want):
        a.setflags(write=False)
    return q, p, want


def same(got, want, tag):
    d2, idx = got
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.is_cuda and idx.is_cuda
    assert d2.shape == idx.shape == (len(want[0]),)
    assert torch.equal(idx.cpu(), torch.from_numpy(np.array(want[1]))), (tag, "idx")
    assert torch.equal(d2.cpu().view(torch.int32), torch.from_numpy(np.array(want[0])).view(torch.int32)), (tag, "d2")


def records_of(ops, p, lo, h, grid):
    """what mesh_distance.nearest_on_grid builds, by hand: the records grouped by cell and the cell starts"""
    cells = ops.nn_cells(p, lo, h, grid)
    cells, order = torch.sort(cells, stable=True)
    n_cells = grid[0] * grid[1] * grid[2]
    start = torch.searchsorted(cells, torch.arange(n_cells + 1, device=DEV, dtype=torch.int32), out_int32=True)
    rec = torch.cat([p[order].view(torch.int32), order.to(torch.int32)[:, None]], dim=1).contiguous()
    return rec.view(torch.float32), start


# ---------------------------------------------------------------------------------------------------- nearest
@pytest.mark.parametrize("nq,nr", dref.SIZES, ids=[f"{a}x{b}" for a, b in dref.SIZES])
@pytest.mark.parametrize("name", dref.INPUTS)
def test_nearest_equals_brute_force(amd, name, nq, nr):
    _, md, _ = amd
    q, p, want = case(name, nq, nr)
    qd, pd = dev(q), dev(p)
    same(md.nearest(qd, pd), want, name)
    assert torch.equal(qd.cpu(), torch.from_numpy(np.array(q))) and torch.equal(pd.cpu(), torch.from_numpy(np.array(p)))


def test_full_grid_walk_from_the_opposite_corner(amd):
    _, md, _ = amd
    q, p, lo, h, grid = dref.corner_case()
    same(md.nearest_on_grid(dev(q), dev(p), lo, h, grid), dref.brute(q, p), "corner")


def test_all_references_in_one_cell_and_queries_far_outside(amd):
    ops, md, _ = amd
    q, p, lo, h, grid = dref.one_cell_cluster()
    assert len(set(ops.nn_cells(dev(p), lo, h, grid).tolist())) == 1
    same(md.nearest_on_grid(dev(q), dev(p), lo, h, grid), dref.brute(q, p), "cluster")


@pytest.mark.parametrize("name,lo", [("uniform", [-1.0, 2.0, 0.5]), ("ties", [-1.0, -1.0, -1.0]), ("cell_faces", [0.0, 0.0, 0.0])])
def test_nn_search_gives_one_result_on_three_grids(amd, name, lo):
    ops, _, _ = amd
    q, p, want = case(name, 1000, 4097)
    qd, pd = dev(q), dev(p)
    outs = []
    for h, grid in ((8.0, (1, 1, 1)), (0.7, (3, 5, 7)), (0.125, (16, 16, 16))):
        rec, start = records_of(ops, pd, lo, h, grid)
        outs.append(ops.nn_search(qd, rec, start, lo, h, grid))
        same(outs[-1], want, (name, grid))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])


def test_nn_cells_equals_the_restatement(amd):
    ops, md, _ = amd
    rng = np.random.default_rng(2)
    lo, h, grid = [-1.0, 0.5, 2.0], 0.3, (7, 5, 3)
    h32 = np.float32(h)
    inside = (np.array(lo) + rng.random((3000, 3)) * np.array(grid) * h).astype(np.float32)
    outside = (np.array(lo) + (rng.random((1000, 3)) * 3 - 1) * np.array(grid) * h).astype(np.float32)
    k = np.stack([rng.integers(-1, g + 2, 1000) for g in grid], axis=1)
    faces = (np.array(lo, np.float32) + k.astype(np.float32) * h32).astype(np.float32)   # on the faces, the outer ones included
    hair = np.nextafter(faces, np.where(rng.random(faces.shape) < 0.5, -np.inf, np.inf).astype(np.float32))
    special = np.array([[np.nan, 1, 2.5], [np.inf, -np.inf, 2.5], [3e38, -3e38, 0], [0, 0, 0]], dtype=np.float32)
    pts = np.concatenate([inside, outside, faces, hair, special])
    want = dref.cells(pts, lo, h, grid)
    assert len(np.unique(want)) == 7 * 5 * 3
    got = ops.nn_cells(dev(pts), lo, h, grid)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(want))
    for nr in (1, 64, 4097):                                                        # and on the grid nearest picks
        p = case("cell_faces", 1000, nr)[1] if nr > 1 else case("cell_faces", 65, 1)[1]
        lo, h, grid = dref.auto_grid(p)
        assert torch.equal(ops.nn_cells(dev(p), lo, h, grid).cpu(), torch.from_numpy(dref.cells(p, lo, h, grid)))


def test_empty_queries_launch_nothing_and_bad_inputs_are_refused(amd, monkeypatch):
    ops, md, _ = amd
    q, p, _ = case("uniform", 63, 64)
    qd, pd = dev(q), dev(p)
    def refuse(*a, **k):
        raise AssertionError("a kernel was launched for no query")
    with monkeypatch.context() as m:
        m.setattr(ops, "nn_search", refuse)
        d2, idx = md.nearest(qd[:0], pd)
        assert d2.shape == idx.shape == (0,) and d2.dtype == torch.float32 and idx.dtype == torch.int32
    with pytest.raises(ValueError, match="no reference"):
        md.nearest(qd, pd[:0])
    for bad in (float("nan"), float("inf"), -float("inf")):
        broken = pd.clone()
        broken[5, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            md.nearest(qd, broken)
        broken = qd.clone()
        broken[7, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            md.nearest(broken, pd)
    for a, b in ((qd.double(), pd), (qd, pd.double()), (qd.t().contiguous().t(), pd), (qd.cpu(), pd), (qd, pd[:, :2].contiguous())):
        with pytest.raises(ValueError):
            md.nearest(a, b)


# ---------------------------------------------------------------------------------------------------- compare
LEVEL = 4                     # icosahedron subdivided four times: 2562 vertices, 5120 faces


def icosphere(level, radius):
    t = (1 + math.sqrt(5)) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (radius * np.array(v)).astype(np.float32), np.array(f, np.int32)


def test_compare_two_spheres(amd):
    """Radius 1 (the mesh) against radius 1.01 (the ground truth), both at LEVEL.  The flat faces sag below their sphere by
    at most R (1 - cos a), a the angle between a face's centre and its corners: measured on the tessellation below, and below
    0.0012 R at LEVEL 4.  So mesh A lies between radius 1 - sag and 1 and mesh B between 1.01 (1 - sag) and 1.01, and -- going
    along the radius -- every point of one surface is between 1.01 (1 - sag) - 1 > 0.0085 and 0.01 + sag < 0.0115 from the other
    surface: the derived bounds on both means, inside the [0.005, 0.02] asserted.  The distances here are between SAMPLES,
    which adds the tangential offset t of the nearest of n = 20 000 samples on an area of 4 pi: P(t > x) = exp(-n x^2 / 4), so
    sqrt(gap^2 + t^2) has a mean of about 0.0165 at a gap of 0.01, and exceeds 0.05 for one sample in 10^5: precision and
    recall 1 there, and 0 at 0.001, a tenth of the smallest gap."""
    _, md, _ = amd
    va, fa = icosphere(LEVEL, 1.0)
    vb, fb = icosphere(LEVEL, 1.01)
    assert va.shape == (2562, 3) and fa.shape == (5120, 3)
    corners = va.astype(np.float64)[fa]
    centre = corners.mean(axis=1)
    sag = 1 - (centre / np.linalg.norm(centre, axis=1, keepdims=True) * corners[:, 0]).sum(axis=1).min()
    assert 0 < sag < 0.0012 and 1.01 * (1 - sag) - 1 > 0.0085 and 0.01 + sag < 0.0115
    args = (dev(va), dev(fa), dev(vb), dev(fb))
    s = md.compare(*args, samples=20000, seed=0, thresholds=(0.05, 0.001))
    print(s, flush=True)
    assert 0.005 <= s["accuracy"]["mean"] <= 0.02 and 0.005 <= s["completeness"]["mean"] <= 0.02
    assert s["accuracy"]["mean"] >= 1.01 * (1 - sag) - 1 and s["completeness"]["mean"] >= 1.01 * (1 - sag) - 1
    assert s["chamfer"] == 0.5 * (s["accuracy"]["mean"] + s["completeness"]["mean"])
    assert s["hausdorff"] == max(s["accuracy"]["max"], s["completeness"]["max"]) >= s["accuracy"]["rms"] >= s["accuracy"]["mean"]
    near, far = s["thresholds"]
    assert near == dict(threshold=0.05, precision=1.0, recall=1.0, fscore=1.0)
    assert far == dict(threshold=0.001, precision=0.0, recall=0.0, fscore=0.0)
    assert md.compare(*args, samples=20000, seed=0, thresholds=(0.05, 0.001)) == s
    assert md.compare(*args, samples=20000, seed=1, thresholds=(0.05, 0.001)) != s
    pa = md.sample_surface(args[0], args[1], 20000, 0)                              # the samples lie on the faces: radius in [1 - sag, 1]
    radius = pa.double().norm(dim=-1)
    assert pa.is_cuda and float(radius.min()) >= 1 - sag - 1e-6 and float(radius.max()) <= 1 + 1e-6


# ---------------------------------------------------------------------------------------------------- export
class SphereField:
    """what mesh.export asks of a renderer, over the analytic sphere of tests/mesh_reference.py's "sphere" field: sigma =
    2.7 - |x - (4.1, 3.9, 4.2)| in the box [0, 8]^3 (at resolution 9 the lattice points are that field's)"""
    CENTRE, RADIUS = (4.1, 3.9, 4.2), 2.7

    def __init__(self):
        self.cfg = types.SimpleNamespace(aabb=(0.0, 0.0, 0.0, 8.0, 8.0, 8.0))
        self.field = types.SimpleNamespace(flat=torch.zeros(1, device=DEV))

    def query_density(self, pts):
        return self.RADIUS - (pts - torch.tensor(self.CENTRE, device=pts.device)).norm(dim=-1)


def test_export_with_simplify_error(amd, tmp_path):
    """K = 2 on a lattice of 33 points per axis (spacing s = 0.25).  A vertex moves to the mean of its cluster cell's members,
    so by less than the cell's diagonal sqrt(3) K s, and a point of a face moves by a convex combination of its corners'
    moves: the surfaces are within sqrt(3) K s of each other.  The scores are between samples: the nearest of n samples on an
    area A is further than rho with probability exp(-n pi rho^2 / A); at rho = 2 sqrt(A ln n / (pi n)) that is n^-4, so with
    the 2 n queries of a call the slack rho is exceeded in fewer than one call in 10^8."""
    _, md, mesh = amd
    r, res, k, n = SphereField(), 33, 2, 20000
    spacing = 8.0 / (res - 1)
    plain = mesh.export(r, str(tmp_path / "plain.ply"), res, 0.0, normals=False, simplify=k)
    stats = mesh.export(r, str(tmp_path / "scored.ply"), res, 0.0, normals=False, simplify=k, simplify_error=n)
    err = stats.pop("simplify_error")
    print(err, flush=True)
    assert stats == plain and "simplify_error" not in plain                          # nothing else changes
    assert open(tmp_path / "plain.ply", "rb").read() == open(tmp_path / "scored.ply", "rb").read()
    assert err["samples"] == n and err["spacing"] == spacing
    area = 4 * math.pi * SphereField.RADIUS ** 2
    slack = 2 * math.sqrt(area * math.log(n) / (math.pi * n))
    assert 0 < err["hausdorff"] <= math.sqrt(3) * k * spacing + slack
    assert err["in_spacings"]["hausdorff"] == err["hausdorff"] / spacing
    assert err["in_spacings"]["accuracy"] == {key: v / spacing for key, v in err["accuracy"].items()}
    assert err["in_spacings"]["completeness"]["mean"] == err["completeness"]["mean"] / spacing
    assert [t["threshold"] for t in err["thresholds"]] == [0.5 * spacing, spacing]
    floor = err["sampling_floor"]                                                   # the extracted mesh against itself: samples, not error
    assert 0 < floor["chamfer"] <= slack and 0 < floor["hausdorff"] <= slack
    assert floor["in_spacings"] == dict(chamfer=floor["chamfer"] / spacing, hausdorff=floor["hausdorff"] / spacing)
    verts, faces = (torch.from_numpy(a).to(DEV) for a in md.read_ply(str(tmp_path / "scored.ply")))
    sigma = mesh.sample_density(r, (0.0,) * 3, (8.0,) * 3, res)
    v0, f0 = mesh.extract(sigma, 0.0, (0.0,) * 3, (8.0,) * 3)
    again = md.compare(verts, faces, v0, f0, n, 0, (0.5 * spacing, spacing))         # the call export makes, by hand
    assert {key: err[key] for key in again} == again


def test_export_without_the_option_is_unchanged(amd, tmp_path, monkeypatch):
    _, md, mesh = amd
    r = SphereField()

    def refuse(*a, **k):
        raise AssertionError("mesh.export measured a distance without being asked to")
    monkeypatch.setattr(md, "compare", refuse)
    monkeypatch.setattr(md, "nearest", refuse)
    stats = mesh.export(r, str(tmp_path / "a.ply"), 9, 0.0, normals=False)
    assert set(stats) == {"verts", "faces", "resolution", "normals"}
    stats = mesh.export(r, str(tmp_path / "b.ply"), 9, 0.0, normals=False, simplify=2, simplify_error=None)
    assert set(stats) == {"verts", "faces", "resolution", "normals", "clusters", "degenerate", "duplicate", "orphans", "cluster_grid",
                          "extracted_verts", "extracted_faces"}
    with pytest.raises(AssertionError, match="without being asked"):
        mesh.export(r, str(tmp_path / "c.ply"), 9, 0.0, normals=False, simplify=2, simplify_error=100)
