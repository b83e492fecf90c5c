"""Mesh simplification on the GPU (csrc/ren_mesh_simplify.hip, mesh.simplify) against the numpy restatement
tests/mesh_simplify_reference.py: vertices, faces and the four counts with exact equality, every case.  The outputs are
functions of the input alone (integer sums, a stable order), so there is no tolerance anywhere in this file."""
import os

import numpy as np
import pytest
import torch

import mesh_simplify_reference as sref
from test_gpu_mesh import golden_renderer  # noqa: F401  (the tiny arch-ngp renderer, a module-scoped fixture)
from test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = sref.LO, sref.HI


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, mesh, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, mesh


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # a copy: the shared references are read-only


def check(mesh, verts, faces, grid, want=None, tag=""):
    """mesh.simplify on the device against the restatement (computed here unless handed in): bit for bit"""
    want_v, want_f, want_stats = sref.simplify(verts, faces, LO, HI, grid) if want is None else want
    got_v, got_f, stats = mesh.simplify(dev(verts), dev(faces), LO, HI, grid)
    print(tag, grid, tuple(got_v.shape), tuple(got_f.shape), stats, flush=True)
    assert got_v.dtype == torch.float32 and got_f.dtype == torch.int32 and got_v.is_cuda and got_f.is_cuda
    assert got_v.shape == (len(want_v), 3) and got_f.shape == (len(want_f), 3), (tag, stats, want_stats)
    assert stats == want_stats, tag
    assert torch.equal(got_f.cpu(), torch.from_numpy(np.array(want_f))), (tag, "faces")
    assert torch.equal(got_v.cpu().view(torch.int32), torch.from_numpy(np.array(want_v)).view(torch.int32)), (tag, "verts")
    return got_v, got_f, stats


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name,grid", [pytest.param(row[0], row[1], id=f"{row[0]}-{'x'.join(str(g) for g in row[1])}")
                                       for row in sref.TABLE])
def test_table_rows_equal_the_restatement(amd, name, grid):
    _, mesh = amd
    verts, faces = sref.mesh_of(name)
    row = next(r for r in sref.TABLE if r[0] == name and r[1] == grid)
    want = sref.table_result(name, grid)
    assert (len(want[0]), len(want[1])) == row[4:6]                                 # the restatement: the case is not vacuous
    check(mesh, verts, faces, grid, want, name)


def test_extracted_mesh_on_the_device_goes_through_unchanged_interfaces(amd):
    """mesh.extract's own output, never on the host, into mesh.simplify: the restatement's result for the restated mesh"""
    _, mesh = amd
    import mesh_reference as ref
    sigma, level = ref.field("two_spheres")
    verts, faces = mesh.extract(dev(sigma), level, LO, HI)
    got_v, got_f, stats = mesh.simplify(verts, faces, LO, HI, (8, 8, 8))
    want_v, want_f, want_stats = sref.table_result("two_spheres", (8, 8, 8))
    assert stats == want_stats and torch.equal(got_f.cpu(), torch.from_numpy(np.array(want_f)))
    assert torch.equal(got_v.cpu(), torch.from_numpy(np.array(want_v)))
    top = ref.topology(got_v.cpu().numpy(), got_f.cpu().numpy())
    assert top["closed"] and top["euler"] == 4


# ---------------------------------------------------------------------------------------------------- edge inputs
def test_corner_indices_out_of_range_are_degenerate(amd):
    _, mesh = amd
    verts, faces = sref.mesh_of("standard_normal")
    faces = faces.copy()
    n = len(verts)
    c, _ = sref.cells(verts, LO, HI, (6, 5, 4))
    fc = ((c[:, 0] * 5 + c[:, 1]) * 4 + c[:, 2])[faces]
    a, b, d, e, f = np.flatnonzero((fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2]))[[0, 1, 2, 50, -1]]
    faces[a, 1], faces[b, 0], faces[d, 2], faces[e, 0] = -1, n, np.iinfo(np.int32).max, np.iinfo(np.int32).min
    faces[f] = (n, -1, n + 7)
    _, _, stats = check(mesh, verts, faces, (6, 5, 4), tag="corners")
    assert stats["degenerate"] == 4408 + 5                                          # five faces that were kept before


def test_nan_and_infinite_coordinates_go_to_cell_zero_or_the_border(amd):
    _, mesh = amd
    verts, faces = sref.mesh_of("standard_normal")
    verts = verts.copy()
    verts[3] = (np.nan, np.nan, np.nan)
    verts[10, 0], verts[11, 1], verts[12, 2] = np.inf, -np.inf, np.nan
    verts[13] = (np.inf, np.inf, np.inf)
    verts[14] = (-np.inf, 1e30, -1e30)
    got_v, _, _ = check(mesh, verts, faces, (6, 5, 4), tag="special")
    assert bool(torch.isfinite(got_v).all())
    tiny = np.array([[np.nan, 1.0, 2.5], [np.inf, -np.inf, 2.5], [0.0, 1.0, 99.0], [-9.0, 1.0, 3.0]], dtype=np.float32)
    tri = np.array([[0, 1, 2], [0, 1, -1], [0, 1, 4], [2, 0, 1], [0, 2, 1]], dtype=np.int32)
    got_v, got_f, stats = check(mesh, tiny, tri, (4, 3, 2), tag="tiny")
    assert stats == dict(clusters=4, degenerate=2, duplicate=1, orphans=1) and got_f.cpu().tolist() == [[0, 2, 1], [0, 1, 2]]
    assert got_v[0, 0].item() == LO[0] and got_v[2, 0].item() == HI[0]              # NaN: the low corner of cell 0; +inf: the box's face


def test_empty_inputs_launch_nothing_they_do_not_need(amd, monkeypatch):
    ops, mesh = amd
    verts, faces = sref.mesh_of("sphere")

    def refuse(*a, **k):
        raise AssertionError("a kernel was launched for an empty stage")
    with monkeypatch.context() as m:
        for name in ("mesh_simplify_faces", "mesh_simplify_heads", "mesh_simplify_vertices", "mesh_simplify_compact_faces"):
            m.setattr(ops, name, refuse)
        _, _, stats = check(mesh, verts, faces[:0], (4, 4, 4), tag="F = 0")
        assert stats == dict(clusters=38, degenerate=0, duplicate=0, orphans=38)
        m.setattr(ops, "mesh_simplify_flags", refuse)
        _, _, stats = check(mesh, verts[:0], faces, (4, 4, 4), tag="V = 0")
        assert stats == dict(clusters=0, degenerate=796, duplicate=0, orphans=0)
        check(mesh, verts[:0], faces[:0], (4, 4, 4), tag="both")
    with monkeypatch.context() as m:                                                # everything dropped: no vertex is written
        for name in ("mesh_simplify_vertices", "mesh_simplify_compact_faces"):
            m.setattr(ops, name, refuse)
        check(mesh, *sref.mesh_of("plane"), (2, 2, 1), tag="all dropped")


@pytest.mark.parametrize("grid", [(1, 7, 5), (9, 1, 4), (6, 5, 1), (1, 1, 9)])
def test_a_grid_with_an_extent_of_one(amd, grid):
    _, mesh = amd
    check(mesh, *sref.mesh_of("standard_normal"), grid, tag="flat grid")


def test_more_occupied_cells_than_one_scan_block(amd):
    """70 000 vertices, one in every cell of (70, 50, 20): the prefix sums over cells and clusters take the multi-block path"""
    _, mesh = amd
    grid = (70, 50, 20)
    rng = np.random.default_rng(7)
    lo, hi, g = np.array(LO), np.array(HI), np.array(grid)
    idx = np.stack(np.meshgrid(*(np.arange(n) for n in grid), indexing="ij"), axis=-1).reshape(-1, 3)
    verts = (lo + (idx + 0.02 + 0.96 * rng.random(idx.shape)) * ((hi - lo) / g)).astype(np.float32)
    verts = verts[rng.permutation(len(verts))]                                      # cell order is not input order
    faces = rng.integers(0, len(verts), (1000, 3)).astype(np.int32)
    want = sref.simplify(verts, faces, LO, HI, grid)
    assert want[2]["clusters"] == 70000 > 65536 and want[2]["orphans"] > 65536 and len(want[1]) > 900
    check(mesh, verts, faces, grid, want, "70k")


# ---------------------------------------------------------------------------------------------------- repeatability
def test_two_calls_are_bit_identical(amd):
    _, mesh = amd
    for name, grid in (("soup", (1, 1, 1)), ("soup", (3, 3, 2)), ("two_spheres", (8, 8, 8))):
        verts, faces = (dev(a) for a in sref.mesh_of(name))
        before = verts.clone(), faces.clone()
        a, b = mesh.simplify(verts, faces, LO, HI, grid), mesh.simplify(verts, faces, LO, HI, grid)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] == b[2]
        assert torch.equal(verts, before[0]) and torch.equal(faces, before[1])      # the input is never written


# ---------------------------------------------------------------------------------------------------- validation
def test_wrong_dtype_layout_or_device_is_refused_before_any_launch(amd, monkeypatch):
    ops, mesh = amd
    verts, faces = (dev(a) for a in sref.mesh_of("sphere"))
    from robust_e_nerf_amd import _lib
    lib = _lib.load()

    class Refusing:
        def __getattr__(self, name):
            if name.startswith("ren_mesh_simplify"):
                raise AssertionError(f"{name} was called")
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "load", lambda: Refusing())
    bad = [(verts.double(), faces), (verts, faces.long()), (verts.cpu(), faces), (verts, faces.cpu()),
           (verts.t().contiguous().t(), faces), (verts, faces.t().contiguous().t()), (verts[:, :2].contiguous(), faces),
           (verts, faces[:, :2].contiguous()), (verts.reshape(-1), faces)]
    for v, f in bad:
        with pytest.raises(ValueError):
            mesh.simplify(v, f, LO, HI, (4, 4, 4))
    for grid in ((0, 4, 4), (4, 4), (1024, 1024, 1025)):
        with pytest.raises(ValueError, match="cluster grid"):
            mesh.simplify(verts, faces, LO, HI, grid)
    with pytest.raises(ValueError, match="finite lo < hi"):
        mesh.simplify(verts, faces, HI, LO, (4, 4, 4))


# ---------------------------------------------------------------------------------------------------- export
def test_export_with_simplify(amd, golden_renderer, tmp_path):
    ops, mesh = amd
    r, aabb = golden_renderer
    res = 24
    lo, hi = aabb[:3], aabb[3:]
    sigma = mesh.sample_density(r, lo, hi, res)
    level = float(sigma.median())
    verts, faces = mesh.extract(sigma, level, lo, hi)
    plain, small = str(tmp_path / "plain.ply"), str(tmp_path / "small.ply")
    stats0 = mesh.export(r, plain, res, level)
    stats = mesh.export(r, small, res, level, simplify=2)
    v, f, n = read_ply(small)
    print(stats0, stats, flush=True)
    assert (stats["verts"], stats["faces"]) == (len(v), len(f)) and stats["normals"] and n is not None
    assert (stats["extracted_verts"], stats["extracted_faces"]) == (verts.shape[0], faces.shape[0]) == (stats0["verts"], stats0["faces"])
    assert stats["cluster_grid"] == (12, 12, 12) == mesh.cluster_grid(res, 2)
    assert 0 < len(f) < stats0["faces"] and 0 < len(v) < stats0["verts"]
    assert stats["faces"] == stats["extracted_faces"] - stats["degenerate"] - stats["duplicate"]
    assert stats["verts"] == stats["clusters"] - stats["orphans"]
    assert f.min() >= 0 and f.max() == len(v) - 1
    want_v, want_f, want_stats = mesh.simplify(verts, faces, lo, hi, (12, 12, 12))
    assert np.array_equal(v, want_v.cpu().numpy()) and np.array_equal(f, want_f.cpu().numpy())
    assert {k: stats[k] for k in want_stats} == want_stats
    assert np.array_equal(n, mesh.vertex_normals(r, want_v).cpu().numpy())          # taken at the new positions
    length = np.linalg.norm(n.astype(np.float64), axis=-1)
    assert ((np.abs(length - 1) < 1e-5) | (length == 0)).all() and length.max() > 0
    assert os.path.getsize(small) < os.path.getsize(plain)


def test_export_without_simplify_writes_the_same_bytes(amd, golden_renderer, tmp_path, monkeypatch):
    ops, mesh = amd
    r, aabb = golden_renderer
    res = 24
    lo, hi = aabb[:3], aabb[3:]
    sigma = mesh.sample_density(r, lo, hi, res)
    level = float(sigma.median())
    verts, faces = mesh.extract(sigma, level, lo, hi)
    by_hand, default, none = (str(tmp_path / name) for name in ("by_hand.ply", "default.ply", "none.ply"))
    mesh.write_ply(by_hand, verts, faces, mesh.vertex_normals(r, verts))

    def refuse(*a, **k):
        raise AssertionError("mesh.export simplified without being asked to")
    with monkeypatch.context() as m:
        m.setattr(ops, "mesh_simplify_cells", refuse)
        stats = mesh.export(r, default, res, level)
        assert mesh.export(r, none, res, level, simplify=None) == stats
    assert stats == dict(verts=verts.shape[0], faces=faces.shape[0], resolution=(res,) * 3, normals=True)
    assert open(default, "rb").read() == open(by_hand, "rb").read() == open(none, "rb").read()
