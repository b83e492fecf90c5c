"""CPU: the numpy restatement of the vertex-clustering simplification (tests/mesh_simplify_reference.py) against properties
that do not come from it, and the figures of the specification's table, before the GPU tests hold the kernels to it;
mesh.cluster_grid; the command line; argument validation; the library's symbols."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_reference as ref
import mesh_simplify_reference as sref
from conftest import REPO

LO, HI = sref.LO, sref.HI
ROWS = [pytest.param(*row, id=f"{row[0]}-{'x'.join(str(g) for g in row[1])}") for row in sref.TABLE]


def rotated(face):
    face = [int(v) for v in face]
    m = face.index(min(face))
    return tuple(face[m:] + face[:m])


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name,grid,V,F,V2,F2,degenerate,duplicate,orphans", ROWS)
def test_table_rows_hold_for_the_restatement(name, grid, V, F, V2, F2, degenerate, duplicate, orphans):
    verts, faces = sref.mesh_of(name)
    out_v, out_f, stats = sref.table_result(name, grid)
    assert (len(verts), len(faces)) == (V, F)
    assert (len(out_v), len(out_f)) == (V2, F2)
    assert (stats["degenerate"], stats["duplicate"], stats["orphans"]) == (degenerate, duplicate, orphans)
    assert stats["clusters"] == V2 + orphans and F == F2 + degenerate + duplicate
    assert out_v.dtype == np.float32 and out_f.dtype == np.int32 and out_v.shape == (V2, 3) and out_f.shape == (F2, 3)


@pytest.mark.parametrize("name,grid,V,F,V2,F2,degenerate,duplicate,orphans", ROWS)
def test_properties_that_do_not_come_from_the_restatement(name, grid, V, F, V2, F2, degenerate, duplicate, orphans):
    verts, faces = sref.mesh_of(name)
    out_v, out_f, _ = sref.table_result(name, grid)
    # every face: three distinct ids below V'; every vertex referenced; no two faces equal up to rotation
    assert ((out_f >= 0) & (out_f < V2)).all()
    assert ((out_f[:, 0] != out_f[:, 1]) & (out_f[:, 1] != out_f[:, 2]) & (out_f[:, 0] != out_f[:, 2])).all()
    assert np.array_equal(np.unique(out_f), np.arange(V2))
    assert len({rotated(f) for f in out_f}) == F2
    # the cells that survive, from the cell of every input vertex alone (the specification's definition; a vertex ON a cell
    # boundary -- the lattice's own lines at k = 1 -- cannot be placed from its rounded position): those of the faces whose
    # three corners lie in three cells, in ascending cell id
    lo, hi, g = np.array(LO), np.array(HI), np.array(grid)
    cw = (hi - lo) / g
    c, _ = sref.cells(verts, LO, HI, grid)
    in_cell = (c[:, 0] * g[1] + c[:, 1]) * g[2] + c[:, 2]
    fc = in_cell[faces]
    apart = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    ids = np.unique(fc[apart])
    assert len(ids) == V2
    # every output vertex lies in the closed cell of its cluster
    where = np.stack([ids // (g[1] * g[2]), (ids // g[2]) % g[1], ids % g[2]], axis=-1)
    cell_lo, cell_hi = (lo + where * cw).astype(np.float32), (lo + (where + 1) * cw).astype(np.float32)
    assert ((out_v >= cell_lo) & (out_v <= cell_hi)).all()
    # the kept faces are a subsequence of the input, mapped corner by corner through the cell of each input vertex
    to_out = {int(c): i for i, c in enumerate(ids)}
    it = iter(range(len(faces)))
    for face in out_f:
        for f in it:                                                  # advances: the order of the input is kept
            mapped = [to_out.get(int(in_cell[c]), -1) for c in faces[f]]
            if mapped == [int(v) for v in face]:
                break
        else:
            raise AssertionError(f"{face} is not the image of a later input face")


def test_sphere_fields_stay_closed():
    for name, grid, euler in (("two_spheres", (8, 8, 8), 4), ("two_spheres", (16, 16, 16), 4), ("sphere", (4, 4, 4), 2)):
        out_v, out_f, _ = sref.table_result(name, grid)
        top = ref.topology(out_v, out_f)
        assert top["closed"] and top["euler"] == euler, (name, grid, top["euler"])


def test_cells_hold_many_vertices_in_the_contention_rows():
    c, _ = sref.cells(sref.mesh_of("two_spheres")[0], LO, HI, (8, 8, 8))
    assert np.bincount((c[:, 0] * 8 + c[:, 1]) * 8 + c[:, 2]).max() == 27
    c, _ = sref.cells(sref.mesh_of("soup")[0], LO, HI, (1, 1, 1))
    assert not c.any() and len(c) == 5000
    soup = sref.mesh_of("soup")[0]
    assert (soup < np.array(LO, dtype=np.float32)).any() and (soup > np.array(HI, dtype=np.float32)).any()   # the clamp is exercised


# ---------------------------------------------------------------------------------------------------- one vertex per cell
def test_one_vertex_per_cell_returns_the_faces_and_moves_nothing_beyond_the_quantisation():
    """each coordinate moves by at most cw * 2^-21 (half a quantisation step) plus one float32 ulp of max(|lo|, |hi|) (the
    final rounding): nothing measured"""
    grid = (7, 5, 3)
    rng = np.random.default_rng(3)
    lo, hi, g = np.array(LO), np.array(HI), np.array(grid)
    cw = (hi - lo) / g
    idx = np.stack(np.meshgrid(*(np.arange(n) for n in grid), indexing="ij"), axis=-1).reshape(-1, 3)
    verts = (lo + (idx + 0.02 + 0.96 * rng.random(idx.shape)) * cw).astype(np.float32)
    n = len(verts)
    step = np.arange(n)
    faces = np.stack([step, (step + 1) % n, (step + 17) % n], axis=-1).astype(np.int32)          # every vertex is referenced
    faces = np.concatenate([faces, faces[:, [0, 2, 1]]])                            # and the mirror images: other keys, both stay
    out_v, out_f, stats = sref.simplify(verts, faces, LO, HI, grid)
    assert stats == dict(clusters=n, degenerate=0, duplicate=0, orphans=0)
    assert np.array_equal(out_f, faces)
    bound = cw * 2.0 ** -21 + np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    assert (np.abs(out_v.astype(np.float64) - verts.astype(np.float64)) <= bound).all()


def test_special_coordinates_and_corner_indices_in_the_restatement():
    verts = np.array([[np.nan, 1.0, 2.5], [np.inf, -np.inf, 2.5], [0.0, 1.0, 99.0], [-9.0, 1.0, 3.0]], dtype=np.float32)
    c, q = sref.cells(verts, LO, HI, (4, 3, 2))
    assert c.tolist() == [[0, 1, 0], [3, 0, 0], [1, 1, 1], [0, 1, 1]]
    assert q[0, 0] == 0 and q[1, 0] == 2 ** 20 and q[1, 1] == 0 and q[2, 2] == 2 ** 20 and q[3, 0] == 0
    faces = np.array([[0, 1, 2], [0, 1, -1], [0, 1, 4], [2, 0, 1], [0, 2, 1]], dtype=np.int32)
    out_v, out_f, stats = sref.simplify(verts, faces, LO, HI, (4, 3, 2))
    assert stats == dict(clusters=4, degenerate=2, duplicate=1, orphans=1)
    assert out_f.tolist() == [[0, 2, 1], [0, 1, 2]] and np.isfinite(out_v).all()
    for empty_v, empty_f in ((verts[:0], faces), (verts, faces[:0]), (verts[:0], faces[:0])):
        out_v, out_f, stats = sref.simplify(empty_v, empty_f, LO, HI, (4, 3, 2))
        assert out_v.shape == (0, 3) and out_f.shape == (0, 3) and stats["degenerate"] == len(empty_f)
        assert stats["clusters"] == stats["orphans"] == (4 if len(empty_v) else 0)


# ---------------------------------------------------------------------------------------------------- the package, no GPU
def test_cluster_grid_values_and_refusals():
    from robust_e_nerf_amd import mesh
    assert mesh.cluster_grid(256, 2) == (128, 128, 128)
    assert mesh.cluster_grid(257, 2) == (128, 128, 128)
    assert mesh.cluster_grid((17, 9, 5), 4) == (4, 2, 1)
    assert mesh.cluster_grid((17, 9, 2), 1) == (16, 8, 1)
    assert mesh.cluster_grid((17, 9, 5), 2.5) == (7, 4, 2)
    assert mesh.cluster_grid(5, 1000) == (1, 1, 1)
    for bad in (0, 0.99, -2, float("nan"), float("inf"), "two", None):
        with pytest.raises(ValueError, match="cluster_grid"):
            mesh.cluster_grid(17, bad)
    with pytest.raises(ValueError, match="resolution"):
        mesh.cluster_grid(1, 2)
    with pytest.raises(ValueError, match="cluster_grid"):                           # before the renderer is touched
        mesh.export(None, "x.ply", 8, 0.0, (0, 0, 0), (1, 1, 1), simplify=0.5)


def test_export_mesh_parses_simplify():
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(REPO, "scripts", "export_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--config", "c.yaml", "--ckpt", "x.ckpt", "--out", "m.ply"]
    assert cli.parse_args(base).simplify is None
    assert cli.parse_args(base + ["--simplify", "2"]).simplify == 2.0
    assert cli.parse_args(base + ["--simplify", "2.5", "--largest", "1"]).simplify == 2.5
    for bad in (["--simplify", "0.5"], ["--simplify", "nan"], ["--simplify", "x"], ["--simplify"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)


def test_ops_refuse_cpu_tensors_and_bad_grids():
    from robust_e_nerf_amd import mesh, ops
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    i32, i64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_cells(verts, LO, HI, (2, 2, 1))
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_flags(i32)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_faces(faces, 4, i32, i64, 2)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_heads(i64[:2], i32[:2], i64[:2], faces, 2)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_vertices(torch.zeros(4, 3, dtype=torch.int64), i32, i64, i32[:2], i64[:2], LO, HI, (2, 2, 1), 2)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_simplify_compact_faces(faces, i32[:2], i64[:2], i64[:2], 1)
    with pytest.raises(ValueError, match="device tensor"):
        mesh.simplify(verts, faces, LO, HI, (2, 2, 1))
    for grid in ((0, 2, 2), (2, 2), (2, 2.5, 2), (1024, 1024, 1025)):
        with pytest.raises(ValueError, match="cluster grid"):
            ops.mesh_simplify_cells(verts, LO, HI, grid)
    for lo, hi in ((LO, LO), (HI, LO), ((float("nan"), 0, 0), HI), (LO, (float("inf"), 2, 4))):
        with pytest.raises(ValueError, match="finite lo < hi"):
            ops.mesh_simplify_cells(verts, lo, hi, (2, 2, 2))


def test_library_exports_the_new_symbols_and_refuses_bad_arguments_before_any_launch():
    from robust_e_nerf_amd import _lib, build
    build.build()
    lib = _lib.load()
    names = ("ren_mesh_simplify_cells", "ren_mesh_simplify_flags", "ren_mesh_simplify_faces", "ren_mesh_simplify_heads",
             "ren_mesh_simplify_vertices", "ren_mesh_simplify_compact_faces")
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert hdr.index("---- mesh simplify") > hdr.index("---- mesh components")
    assert "ren_mesh_simplify.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE["ren_mesh_simplify.hip"]
    assert lib.ren_abi_version() == 25
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)        # aligned / misaligned non-null addresses: nothing is dereferenced
    bad, d3 = _lib.REN_ERR_BAD_ARG, ctypes.c_double * 3
    lo, hi = d3(*LO), d3(*HI)
    cells = lib.ren_mesh_simplify_cells
    assert cells(one, 0, lo, hi, 2, 2, 2, one, one, one, None) == _lib.REN_OK       # no vertex: nothing is launched
    for g in ((0, 2, 2), (2, -1, 2), (2, 2, 0), (1024, 1024, 1025), (2 ** 20, 2 ** 20, 1)):
        assert cells(one, 8, lo, hi, *g, one, one, one, None) == bad
    for V in (-1, 2 ** 31):
        assert cells(one, V, lo, hi, 2, 2, 2, one, one, one, None) == bad
    for blo, bhi in ((lo, lo), (hi, lo), (d3(float("nan"), 0, 0), hi), (lo, d3(float("inf"), 2, 4)), (None, hi), (lo, None)):
        assert cells(one, 8, blo, bhi, 2, 2, 2, one, one, one, None) == bad
    for null in range(4):
        ptrs = [one] * 4
        ptrs[null] = None
        assert cells(ptrs[0], 8, lo, hi, 2, 2, 2, ptrs[1], ptrs[2], ptrs[3], None) == bad
        ptrs[null] = odd
        assert cells(ptrs[0], 8, lo, hi, 2, 2, 2, ptrs[1], ptrs[2], ptrs[3], None) == bad
    flags = lib.ren_mesh_simplify_flags
    for args in ((None, 8, one), (one, 8, None), (one, 0, one), (one, 2 ** 30 + 1, one), (odd, 8, one)):
        assert flags(*args, None) == bad
    faces = lib.ren_mesh_simplify_faces
    assert faces(one, 0, 8, one, one, 8, 4, one, one, one, one, None) == _lib.REN_OK
    for F, V, n_cells, clusters in ((-1, 8, 8, 4), (2 ** 31, 8, 8, 4), (4, -1, 8, 4), (4, 8, 0, 0), (4, 8, 8, 9), (4, 8, 8, -1)):
        assert faces(one, F, V, one, one, n_cells, clusters, one, one, one, one, None) == bad
    for null in range(7):
        ptrs = [one] * 7
        ptrs[null] = None
        assert faces(ptrs[0], 4, 8, ptrs[1], ptrs[2], 8, 4, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None) == bad
    heads = lib.ren_mesh_simplify_heads
    assert heads(one, one, one, one, 0, 4, one, one, None) == _lib.REN_OK
    assert heads(one, one, one, one, -1, 4, one, one, None) == bad
    assert heads(one, one, one, one, 4, 2 ** 30 + 1, one, one, None) == bad
    for null in range(6):
        ptrs = [one] * 6
        ptrs[null] = None
        assert heads(*ptrs[:4], 4, 4, ptrs[4], ptrs[5], None) == bad
    vertices = lib.ren_mesh_simplify_vertices
    assert vertices(one, one, one, one, one, 2, 2, 2, lo, hi, 4, 0, one, None) == _lib.REN_OK
    assert vertices(one, one, one, one, one, 2, 2, 2, lo, hi, 4, 5, one, None) == bad             # more rows than clusters
    assert vertices(one, one, one, one, one, 2, 2, 2, lo, hi, 9, 4, one, None) == bad             # more clusters than cells
    assert vertices(one, one, one, one, one, 2, 0, 2, lo, hi, 4, 4, one, None) == bad
    assert vertices(one, one, one, one, one, 2, 2, 2, hi, lo, 4, 4, one, None) == bad
    for null in range(6):
        ptrs = [one] * 6
        ptrs[null] = None
        assert vertices(*ptrs[:5], 2, 2, 2, lo, hi, 4, 4, ptrs[5], None) == bad
    compact = lib.ren_mesh_simplify_compact_faces
    assert compact(one, one, one, one, 4, 4, 0, one, None) == _lib.REN_OK
    assert compact(one, one, one, one, 4, 4, 5, one, None) == bad                                 # more rows than faces
    assert compact(one, one, one, one, -1, 4, 0, one, None) == bad
    for null in range(5):
        ptrs = [one] * 5
        ptrs[null] = None
        assert compact(*ptrs[:4], 4, 4, 2, ptrs[4], None) == bad
