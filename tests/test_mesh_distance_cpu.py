"""CPU: the shell-by-shell restatement of the grid nearest-neighbour search (tests/mesh_distance_reference.py) against the brute
force it must equal, before the GPU tests hold the kernel to the same brute force; mesh_distance.nn_grid, scores, read_ply,
sample_surface; the command lines; argument validation; the library's symbols."""
import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_distance_reference as dref
from conftest import REPO


@pytest.fixture(scope="module")
def md():
    from robust_e_nerf_amd import mesh_distance
    return mesh_distance


def same(got, want, tag):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(got[1], want[1]), (tag, "idx")
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), (tag, "d2")


# ---------------------------------------------------------------------------------------------------- the search logic
@pytest.mark.parametrize("nq,nr", dref.SIZES, ids=[f"{a}x{b}" for a, b in dref.SIZES])
@pytest.mark.parametrize("name", dref.INPUTS)
def test_grid_search_equals_brute_force(name, nq, nr):
    q, p = dref.make(name, nq, nr)
    assert q.shape == (nq, 3) and p.shape == (nr, 3) and q.dtype == p.dtype == np.float32
    same(dref.grid_search(q, p), dref.brute(q, p), name)


def test_the_adversarial_inputs_are_what_they_claim(md):
    q, p = dref.make("ties", 1000, 4097)
    d = q[:, None, :].astype(np.float64) - p[None, :, :]
    d2 = (d * d).sum(-1)
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.9     # the minimum is attained more than once
    for name, flat in (("plane", (2,)), ("line", (0, 2))):
        lo, h, grid = dref.auto_grid(dref.make(name, 63, 64)[1])
        assert all(grid[a] == 1 for a in flat) and max(grid) > 1
    q, p = dref.make("cell_faces", 1000, 4097)
    lo, h, grid = dref.auto_grid(p)
    k = p.astype(np.float64) / float(np.float32(h))
    assert max(grid) > 4 and (np.abs(k - np.round(k)) < 1e-6).mean() > 0.9          # on faces (but for the cap at the box)
    q, p = dref.make("cluster_far_queries", 1000, 4097)
    lo, hi = p.min(axis=0), p.max(axis=0)
    outside = ((q < lo) | (q > hi)).any(axis=1)
    assert outside.all() and (np.abs(q - p[0]).max(axis=1) > 90 * (hi - lo).max()).all()
    for sign in (-1, 1):
        for a in range(3):
            assert ((q[:, a] - p[0, a]) * sign > 50 * (hi - lo).max()).any()         # on every side


def test_full_grid_walk_and_one_cell_cluster_on_explicit_grids():
    q, p, lo, h, grid = dref.corner_case()
    assert dref.cells(p, lo, h, grid).tolist() == [0] and set(dref.cells(q, lo, h, grid).tolist()) == {16 ** 3 - 1}
    same(dref.grid_search(q, p, lo, h, grid), dref.brute(q, p), "corner")
    q, p, lo, h, grid = dref.one_cell_cluster()
    assert len(set(dref.cells(p, lo, h, grid).tolist())) == 1
    same(dref.grid_search(q, p, lo, h, grid), dref.brute(q, p), "cluster")


@pytest.mark.parametrize("h,grid", [(8.0, (1, 1, 1)), (0.7, (3, 5, 7)), (0.125, (16, 16, 16))])
def test_the_result_does_not_depend_on_the_grid(h, grid):
    q, p = dref.make("uniform", 63, 64)
    same(dref.grid_search(q, p, [-1.0, 2.0, 0.5], h, grid), dref.brute(q, p), grid)
    q, p = dref.make("ties", 63, 64)
    same(dref.grid_search(q, p, [-1.0, -1.0, -1.0], h, grid), dref.brute(q, p), grid)


def test_points_a_hair_from_a_cell_face():
    """references on a cell face and a hair beyond it, queries a hair before a face: the best candidate of the first shells is
    about one cell edge away, where the stopping rule decides"""
    lo, h, grid = [0.0, 0.0, 0.0], 1.0, (8, 1, 1)
    p = np.array([[1.5, 0, 0], [np.nextafter(np.float32(4.0), np.float32(5.0)), 0, 0], [4.0, 0, 0]], np.float32)
    q = np.array([[2.5, 0, 0], [np.nextafter(np.float32(3.0), np.float32(2.0)), 0, 0]], np.float32)
    same(dref.grid_search(q, p, lo, h, grid), dref.brute(q, p), "face")


# ---------------------------------------------------------------------------------------------------- nn_grid
def test_nn_grid(md):
    for lo, hi, n in (((0, 0, 0), (1, 1, 1), 1), ((0, 0, 0), (1, 1, 1), 10 ** 6), ((-3, 2, 1), (5, 2.5, 1.001), 12345),
                      ((0, 0, 0), (1e-30, 1e30, 1), 2 ** 31 - 1), ((0, 0, 0), (1000, 1, 1), 10 ** 9)):
        h, grid = md.nn_grid(lo, hi, n)
        assert h > 0 and math.isfinite(h) and len(grid) == 3 and all(isinstance(g, int) and 1 <= g <= 512 for g in grid)
        assert all(g == 512 or (g - 1) * h <= b - a < g * h for g, a, b in zip(grid, lo, hi))   # hi lies in the last cell
    h, grid = md.nn_grid((0, 0, 0), (1, 1, 1), 4 * 10 ** 6)
    assert grid in ((100, 100, 100), (101, 101, 101)) and abs(h - 0.01) < 1e-9       # a million cells for four million references
    assert md.nn_grid((0, 0, 0), (1, 1, 1), 4 * 10 ** 6, per_cell=32.0)[1] in ((50, 50, 50), (51, 51, 51))
    assert md.nn_grid((0, 0, 0), (2, 3, 0), 1000)[1][2] == 1                         # planar
    assert md.nn_grid((0, 5, 0), (0, 9, 0), 1000)[1] in ((1, 250, 1), (1, 251, 1))   # collinear: four to a cell of the length
    assert md.nn_grid((1, 2, 3), (1, 2, 3), 1000) == (1.0, (1, 1, 1))                # one point
    h, grid = md.nn_grid((0, 0, 0), (1000, 1, 1), 10 ** 9)                           # h grown until the long axis fits
    assert grid[0] == 512 and h >= 1000 / 512
    for lo, hi in (((0, 0, 0), (1, 1, 1)), ((0, 0, 0), (4, 1, 0)), ((-1, -1, -1), (1, 30, 2))):
        cells = [math.prod(md.nn_grid(lo, hi, n)[1]) for n in (1, 2, 3, 10, 100, 10 ** 3, 10 ** 4, 10 ** 6, 10 ** 8, 10 ** 10)]
        edges = [md.nn_grid(lo, hi, n)[0] for n in (1, 2, 3, 10, 100, 10 ** 3, 10 ** 4, 10 ** 6, 10 ** 8, 10 ** 10)]
        assert cells == sorted(cells) and edges == sorted(edges, reverse=True) and cells[-1] > cells[0]
    for bad in (((0, 0, 0), (1, 1, -1), 5), ((0, 0), (1, 1), 5), ((0, 0, 0), (1, 1, float("inf")), 5), ((0, 0, 0), (1, 1, 1), 0),
                ((float("nan"), 0, 0), (1, 1, 1), 5)):
        with pytest.raises(ValueError):
            md.nn_grid(*bad)
    with pytest.raises(ValueError):
        md.nn_grid((0, 0, 0), (1, 1, 1), 5, per_cell=0.0)


# ---------------------------------------------------------------------------------------------------- scores
def test_scores_against_hand_computed_values(md):
    d_ab, d_ba = [0.0, 1.0, 2.0, 5.0], [3.0, 4.0]
    s = md.scores(torch.tensor(d_ab), np.array(d_ba), thresholds=(1.0, 3.5, 10.0, 0.0))
    assert s["accuracy"] == dict(mean=2.0, rms=math.sqrt(7.5), max=5.0)
    assert s["completeness"] == dict(mean=3.5, rms=math.sqrt(12.5), max=4.0)
    assert s["chamfer"] == 2.75 and s["hausdorff"] == 5.0
    want = [(1.0, 0.5, 0.0, 0.0), (3.5, 0.75, 0.5, 0.6), (10.0, 1.0, 1.0, 1.0), (0.0, 0.25, 0.0, 0.0)]
    assert [t["threshold"] for t in s["thresholds"]] == [w[0] for w in want]
    for t, (_, p, r, f) in zip(s["thresholds"], want):
        assert t["precision"] == p and t["recall"] == r and t["fscore"] == pytest.approx(f, rel=1e-12)
    none = md.scores([1.0, 2.0], [3.0], thresholds=(0.5,))["thresholds"][0]          # P + R = 0: no division
    assert none == dict(threshold=0.5, precision=0.0, recall=0.0, fscore=0.0)
    assert md.scores([1.0], [2.0])["thresholds"] == []
    rng = np.random.default_rng(3)                                                  # float64 sums: n 2^-53 bounds the error
    a, b = rng.random(100001), rng.random(77777) * 3
    s = md.scores(a, b.astype(np.float32), (0.5,))
    b = b.astype(np.float32).astype(np.float64)
    assert s["accuracy"]["mean"] == pytest.approx(math.fsum(a) / len(a), rel=1e-9)
    assert s["completeness"]["mean"] == pytest.approx(math.fsum(b) / len(b), rel=1e-9)
    assert s["accuracy"]["rms"] == pytest.approx(math.sqrt(math.fsum(a * a) / len(a)), rel=1e-9)
    assert s["chamfer"] == pytest.approx(0.5 * (math.fsum(a) / len(a) + math.fsum(b) / len(b)), rel=1e-9)
    assert s["hausdorff"] == max(a.max(), b.max())
    assert s["thresholds"][0]["precision"] == (a <= 0.5).mean() and s["thresholds"][0]["recall"] == (b <= 0.5).mean()
    for bad in (([], [1.0]), ([1.0], [])):
        with pytest.raises(ValueError):
            md.scores(*bad)


# ---------------------------------------------------------------------------------------------------- read_ply
QUAD_PLY = """ply
format ascii 1.0
comment a quad, a triangle and a pentagon over double vertices with a colour, and an element to skip
element vertex 6
property double x
property uchar red
property double y
property double z
element marker 2
property int id
property float weight
element face 3
property list uchar int vertex_indices
property uchar flag
end_header
0 255 0 0
1 255 0 0
1 0 1 0.5
0 0 1 0.5
2 7 2 2
0.1234567890123 1 2 3
7 0.5
8 0.25
4 0 1 2 3 1
3 3 2 4 0
5 0 1 2 4 5 1
"""


def test_read_ply_round_trips_write_ply(md, tmp_path):
    from robust_e_nerf_amd import mesh
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((50, 3)).astype(np.float32)
    faces = rng.integers(0, 50, (80, 3)).astype(np.int32)
    normals = rng.standard_normal((50, 3)).astype(np.float32)
    for name, nrm in (("plain.ply", None), ("normals.ply", normals)):
        path = str(tmp_path / name)
        mesh.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), None if nrm is None else torch.from_numpy(nrm))
        v, f = md.read_ply(path)
        assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(v, verts) and np.array_equal(f, faces)
    path = str(tmp_path / "empty.ply")
    mesh.write_ply(path, verts, faces[:0])
    v, f = md.read_ply(path)
    assert np.array_equal(v, verts) and f.shape == (0, 3)


def test_read_ply_ascii_polygons_doubles_and_skipped_properties(md, tmp_path):
    path = str(tmp_path / "quad.ply")
    open(path, "w").write(QUAD_PLY)
    v, f = md.read_ply(path)
    assert v.dtype == np.float32 and v.shape == (6, 3) and v[2].tolist() == [1.0, 1.0, 0.5]
    assert v[5].tolist() == [float(np.float32(0.1234567890123)), 2.0, 3.0]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 4], [0, 1, 2], [0, 2, 4], [0, 4, 5]]


def test_read_ply_binary_with_mixed_polygons_and_index_types(md, tmp_path):
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty double z\n"
              "property short tag\nelement face 3\nproperty uchar flag\nproperty list ushort uint vertex_index\nend_header\n")
    vt = np.zeros(5, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f8"), ("tag", "<i2")])
    vt["x"], vt["y"], vt["z"] = np.arange(5), 2 * np.arange(5), 0.5 * np.arange(5)
    body = vt.tobytes()
    for poly in ([0, 1, 2], [1, 2, 3, 4], [4, 0, 2]):
        body += np.uint8(9).tobytes() + np.uint16(len(poly)).tobytes() + np.array(poly, "<u4").tobytes()
    path = str(tmp_path / "mixed.ply")
    open(path, "wb").write(header.encode() + body)
    v, f = md.read_ply(path)
    assert v.tolist() == [[k, 2 * k, 0.5 * k] for k in range(5)]
    assert f.tolist() == [[0, 1, 2], [1, 2, 3], [1, 3, 4], [4, 0, 2]]
    open(path, "wb").write(header.encode() + body[:-3])
    with pytest.raises(ValueError, match="ends inside"):
        md.read_ply(path)


def test_read_ply_refuses_what_it_does_not_read(md, tmp_path):
    path = str(tmp_path / "bad.ply")
    ok = QUAD_PLY
    cases = {"big-endian": ok.replace("format ascii 1.0", "format binary_big_endian 1.0"),
             "no y": ok.replace("property double y\n", "property double why\n"),
             "integer x": ok.replace("property double x", "property int x"),
             "list on a vertex": ok.replace("property uchar red", "property list uchar int red"),
             "list on another element": ok.replace("property int id", "property list uchar int id"),
             "corner out of range": ok.replace("3 3 2 4 0", "3 3 2 6 0"),
             "not a ply": ok.replace("ply\n", "plz\n", 1),
             "no end": ok.replace("end_header\n", ""),
             "truncated": ok[: ok.index("4 0 1 2 3 1")]}
    for tag, text in cases.items():
        open(path, "w").write(text)
        with pytest.raises(ValueError):
            md.read_ply(path)
        print(tag, "refused")


# ---------------------------------------------------------------------------------------------------- sample_surface
def barycentric(p, a, b, c):
    """coordinates of p's projection onto the plane of (a, b, c) and its distance from that plane, float64"""
    n = np.cross(b - a, c - a)
    area2 = np.linalg.norm(n)
    n = n / area2
    off = (p - a) @ n
    foot = p - off[:, None] * n
    w = np.stack([np.cross(b - foot, c - foot) @ n, np.cross(c - foot, a - foot) @ n, np.cross(a - foot, b - foot) @ n], axis=-1) / area2
    return w, np.abs(off)


def test_sample_surface_on_the_cpu_device(md):
    verts = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 3], [5, 5, 5], [5, 5, 5], [7, 7, 7]], dtype=torch.float32)
    faces = torch.tensor([[4, 5, 6], [0, 1, 2], [4, 4, 4], [0, 1, 3], [1, 2, 3], [4, 5, 6]], dtype=torch.int32)   # three of zero area
    pts = md.sample_surface(verts, faces, 20000, seed=7)
    assert pts.shape == (20000, 3) and pts.dtype == torch.float32 and pts.is_contiguous()
    assert torch.equal(pts, md.sample_surface(verts, faces, 20000, seed=7))
    assert not torch.equal(pts, md.sample_surface(verts, faces, 20000, seed=8))
    assert torch.equal(pts, md.sample_surface(verts, faces.long(), 20000, seed=7))
    p, v = pts.double().numpy(), verts.double().numpy()
    scale, owner = 7.0, np.full(len(p), -1)
    for k, face in enumerate(faces.tolist()):
        if k in (0, 2, 5):
            continue
        w, off = barycentric(p, *v[face])
        owner[(off <= 1e-6 * scale) & (w >= -1e-6).all(axis=1) & (owner < 0)] = k
    assert (owner >= 0).all()                                                       # in the plane and inside some real face
    assert np.abs(p - 5).max(axis=1).min() > 1                                      # nothing near the degenerate faces' points
    areas = {1: 2.0, 3: 3.0, 4: 0.5 * np.linalg.norm(np.cross(v[2] - v[1], v[3] - v[1]))}
    total = sum(areas.values())
    for k, area in areas.items():                                                   # by area: 6 sigma of the binomial count
        share = area / total
        assert abs((owner == k).mean() - share) < 6 * math.sqrt(share * (1 - share) / len(p))
    one = md.sample_surface(verts, torch.tensor([[4, 5, 6], [0, 1, 2]]), 500, seed=0).double().numpy()   # one real, one degenerate
    w, off = barycentric(one, *v[[0, 1, 2]])
    assert (off <= 1e-6 * scale).all() and (w >= -1e-6).all()
    assert md.sample_surface(verts, faces, 0, seed=0).shape == (0, 3)
    for bad_faces in (faces[[0, 2, 5]], faces[:0], torch.tensor([[0, 1, 7]]), torch.tensor([[0, -1, 2]])):
        with pytest.raises(ValueError):
            md.sample_surface(verts, bad_faces, 10, seed=0)
    with pytest.raises(ValueError):
        md.sample_surface(verts, faces.float(), 10, seed=0)


# ---------------------------------------------------------------------------------------------------- validation
def test_ops_and_nearest_refuse_bad_arguments_without_a_device(md):
    from robust_e_nerf_amd import ops
    pts, lo = torch.zeros(4, 3), (0.0, 0.0, 0.0)
    rec, start = torch.zeros(4, 4), torch.zeros(9, dtype=torch.int32)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.nn_cells(pts, lo, 0.5, (2, 2, 2))
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.nn_search(pts, rec, start, lo, 0.5, (2, 2, 2))
    for bad in (pts.double(), pts[:, :2], pts.reshape(-1)):
        with pytest.raises(ValueError):
            ops.nn_cells(bad, lo, 0.5, (2, 2, 2))
        with pytest.raises(ValueError):
            ops.nn_search(bad, rec, start, lo, 0.5, (2, 2, 2))
        with pytest.raises(ValueError):
            md.nearest(bad, pts)
        with pytest.raises(ValueError):
            md.nearest(pts, bad)
    with pytest.raises(ValueError, match="ref_records"):
        ops.nn_search(pts, pts, start, lo, 0.5, (2, 2, 2))
    with pytest.raises(ValueError, match="cell_start"):
        ops.nn_search(pts, rec, start[:8], lo, 0.5, (2, 2, 2))
    with pytest.raises(ValueError):
        ops.nn_search(pts, rec, start.long(), lo, 0.5, (2, 2, 2))
    for grid in ((0, 2, 2), (2, 2), (2, 2.5, 2), (513, 1, 1)):
        with pytest.raises(ValueError, match="grid"):
            ops.nn_cells(pts, lo, 0.5, grid)
    for h in (0.0, -1.0, float("nan"), float("inf"), 1e-40, 1e39):
        with pytest.raises(ValueError, match="cell edge"):
            ops.nn_cells(pts, lo, h, (2, 2, 2))
    for bad_lo in ((0.0, 0.0), (float("nan"), 0, 0), (0, float("inf"), 0), (1e39, 0, 0)):
        with pytest.raises(ValueError, match="lo"):
            ops.nn_cells(pts, bad_lo, 0.5, (2, 2, 2))
    with pytest.raises(ValueError, match="device tensor"):
        md.nearest(pts, pts)
    with pytest.raises(ValueError, match="device tensor"):
        md.nearest_on_grid(pts, pts, lo, 0.5, (2, 2, 2))


def test_library_exports_the_new_symbols_and_refuses_bad_arguments_before_any_launch():
    from robust_e_nerf_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    for name in ("ren_nn_cells", "ren_nn_search"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert hdr.index("---- mesh distance") > hdr.index("---- mesh simplify")
    assert "ren_mesh_distance.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE["ren_mesh_distance.hip"]
    assert lib.ren_abi_version() == 25
    one, odd, odd16 = ctypes.c_void_p(256), ctypes.c_void_p(258), ctypes.c_void_p(264)   # nothing is dereferenced
    bad, f3, f = _lib.REN_ERR_BAD_ARG, ctypes.c_float * 3, ctypes.c_float
    lo = f3(0, 0, 0)
    cells, search = lib.ren_nn_cells, lib.ren_nn_search
    assert cells(one, 0, lo, f(2.0), 2, 2, 2, one, None) == _lib.REN_OK              # no point: nothing is launched
    assert cells(None, 0, lo, f(2.0), 2, 2, 2, None, None) == _lib.REN_OK
    for g in ((0, 2, 2), (2, -1, 2), (2, 2, 0), (513, 2, 2), (2, 2, 2 ** 20)):
        assert cells(one, 8, lo, f(2.0), *g, one, None) == bad
        assert search(one, 8, one, one, 8, lo, f(0.5), f(2.0), *g, one, one, None) == bad
    for n in (-1, 2 ** 31):
        assert cells(one, n, lo, f(2.0), 2, 2, 2, one, None) == bad
        assert search(one, n, one, one, 8, lo, f(0.5), f(2.0), 2, 2, 2, one, one, None) == bad
        assert search(one, 8, one, one, n, lo, f(0.5), f(2.0), 2, 2, 2, one, one, None) == bad
    for inv in (0.0, -2.0, float("nan"), float("inf")):
        assert cells(one, 8, lo, f(inv), 2, 2, 2, one, None) == bad
    for blo in (None, f3(float("nan"), 0, 0), f3(0, float("inf"), 0)):
        assert cells(one, 8, blo, f(2.0), 2, 2, 2, one, None) == bad
        assert search(one, 8, one, one, 8, blo, f(0.5), f(2.0), 2, 2, 2, one, one, None) == bad
    for ptrs in ((None, one), (one, None), (odd, one), (one, odd)):
        assert cells(ptrs[0], 8, lo, f(2.0), 2, 2, 2, ptrs[1], None) == bad
    assert search(one, 0, one, one, 8, lo, f(0.5), f(2.0), 2, 2, 2, one, one, None) == _lib.REN_OK   # no query: no launch
    assert search(None, 0, None, one, 0, lo, f(0.5), f(2.0), 2, 2, 2, None, None, None) == _lib.REN_OK
    for h, inv in ((0.0, 2.0), (-0.5, -2.0), (0.5, 0.0), (float("nan"), 2.0), (float("inf"), 0.0), (0.5, 2.001), (0.5, 1.0), (1e-39, 1e38)):
        assert search(one, 8, one, one, 8, lo, f(h), f(inv), 2, 2, 2, one, one, None) == bad      # also h and 1 / h that disagree
    for null in range(5):
        ptrs = [one] * 5
        ptrs[null] = None
        assert search(ptrs[0], 8, ptrs[1], ptrs[2], 8, lo, f(0.5), f(2.0), 2, 2, 2, ptrs[3], ptrs[4], None) == bad
        ptrs[null] = odd16 if null == 1 else odd                                    # the records want 16 bytes
        assert search(ptrs[0], 8, ptrs[1], ptrs[2], 8, lo, f(0.5), f(2.0), 2, 2, 2, ptrs[3], ptrs[4], None) == bad


# ---------------------------------------------------------------------------------------------------- command lines
def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_lines():
    cli = load_script("export_mesh")
    base = ["--config", "c.yaml", "--out", "m.ply"]
    assert cli.parse_args(base).simplify_error is None
    assert cli.parse_args(base + ["--simplify", "2"]).simplify_error is None
    assert cli.parse_args(base + ["--simplify", "2", "--simplify-error"]).simplify_error == 1_000_000
    assert cli.parse_args(base + ["--simplify", "2", "--simplify-error", "5000"]).simplify_error == 5000
    for bad in (["--simplify-error"], ["--simplify", "2", "--simplify-error", "0"], ["--simplify", "2", "--simplify-error", "x"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    ev = load_script("eval_mesh")
    args = ev.parse_args(["--mesh", "a.ply", "--gt", "b.ply"])
    assert (args.samples, args.seed, args.threshold, args.out) == (1_000_000, 0, [], None)
    args = ev.parse_args(["--mesh", "a.ply", "--gt", "b.ply", "--samples", "1000", "--seed", "3", "--threshold", "0.01", "0.05",
                          "--out", "s.json"])
    assert (args.samples, args.seed, args.threshold, args.out) == (1000, 3, [0.01, 0.05], "s.json")
    for bad in ([], ["--mesh", "a.ply"], ["--mesh", "a.ply", "--gt", "b.ply", "--samples", "0"],
                ["--mesh", "a.ply", "--gt", "b.ply", "--threshold", "-1"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    json.dumps(vars(args))


def test_export_refuses_simplify_error_without_simplify():
    from robust_e_nerf_amd import mesh
    for kw in (dict(simplify_error=100), dict(simplify=2, simplify_error=0), dict(simplify=2, simplify_error=2.5)):
        with pytest.raises(ValueError, match="simplify_error"):
            mesh.export(None, "m.ply", 8, 1.0, **kw)
