"""CPU: the numpy restatement of the mesh extraction (tests/mesh_reference.py) against the properties a correct extraction
must have, before the GPU tests hold the kernels to it; the PLY writer; argument validation; the command line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_reference as ref
from conftest import REPO


def lattice_box(res):
    """the box in which world coordinates are lattice indices"""
    return (0.0, 0.0, 0.0), tuple(float(n - 1) for n in res)


@pytest.fixture(scope="module")
def table_meshes():
    out = {}
    for name in ref.TABLE:
        sigma, level = ref.field(name)
        verts, faces, mask, fcount = ref.extract(sigma, level, *lattice_box(sigma.shape))
        out[name] = dict(sigma=sigma, verts=verts, faces=faces, mask=mask, fcount=fcount, topo=ref.topology(verts, faces))
    return out


def test_orientation_table_equals_midpoint_geometry():
    """the kernel's form of the orientation (16-bit table, inverted for odd permutations) against the integer geometry of the
    edge midpoints, for every tetrahedron and every inside set that has triangles"""
    for t in range(6):
        for s in range(1, 15):
            assert ref.flip_by_table(t, s) == ref.flip_by_midpoints(t, s), (t, s)
    assert ref.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    for t, perm in enumerate(ref.PERMS):
        assert round(np.linalg.det(np.eye(3)[list(perm)])) == (-1 if ref.ODD_PERMS >> t & 1 else 1)


@pytest.mark.parametrize("name", sorted(ref.TABLE))
def test_reference_on_the_table_fields(table_meshes, name):
    """V, F, closedness and the Euler number the specification states for the four fields.  The binding conditions are
    closedness, the Euler number and where the boundary lies; the counts of the two sphere fields and of the plane depend on
    float32 classifications at the surface and are what this restatement gives (they equal the specification's; for the plane
    see mesh_reference.field)."""
    m = table_meshes[name]
    n_verts, n_faces, closed, euler = ref.TABLE[name]
    topo = m["topo"]
    print(name, len(m["verts"]), len(m["faces"]), topo["closed"], topo["euler"], topo["n_boundary"])
    assert topo["closed"] == closed and topo["euler"] == euler
    assert (len(m["verts"]), len(m["faces"])) == (n_verts, n_faces)
    assert int(m["fcount"].sum()) == n_faces and len(m["fcount"]) == np.prod([n - 1 for n in m["sigma"].shape])
    assert m["faces"].min() >= 0 and m["faces"].max() == n_verts - 1 and len(np.unique(m["faces"])) == n_verts
    if closed:
        assert topo["n_boundary"] == 0


def test_reference_sphere_normals_point_outwards(table_meshes):
    m = table_meshes["sphere"]
    v = m["verts"].astype(np.float64)[m["faces"]]
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    radial = v.mean(axis=1) - np.array([4.1, 3.9, 4.2])
    assert ((normal * radial).sum(-1) > 0).all()
    assert ref.zero_area(m["verts"], m["faces"]) == 0


def test_reference_plane_boundary_lies_on_the_box(table_meshes):
    m = table_meshes["plane"]
    assert m["topo"]["n_boundary"] == 26
    v = m["verts"].astype(np.float64)
    top = np.array(m["sigma"].shape, dtype=np.float64) - 1
    for a, b in m["topo"]["boundary"]:
        on_face = ((v[a] == 0) & (v[b] == 0)) | ((v[a] == top) & (v[b] == top))          # both ends on one face of the box
        assert on_face.any(), (v[a], v[b])
    # evaluated left to right in float32 the plane misses the lattice point (2, 2, 1) by -5.2e-8: other counts, same topology
    i, j, k = ref._grid((5, 4, 3))
    f = np.float32
    alt = f(1.3) - f(0.5) * i - f(0.2) * j + f(0.1) * k
    va, fa, _, _ = ref.extract(alt, 0.0, *lattice_box(alt.shape))
    ta = ref.topology(va, fa)
    assert (len(va), len(fa), ta["n_boundary"], ta["euler"], ta["closed"]) == (43, 60, 24, 1, False)


def test_reference_zero_area_triangles_pair_up(table_meshes):
    """sigma == level exactly at lattice points: 288 of the 384 triangles have no area, and the mesh is closed all the same"""
    m = table_meshes["octahedron"]
    assert ref.zero_area(m["verts"], m["faces"]) == 288
    assert m["topo"]["closed"]


def test_reference_float64_agrees_with_float32(table_meshes):
    m = table_meshes["sphere"]
    v64, f64, _, _ = ref.extract(m["sigma"], 0.0, *lattice_box(m["sigma"].shape), dtype=np.float64)
    assert np.array_equal(f64, m["faces"]) and v64.dtype == np.float64
    assert np.abs(v64 - m["verts"]).max() <= 8 * 2.0 ** -24 * 8


# ---------------------------------------------------------------------------------------------------- PLY
def read_ply(path):
    """-> verts (V, 3) float32, faces (F, 3) int32, normals (V, 3) float32 or None; a reader of its own, numpy only"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_verts = n_faces = None
    props, element = [], None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                n_verts = int(w[2])
            else:
                assert element == "face"
                n_faces = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            assert w[1] == "float"
            props.append(w[2])
        elif w[:1] == ["property"]:
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    assert props in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"])
    v = np.frombuffer(raw, dtype="<f4", count=n_verts * len(props), offset=end).reshape(n_verts, len(props))
    rec = np.frombuffer(raw, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=n_faces, offset=end + v.nbytes)
    assert end + v.nbytes + rec.nbytes == len(raw) and (rec["n"] == 3).all()
    return v[:, :3].copy(), rec["idx"].astype(np.int32).reshape(n_faces, 3), (v[:, 3:].copy() if len(props) == 6 else None)


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("empty", [False, True])
def test_write_ply_round_trip(tmp_path, table_meshes, with_normals, empty):
    from robust_e_nerf_amd import mesh
    m = table_meshes["plane"]
    verts, faces = (m["verts"][:0], m["faces"][:0]) if empty else (m["verts"], m["faces"])
    normals = np.random.default_rng(0).standard_normal(verts.shape).astype(np.float32) if with_normals else None
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), None if normals is None else torch.from_numpy(normals))
    v, f, n = read_ply(path)
    assert v.shape == (len(verts), 3) and f.shape == (len(faces), 3)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    assert (n is None) == (normals is None) and (n is None or np.array_equal(n, normals))
    if with_normals and not empty:
        with pytest.raises(ValueError):
            mesh.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(normals[:-1]))


# ---------------------------------------------------------------------------------------------------- argument validation
def test_ops_refuse_cpu_tensors_and_wrong_layouts():
    from robust_e_nerf_amd import ops
    sigma = torch.zeros(3, 3, 3)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_classify(sigma, 0.0)
    n, cubes = 27, 8
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_write(sigma, 0.0, torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64),
                       torch.zeros(cubes, dtype=torch.int64), (0, 0, 0), (1, 1, 1), 0, 0)
    with pytest.raises(ValueError, match="every extent >= 2"):
        ops.mesh_classify(torch.zeros(3, 1, 3), 0.0)
    with pytest.raises(ValueError, match="every extent >= 2"):
        ops.mesh_classify(torch.zeros(27), 0.0)
    with pytest.raises(ValueError, match="NaN"):
        ops.mesh_classify(sigma, float("nan"))
    with pytest.raises(ValueError, match="lo < hi"):
        ops.mesh_write(sigma, 0.0, torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64),
                       torch.zeros(cubes, dtype=torch.int64), (0, 0, 0), (1, 0, 1), 0, 0)
    with pytest.raises(ValueError, match="foff"):
        ops.mesh_write(sigma, 0.0, torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64),
                       torch.zeros(n, dtype=torch.int64), (0, 0, 0), (1, 1, 1), 0, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.mesh_write(sigma, 0.0, torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int64),
                       torch.zeros(cubes, dtype=torch.int64), (0, 0, 0), (1, 1, 1), 2 ** 31, 5)


def test_library_refuses_bad_arguments_before_any_launch():
    """the C entry points return REN_ERR_BAD_ARG without a device: extents, lattice size, NaN level, null pointers"""
    import ctypes
    from robust_e_nerf_amd import _lib, build
    build.build()
    lib = _lib.load()
    f3 = ctypes.c_float * 3
    one = ctypes.c_void_p(256)                       # an aligned non-null address: nothing is launched, nothing dereferenced
    bad = _lib.REN_ERR_BAD_ARG
    assert lib.ren_mesh_classify(one, 1, 2, 2, 0.0, one, one, one, None) == bad
    assert lib.ren_mesh_classify(one, 1025, 1024, 1024, 0.0, one, one, one, None) == bad
    assert lib.ren_mesh_classify(one, 2, 2, 2, float("nan"), one, one, one, None) == bad
    assert lib.ren_mesh_classify(None, 2, 2, 2, 0.0, one, one, one, None) == bad
    assert lib.ren_mesh_classify(one, 2, 2, 2, 0.0, one, None, one, None) == bad
    lo, hi, h = f3(0, 0, 0), f3(1, 1, 1), f3(1, 1, 1)
    assert lib.ren_mesh_write(one, one, one, one, 2, 2, 2, 0.0, lo, hi, h, 0, 0, None, None, None) == _lib.REN_OK   # zero totals
    assert lib.ren_mesh_write(one, one, one, one, 2, 2, 2, 0.0, lo, hi, h, 3, 1, None, one, None) == bad
    assert lib.ren_mesh_write(one, one, one, one, 2, 2, 2, 0.0, lo, hi, h, 2 ** 31, 1, one, one, None) == bad
    assert lib.ren_mesh_write(one, one, one, one, 2, 2, 2, 0.0, hi, lo, h, 3, 1, one, one, None) == bad
    assert lib.ren_mesh_write(one, one, one, one, 2, 2, 2, 0.0, lo, hi, f3(1, 0, 1), 3, 1, one, one, None) == bad
    assert lib.ren_mesh_write(one, one, ctypes.c_void_p(260), one, 2, 2, 2, 0.0, lo, hi, h, 3, 1, one, one, None) == bad


def test_mesh_module_validation():
    from robust_e_nerf_amd import mesh
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for res in (1, (4, 1, 4), (4, 4), 2.5):
        with pytest.raises(ValueError, match="resolution"):
            mesh.sample_density(None, lo, hi, res)
    with pytest.raises(ValueError, match="2\\^30"):
        mesh.sample_density(None, lo, hi, (1025, 1024, 1024))
    with pytest.raises(ValueError, match="2\\^30"):
        mesh.lattice_points(lo, hi, 1025, 0, 4, device="cpu")
    for bad_hi in ((1.0, 0.0, 1.0), (1.0, 1.0, -1.0), (0.0, 1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="lo < hi"):
            mesh.sample_density(None, lo, bad_hi, 4)
        with pytest.raises(ValueError, match="lo < hi"):
            mesh.extract(torch.zeros(2, 2, 2), 0.0, lo, bad_hi)
    with pytest.raises(ValueError, match="NaN"):
        mesh.extract(torch.zeros(2, 2, 2), float("nan"), lo, hi)
    with pytest.raises(ValueError, match="2\\^30"):                             # a stride-0 view: no memory behind it
        mesh.extract(torch.zeros(1).expand(1025, 1024, 1024), 0.0, lo, hi)
    with pytest.raises(ValueError, match="every extent >= 2"):
        mesh.extract(torch.zeros(4, 1, 4), 0.0, lo, hi)
    with pytest.raises(ValueError, match="CPU tensor"):
        mesh.extract(torch.zeros(2, 2, 2), 0.0, lo, hi)


def test_lattice_points_on_the_cpu():
    from robust_e_nerf_amd import mesh
    lo, hi, res = (-1.5, 0.25, 2.0), (2.5, 1.75, 3.5), (5, 4, 3)
    pts = mesh.lattice_points(lo, hi, res, 0, 60, device="cpu")
    assert pts.shape == (60, 3) and pts.dtype == torch.float32
    assert pts[0].tolist() == list(lo) and pts[59].tolist() == list(hi)
    assert pts[(2 * 4 + 3) * 3 + 1].tolist() == [0.5, 1.75, 2.75]
    assert torch.equal(mesh.lattice_points(lo, hi, res, 7, 31, device="cpu"), pts[7:31])
    with pytest.raises(ValueError):
        mesh.lattice_points(lo, hi, res, 0, 61, device="cpu")


# ---------------------------------------------------------------------------------------------------- command line
def _cli():
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(REPO, "scripts", "export_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_export_mesh_argument_parsing(capsys):
    cli = _cli()
    base = ["--config", "c.yaml", "--ckpt", "x.ckpt", "--out", "m.ply"]
    a = cli.parse_args(base)
    assert a.resolution == (256, 256, 256) and a.level == 10.0 and a.aabb is None and not a.no_normals
    assert cli.parse_args(base + ["--resolution", "64"]).resolution == (64, 64, 64)
    assert cli.parse_args(base + ["--resolution", "64", "32", "16"]).resolution == (64, 32, 16)
    b = cli.parse_args(base + ["--level", "2.5", "--aabb", "-1", "-2", "-3", "1", "2", "3", "--no-normals"])
    assert b.level == 2.5 and b.aabb == [-1.0, -2.0, -3.0, 1.0, 2.0, 3.0] and b.no_normals
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--resolution", "64", "32"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--config", "c.yaml", "--ckpt", "x.ckpt"])                       # --out is required
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    assert "not a value measured" in " ".join(capsys.readouterr().out.split())
