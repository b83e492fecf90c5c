"""Level-set mesh on the GPU (csrc/ren_mesh.hip, robust_e_nerf_amd/mesh.py) against the numpy restatement
tests/mesh_reference.py, index for index.

Rule of every comparison (`check`): faces and the vertex count equal; every vertex within
8 x 2^-24 x (|lo| + (hi - lo)) per axis of the restatement evaluated in float64 (a few roundings of lo + u h); and -- the
library is built with correctly rounded float32 division -- bit-equal to the restatement evaluated in float32.
"""
import numpy as np
import pytest
import torch

import mesh_reference as ref
from conftest import field_params_from, load_golden, t
from test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = (-1.5, 0.25, 2.0), (2.5, 1.75, 3.5)                       # a box in which no axis is trivial
TOL = np.array([8 * 2.0 ** -24 * (abs(a) + (b - a)) for a, b in zip(LO, HI)])


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, mesh, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, mesh


_REF = {}


def reference(key, sigma, level):
    """the restatement of one case in float32 and float64, computed once"""
    if key not in _REF:
        v32, faces, _, _ = ref.extract(sigma, level, LO, HI)
        v64, f64, _, _ = ref.extract(sigma, level, LO, HI, dtype=np.float64)
        assert np.array_equal(faces, f64)
        _REF[key] = (v32, v64, faces)
    return _REF[key]


def run(mesh, sigma, level):
    verts, faces = mesh.extract(torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float32)).to(DEV), level, LO, HI)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.dim() == 2 and faces.dim() == 2
    assert verts.shape[1] == 3 and faces.shape[1] == 3
    return verts.cpu().numpy(), faces.cpu().numpy()


def check(got, want, tag):
    (verts, faces), (v32, v64, f_ref) = got, want
    assert verts.shape == v32.shape and faces.shape == f_ref.shape, (tag, verts.shape, v32.shape, faces.shape, f_ref.shape)
    assert np.array_equal(faces, f_ref), tag
    if len(verts):
        err = np.abs(verts.astype(np.float64) - v64).max(axis=0)
        assert (err <= TOL).all(), (tag, err, TOL)
        assert np.isfinite(verts).all() and (verts >= np.array(LO, dtype=np.float32)).all() and (verts <= np.array(HI, dtype=np.float32)).all(), tag
    assert np.array_equal(verts.view(np.uint32), v32.view(np.uint32)), (tag, "not bit-equal to the float32 restatement")


def test_all_256_patterns_of_one_cube(amd):
    """the 2 x 2 x 2 lattice with every inside / outside pattern: +-1 plus a distinct offset per corner, so that t differs from
    edge to edge; every tetrahedron case in every position"""
    _, mesh = amd
    offset = np.array([0.0, 0.07, 0.13, 0.21, 0.29, 0.36, 0.44, 0.52], dtype=np.float32).reshape(2, 2, 2)
    n_faces = 0
    for pattern in range(256):
        sign = np.array([1.0 if pattern >> c & 1 else -1.0 for c in range(8)], dtype=np.float32).reshape(2, 2, 2)
        sigma = sign + offset
        got = run(mesh, sigma, 0.0)
        check(got, reference(("cube", pattern), sigma, 0.0), f"pattern {pattern}")
        n_faces += len(got[1])
        if pattern in (0, 255):
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    assert n_faces > 256


@pytest.mark.parametrize("res", [(3, 2, 2), (2, 3, 2), (2, 2, 3), (5, 4, 3)])
def test_vertices_shared_across_each_axis(amd, res):
    """two cubes side by side along each axis, and a seeded random field on unequal extents (a transposed stride would show)"""
    _, mesh = amd
    sigma = np.random.default_rng(sum(res) * 7 + res[0]).standard_normal(res).astype(np.float32)
    got = run(mesh, sigma, 0.0)
    assert len(got[1]) > 0
    check(got, reference(("random", res), sigma, 0.0), f"random {res}")


@pytest.fixture(scope="module")
def table_runs(amd):
    _, mesh = amd
    out = {}
    for name in ref.TABLE:
        sigma, level = ref.field(name)
        out[name] = (run(mesh, sigma, level), reference(("table", name), sigma, level))
    return out


@pytest.mark.parametrize("name", sorted(ref.TABLE))
def test_table_fields_against_the_reference(table_runs, name):
    got, want = table_runs[name]
    assert (len(got[0]), len(got[1])) == ref.TABLE[name][:2]
    check(got, want, name)


@pytest.mark.parametrize("name", ["sphere", "two_spheres", "octahedron"])
def test_topology_of_the_kernels_own_output(table_runs, name):
    (verts, faces), _ = table_runs[name]
    topo = ref.topology(verts, faces)
    assert topo["closed"] and topo["n_boundary"] == 0 and topo["euler"] == ref.TABLE[name][3]
    if name == "octahedron":
        assert ref.zero_area(verts, faces) > 0                    # the triangles without area are there and pair up


def test_lattice_above_one_scan_block(amd):
    """41^3 = 68 921 points: past the 65 536 at which exclusive_scan leaves its one-launch path"""
    _, mesh = amd
    sigma = ref.sphere_field((41, 41, 41), (20.2, 19.7, 20.4), 13.3)
    assert sigma.size > 65536
    got = run(mesh, sigma, 0.0)
    check(got, reference("sphere41", sigma, 0.0), "sphere 41^3")
    topo = ref.topology(*got)
    assert topo["closed"] and topo["euler"] == 2


def _edge_field():
    return np.random.default_rng(5).uniform(-1.0, 1.0, (5, 4, 3)).astype(np.float32)       # h = (1, 0.5, 0.75): exact


@pytest.mark.parametrize("case", ["all_outside", "all_inside", "nan", "inf", "neg_inf", "level_in_field"])
def test_edge_values(amd, case):
    """no fault, the reference's result, every vertex finite and inside the box"""
    _, mesh = amd
    sigma, level = _edge_field(), 0.0
    if case == "all_outside":
        level = 2.0
    elif case == "all_inside":
        level = -2.0
    elif case == "nan":
        sigma[2, 1, 1] = np.nan
        sigma[0, 0, 0] = np.nan
    elif case == "inf":
        sigma[2, 2, 1] = np.inf
        sigma[4, 3, 2] = np.inf
    elif case == "neg_inf":
        sigma[2, 2, 1] = -np.inf
        sigma[0, 3, 0] = -np.inf
    else:
        level = float(sigma[3, 1, 1])
        sigma[1, 2, 0] = sigma[3, 1, 1]
    got = run(mesh, sigma, level)
    check(got, reference(("edge", case), sigma, level), case)
    if case in ("all_outside", "all_inside"):
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    else:
        assert len(got[1]) > 0 and got[1].max() == len(got[0]) - 1


def test_two_calls_are_bit_identical(amd):
    _, mesh = amd
    sigma = torch.from_numpy(ref.field("two_spheres")[0]).to(DEV)
    v0, f0 = mesh.extract(sigma, 0.0, LO, HI)
    v1, f1 = mesh.extract(sigma, 0.0, LO, HI)
    assert torch.equal(v0, v1) and torch.equal(f0, f1) and v0.shape[0] == 890


def test_ops_refuse_wrong_dtype_and_layout(amd):
    ops, _ = amd
    sigma = torch.zeros(4, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="dtype"):
        ops.mesh_classify(sigma.double(), 0.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.mesh_classify(sigma.permute(2, 1, 0)[:, :, ::2], 0.0)
    mask, vcount, fcount = ops.mesh_classify(sigma, 0.0)
    assert mask.shape == (64,) and vcount.shape == (64,) and fcount.shape == (27,)
    assert not bool(mask.any()) and not bool(vcount.any()) and not bool(fcount.any())      # sigma == level everywhere: all inside
    voff, _ = ops.exclusive_scan(vcount)
    foff, _ = ops.exclusive_scan(fcount)
    with pytest.raises(ValueError, match="dtype"):
        ops.mesh_write(sigma, 0.0, mask, voff.int(), foff, LO, HI, 0, 0)


# ---------------------------------------------------------------------------------------------- on a real field
RES = 24


@pytest.fixture(scope="module")
def golden_renderer(amd, full_table_cache):
    """the renderer of tests/test_gpu_normals.py's density_gradient test: the golden fixture field_aabb"""
    from robust_e_nerf_amd import engine
    g = load_golden("field_aabb")
    table = full_table_cache(g["table_seed"], g["table_scale"])
    aabb = tuple(float(v) for v in t(g["aabb"]).float())
    fld = engine.NGPField(DEV)
    fld.load(field_params_from(g, table))
    cfg = engine.RenderCfg(aabb=aabb, contraction_type=int(g["contraction_type"]), occ_res=(8, 8, 8))
    return engine.Renderer(fld, cfg), aabb


def test_sample_density_equals_query_density(amd, golden_renderer):
    _, mesh = amd
    r, aabb = golden_renderer
    lo, hi = aabb[:3], aabb[3:]
    sigma = mesh.sample_density(r, lo, hi, RES)
    assert sigma.shape == (RES, RES, RES) and sigma.dtype == torch.float32 and sigma.is_cuda
    pts = mesh.lattice_points(lo, hi, RES, 0, RES ** 3, DEV)
    assert torch.equal(sigma.reshape(-1), r.query_density(pts).reshape(-1))
    assert torch.equal(mesh.sample_density(r, lo, hi, (RES, RES, RES), chunk=5000), sigma)   # a point does not depend on its chunk
    assert torch.equal(pts[0].cpu(), torch.tensor(lo)) and torch.equal(pts[-1].cpu(), torch.tensor(hi))


def test_export_on_a_real_field(amd, golden_renderer, tmp_path):
    """level = the median of the sampled grid: the PLY holds extract's mesh, every index is below V, every vertex is inside the
    box, the normals are unit or zero and are the normalised -density_gradient at the vertices"""
    _, mesh = amd
    r, aabb = golden_renderer
    lo, hi = aabb[:3], aabb[3:]
    sigma = mesh.sample_density(r, lo, hi, RES)
    level = float(sigma.median())
    verts, faces = mesh.extract(sigma, level, lo, hi)
    path = str(tmp_path / "field.ply")
    stats = mesh.export(r, path, RES, level)
    v, f, n = read_ply(path)
    n_verts, n_faces = verts.shape[0], faces.shape[0]
    assert n_verts > 100 and n_faces > 100
    assert stats == dict(verts=n_verts, faces=n_faces, resolution=(RES, RES, RES), normals=True)
    assert np.array_equal(v, verts.cpu().numpy()) and np.array_equal(f, faces.cpu().numpy())
    assert f.min() >= 0 and f.max() < n_verts
    assert (v >= np.array(lo, dtype=np.float32)).all() and (v <= np.array(hi, dtype=np.float32)).all()
    got, want = ref.extract(sigma.cpu().numpy(), level, lo, hi)[:2]
    assert np.array_equal(f, want) and np.array_equal(v.view(np.uint32), got.view(np.uint32))
    normals = mesh.vertex_normals(r, verts)
    assert np.array_equal(n, normals.cpu().numpy())
    _, grad = r.density_gradient(verts)
    length = grad.double().norm(dim=-1, keepdim=True)
    expected = torch.where(length > 0, -grad.double() / length.clamp_min(1e-300), torch.zeros_like(grad.double()))
    assert float((normals.double() - expected).abs().max()) < 1e-6
    nl = normals.double().norm(dim=-1)
    assert bool((((nl - 1).abs() < 1e-5) | (nl == 0)).all()) and bool(((nl == 0) == (length[:, 0] == 0)).all())
    assert float(nl.max()) > 0
    assert torch.equal(mesh.vertex_normals(r, verts, chunk=257), normals)
    # a box of the caller's and three resolutions
    sub_lo, sub_hi = [a + 0.25 * (b - a) for a, b in zip(lo, hi)], [a + 0.75 * (b - a) for a, b in zip(lo, hi)]
    res3 = (12, 9, 7)
    stats3 = mesh.export(r, path, res3, level, sub_lo, sub_hi, normals=False)
    v3, f3, n3 = read_ply(path)
    e3 = mesh.extract(mesh.sample_density(r, sub_lo, sub_hi, res3), level, sub_lo, sub_hi)
    assert n3 is None and stats3["resolution"] == res3 and not stats3["normals"]
    assert np.array_equal(v3, e3[0].cpu().numpy()) and np.array_equal(f3, e3[1].cpu().numpy())


def test_vanilla_architecture_exports_without_normals(amd, tmp_path):
    _, mesh = amd
    from robust_e_nerf_amd import config, engine, vanilla
    fld = vanilla.VanillaField(DEV, 1)
    config.init_field(fld, "mlp", 1, torch.Generator().manual_seed(0))
    r = vanilla.VanillaRenderer(fld, engine.RenderCfg(aabb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)))
    sigma = mesh.sample_density(r, (-1.0,) * 3, (1.0,) * 3, 12)
    assert sigma.shape == (12, 12, 12)
    assert torch.equal(sigma.reshape(-1), r.query_density(mesh.lattice_points((-1.0,) * 3, (1.0,) * 3, 12, 0, 12 ** 3, DEV)).reshape(-1))
    level = float(sigma.median())
    verts, faces = mesh.extract(sigma, level, (-1.0,) * 3, (1.0,) * 3)
    with pytest.raises(NotImplementedError):
        mesh.vertex_normals(r, verts)
    with pytest.raises(NotImplementedError):
        mesh.vertex_normals(r, verts[:0])
    path = str(tmp_path / "vanilla.ply")
    with pytest.raises(NotImplementedError):
        mesh.export(r, path, 12, level)
    stats = mesh.export(r, path, 12, level, normals=False)
    v, f, n = read_ply(path)
    assert n is None and stats["verts"] == len(v) == verts.shape[0] and stats["faces"] == len(f) == faces.shape[0]
    assert np.array_equal(v, verts.cpu().numpy()) and np.array_equal(f, faces.cpu().numpy())
