"""CPU: the numpy restatement of the depth-map fusion (tests/tsdf_reference.py) -- independence of how the views are split
into calls, and the geometry of what it fuses (a sphere seen from two rings of cameras, meshed by the marching-tetrahedra
restatement) -- before the GPU tests hold the kernel to it bit for bit; mask_depth and pack_cameras; the command line;
argument validation of ren_tsdf_integrate without a device."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_reference as mref
import tsdf_reference as tref
from conftest import REPO


# ---------------------------------------------------------------------------------------------------- the restatement
def small_case():
    rng = np.random.default_rng(11)
    centres = [(2.0, 0.3, 0.4), (-0.2, 1.9, -0.5), (0.1, -0.4, 2.2), (-1.8, -0.9, 0.2), (0.2, 0.1, 0.1)]     # the last: inside
    cams = tref.pack(centres, [tref.look_at(c, (0.05, -0.03, 0.02)) for c in centres])
    K = tref.pinhole(10.0, 12, 16)
    K[0, 1] = 0.25
    depth = tref.sphere_depth(cams, K, 12, 16, 0.6)
    depth[rng.random(depth.shape) < 0.1] = np.nan
    return depth, cams, K, (-1.0, -0.8, -0.9), (1.0, 0.9, 0.7), (5, 7, 9), 0.4


def test_the_reference_does_not_depend_on_how_the_views_are_split():
    depth, cams, K, lo, hi, res, trunc = small_case()
    field, count, (total, _) = tref.fuse(depth, cams, K, lo, hi, res, trunc)
    assert field.dtype == np.float32 and count.dtype == np.int32 and field.shape == res and count.max() >= 3 and count.min() == 0
    assert np.array_equal(field == -1.0, (count == 0) | (field == -1.0)) and (field[count == 0] == -1.0).all()
    for split in ([1, 2, 3, 4], [2]):
        state = None
        for part in zip([0] + split, split + [len(depth)]):
            f, c, state = tref.fuse(depth[part[0]: part[1]], cams[part[0]: part[1]], K, lo, hi, res, trunc, state=state)
        assert np.array_equal(state[0].view(np.int32), total.view(np.int32)) and np.array_equal(c, count)
        assert np.array_equal(f.view(np.int32), field.view(np.int32))
    f0, c0, s0 = tref.fuse(depth[:0], cams[:0], K, lo, hi, res, trunc, state=state)                  # no view: untouched
    assert np.array_equal(s0[0].view(np.int32), total.view(np.int32)) and np.array_equal(c0, count)


def test_the_lattice_is_that_of_mesh_lattice_points():
    from robust_e_nerf_amd import mesh
    for lo, hi, res in (((-1.0, -0.8, -0.9), (1.0, 0.9, 0.7), (5, 7, 9)), ((0.1, 0.2, 0.3), (0.7, 1.3, 2.9), (3, 70, 67))):
        n = res[0] * res[1] * res[2]
        want = mesh.lattice_points(lo, hi, res, 0, n, device="cpu").numpy()
        assert np.array_equal(tref.lattice(lo, hi, res).view(np.int32), want.view(np.int32))


def test_sphere_depth_is_the_depth_of_the_sphere():
    depth, cams, K = tref.sphere_inputs()
    assert depth.shape == (12, 64, 64) and np.isinf(depth).any() and np.isfinite(depth).any()
    centre = depth[:, 32, 32]                                                      # half a pixel off the axis: just over 1.5
    assert (np.abs(centre - 1.5) < 1e-3).all() and (depth[np.isfinite(depth)] >= 1.5 - 1e-6).all()
    assert (depth[np.isfinite(depth)] <= math.sqrt(4.0 - 0.25) + 1e-6).all()        # the tangent points


@pytest.fixture(scope="module")
def sphere_mesh():
    depth, cams, K = tref.sphere_inputs()
    s = tref.SPHERE
    field, count, _ = tref.fuse(depth, cams, K, s["lo"], s["hi"], s["res"], s["trunc"])
    verts, faces, _, _ = mref.extract(tref.fill_inner_shell(field), 0.0, s["lo"], s["hi"])
    return field, count, verts, faces


def test_geometry_of_the_fused_sphere(sphere_mesh):
    """sphere of radius 0.5, 12 cameras on two rings at distance 2, 64 x 64 pixels at f = 64, lattice 33^3 over [-1, 1]^3, trunc
    three spacings, free space carved by the +inf of the renderer: the mean of | |vertex| - 0.5 | over the outer surface stays
    below half a lattice spacing (0.03125) and the maximum below twice the maximum measured with the restatement alone
    (tsdf_reference.MEASURED_MAX; the maximum sits at silhouette pixels, where the nearest-pixel depth jumps)."""
    field, count, verts, faces = sphere_mesh
    s = tref.SPHERE
    assert len(verts) > 500 and len(faces) > 1000
    mean, worst, rad = tref.radial_error(verts)
    print(f"fused sphere: {len(verts)} vertices, {len(faces)} faces; | |v| - r |: mean {mean:.6f}, max {worst:.6f}; "
          f"spacing {s['spacing']}, smallest radius {rad.min():.4f}")
    assert rad.min() > s["radius"] - s["trunc"] / 2                                 # the inner shell is filled: one surface
    assert mean < 0.5 * s["spacing"]
    assert worst < 2.0 * tref.MEASURED_MAX
    assert abs(mean - tref.MEASURED_MEAN) < 1e-5 and abs(worst - tref.MEASURED_MAX) < 1e-5    # what DESIGN 3.15 quotes
    topo = mref.topology(verts, faces)
    assert topo["closed"] and topo["euler"] == 2


def test_the_inner_shell_is_there_without_the_fill(sphere_mesh):
    """points farther than trunc behind every surface are never seen: outside, at depth about trunc"""
    field, count, _, _ = sphere_mesh
    s = tref.SPHERE
    x = tref.lattice(s["lo"], s["hi"], s["res"]).astype(np.float64)
    rad = np.linalg.norm(x, axis=1)
    deep = rad < s["radius"] - s["trunc"] - s["spacing"]
    assert deep.sum() > 50 and (count.reshape(-1)[deep] == 0).all() and (field.reshape(-1)[deep] == -1.0).all()
    far = rad > s["radius"] + s["trunc"] + s["spacing"]
    assert (field.reshape(-1)[far & (count.reshape(-1) > 0)] == -1.0).all()          # carved free space


# ---------------------------------------------------------------------------------------------------- the torch pieces
def test_mask_depth_and_pack_cameras():
    from robust_e_nerf_amd import tsdf
    nan, inf = math.nan, math.inf
    depth = torch.tensor([[1.0, 2.0, 0.0, -1.0], [nan, inf, 3.0, 4.0]])
    opac = torch.tensor([[0.9, 0.1, 0.9, 0.9], [0.9, 0.9, 0.5, 0.49]])
    for carve, gap in ((False, nan), (True, inf)):
        got = tsdf.mask_depth(depth, opac, 0.5, carve)
        want = torch.tensor([[1.0, gap, nan, nan], [nan, nan, 3.0, gap]])
        assert got.dtype == torch.float32 and torch.equal(got.nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0))
    pos, rot = torch.arange(6.0).reshape(2, 3), torch.arange(18.0).reshape(2, 3, 3) + 10
    cams = tsdf.pack_cameras(pos, rot)
    assert cams.shape == (2, 12) and cams.is_contiguous() and cams[1].tolist() == [3, 4, 5] + list(range(19, 28))
    with pytest.raises(ValueError):
        tsdf.pack_cameras(pos, rot[:1])
    assert tsdf.default_trunc((-1, -1, -1), (1, 1, 3), (33, 17, 33)) == 3 * 0.125


def test_ops_refuse_bad_arguments_without_a_device():
    from robust_e_nerf_amd import ops
    depth, cams, K = torch.zeros(2, 4, 4), torch.zeros(2, 12), torch.eye(3)
    total, count = torch.zeros(3, 3, 3), torch.zeros(3, 3, 3, dtype=torch.int32)
    lo, hi, res = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 3, 3)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.tsdf_integrate(depth, cams, K, lo, hi, res, 0.1, 1e-6, total, count)
    for kw in (dict(depth=depth[0]), dict(cams=cams[:1]), dict(cams=torch.zeros(2, 9)), dict(K=torch.eye(4)), dict(hi=(1.0, 0.0, 1.0)),
               dict(lo=(math.nan, 0.0, 0.0)), dict(res=(3, 3)), dict(res=(3, 1, 3)), dict(res=(1024, 1024, 1025)), dict(trunc=0.0),
               dict(trunc=math.inf), dict(z_min=-1.0), dict(z_min=math.nan), dict(total=total[:2]), dict(count=count[:2])):
        a = dict(depth=depth, cams=cams, K=K, lo=lo, hi=hi, res=res, trunc=0.1, z_min=1e-6, total=total, count=count)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.tsdf_integrate(a["depth"], a["cams"], a["K"], a["lo"], a["hi"], a["res"], a["trunc"], a["z_min"], a["total"], a["count"])
    assert ops.TSDF_VIEW_BATCH >= 1


# ---------------------------------------------------------------------------------------------------- the library
def test_library_exports_the_entry_point_and_refuses_bad_arguments_before_any_launch():
    from robust_e_nerf_amd import _lib, build, ops
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    assert hasattr(lib, "ren_tsdf_integrate") and "ren_tsdf_integrate" in _lib.SIGNATURES and "int ren_tsdf_integrate(" in hdr
    assert hdr.index("---- tsdf") > hdr.index("---- mesh distance")
    assert f"#define REN_TSDF_VIEW_BATCH {ops.TSDF_VIEW_BATCH} " in hdr and f"#define REN_TSDF_MAX_IMAGE {ops.TSDF_MAX_IMAGE} " in hdr
    assert "ren_tsdf.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE["ren_tsdf.hip"]
    assert lib.ren_abi_version() == 25
    one, odd, odd8 = ctypes.c_void_p(256), ctypes.c_void_p(258), 260                 # no device pointer is dereferenced
    bad, ok, f = _lib.REN_ERR_BAD_ARG, _lib.REN_OK, ctypes.c_float
    f5, d3 = ctypes.c_float * 5, ctypes.c_double * 3
    good = dict(depth=one, V=2, H=4, W=4, cams=one, K5=f5(8, 0, 1.5, 8, 1.5), lo=d3(0, 0, 0), step=d3(0.5, 0.5, 0.5), nx=3, ny=3, nz=3,
                trunc=f(0.1), z_min=f(1e-6), sum=one, count=one, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ren_tsdf_integrate(*(a[k] for k in good))

    assert call(V=0) == ok and call(V=0, depth=None, cams=None) == ok               # no view: nothing is launched
    assert call(H=0, depth=None) == ok and call(W=0, depth=None) == ok               # no pixel: every view skips every point
    for kw in (dict(V=-1), dict(H=-1), dict(W=-1), dict(H=16385), dict(W=16385), dict(V=2 ** 17, H=128, W=128),
               dict(V=8, H=16384, W=16384)):
        assert call(**kw) == bad, kw
    assert call(V=2 ** 17 - 1, H=128, W=128, nx=1) == bad                            # (just below 2^31 pixels: the lattice refuses)
    for kw in (dict(nx=1), dict(ny=1), dict(nz=0), dict(nx=-3), dict(nx=1024, ny=1024, nz=1025), dict(nx=2 ** 16, ny=2 ** 16, nz=2)):
        assert call(**kw) == bad, kw
    for v in (0.0, -0.1, math.nan, math.inf):
        assert call(trunc=f(v)) == bad and call(z_min=f(v)) == bad, v
    for v in (math.nan, math.inf, -math.inf):
        assert call(lo=d3(0, v, 0)) == bad and call(step=d3(0.5, 0.5, v)) == bad, v
    for v in (0.0, -0.5):
        assert call(step=d3(v, 0.5, 0.5)) == bad, v
    for name in ("depth", "cams", "K5", "lo", "step", "sum", "count"):
        assert call(**{name: None}) == bad, name
    assert call(V=0, sum=None) == bad and call(V=0, count=None) == bad and call(V=0, K5=None) == bad
    for name in ("depth", "cams", "sum", "count"):
        assert call(**{name: odd}) == bad, name
    for name, kind in (("lo", ctypes.c_double), ("step", ctypes.c_double), ("K5", ctypes.c_float)):
        assert call(**{name: ctypes.cast(ctypes.c_void_p(odd8 if kind is ctypes.c_double else 258), ctypes.POINTER(kind))}) == bad, name


# ---------------------------------------------------------------------------------------------------- the command line
def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(capsys):
    cli = load_script("export_mesh")
    base = ["--config", "c.yaml", "--out", "m.ply"]
    args = cli.parse_args(base)
    assert (args.tsdf, args.tsdf_views, args.tsdf_trunc, args.tsdf_min_opacity, args.tsdf_carve) == (False, 64, None, 0.5, False)
    assert args.level == 10.0
    args = cli.parse_args(base + ["--tsdf", "--tsdf-views", "8", "--tsdf-trunc", "0.05", "--tsdf-min-opacity", "0.3", "--tsdf-carve"])
    assert (args.tsdf, args.tsdf_views, args.tsdf_trunc, args.tsdf_min_opacity, args.tsdf_carve) == (True, 8, 0.05, 0.3, True)
    for bad in (["--tsdf", "--tsdf-views", "0"], ["--tsdf", "--tsdf-trunc", "0"], ["--tsdf", "--tsdf-trunc", "nan"],
                ["--tsdf", "--tsdf-min-opacity", "1.5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    capsys.readouterr()
    cli.parse_args(base + ["--tsdf", "--level", "3"])
    assert "--level is ignored" in capsys.readouterr().err
    cli.parse_args(base + ["--tsdf"])
    assert "--level" not in capsys.readouterr().err
    help_text = cli.build_parser().format_help()
    assert "--tsdf" in help_text and "inner shell" in " ".join(help_text.split()) and "--fill-cavities" in help_text


def test_view_times_are_evenly_spaced():
    from robust_e_nerf_amd import data
    ts = torch.tensor([100, 150, 400, 1100], dtype=torch.int64)
    assert data.even_view_times(ts, 1).tolist() == [100.0] and data.even_view_times(ts, 1).dtype == torch.float64
    assert data.even_view_times(ts, 5).tolist() == [100.0, 350.0, 600.0, 850.0, 1100.0]
    with pytest.raises(ValueError):
        data.even_view_times(ts, 0)
