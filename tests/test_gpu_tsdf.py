"""Depth-map fusion on the GPU (csrc/ren_tsdf.hip, robust_e_nerf_amd/tsdf.py) against the numpy restatement
tests/tsdf_reference.py: torch.equal on the bits of sum and on count, no tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

import tsdf_reference as tref
from conftest import field_params_from, load_golden, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = (-1.0, -0.8, -0.9), (1.0, 0.9, 0.7)                       # a box in which no axis is trivial
TRUNC, Z_MIN = 0.4, 1e-6


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, mesh, ops, tsdf
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, mesh, tsdf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_fuse(tsdf, depth, cams, K, lo, hi, res, trunc, z_min, state=None):
    cams = np.asarray(cams, dtype=np.float32).reshape(-1, 12)
    return tsdf.fuse(dev(depth), K, dev(cams[:, :3]), dev(cams[:, 3:].reshape(-1, 3, 3)), lo, hi, res, trunc, z_min, state=state)


def same(got, want, tag):
    """(field, count, (sum, count)) of tsdf.fuse against the reference's: bits of sum and field, count"""
    (field, count, (total, _)), (r_field, r_count, (r_total, _)) = got, want
    assert total.dtype == torch.float32 and count.dtype == torch.int32 and field.dtype == torch.float32
    assert field.shape == r_field.shape and count.shape == r_count.shape
    assert torch.equal(count.cpu(), torch.from_numpy(r_count)), (tag, "count")
    assert torch.equal(total.cpu().reshape(-1).view(torch.int32), torch.from_numpy(r_total).view(torch.int32)), (tag, "sum")
    unseen = count == 0
    assert bool((field[unseen] == -1.0).all()), (tag, "field where count == 0")
    seen = ~unseen.cpu()
    assert torch.equal(field.cpu()[seen].view(torch.int32), torch.from_numpy(r_field)[seen].view(torch.int32)), (tag, "field")


def scene(n_views, height, width, seed):
    """random cameras around the box looking inwards; with three views and more the second stands INSIDE the box (points lie
    behind it) and the third looks AWAY (every point is skipped); depths around the camera distance, so that both
    truncations and the band between them occur, with NaN, +inf, 0 and negative pixels sprinkled in"""
    rng = np.random.default_rng(seed)
    centres, rots = [], []
    for v in range(n_views):
        direction = rng.standard_normal(3)
        c = 2.2 * direction / np.linalg.norm(direction)
        target = rng.uniform(-0.2, 0.2, 3)
        if n_views >= 3 and v == 1:
            c = np.array([0.15, -0.1, 0.05])
        if n_views >= 3 and v == 2:
            target = 2.0 * c
        centres.append(c)
        rots.append(tref.look_at(c, target))
    cams = tref.pack(centres, rots)
    K = tref.pinhole(0.45 * max(height, width), height, width)
    K[0, 1] = 0.125
    if height == width == 1:
        K = np.array([[0.6, 0.0, 0.0], [0.0, 0.6, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    depth = rng.uniform(1.2, 3.2, (n_views, height, width)).astype(np.float32)
    kind = rng.random(depth.shape)
    for value, (a, b) in ((np.nan, (0.0, 0.05)), (np.inf, (0.05, 0.15)), (0.0, (0.15, 0.18)), (-1.5, (0.18, 0.21))):
        depth[(kind >= a) & (kind < b)] = value
    if n_views >= 3:
        depth[1] = np.where(np.isfinite(depth[1]), depth[1] - 1.2, depth[1])        # the inside camera is nearer to everything
    return depth, cams, K


def view_counts():
    from robust_e_nerf_amd import ops
    return (1, 3, ops.TSDF_VIEW_BATCH + 1)                                         # the last: one more than the kernel stages at once


# (5, 7, 9): all extents different and odd; (2, 2, 2): the smallest; (3, 70, 67): several workgroups with a ragged tail and a
# k-line that is no multiple of 64
@pytest.mark.parametrize("res", [(5, 7, 9), (2, 2, 2), (3, 70, 67)], ids=lambda r: "x".join(map(str, r)))
def test_sum_and_count_equal_the_reference(amd, res):
    _, _, tsdf = amd
    seen_terms = set()
    for n_views in view_counts():
        for height, width in ((12, 16), (16, 12), (1, 1)):
            depth, cams, K = scene(n_views, height, width, seed=n_views * 100 + height)
            want = tref.fuse(depth, cams, K, LO, HI, res, TRUNC, Z_MIN)
            same(gpu_fuse(tsdf, depth, cams, K, LO, HI, res, TRUNC, Z_MIN), want, (res, n_views, height, width))
            if n_views == 1 and (height, width) != (1, 1):
                total, count = want[2]
                seen_terms |= {"unseen"} if (count == 0).any() else set()
                seen_terms |= {"free"} if (total[count == 1] == 1.0).any() else set()
                seen_terms |= {"band"} if (np.abs(total[count == 1]) < 1.0).any() else set()
    if res != (2, 2, 2):
        assert seen_terms == {"unseen", "free", "band"}, seen_terms                   # the inputs reach every branch


def test_a_camera_that_looks_away_and_one_inside_the_box(amd):
    _, _, tsdf = amd
    res = (5, 7, 9)
    c = np.array([2.0, 0.3, -0.4])
    away = tref.pack([c], [tref.look_at(c, 2.0 * c)])
    K = tref.pinhole(6.0, 12, 16)
    depth = np.full((1, 12, 16), 2.0, dtype=np.float32)
    got = gpu_fuse(tsdf, depth, away, K, LO, HI, res, TRUNC, Z_MIN)
    same(got, tref.fuse(depth, away, K, LO, HI, res, TRUNC, Z_MIN), "away")
    assert not bool(got[1].any()) and bool((got[0] == -1.0).all())                  # every point lies behind the camera
    c = np.array([0.1, 0.05, -0.1])
    inside = tref.pack([c], [tref.look_at(c, (1.0, 0.2, 0.3))])
    depth = np.full((1, 12, 16), 0.5, dtype=np.float32)
    got = gpu_fuse(tsdf, depth, inside, K, LO, HI, res, TRUNC, Z_MIN)
    want = tref.fuse(depth, inside, K, LO, HI, res, TRUNC, Z_MIN)
    same(got, want, "inside")
    assert 0 < int(got[1].sum()) < got[1].numel()


# ---------------------------------------------------------------------------------------------------- exact ties
# An axis-aligned camera at (0, 0, -2) looking along +z, k00 = k11 = 8, principal point (3.5, 2.5), 8 x 6 pixels; lattice
# coordinates multiples of 1 / 8: x in [-0.5, 0.5] (9), y in [-0.375, 0.375] (7), z in {-1.5, -1, -0.5, 0} -> depth 0.5, 1, 1.5, 2.
# At depth 1, u + 0.5 = 8 x + 4 is the integer 0 .. 8: exactly 0 is kept, exactly W = 8 is skipped; v + 0.5 = 8 y + 3 is 0 .. 6,
# exactly H = 6 is skipped.  At depth 2 they are half-integers.  z_min = 0.5: the plane at depth 0.5 has z == z_min, skipped.
TIE_LO, TIE_HI, TIE_RES = (-0.5, -0.375, -1.5), (0.5, 0.375, 0.0), (9, 7, 4)
TIE_CAM = np.array([[0, 0, -2, 1, 0, 0, 0, 1, 0, 0, 0, 1]], dtype=np.float32)
TIE_K = np.array([[8, 0, 3.5], [0, 8, 2.5], [0, 0, 1]], dtype=np.float32)
TIE_TRUNC, TIE_Z_MIN = 0.25, 0.5


def test_exact_ties_by_hand(amd):
    _, _, tsdf = amd
    for D, term in ((0.75, -1.0), (1.25, 1.0), (1.0, 0.0), (math.inf, 1.0)):         # s == -trunc: kept, t = -1; s == trunc: t = 1
        depth = np.full((1, 6, 8), D, dtype=np.float32)
        field, count, (total, _) = gpu_fuse(tsdf, depth, TIE_CAM, TIE_K, TIE_LO, TIE_HI, TIE_RES, TIE_TRUNC, TIE_Z_MIN)
        plane = count[:, :, 1].cpu()                                                # depth 1
        want = torch.zeros(9, 7, dtype=torch.int32)
        want[:8, :6] = 1                                                            # fu = 8 = W and fv = 6 = H are skipped, 0 is kept
        assert torch.equal(plane, want), D
        assert bool((total[:8, :6, 1] == term).all()) and bool((total[8, :, 1] == 0).all()) and bool((total[:, 6, 1] == 0).all()), D
        assert not bool(count[:, :, 0].any()), D                                    # z == z_min
        same((field, count, (total, count)), tref.fuse(depth, TIE_CAM, TIE_K, TIE_LO, TIE_HI, TIE_RES, TIE_TRUNC, TIE_Z_MIN), D)
    for D in (0.0, -1.0, math.nan):                                                 # no information
        depth = np.full((1, 6, 8), D, dtype=np.float32)
        _, count, (total, _) = gpu_fuse(tsdf, depth, TIE_CAM, TIE_K, TIE_LO, TIE_HI, TIE_RES, TIE_TRUNC, TIE_Z_MIN)
        assert not bool(count.any()) and not bool(total.any()), D


def test_exact_ties_with_mixed_depths(amd):
    _, _, tsdf = amd
    values = np.array([0.75, 1.25, 0.0, -1.0, np.nan, np.inf, 1.0, 1.125, 0.7499999, 1.75, 2.25, 0.5], dtype=np.float32)
    idx = np.arange(48).reshape(6, 8)
    depth = np.stack([values[(idx * 5 + shift) % len(values)] for shift in range(3)])
    cams = np.repeat(TIE_CAM, 3, axis=0)
    got = gpu_fuse(tsdf, depth, cams, TIE_K, TIE_LO, TIE_HI, TIE_RES, TIE_TRUNC, TIE_Z_MIN)
    want = tref.fuse(depth, cams, TIE_K, TIE_LO, TIE_HI, TIE_RES, TIE_TRUNC, TIE_Z_MIN)
    same(got, want, "mixed")
    assert set(np.unique(want[1])) == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------- chunking, V == 0
def test_the_split_into_calls_does_not_matter_and_no_view_changes_nothing(amd):
    ops, _, tsdf = amd
    res = (3, 70, 67)
    depth, cams, K = scene(5, 12, 16, seed=77)
    whole = gpu_fuse(tsdf, depth, cams, K, LO, HI, res, TRUNC, Z_MIN)
    for cuts in ([0, 1, 2, 3, 4, 5], [0, 2, 5]):
        state = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = gpu_fuse(tsdf, depth[a:b], cams[a:b], K, LO, HI, res, TRUNC, Z_MIN, state=state)
            state = part[2]
        assert torch.equal(part[0].view(torch.int32), whole[0].view(torch.int32)) and torch.equal(part[1], whole[1]), cuts
        assert torch.equal(state[0].view(torch.int32), whole[2][0].view(torch.int32)) and torch.equal(state[1], whole[2][1]), cuts
    before = (whole[2][0].clone(), whole[2][1].clone())
    none = gpu_fuse(tsdf, depth[:0], cams[:0], K, LO, HI, res, TRUNC, Z_MIN, state=whole[2])
    assert none[2][0] is whole[2][0] and torch.equal(none[2][0].view(torch.int32), before[0].view(torch.int32))
    assert torch.equal(none[2][1], before[1]) and torch.equal(none[0].view(torch.int32), whole[0].view(torch.int32))
    again = gpu_fuse(tsdf, depth, cams, K, LO, HI, res, TRUNC, Z_MIN)                # a pure function of its inputs
    assert torch.equal(again[0].view(torch.int32), whole[0].view(torch.int32)) and torch.equal(again[1], whole[1])
    with pytest.raises(ValueError, match="dtype"):
        ops.tsdf_integrate(dev(depth).double(), dev(cams), K, LO, HI, res, TRUNC, Z_MIN, whole[2][0], whole[2][1])


# ---------------------------------------------------------------------------------------------------- end to end
def test_fused_sphere_end_to_end(amd):
    """the CPU test's sphere set-up with the reference renderer's depth maps uploaded: tsdf.fuse, mesh.clean(fill_cavities=True),
    mesh.extract at level 0 -- the field equals the reference's, the inner shell is gone, and the CPU test's two bounds hold"""
    _, mesh, tsdf = amd
    s = tref.SPHERE
    depth, cams, K = tref.sphere_inputs()
    got = gpu_fuse(tsdf, depth, cams, K, s["lo"], s["hi"], s["res"], s["trunc"], 1e-6)
    same(got, tref.fuse(depth, cams, K, s["lo"], s["hi"], s["res"], s["trunc"]), "sphere")
    field, stats = mesh.clean(got[0], 0.0, fill_cavities=True)
    assert stats["cavities"] >= 1 and stats["filled_points"] > 50
    verts, faces = mesh.extract(field, 0.0, s["lo"], s["hi"])
    assert verts.shape[0] > 500 and faces.shape[0] > 1000
    mean, worst, rad = tref.radial_error(verts.cpu().numpy())
    print(f"fused sphere on the GPU: {verts.shape[0]} vertices, {faces.shape[0]} faces; mean {mean:.6f}, max {worst:.6f}")
    assert rad.min() > s["radius"] - s["trunc"] / 2                                 # no vertex of an inner shell
    assert mean < 0.5 * s["spacing"] and worst < 2.0 * tref.MEASURED_MAX
    unfilled = mesh.extract(got[0], 0.0, s["lo"], s["hi"])[0]
    assert float(unfilled.norm(dim=1).min()) < s["radius"] - s["trunc"] / 2         # it was there before the fill


@pytest.fixture(scope="module")
def golden_renderer(amd, full_table_cache):
    """the renderer of tests/test_gpu_mesh.py's export test: the golden fixture field_aabb"""
    from robust_e_nerf_amd import engine
    g = load_golden("field_aabb")
    table = full_table_cache(g["table_seed"], g["table_scale"])
    aabb = tuple(float(v) for v in t(g["aabb"]).float())
    fld = engine.NGPField(DEV)
    fld.load(field_params_from(g, table))
    cfg = engine.RenderCfg(aabb=aabb, contraction_type=int(g["contraction_type"]), occ_res=(8, 8, 8))
    return engine.Renderer(fld, cfg), aabb


def test_export_on_a_real_field(amd, golden_renderer, tmp_path):
    """17^3 lattice, 4 views of 16 x 16 around the box: the PLY holds what the returned dict counts, and the fused field is
    that of fuse over the same renders"""
    _, mesh, tsdf = amd
    from robust_e_nerf_amd import evaluation, mesh_distance
    r, aabb = golden_renderer
    lo, hi = np.array(aabb[:3]), np.array(aabb[3:])
    mid, half = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    centres = [mid + 2.0 * half * np.array(d) / np.linalg.norm(d) for d in ((1, 0.2, 0.3), (-0.3, 1, 0.2), (0.2, -0.3, -1), (-1, -1, 0.4))]
    cams = tref.pack(centres, [tref.look_at(c, mid) for c in centres])
    K = tref.pinhole(14.0, 16, 16)
    Kinv = torch.from_numpy(np.linalg.inv(K.astype(np.float64)).astype(np.float32)).to(DEV)
    cam_pos, cam_rot = dev(cams[:, :3]), dev(cams[:, 3:].reshape(-1, 3, 3))
    path = str(tmp_path / "tsdf.ply")
    stats = tsdf.export(r, path, K, Kinv, cam_pos, cam_rot, 16, 16, 17, min_opacity=0.1, carve=True, views_per_call=3)
    v, f = mesh_distance.read_ply(path)
    assert stats["verts"] == len(v) and stats["faces"] == len(f) and stats["resolution"] == (17, 17, 17) and stats["normals"]
    assert stats["views"] == 4 and stats["tsdf"] is True and 0 < stats["observed"] <= 17 ** 3
    assert stats["trunc"] == tsdf.default_trunc(aabb[:3], aabb[3:], 17)
    maps = []
    for k in range(4):
        _, opacity, depth = evaluation.render_image(r, Kinv, cam_pos[k], cam_rot[k], 16, 16)
        maps.append(tsdf.mask_depth(depth, opacity, 0.1, True))
    field, count, _ = tsdf.fuse(torch.stack(maps), K, cam_pos, cam_rot, aabb[:3], aabb[3:], 17, stats["trunc"])
    assert int((count > 0).sum()) == stats["observed"]
    verts, faces = mesh.extract(field, 0.0, aabb[:3], aabb[3:])
    assert np.array_equal(v, verts.cpu().numpy()) and np.array_equal(f, faces.cpu().numpy())
