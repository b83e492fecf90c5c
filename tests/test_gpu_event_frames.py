"""GPU: event frames (csrc/ren_event_frames.hip, robust_e_nerf_amd.event_frames).  Kernel A (events -> per-window count
images) and kernel B (per-window comparison sums) against the numpy restatements of tests/event_frames_reference.py;
predicted_change against evaluation.render_image; the closed loop prediction -> events -> counts -> comparison; the CLI."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import REPO
import event_frames_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(x).to(DEV).contiguous()


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, engine, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, engine


# ------------------------------------------------------------------------------------------------------------ kernel A
def _events(n, H, W, edges, seed, outside=True):
    """n time-ordered events over [edges[0] - 50, edges[-1] + 50): some exactly on every edge (n permitting), and, with
    `outside`, some with coordinates outside the image"""
    g = np.random.default_rng(seed)
    edges = np.asarray(edges, np.int64)
    ts = g.integers(int(edges[0]) - 50, int(edges[-1]) + 50, n).astype(np.int64)
    k = min(n // 2, len(edges))
    if k:
        ts[g.choice(n, size=k, replace=False)] = edges[g.choice(len(edges), size=k, replace=False)]
    ts.sort()
    pos = np.stack([g.integers(0, W, n), g.integers(0, H, n)], -1).astype(np.uint16)
    if outside and n >= 8:
        pos[g.choice(n, 4, replace=False)] = [[W, 0], [0, H], [65535, 65535], [W + 1, H - 1]]
    return pos, ts, g.random(n) < 0.5


def _check_counts(ops, pos, ts, pol, edges, H, W):
    """both forms of the kernel == the restatement, element for element; the call repeated: bitwise equal"""
    want = torch.from_numpy(ref.count_images(pos, ts, pol, edges, H, W))
    args = (dev(pos), dev(ts), dev(pol), dev(np.asarray(edges, np.int64)), H, W)
    got = ops.event_frames(*args)
    assert got.dtype == torch.int32 and got.shape == want.shape and got.is_cuda
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} counters differ"
    assert torch.equal(ops.event_frames(*args), got)
    assert torch.equal(ops.event_frames(*args, merge=True), got)
    return want


EDGES5 = [100, 180, 180, 260, 300, 420]          # window 1 is empty: edges[1] == edges[2]


@pytest.mark.parametrize("n", [0, 1, 65, 64 * 5 + 1, 256 * 3 + 1])
def test_counts_small_streams_and_tail_lanes(amd, n):
    """5 x 7 pixels (W no multiple of anything), V = 1 and V = 5 with an empty window: no event, one event, one lane past a
    wave, past five waves, past three workgroups; events before the first edge, at and after the last, on interior edges,
    outside the image"""
    ops, _ = amd
    H, W = 5, 7
    for edges in ([100, 420], EDGES5):
        pos, ts, pol = _events(n, H, W, edges, n + len(edges))
        want = _check_counts(ops, pos, ts, pol, edges, H, W)
        if n >= 65 and len(edges) == 6:
            assert int(want[1].sum()) == 0 and int(want.sum()) < n
            assert (ts < edges[0]).any() and (ts >= edges[-1]).any()


def test_counts_edge_rules_one_event_at_a_time(amd):
    """a single event exactly on an interior edge opens the later window; on the last edge, before the first edge, at x == W
    or y == H it is dropped"""
    ops, _ = amd
    H, W = 5, 7
    for t, xy, where in ((260, (2, 3), 3), (180, (6, 4), 2), (100, (0, 0), 0), (419, (1, 1), 4), (420, (1, 1), None),
                         (99, (1, 1), None), (200, (7, 0), None), (200, (0, 5), None)):
        pos, ts, pol = np.array([xy], np.uint16), np.array([t], np.int64), np.array([True])
        want = _check_counts(ops, pos, ts, pol, EDGES5, H, W)
        assert int(want.sum()) == (0 if where is None else 1)
        if where is not None:
            assert int(want[where, 0, xy[1], xy[0]]) == 1


def test_counts_maximum_contention(amd):
    """4 096 events on one pixel and one polarity, in one window"""
    ops, _ = amd
    n = 4096
    pos = np.tile(np.array([[3, 2]], np.uint16), (n, 1))
    ts = np.sort(np.random.default_rng(1).integers(100, 420, n)).astype(np.int64)
    want = _check_counts(ops, pos, ts, np.zeros(n, bool), [100, 420], 5, 7)
    assert int(want[0, 1, 2, 3]) == n and int(want.sum()) == n


def test_counts_more_events_than_one_pass_of_the_grid(amd):
    """2 048 workgroups x 256 lanes take one event each per trip of the grid-stride loop: one wave's worth more than a trip"""
    ops, _ = amd
    n = 2048 * 256 + 65
    pos, ts, pol = _events(n, 5, 7, EDGES5, 9)
    _check_counts(ops, pos, ts, pol, EDGES5, 5, 7)


@pytest.mark.parametrize("n_edges", [4095, 4096, 4097])
def test_counts_on_both_sides_of_the_lds_staging_bound(amd, n_edges):
    """V + 1 = 4 095 and 4 096 edges are searched in LDS, 4 097 in global memory"""
    ops, _ = amd
    assert ops.EVENT_FRAMES_LDS_EDGES == 4096
    g = np.random.default_rng(n_edges)
    edges = np.sort(g.integers(0, 1_000_000, n_edges)).astype(np.int64)          # irregular windows, some of them empty
    pos, ts, pol = _events(3000, 5, 7, edges, n_edges)
    want = _check_counts(ops, pos, ts, pol, edges, 5, 7)
    hit = want.sum((1, 2, 3))
    assert int((hit > 0).sum()) > 1000 and int(want.sum()) > 2500


def test_counts_sensor_size(amd):
    """346 x 260, 200 000 events, V = 8, a hot pixel"""
    ops, _ = amd
    H, W = 260, 346
    edges = np.arange(9, dtype=np.int64) * 1_000_000 + 5000
    pos, ts, pol = _events(200_000, H, W, edges, 4)
    pos[::50] = [345, 259]
    want = _check_counts(ops, pos, ts, pol, edges, H, W)
    assert int(want[:, :, 259, 345].sum()) > 3000


def test_event_frames_accepts_the_npz_arrays_and_checks_edges(amd):
    """event_frames.accumulate: numpy or torch, host or device; decreasing edges are refused"""
    from robust_e_nerf_amd import event_frames as ef
    pos, ts, pol = _events(500, 5, 7, EDGES5, 2)
    want = torch.from_numpy(ref.count_images(pos, ts, pol, EDGES5, 5, 7))
    raw = dict(position=pos, timestamp=ts, polarity=pol)
    assert torch.equal(ef.accumulate(raw, EDGES5, 5, 7).cpu(), want)
    raw_t = dict(position=torch.from_numpy(pos.astype(np.int32)).to(DEV), timestamp=dev(ts), polarity=dev(pol.astype(np.uint8)))
    assert torch.equal(ef.accumulate(raw_t, torch.tensor(EDGES5), 5, 7).cpu(), want)
    with pytest.raises(ValueError, match="non-decreasing"):
        ef.accumulate(raw, EDGES5[::-1], 5, 7)


# ------------------------------------------------------------------------------------------------------------ kernel B
@pytest.mark.parametrize("shape", [(5, 7), (75, 139), (260, 346)])
@pytest.mark.parametrize("V", [1, 3])
def test_compare_sums_match_the_float64_restatement(amd, shape, V):
    """Each of the seven sums within n_pixels x 2^-52 x sum |terms| of the correctly rounded sum of the same float64 terms --
    the bound of any summation order of n_pixels float64 terms (n - 1 additions, each within 2^-53 relative of a partial sum
    that never exceeds sum |terms|), with a factor 2 to spare; the two integer counts exact.  V = 3: window 1 has no valid
    pixel, window 2 a constant prediction.  75 x 139 and 260 x 346 end in partial tiles of 2 048 pixels."""
    ops, _ = amd
    H, W = shape
    g = np.random.default_rng(H * 31 + W + V)
    c_p, c_n = 0.31, 0.23
    counts = g.poisson(1.2, (V, 2, H, W)).astype(np.int32)
    counts[:, :, g.random((H, W)) < 0.3] = 0
    m = c_p * counts[:, 0] - c_n * counts[:, 1]
    pred = (m + 0.2 * g.standard_normal((V, H, W))).astype(np.float32)
    valid = (g.random((V, H, W)) < 0.9).astype(np.uint8)
    if V == 3:
        valid[1] = 0
        pred[2] = 0.37
    want, mags = ref.compare_sums(counts, pred, valid, c_p, c_n)
    got_d = ops.event_frame_compare(dev(counts), dev(pred), dev(valid), c_p, c_n)
    assert got_d.dtype == torch.float64 and got_d.shape == (V, 9)
    got = got_d.cpu().numpy()
    bound = H * W * 2.0 ** -52 * mags
    err = np.abs(got - want)
    print(f"{H} x {W} x {V}: largest error / bound over the seven sums {float((err[:, :7] / np.maximum(bound[:, :7], 1e-300)).max()):.3f}")
    assert np.all(err[:, :7] <= bound[:, :7]), (err, bound)
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 7:], want[:, 7:])
    if V == 3:
        assert np.all(got[1] == 0.0)
        assert got[2, 2] != 0.0
    again = ops.event_frame_compare(dev(counts), dev(pred), dev(valid.astype(bool)), c_p, c_n)
    assert torch.equal(again, got_d)                                  # fixed-order sums: bitwise repeatable
    from robust_e_nerf_amd import event_frames as ef
    sc = ef.compare(dev(counts), dev(pred), dev(valid), c_p, c_n)
    assert sc["n_valid"].tolist() == want[:, 0].astype(np.int64).tolist()
    ok = valid[0].astype(bool)
    assert abs(float(sc["corr"][0]) - float(np.corrcoef(m[0][ok], pred[0][ok].astype(np.float64))[0, 1])) < 1e-9
    if V == 3:
        assert math.isnan(float(sc["corr"][1])) and math.isnan(float(sc["corr"][2])) and math.isnan(float(sc["explained"][1]))


# ---------------------------------------------------------------------------------------------------- predicted_change
H_IMG, W_IMG = 24, 32
N_POSES = 5
EDGES_NS = [500_000, 1_500_000, 2_200_000, 3_900_000]          # three contiguous windows inside the trajectory [0, 4 ms]


def _trajectory():
    """the camera of the small scene swinging about the y axis: pose k at k ms, angle 0.1 + 0.15 k, looking at the box"""
    a = 0.1 + 0.15 * np.arange(N_POSES)
    tab_ts = torch.from_numpy((np.arange(N_POSES) * 1_000_000).astype(np.int64))
    tab_pos = torch.from_numpy(np.stack([-3.0 * np.sin(a), np.full_like(a, 0.1), -3.0 * np.cos(a)], -1).astype(np.float32))
    tab_quat = torch.from_numpy(np.stack([0 * a, np.sin(a / 2), 0 * a, np.cos(a / 2)], -1).astype(np.float32))      # XYZW
    return tab_ts, tab_pos, tab_quat


@pytest.fixture(scope="module")
def small_scene(amd):
    """a small random field (table of order 0.3: a dense, bumpy fog), occupancy grid fully on (tests/test_gpu_normals.py's
    scene), a pinhole camera of 32 x 24 pixels and a five-pose trajectory"""
    from oracle import field as ofield, hashgrid
    ops, engine = amd
    spec = hashgrid.make_spec()
    p = ofield.init_params(spec, 1, seed=3, table_kind="uniform", table_scale=0.3)
    fld = engine.NGPField(DEV)
    fld.load(p)
    cfg = engine.RenderCfg(aabb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), occ_res=(16, 16, 16), render_step_size=0.05)
    r = engine.Renderer(fld, cfg)
    r.binary.fill_(1)
    K = torch.tensor([[40.0, 0.0, W_IMG / 2], [0.0, 40.0, H_IMG / 2], [0.0, 0.0, 1.0]])
    tab_ts, tab_pos, tab_quat = _trajectory()
    return types.SimpleNamespace(r=r, fld=fld, Kinv=dev(torch.linalg.inv(K)), K=K, tab_ts=tab_ts, tab_pos=tab_pos,
                                 tab_quat=tab_quat)


@pytest.fixture(scope="module")
def prediction(amd, small_scene):
    """predicted_change of the three windows, computed once: (pred, valid, number of images rendered)"""
    from robust_e_nerf_amd import evaluation, event_frames as ef
    s = small_scene
    calls = []
    real = evaluation.render_image

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    evaluation.render_image = counting
    try:
        pred, valid = ef.predicted_change(s.r, s.Kinv, s.tab_ts, s.tab_pos, s.tab_quat, EDGES_NS, H_IMG, W_IMG)
    finally:
        evaluation.render_image = real
    return pred, valid, len(calls)


def test_predicted_change_is_the_difference_of_two_renders(amd, small_scene, prediction):
    """pred[v] == log(render_image(t_{v+1})) - log(render_image(t_v)) bit for bit at 24 x 32 for three contiguous windows, from
    exactly V + 1 = 4 renders; valid = both renders' opacity > 0 (no background colour); a repeated edge renders once"""
    from robust_e_nerf_amd import evaluation, event_frames as ef
    ops, _ = amd
    s = small_scene
    pred, valid, n_renders = prediction
    assert n_renders == len(EDGES_NS) == 4
    assert pred.shape == (3, H_IMG, W_IMG) and pred.dtype == torch.float32 and valid.shape == pred.shape and valid.dtype == torch.bool
    pos, rot = ops.trajectory(dev(torch.tensor(EDGES_NS, dtype=torch.float64)), dev(s.tab_ts), dev(s.tab_pos), dev(s.tab_quat))
    imgs = [evaluation.render_image(s.r, s.Kinv, pos[k], rot[k].contiguous(), H_IMG, W_IMG) for k in range(4)]
    for v in range(3):
        assert torch.equal(pred[v], imgs[v + 1][0].log() - imgs[v][0].log()), v
        assert torch.equal(valid[v], (imgs[v + 1][1] > 0) & (imgs[v][1] > 0)), v
    assert bool(valid.any()) and float(pred[valid].abs().max()) > 0                # the scene is seen and the camera moves
    # with a background colour every pixel is valid; an empty window (equal edges) predicts no change and renders once
    bk = torch.tensor([0.55], device=DEV)
    p2, v2 = ef.predicted_change(s.r, s.Kinv, s.tab_ts, s.tab_pos, s.tab_quat, [500_000, 500_000, 1_500_000], H_IMG, W_IMG, bkgd=bk)
    assert bool(v2.all()) and bool((p2[0] == 0).all()) and float(p2[1].abs().max()) > 0


def test_predicted_change_on_a_distorted_sensor_renders_the_undistorted_grid(amd, small_scene):
    """calib with non-zero distortion: the rays leave from data.undistort_points of the integer grid (render_pixels)"""
    from robust_e_nerf_amd import data, evaluation, event_frames as ef
    ops, _ = amd
    s = small_scene
    calib = dict(intrinsics=s.K.numpy().astype(np.float64), distortion_params=np.array([-0.05, 0.01, 0.001, -0.002]),
                 distortion_model="plumb_bob")
    bk = torch.tensor([0.55], device=DEV)
    pred, valid = ef.predicted_change(s.r, s.Kinv, s.tab_ts, s.tab_pos, s.tab_quat, EDGES_NS[:2], H_IMG, W_IMG, bkgd=bk, calib=calib)
    grid = evaluation.pixel_grid(H_IMG, W_IMG, "cpu").reshape(-1, 2).numpy().astype(np.float64)
    px = dev(torch.from_numpy(data.undistort_points(grid, calib["intrinsics"], calib["distortion_params"], "plumb_bob").astype(np.float32)))
    pos, rot = ops.trajectory(dev(torch.tensor(EDGES_NS[:2], dtype=torch.float64)), dev(s.tab_ts), dev(s.tab_pos), dev(s.tab_quat))
    n = px.shape[0]
    logs = [evaluation.render_pixels(s.r, s.Kinv, px, pos[k].expand(n, 3).contiguous(), rot[k].expand(n, 3, 3).contiguous(), bk)[0].log()
            for k in range(2)]
    assert torch.equal(pred[0].reshape(-1), logs[1] - logs[0]) and bool(valid.all())
    plain, _ = ef.predicted_change(s.r, s.Kinv, s.tab_ts, s.tab_pos, s.tab_quat, EDGES_NS[:2], H_IMG, W_IMG, bkgd=bk)
    assert not torch.equal(plain, pred)


# --------------------------------------------------------------------------------------------------------- closed loop
def test_closed_loop_prediction_to_events_to_comparison(amd, prediction):
    """No simulator: the prediction itself is turned into counts n = trunc(pred / C) per pixel (c_p = c_n = C), the counts into
    an event list with timestamps inside each window, the list is accumulated and compared.  Then m = C n differs from p by
    less than C on every valid pixel, so explained == 1.0 exactly; corr > 0.9 is a sanity condition, not a measurement."""
    from robust_e_nerf_amd import event_frames as ef
    pred, valid, _ = prediction
    V = pred.shape[0]
    C = float(pred[valid].abs().double().median()) / 2.5             # most valid pixels get a few events
    assert C > 0
    n = torch.where(valid, torch.trunc(pred.double() / C), torch.zeros_like(pred, dtype=torch.float64)).to(torch.int64).cpu()
    assert float((n[valid.cpu()] != 0).double().mean()) > 0.5 and int(n.abs().sum()) < 2_000_000
    edges = torch.tensor(EDGES_NS)
    v_i, y_i, x_i = torch.nonzero(n, as_tuple=True)
    reps = n[v_i, y_i, x_i].abs()
    first = torch.cumsum(reps, 0) - reps
    j = torch.arange(int(reps.sum())) - torch.repeat_interleave(first, reps)              # 0 .. |n| - 1 within a pixel's events
    v_e, y_e, x_e, k_e = (torch.repeat_interleave(a, reps) for a in (v_i, y_i, x_i, reps))
    length = (edges[1:] - edges[:-1])[v_e]
    ts = edges[v_e] + (j * length) // k_e                                                   # in [edges[v], edges[v + 1])
    assert bool((ts >= edges[v_e]).all()) and bool((ts < edges[v_e + 1]).all())
    order = torch.argsort(ts, stable=True)
    raw = dict(position=torch.stack([x_e, y_e], -1)[order].numpy().astype(np.uint16), timestamp=ts[order].numpy(),
               polarity=(torch.repeat_interleave(n[v_i, y_i, x_i], reps) > 0)[order].numpy())
    counts = ef.accumulate(raw, edges, H_IMG, W_IMG)
    assert torch.equal((counts[:, 0] - counts[:, 1]).cpu().long(), n) and int(counts.sum()) == int(reps.sum())
    sc = ef.compare(counts, pred, valid, C, C)
    m64 = C * (counts[:, 0] - counts[:, 1]).double()
    assert bool(((pred.double() - m64).abs() < C)[valid].all())
    print("closed loop: C", C, "events", int(reps.sum()), "corr", sc["corr"].tolist(), "rmse/C", sc["rmse_over_c"].tolist())
    assert sc["n_valid"].tolist() == valid.sum((1, 2)).tolist()
    assert all(float(e) == 1.0 for e in sc["explained"]) and sc["mean_explained"] == 1.0
    assert all(float(c) > 0.9 for c in sc["corr"])
    assert torch.equal(ef.measured_change(counts, C, C), m64.float())
    img = ef.frame_png(ef.measured_change(counts, C, C)[0], pred[0], valid[0], C)
    assert img.shape == (H_IMG, 3 * W_IMG, 3) and bool((img[:, :W_IMG][~valid[0].cpu()] == 128).all())


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_writes_the_pictures_and_the_npz(amd, tmp_path):
    """scripts/event_frames.py on a tiny dataset in the reference's layout and a checkpoint in its state-dict format"""
    import yaml
    from PIL import Image
    from robust_e_nerf_amd import checkpoint, config, engine
    root, out = os.path.join(tmp_path, "dataset"), os.path.join(tmp_path, "out")
    os.makedirs(root)
    tab_ts, tab_pos, tab_quat = _trajectory()
    K = np.array([[40.0, 0.0, W_IMG / 2], [0.0, 40.0, H_IMG / 2], [0.0, 0.0, 1.0]])
    edges = [0, 1_333_333, 2_666_666, 4_000_000]                      # window_edges(0, 4 ms, 3)
    pos, ts, pol = _events(3000, H_IMG, W_IMG, edges, 12, outside=False)
    np.savez(os.path.join(root, "raw_events.npz"), position=pos, timestamp=ts, polarity=pol)
    np.savez(os.path.join(root, "camera_poses.npz"), T_wc_timestamp=tab_ts.numpy(), T_wc_position=tab_pos.numpy(),
             T_wc_orientation=tab_quat.numpy())
    np.savez(os.path.join(root, "camera_calibration.npz"), intrinsics=K, img_width=W_IMG, img_height=H_IMG,
             distortion_params=np.zeros(4), distortion_model="plumb_bob", bayer_pattern="", pos_contrast_threshold=0.25,
             neg_contrast_threshold=0.2, refractory_period=0.0)
    cfg = yaml.safe_load(open(os.path.join(REPO, "configs", "synthetic_smoke.yaml")))
    cfg["model"]["nerf"]["occ_grid"]["resolution"] = 16
    cfg_path = os.path.join(tmp_path, "cfg.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    ncfg = cfg["model"]["nerf"]
    rcfg = config.render_cfg(cfg, tab_pos)
    fld, r = config.make_renderer(ncfg, rcfg, 1, DEV)
    config.init_field(fld, "ngp", 1, torch.Generator().manual_seed(0))
    sd = checkpoint.field_state_dict(fld, "ngp", rcfg.aabb)
    sd[checkpoint.OCC + "_binary"] = torch.ones(16, 16, 16, dtype=torch.bool)
    sd[checkpoint.CT_KEY] = torch.tensor([0.5])
    sd[checkpoint.BKGD_KEY] = torch.tensor([0.3])
    ckpt = os.path.join(tmp_path, "model.ckpt")
    torch.save({"state_dict": sd}, ckpt)
    run = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "event_frames.py"), "--config", cfg_path, "--ckpt", ckpt,
                          "--dataset-dir", root, "--out", out, "--windows", "3"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len([l for l in lines if l.startswith("window ")]) == 3 and len([l for l in lines if l.startswith("mean:")]) == 1
    assert sorted(os.listdir(os.path.join(out, "event_frames"))) == ["0.png", "1.png", "2.png"]
    im = Image.open(os.path.join(out, "event_frames", "1.png"))
    assert im.mode == "RGB" and im.size == (3 * W_IMG, H_IMG)
    z = np.load(os.path.join(out, "event_frames.npz"))
    assert {"edges", "counts", "predicted", "valid", "scores", "score_columns", "sums", "c_p", "c_n"} <= set(z.files)
    assert z["edges"].tolist() == edges
    assert np.array_equal(z["counts"], ref.count_images(pos, ts, pol, edges, H_IMG, W_IMG))
    assert z["predicted"].shape == (3, H_IMG, W_IMG) and z["valid"].shape == (3, H_IMG, W_IMG) and z["valid"].all()
    assert z["scores"].shape == (3, 5) and list(z["score_columns"]) == ["n_valid", "n_active", "corr", "rmse_over_c", "explained"]
    assert z["scores"][:, 0].tolist() == [H_IMG * W_IMG] * 3
    assert abs(float(z["c_n"]) - 0.2) < 1e-12 and abs(float(z["c_p"]) - math.log1p(math.exp(0.5)) * 0.2) < 1e-6
    want, _ = ref.compare_sums(z["counts"], z["predicted"], z["valid"], float(z["c_p"]), float(z["c_n"]))
    assert np.array_equal(z["sums"][:, [0, 7, 8]], want[:, [0, 7, 8]])
