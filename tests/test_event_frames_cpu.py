"""CPU: the numpy restatements the event-frame kernels are held to (tests/event_frames_reference.py) against the literal
definition, the host side of robust_e_nerf_amd.event_frames (window arithmetic, derived scores, the picture), the C-ABI entry
points of csrc/ren_event_frames.hip (declared, exported, bound, argument validation before any launch) and the CLI's --help."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import event_frames_reference as ref


def _stream(n, H, W, edges, seed):
    """a few hundred time-ordered events: some exactly on every edge, some before the first / at and after the last edge,
    some outside the image"""
    g = np.random.default_rng(seed)
    lo, hi = int(edges[0]) - 50, int(edges[-1]) + 50
    ts = g.integers(lo, hi, n).astype(np.int64)
    on_edge = g.choice(n, size=3 * len(edges), replace=False)
    ts[on_edge] = np.tile(np.asarray(edges, np.int64), 3)
    ts.sort()
    pos = np.stack([g.integers(0, W, n), g.integers(0, H, n)], -1).astype(np.uint16)
    pos[g.choice(n, 6, replace=False)] = [[W, 0], [0, H], [W + 3, H + 1], [65535, 0], [0, 65535], [W, H]]
    return pos, ts, g.random(n) < 0.5


def test_restatement_equals_the_literal_definition():
    H, W = 5, 7
    edges = np.array([100, 180, 180, 260, 300, 420], np.int64)            # window 1 is empty by construction (equal edges)
    pos, ts, pol = _stream(400, H, W, edges, 0)
    assert (ts < edges[0]).any() and (ts >= edges[-1]).any() and (ts == edges[-1]).any() and (ts == edges[2]).any()
    got = ref.count_images(pos, ts, pol, edges, H, W)
    want = ref.count_images_loop(pos, ts, pol, edges, H, W)
    assert got.dtype == np.int32 and got.shape == (5, 2, H, W)
    assert np.array_equal(got, want)
    assert got[1].sum() == 0 and got[0].sum() > 0 and got[2].sum() > 0
    inside = (ts >= edges[0]) & (ts < edges[-1]) & (pos[:, 0] < W) & (pos[:, 1] < H)
    assert got.sum() == inside.sum() and got[:, 0].sum() == (inside & pol).sum()
    # an event exactly on an interior edge opens the later window; a window nothing falls into stays zero
    one = ref.count_images(np.array([[2, 3]], np.uint16), np.array([260]), np.array([True]), edges, H, W)
    assert one[3, 0, 3, 2] == 1 and one.sum() == 1
    far = ref.count_images(pos, ts, pol, np.array([1000, 2000, 3000]), H, W)
    assert far.sum() == 0


def test_compare_restatement_on_a_hand_made_window():
    counts = np.zeros((1, 2, 1, 4), np.int32)
    counts[0, 0, 0] = [2, 0, 1, 5]
    counts[0, 1, 0] = [0, 1, 1, 0]
    pred = np.array([[[0.5, -0.2, 0.0, 9.0]]], np.float32)
    valid = np.array([[[1, 1, 1, 0]]], np.uint8)
    sums, mags = ref.compare_sums(counts, pred, valid, 0.25, 0.2)
    m = [0.5, -0.2, 0.25 - 0.2]
    p = [0.5, float(np.float32(-0.2)), 0.0]
    want = [3, sum(m), sum(p), sum(a * a for a in m), sum(b * b for b in p), sum(a * b for a, b in zip(m, p)),
            sum((b - a) ** 2 for a, b in zip(m, p)), 3, 3]
    assert sums.shape == (1, 9) and np.allclose(sums[0], want, rtol=0, atol=1e-15)
    assert np.all(mags >= np.abs(sums))


def test_window_edges():
    from robust_e_nerf_amd import event_frames as ef
    e = ef.window_edges(1000, 2000, n_windows=4)
    assert e.dtype == torch.int64 and e.tolist() == [1000, 1250, 1500, 1750, 2000]
    assert ef.window_edges(0, 10, n_windows=3).tolist() == [0, 3, 6, 10]                  # floor division, ends on t_last
    assert ef.window_edges(1000, 2000, window_ns=300).tolist() == [1000, 1300, 1600, 1900]  # whole windows that fit
    assert ef.window_edges(1000, 2000, window_ns=300, start_ns=1100).tolist() == [1100, 1400, 1700, 2000]
    assert ef.window_edges(1000, 2000, n_windows=2, window_ns=100, start_ns=1500).tolist() == [1500, 1600, 1700]
    assert ef.window_edges(5, 2 ** 40, n_windows=1).tolist() == [5, 2 ** 40]
    for kw in (dict(), dict(n_windows=0), dict(window_ns=0), dict(window_ns=2000), dict(n_windows=4, window_ns=300),
               dict(n_windows=2, start_ns=999), dict(n_windows=2, start_ns=2000)):
        with pytest.raises(ValueError):
            ef.window_edges(1000, 2000, **kw)


def test_accumulate_refuses_decreasing_edges_before_touching_the_device():
    from robust_e_nerf_amd import event_frames as ef
    raw = dict(position=np.zeros((1, 2), np.uint16), timestamp=np.zeros(1, np.int64), polarity=np.ones(1, bool))
    with pytest.raises(ValueError, match="non-decreasing"):
        ef.accumulate(raw, [0, 10, 5], 4, 4)
    with pytest.raises(ValueError):
        ef.accumulate(raw, [0], 4, 4)
    # the words the kernel reads: x in the low half, y in the high half, for uint16 and for wider integer arrays alike
    pos = np.array([[3, 1], [65535, 2], [0, 65535]], np.uint16)
    want = [3 | 1 << 16, 65535 | 2 << 16, np.int32(-65536)]
    assert ef._position_words(pos).tolist() == [int(w) for w in want]
    assert ef._position_words(torch.from_numpy(pos.astype(np.int64))).tolist() == [int(w) for w in want]
    with pytest.raises(ValueError):
        ef._position_words(np.array([[70000, 0]]))


def test_measured_change_and_bayer_channels():
    from robust_e_nerf_amd import event_frames as ef
    counts = torch.zeros(1, 2, 2, 2, dtype=torch.int32)
    counts[0, 0, 0, 0], counts[0, 1, 0, 1], counts[0, 0, 1, 1], counts[0, 1, 1, 1] = 3, 2, 1, 1
    m = ef.measured_change(counts, 0.3, 0.2)
    assert m.dtype == torch.float32 and m.shape == (1, 2, 2)
    assert torch.equal(m, torch.tensor([[[0.9, -0.4], [0.0, 0.3 - 0.2]]], dtype=torch.float64).float())
    from robust_e_nerf_amd import data
    chan = ef.bayer_channels(4, 6, "RGGB", "cpu")
    ev = data.colorize_events({"position": torch.tensor([[x, y] for y in range(4) for x in range(6)])}, "RGGB")
    assert torch.equal(chan.reshape(-1), ev["channel_idx"].long())


def test_scores_follow_from_the_sums():
    from robust_e_nerf_amd import event_frames as ef
    c_p, c_n = 0.3, 0.2
    m = np.array([0.3, -0.2, 0.6, 0.0, 0.1])
    p = np.array([0.25, -0.1, 0.2, 0.05, 0.1])

    def row(m, p, n_expl, n_act):
        return [len(m), m.sum(), p.sum(), (m * m).sum(), (p * p).sum(), (m * p).sum(), ((p - m) ** 2).sum(), n_expl, n_act]
    const = np.full(5, 0.7)
    sums = torch.tensor([row(m, p, 4, 4),
                         [0] * 9,                                        # no valid pixel
                         row(m, const, 2, 4),                            # constant prediction: no variance
                         row(np.zeros(5), p, 5, 0),                      # no event at all: measured change constant
                         row(m, m, 5, 4)], dtype=torch.float64)
    sc = ef.scores_from_sums(sums, c_p, c_n)
    assert sc["n_valid"].tolist() == [5, 0, 5, 5, 5] and sc["n_active"].tolist() == [4, 0, 4, 0, 4]
    assert sc["n_valid"].dtype == torch.int64
    assert abs(float(sc["corr"][0]) - float(np.corrcoef(m, p)[0, 1])) < 1e-12
    assert abs(float(sc["rmse_over_c"][0]) - math.sqrt(((p - m) ** 2).mean()) / 0.25) < 1e-12
    assert float(sc["explained"][0]) == 0.8
    assert all(math.isnan(float(sc[k][1])) for k in ("corr", "rmse_over_c", "explained"))
    assert math.isnan(float(sc["corr"][2])) and math.isnan(float(sc["corr"][3]))
    assert float(sc["explained"][2]) == 0.4 and float(sc["explained"][3]) == 1.0
    assert abs(float(sc["corr"][4]) - 1.0) < 1e-12 and float(sc["rmse_over_c"][4]) == 0.0
    # means: over the windows that have valid pixels; windows without a defined correlation do not enter mean_corr
    assert abs(sc["mean_explained"] - (0.8 + 0.4 + 1.0 + 1.0) / 4) < 1e-15
    assert abs(sc["mean_corr"] - (float(sc["corr"][0]) + float(sc["corr"][4])) / 2) < 1e-15
    rm = [float(sc["rmse_over_c"][i]) for i in (0, 2, 3, 4)]
    assert abs(sc["mean_rmse_over_c"] - sum(rm) / 4) < 1e-15
    empty = ef.scores_from_sums(torch.zeros(2, 9, dtype=torch.float64), c_p, c_n)
    assert math.isnan(empty["mean_corr"]) and math.isnan(empty["mean_explained"])


def test_frame_png():
    from robust_e_nerf_amd import event_frames as ef
    H, W, c = 4, 5, 0.25
    m = torch.zeros(H, W)
    p = torch.zeros(H, W)
    m[0, 0], m[0, 1], m[0, 2], m[0, 3] = 4 * c, -4 * c, 2 * c, 100.0
    p[0, 0], p[1, 0] = 4 * c, -2 * c
    valid = torch.ones(H, W, dtype=torch.bool)
    valid[3, 4] = False
    valid[0, 3] = False
    img = ef.frame_png(m, p, valid, c)
    assert img.dtype == torch.uint8 and img.shape == (H, 3 * W, 3) and img.device.type == "cpu"
    px = lambda panel, y, x: img[y, panel * W + x].tolist()
    assert px(0, 0, 0) == [255, 0, 0] and px(0, 0, 1) == [0, 0, 255]            # +- 4 mean thresholds: full red / full blue
    assert px(0, 0, 2) == [255, 128, 128] and px(1, 1, 0) == [128, 128, 255]    # half way
    assert px(0, 2, 2) == [255, 255, 255] and px(2, 0, 0) == [255, 255, 255]    # no change | zero residual: white
    assert px(2, 1, 0) == [128, 128, 255]                                       # residual = predicted - measured
    for panel in range(3):                                                      # invalid pixels: grey, whatever the value
        assert px(panel, 3, 4) == [128, 128, 128] and px(panel, 0, 3) == [128, 128, 128]
    assert torch.equal(ef.frame_png(m, p, valid.to(torch.uint8), 2 * c, span=2.0), img)   # the range is span x c_mean
    with pytest.raises(ValueError):
        ef.frame_png(m, p[:2], valid, c)


def test_cli_help():
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "event_frames.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ("--config", "--ckpt", "--dataset-dir", "--out", "--windows", "--window-ms", "--start-ms", "--height", "--width"):
        assert flag in out.stdout, flag


@pytest.fixture(scope="module")
def lib():
    from robust_e_nerf_amd import build
    build.build()
    from robust_e_nerf_amd import _lib
    return _lib.load()


NEW_SYMBOLS = ("ren_event_frames", "ren_event_frame_compare", "ren_event_frame_compare_scratch_doubles")


def test_entry_points_are_declared_exported_and_bound(lib):
    from robust_e_nerf_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "ren_event_frames.hip" in build.SOURCES
    assert f"#define REN_EVENT_FRAMES_LDS_EDGES {ops.EVENT_FRAMES_LDS_EDGES}\n" in hdr
    assert f"#define REN_EVENT_FRAMES_MERGE {ops.EVENT_FRAMES_MERGE}\n" in hdr
    assert lib.ren_abi_version() == 25
    # nine doubles per tile of 2048 pixels of every window; nothing for a shape without pixels or windows
    assert lib.ren_event_frame_compare_scratch_doubles(1, 5, 7) == 9
    assert lib.ren_event_frame_compare_scratch_doubles(3, 32, 64) == 3 * 9
    assert lib.ren_event_frame_compare_scratch_doubles(3, 32, 65) == 3 * 2 * 9
    assert lib.ren_event_frame_compare_scratch_doubles(64, 260, 346) == 64 * 44 * 9
    for bad in ((0, 5, 7), (-1, 5, 7), (1, 0, 7), (1, 5, 0), (1, -5, -7)):
        assert lib.ren_event_frame_compare_scratch_doubles(*bad) == 0, bad


def test_argument_validation_needs_no_gpu(lib):
    """REN_ERR_BAD_ARG is returned before any launch: host buffers stand in for device memory and are never touched"""
    from robust_e_nerf_amd import _lib, ops
    buf = (ctypes.c_double * 64)()
    fp = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(pos=fp, ts=fp, pol=fp, N=4, edges=fp, V=1, H=2, W=2, flags=0, counts=fp)

    def frames(**kw):
        a = dict(good, **kw)
        return lib.ren_event_frames(a["pos"], a["ts"], a["pol"], a["N"], a["edges"], a["V"], a["H"], a["W"], a["flags"],
                                    a["counts"], None)
    for kw in (dict(pos=None), dict(ts=None), dict(pol=None), dict(edges=None), dict(counts=None), dict(N=-1), dict(V=0),
               dict(V=-2), dict(H=0), dict(W=0), dict(H=-1), dict(flags=2), dict(flags=-1), dict(N=0, edges=None),
               dict(N=0, counts=None), dict(N=0, V=0)):
        assert frames(**kw) == _lib.REN_ERR_BAD_ARG, kw
    assert frames(N=0) == _lib.REN_OK and frames(N=0, pos=None, ts=None, pol=None) == _lib.REN_OK     # nothing to launch
    assert all(v == 0.0 for v in buf)
    gc = dict(counts=fp, pred=fp, valid=fp, V=1, H=2, W=2, c_p=0.25, c_n=0.25, out=fp, scratch=fp)

    def compare(**kw):
        a = dict(gc, **kw)
        return lib.ren_event_frame_compare(a["counts"], a["pred"], a["valid"], a["V"], a["H"], a["W"], a["c_p"], a["c_n"],
                                           a["out"], a["scratch"], None)
    for kw in (dict(counts=None), dict(pred=None), dict(valid=None), dict(out=None), dict(scratch=None), dict(V=0), dict(H=0),
               dict(W=0), dict(W=-3), dict(c_p=math.nan), dict(c_n=math.inf)):
        assert compare(**kw) == _lib.REN_ERR_BAD_ARG, kw
    with pytest.raises(ValueError):                                   # no CPU fallback on the product path
        ops.event_frames(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.bool),
                         torch.tensor([0, 1]), 2, 2)
    with pytest.raises(ValueError):
        ops.event_frame_compare(torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.zeros(1, 2, 2), torch.ones(1, 2, 2, dtype=torch.bool),
                                0.25, 0.25)
