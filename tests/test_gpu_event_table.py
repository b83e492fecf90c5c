"""GPU: the event table built on the device (csrc/ren_event_table.hip, data.build_event_table / load_event_table) against the
host functions it replaces at start-up: undistort_events(colorize_events(queue_raw_events(..., device=None))) and
max_refractory_period.  Integer arithmetic and a table gather only: every comparison is torch.equal plus the dtype."""
import os

import numpy as np
import pytest
import torch

from robust_e_nerf_amd import data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 2, 63, 64, 65, 257, 1000, 4099]
DIST = {"plumb_bob": np.array([-0.35, 0.12, 0.004, -0.003]), "equidistant": np.array([-0.08, 0.05, -0.02, 0.006])}


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops


def calibration(W, H, model=None, bayer=""):
    f = 0.8 * W
    K = np.array([[f, 0.0, W / 2 - 0.4], [0.0, 1.03 * f, H / 2 - 0.3], [0.0, 0.0, 1.0]])
    return dict(intrinsics=K, img_width=np.uint16(W), img_height=np.uint16(H), distortion_model=np.array(model or "plumb_bob"),
                distortion_params=np.zeros(0) if model is None else DIST[model], bayer_pattern=np.array(bayer))


def stream(n, W, H, seed, rows=None, span=3):
    """n time-ordered events; timestamps drawn from span * n values, so some repeat (also on one pixel); rows: confine y"""
    g = np.random.default_rng(seed)
    y = g.integers(0, H, n) if rows is None else g.integers(H - rows, H, n)
    pos = np.stack([g.integers(0, W, n), y], -1).astype(np.uint16)
    ts = np.sort(g.integers(0, span * n + 1, n)).astype(np.int64)
    return pos, ts, g.random(n) < 0.5


def reference(pos, ts, pol, calib):
    W = int(calib["img_width"])
    ev = data.queue_raw_events(pos, ts, pol, W, device=None)
    ev = data.undistort_events(data.colorize_events(ev, str(calib["bayer_pattern"])), calib)
    return ev, data.max_refractory_period(pos, ts, W)


def same_table(got, want, on_device=True):
    assert list(got) == list(want)
    for k in want:
        assert got[k].is_cuda == on_device, k
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, tuple(got[k].shape))
        assert torch.equal(got[k].cpu(), want[k]), f"{k}: {int((got[k].cpu() != want[k]).sum())} values differ"


def check(pos, ts, pol, calib):
    want, want_tau = reference(pos, ts, pol, calib)
    assert not torch.isnan(want["position"]).any()
    got, tau = data.build_event_table(pos, ts, pol, calib, DEV)
    same_table(got, want)
    assert tau.dtype == torch.float64 and tau.dim() == 0 and not tau.is_cuda and torch.equal(tau, want_tau), (tau, want_tau)
    return want, want_tau


# ------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", SIZES)
def test_small_sensor_every_size(amd, n):
    """5 x 3 pixels: nearly every event has a predecessor and the runs of a pixel cross wave and workgroup boundaries;
    the calibration and the Bayer pattern change with the size"""
    i = SIZES.index(n)
    calib = calibration(5, 3, [None, "plumb_bob", "equidistant"][i % 3], ["", "RGGB", "BGGR"][(i // 3) % 3])
    want, _ = check(*stream(n, 5, 3, n), calib)
    if n >= 63:
        assert n - 15 - n // 4 < len(want["position"]) < n


@pytest.mark.parametrize("n", SIZES)
def test_large_keys_every_size(amd, n):
    """1280 x 720 with the events in the last two rows: keys up to 921 599"""
    want, _ = check(*stream(n, 1280, 720, n + 1, rows=2), calibration(1280, 720))
    if n == 4099:
        assert len(want["position"]) > 1000


def test_large_sensor_with_a_lookup_table(amd):
    check(*stream(4099, 1280, 720, 3, rows=2), calibration(1280, 720, "equidistant", "RGGB"))


def test_more_events_than_one_pass_of_the_grid(amd):
    """2 048 workgroups take one event per lane per trip of the grid-stride loops: one wave's worth more than a trip"""
    n = 2048 * amd.EVENT_TABLE_THREADS + 65
    check(*stream(n, 5, 3, 11), calibration(5, 3, "plumb_bob", "BGGR"))


# ------------------------------------------------------------------------------------------------------------ streams
def test_all_events_on_one_pixel(amd):
    n = 257
    pos = np.tile(np.array([[3, 1]], np.uint16), (n, 1))
    ts = (np.arange(n, dtype=np.int64) * 7 + 5)
    want, tau = check(pos, ts, np.arange(n) % 3 == 0, calibration(5, 3, "equidistant", "RGGB"))
    assert len(want["position"]) == n - 1 and float(tau) == 7.0


@pytest.mark.parametrize("sensor", [(5, 3), (37, 23)])
def test_all_events_on_distinct_pixels(amd, sensor):
    """no event has a predecessor: M = 0, tau_max = inf, empty tensors of the table's dtypes (37 x 23: three workgroups)"""
    W, H = sensor
    pix = np.random.default_rng(0).permutation(W * H)
    pos = np.stack([pix % W, pix // W], -1).astype(np.uint16)
    want, tau = check(pos, np.arange(W * H, dtype=np.int64), np.ones(W * H, bool), calibration(W, H, "plumb_bob", "RGGB"))
    assert len(want["position"]) == 0 and float(tau) == float("inf")
    got, _ = data.build_event_table(pos, np.arange(W * H, dtype=np.int64), np.ones(W * H, bool), calibration(W, H), DEV)
    assert got["position"].shape == (0, 2) and got["position"].dtype == torch.float32 and "channel_idx" not in got
    assert all(got[k].dtype == torch.int64 and got[k].shape == (0,) for k in ("start_ts", "end_ts", "num_pos", "num_neg"))


def test_equal_timestamps_first_middle_last(amd):
    """one pixel fires at 10, 10, 20, 30, 30, 40, 50, 50 between events of other pixels: the repeats are dropped, and the
    dropped 30 is still the predecessor of 40 (start 30)"""
    mine = np.array([10, 10, 20, 30, 30, 40, 50, 50], np.int64)
    other = np.array([5, 15, 25, 35, 45, 55], np.int64)
    ts = np.concatenate([mine, other])
    pos = np.concatenate([np.tile([[2, 1]], (8, 1)), np.tile([[4, 2]], (6, 1))]).astype(np.uint16)
    o = np.argsort(ts, kind="stable")
    pos, ts = pos[o], ts[o]
    want, tau = check(pos, ts, np.ones(14, bool), calibration(5, 3))
    on = (want["position"] == torch.tensor([2.0, 1.0])).all(1)
    assert want["start_ts"][on].tolist() == [10, 20, 30, 40] and want["end_ts"][on].tolist() == [20, 30, 40, 50]
    assert float(tau) == 10.0


def test_timestamps_above_2_pow_40_with_differences_above_2_pow_32(amd):
    n = 1000
    g = np.random.default_rng(4)
    ts = (2 ** 41 + np.cumsum(g.integers(2 ** 32 + 1, 2 ** 34, n))).astype(np.int64)
    pos, _, pol = stream(n, 5, 3, 4)
    want, tau = check(pos, ts, pol, calibration(5, 3, None, "BGGR"))
    assert int(want["start_ts"].min()) > 2 ** 40 and float(tau) > 2 ** 32


def test_minimum_in_every_part_of_the_reduction(amd):
    """one pixel, so sorted slot = stream index; every interval is 1000 but one of 7.  Slot 0 has no predecessor, so slot 1
    is the first of the first workgroup that holds an interval; then the last slot of a full workgroup, the first of the
    next (its predecessor belongs to another workgroup), and slots of the final, partial workgroup"""
    T = amd.EVENT_TABLE_THREADS
    n = 3 * T + 17
    pos = np.tile(np.array([[1, 2]], np.uint16), (n, 1))
    calib = calibration(5, 3)
    for slot in (1, T - 1, T, 2 * T - 1, 3 * T, 3 * T + 8, n - 1):
        d = np.full(n, 1000, np.int64)
        d[slot] = 7
        ts = np.cumsum(d)
        table, tau = data.build_event_table(pos, ts, np.ones(n, bool), calib, DEV)
        assert float(tau) == 7.0 and torch.equal(tau, data.max_refractory_period(pos, ts, 5)), slot
        assert len(table["start_ts"]) == n - 1 and int(table["end_ts"][slot - 1] - table["start_ts"][slot - 1]) == 7


# ------------------------------------------------------------------------------------------------------------ sensors and storage
@pytest.mark.parametrize("bayer", ["", "RGGB", "BGGR"])
@pytest.mark.parametrize("model", [None, "plumb_bob", "equidistant"])
def test_bayer_patterns_and_distortion_models(amd, bayer, model):
    want, _ = check(*stream(1000, 37, 23, 6), calibration(37, 23, model, bayer))
    assert ("channel_idx" in want) == (bayer != "")
    if model is not None:
        assert not torch.equal(want["position"], want["position"].round())


@pytest.mark.parametrize("pol_dtype", [bool, np.uint8])
@pytest.mark.parametrize("pos_dtype", [np.uint16, np.int32, np.int64, np.int16])
def test_positions_and_polarity_as_stored(amd, pos_dtype, pol_dtype):
    """uint16 / int32 / int64 coordinates go to the kernel at their stored width, other integer widths as int32"""
    pos, ts, pol = stream(1000, 37, 23, 8)
    check(pos.astype(pos_dtype), ts, pol.astype(pol_dtype), calibration(37, 23, "equidistant", "RGGB"))


def test_two_builds_are_equal(amd):
    pos, ts, pol = stream(4099, 37, 23, 9)
    calib = calibration(37, 23, "equidistant", "BGGR")
    (a, tau_a), (b, tau_b) = (data.build_event_table(pos, ts, pol, calib, DEV) for _ in range(2))
    same_table(b, {k: v.cpu() for k, v in a.items()})
    assert torch.equal(tau_a, tau_b)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_dataset_directory_caches_and_batches(amd, tmp_path):
    """a dataset directory (4 099 events, 37 x 23, equidistant, RGGB): load_event_table == load_events +
    load_max_refractory_period with and without the permutation; both caches appear in the forms those functions read; with
    raw_events.npz gone the caches give the same table; EventBatcher draws the same first batch from the device table"""
    root = str(tmp_path)
    W, H = 37, 23
    pos, ts, pol = stream(4099, W, H, 10)
    np.savez(os.path.join(root, data.RAW_EVENTS), position=pos, timestamp=ts, polarity=pol)
    np.savez(os.path.join(root, data.CAMERA_CALIBRATION), **calibration(W, H, "equidistant", "RGGB"))
    want = {seed: data.load_events(root, seed, use_cache=False, device=None) for seed in (None, 5)}
    want_tau = data.load_max_refractory_period(root)
    assert sorted(os.listdir(root)) == sorted([data.RAW_EVENTS, data.CAMERA_CALIBRATION])

    got, tau = data.load_event_table(root, device=DEV)
    same_table(got, want[None])
    assert tau.dtype == torch.float64 and torch.equal(tau, want_tau)
    assert os.path.isfile(os.path.join(root, data.TF_EVENTS)) and os.path.isfile(os.path.join(root, data.MAX_REFRACTORY_PERIOD))
    same_table(data.load_events(root), want[None], on_device=False)                     # events.pt as load_events reads it
    assert torch.equal(data.load_max_refractory_period(root), want_tau)
    os.remove(os.path.join(root, data.TF_EVENTS))
    os.remove(os.path.join(root, data.MAX_REFRACTORY_PERIOD))
    same_table(data.load_event_table(root, 5, device=DEV)[0], want[5])                  # built, then permuted on the device

    os.remove(os.path.join(root, data.RAW_EVENTS))
    for seed in (None, 5):
        again, tau2 = data.load_event_table(root, seed, device=DEV)
        same_table(again, want[seed])
        assert torch.equal(tau2, want_tau)

    a = data.EventBatcher(got, 64, DEV, seed=3).next()
    b = data.EventBatcher(want[None], 64, DEV, seed=3).next()
    assert list(a) == list(b)
    for k in b:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
