"""CPU: the event noise filter's definition and host side.  The numpy reference the GPU tests use (event_filter_reference) against
a literal double loop over the definition; data.hot_pixel_threshold against numpy's mean / std; the refusals of
data.filter_events and ops.event_support, which fire before anything reaches a device; the argument validation of
ren_event_support, which returns before any launch; load_event_table's default path, which never calls the filter."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from event_filter_reference import STATS, filter_reference
from robust_e_nerf_amd import data

W, H = 5, 4


def calibration(w=W, h=H):
    return dict(intrinsics=np.eye(3), img_width=np.uint16(w), img_height=np.uint16(h), distortion_model=np.array("plumb_bob"),
                distortion_params=np.zeros(0), bayer_pattern=np.array(""))


def literal(x, y, t, hot, dt, include_self):
    """the definition, event by event against every other event"""
    n = len(t)
    keep = np.zeros(n, bool)
    for e in range(n):
        if hot[y[e] * W + x[e]]:
            continue
        ok = dt is None
        for o in range(n):
            if ok:
                break
            if o == e or max(abs(int(x[e]) - int(x[o])), abs(int(y[e]) - int(y[o]))) > 1 or hot[y[o] * W + x[o]]:
                continue
            if (x[o], y[o]) == (x[e], y[e]) and not include_self:
                continue
            ok = 0 <= int(t[e]) - int(t[o]) <= dt
        keep[e] = ok
    return keep


def small_stream(seed, n=300):
    """300 events on 5 x 4 over 2 400 time units, time-ordered with repeats; pixel (2, 1) takes a third of them"""
    g = np.random.default_rng(seed)
    x, y = g.integers(0, W, n), g.integers(0, H, n)
    burst = g.random(n) < 1 / 3
    x[burst], y[burst] = 2, 1
    return x, y, np.sort(g.integers(0, 8 * n, n))


@pytest.mark.parametrize("dt", [0, 3, 50])
@pytest.mark.parametrize("include_self", [False, True])
def test_reference_is_the_definition(include_self, dt):
    for seed, k in ((0, 2.0), (1, None)):
        x, y, t = small_stream(seed)
        keep, stats = filter_reference(x, y, t, W, H, dt, k, include_self)
        counts = np.bincount(y * W + x, minlength=H * W)
        c = counts[counts > 0]
        hot = np.zeros(H * W, bool) if k is None else counts > math.floor(c.mean() + k * c.std())
        assert hot.sum() == (0 if k is None else 1) and stats["hot_pixels"] == hot.sum()
        want = literal(x, y, t, hot, dt, include_self)
        assert np.array_equal(keep, want), np.nonzero(keep != want)[0][:10]
        assert 0 < want.sum() < (~hot[y * W + x]).sum()                          # some events of normal pixels go, some stay
        assert list(stats) == list(STATS) and stats["kept"] == want.sum() and stats["dropped_hot"] == hot[y * W + x].sum()
        assert stats["kept"] + stats["dropped_hot"] + stats["dropped_unsupported"] == len(t) == stats["events"]
    # without a window every event is supported: only the hot pixel's go
    x, y, t = small_stream(0)
    keep, _ = filter_reference(x, y, t, W, H, None, 2.0, include_self)
    assert np.array_equal(keep, ~((x == 2) & (y == 1)))


def test_reference_does_not_depend_on_the_order_of_the_events():
    x, y, t = small_stream(2)
    keep, stats = filter_reference(x, y, t, W, H, 3, 2.0, True)
    perm = np.random.default_rng(3).permutation(len(t))
    keep_p, stats_p = filter_reference(x[perm], y[perm], t[perm], W, H, 3, 2.0, True)
    assert np.array_equal(keep_p, keep[perm]) and stats_p == stats


@pytest.mark.parametrize("counts", [[3, 1, 4, 1, 5, 9, 2, 6], [7, 7, 7, 7, 7], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 400], [12],
                                    [2, 0, 0, 5, 0, 11, 3]])
@pytest.mark.parametrize("k", [0.0, 0.5, 3.0])
def test_hot_pixel_threshold_is_floor_of_mean_plus_k_std(counts, k):
    """against numpy's mean / std (two passes, float64) over the active pixels.  The two roundings may differ by a few ulp, so
    every case is first shown to lie away from an integer by far more than that"""
    c = np.array([v for v in counts if v > 0], np.float64)
    exact = c.mean() + k * c.std()
    if not (c == c[0]).all():
        assert abs(exact - round(exact)) > 1e-6
    got = data.hot_pixel_threshold(int(c.sum()), int((c * c).sum()), len(c), k)
    assert isinstance(got, int) and got == math.floor(exact)
    if (c == c[0]).all():                                                         # sigma = 0: the threshold is the count, nothing is hot
        assert got == int(c[0]) and not (c > got).any()
    if k == 0.0:
        assert got == math.floor(c.sum() / len(c))


def test_hot_pixel_threshold_takes_exact_integer_sums():
    big = 2 ** 31 - 1                                                             # sum c^2 beyond float64's integers, not beyond int
    assert data.hot_pixel_threshold(3 * big, 3 * big * big, 3, 5.0) == big
    assert data.hot_pixel_threshold(0, 0, 0, 3.0) == 0
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            data.hot_pixel_threshold(10, 40, 3, bad)


@pytest.fixture(scope="module")
def lib():
    from robust_e_nerf_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ host refusals
def _no_ops(monkeypatch):
    from robust_e_nerf_amd import ops

    def reached(*a, **k):
        raise AssertionError("the library was reached before the host checks")
    monkeypatch.setattr(ops, "event_support", reached)
    monkeypatch.setattr(torch, "sort", reached)


def test_filter_refuses_bad_streams_before_any_device_work(monkeypatch):
    _no_ops(monkeypatch)
    pos = np.array([[1, 2], [3, 0], [4, 3]], np.uint16)
    ts, pol, calib = np.array([5, 7, 7], np.int64), np.ones(3, bool), calibration()
    run = lambda p=pos, t=ts, q=pol, **kw: data.filter_events(p, t, q, calib, **{"dt": 3, "device": "cpu", **kw})
    with pytest.raises(ValueError, match="must not decrease"):
        run(t=np.array([5, 7, 6], np.int64))
    for bad in ((W, 0), (0, H)):
        with pytest.raises(ValueError, match="outside"):
            run(p=np.array([[1, 2], bad, [4, 3]], np.uint16))
    with pytest.raises(ValueError, match="same number"):
        run(t=ts[:2])
    with pytest.raises(ValueError, match="same number"):
        run(q=np.ones(4, bool))
    with pytest.raises(ValueError, match="integer position"):
        run(t=ts.astype(np.float64))
    for bad in (-1, 2.5, True, 2 ** 63):
        with pytest.raises(ValueError, match="dt must be"):
            run(dt=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="hot-pixel factor"):
            run(hot_sigma=bad)


def test_filter_without_work_launches_nothing(monkeypatch):
    """N = 0 -> an empty result; both options None -> all True: neither uploads, sorts or launches"""
    _no_ops(monkeypatch)
    calib = calibration()
    keep, stats = data.filter_events(np.zeros((0, 2), np.uint16), np.zeros(0, np.int64), np.zeros(0, bool), calib, dt=5,
                                     hot_sigma=3.0, device="cpu")
    assert keep.dtype == np.bool_ and keep.shape == (0,) and list(stats) == list(STATS)
    assert stats == dict(events=0, kept=0, dropped_unsupported=0, dropped_hot=0, hot_pixels=0, hot_threshold=0, active_pixels=0)
    assert stats == filter_reference([], [], [], W, H, 5, 3.0, False)[1]
    pos = np.array([[1, 2], [3, 0], [1, 2]], np.uint16)
    keep, stats = data.filter_events(pos, np.array([5, 7, 7], np.int64), np.ones(3, bool), calib, device="cpu")
    assert keep.dtype == np.bool_ and keep.tolist() == [True] * 3
    assert stats == dict(events=3, kept=3, dropped_unsupported=0, dropped_hot=0, hot_pixels=0, hot_threshold=None, active_pixels=2)
    ref_keep, ref_stats = filter_reference(pos[:, 0], pos[:, 1], [5, 7, 7], W, H, None, None, False)
    assert ref_keep.tolist() == keep.tolist() and ref_stats == stats


def test_event_support_refuses_before_any_launch(lib):
    """wrong shapes, dtypes, devices, a negative dt and len(seg) != H * W + 1 are ValueErrors of ops.event_support itself; CPU
    tensors of the right form get as far as the pointer check and are refused there (no CPU fallback); N = 0 returns empty"""
    from robust_e_nerf_amd import ops
    n = 6
    good = dict(pix_sorted=torch.zeros(n, dtype=torch.int32), order=torch.arange(n), ts_sorted=torch.arange(n),
                seg=torch.zeros(H * W + 1, dtype=torch.int32), hot=torch.zeros(H * W, dtype=torch.uint8), height=H, width=W, dt=3)
    cases = dict(pix_sorted=torch.zeros(n, dtype=torch.int64), order=torch.arange(n, dtype=torch.int32),
                 ts_sorted=torch.arange(n, dtype=torch.int32), seg=torch.zeros(H * W + 1, dtype=torch.int64),
                 hot=torch.zeros(H * W, dtype=torch.bool))
    for name, bad in cases.items():
        with pytest.raises(ValueError, match=f"event_support: {name} must be"):
            ops.event_support(**{**good, name: bad})
    for name, bad in dict(pix_sorted=good["pix_sorted"][:-1], order=torch.arange(n + 1), seg=good["seg"][:-1],
                          hot=good["hot"][:-1]).items():
        with pytest.raises(ValueError, match="event_support: .* must be \\("):
            ops.event_support(**{**good, name: bad})
    with pytest.raises(ValueError, match="seg must be"):
        ops.event_support(**{**good, "height": H + 1, "hot": None})
    for bad in (-1, -2 ** 40, 2 ** 63):
        with pytest.raises(ValueError, match="dt must be"):
            ops.event_support(**{**good, "dt": bad})
    with pytest.raises(ValueError, match="at least one pixel"):
        ops.event_support(**{**good, "height": 0, "seg": torch.zeros(1, dtype=torch.int32), "hot": None})
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.event_support(**good)
    e = lambda dt: torch.empty(0, dtype=dt)
    out = ops.event_support(e(torch.int32), e(torch.int64), e(torch.int64), good["seg"], None, H, W, None)
    assert out.dtype == torch.uint8 and out.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ library
def test_argument_validation_without_gpu(lib):
    """null or misaligned required pointers, negative N, an empty sensor, include_self other than 0 / 1 -> REN_ERR_BAD_ARG;
    N or H * W of 2^31 -> REN_ERR_UNSUPPORTED; before any launch (the pointers below are never dereferenced)"""
    from robust_e_nerf_amd import _lib
    p, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)

    def sup(pix=p, order=p, ts=p, seg=p, hot=p, n=4, h=H, w=W, dt=3, inc=0, keep=p):
        return lib.ren_event_support(pix, order, ts, seg, hot, n, h, w, dt, inc, keep, None)
    for name in ("pix", "order", "ts", "seg", "keep"):
        assert sup(**{name: None}) == _lib.REN_ERR_BAD_ARG, name
    assert sup(order=odd) == _lib.REN_ERR_BAD_ARG and sup(ts=odd) == _lib.REN_ERR_BAD_ARG       # int64 arrays on a 4-byte boundary
    assert sup(pix=ctypes.c_void_p((1 << 20) + 2)) == _lib.REN_ERR_BAD_ARG
    assert sup(n=-1) == _lib.REN_ERR_BAD_ARG and sup(h=0) == _lib.REN_ERR_BAD_ARG and sup(w=0) == _lib.REN_ERR_BAD_ARG
    assert sup(inc=2) == _lib.REN_ERR_BAD_ARG and sup(inc=-1) == _lib.REN_ERR_BAD_ARG
    assert sup(n=2 ** 31) == _lib.REN_ERR_UNSUPPORTED
    assert sup(h=65536, w=32768) == _lib.REN_ERR_UNSUPPORTED                                     # H * W = 2^31
    assert sup(pix=None, order=None, ts=None, seg=None, hot=None, keep=None, n=0) == _lib.REN_OK  # nothing to do, nothing launched


def test_symbol_is_declared_bound_and_built(lib):
    from robust_e_nerf_amd import _lib, build, ops
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    assert "/* ---- event filter (csrc/ren_event_filter.hip)" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint ren_event_support\s*\(", code)
    assert "ren_event_support" in _lib.SIGNATURES and hasattr(lib, "ren_event_support")
    assert "ren_event_filter.hip" in build.SOURCES
    assert re.search(rf"#define REN_EVENT_FILTER_THREADS {ops.EVENT_FILTER_THREADS}\b", code)
    assert re.search(rf"#define REN_EVENT_FILTER_MAX_BLOCKS {ops.EVENT_FILTER_MAX_BLOCKS}\b", code)
    assert lib.ren_abi_version() == 25


# ------------------------------------------------------------------------------------------------------------ load_event_table
def test_load_event_table_default_path_never_calls_the_filter(tmp_path, monkeypatch):
    """without event_filter the cached table comes back as before and filter_events is not reached; with it, the filter is
    called with the dict's options and the caches are neither read nor written"""
    def reached(*a, **k):
        raise AssertionError("filter_events was called on the default path")
    monkeypatch.setattr(data, "filter_events", reached)
    g = np.random.default_rng(2)
    n = 50
    pos = np.stack([g.integers(0, W, n), g.integers(0, H, n)], -1).astype(np.int64)
    ts = np.sort(g.integers(0, 10_000, n)).astype(np.int64)
    pol = g.random(n) < 0.5
    events = data.undistort_events(data.queue_raw_events(pos, ts, pol, W), dict(distortion_params=np.zeros(0)))
    root = str(tmp_path)
    torch.save(events, os.path.join(root, data.TF_EVENTS))
    torch.save(data.max_refractory_period(pos, ts, W), os.path.join(root, data.MAX_REFRACTORY_PERIOD))
    for kw in ({}, {"event_filter": None}):
        got, tau = data.load_event_table(root, device="cpu", **kw)
        assert list(got) == list(events) and all(torch.equal(got[k], events[k]) for k in events)
        assert torch.equal(tau, data.load_max_refractory_period(root))

    seen = {}

    def fake_filter(position, timestamp, polarity, calib, **kw):
        seen.update(kw, n=len(timestamp))
        raise RuntimeError("stop here: the table build needs the device")
    monkeypatch.setattr(data, "filter_events", fake_filter)
    np.savez(os.path.join(root, data.RAW_EVENTS), position=pos.astype(np.uint16), timestamp=ts, polarity=pol)
    np.savez(os.path.join(root, data.CAMERA_CALIBRATION), **calibration())
    before = {f: os.path.getmtime(os.path.join(root, f)) for f in os.listdir(root)}
    with pytest.raises(RuntimeError, match="stop here"):
        data.load_event_table(root, device="cpu", event_filter=dict(dt=100, hot_sigma=3.0))
    assert seen == dict(dt=100, hot_sigma=3.0, device="cpu", n=n)
    assert before == {f: os.path.getmtime(os.path.join(root, f)) for f in os.listdir(root)}
