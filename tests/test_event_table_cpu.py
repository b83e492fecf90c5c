"""CPU: the host side of the device-built event table (data.undistortion_lut, build_event_table's checks, the cache path of
load_event_table) and the argument validation of ren_event_intervals / ren_event_table_write, which returns before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from robust_e_nerf_amd import data

W, H = 37, 23
K = np.array([[30.0, 0.0, 17.6], [0.0, 31.0, 11.2], [0.0, 0.0, 1.0]])
DIST = {"plumb_bob": np.array([-0.35, 0.12, 0.004, -0.003]), "equidistant": np.array([-0.08, 0.05, -0.02, 0.006])}


def calibration(model=None, bayer="", dist=None):
    d = np.zeros(0) if model is None else DIST[model]
    return dict(intrinsics=K, img_width=np.uint16(W), img_height=np.uint16(H), distortion_params=d if dist is None else dist,
                distortion_model=np.array(model or "plumb_bob"), bayer_pattern=np.array(bayer))


@pytest.fixture(scope="module")
def lib():
    from robust_e_nerf_amd import build, _lib
    build.build()
    return _lib.load()


def test_lut_is_none_without_distortion():
    assert data.undistortion_lut(calibration()) is None
    assert data.undistortion_lut(calibration("plumb_bob", dist=np.zeros(4))) is None
    assert data.undistortion_lut(calibration("equidistant", dist=np.zeros(4, np.float32))) is None


@pytest.mark.parametrize("model", ["equidistant", "plumb_bob"])
def test_lut_gather_is_bitwise_the_per_event_undistortion(model):
    calib = calibration(model)
    lut = data.undistortion_lut(calib)
    assert lut.dtype == np.float32 and lut.shape == (H * W, 2)
    g = np.random.default_rng(5)
    pos = np.stack([g.integers(0, W, 2000), g.integers(0, H, 2000)], -1).astype(np.int64)
    want = data.undistort_events({"position": torch.from_numpy(pos)}, calib)["position"].numpy()
    assert want.dtype == np.float32 and np.abs(want - pos).max() > 0.5              # the coefficients do move pixels
    got = lut[pos[:, 1] * W + pos[:, 0]]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _no_ops(monkeypatch):
    from robust_e_nerf_amd import ops

    def reached(*a, **k):
        raise AssertionError("the library was reached before the host checks")
    monkeypatch.setattr(ops, "event_intervals", reached)
    monkeypatch.setattr(ops, "event_table_write", reached)


@pytest.mark.parametrize("bad", [(W, 0), (0, H)])
def test_build_refuses_a_pixel_outside_the_sensor_before_any_library_call(monkeypatch, bad):
    _no_ops(monkeypatch)
    pos = np.array([[1, 2], bad, [3, 4]], np.uint16)
    with pytest.raises(ValueError, match="outside"):
        data.build_event_table(pos, np.arange(3, dtype=np.int64), np.ones(3, bool), calibration("equidistant"), "cpu")


def test_build_refuses_unequal_lengths_before_any_library_call(monkeypatch):
    _no_ops(monkeypatch)
    pos = np.zeros((3, 2), np.uint16)
    for ts, pol in ((np.arange(2), np.ones(3, bool)), (np.arange(3), np.ones(4, bool))):
        with pytest.raises(ValueError, match="same number"):
            data.build_event_table(pos, ts.astype(np.int64), pol, calibration(), "cpu")


def test_argument_validation_without_gpu(lib):
    """null or misaligned required pointers -> REN_ERR_BAD_ARG, N or H * W of 2^31 -> REN_ERR_UNSUPPORTED, before any launch
    (the pointers below are never dereferenced)"""
    from robust_e_nerf_amd import _lib
    p, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    big = 2 ** 31
    iv = lib.ren_event_intervals
    assert iv(None, p, p, 4, p, p, p, None) == _lib.REN_ERR_BAD_ARG
    assert iv(p, p, None, 4, p, p, p, None) == _lib.REN_ERR_BAD_ARG
    assert iv(p, p, p, 4, p, p, None, None) == _lib.REN_ERR_BAD_ARG
    assert iv(p, p, p, 0, p, p, None, None) == _lib.REN_ERR_BAD_ARG                # the minimum word is required even for N = 0
    assert iv(p, p, p, -1, p, p, p, None) == _lib.REN_ERR_BAD_ARG
    assert iv(p, odd, p, 4, p, p, p, None) == _lib.REN_ERR_BAD_ARG                 # int64 array on a 4-byte boundary
    assert iv(p, p, p, 4, p, p, odd, None) == _lib.REN_ERR_BAD_ARG
    assert iv(p, p, p, big, p, p, p, None) == _lib.REN_ERR_UNSUPPORTED
    assert iv(None, None, None, 0, None, None, p, None) == _lib.REN_OK             # nothing to do, nothing launched

    def tw(valid=p, offsets=p, position=p, pb=2, ts=p, start=p, pol=p, n=4, m=2, lut=None, h=H, w=W, bayer=None, o=(p,) * 5,
           chan=None):
        return lib.ren_event_table_write(valid, offsets, position, pb, ts, start, pol, n, m, lut, h, w, bayer, *o, chan, None)
    for name in ("valid", "offsets", "position", "ts", "start", "pol"):
        assert tw(**{name: None}) == _lib.REN_ERR_BAD_ARG, name
    for k in range(5):
        assert tw(o=tuple(None if i == k else p for i in range(5))) == _lib.REN_ERR_BAD_ARG
    assert tw(start=odd) == _lib.REN_ERR_BAD_ARG and tw(lut=odd) == _lib.REN_ERR_BAD_ARG
    assert tw(position=odd, pb=8) == _lib.REN_ERR_BAD_ARG and tw(position=odd, pb=2, m=0) == _lib.REN_OK
    assert tw(pb=3) == _lib.REN_ERR_BAD_ARG and tw(m=5) == _lib.REN_ERR_BAD_ARG and tw(h=0) == _lib.REN_ERR_BAD_ARG
    code = (ctypes.c_uint8 * 4)(0, 1, 1, 2)
    assert tw(bayer=ctypes.cast(code, ctypes.c_void_p)) == _lib.REN_ERR_BAD_ARG    # a channel code without its output
    assert tw(chan=p) == _lib.REN_ERR_BAD_ARG
    assert tw(n=big, m=2) == _lib.REN_ERR_UNSUPPORTED
    assert tw(h=65536, w=32768) == _lib.REN_ERR_UNSUPPORTED                        # H * W = 2^31
    assert tw(n=4, m=0) == _lib.REN_OK and tw(n=0, m=0) == _lib.REN_OK


def test_both_symbols_are_declared_and_bound(lib):
    from robust_e_nerf_amd import _lib, build, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ren_amd.h")).read(), flags=re.S)
    for name in ("ren_event_intervals", "ren_event_table_write"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "ren_event_table.hip" in build.SOURCES
    assert re.search(rf"#define REN_EVENT_TABLE_THREADS {ops.EVENT_TABLE_THREADS}\b", hdr)
    assert lib.ren_abi_version() == 25


def test_ops_return_empty_tensors_without_a_launch():
    """N = 0 and M = 0 never reach the library (CPU tensors would be refused there)"""
    from robust_e_nerf_amd import ops
    e = lambda dt, *s: torch.empty(*s, dtype=dt)
    valid, start, md = ops.event_intervals(e(torch.int32, 0), e(torch.int64, 0), e(torch.int64, 0))
    assert (valid.dtype, start.dtype, md.dtype) == (torch.uint8, torch.int64, torch.int64)
    assert valid.shape == (0,) and start.shape == (0,) and int(md) == 2 ** 63 - 1
    for n in (0, 3):
        out = ops.event_table_write(torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.int32), e(torch.uint16, n, 2),
                                    e(torch.int64, n), e(torch.int64, n), e(torch.bool, n), 0, H, W, None, [0, 1, 1, 2])
        assert list(out) == ["position", "start_ts", "end_ts", "num_pos", "num_neg", "channel_idx"]
        assert out["position"].shape == (0, 2) and out["position"].dtype == torch.float32
        assert all(out[k].dtype == torch.int64 and out[k].shape == (0,) for k in ("start_ts", "end_ts", "num_pos", "num_neg"))
        assert out["channel_idx"].dtype == torch.uint8
    with pytest.raises(ValueError):
        ops.event_table_write(torch.ones(3, dtype=torch.uint8), torch.arange(3, dtype=torch.int32), e(torch.uint16, 3, 2),
                              e(torch.int64, 3), e(torch.int64, 3), e(torch.bool, 3), 3, H, W)      # CPU tensors: refused


def test_load_event_table_reads_both_caches_and_nothing_else(tmp_path, monkeypatch):
    """events.pt and max_refractory_period.pt present, raw_events.npz and the calibration absent, the ops poisoned: the caches
    come back, permuted as load_events permutes"""
    _no_ops(monkeypatch)
    g = np.random.default_rng(2)
    n = 50
    pos = np.stack([g.integers(0, 5, n), g.integers(0, 3, n)], -1).astype(np.int64)
    ts = np.sort(g.integers(0, 10_000, n)).astype(np.int64)
    events = data.colorize_events(data.queue_raw_events(pos, ts, g.random(n) < 0.5, 5), "RGGB")
    events = data.undistort_events(events, dict(distortion_params=np.zeros(0)))
    assert len(events["position"]) > 10
    root = str(tmp_path)
    torch.save(events, os.path.join(root, data.TF_EVENTS))
    torch.save(data.max_refractory_period(pos, ts, 5), os.path.join(root, data.MAX_REFRACTORY_PERIOD))
    for seed in (None, 7):
        got, tau = data.load_event_table(root, seed, device="cpu")
        want = data.load_events(root, seed)
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        assert tau.dtype == torch.float64 and torch.equal(tau, data.load_max_refractory_period(root))
    assert sorted(os.listdir(root)) == sorted([data.TF_EVENTS, data.MAX_REFRACTORY_PERIOD])
