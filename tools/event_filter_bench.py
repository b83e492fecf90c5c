"""Cost of the event noise filter (csrc/ren_event_filter.hip, data.filter_events) on a synthetic time-ordered recording of a
640 x 480 sensor: uniform pixels, a few hot pixels that take 5 % of the events, time steps of 0 .. 99 ns.

Per size the mask is compared with the numpy restatement (tests/event_filter_reference.py, np.array_equal) before anything is
timed.  Then, warm: the launch alone with device events (median of --repeats, min and max are the spread), set against the
COALESCED byte count of the sorted arrays -- 20 B read per event (key, stream index, time) and 1 B written, the least any filter
over this structure moves; the searches' gathers come on top and are why the launch is not expected near that bound -- and
the whole data.filter_events (host arrays in, host mask out, wall time ending in the copy back) against the wall time of the
numpy reference on the same stream.

    python tools/event_filter_bench.py [--n 1000000 10000000] [--support-us 1500] [--hot-sigma 5] [--repeats 7]

Writes --out (default profiles/event_filter_bench.json).  GPU only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from robust_e_nerf_amd import data, ops

DEV = "cuda:0"
W, H = 640, 480
CALIB = dict(intrinsics=np.eye(3), img_width=np.uint16(W), img_height=np.uint16(H), distortion_model=np.array("plumb_bob"),
             distortion_params=np.zeros(0), bayer_pattern=np.array(""))
COALESCED_BYTES_PER_EVENT = 4 + 8 + 8 + 1              # key, order, ts_sorted read once; one flag written


def synthetic_stream(n, seed, hot_pixels=8, hot_share=0.05):
    g = np.random.default_rng(seed)
    pos = np.empty((n, 2), np.uint16)
    pos[:, 0] = g.integers(0, W, n, dtype=np.uint16)
    pos[:, 1] = g.integers(0, H, n, dtype=np.uint16)
    at_hot = g.random(n) < hot_share
    where = np.stack([g.integers(0, W, hot_pixels), g.integers(0, H, hot_pixels)], -1).astype(np.uint16)
    pos[at_hot] = where[g.integers(0, hot_pixels, int(at_hot.sum()))]
    return pos, np.cumsum(g.integers(0, 100, n, dtype=np.int64)), np.zeros(n, bool)


def device_events(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return dict(median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4), repeats=repeats)


def wall(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out.sort()
    return dict(median_s=round(out[len(out) // 2], 4), min_s=round(out[0], 4), max_s=round(out[-1], 4), repeats=repeats)


def run(n, dt, k, repeats, hbm_gbs):
    from event_filter_reference import filter_reference
    say = lambda *a: print(*a, file=sys.stderr, flush=True)
    pos, ts, pol = synthetic_stream(n, 0)
    whole = lambda: data.filter_events(pos, ts, pol, CALIB, dt=dt, hot_sigma=k, device=DEV)
    keep, stats = whole()
    t0 = time.perf_counter()
    want, want_stats = filter_reference(pos[:, 0], pos[:, 1], ts, W, H, dt, k, False)
    t_ref = time.perf_counter() - t0
    assert np.array_equal(keep, want) and stats == want_stats, "the device mask differs from the numpy reference"
    say(f"n = {n}: {stats}; mask equal to the reference ({t_ref:.2f} s of numpy)")
    res = dict(n=n, height=H, width=W, support_ns=dt, hot_sigma=k, stats=stats, hbm_gbs=hbm_gbs,
               numpy_reference_s=round(t_ref, 3), filter_events_whole=wall(whole, repeats))
    res["whole_over_numpy_reference"] = round(t_ref / res["filter_events_whole"]["median_s"], 2)
    # the launch alone, on the tensors filter_events forms
    pix_sorted, order = torch.sort(data._pixel_keys(torch.from_numpy(pos).to(DEV), W), stable=True)
    seg = torch.searchsorted(pix_sorted, torch.arange(H * W + 1, device=DEV, dtype=torch.int32), out_int32=True)
    counts = (seg[1:] - seg[:-1]).to(torch.int64)
    hot = None if k is None else (counts > stats["hot_threshold"]).to(torch.uint8)
    ts_sorted = torch.from_numpy(ts).to(DEV)[order]
    launch = device_events(lambda: ops.event_support(pix_sorted, order, ts_sorted, seg, hot, H, W, dt, False), repeats)
    gbs = n * COALESCED_BYTES_PER_EVENT / (launch["median_ms"] * 1e-3) / 1e9
    launch.update(coalesced_bytes_per_event=COALESCED_BYTES_PER_EVENT, coalesced_gb_per_s=round(gbs, 1),
                  share_of_coalesced_bound=round(gbs / hbm_gbs, 4), mean_events_per_active_pixel=round(n / stats["active_pixels"], 1))
    res["ren_event_support"] = launch
    res["upload_keys_stable_sort"] = device_events(lambda: torch.sort(data._pixel_keys(torch.from_numpy(pos).to(DEV), W), stable=True), repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--support-us", type=float, default=1500.0)
    ap.add_argument("--hot-sigma", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the byte bound is taken against (GB/s)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "event_filter_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("event_filter_bench needs the GPU")
    results = dict(device=torch.cuda.get_device_name(0), runs=[])
    results["not_measured"] = ("kernel time from a profiler trace (device events around the call instead); hardware counters, so the "
                               "lines the searches touch and their cache hit rates; a real recording (TUM-VIE, DAVIS), whose events "
                               "cluster at edges instead of spreading uniformly; sizes, windows and sensors other than those listed")
    for n in args.n:
        results["runs"].append(run(n, int(round(args.support_us * 1e3)), args.hot_sigma, args.repeats, args.hbm_gbs))
        print(json.dumps(results["runs"][-1]), flush=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
