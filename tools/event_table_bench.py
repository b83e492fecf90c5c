"""Start-up cost of the event table (csrc/ren_event_table.hip, data.build_event_table) on a synthetic time-ordered recording of
a 1280 x 720 equidistant sensor, against the path the table took before: data._queue_raw_events_device (int64 widening, the
sort, the copy back to the host), colorize_events and undistort_events on the host, the upload, and max_refractory_period
on the host.

Per size: both results are compared key by key (torch.equal) before anything is timed.  Then, warm, per path the median wall
time of --repeats runs that end in a device synchronise (min and max are the spread), and torch.cuda.max_memory_allocated of
one run per event.  The old path is timed stage by stage; its host stages are plain numpy, need no warm-up, and can be given
fewer repeats (--host-repeats) because one run of them takes minutes at 2 x 10^8 events.  The two kernels, the sort and the
prefix sum are timed on their own with device events; the kernels' rates are set against --hbm-gbs with the bytes counted
from the shapes (BYTES below; gathers and scatters counted at the bytes they use, not at the lines they touch).

    python tools/event_table_bench.py                    # 2 x 10^7 and 2 x 10^8, each in a child process under its own timeout
    python tools/event_table_bench.py --n 20000000       # one size, in this process

Results are merged into --out (default profiles/event_table_bench.json) by size.  GPU only."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from robust_e_nerf_amd import data, ops

DEV = "cuda:0"
W, H = 1280, 720
SIZES = {20_000_000: 900, 200_000_000: 1200}           # size -> time limit of its child process (s)
DIST = np.array([-0.08, 0.05, -0.02, 0.006])
K = np.array([[1050.0, 0.0, 639.6], [0.0, 1052.0, 359.7], [0.0, 0.0, 1.0]])
CALIB = dict(intrinsics=K, img_width=np.uint16(W), img_height=np.uint16(H), distortion_model=np.array("equidistant"),
             distortion_params=DIST, bayer_pattern=np.array(""))


def bytes_per_event(kept_share):
    """what the algorithm needs per event of the stream; kept_share = M / N"""
    intervals = 4 + 8 + 8 + 1 + 8 * kept_share                    # key, order, ts gather | valid scatter, start_ts scatter
    write = 1 + 4 + 4 + kept_share * (8 + 8 + 1 + 8 + 40)         # flag, offset, uint16 pair | ts, start_ts, polarity, LUT | row
    return intervals, write


def synthetic_stream(n, seed):
    g = np.random.default_rng(seed)
    pos = np.empty((n, 2), np.uint16)
    pos[:, 0] = g.integers(0, W, n, dtype=np.uint16)
    pos[:, 1] = g.integers(0, H, n, dtype=np.uint16)
    ts = np.cumsum(g.integers(0, 100, n, dtype=np.int64))         # time-ordered, 1 % of the steps are 0 ns
    return pos, ts, g.random(n) < 0.5


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(ts):
    ts = sorted(ts)
    return dict(median_s=round(ts[len(ts) // 2], 4), min_s=round(ts[0], 4), max_s=round(ts[-1], 4), repeats=len(ts))


def old_path(pos, ts, pol, timing=None):
    """the table and tau_max as the start-up built them before; timing: dict of lists that the stage times are appended to"""
    ev, t_dev = sync_time(lambda: data._queue_raw_events_device(pos, ts, pol, W, DEV))
    raw_position = ev["position"]
    ev, t_host = sync_time(lambda: data.undistort_events(data.colorize_events(ev, ""), CALIB))
    table, t_up = sync_time(lambda: {k: v.to(DEV) for k, v in ev.items()})
    tau, t_tau = sync_time(lambda: data.max_refractory_period(pos, ts, W))
    if timing is not None:
        for k, v in (("queue_on_device_with_copies", t_dev), ("colorize_undistort_host", t_host), ("upload", t_up),
                     ("max_refractory_period_host", t_tau)):
            timing.setdefault(k, []).append(v)
    return table, tau, raw_position


def positions_restated(pos, ts):
    """the kept events' positions by torch alone: the lookup table gathered at the int32 keys of the kept events"""
    pos_d, ts_d = torch.from_numpy(pos).to(DEV), torch.from_numpy(ts).to(DEV)
    word = pos_d.view(torch.int32).view(-1)
    pix = ((word >> 16) & 0xffff) * W + (word & 0xffff)
    valid = ops.event_intervals(*torch.sort(pix, stable=True), ts_d)[0]
    lut = torch.from_numpy(data.undistortion_lut(CALIB)).to(DEV)
    return lut[pix[torch.nonzero(valid)[:, 0]].long()]


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def run(n, repeats, host_repeats, hbm_gbs):
    say = lambda *a: print(*a, file=sys.stderr, flush=True)
    pos, ts, pol = synthetic_stream(n, 0)
    say(f"n = {n}: stream generated")
    new = lambda: data.build_event_table(pos, ts, pol, CALIB, DEV)
    (table, tau), first_new = sync_time(new)
    old_t = {}
    (want, want_tau, raw), first_old = sync_time(lambda: old_path(pos, ts, pol, old_t if host_repeats == 1 else None))
    assert list(table) == list(want) and torch.equal(tau, want_tau), (tau, want_tau)
    bad = []
    for k in want:
        if table[k].dtype != want[k].dtype or table[k].shape != want[k].shape:
            bad.append(f"{k}: {table[k].dtype} {tuple(table[k].shape)} against {want[k].dtype} {tuple(want[k].shape)}")
        elif not torch.equal(table[k], want[k]):
            ne = (table[k] != want[k]).reshape(len(want[k]), -1).any(1)
            i = int(torch.nonzero(ne)[0])
            bad.append(f"{k}: {int(ne.sum())} rows differ, first at {i}: {table[k][i].tolist()} against {want[k][i].tolist()}")
    # seen at 2 x 10^8 events: the old path's gather of the 3.2 GB int64 position tensor comes back with a 2 GiB run of zeros,
    # i.e. 2^27 events at pixel (0, 0) where a uniform stream has m / (H W) of them; every other column agrees.  The new
    # positions are then held to a torch restatement (the lookup table gathered at the kept events' keys) instead.
    at_origin = int(((raw[:, 0] == 0) & (raw[:, 1] == 0)).sum())
    del raw
    if at_origin > 10 * len(want["position"]) / (H * W) + 1000 and len(bad) == 1 and bad[0].startswith("position: "):
        say(f"n = {n}: the old path returned {at_origin} events at pixel (0, 0); {bad[0]}")
        assert torch.equal(table["position"], positions_restated(pos, ts)), "new positions differ from the torch restatement"
        bad = []
    assert not bad, "the two paths disagree -- " + "; ".join(bad)
    m = len(table["position"])
    say(f"n = {n}: {m} kept, tau_max {float(tau)}, both paths agree (first runs: new {first_new:.2f} s, old {first_old:.2f} s)")
    del table, want
    res = dict(n=n, kept=m, height=H, width=W, distortion_model="equidistant", tau_max=float(tau), hbm_gbs=hbm_gbs,
               first_run_s=dict(new=round(first_new, 3), old=round(first_old, 3)), old_path_events_at_pixel_0_0=at_origin)

    # ---- the whole paths, host arrays in, device table out
    t_new = []
    for _ in range(repeats):
        t_new.append(sync_time(new)[1])
        say(f"  new path {t_new[-1]:.3f} s")
    res["new_path"] = stats(t_new)
    if host_repeats > 1:                                          # the first run above was the warm-up
        for _ in range(host_repeats):
            t0 = time.perf_counter()
            old_path(pos, ts, pol, old_t)
            say(f"  old path {time.perf_counter() - t0:.3f} s")
    else:                                                         # host stages from the first run; the device stage repeated
        for _ in range(repeats):
            old_t["queue_on_device_with_copies"].append(sync_time(lambda: data._queue_raw_events_device(pos, ts, pol, W, DEV))[1])
            say(f"  old device stage {old_t['queue_on_device_with_copies'][-1]:.3f} s")
        old_t["queue_on_device_with_copies"].pop(0)               # its first run loaded code objects
    res["old_path_stages"] = {k: stats(v) for k, v in old_t.items()}
    res["old_path_total_median_s"] = round(sum(v["median_s"] for v in res["old_path_stages"].values()), 4)
    res["speedup_whole_path"] = round(res["old_path_total_median_s"] / res["new_path"]["median_s"], 2)
    res["speedup_over_old_device_stage_alone"] = round(
        res["old_path_stages"]["queue_on_device_with_copies"]["median_s"] / res["new_path"]["median_s"], 2)
    res["peak_device_bytes_per_event"] = dict(
        new=round(peak_bytes(new) / n, 2),
        old=round(peak_bytes(lambda: {k: v.to(DEV) for k, v in data._queue_raw_events_device(pos, ts, pol, W, DEV).items()}) / n, 2))

    # ---- the device pieces of the new path on their own
    pos_d, ts_d, pol_d = (torch.from_numpy(a).to(DEV) for a in (pos, ts, pol))
    lut = torch.from_numpy(data.undistortion_lut(CALIB)).to(DEV)
    word = pos_d.view(torch.int32).view(-1)
    pix = ((word >> 16) & 0xffff) * W + (word & 0xffff)
    pix_sorted, order = torch.sort(pix, stable=True)
    valid, start_ts, _ = ops.event_intervals(pix_sorted, order, ts_d)
    offsets = torch.cumsum(valid, 0, dtype=torch.int32).sub_(valid)
    b_iv, b_wr = bytes_per_event(m / n)
    pieces = dict(stable_sort=device_events(lambda: torch.sort(pix, stable=True), repeats),
                  prefix_sum=device_events(lambda: torch.cumsum(valid, 0, dtype=torch.int32).sub_(valid), repeats),
                  ren_event_intervals=device_events(lambda: ops.event_intervals(pix_sorted, order, ts_d), repeats),
                  ren_event_table_write=device_events(
                      lambda: ops.event_table_write(valid, offsets, pos_d, ts_d, start_ts, pol_d, m, H, W, lut), repeats))
    pieces["pixel_keys"] = device_events(lambda: ((word >> 16) & 0xffff) * W + (word & 0xffff), repeats)
    for name, b in (("ren_event_intervals", b_iv), ("ren_event_table_write", b_wr)):
        gbs = n * b / (pieces[name]["median_ms"] * 1e-3) / 1e9
        pieces[name].update(bytes_per_event=round(b, 2), gb_per_s=round(gbs, 1), share_of_read_write_bound=round(gbs / hbm_gbs, 4))
    res["device_pieces"] = pieces
    res["new_device_work_ms"] = round(sum(v["median_ms"] for v in pieces.values()), 4)
    del pix, pix_sorted, order, valid, start_ts, offsets, word

    # ---- where the rest of the new path's wall time goes: its host pieces, and the upload at the stored widths
    host = dict(undistortion_lut=[], range_check=[], upload=[])
    for _ in range(repeats):
        host["undistortion_lut"].append(sync_time(lambda: data.undistortion_lut(CALIB))[1])
        host["range_check"].append(sync_time(lambda: (pos.min(0), pos.max(0)))[1])
        host["upload"].append(sync_time(lambda: [torch.from_numpy(a).to(DEV) for a in (pos, ts, pol)])[1])
    res["new_path_host_pieces"] = {k: stats(v) for k, v in host.items()}

    # ---- the device work of the old path on its own: the torch operations of data._queue_raw_events_device, restated here
    # on tensors that are already uploaded and widened (no copies in the timed region)
    pos64, pol64 = pos_d.to(torch.int64), pol_d.to(torch.int64)

    def old_device_ops():
        pix = pos64[:, 1] * W + pos64[:, 0]
        ps, order = torch.sort(pix, stable=True)
        ts_sorted = ts_d[order]
        first = torch.ones(1, dtype=torch.bool, device=DEV)
        valid_sorted = ~torch.cat([first, (ps[1:] != ps[:-1]) | (ts_sorted[1:] == ts_sorted[:-1])])
        prev_ts = torch.cat([ts_sorted[:1], ts_sorted[:-1]])
        start, valid = torch.empty_like(ts_d), torch.empty_like(valid_sorted)
        start[order] = prev_ts
        valid[order] = valid_sorted
        keep = torch.nonzero(valid)[:, 0]
        return pos64[keep], start[keep], ts_d[keep], pol64[keep], 1 - pol64[keep]
    res["old_device_work_restated_ms"] = device_events(old_device_ops, repeats)
    res["device_work_old_over_new"] = round(res["old_device_work_restated_ms"]["median_ms"] / res["new_device_work_ms"], 2)
    return res


def merge(path, res):
    runs = []
    if os.path.isfile(path):
        with open(path) as f:
            runs = [r for r in json.load(f)["runs"] if r["n"] != res["n"]]
    runs = sorted(runs + [res], key=lambda r: r["n"])
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(runs=runs), f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, help="one size, in this process (default: every size of SIZES in a child process each)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, help="repeats of the old path's host stages (default: --repeats; 1 = the first run's)")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the byte bound is taken against (GB/s)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "event_table_bench.json"))
    args = ap.parse_args()
    if args.repeats < 1 or (args.host_repeats is not None and args.host_repeats < 1):
        raise SystemExit("repeats must be at least 1")
    if args.n is None:
        for n, limit in SIZES.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(n), "--repeats", str(args.repeats), "--hbm-gbs",
                   str(args.hbm_gbs), "--out", args.out] + (["--host-repeats", str(args.host_repeats)] if args.host_repeats else [])
            rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd).returncode
            if rc != 0:                                           # nothing more is started on the device after a failure
                raise SystemExit(f"n = {n}: exit status {rc}")
        return
    if not torch.cuda.is_available():
        raise SystemExit("event_table_bench needs the GPU")
    res = run(args.n, args.repeats, args.host_repeats or args.repeats, args.hbm_gbs)
    print(json.dumps(res), flush=True)
    merge(args.out, res)


if __name__ == "__main__":
    main()
