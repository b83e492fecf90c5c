"""Event frames (csrc/ren_event_frames.hip, ops.event_frames) on a synthetic recording: N time-ordered events at 346 x 260 with
a hot-pixel tail (--hot-share of the events on --hot-pixels pixels with Zipf weights, the rest uniform), binned into V windows.

Times, warm, as the median of --iters launches (HIP events; min and max are printed as the spread): the plain atomic kernel,
the form that merges equal counters within a wave, and the same result computed by torch on the same device tensors
(searchsorted on the edges, then bincount and index_add_ of the flat counter index; the faster of the two is the baseline).
Reports events/s, GB/s of the 13 B/event the kernel reads, and that rate's share of --hbm-gbs.  The three results are
compared element for element before anything is timed.  One JSON line; --out writes it to a file too.  GPU only.

    python tools/event_frames_bench.py --n 50000000 --windows 64 [--out profiles/event_frames_bench.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from robust_e_nerf_amd import ops

DEV = "cuda:0"
H, W = 260, 346
BYTES_PER_EVENT = 13          # 4 (x | y << 16) + 8 (timestamp) + 1 (polarity)


def synthetic_stream(n, hot_share, hot_pixels, t_end_ns, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(W, (n,), generator=g, device=DEV, dtype=torch.int32)
    y = torch.randint(H, (n,), generator=g, device=DEV, dtype=torch.int32)
    if hot_pixels > 0 and hot_share > 0:
        hx = torch.randint(W, (hot_pixels,), generator=g, device=DEV, dtype=torch.int32)
        hy = torch.randint(H, (hot_pixels,), generator=g, device=DEV, dtype=torch.int32)
        weights = 1.0 / torch.arange(1, hot_pixels + 1, device=DEV, dtype=torch.float32)
        cdf = torch.cumsum(weights / weights.sum(), 0)
        which = torch.searchsorted(cdf, torch.rand(n, generator=g, device=DEV)).clamp_max(hot_pixels - 1)
        hot = torch.rand(n, generator=g, device=DEV) < hot_share
        x, y = torch.where(hot, hx[which], x), torch.where(hot, hy[which], y)
    words = (x | (y << 16)).contiguous()
    ts = torch.sort(torch.randint(t_end_ns, (n,), generator=g, device=DEV, dtype=torch.int64)).values
    pol = torch.rand(n, generator=g, device=DEV) < 0.5
    return words, ts, pol


def torch_index(words, ts, pol, edges, V):
    v = torch.searchsorted(edges, ts, right=True) - 1
    x, y = words & 0xffff, (words >> 16) & 0xffff
    keep = (v >= 0) & (v < V) & (x < W) & (y < H)
    return (((v * 2 + (~pol).long()) * H + y) * W + x)[keep]


def torch_bincount(words, ts, pol, edges, V):
    return torch.bincount(torch_index(words, ts, pol, edges, V), minlength=V * 2 * H * W).view(V, 2, H, W)


def torch_index_add(words, ts, pol, edges, V):
    idx = torch_index(words, ts, pol, edges, V)
    out = torch.zeros(V * 2 * H * W, device=DEV, dtype=torch.int32)
    return out.index_add_(0, idx, torch.ones(idx.shape[0], device=DEV, dtype=torch.int32)).view(V, 2, H, W)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hot-share", type=float, default=0.02)
    ap.add_argument("--hot-pixels", type=int, default=64)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the read bound is taken against (GB/s)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("event_frames_bench needs the GPU")
    n, V = args.n, args.windows
    t_end = 10_000_000_000
    words, ts, pol = synthetic_stream(n, args.hot_share, args.hot_pixels, t_end, 0)
    edges = (torch.arange(V + 1, dtype=torch.int64) * (t_end // V)).to(DEV)       # the last (t_end % V) ns fall outside

    plain = ops.event_frames(words, ts, pol, edges, H, W)
    merged = ops.event_frames(words, ts, pol, edges, H, W, merge=True)
    want = torch_bincount(words, ts, pol, edges, V)
    assert torch.equal(plain, merged) and torch.equal(plain.long(), want), "kernel and torch disagree"
    assert torch.equal(torch_index_add(words, ts, pol, edges, V), plain)
    binned = int(plain.sum())
    del merged, want

    out = torch.zeros_like(plain)
    res = dict(n=n, windows=V, height=H, width=W, hot_share=args.hot_share, hot_pixels=args.hot_pixels, events_binned=binned,
               largest_count=int(plain.max()), iters=args.iters)
    # kernel only (the counts keep growing: the time of an add does not depend on the value); then with the zero fill a call needs
    res["hip_plain_kernel"] = timed(lambda: ops.event_frames(words, ts, pol, edges, H, W, out=out), args.iters)
    res["hip_merge_kernel"] = timed(lambda: ops.event_frames(words, ts, pol, edges, H, W, merge=True, out=out), args.iters)
    res["hip_plain_with_zero_fill"] = timed(lambda: ops.event_frames(words, ts, pol, edges, H, W), args.iters)
    res["hip_merge_with_zero_fill"] = timed(lambda: ops.event_frames(words, ts, pol, edges, H, W, merge=True), args.iters)
    res["torch_bincount"] = timed(lambda: torch_bincount(words, ts, pol, edges, V), args.iters)
    res["torch_index_add"] = timed(lambda: torch_index_add(words, ts, pol, edges, V), args.iters)
    res["hip_plain_kernel_again"] = timed(lambda: ops.event_frames(words, ts, pol, edges, H, W, out=out), args.iters)
    ms = res["hip_plain_kernel"]["median_ms"]
    base = min(res["torch_bincount"]["median_ms"], res["torch_index_add"]["median_ms"])
    gbs = n * BYTES_PER_EVENT / (ms * 1e-3) / 1e9
    res.update(events_per_s=round(n / (ms * 1e-3), 1), read_gb_per_s=round(gbs, 2),
               read_bound_ms=round(n * BYTES_PER_EVENT / (args.hbm_gbs * 1e9) * 1e3, 4),
               share_of_read_bound=round(gbs / args.hbm_gbs, 4), torch_baseline_ms=base,
               speedup_over_torch=round(base / res["hip_plain_with_zero_fill"]["median_ms"], 2))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
