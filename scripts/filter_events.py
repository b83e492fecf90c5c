"""Take the noise events out of a recording before training (robust_e_nerf_amd.data.filter_events).

    python scripts/filter_events.py --dataset-dir IN --out OUT [--support-us D] [--hot-sigma K] [--include-self]

IN holds raw_events.npz and camera_calibration.npz (the reference's layout).  --hot-sigma K drops the events of HOT pixels:
those that hold more than floor(mean + K standard deviations) events, mean and deviation taken over the pixels that fired at
all.  --support-us D drops the events WITHOUT SUPPORT: no other event at one of the eight neighbouring pixels (hot ones do not
count; the pixel itself counts with --include-self) in the D microseconds up to the event, equal timestamps included.
Timestamps are nanoseconds.  The decision runs on the GPU and does not depend on the order of the stream.

OUT/raw_events.npz holds the kept events with the keys and dtypes of the input; every other .npz of IN is copied, so OUT is a
dataset directory (no events.pt / max_refractory_period.pt: those caches would belong to the unfiltered stream).  The counts
are printed and written to OUT/event_filter.json.
"""
import argparse
import json
import os
import shutil
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dataset-dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--support-us", type=float, help="support window in microseconds (default: no support test)")
    ap.add_argument("--hot-sigma", type=float, help="hot-pixel factor K (default: no pixel is hot)")
    ap.add_argument("--include-self", action="store_true", help="an earlier event at the pixel itself supports too")
    args = ap.parse_args()
    if os.path.abspath(args.out) == os.path.abspath(args.dataset_dir):
        raise SystemExit("--out must differ from --dataset-dir: the recording is not overwritten")

    from robust_e_nerf_amd import data
    raw = np.load(os.path.join(args.dataset_dir, data.RAW_EVENTS))
    calib = np.load(os.path.join(args.dataset_dir, data.CAMERA_CALIBRATION))
    dt = None if args.support_us is None else int(round(args.support_us * 1e3))
    keep, stats = data.filter_events(raw["position"], raw["timestamp"], raw["polarity"], calib, dt=dt, hot_sigma=args.hot_sigma,
                                     include_self=args.include_self)
    os.makedirs(args.out, exist_ok=True)
    per_event = {"position", "timestamp", "polarity"}
    np.savez(os.path.join(args.out, data.RAW_EVENTS), **{k: raw[k][keep] if k in per_event else raw[k] for k in raw.files})
    for f in sorted(os.listdir(args.dataset_dir)):
        if f.endswith(".npz") and f != data.RAW_EVENTS:
            shutil.copyfile(os.path.join(args.dataset_dir, f), os.path.join(args.out, f))
    stats = dict(stats, support_ns=dt, hot_sigma=args.hot_sigma, include_self=bool(args.include_self))
    with open(os.path.join(args.out, "event_filter.json"), "w") as f:
        json.dump(stats, f, indent=1)
        f.write("\n")
    print(json.dumps(stats), flush=True)


if __name__ == "__main__":
    main()
