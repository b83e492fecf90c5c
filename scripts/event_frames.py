"""Compare windows of recorded events with the brightness change a checkpoint predicts (robust_e_nerf_amd.event_frames).

    python scripts/event_frames.py --config <YAML> --ckpt runs/train/last.ckpt --dataset-dir DIR --out DIR \
        [--windows V | --window-ms D] [--start-ms S] [--height 260 --width 346]

The dataset directory holds raw_events.npz, camera_poses.npz and camera_calibration.npz (the reference's layout).  The time
span of the trajectory, from --start-ms after its first pose, is cut into --windows equal windows (default 8) or into
windows of --window-ms (both: that many windows of that length).  Per window the events are counted per pixel and polarity
on the GPU, the field is rendered at the window's two boundary poses, and the measured change C_p n+ - C_n n- is scored
against log I(t1) - log I(t0): C_n is the calibration's negative threshold, C_p = softplus(trained ratio) x C_n as training
resumes it from the checkpoint (the calibration's positive threshold when the checkpoint has no ratio).  One line per window
and their means are printed; <out>/event_frames/<v>.png shows measured | predicted | residual, and <out>/event_frames.npz
holds edges, counts, predicted, valid, the score table (`scores`, columns `score_columns`), the nine sums and c_p / c_n.
Events the refractory period suppressed are not added back: the measured image undercounts where a pixel fires faster.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

SCORE_COLUMNS = ("n_valid", "n_active", "corr", "rmse_over_c", "explained")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--ckpt", help="checkpoint (default: the YAML's model.checkpoint_filepath)")
    ap.add_argument("--dataset-dir", help="default: the YAML's data.dataset_directory")
    ap.add_argument("--out", required=True)
    ap.add_argument("--windows", type=int, help="number of windows (default 8, or as many --window-ms windows as fit)")
    ap.add_argument("--window-ms", type=float, help="window length in milliseconds")
    ap.add_argument("--start-ms", type=float, default=0.0, help="first window's start, after the trajectory's first pose")
    ap.add_argument("--height", type=int)
    ap.add_argument("--width", type=int)
    args = ap.parse_args()

    import render
    from PIL import Image
    from robust_e_nerf_amd import checkpoint, config, data, event_frames as ef
    cfg, ckpt = render.load_config(args.config, args.ckpt)
    dev = "cuda:0"
    torch.cuda.set_device(0)
    ncfg = cfg["model"]["nerf"]
    root = args.dataset_dir or cfg["data"]["dataset_directory"]
    if not root:
        raise SystemExit("no dataset directory: pass --dataset-dir or set data.dataset_directory")
    tab_ts, tab_pos, tab_quat = data.load_camera_poses(root)
    calib = data.load_calibration(root)
    height, width = args.height or int(calib["img_height"]), args.width or int(calib["img_width"])
    bayer = str(calib["bayer_pattern"]) if "bayer_pattern" in calib else ""
    rcfg = config.render_cfg(cfg, tab_pos)
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    arch = ncfg.get("arch", "ngp")
    fld, r = config.make_renderer(ncfg, rcfg, checkpoint.radiance_dim(sd, arch), dev)
    bkgd = checkpoint.load_render_state(sd, fld, r, arch)

    c_n = float(calib["neg_contrast_threshold"])
    if checkpoint.CT_KEY in sd:                            # the trained positive-to-negative ratio (event_generation_params.py:51-70)
        c_p = float(torch.nn.functional.softplus(sd[checkpoint.CT_KEY].reshape(-1)[0].to(torch.float32))) * c_n
    else:
        c_p = float(calib["pos_contrast_threshold"])

    t_first, t_last = int(tab_ts[0]), int(tab_ts[-1])
    window_ns = None if args.window_ms is None else int(round(args.window_ms * 1e6))
    n_windows = args.windows if (args.windows is not None or window_ns is not None) else 8
    edges = ef.window_edges(t_first, t_last, n_windows, window_ns, t_first + int(round(args.start_ms * 1e6)))

    raw = np.load(os.path.join(root, data.RAW_EVENTS))
    counts = ef.accumulate({k: raw[k] for k in ("position", "timestamp", "polarity")}, edges, height, width, dev)
    pred, valid = ef.predicted_change(r, calib["Kinv"].to(dev, torch.float32).contiguous(), tab_ts, tab_pos, tab_quat, edges,
                                      height, width, bkgd=bkgd, calib=calib, bayer_pattern=bayer)
    sc = ef.compare(counts, pred, valid, c_p, c_n)
    measured = ef.measured_change(counts, c_p, c_n)

    out_dir = os.path.join(args.out, "event_frames")
    os.makedirs(out_dir, exist_ok=True)
    print(f"C_p {c_p:.4f}  C_n {c_n:.4f}  {int(counts.sum())} of {len(raw['timestamp'])} events in {edges.numel() - 1} windows "
          f"of {height} x {width}")
    for v in range(edges.numel() - 1):
        print(f"window {v}: [{(int(edges[v]) - t_first) / 1e6:.3f}, {(int(edges[v + 1]) - t_first) / 1e6:.3f}) ms  "
              f"valid {int(sc['n_valid'][v])}  active {int(sc['n_active'][v])}  corr {float(sc['corr'][v]):.4f}  "
              f"rmse/C {float(sc['rmse_over_c'][v]):.4f}  explained {float(sc['explained'][v]):.4f}", flush=True)
        Image.fromarray(ef.frame_png(measured[v], pred[v], valid[v], (c_p + c_n) / 2).numpy(), mode="RGB").save(
            os.path.join(out_dir, f"{v}.png"))
    print(f"mean: corr {sc['mean_corr']:.4f}  rmse/C {sc['mean_rmse_over_c']:.4f}  explained {sc['mean_explained']:.4f}", flush=True)
    table = torch.stack([sc[k].to(torch.float64) for k in SCORE_COLUMNS], 1).numpy()
    np.savez(os.path.join(args.out, "event_frames.npz"), edges=edges.numpy(), counts=counts.cpu().numpy(),
             predicted=pred.cpu().numpy(), valid=valid.cpu().numpy(), scores=table, score_columns=np.array(SCORE_COLUMNS),
             sums=sc["sums"].numpy(), c_p=c_p, c_n=c_n)


if __name__ == "__main__":
    main()
