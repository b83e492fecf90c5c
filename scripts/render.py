"""Render views from a checkpoint: the inference side of the reference's `evaluation_step` / `evaluation_epoch_end`
(robust_e_nerf/models/robust_e_nerf.py:533-571, 634-677) for a checkpoint written by scripts/train.py or by the
reference (same state-dict keys).

    python scripts/render.py --config <YAML> --ckpt runs/train/last.ckpt --out renders/ \
        [--dataset-dir DIR | --synthetic] [--every 50] [--height 260 --width 346] [--gt-dir DIR] [--normals]
    python scripts/render.py --config <test YAML> --stage test --out renders/      # --ckpt: model.checkpoint_filepath

Poses come from the dataset's camera_poses.npz (every `--every`-th pose) or from the synthetic benchmark orbit; the
intrinsics from camera_calibration.npz.  Each view is written as <index>.png (8-bit, intensity clipped to [0, 1] after an
optional gain) and all of them as views.npz (float32 intensity, opacity, z-depth).  With --gt-dir (files <index>.npy:
linear intensity images of the same size) the prediction is aligned to the ground truth by the reference's affine fit in
log space and the PSNR of every view and their mean are printed (metric.py:60-72).  With --stage val | test the
dataset's posed views are scored as the reference's validation / test epochs score them: aligned L1, PSNR and SSIM per
view and their means (metric.py:54-81), and with model.eval_save_pred_intensity_img the aligned predictions are written
to <out>/predictions/<sample_id>.png (robust_e_nerf.py:736-780).  With --normals (arch ngp) every view's surface-normal map --
the composited direction of -grad(sigma), camera frame -- is written as <out>/normals/<index>.png (RGB = (n + 1) / 2,
transparent pixels white) and added to views.npz as `normal` (float32, (views, 3, H, W)).
"""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def load_config(config: str, ckpt=None):
    """the YAML, checked against what the kernels implement (config.check_supported), and the checkpoint to load: --ckpt, or
    model.checkpoint_filepath as the reference's test YAMLs give it (configs/test/*.yaml)"""
    from robust_e_nerf_amd import config as schema
    cfg = yaml.safe_load(open(config))
    ncfg = cfg["model"]["nerf"]
    schema.check_supported(ncfg, ncfg.get("arch", "ngp"))
    ckpt = ckpt or cfg["model"].get("checkpoint_filepath")
    if not ckpt:
        raise SystemExit(f"{config}: no checkpoint: pass --ckpt or set model.checkpoint_filepath")
    return cfg, ckpt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--ckpt", help="checkpoint to render (default: the YAML's model.checkpoint_filepath)")
    ap.add_argument("--out", default="renders")
    ap.add_argument("--dataset-dir")
    ap.add_argument("--synthetic", action="store_true", help="poses / intrinsics of the synthetic benchmark orbit")
    ap.add_argument("--every", type=int, default=100, help="render every N-th pose of the trajectory")
    ap.add_argument("--height", type=int)
    ap.add_argument("--width", type=int)
    ap.add_argument("--gain", type=float, default=1.0, help="multiplies the intensity before the 8-bit PNG is written")
    ap.add_argument("--gt-dir", help="<index>.npy ground-truth intensity images: aligned PSNR is reported")
    ap.add_argument("--stage", choices=["val", "test"],
                    help="evaluate on the dataset's posed images (views/transforms_<stage>.json, the reference's PosedImage "
                         "layout) instead of rendering along the trajectory: aligned L1 / PSNR / SSIM per view and their means, as "
                         "the reference's validation / test epochs (robust_e_nerf.py:519-696)")
    ap.add_argument("--chunk", type=int, help="rays per render call (default: whole image for arch ngp, 16 384 for arch mlp)")
    ap.add_argument("--normals", action="store_true",
                    help="also write surface-normal maps (camera frame) to <out>/normals/<index>.png and views.npz (arch ngp)")
    args = ap.parse_args()

    from robust_e_nerf_amd import checkpoint, config, data, evaluation, ops
    cfg, ckpt = load_config(args.config, args.ckpt)
    dev = "cuda:0"
    torch.cuda.set_device(0)
    dcfg, mcfg, ncfg = cfg["data"], cfg["model"], cfg["model"]["nerf"]
    if args.synthetic:
        import bench
        tab_ts, tab_pos, tab_quat, Kinv, height, width = data.load_trajectory_camera(None, bench.synthetic_scene(), args.height, args.width)
    else:
        root = args.dataset_dir or dcfg["dataset_directory"]
        tab_ts, tab_pos, tab_quat, Kinv, height, width = data.load_trajectory_camera(root, None, args.height, args.width)
    rcfg = config.render_cfg(cfg, tab_pos)
    sd = torch.load(ckpt, map_location="cpu", weights_only=False)["state_dict"]
    arch = ncfg.get("arch", "ngp")
    if args.normals and arch != "ngp":
        raise SystemExit("--normals: arch ngp only")
    if args.normals and args.stage:
        raise SystemExit("--normals renders along the trajectory; it has no meaning with --stage")
    fld, r = config.make_renderer(ncfg, rcfg, checkpoint.radiance_dim(sd, arch), dev)
    bkgd = checkpoint.load_render_state(sd, fld, r, arch)

    os.makedirs(args.out, exist_ok=True)
    from PIL import Image
    if args.stage:
        if args.synthetic:
            raise SystemExit("--stage needs a dataset directory with a views/ folder")
        posed = data.load_eval_views(root, args.stage, dcfg, cfg.get("eval_target"))      # datamodule.py:100-134
        save = os.path.join(args.out, "predictions") if mcfg.get("eval_save_pred_intensity_img") else None
        m = evaluation.evaluate_posed_images(r, posed, bkgd, chunk=args.chunk, save_dir=save)
        for sid, (l1v, ps), ss in zip(posed["sample_id"], m["per_view"].tolist(), m["per_view_ssim"].tolist()):
            print(f"{args.stage} view {sid}: l1 {l1v:.5f}  psnr {ps:.2f} dB  ssim {ss:.4f}")
        np.savez(os.path.join(args.out, f"{args.stage}_metrics.npz"), sample_id=np.array(posed["sample_id"]),
                 l1_psnr=m["per_view"].numpy(), ssim=m["per_view_ssim"].numpy())
        print(f"{args.stage}: {m['n_views']} views, mean l1 {m['l1']:.5f}, mean PSNR {m['psnr']:.2f} dB, "
              f"mean SSIM {m['ssim']:.4f}", flush=True)
        return
    Kinv_d = Kinv.to(dev, torch.float32)
    idx = list(range(0, tab_ts.shape[0], max(1, args.every)))
    pos_all, rot_all = ops.trajectory(tab_ts[idx].to(dev, torch.float64), tab_ts.to(dev), tab_pos.to(dev), tab_quat.to(dev))
    imgs, opacs, depths, scores, normals = [], [], [], [], []
    if args.normals:
        os.makedirs(os.path.join(args.out, "normals"), exist_ok=True)
    for k, i in enumerate(idx):
        img, opac, depth = evaluation.render_image(r, Kinv_d, pos_all[k], rot_all[k], height, width, bkgd=bkgd, chunk=args.chunk)
        imgs.append(img.cpu()); opacs.append(opac.cpu()); depths.append(depth.cpu())
        shown = img
        if args.gt_dir:
            gt = torch.from_numpy(np.load(os.path.join(args.gt_dir, f"{i}.npy"))).to(dev, torch.float32)
            shown = evaluation.affine_align_log(img, gt + rcfg.min_modeled_intensity)
            scores.append(evaluation.psnr(shown, gt + rcfg.min_modeled_intensity, 1.0))
            print(f"view {i}: PSNR {scores[-1]:.2f} dB", flush=True)
        u8 = (shown * args.gain).clamp(0, 1).mul(255).round().byte().cpu().numpy()
        if u8.ndim == 3:
            u8 = np.transpose(u8, (1, 2, 0))
        Image.fromarray(u8, mode="L" if u8.ndim == 2 else "RGB").save(os.path.join(args.out, f"{i}.png"))
        if args.normals:
            nrm, n_opac = evaluation.render_normal_image(r, Kinv_d, pos_all[k], rot_all[k], height, width, chunk=args.chunk)
            normals.append(nrm.cpu())
            Image.fromarray(evaluation.normal_png(nrm, n_opac).numpy(), mode="RGB").save(
                os.path.join(args.out, "normals", f"{i}.png"))
    extra = dict(normal=torch.stack(normals).numpy()) if args.normals else {}
    np.savez(os.path.join(args.out, "views.npz"), index=np.array(idx), intensity=torch.stack(imgs).numpy(),
             opacity=torch.stack(opacs).numpy(), depth=torch.stack(depths).numpy(), **extra)
    msg = f"{len(idx)} views of {height} x {width} written to {args.out}"
    if scores:
        msg += f"; mean PSNR {sum(scores) / len(scores):.2f} dB"
    print(msg, flush=True)


if __name__ == "__main__":
    main()
