#!/usr/bin/env python
"""Minimal trainer shell over the HIP hot path, driven by the reference's YAML schema.

    python scripts/train.py --config /path/to/configs/train/synthetic.yaml [--dataset-dir DIR] [--out DIR]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/train.py --config ...

Replaces ``scripts/run.py`` + the PyTorch-Lightning fit loop for training (robust_e_nerf/models/robust_e_nerf.py:
301-517,782-950): epochs x ``limit_train_batches`` steps, MultiStepLR stepped per epoch, occupancy-grid update
every step, dynamic event batch size from the ray-sample budget, one process per GPU with an RCCL all-reduce of
the flat gradient.  Checkpoints carry the reference's state-dict key names so weights move both ways.
``--synthetic N`` trains on the benchmark's synthetic orbit instead of a dataset directory.
"""
import argparse
import math
import os
import sys
import time

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def softplus_inv(y):
    return float(y + math.log(-math.expm1(-y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--dataset-dir")
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic events (no dataset directory)")
    ap.add_argument("--out", default="runs/train")
    ap.add_argument("--max-epochs", type=int)
    ap.add_argument("--limit-train-batches", type=int)
    ap.add_argument("--resume")
    ap.add_argument("--mlp-bf16", action="store_true",
                    help="bf16 MLP operands, fp32 accumulate / composite (same as float32_matmul_precision: medium)")
    ap.add_argument("--accumulate-grad-batches", type=int, help="overrides trainer.accumulate_grad_batches")
    ap.add_argument("--batch-size-quantum", type=int, default=1,
                    help="round the dynamic batch size (robust_e_nerf.py:907-950) DOWN to a multiple of this many events: step "
                         "shapes then repeat and engine.Trainer replays a captured hipGraph instead of enqueuing ~80 launches "
                         "(1 = the reference's exact int(budget / mean samples per ray), the default)")
    ap.add_argument("--no-validation", action="store_true", help="skip the validation epochs over views/transforms_val.json")
    ap.add_argument("--limit-val-batches", type=int, help="validate on the first N views only")
    ap.add_argument("--event-support-us", type=float,
                    help="noise filter before the table is built (data.filter_events): drop an event without another event at one "
                         "of its eight neighbouring pixels in the D microseconds up to it (off by default)")
    ap.add_argument("--hot-pixel-sigma", type=float,
                    help="noise filter: drop the events of pixels that hold more than mean + K standard deviations of the "
                         "per-pixel event count, and do not let them support their neighbours (off by default)")
    args = ap.parse_args()
    cfg = yaml.safe_load(open(args.config))
    rank, local_rank, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl")
    dev = f"cuda:{local_rank}"
    torch.cuda.set_device(local_rank)
    seed = cfg.get("seed") or 0
    torch.manual_seed(seed)

    from robust_e_nerf_amd import checkpoint, config, data, engine

    # ---- data: event table in HBM, poses, calibration --------------------------------------------------
    dcfg, mcfg, ncfg = cfg["data"], cfg["model"], cfg["model"]["nerf"]
    if args.synthetic:
        import bench
        tab_ts, tab_pos, tab_quat, Kinv = (torch.from_numpy(a) for a in bench.synthetic_scene())
        ev = bench.synthetic_events(args.synthetic, int(tab_ts[-1]), seed=1)
        events = {k: torch.from_numpy(ev[k]) for k in ("position", "start_ts", "end_ts", "num_pos", "num_neg")}
        pos_ct, neg_ct, tau0, tau_max = 0.25, 0.25, 0.0, torch.tensor(1e5, dtype=torch.float64)
    else:
        root = args.dataset_dir or dcfg["dataset_directory"]
        # the event table is built (or read from its caches) on the device together with tau_max: one sort, two launches
        event_filter = None
        if args.event_support_us is not None or args.hot_pixel_sigma is not None:         # timestamps are nanoseconds
            event_filter = dict(dt=None if args.event_support_us is None else int(round(args.event_support_us * 1e3)),
                                hot_sigma=args.hot_pixel_sigma)
        events, tau_max = data.load_event_table(root, dcfg.get("train_dataset_perm_seed"), device=dev, event_filter=event_filter)
        tau_max = tau_max.to(torch.float64)
        tab_ts, tab_pos, tab_quat = data.load_camera_poses(root)
        calib = data.load_calibration(root)
        Kinv = calib["Kinv"]
        pos_ct, neg_ct = float(calib["pos_contrast_threshold"]), float(calib["neg_contrast_threshold"])
        tau0 = float(calib["refractory_period"])
        if not (0 <= tau0 < float(tau_max)):               # event_generation_params.py:89,113-130
            import warnings
            warnings.warn(f"Calibrated refractory period ({tau0}) is not in [0, max. refractory period = {float(tau_max)}): "
                          f"redefining it to 0.999 of the max. refractory period")
            tau0 = 0.999 * float(tau_max)
    budget = int(dcfg["train_eff_ray_sample_batch_size"])
    batch_size = max(1, int(dcfg["train_init_eff_batch_size"]) // world)
    batcher = data.EventBatcher(events, batch_size, dev, seed=seed, rank=rank,
                                dataset_ratio=dcfg.get("train_dataset_ratio", 1.0))

    # ---- model ----------------------------------------------------------------------------------------------
    rcfg = config.render_cfg(cfg, tab_pos, mlp_bf16=args.mlp_bf16)
    arch = ncfg.get("arch", "ngp")
    C = 3 if "channel_idx" in events else 1                 # Bayer sensor -> radiance_dim 3 (robust_e_nerf.py:230-233)
    fld, renderer = config.make_renderer(ncfg, rcfg, C, dev)
    config.init_field(fld, arch, C, torch.Generator().manual_seed(seed))
    tcfg = config.train_cfg(cfg)
    tau_raw = float(tau_max) * torch.logit(torch.tensor(max(tau0, 1e-9) / float(tau_max), dtype=torch.float64)) if tau0 > 0 \
        else torch.tensor(-1e30, dtype=torch.float64)
    tr = engine.Trainer(renderer, tcfg, Kinv=Kinv, tab_ts=tab_ts, tab_pos=tab_pos, tab_quat=tab_quat,
                        p2n_raw=torch.tensor(softplus_inv(pos_ct / neg_ct)), neg_ct=torch.tensor(neg_ct),
                        tau_raw=tau_raw, tau_max=tau_max, bkgd_raw=torch.tensor([softplus_inv(1.0)] * fld.C),
                        world_size=world, process_group=None)
    start_epoch, start_step = 0, 0
    resume_rng = None
    if args.resume:
        ck = torch.load(args.resume, map_location="cpu", weights_only=False)
        checkpoint.load_train_state(ck["state_dict"], tr, arch)
        if "optimizer_state" in ck:                          # absent in a reference (PL) checkpoint: fresh moments then
            tr.load_optimizer_state_dict(ck["optimizer_state"])
            start_epoch, start_step = int(ck["epoch"]) + 1, int(ck["global_step"])
            if rank == 0:
                print(f"resumed {args.resume}: epoch {start_epoch}, global_step {start_step}, raw C_p/C_n ratio "
                      f"{float(tr.ct[0]):.4f}, tau {tr.tau:.6g}", flush=True)
            if "batch_size" in ck:
                batch_size = int(ck["batch_size"])
                batcher.set_batch_size(batch_size)
            resume_rng = ck.get("rng_state")

    # ---- fit loop ---------------------------------------------------------------------------------------------
    tcf, sched = cfg["trainer"], cfg["lr_scheduler"]["multi_step_lr"]
    max_epochs = args.max_epochs or int(tcf["max_epochs"])
    per_epoch = args.limit_train_batches or int(tcf["limit_train_batches"])
    log_every = int(tcf.get("log_every_n_steps", 100))
    accum = int(args.accumulate_grad_batches or tcf.get("accumulate_grad_batches", 1) or 1)
    # a new batch size takes effect two batches later (one batch is already pre-fetched, robust_e_nerf.py:925-931)
    from collections import deque
    pending = deque([batch_size])
    jgen = torch.Generator(device=dev).manual_seed(seed + 17 + rank)
    if resume_rng is not None:
        # continue the random streams (event indices / normalized samplers, ray jitters, occupancy-grid refresh) and the
        # in-flight batch-size queue where the checkpointed run left them: a resumed run then equals the uninterrupted one
        # instead of replaying epoch 0's draws.  Every rank's generator states are in the checkpoint (gathered to rank 0 when
        # it was written); a checkpoint written by a different world size re-seeds the ranks it has no state for.
        per_rank = resume_rng.get("per_rank")
        if per_rank is None:                                    # round-3 checkpoints: rank 0's states only
            per_rank = [{"batcher": resume_rng["batcher"], "jitter": resume_rng["jitter"]}]
        if rank < len(per_rank):
            batcher.gen.set_state(per_rank[rank]["batcher"])
            jgen.set_state(per_rank[rank]["jitter"])
        else:
            batcher.gen.manual_seed(seed + rank + 7919 * start_epoch)
            jgen.manual_seed(seed + 17 + rank + 7919 * start_epoch)
            print(f"rank {rank}: no random-stream state in {args.resume} (written by {len(per_rank)} rank(s)): re-seeded",
                  flush=True)
        if resume_rng.get("occ") is not None:                   # identical on every rank by construction
            renderer._occ_gen = torch.Generator(device=dev)
            renderer._occ_gen.set_state(resume_rng["occ"])
        if resume_rng.get("pending"):
            pending = deque(int(b) for b in resume_rng["pending"])
    os.makedirs(args.out, exist_ok=True)
    val_views, val_every = None, int(tcf.get("check_val_every_n_epoch", 1) or 1)
    if not args.synthetic and not args.no_validation and \
            data.has_posed_images(root, data.eval_transforms_stage("val", cfg.get("eval_target"))):
        # datamodule.py:100-134: eval_target's views, eval_dataset_perm_seed, first val_dataset_ratio (x val_eff_batch_size)
        val_views = data.load_eval_views(root, "val", dcfg, cfg.get("eval_target"))
        if rank == 0:
            print(f"validation: {len(val_views['sample_id'])} posed views every {val_every} epoch(s)", flush=True)
    step, t0, rays = start_step, time.perf_counter(), 0
    for epoch in range(start_epoch, max_epochs):
        tr.set_epoch(epoch, tuple(sched["milestones"]), float(sched["gamma"]))
        for bi in range(per_epoch):
            batch = batcher.next()
            B = batch["position"].shape[0]
            j = torch.rand(3, B, device=dev, generator=jgen)
            loss, aux = tr.step(batch, j[0], j[1], global_step=step, jitter_grad=j[2], batch_index=bi,
                                accumulate_grad_batches=accum)
            rays += (3 if tcfg.w_grad > 0 else 2) * B
            nb = tr.update_train_batch_size(aux, budget, accum, bi)              # robust_e_nerf.py:907-950
            if nb is not None:
                pending.append(nb)
            nxt = pending.popleft() if len(pending) > 1 else pending[0]
            if args.batch_size_quantum > 1:
                nxt = max(args.batch_size_quantum, nxt // args.batch_size_quantum * args.batch_size_quantum)
            batcher.set_batch_size(nxt)
            step += (bi + 1) % accum == 0                                        # global_step counts optimiser steps
            if rank == 0 and (bi + 1) % accum == 0 and step % log_every == 0:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"epoch {epoch} step {step}  loss {float(loss):.5f}  batch {B}  samples/ray {aux['n'] / max(aux['rays'], 1):.1f}"
                      f"  {rays * world / dt / 1e6:.2f} M rays/s  mem {torch.cuda.memory_allocated() / 2**30:.1f}/"
                      f"{torch.cuda.memory_reserved() / 2**30:.1f} GiB" +
                      (f"  device counts ({tr.device_count_overflows} repeated passes)" if tr.device_counts_ok() else "") +
                      (f"  graph replays {tr.graph_replays} / captures {tr.graph_captures}" if tr.graph_replays else ""), flush=True)
                t0, rays = time.perf_counter(), 0
        # ---- validation epoch (trainer.check_val_every_n_epoch, synthetic.yaml:152-154; robust_e_nerf.py:519-571):
        # the dataset's posed validation views, rendered by all ranks, aligned and scored as the reference does
        if val_views is not None and (epoch + 1) % val_every == 0:
            from robust_e_nerf_amd import evaluation
            bk = torch.nn.functional.softplus(tr.small[: fld.C]) if tcfg.bkgd_is_param else None
            # model.eval_save_pred_intensity_img: the aligned predictions in <out>/predictions/, overwritten every epoch (:736-780)
            save = os.path.join(args.out, "predictions") if mcfg.get("eval_save_pred_intensity_img") else None
            vm = evaluation.evaluate_posed_images(renderer, val_views, bk, rank, world, limit=args.limit_val_batches,
                                                  save_dir=save)
            if rank == 0:
                print(f"epoch {epoch} validation over {vm['n_views']} views: val/l1 {vm['l1']:.5f}  val/psnr {vm['psnr']:.3f} dB"
                      f"  val/ssim {vm['ssim']:.4f}", flush=True)
        mine_rng = {"batcher": batcher.gen.get_state().cpu(), "jitter": jgen.get_state().cpu()}
        rank_rng = [mine_rng]
        if world > 1:                                           # every rank's generator states travel to rank 0's file
            rank_rng = [None] * world
            dist.all_gather_object(rank_rng, mine_rng)
        if rank == 0:
            rng = {"per_rank": rank_rng, "pending": list(pending),
                   "occ": renderer._occ_gen.get_state() if renderer._occ_gen is not None else None}
            torch.save({"state_dict": checkpoint.model_state_dict(tr, arch), "epoch": epoch, "global_step": step,
                        "optimizer_state": tr.optimizer_state_dict(), "batch_size": batcher.batch_size, "rng_state": rng},
                       os.path.join(args.out, "last.ckpt"))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
