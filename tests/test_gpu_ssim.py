"""GPU: SSIM of the evaluation epochs on the HIP kernel (csrc/ren_metrics.hip) against the float64 restatement of
torchmetrics.functional.ssim as the reference calls it (loss_metric/metric.py:74-81; tests/ssim_reference.py), through
evaluation.evaluate_posed_images (one and two ranks, robust_e_nerf.py:684-696), the prediction images
(robust_e_nerf.py:736-780) and the CLIs."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO
import ssim_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _planes(P, H, W, seed, data_range):
    """targets in (1e-3, data_range) with some values above it; predictions = noisy targets; plane 1 (if any) lives near
    1e-3, the last plane (P > 2) is constant"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.rand(P, H, W, generator=g, device=DEV) * 1.15 * data_range + 1e-3
    p = (t + 0.08 * data_range * torch.randn(P, H, W, generator=g, device=DEV)).clamp_min(1e-4)
    if P > 1:
        t[1] = 1e-3 * (1 + 0.5 * torch.rand(H, W, generator=g, device=DEV))
        p[1] = t[1] * (1 + 0.2 * torch.randn(H, W, generator=g, device=DEV))
    if P > 2:
        t[-1], p[-1] = 0.5 * data_range, 0.5 * data_range
    return p.contiguous(), t.contiguous()


CASES = [((11, 11), 1, 1.0), ((11, 12), 3, 0.8), ((17, 300), 7, 1.0), ((260, 346), 3, 0.8), ((480, 640), 1, 1.0),
         ((480, 640), 3, 0.8), ((800, 800), 3, 1.0), ((75, 139), 7, 0.8)]


@pytest.mark.parametrize("shape,P,data_range", CASES)
def test_ssim_planes_match_the_float64_restatement(shape, P, data_range):
    from robust_e_nerf_amd import ops
    H, W = shape
    p, t = _planes(P, H, W, H * 7 + W + P, data_range)
    got = ops.ssim_planes(p, t, data_range)
    want = ref.ssim_planes_banded(p, t, data_range)
    err = float((got - want).abs().max())
    print(f"{H} x {W} x {P} planes, data_range {data_range}: max |kernel - float64| = {err:.2e}")
    assert got.dtype == torch.float64 and got.shape == (P,)
    assert err <= 1e-9, (got, want)
    if P > 2:
        assert abs(float(got[-1]) - 1.0) <= 1e-12                  # constant plane, equal images
    again = ops.ssim_planes(p, t, data_range)
    assert torch.equal(got, again)                                # no atomics: bitwise repeatable


def test_ssim_of_identical_images_is_one():
    from robust_e_nerf_amd import ops
    for (H, W) in ((11, 11), (64, 80), (260, 346)):
        _, t = _planes(3, H, W, H + W, 1.0)
        got = ops.ssim_planes(t, t, 1.0)
        assert float((got - 1.0).abs().max()) <= 1e-12, got


def test_ssim_views_and_channels():
    """evaluation.ssim: (H, W) and (C, H, W) are one view, (V, C, H, W) and batched (V, H, W) are V views; a view's value is
    the mean of its channels' values"""
    from robust_e_nerf_amd import evaluation, ops
    p, t = _planes(6, 40, 52, 11, 1.0)
    planes = ops.ssim_planes(p, t, 1.0)
    assert torch.equal(evaluation.ssim(p[0], t[0], 1.0), planes[:1])
    assert torch.allclose(evaluation.ssim(p[:3], t[:3], 1.0), planes[:3].mean()[None], rtol=0, atol=1e-15)
    assert torch.allclose(evaluation.ssim(p.view(2, 3, 40, 52), t.view(2, 3, 40, 52), 1.0), planes.view(2, 3).mean(1),
                          rtol=0, atol=1e-15)
    assert torch.equal(evaluation.ssim(p, t, 1.0, batched=True), planes)
    assert math.isnan(float(evaluation.ssim(p[0, :10], t[0, :10], 1.0)[0]))          # no valid window: NaN as torchmetrics


# ---- evaluate_posed_images on a simulated dataset in the reference's layout -----------------------------------------------
def _dataset(root):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import e2e_synthetic as e2e
    e2e.simulate(root, n_poses=61, val_views=3)


def _renderer():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import e2e_synthetic as e2e
    from robust_e_nerf_amd import engine
    fld = engine.NGPField(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    fld.flat.copy_((torch.rand(fld.flat.shape, device=DEV, generator=gen) * 2 - 1) * 0.1)
    r = engine.Renderer(fld, engine.RenderCfg(aabb=e2e.AABB, render_step_size=3 * math.sqrt(3) / 1024))
    r.binary.fill_(1)
    return r, torch.tensor([0.55], device=DEV)


def _posed(root):
    import yaml
    from robust_e_nerf_amd import data
    dcfg = yaml.safe_load(open(os.path.join(REPO, "configs", "synthetic_smoke.yaml")))["data"]
    return data.load_eval_views(root, "val", dcfg)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ssim_dataset"))
    _dataset(root)
    return root


def test_evaluate_posed_images_scores_ssim_and_writes_predictions(dataset, tmp_path):
    from PIL import Image
    from robust_e_nerf_amd import evaluation
    r, bk = _renderer()
    posed = _posed(dataset)
    assert len(posed["sample_id"]) == 3
    save = os.path.join(tmp_path, "predictions")
    m = evaluation.evaluate_posed_images(r, posed, bk, save_dir=save)
    # the restatement on the aligned views: ONE fit over all views, then SSIM per view with the target's largest value
    Kinv = torch.linalg.inv(posed["intrinsics"].double()).float().contiguous().to(DEV)
    H, W = posed["img"].shape[-2:]
    preds = [evaluation.render_image(r, Kinv, posed["T_wc_position"][v].to(DEV), posed["T_wc_orientation"][v].to(DEV).contiguous(),
                                     H, W, bk)[0].clamp_min(1e-12) for v in range(3)]
    aligned = torch.stack([evaluation.apply_affine(p_, m["scale"], m["offset"]) for p_ in preds])
    tgts = posed["img"][:3].to(DEV)
    hi, lo = posed["max_normalized_pixel_value"], posed["min_normalized_pixel_value"]
    want = ref.ssim_planes_banded(aligned, tgts, hi).cpu()
    print("per-view SSIM", m["per_view_ssim"].tolist(), "restatement", want.tolist())
    assert m["per_view_ssim"].dtype == torch.float64 and m["per_view_ssim"].shape == (3,)
    assert float((m["per_view_ssim"] - want).abs().max()) <= 1e-9
    assert abs(m["ssim"] - float(want.mean())) <= 1e-9
    # L1 / PSNR: shape, dtype and values as align_and_score gives them, rounded to float32 as before
    sc, _ = evaluation.align_and_score(torch.stack(preds), tgts, hi - lo)
    assert m["per_view"].shape == (3, 2) and m["per_view"].dtype == torch.float32
    assert torch.equal(m["per_view"], sc.to(torch.float32))
    assert abs(m["l1"] - float(m["per_view"][:, 0].double().mean())) <= 1e-6 * m["l1"]
    assert abs(m["psnr"] - float(m["per_view"][:, 1].double().mean())) <= 1e-5
    # the prediction images: round(255 clamp((x - min) / (max - min), 0, 1)), 8-bit grey, one per view
    assert sorted(os.listdir(save)) == sorted(f"{s}.png" for s in posed["sample_id"])
    for v, sid in enumerate(posed["sample_id"]):
        img = Image.open(os.path.join(save, f"{sid}.png"))
        assert img.mode == "L" and img.size == (W, H)
        want_u8 = (255 * ((aligned[v].cpu() - lo) / (hi - lo)).clamp(min=0, max=1)).round().to(torch.uint8).numpy()
        assert np.array_equal(np.asarray(img), want_u8), sid


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, root, out_dir):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from robust_e_nerf_amd import evaluation, parallel
    torch.cuda.set_device(DEV)
    parallel.init_from_env(backend="gloo")
    r, bk = _renderer()
    m = evaluation.evaluate_posed_images(r, _posed(root), bk, rank, 2, save_dir=os.path.join(out_dir, "predictions"))
    torch.save({k: m[k] for k in ("per_view", "per_view_ssim", "ssim", "l1", "psnr")}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_the_same_ssim(dataset, tmp_path):
    """gloo, both ranks on cuda:0: 3 views over 2 ranks (rank 1 renders a wrap-around repeat of view 0, left out of the
    means and the prediction folder); the gathered per-view SSIM equals the single-rank one"""
    from robust_e_nerf_amd import evaluation
    mp.spawn(_worker, args=(_free_port(), dataset, str(tmp_path)), nprocs=2, join=True)
    r, bk = _renderer()
    posed = _posed(dataset)
    one = evaluation.evaluate_posed_images(r, posed, bk)
    for rank in range(2):
        got = torch.load(os.path.join(tmp_path, f"r{rank}.pt"))
        assert got["per_view_ssim"].shape == (3,)
        assert float((got["per_view_ssim"] - one["per_view_ssim"]).abs().max()) <= 1e-10, (got["per_view_ssim"], one["per_view_ssim"])
        assert abs(got["ssim"] - one["ssim"]) <= 1e-10
        assert got["per_view"].shape == (3, 2)
    assert sorted(os.listdir(os.path.join(tmp_path, "predictions"))) == sorted(f"{s}.png" for s in posed["sample_id"])


def test_train_and_render_cli_report_ssim_and_write_predictions(tmp_path):
    """scripts/train.py's validation epoch prints val/ssim after val/psnr and, with model.eval_save_pred_intensity_img,
    writes <out>/predictions/; scripts/render.py --stage val prints the mean SSIM, stores it in val_metrics.npz and writes
    the same folder"""
    import yaml
    ddir = os.path.join(tmp_path, "dataset")
    _dataset(ddir)
    cfg = yaml.safe_load(open(os.path.join(REPO, "configs", "synthetic_smoke.yaml")))
    cfg["data"]["dataset_directory"] = ddir
    cfg["model"]["eval_save_pred_intensity_img"] = True
    cfg["trainer"].update(max_epochs=1, limit_train_batches=20, check_val_every_n_epoch=1)
    path = os.path.join(tmp_path, "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    run = os.path.join(tmp_path, "run")
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train.py"), "--config", path, "--out", run],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    vals = [l for l in out.stdout.splitlines() if "val/psnr" in l]
    assert len(vals) == 1 and "val/ssim" in vals[0], out.stdout[-1500:]
    assert vals[0].index("val/psnr") < vals[0].index("val/ssim")
    ss = float(vals[0].split("val/ssim")[1].split()[0])
    assert math.isfinite(ss) and -1.0 <= ss <= 1.0
    assert len([f for f in os.listdir(os.path.join(run, "predictions")) if f.endswith(".png")]) == 3
    rv = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "render.py"), "--config", path, "--ckpt",
                         os.path.join(run, "last.ckpt"), "--out", os.path.join(tmp_path, "val"), "--stage", "val"],
                        capture_output=True, text=True, timeout=600)
    assert rv.returncode == 0, rv.stderr[-2000:]
    line = [l for l in rv.stdout.splitlines() if l.startswith("val:")][0]
    assert "mean l1" in line and "mean PSNR" in line and "mean SSIM" in line, line
    assert abs(float(line.split("mean SSIM")[1].split()[0]) - ss) < 2e-4, (line, ss)       # same checkpoint, same views
    z = np.load(os.path.join(tmp_path, "val", "val_metrics.npz"))
    assert z["ssim"].shape == (3,) and z["l1_psnr"].shape == (3, 2)
    assert abs(float(z["ssim"].mean()) - ss) < 2e-4
    assert len([f for f in os.listdir(os.path.join(tmp_path, "val", "predictions")) if f.endswith(".png")]) == 3
