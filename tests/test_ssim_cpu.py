"""CPU: the float64 SSIM restatement the GPU tests hold the kernel to, the C-ABI entry points of csrc/ren_metrics.hip
(exported, bound, argument validation before any launch) and scripts/render.py's config path for the reference's test
YAMLs (loss_metric/metric.py:74-81, robust_e_nerf.py:684-780, configs/test/*.yaml)."""
import ctypes
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
import ssim_reference as ref


def _pair(P, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(P, H, W, generator=g, dtype=torch.float64) * 0.9 + 1e-3
    p = (t + 0.1 * torch.randn(P, H, W, generator=g, dtype=torch.float64)).clamp_min(1e-3)
    return p, t


@pytest.mark.parametrize("H,W", [(11, 11), (11, 12), (13, 17), (23, 19)])
def test_banded_restatement_equals_sliding_windows_and_padded_convolution(H, W):
    p, t = _pair(2, H, W, H * 100 + W)
    for rng in (1.0, 0.8):
        banded = ref.ssim_planes_banded(p, t, rng)
        conv = ref.ssim_planes_padded_conv(p, t, rng)
        direct = torch.tensor([ref.ssim_plane_direct(p[i].numpy(), t[i].numpy(), rng) for i in range(2)], dtype=torch.float64)
        assert float((banded - direct).abs().max()) < 1e-13, (banded, direct)
        assert float((banded - conv).abs().max()) < 1e-13, (banded, conv)


def test_banded_restatement_at_image_size_and_identity():
    p, t = _pair(1, 120, 160, 3)
    assert float((ref.ssim_planes_banded(p, t, 1.0) - ref.ssim_planes_padded_conv(p, t, 1.0)).abs().max()) < 1e-13
    assert abs(float(ref.ssim_planes_banded(t, t, 1.0)[0]) - 1.0) < 1e-14
    assert abs(float(ref.gauss().sum()) - 1.0) < 1e-15 and ref.gauss().shape == (11,)


@pytest.fixture(scope="module")
def lib():
    from robust_e_nerf_amd import build
    build.build()
    from robust_e_nerf_amd import _lib
    return _lib.load()


def test_ssim_entry_points_are_exported_and_bound(lib):
    from robust_e_nerf_amd import _lib
    for name in ("ren_ssim_planes", "ren_ssim_scratch_doubles"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # one double per 64 x 64 tile of the valid region of every plane; no valid window -> 0
    assert lib.ren_ssim_scratch_doubles(3, 11, 11) == 3
    assert lib.ren_ssim_scratch_doubles(2, 74, 75) == 2 * 2
    assert lib.ren_ssim_scratch_doubles(600, 800, 800) == 600 * 13 * 13
    assert lib.ren_ssim_scratch_doubles(1, 10, 100) == 0 and lib.ren_ssim_scratch_doubles(0, 100, 100) == 0


def test_ssim_argument_validation_needs_no_gpu(lib):
    """REN_ERR_BAD_ARG is returned before any launch: host buffers stand in for device memory and are never touched"""
    from robust_e_nerf_amd import _lib
    buf = (ctypes.c_double * 64)()
    fp = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(pred=fp, target=fp, P=1, H=11, W=11, rng=1.0, out=fp, scratch=fp)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ren_ssim_planes(a["pred"], a["target"], a["P"], a["H"], a["W"], a["rng"], a["out"], a["scratch"], None)
    bad = [dict(pred=None), dict(target=None), dict(out=None), dict(scratch=None), dict(P=0), dict(P=-3), dict(H=10),
           dict(W=10), dict(H=0), dict(W=-1), dict(rng=0.0), dict(rng=-1.0), dict(rng=math.inf), dict(rng=-math.inf),
           dict(rng=math.nan)]
    for kw in bad:
        assert call(**kw) == _lib.REN_ERR_BAD_ARG, kw
    from robust_e_nerf_amd import ops
    with pytest.raises(ValueError):                                   # no CPU fallback on the product path
        ops.ssim_planes(torch.rand(1, 16, 16), torch.rand(1, 16, 16), 1.0)
    with pytest.raises(ValueError):
        ops.ssim_planes(torch.rand(16, 16), torch.rand(16, 16), 1.0)


REFERENCE_TEST_CONFIGS = sorted(glob.glob(os.path.join(GOLDEN, "configs_test", "*.yaml")))


def test_render_cli_accepts_the_reference_test_configs():
    """the reference's four test YAMLs (configs/test/*.yaml, fixtures in tests/golden/configs_test) pass render.py's schema
    check, name their checkpoint in model.checkpoint_filepath (the --ckpt fallback) and ask for the prediction images"""
    assert len(REFERENCE_TEST_CONFIGS) == 4
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import render
    for path in REFERENCE_TEST_CONFIGS:
        cfg, ckpt = render.load_config(path)
        assert ckpt == cfg["model"]["checkpoint_filepath"] and ckpt.endswith(".ckpt"), path
        assert cfg["model"]["eval_save_pred_intensity_img"] is True, path
        assert render.load_config(path, "given.ckpt")[1] == "given.ckpt"


def test_render_cli_without_a_checkpoint_fails_loudly(tmp_path):
    import yaml
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import render
    cfg = yaml.safe_load(open(os.path.join(REPO, "configs", "synthetic_smoke.yaml")))
    cfg["model"].pop("checkpoint_filepath", None)
    path = os.path.join(tmp_path, "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    with pytest.raises(SystemExit):
        render.load_config(path)
