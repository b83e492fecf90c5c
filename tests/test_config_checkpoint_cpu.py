"""robust_e_nerf_amd.config / robust_e_nerf_amd.checkpoint on the CPU: the YAML schema -> RenderCfg / TrainCfg, the order in
which a fresh field draws its parameters, and the state-dict format a checkpoint carries.  No GPU, no library load."""
import copy
import json
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import yaml

from robust_e_nerf_amd import checkpoint, config, ops, vanilla

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB_POS = torch.tensor([[-1.0, -2.0, 0.5], [3.0, 0.25, 1.5]])            # `aabb: auto` = (-1, -2, 0.5, 3, 0.25, 1.5): extents 4, 2.25, 1
UNIT = math.sqrt(3) / 1024                                               # render_step_size: auto = largest extent x this

# what every one of the six YAMLs sets alike ...
RENDER_COMMON = dict(early_stop_eps=1e-4, alpha_thre=0.0, min_modeled_intensity=1e-3, occ_thre=1e-2, ema_decay=0.95,
                     warmup_steps=256, occ_n=16, mlp_bf16=False, mlp_precision="highest", base_hidden_activation="softplus",
                     density_activation="shifted_trunc_exp", head_hidden_activation="softplus", radiance_activation="softplus")
TRAIN_COMMON = dict(err_diff="mse", w_diff=1.0, pw_diff="mean_contrast_reciprocal_sq", err_grad="mape", pw_grad=None, lr=0.01,
                    weight_decay=1e-6, lr_contrast_threshold=0.1, relative_lr_refractory_period=50.0)
# ... and what they set differently, read off the files: (RenderCfg fields, largest aabb extent, TrainCfg fields)
SPHERE = dict(contraction_type=ops.UN_BOUNDED_SPHERE, occ_res=(256,) * 3, cone_angle=0.004)
BOX = dict(aabb=(-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), contraction_type=ops.AABB, occ_res=(128,) * 3, near_plane=None,
           far_plane=None, cone_angle=0.0)
REAL = dict(w_grad=1e-3, bkgd_is_param=False, train_contrast_threshold=True, train_refractory_period=True)
EXPECTED = {
    "synthetic_smoke": (BOX, 3.0, dict(w_grad=1e-3, bkgd_is_param=True, train_contrast_threshold=True,
                                       train_refractory_period=False)),
    "tumvie_settings_smoke": (dict(SPHERE, aabb=(-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), near_plane=0.05, far_plane=6.0), 3.0, REAL),
    "mocap-1d-trans": (dict(SPHERE, aabb=(-0.5, -0.5, 0.6, 0.5, 0.5, 1.6), near_plane=0.05, far_plane=3.0), 1.0, REAL),
    "mocap-desk2": (dict(SPHERE, aabb=(0.5, -2.1, 0.6, 2.0, -0.6, 1.6), near_plane=0.05, far_plane=3.0), 1.5, REAL),
    "office-maze": (dict(SPHERE, aabb=(-2.3, -3.2, 0.0, 1.7, 2.8, 3.0), near_plane=0.01, far_plane=4.0), 6.0, REAL),
    "synthetic": (BOX, 3.0, dict(w_grad=0.0, bkgd_is_param=True, train_contrast_threshold=False,
                                 train_refractory_period=False)),
}


def load_cfg(name):
    if name.endswith("_smoke"):
        return yaml.safe_load(open(os.path.join(REPO, "configs", name + ".yaml")))
    return json.loads(str(np.load(os.path.join(REPO, "tests", "golden", "train_configs.npz"))[name]))


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_render_and_train_cfg_from_yaml(name):
    cfg = load_cfg(name)
    want_r, extent, want_t = EXPECTED[name]
    rcfg, tcfg = config.render_cfg(cfg, TAB_POS), config.train_cfg(cfg)
    for k, v in dict(RENDER_COMMON, **want_r).items():
        assert getattr(rcfg, k) == v and type(getattr(rcfg, k)) is type(v), (k, getattr(rcfg, k), v)
    assert rcfg.render_step_size == pytest.approx(extent * UNIT, rel=1e-12)
    for k, v in dict(TRAIN_COMMON, **want_t).items():
        assert getattr(tcfg, k) == v and type(getattr(tcfg, k)) is type(v), (k, getattr(tcfg, k), v)
    # aabb: auto spans the pose table, and the auto step follows it; everything else as before
    auto = copy.deepcopy(cfg)
    auto["model"]["nerf"]["aabb"] = "auto"
    acfg = config.render_cfg(auto, TAB_POS)
    assert acfg.aabb == (-1.0, -2.0, 0.5, 3.0, 0.25, 1.5) and acfg.render_step_size == pytest.approx(4.0 * UNIT, rel=1e-12)
    assert all(getattr(acfg, k) == v for k, v in dict(RENDER_COMMON, **want_r).items() if k != "aabb")
    # an explicit step size is taken as it stands
    auto["model"]["nerf"]["render_step_size"] = 0.005
    assert config.render_cfg(auto, TAB_POS).render_step_size == 0.005


def test_float32_matmul_precision():
    cfg = load_cfg("synthetic_smoke")
    assert "float32_matmul_precision" not in cfg and config.render_cfg(cfg, TAB_POS).mlp_precision == "highest"
    cfg["float32_matmul_precision"] = "high"
    r = config.render_cfg(cfg, TAB_POS)
    assert (r.mlp_precision, r.mlp_bf16) == ("high", False)
    r = config.render_cfg(cfg, TAB_POS, mlp_bf16=True)                     # scripts/train.py --mlp-bf16
    assert (r.mlp_precision, r.mlp_bf16) == ("medium", True)
    cfg["float32_matmul_precision"] = "medium"
    r = config.render_cfg(cfg, TAB_POS)
    assert (r.mlp_precision, r.mlp_bf16) == ("medium", True)
    cfg["float32_matmul_precision"] = "tf32"
    with pytest.raises(ValueError, match="float32_matmul_precision"):
        config.render_cfg(cfg, TAB_POS)


def test_activation_alternatives_reach_render_cfg():
    cfg = load_cfg("synthetic")
    cfg["model"]["nerf"]["ngp"]["mlp_head"]["radiance_activation"] = "sigmoid"
    cfg["model"]["nerf"]["mlp"]["hidden_activation"] = "relu"
    r = config.render_cfg(cfg, TAB_POS)
    assert (r.radiance_activation, r.base_hidden_activation, r.head_hidden_activation) == ("sigmoid", "softplus", "softplus")
    cfg["model"]["nerf"]["arch"] = "mlp"
    r = config.render_cfg(cfg, TAB_POS)
    assert (r.radiance_activation, r.base_hidden_activation, r.head_hidden_activation) == ("softplus", "relu", "relu")


class RecordingField:
    """what init_field needs of a field: n_table (arch ngp) and load(), which keeps what it was given"""
    n_table = 1000

    def load(self, p):
        self.loaded = p


def _lin(o, i, gen):                                         # nn.Linear default init, as scripts/train.py drew it inline
    b = 1 / math.sqrt(i)
    return (torch.rand(o, i, generator=gen) * 2 - 1) * b, (torch.rand(o, generator=gen) * 2 - 1) * b


@pytest.mark.parametrize("C", [1, 3])
def test_init_field_draws_in_the_order_of_the_inline_initialisation(C):
    """the recipe below is the code scripts/train.py ran before init_field existed: a seed gives the same model, bit for bit"""
    gen = torch.Generator().manual_seed(0)
    want = {"hash": (torch.rand(RecordingField.n_table, generator=gen) * 2 - 1) * 1e-4}
    for k, (o, i) in {"base.w0": (64, 32), "base.wo": (16, 64), "head.w0": (64, 31), "head.w1": (64, 64), "head.wo": (C, 64)}.items():
        want[k], want[k.replace(".w", ".b")] = _lin(o, i, gen)
    fld = RecordingField()
    config.init_field(fld, "ngp", C, torch.Generator().manual_seed(0))
    assert list(fld.loaded) == list(want) and all(torch.equal(fld.loaded[k], want[k]) for k in want)
    assert float(fld.loaded["hash"].abs().max()) <= 1e-4 and fld.loaded["head.wo"].shape == (C, 64)

    gen = torch.Generator().manual_seed(0)
    want = {k: v for name, o, i in vanilla.layer_shapes(C) for k, v in zip((name + ".weight", name + ".bias"), _lin(o, i, gen))}
    fld = RecordingField()
    config.init_field(fld, "mlp", C, torch.Generator().manual_seed(0))
    assert list(fld.loaded) == list(want) and all(torch.equal(fld.loaded[k], want[k]) for k in want)


# ---- the state dict of a checkpoint, on stand-ins with CPU tensors of the real shapes -------------------------------------
REF_FIELD = ("mlp_base.1.hidden_layers.0", "mlp_base.1.output_layer", "mlp_head.hidden_layers.0", "mlp_head.hidden_layers.1",
             "mlp_head.output_layer")                        # the reference's Linear modules, in the order of SHAPES
SHAPES = {"base.w0": (64, 32), "base.wo": (16, 64), "head.w0": (64, 31), "head.w1": (64, 64), "head.wo": (1, 64)}
OCC_RES = (4, 4, 4)
AABB = (-1.0, -2.0, 0.5, 3.0, 0.25, 1.5)


def stand_in_trainer(head_weight_norm=False, bkgd_is_param=True):
    views = {}
    for k, (o, i) in SHAPES.items():
        if head_weight_norm and k.startswith("head"):
            views[k + "_g"], views[k + "_v"] = torch.rand(o, 1), torch.rand(o, i)
        else:
            views[k] = torch.rand(o, i)
        views[k.replace(".w", ".b")] = torch.rand(o)
    loaded = {}
    fld = NS(C=1, table=torch.rand(1000), trainable_views=lambda: views, load=loaded.update, loaded=loaded)
    r = NS(field=fld, cfg=NS(aabb=AABB, occ_res=OCC_RES), occs=torch.rand(64), binary=(torch.rand(64) > 0.5).to(torch.uint8))
    events = []
    return NS(r=r, t=NS(bkgd_is_param=bkgd_is_param), ct=torch.tensor([0.3, 0.0, 0.0, 0.0]), small=torch.tensor([0.5, 0, 0, 0]),
              tau_raw=torch.tensor(-7.0, dtype=torch.float64), load_event_params=lambda *a: events.append(a), events=events)


@pytest.mark.parametrize("head_weight_norm,bkgd_is_param", [(False, True), (True, False)])
def test_model_state_dict_keys_dtypes_shapes(head_weight_norm, bkgd_is_param):
    tr = stand_in_trainer(head_weight_norm, bkgd_is_param)
    sd = checkpoint.model_state_dict(tr, "ngp")
    want = {"contrast_threshold.parametrizations.p2n_contrast_threshold_ratio.original": (torch.float32, (1,)),
            "refractory_period.parametrizations._refractory_period.original": (torch.float64, ()),
            "nerf.occupancy_grid._roi_aabb": (torch.float32, (6,)), "nerf.occupancy_grid._binary": (torch.bool, OCC_RES),
            "nerf.occupancy_grid.resolution": (torch.int32, (3,)), "nerf.occupancy_grid.occs": (torch.float32, (64,)),
            "nerf.radiance_field.aabb": (torch.float32, (6,)), "nerf.radiance_field.mlp_base.0.params": (torch.float32, (1000,))}
    if bkgd_is_param:
        want["nerf.parametrizations.render_bkgd.original"] = (torch.float32, (1,))
    for stem, (k, (o, i)) in zip(REF_FIELD, SHAPES.items()):
        if head_weight_norm and k.startswith("head"):
            want[f"nerf.radiance_field.{stem}.weight_g"] = (torch.float32, (o, 1))
            want[f"nerf.radiance_field.{stem}.weight_v"] = (torch.float32, (o, i))
        else:
            want[f"nerf.radiance_field.{stem}.weight"] = (torch.float32, (o, i))
        want[f"nerf.radiance_field.{stem}.bias"] = (torch.float32, (o,))
    assert set(sd) == set(want), set(sd) ^ set(want)
    for k, (dtype, shape) in want.items():
        assert sd[k].dtype == dtype and tuple(sd[k].shape) == shape and sd[k].device.type == "cpu", k
    assert sd["nerf.occupancy_grid._roi_aabb"].tolist() == pytest.approx(list(AABB))
    assert sd["nerf.occupancy_grid.resolution"].tolist() == list(OCC_RES)
    assert torch.equal(sd["nerf.occupancy_grid._binary"].reshape(-1), tr.r.binary.bool())
    assert torch.equal(sd["nerf.occupancy_grid.occs"], tr.r.occs) and sd["nerf.occupancy_grid.occs"] is not tr.r.occs
    assert float(sd[checkpoint.CT_KEY]) == pytest.approx(0.3) and float(sd[checkpoint.TAU_KEY]) == -7.0
    assert checkpoint.radiance_dim(sd, "ngp") == 1


def test_state_dict_loads_back_and_a_missing_grid_is_refused():
    src = stand_in_trainer(head_weight_norm=True)
    src.small[0] = 0.75
    sd = checkpoint.model_state_dict(src, "ngp")
    dst = stand_in_trainer(head_weight_norm=True)
    checkpoint.load_train_state(sd, dst, "ngp")
    views = src.r.field.trainable_views()
    assert set(dst.r.field.loaded) == set(views) | {"hash"}
    assert all(torch.equal(dst.r.field.loaded[k], v) for k, v in views.items())
    assert torch.equal(dst.r.field.loaded["hash"], src.r.field.table)
    assert torch.equal(dst.r.occs, src.r.occs) and torch.equal(dst.r.binary, src.r.binary)
    assert float(dst.small[0]) == 0.75 and len(dst.events) == 1
    assert float(dst.events[0][0]) == pytest.approx(0.3) and float(dst.events[0][1]) == -7.0
    # the render side: field + binary grid, background through softplus
    dst = stand_in_trainer(head_weight_norm=True)
    bk = checkpoint.load_render_state(sd, dst.r.field, dst.r, "ngp")
    assert torch.equal(dst.r.binary, src.r.binary) and set(dst.r.field.loaded) == set(views) | {"hash"}
    assert bk.shape == (1,) and float(bk) == pytest.approx(math.log1p(math.exp(0.75)))
    no_bk = {k: v for k, v in sd.items() if k != checkpoint.BKGD_KEY}
    assert checkpoint.load_render_state(no_bk, dst.r.field, dst.r, "ngp") is None
    with pytest.raises(KeyError, match="occupancy grid"):
        checkpoint.load_train_state({k: v for k, v in sd.items() if "occupancy_grid" not in k}, stand_in_trainer(True), "ngp")
