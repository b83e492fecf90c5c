"""The reference's YAML schema (configs/train/*.yaml) -> our objects: RenderCfg, TrainCfg, field + renderer, and the fresh
initialisation of a field.  scripts/train.py, scripts/render.py and the tools build their model through these."""
import math

import torch

from . import data, engine, ops, vanilla

SUPPORTED = {  # what the fused kernels implement = what every shipped configs/train/*.yaml selects
    "ngp": {"dir_encoding": {"degree": 4},
            "mlp_base": {"hidden_activation": "softplus", "density_activation": "shifted_trunc_exp", "n_neurons": 64,
                         "n_hidden_layers": 1, "geo_feat_dim": 15, "weight_norm": False},
            "mlp_head": {"hidden_activation": "softplus", "radiance_activation": "softplus", "n_neurons": 64,
                         "n_hidden_layers": 2, "weight_norm": False}},
    "mlp": {"net_depth": 8, "net_width": 256, "skip_layer": 4, "net_depth_condition": 1, "net_width_condition": 128,
            "hidden_activation": "softplus", "density_activation": "shifted_trunc_exp", "radiance_activation": "softplus",
            "pos_encoder_max_deg": 10, "view_encoder_max_deg": 4, "weight_norm": False},
}


# arch ngp: the activation alternatives of the YAML (models/nerf.py:8-29) run on the exact-f32 fused MLP kernels
NGP_ACTIVATIONS = {("mlp_base", "hidden_activation"): ("softplus", "relu"),
                   ("mlp_base", "density_activation"): ("shifted_trunc_exp", "softplus", "shifted_softplus"),
                   ("mlp_head", "hidden_activation"): ("softplus", "relu"),
                   ("mlp_head", "radiance_activation"): ("softplus", "sigmoid")}
# arch mlp: one hidden activation for the whole MLP (external/mlp.py:258); alternatives run on the per-layer launches
MLP_ACTIVATIONS = {("hidden_activation",): ("softplus", "relu"),
                   ("density_activation",): ("shifted_trunc_exp", "softplus", "shifted_softplus"),
                   ("radiance_activation",): ("softplus", "sigmoid")}
ACTIVATIONS = {"ngp": NGP_ACTIVATIONS, "mlp": MLP_ACTIVATIONS}


def activation_fields(ncfg, arch) -> dict:
    """RenderCfg fields for model.nerf.ngp.mlp_base / mlp_head (arch mlp: model.nerf.mlp) activations (absent keys: the
    shipped values)"""
    if arch == "mlp":
        m = ncfg.get("mlp") or {}
        hid = m.get("hidden_activation", "softplus")
        return dict(base_hidden_activation=hid, head_hidden_activation=hid,
                    density_activation=m.get("density_activation", "shifted_trunc_exp"),
                    radiance_activation=m.get("radiance_activation", "softplus"))
    g = ncfg.get("ngp") or {}
    b, h = g.get("mlp_base") or {}, g.get("mlp_head") or {}
    return dict(base_hidden_activation=b.get("hidden_activation", "softplus"),
                density_activation=b.get("density_activation", "shifted_trunc_exp"),
                head_hidden_activation=h.get("hidden_activation", "softplus"),
                radiance_activation=h.get("radiance_activation", "softplus"))


def weight_norm_flags(ncfg, arch):
    """(mlp_base.weight_norm, mlp_head.weight_norm) of model.nerf.ngp; arch mlp: model.nerf.mlp.weight_norm (one flag)"""
    if arch == "mlp":
        return bool((ncfg.get("mlp") or {}).get("weight_norm", False))
    g = ncfg.get("ngp") or {}
    return (bool((g.get("mlp_base") or {}).get("weight_norm", False)), bool((g.get("mlp_head") or {}).get("weight_norm", False)))


def check_supported(ncfg, arch):
    """Fail loudly on hyper-parameters the HIP kernels do not implement (no silent fallback)."""
    def walk(want, got, path):
        for k, v in want.items():
            if k not in got:
                continue                                        # absent key = the reference default = supported value
            if isinstance(v, dict):
                walk(v, got[k] or {}, path + [k])
            elif tuple(path[1:] + [k]) in ACTIVATIONS[arch]:
                if got[k] not in ACTIVATIONS[arch][tuple(path[1:] + [k])]:
                    raise NotImplementedError(f"model.nerf.{'.'.join(path + [k])} = {got[k]!r}: one of "
                                              f"{ACTIVATIONS[arch][tuple(path[1:] + [k])]} (models/nerf.py:17-29)")
            elif k == "weight_norm" and isinstance(got[k], bool):
                continue                                        # a reparametrisation of the trainable block (NGPField / VanillaField)
            elif got[k] != v:
                raise NotImplementedError(f"model.nerf.{'.'.join(path + [k])} = {got[k]!r}: the MI355X kernels implement {v!r} only")
    walk(SUPPORTED[arch], ncfg.get(arch) or {}, [arch])
    pe = (ncfg.get("ngp") or {}).get("pos_encoding") or {}
    if arch == "ngp" and (pe.get("otype", "HashGrid") not in ("HashGrid", "DenseGrid", "TiledGrid")
                          or pe.get("interpolation", "Linear") != "Linear"
                          or pe.get("n_features_per_level", 2) != 2 or pe.get("n_levels", 16) != 16):
        raise NotImplementedError(f"model.nerf.ngp.pos_encoding {pe}: HashGrid / DenseGrid / TiledGrid, Linear interpolation, "
                                  "16 levels x 2 features only")


def render_cfg(cfg, tab_pos, mlp_bf16=False) -> engine.RenderCfg:
    """model.nerf.*, model.min_modeled_intensity and float32_matmul_precision; tab_pos: the camera positions `aabb: auto` spans"""
    mcfg, ncfg = cfg["model"], cfg["model"]["nerf"]
    aabb = ncfg["aabb"]
    if aabb == "auto":                                       # robust_e_nerf.py:206-212
        aabb = torch.cat([tab_pos.min(0).values, tab_pos.max(0).values]).tolist()
    ct = {"aabb": ops.AABB, "tanh": ops.UN_BOUNDED_TANH, "sphere": ops.UN_BOUNDED_SPHERE}[ncfg["contraction_type"]]
    step_size = ncfg["render_step_size"]
    if step_size == "auto":                                  # robust_e_nerf.py:220-226
        step_size = max(aabb[3 + k] - aabb[k] for k in range(3)) * math.sqrt(3) / 1024
    og = ncfg["occ_grid"]
    precision = cfg.get("float32_matmul_precision", "highest")     # scripts/run.py:34-35; what each name runs: RenderCfg.mlp_precision
    if precision not in ("highest", "high", "medium"):
        raise ValueError(f"float32_matmul_precision: {precision!r} (highest | high | medium)")
    mlp_bf16 = mlp_bf16 or precision == "medium"             # bf16 operands, fp32 accumulation (BASELINE configs[2])
    return engine.RenderCfg(aabb=tuple(float(v) for v in aabb), contraction_type=ct, occ_res=(int(og["resolution"]),) * 3,
                            near_plane=ncfg.get("near_plane"), far_plane=ncfg.get("far_plane"),
                            render_step_size=float(step_size), cone_angle=float(ncfg["cone_angle"]),
                            early_stop_eps=float(ncfg["early_stop_eps"]), alpha_thre=float(ncfg["alpha_thre"]),
                            min_modeled_intensity=float(mcfg["min_modeled_intensity"]), occ_thre=float(og["occ_thre"]),
                            ema_decay=float(og["ema_decay"]), warmup_steps=int(og["warmup_steps"]), occ_n=int(og["n"]),
                            mlp_bf16=mlp_bf16, mlp_precision="medium" if mlp_bf16 else precision,
                            **activation_fields(ncfg, ncfg.get("arch", "ngp")))


def train_cfg(cfg) -> engine.TrainCfg:
    """loss.*, optimizer.* and the freeze flags of the event parameters"""
    fn, w, pw, lr = cfg["loss"]["error_fn"], cfg["loss"]["weight"], cfg["loss"]["param_weight"], cfg["optimizer"]["lr"]
    return engine.TrainCfg(
        err_diff=fn["log_intensity_diff"], w_diff=float(w["log_intensity_diff"]), pw_diff=pw.get("log_intensity_diff"),
        err_grad=fn["log_intensity_grad"], w_grad=float(w["log_intensity_grad"]), pw_grad=pw.get("log_intensity_grad"),
        lr=float(lr["default"]), weight_decay=float(w["nerf_mlp_weight_decay"]),
        # a parameter only with alpha_over_white_bg (robust_e_nerf.py:154-159); without, nothing is composited behind the rays
        # and the loss is masked with is_valid = opacity > 0 (:868-871): mocap-*, office-maze
        bkgd_is_param=data.alpha_over_white_bg_of(cfg["data"]),
        train_contrast_threshold=not cfg["model"]["contrast_threshold"]["freeze"], lr_contrast_threshold=float(lr["contrast_threshold"]),
        train_refractory_period=not cfg["model"]["refractory_period"]["freeze"],
        relative_lr_refractory_period=float(cfg["optimizer"]["relative_lr"]["refractory_period"]))


def make_renderer(ncfg, rcfg, C, device):
    """(field, renderer) of model.nerf.arch with C radiance channels; the parameters come from init_field() or a checkpoint"""
    arch = ncfg.get("arch", "ngp")
    check_supported(ncfg, arch)
    if arch == "mlp":
        fld = vanilla.VanillaField(device, C, weight_norm=weight_norm_flags(ncfg, arch))
        return fld, vanilla.VanillaRenderer(fld, rcfg)
    fld = engine.NGPField(device, C, (ncfg.get("ngp") or {}).get("pos_encoding"), weight_norm=weight_norm_flags(ncfg, arch))
    return fld, engine.Renderer(fld, rcfg)


def init_field(fld, arch, C, generator):
    """Fresh parameters.  The draws keep one order, so that a seed gives one model: arch ngp the hash table, then weight and
    bias of base.w0, base.wo, head.w0, head.w1, head.wo; arch mlp weight and bias per layer of vanilla.layer_shapes(C)."""
    def lin(o, i):                                           # nn.Linear default init (hidden_init=None, ngp.py:179-185)
        b = 1 / math.sqrt(i)
        return (torch.rand(o, i, generator=generator) * 2 - 1) * b, (torch.rand(o, generator=generator) * 2 - 1) * b
    if arch == "mlp":
        return fld.load({k: v for name, o, i in vanilla.layer_shapes(C) for k, v in zip((name + ".weight", name + ".bias"), lin(o, i))})
    p = {"hash": (torch.rand(fld.n_table, generator=generator) * 2 - 1) * 1e-4}          # tcnn grid init U(+-1e-4)
    for k, (o, i) in {"base.w0": (64, 32), "base.wo": (16, 64), "head.w0": (64, 31), "head.w1": (64, 64), "head.wo": (C, 64)}.items():
        p[k], p[k.replace(".w", ".b")] = lin(o, i)
    fld.load(p)
