"""The reference's state-dict format (VERDICT row f3): its module names for the field, the four persistent buffers of
nerfacc.OccupancyGrid and the three parametrisation keys, so that a checkpoint moves both ways.  One writer, two readers."""
import torch

NGP_KEYS = {"hash": "mlp_base.0.params", "base.w0": "mlp_base.1.hidden_layers.0.weight",
            "base.b0": "mlp_base.1.hidden_layers.0.bias", "base.wo": "mlp_base.1.output_layer.weight",
            "base.bo": "mlp_base.1.output_layer.bias", "head.w0": "mlp_head.hidden_layers.0.weight",
            "head.b0": "mlp_head.hidden_layers.0.bias", "head.w1": "mlp_head.hidden_layers.1.weight",
            "head.b1": "mlp_head.hidden_layers.1.bias", "head.wo": "mlp_head.output_layer.weight",
            "head.bo": "mlp_head.output_layer.bias"}
PREFIX = "nerf.radiance_field."                       # RobustENeRF.nerf (models/nerf.py) . radiance_field
OCC = "nerf.occupancy_grid."                          # NeRF.occupancy_grid = nerfacc.OccupancyGrid (models/nerf.py:98-102)
CT_KEY = "contrast_threshold.parametrizations.p2n_contrast_threshold_ratio.original"
TAU_KEY = "refractory_period.parametrizations._refractory_period.original"
BKGD_KEY = "nerf.parametrizations.render_bkgd.original"   # models/nerf.py:81-88 (softplus-parametrised parameter)


def field_state_dict(fld, arch, aabb):
    """parameters + persistent buffers of the reference's radiance field module (ngp.py:152, mlp.py:217-219,269)"""
    buf = {PREFIX + "aabb": torch.tensor(aabb, dtype=torch.float32)}
    if arch == "mlp":
        buf[PREFIX + "posi_encoder.scales"] = torch.tensor([2 ** i for i in range(10)])
        buf[PREFIX + "view_encoder.scales"] = torch.tensor([2 ** i for i in range(4)])
        return dict(buf, **{PREFIX + k: v.detach().cpu().clone() for k, v in fld.state_dict(trainable=True).items()})
    sd = dict(buf, **{PREFIX + NGP_KEYS["hash"]: fld.table.detach().cpu().clone()})
    for k, v in fld.trainable_views().items():               # weight_norm: "<layer>.weight_g" / ".weight_v" (ngp.py:207-228)
        name = NGP_KEYS[k[:-2]] + k[-2:] if k[-2:] in ("_g", "_v") else NGP_KEYS[k]
        sd[PREFIX + name] = v.detach().cpu().clone()
    return sd


def load_field_state_dict(fld, arch, sd):
    sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    if arch == "mlp":
        fld.load(sd)
    else:
        p = {}
        for ours, theirs in NGP_KEYS.items():
            if theirs in sd:
                p[ours] = sd[theirs]
            else:                                            # a weight-normalised layer (ngp.py:207-228)
                p[ours + "_g"], p[ours + "_v"] = sd[theirs + "_g"], sd[theirs + "_v"]
        fld.load(p)


def model_state_dict(trainer, arch) -> dict:
    """the `state_dict` of a checkpoint: what the reference's RobustENeRF module holds for the same model"""
    r, cfg = trainer.r, trainer.r.cfg
    sd = field_state_dict(r.field, arch, cfg.aabb)
    sd[CT_KEY] = trainer.ct[:1].detach().cpu().clone()
    sd[TAU_KEY] = trainer.tau_raw.detach().clone()
    if trainer.t.bkgd_is_param:
        sd[BKGD_KEY] = trainer.small[: r.field.C].detach().cpu().clone()
    # the persistent buffers of nerfacc 0.3.x's OccupancyGrid (models/nerf.py:98-102; grid_coords / grid_indices are not)
    sd[OCC + "_roi_aabb"] = torch.tensor(cfg.aabb, dtype=torch.float32)
    sd[OCC + "_binary"] = r.binary.detach().cpu().bool().view(*cfg.occ_res)
    sd[OCC + "resolution"] = torch.tensor(cfg.occ_res, dtype=torch.int32)
    sd[OCC + "occs"] = r.occs.detach().cpu().clone()
    return sd


def radiance_dim(sd, arch) -> int:
    """channels of the radiance output layer (1, or 3 for a Bayer sensor: robust_e_nerf.py:230-233)"""
    return int(sd[PREFIX + ("mlp.rgb_layer.output_layer.bias" if arch == "mlp" else NGP_KEYS["head.bo"])].numel())


def load_render_state(sd, field, renderer, arch):
    """what a render needs: the field, the binary occupancy grid; returns the background colour (None: not a parameter)"""
    load_field_state_dict(field, arch, sd)
    renderer.binary.copy_(sd[OCC + "_binary"].reshape(-1).to(torch.uint8).to(renderer.binary.device))
    return torch.nn.functional.softplus(sd[BKGD_KEY].to(renderer.binary.device, torch.float32).reshape(-1)) if BKGD_KEY in sd else None


def load_train_state(sd, trainer, arch):
    """what training continues from: load_render_state() + the raw background, the grid's densities, the event parameters"""
    r = trainer.r
    if OCC + "_binary" not in sd or OCC + "occs" not in sd:
        raise KeyError(f"no occupancy grid ({OCC}occs / {OCC}_binary) in the checkpoint")
    load_render_state(sd, r.field, r, arch)
    if trainer.t.bkgd_is_param:
        trainer.small[: r.field.C] = sd[BKGD_KEY].to(r.occs.device, torch.float32).reshape(-1)
    r.occs.copy_(sd[OCC + "occs"].to(r.occs.device).reshape(-1))
    trainer.load_event_params(sd.get(CT_KEY), sd.get(TAU_KEY))
