"""Thin tensor-level wrappers over the C ABI: torch owns memory and streams, the HIP library does
the arithmetic.  Every function enqueues on ``torch.cuda.current_stream()`` and never syncs.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import GridDesc, SceneDesc, check

AABB, UN_BOUNDED_TANH, UN_BOUNDED_SPHERE = 0, 1, 2
FRAG_FLOATS_PER_BLOCK = 16 * 64          # hash features, fragment layout, per 32 samples
BASE_FLOATS_PER_BLOCK = 8 * 64           # saved base-MLP outputs, per 32 samples

_DT = {torch.float32: 4, torch.float64: 8, torch.int32: 4, torch.int64: 8, torch.uint8: 1, torch.bool: 1}


KNOBS = {"hgb_no_pairs": 0, "hgb_halve_regions": 1, "march_sequential": 2, "hg_variant": 3, "vfield_plain": 4, "hgb_subregion": 5}     # include/ren_amd.h REN_KNOB_*


class knob:
    """`with ops.knob("hgb_halve_regions", 1): ...` -- set a verification / tuning knob of the library for a block"""

    def __init__(self, name: str, value: int):
        self.k, self.v = KNOBS[name], int(value)

    def __enter__(self):
        lib = _lib.load()
        self.old = lib.ren_get_knob(self.k)
        check(lib.ren_set_knob(self.k, self.v), "ren_set_knob")

    def __exit__(self, *a):
        _lib.load().ren_set_knob(self.k, self.old)


# Activation alternatives of the YAML (robust_e_nerf/models/nerf.py:8-29) -> the `activations` argument of the ren_mlp_* /
# ren_vanilla_* entry points (include/ren_amd.h); every wrapper below takes it as `act` (0 = the shipped configs)
HIDDEN_ACTS = {"softplus": 0, "relu": 1}
DENSITY_ACTS = {"shifted_trunc_exp": 0, "softplus": 1, "shifted_softplus": 2}
RADIANCE_ACTS = {"softplus": 0, "sigmoid": 1}


def activation_code(base_hidden="softplus", density="shifted_trunc_exp", head_hidden="softplus", radiance="softplus") -> int:
    """0 = the shipped configs; unknown names raise NotImplementedError as the reference's table lookups would KeyError"""
    try:
        return (HIDDEN_ACTS[base_hidden] | DENSITY_ACTS[density] << 2 | HIDDEN_ACTS[head_hidden] << 4 |
                RADIANCE_ACTS[radiance] << 6)
    except KeyError as e:
        raise NotImplementedError(f"activation {e.args[0]!r} (models/nerf.py:17-29)") from e


def _ptr(t: Optional[torch.Tensor], dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("robust_e_nerf_amd kernels take device (ROCm) tensors; got a CPU tensor")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise ValueError(f"expected dtype {dtype}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


try:                                     # the raw handle of torch's current stream: two C calls instead of the ~8 us of Python that
    _raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice   # torch.cuda.current_stream() costs per launch
except AttributeError:                   # (a torch build without them)
    _raw_stream = None


def _stream():
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f(x):
    return ctypes.c_float(float(x))


NAN = float("nan")


# ------------------------------------------------------------------------------- descriptors
def make_grid_desc(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16,
                   per_level_scale=1.4472692012786865, otype="HashGrid") -> Tuple[GridDesc, int]:
    """tcnn grid level table (float32 arithmetic) -> (descriptor, number of float params).  otype (the YAML's
    pos_encoding.otype, configs/train/synthetic.yaml:63): HashGrid (level size capped at 2^log2_hashmap_size, spatial hash
    beyond), DenseGrid (no cap, never hashed), TiledGrid (capped at base_resolution^3, the dense index wraps)."""
    import numpy as np
    if otype not in ("HashGrid", "DenseGrid", "TiledGrid"):
        raise NotImplementedError(f"pos_encoding.otype={otype}")
    if n_features_per_level != 2:
        raise NotImplementedError("n_features_per_level must be 2")
    if n_levels > _lib.MAX_LEVELS:
        raise NotImplementedError("n_levels must be <= 16")
    g = GridDesc()
    g.n_levels = n_levels
    log2_pls = np.log2(np.float32(per_level_scale)).astype(np.float32)
    offset = 0
    for lvl in range(n_levels):
        scale = np.float32(np.exp2(np.float32(lvl) * log2_pls).astype(np.float32) * np.float32(base_resolution)
                           - np.float32(1.0))
        res = int(np.ceil(scale)) + 1
        dense = res ** 3
        size = (min(dense, 2 ** 31 - 1) + 7) // 8 * 8
        if otype == "HashGrid":
            size = min(size, 1 << log2_hashmap_size)
        elif otype == "TiledGrid":
            size = min(size, base_resolution ** 3)
        if offset + size >= 1 << 32:
            raise NotImplementedError("grid with more than 2^32 entries")
        g.scale[lvl] = float(scale)
        g.res[lvl] = res
        g.size[lvl] = size
        g.offset[lvl] = offset
        g.hashed[lvl] = 1 if (otype == "HashGrid" and dense > size) else 0
        offset += size
    return g, offset * 2


def make_scene_desc(aabb: Sequence[float], contraction_type: int) -> SceneDesc:
    s = SceneDesc()
    for k in range(6):
        s.aabb[k] = float(aabb[k])
    s.contraction_type = int(contraction_type)
    return s


def mlp_param_count(radiance_dim: int = 1) -> int:
    return 9360 + 65 * radiance_dim


MLP_SLICES = {  # name -> (offset, shape) for radiance_dim C (filled by mlp_slices)
}


def mlp_slices(C: int = 1):
    """Views of the concatenated MLP parameter block in torch nn.Linear layout."""
    return {
        "base.w0": (0, (64, 32)), "base.b0": (2048, (64,)), "base.wo": (2112, (16, 64)), "base.bo": (3136, (16,)),
        "head.w0": (3152, (64, 31)), "head.b0": (5136, (64,)), "head.w1": (5200, (64, 64)), "head.b1": (9296, (64,)),
        "head.wo": (9360, (C, 64)), "head.bo": (9360 + 64 * C, (C,)),
    }


# ---- torch.nn.utils.weight_norm over the Linear layers of an MLP (ngp.py:207-228, mlp.py:303-319) -------------------
def weight_norm_layers(layers):
    """layers: [(weight offset, rows, cols, first g index)] -> the host int32 table ren_weight_norm_* take."""
    import ctypes
    flat = [int(v) for layer in layers for v in layer]
    return (ctypes.c_int32 * len(flat))(*flat), len(layers)


def weight_norm_fwd(raw, g, table, eff):
    """eff = raw with W[r, :] = g[r] v[r, :] / ||v[r, :]|| in the listed layers"""
    import ctypes
    arr, n_layers = table
    check(_lib.load().ren_weight_norm_fwd(_ptr(raw), _ptr(g), ctypes.cast(arr, ctypes.c_void_p), n_layers, raw.numel(),
                                          _ptr(eff), _stream()), "ren_weight_norm_fwd")
    return eff


def weight_norm_bwd(raw, g, d_eff, table, d_raw, d_g, zero_d_eff: bool = False):
    """(d_raw, d_g) = gradient w.r.t. (v / biases / plain weights, g) from d_eff; zero_d_eff: clear d_eff afterwards"""
    import ctypes
    arr, n_layers = table
    check(_lib.load().ren_weight_norm_bwd(_ptr(raw), _ptr(g), _ptr(d_eff), ctypes.cast(arr, ctypes.c_void_p), n_layers,
                                          raw.numel(), _ptr(d_raw), _ptr(d_g), int(zero_d_eff), _stream()),
          "ren_weight_norm_bwd")


def n_blocks32(n: int) -> int:
    return (n + 31) // 32


# ------------------------------------------------------------------------------- pose / rays
def trajectory(ts: torch.Tensor, tab_ts, tab_pos, tab_quat):
    B = ts.shape[0]
    pos = torch.empty(B, 3, device=ts.device, dtype=torch.float32)
    rot = torch.empty(B, 3, 3, device=ts.device, dtype=torch.float32)
    if B == 0:                                           # empty tensors have no storage: their null pointers are no bad arguments
        return pos, rot
    check(_lib.load().ren_trajectory_fwd(_ptr(ts, torch.float64), B, _ptr(tab_ts, torch.int64),
                                         _ptr(tab_pos, torch.float32), _ptr(tab_quat, torch.float32),
                                         tab_ts.shape[0], _ptr(pos), _ptr(rot), _stream()), "ren_trajectory_fwd")
    return pos, rot


def raygen(Kinv, px, pos, rot):
    B = px.shape[0]
    o = torch.empty(B, 3, device=px.device, dtype=torch.float32)
    d = torch.empty(B, 3, device=px.device, dtype=torch.float32)
    if B == 0:
        return o, d
    check(_lib.load().ren_raygen_fwd(_ptr(Kinv, torch.float32), _ptr(px, torch.float32), _ptr(pos, torch.float32),
                                     _ptr(rot, torch.float32), B, _ptr(o), _ptr(d), _stream()), "ren_raygen_fwd")
    return o, d


def pose_rays(ts, px, Kinv, tab_ts, tab_pos, tab_quat):
    """trajectory() + raygen() in one launch; px (B, 2) is reused cyclically when ts has a multiple of B entries"""
    R = ts.shape[0]
    o = torch.empty(R, 3, device=ts.device, dtype=torch.float32)
    d = torch.empty(R, 3, device=ts.device, dtype=torch.float32)
    if R == 0:
        return o, d
    check(_lib.load().ren_pose_rays_fwd(_ptr(ts, torch.float64), R, _ptr(px, torch.float32), px.shape[0], _ptr(Kinv, torch.float32),
                                        _ptr(tab_ts, torch.int64), _ptr(tab_pos, torch.float32), _ptr(tab_quat, torch.float32),
                                        tab_ts.shape[0], _ptr(o), _ptr(d), _stream()), "ren_pose_rays_fwd")
    return o, d


# ------------------------------------------------------------------------------- sampling
def ray_aabb_intersect(o, d, aabb: Sequence[float], near: Optional[float] = None, far: Optional[float] = None):
    n = o.shape[0]
    tmin = torch.empty(n, device=o.device, dtype=torch.float32)
    tmax = torch.empty(n, device=o.device, dtype=torch.float32)
    ab = (ctypes.c_float * 6)(*[float(v) for v in aabb])
    check(_lib.load().ren_ray_aabb_intersect(_ptr(o, torch.float32), _ptr(d, torch.float32), n, ab,
                                             _f(NAN if near is None else near), _f(NAN if far is None else far),
                                             _ptr(tmin), _ptr(tmax), _stream()), "ren_ray_aabb_intersect")
    return tmin, tmax


def uniform(n: int, seed: int, offset: int = 0, device="cuda:0", out=None):
    """n iid U[0, 1) floats from the library's Philox stream (seed, offset): jitter without a torch RNG launch"""
    if out is None:
        out = torch.empty(n, device=device, dtype=torch.float32)
    check(_lib.load().ren_uniform(int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), n, _ptr(out), _stream()), "ren_uniform")
    return out


def exclusive_scan(counts: torch.Tensor):
    n = counts.shape[0]
    offsets = torch.empty(n, device=counts.device, dtype=torch.int64)
    total = torch.empty(1, device=counts.device, dtype=torch.int64)
    scratch = torch.empty(1024, device=counts.device, dtype=torch.int64) if n > 65536 else None
    check(_lib.load().ren_exclusive_scan(_ptr(counts, torch.int32), n, _ptr(offsets), _ptr(total), _ptr(scratch),
                                         _stream()), "ren_exclusive_scan")
    return offsets, total


MARCH_VERIFIED_DIV = 0x100          # include/ren_amd.h REN_MARCH_VERIFIED_DIV: OR into `mode` of ray_march_count / _write


def march_div_check(roi, device) -> bool:
    """True when the marcher's multiply-add division is bit-identical to the IEEE division for the extents of `roi` (every
    float numerator of 2^-100 < |a| < 2^100 tried on the device, ~20 ms): the caller may then pass mode | MARCH_VERIFIED_DIV"""
    ext = [float(roi[3 + k]) - float(roi[k]) for k in range(3)]
    if not all(2.0 ** -59 < e < 2.0 ** 59 for e in ext) or not all(2.0 ** -59 < abs(float(roi[k])) < 2.0 ** 59 for k in range(3)):
        return False                                  # (a box corner at 0: differences p - corner could leave the checked range)
    roi_c = (ctypes.c_float * 6)(*[float(v) for v in roi])
    out = torch.zeros(1, dtype=torch.int64, device=device)
    check(_lib.load().ren_march_div_check(roi_c, _ptr(out, torch.int64), _stream()), "ren_march_div_check")
    return int(out.item()) == 0


def ray_march_count(o, d, t_min, t_max, jitter, roi, res, binary, ct, step, cone, mode, n_uniform, cache=None):
    """cache: optional float32 (n_rays, cap, 2) interval cache filled here and consumed by ray_march_write"""
    n = o.shape[0]
    counts = torch.empty(n, device=o.device, dtype=torch.int32)
    roi_c = (ctypes.c_float * 6)(*[float(v) for v in roi])
    res_c = (ctypes.c_int32 * 3)(*[int(v) for v in res])
    check(_lib.load().ren_ray_march(_ptr(o), _ptr(d), _ptr(t_min), _ptr(t_max), _ptr(jitter), n, roi_c, res_c,
                                    _ptr(binary, (torch.uint8, torch.bool)), ct, _f(step), _f(cone), mode, n_uniform,
                                    None, _ptr(counts), None, None, None, _ptr(cache, torch.float32),
                                    0 if cache is None else cache.shape[1], _stream()), "ren_ray_march(count)")
    return counts


def ray_march_write(o, d, t_min, t_max, jitter, roi, res, binary, ct, step, cone, mode, n_uniform,
                    offsets, n_total: int, out=None, counts=None, cache=None, unit_scene: Optional[SceneDesc] = None):
    """unit_scene: the launch also stores the samples' unit-cube positions (ren_ray_march_unit) -> (ri, ts, te, x_unit)"""
    n = o.shape[0]
    if out is None:
        ri = torch.empty(n_total, device=o.device, dtype=torch.int32)
        ts = torch.empty(n_total, device=o.device, dtype=torch.float32)
        te = torch.empty(n_total, device=o.device, dtype=torch.float32)
    else:
        ri, ts, te = out
    xu = torch.empty(n_total, 3, device=o.device, dtype=torch.float32) if unit_scene is not None else None
    ret = (ri, ts, te) if xu is None else (ri, ts, te, xu)
    if n_total == 0:                                  # no ray meets an occupied cell: nothing to write
        return ret
    roi_c = (ctypes.c_float * 6)(*[float(v) for v in roi])
    res_c = (ctypes.c_int32 * 3)(*[int(v) for v in res])
    args = (_ptr(o), _ptr(d), _ptr(t_min), _ptr(t_max), _ptr(jitter), n, roi_c, res_c,
            _ptr(binary, (torch.uint8, torch.bool)), ct, _f(step), _f(cone), mode, n_uniform,
            _ptr(offsets, torch.int64), _ptr(counts, torch.int32), _ptr(ri), _ptr(ts), _ptr(te),
            _ptr(cache, torch.float32) if counts is not None else None,
            0 if (cache is None or counts is None) else cache.shape[1])
    if xu is None:
        check(_lib.load().ren_ray_march(*args, _stream()), "ren_ray_march(write)")
    else:
        check(_lib.load().ren_ray_march_unit(*args, ctypes.byref(unit_scene), _ptr(xu), _stream()), "ren_ray_march_unit")
    return ret


def unit_positions(scene: SceneDesc, rays, samples, n: int, n_dev=None, out=None):
    """(n, 3) unit-cube positions of a packed sample stream, as hashgrid_fwd forms them from the stream itself"""
    (o, d), (ri, ts, te) = rays, samples
    if out is None:
        out = torch.empty(n, 3, device=o.device, dtype=torch.float32)
    check(_lib.load().ren_unit_positions(ctypes.byref(scene), _ptr(o), _ptr(d), _ptr(ri, torch.int32), _ptr(ts), _ptr(te), n,
                                         _ptr(out, torch.float32), _ptr(n_dev, torch.int64), _stream()), "ren_unit_positions")
    return out


def count_guard(counts, total, capacity: int, n_out, stats=None, counts_also=None):
    """device-side sample count: n_out[0] = total if it fits `capacity`, else 0 with every ray's count (and counts_also's)
    cleared; stats = (total as found, 1 if it did not fit else 0); see include/ren_amd.h ("device-side sample counts")"""
    check(_lib.load().ren_count_guard(_ptr(counts, torch.int32), _ptr(counts_also, torch.int32), counts.shape[0],
                                      _ptr(total, torch.int64), int(capacity), _ptr(n_out, torch.int64), _ptr(stats, torch.int64),
                                      _stream()), "ren_count_guard")


def scan_guard(counts, capacity: int, n_out, stats=None, counts_also=None):
    """exclusive_scan + count_guard (one launch for up to 65 536 rays) -> offsets, total"""
    n = counts.shape[0]
    offsets = torch.empty(n, device=counts.device, dtype=torch.int64)
    total = torch.empty(1, device=counts.device, dtype=torch.int64)
    scratch = torch.empty(1024, device=counts.device, dtype=torch.int64) if n > 65536 else None
    check(_lib.load().ren_scan_guard(_ptr(counts, torch.int32), _ptr(counts_also, torch.int32), n, _ptr(offsets), _ptr(total),
                                     int(capacity), _ptr(n_out, torch.int64), _ptr(stats, torch.int64), _ptr(scratch), _stream()),
          "ren_scan_guard")
    return offsets, total


def frag_zero_tail(feat, capacity: int, n_dev):
    check(_lib.load().ren_frag_zero_tail(_ptr(feat, torch.float32), int(capacity), _ptr(n_dev, torch.int64), _stream()),
          "ren_frag_zero_tail")


def visibility(offsets, counts, sigmas, ts, te, eps: float, alpha_thre: float):
    n_rays = counts.shape[0]
    keep = torch.empty(ts.shape[0], device=ts.device, dtype=torch.uint8)
    kept = torch.empty(n_rays, device=ts.device, dtype=torch.int32)
    check(_lib.load().ren_visibility(_ptr(offsets, torch.int64), _ptr(counts, torch.int32), n_rays,
                                     _ptr(sigmas, torch.float32), _ptr(ts), _ptr(te), _f(eps), _f(alpha_thre),
                                     _ptr(keep), _ptr(kept), _stream()), "ren_visibility")
    return keep, kept


def compact_samples(offsets, counts, new_offsets, keep, ts, te, n_new: int, x_unit=None):
    """x_unit: the samples' unit positions (ray_march_write(unit_scene=...)) are compacted with them -> (ri, ts, te, x_unit)"""
    n_rays = counts.shape[0]
    ri2 = torch.empty(n_new, device=ts.device, dtype=torch.int32)
    ts2 = torch.empty(n_new, device=ts.device, dtype=torch.float32)
    te2 = torch.empty(n_new, device=ts.device, dtype=torch.float32)
    if x_unit is not None:
        xu2 = torch.empty(n_new, 3, device=ts.device, dtype=torch.float32)
        if n_new > 0:
            check(_lib.load().ren_compact_samples_unit(_ptr(offsets), _ptr(counts), _ptr(new_offsets), n_rays, _ptr(keep),
                                                       _ptr(ts), _ptr(te), _ptr(x_unit, torch.float32), _ptr(ri2), _ptr(ts2),
                                                       _ptr(te2), _ptr(xu2), _stream()), "ren_compact_samples_unit")
        return ri2, ts2, te2, xu2
    if n_new == 0:                                    # everything culled by the visibility test
        return ri2, ts2, te2
    check(_lib.load().ren_compact_samples(_ptr(offsets), _ptr(counts), _ptr(new_offsets), n_rays, _ptr(keep),
                                          _ptr(ts), _ptr(te), _ptr(ri2), _ptr(ts2), _ptr(te2), _stream()),
          "ren_compact_samples")
    return ri2, ts2, te2


def compact_features(offsets, counts, new_offsets, keep, feat, n_new: int, n_dev=None):
    """fragment-layout features of the kept samples at their compacted positions (padding lanes zero).
    n_dev: n_new is the capacity, the number of kept samples is on the device"""
    out = torch.empty(n_blocks32(n_new) * FRAG_FLOATS_PER_BLOCK, device=feat.device, dtype=torch.float32)
    if n_new == 0:
        return out
    if n_dev is None:
        out[-FRAG_FLOATS_PER_BLOCK:].zero_()
    check(_lib.load().ren_compact_features(_ptr(offsets, torch.int64), _ptr(counts, torch.int32), _ptr(new_offsets, torch.int64),
                                           counts.shape[0], _ptr(keep), _ptr(feat, torch.float32), _ptr(out), _stream()),
          "ren_compact_features")
    if n_dev is not None:
        frag_zero_tail(out, n_new, n_dev)            # lanes beyond the count in its last 32-sample block
    return out


def pack_info(ray_indices: torch.Tensor, n_rays: int):
    n = ray_indices.shape[0]
    offsets = torch.empty(n_rays, device=ray_indices.device, dtype=torch.int64)
    counts = torch.empty(n_rays, device=ray_indices.device, dtype=torch.int32)
    check(_lib.load().ren_pack_info(_ptr(ray_indices, torch.int32), n, n_rays, _ptr(offsets), _ptr(counts),
                                    _stream()), "ren_pack_info")
    return offsets, counts


# ------------------------------------------------------------------------------- hash grid
def hashgrid_fwd(grid: GridDesc, table, *, x_unit=None, scene: Optional[SceneDesc] = None, rays=None,
                 samples=None, n: int, layout: int, out=None, n_dev=None):
    L = grid.n_levels
    dev = table.device
    if out is None:
        out = (torch.empty(n, 2 * L, device=dev, dtype=torch.float32) if layout == 0
               else torch.empty(n_blocks32(n) * FRAG_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32))
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    check(_lib.load().ren_hashgrid_fwd(ctypes.byref(grid), _ptr(table, torch.float32), _ptr(x_unit),
                                       ctypes.byref(scene) if scene is not None else None,
                                       _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout, _ptr(out), _ptr(n_dev, torch.int64),
                                       _stream()), "ren_hashgrid_fwd")
    return out


def hashgrid_bwd(grid: GridDesc, grad_table, dfeat, *, x_unit=None, scene=None, rays=None, samples=None,
                 n: int, layout: int):
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    check(_lib.load().ren_hashgrid_bwd(ctypes.byref(grid), _ptr(grad_table, torch.float32), _ptr(x_unit),
                                       ctypes.byref(scene) if scene is not None else None,
                                       _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout,
                                       _ptr(dfeat, torch.float32), _stream()), "ren_hashgrid_bwd")


def hashgrid_bwd_input(grid: GridDesc, table, dfeat, *, x_unit=None, scene=None, rays=None, samples=None,
                       n: int, layout: int, out=None):
    """dx (n, 3) = J_x^T dfeat of the encoding, one launch (csrc/ren_normals.hip).  x_unit: gradient w.r.t. the unit-cube
    position; scene + rays + samples: world-space gradient at the sample midpoints (through the contraction)."""
    if out is None:
        out = torch.empty(n, 3, device=table.device, dtype=torch.float32)
    if n == 0:                                           # empty tensors have no storage: their null pointers are no bad arguments
        return out
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    check(_lib.load().ren_hashgrid_bwd_input(ctypes.byref(grid), _ptr(table, torch.float32), _ptr(x_unit),
                                             ctypes.byref(scene) if scene is not None else None,
                                             _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout,
                                             _ptr(dfeat, torch.float32), _ptr(out, torch.float32), _stream()),
          "ren_hashgrid_bwd_input")
    return out


def hashgrid_bwd_binned_workspace_bytes(n: int) -> int:
    return int(_lib.load().ren_hashgrid_bwd_binned_workspace_bytes(n))


def hashgrid_bwd_binned(grid: GridDesc, grad_table, dfeat, workspace, *, x_unit=None, scene=None, rays=None,
                        samples=None, n: int, layout: int, level_mask: Optional[int] = None, tangent=None, n_dev=None):
    """LDS-binned (atomic-free) variant of hashgrid_bwd; workspace: uint8 tensor of
    hashgrid_bwd_binned_workspace_bytes(n) bytes.  level_mask: only the levels whose bit is set; tangent: (rays_do,
    rays_dd, dfeatd) of the log-intensity-gradient render."""
    if workspace.numel() * workspace.element_size() < hashgrid_bwd_binned_workspace_bytes(n):
        raise ValueError("hashgrid_bwd_binned: workspace too small")
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    if level_mask is not None or tangent is not None:
        do, dd, dfd = tangent if tangent is not None else (None, None, None)
        check(_lib.load().ren_hashgrid_bwd_binned_levels(
            ctypes.byref(grid), _ptr(grad_table, torch.float32), _ptr(x_unit), ctypes.byref(scene) if scene is not None else None,
            _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout, _ptr(dfeat, torch.float32), _ptr(do), _ptr(dd), _ptr(dfd),
            0xFFFFFFFF if level_mask is None else int(level_mask), _ptr(workspace), _ptr(n_dev, torch.int64), _stream()),
              "ren_hashgrid_bwd_binned_levels")
        return
    check(_lib.load().ren_hashgrid_bwd_binned(ctypes.byref(grid), _ptr(grad_table, torch.float32), _ptr(x_unit),
                                              ctypes.byref(scene) if scene is not None else None,
                                              _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout,
                                              _ptr(dfeat, torch.float32), _ptr(workspace), _ptr(n_dev, torch.int64), _stream()),
          "ren_hashgrid_bwd_binned")


BINNED_MAX_LEVEL_ENTRIES = 1 << 19          # 64 bins of 8 192 entries: what ren_hashgrid_bwd_binned takes per level


def binned_supported(grid: GridDesc) -> bool:
    """False for a DenseGrid with a level above 2^19 entries: such a grid takes the per-update atomic scatter"""
    return max(int(grid.size[l]) for l in range(grid.n_levels)) <= BINNED_MAX_LEVEL_ENTRIES


def hashgrid_bwd_auto(grid: GridDesc, grad_table, dfeat, *, x_unit=None, scene=None, rays=None, samples=None, n: int,
                      layout: int):
    """parameter gradient of the module seams (field.NGPradianceField, tcnn_api.Encoding): the binned scatter with a
    workspace of its own, or the atomic scatter for grids the binned one refuses (as engine.Renderer chooses)"""
    if binned_supported(grid):
        ws = torch.empty(hashgrid_bwd_binned_workspace_bytes(n), device=dfeat.device, dtype=torch.uint8)
        hashgrid_bwd_binned(grid, grad_table, dfeat, ws, x_unit=x_unit, scene=scene, rays=rays, samples=samples, n=n,
                            layout=layout)
    else:
        hashgrid_bwd(grid, grad_table, dfeat, x_unit=x_unit, scene=scene, rays=rays, samples=samples, n=n, layout=layout)


def hashgrid_bwd_binned_begin(grid: GridDesc, workspace, *, scene, rays, samples, n: int, layout: int = 1):
    """phase 1 of hashgrid_bwd_binned: clear + count + offsets (sample stream only)"""
    if workspace.numel() * workspace.element_size() < hashgrid_bwd_binned_workspace_bytes(n):
        raise ValueError("hashgrid_bwd_binned: workspace too small")
    (o, d), (ri, ts, te) = rays, samples
    check(_lib.load().ren_hashgrid_bwd_binned_begin(ctypes.byref(grid), None, ctypes.byref(scene), _ptr(o), _ptr(d), _ptr(ri),
                                                    _ptr(ts), _ptr(te), n, layout, _ptr(workspace), _stream()),
          "ren_hashgrid_bwd_binned_begin")


def hashgrid_bwd_binned_scatter(grid: GridDesc, grad_table, dfeat, workspace, *, scene, rays, samples, n: int, first: int,
                                m: int, layout: int = 1):
    """phase 2: scatter samples [first, first + m) of the stream (dfeat, samples: the WHOLE stream's tensors)"""
    (o, d), (ri, ts, te) = rays, samples
    check(_lib.load().ren_hashgrid_bwd_binned_scatter(ctypes.byref(grid), _ptr(grad_table, torch.float32), None, ctypes.byref(scene),
                                                      _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n, layout,
                                                      _ptr(dfeat, torch.float32), first, m, _ptr(workspace), _stream()),
          "ren_hashgrid_bwd_binned_scatter")


def hashgrid_bwd_binned_finish(grid: GridDesc, grad_table, workspace, *, n: int, layout: int = 1):
    """phase 3: partition + accumulate + flush"""
    check(_lib.load().ren_hashgrid_bwd_binned_finish(ctypes.byref(grid), _ptr(grad_table, torch.float32), n, layout,
                                                     _ptr(workspace), _stream()), "ren_hashgrid_bwd_binned_finish")


# ------------------------------------------------------------------------------- fused MLPs
def mlp_fwd(mlp_params, C: int, feat, scene: SceneDesc, *, x_world=None, dirs=None, rays=None, samples=None,
            n: int, density_only: bool = False, save_base: bool = False, out=None, bf16: bool = False, act: int = 0):
    """bf16=True: `mlp_params` must be the bf16-rounded copy of the block (see ren_mlp_fwd_bf16)."""
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    if out is None:
        sigma = torch.empty(n, device=dev, dtype=torch.float32)
        rgb = None if density_only else torch.empty(n, C, device=dev, dtype=torch.float32)
        base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32) if save_base else None
    else:
        rgb, sigma, base = out
    fn = _lib.load().ren_mlp_fwd_bf16 if bf16 else _lib.load().ren_mlp_fwd
    check(fn(_ptr(mlp_params, torch.float32), C, int(act), _ptr(feat, torch.float32), ctypes.byref(scene),
             _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n,
             1 if density_only else 0, _ptr(rgb), _ptr(sigma), _ptr(base), _stream()),
          "ren_mlp_fwd")
    return rgb, sigma, base


def mlp_fwd_save(mlp_params, C: int, feat, scene: SceneDesc, *, rays=None, samples=None, x_world=None, dirs=None,
                 n: int, bf16: bool = False, act: int = 0):
    """Training forward: also saves base outputs and the hidden activations (768 B/sample) for mlp_bwd_saved.
    -> rgb, sigma, base, acts"""
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    sigma = torch.empty(n, device=dev, dtype=torch.float32)
    rgb = torch.empty(n, C, device=dev, dtype=torch.float32)
    base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    lib = _lib.load()
    acts = torch.empty(int(lib.ren_mlp_act_save_floats(n)), device=dev, dtype=torch.float32)
    check(lib.ren_mlp_fwd_save(_ptr(mlp_params, torch.float32), C, int(act), 1 if bf16 else 0, _ptr(feat, torch.float32),
                               ctypes.byref(scene), _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d), _ptr(ri), _ptr(ts),
                               _ptr(te), n, _ptr(rgb), _ptr(sigma), _ptr(base), _ptr(acts), _stream()), "ren_mlp_fwd_save")
    return rgb, sigma, base, acts


def mlp_bwd_saved(mlp_params, C: int, feat, base_out, acts, scene: SceneDesc, *, rays=None, samples=None, x_world=None,
                  dirs=None, n: int, rgb, d_rgb, d_sigma, grad_mlp_params, workspace, bf16: bool = False, act: int = 0):
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    d_base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    dfeat = torch.empty(n_blocks32(n) * FRAG_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    check(_lib.load().ren_mlp_bwd_saved(_ptr(mlp_params, torch.float32), C, int(act), 1 if bf16 else 0, _ptr(feat), _ptr(base_out),
                                        _ptr(acts), ctypes.byref(scene), _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d),
                                        _ptr(ri), _ptr(ts), _ptr(te), n, _ptr(rgb), _ptr(d_rgb), _ptr(d_sigma),
                                        _ptr(d_base), _ptr(dfeat), _ptr(grad_mlp_params, torch.float32), _ptr(workspace),
                                        _stream()), "ren_mlp_bwd_saved")
    return dfeat


def mlp_fwd_x(mlp_params, C: int, mode: int, feat, scene: SceneDesc, *, rays=None, samples=None, x_world=None, dirs=None,
              n: int, density_only: bool = False, save: bool = False, out=None, share_cu: bool = False, save_acts: bool = True,
              act: int = 0, n_dev=None):
    """Split-bf16 matrix-core kernels (csrc/ren_mlp_x.hip).  mode 6: fp32 accuracy; mode 3: two bf16 pieces / three products
    (float32_matmul_precision "high"); mode 1: plain bf16 operands.
    -> rgb, sigma, base, acts (base/acts None unless save; acts None with save_acts=False: mlp_bwd_x then recomputes
    the hidden activations); out: preallocated (rgb, sigma, base, acts) views"""
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    lib = _lib.load()
    if out is not None:
        rgb, sigma, base, acts = out
    else:
        sigma = torch.empty(n, device=dev, dtype=torch.float32)
        rgb = None if density_only else torch.empty(n, C, device=dev, dtype=torch.float32)
        base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32) if save else None
        acts = torch.empty(int(lib.ren_mlp_act_save_floats(n)), device=dev, dtype=torch.float32) if (save and save_acts) else None
    check(lib.ren_mlp_fwd_x(_ptr(mlp_params, torch.float32), C, int(act), mode, _ptr(feat, torch.float32), ctypes.byref(scene),
                            _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d), _ptr(ri), _ptr(ts), _ptr(te), n,
                            (1 if density_only else 0) | (2 if share_cu else 0), _ptr(rgb), _ptr(sigma), _ptr(base),
                            _ptr(acts), _ptr(n_dev, torch.int64), _stream()), "ren_mlp_fwd_x")
    return rgb, sigma, base, acts


def mlp_act_save_floats(n: int) -> int:
    return int(_lib.load().ren_mlp_act_save_floats(n))


def mlp_bwd_x_workspace_floats(C: int) -> int:
    return int(_lib.load().ren_mlp_bwd_x_workspace_floats(C))


def mlp_bwd_x(mlp_params, C: int, mode: int, feat, base_out, acts, scene: SceneDesc, *, rays=None, samples=None,
              x_world=None, dirs=None, n: int, rgb, d_rgb, d_sigma, grad_mlp_params, workspace, dfeat=None, d_base=None,
              act: int = 0, grid_cus: int = 0, n_dev=None):
    """grid_cus: CUs the two persistent kernels occupy (0 = all; the chunked backward leaves some to the scatter)"""
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    if d_base is None:
        d_base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    if dfeat is None:
        dfeat = torch.empty(n_blocks32(n) * FRAG_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    check(_lib.load().ren_mlp_bwd_x(_ptr(mlp_params, torch.float32), C, int(act), mode, _ptr(feat), _ptr(base_out), _ptr(acts),
                                    ctypes.byref(scene), _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d), _ptr(ri), _ptr(ts),
                                    _ptr(te), n, _ptr(rgb), _ptr(d_rgb), _ptr(d_sigma), _ptr(d_base), _ptr(dfeat),
                                    _ptr(grad_mlp_params, torch.float32), _ptr(workspace), int(grid_cus), _ptr(n_dev, torch.int64), _stream()),
          "ren_mlp_bwd_x")
    return dfeat


def mlp_bwd_workspace_floats(C: int) -> int:
    return int(_lib.load().ren_mlp_bwd_workspace_floats(C))


def mlp_bwd(mlp_params, C: int, feat, base_out, scene: SceneDesc, *, x_world=None, dirs=None, rays=None,
            samples=None, n: int, rgb, d_rgb, d_sigma, grad_mlp_params, workspace, d_base=None, dfeat=None,
            bf16: bool = False, act: int = 0):
    dev = feat.device
    o, d = rays if rays is not None else (None, None)
    ri, ts, te = samples if samples is not None else (None, None, None)
    if d_base is None:
        d_base = torch.empty(n_blocks32(n) * BASE_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    if dfeat is None:
        dfeat = torch.empty(n_blocks32(n) * FRAG_FLOATS_PER_BLOCK, device=dev, dtype=torch.float32)
    fn = _lib.load().ren_mlp_bwd_bf16 if bf16 else _lib.load().ren_mlp_bwd
    check(fn(_ptr(mlp_params, torch.float32), C, int(act), _ptr(feat), _ptr(base_out),
                                  ctypes.byref(scene), _ptr(x_world), _ptr(dirs), _ptr(o), _ptr(d), _ptr(ri),
                                  _ptr(ts), _ptr(te), n, _ptr(rgb), _ptr(d_rgb), _ptr(d_sigma), _ptr(d_base),
                                  _ptr(dfeat), _ptr(grad_mlp_params, torch.float32), _ptr(workspace), _stream()),
          "ren_mlp_bwd")
    return dfeat


# ------------------------------------------------------------------------------- compositing
def composite_fwd(offsets, counts, ts, te, sigmas, rgbs, C: int, bkgd, save: bool = True):
    n_rays = counts.shape[0]
    dev = ts.device
    colors = torch.empty(n_rays, C, device=dev, dtype=torch.float32) if rgbs is not None else None
    opac = torch.empty(n_rays, device=dev, dtype=torch.float32)
    depth = torch.empty(n_rays, device=dev, dtype=torch.float32)
    w = torch.empty(ts.shape[0], device=dev, dtype=torch.float32) if save else None
    T = torch.empty(ts.shape[0], device=dev, dtype=torch.float32) if save else None
    check(_lib.load().ren_composite_fwd(_ptr(offsets, torch.int64), _ptr(counts, torch.int32), n_rays, _ptr(ts),
                                        _ptr(te), _ptr(sigmas), _ptr(rgbs), C, _ptr(bkgd), _ptr(colors), _ptr(opac),
                                        _ptr(depth), _ptr(w), _ptr(T), _stream()), "ren_composite_fwd")
    return colors, opac, depth, w, T


def composite_bwd(offsets, counts, ts, te, sigmas, rgbs, C: int, bkgd, w, T, opac, g_colors, g_opac=None,
                  g_depth=None, want_bkgd: bool = False, g_weights=None):
    n_rays = counts.shape[0]
    dev = ts.device
    d_sig = torch.empty(ts.shape[0], device=dev, dtype=torch.float32)
    d_rgb = torch.empty(ts.shape[0], C, device=dev, dtype=torch.float32) if rgbs is not None else None
    d_bk = torch.empty(n_rays, C, device=dev, dtype=torch.float32) if want_bkgd else None
    check(_lib.load().ren_composite_bwd(_ptr(offsets), _ptr(counts), n_rays, _ptr(ts), _ptr(te), _ptr(sigmas),
                                        _ptr(rgbs), C, _ptr(bkgd), _ptr(w), _ptr(T), _ptr(opac),
                                        _ptr(g_colors, torch.float32), _ptr(g_opac), _ptr(g_depth), _ptr(g_weights),
                                        _ptr(d_sig), _ptr(d_rgb), _ptr(d_bk), _stream()), "ren_composite_bwd")
    return d_sig, d_rgb, d_bk


def column_sum(x: torch.Tensor):
    rows, C = x.shape
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    scratch = torch.empty(512, device=x.device, dtype=torch.float32)
    check(_lib.load().ren_column_sum(_ptr(x, torch.float32), rows, C, _ptr(out), _ptr(scratch), _stream()),
          "ren_column_sum")
    return out


# ------------------------------------------------------------------------------- evaluation metrics
def ssim_scratch_doubles(P: int, H: int, W: int) -> int:
    return int(_lib.load().ren_ssim_scratch_doubles(P, H, W))


def ssim_planes(pred: torch.Tensor, target: torch.Tensor, data_range: float) -> torch.Tensor:
    """(P, H, W) float32 device tensors -> (P,) float64: the mean SSIM of every plane over its (H - 10) x (W - 10) valid
    windows (torchmetrics ssim with the reference's arguments, loss_metric/metric.py:74-81), one launch for all planes"""
    if pred.dim() != 3 or pred.shape != target.shape:
        raise ValueError(f"ssim_planes takes two (P, H, W) tensors of one shape; got {tuple(pred.shape)}, {tuple(target.shape)}")
    pred, target = pred.contiguous(), target.contiguous()
    P, H, W = pred.shape
    out = torch.empty(P, device=pred.device, dtype=torch.float64)
    scratch = torch.empty(max(1, ssim_scratch_doubles(P, H, W)), device=pred.device, dtype=torch.float64)
    check(_lib.load().ren_ssim_planes(_ptr(pred, torch.float32), _ptr(target, torch.float32), P, H, W, float(data_range),
                                      _ptr(out), _ptr(scratch), _stream()), "ren_ssim_planes")
    return out


# ------------------------------------------------------------------------------- event frames
EVENT_FRAMES_LDS_EDGES = 4096        # REN_EVENT_FRAMES_LDS_EDGES: the edges are searched in LDS while V + 1 <= this
EVENT_FRAMES_MERGE = 1               # REN_EVENT_FRAMES_MERGE


def event_frames(position: torch.Tensor, timestamp: torch.Tensor, polarity: torch.Tensor, edges: torch.Tensor, height: int,
                 width: int, merge: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the raw stream of raw_events.npz on the device -- position (N, 2) uint16 (x, y) [or (N,) int32 words x | y << 16],
    timestamp (N,) int64 in time order, polarity (N,) bool / uint8 -- binned into the windows [edges[v], edges[v + 1]) of
    `edges` (V + 1,) int64: -> counts (V, 2, H, W) int32, plane 0 the positive and plane 1 the negative events.  Events
    outside every window or outside the image are dropped.  Integer atomics: exact, bitwise repeatable.  `merge`: one atomic
    per distinct counter of a wave (same result).  `out`: add to these counts instead of to zeros."""
    n = timestamp.shape[0]
    if position.dtype == torch.uint16 and position.dim() == 2 and position.shape == (n, 2):
        words = position.contiguous().view(torch.int32).view(-1) if n else torch.empty(0, device=position.device, dtype=torch.int32)
    elif position.dtype == torch.int32 and position.shape == (n,):
        words = position.contiguous()
    else:
        raise ValueError(f"event_frames: position must be (N, 2) uint16 or (N,) int32 words; got {position.dtype} "
                         f"{tuple(position.shape)} for {n} timestamps")
    if polarity.shape != (n,) or polarity.dtype not in (torch.bool, torch.uint8, torch.int8):
        raise ValueError(f"event_frames: polarity must be (N,) bool / uint8; got {polarity.dtype} {tuple(polarity.shape)}")
    if edges.dim() != 1 or edges.shape[0] < 2:
        raise ValueError("event_frames: edges must hold at least two times")
    V = edges.shape[0] - 1
    if out is None:
        out = torch.zeros(V, 2, height, width, device=edges.device, dtype=torch.int32)
    elif out.shape != (V, 2, height, width):
        raise ValueError(f"event_frames: out must be ({V}, 2, {height}, {width}); got {tuple(out.shape)}")
    check(_lib.load().ren_event_frames(_ptr(words), _ptr(timestamp.contiguous(), torch.int64), _ptr(polarity.contiguous()), n,
                                       _ptr(edges.contiguous(), torch.int64), V, height, width,
                                       EVENT_FRAMES_MERGE if merge else 0, _ptr(out, torch.int32), _stream()), "ren_event_frames")
    return out


def event_frame_compare_scratch_doubles(V: int, H: int, W: int) -> int:
    return int(_lib.load().ren_event_frame_compare_scratch_doubles(V, H, W))


def event_frame_compare(counts: torch.Tensor, pred: torch.Tensor, valid: torch.Tensor, c_p: float, c_n: float) -> torch.Tensor:
    """counts (V, 2, H, W) int32, pred (V, H, W) float32, valid (V, H, W) bool / uint8 -> (V, 9) float64 per window, over
    the pixels with valid != 0 and with m = c_p n+ - c_n n- in float64:
    [count, sum m, sum p, sum m^2, sum p^2, sum m p, sum (p - m)^2, #{|p - m| <= max(c_p, c_n)}, #{n+ + n- > 0}].
    Two launches, fixed-order sums, no float atomics: bitwise repeatable."""
    if counts.dim() != 4 or counts.shape[1] != 2:
        raise ValueError(f"event_frame_compare: counts must be (V, 2, H, W); got {tuple(counts.shape)}")
    V, _, H, W = counts.shape
    if pred.shape != (V, H, W) or valid.shape != (V, H, W):
        raise ValueError(f"event_frame_compare: pred / valid must be ({V}, {H}, {W}); got {tuple(pred.shape)}, {tuple(valid.shape)}")
    if valid.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"event_frame_compare: valid must be bool / uint8; got {valid.dtype}")
    out = torch.empty(V, 9, device=counts.device, dtype=torch.float64)
    scratch = torch.empty(max(1, event_frame_compare_scratch_doubles(V, H, W)), device=counts.device, dtype=torch.float64)
    check(_lib.load().ren_event_frame_compare(_ptr(counts.contiguous(), torch.int32), _ptr(pred.contiguous(), torch.float32),
                                              _ptr(valid.contiguous()), V, H, W, float(c_p), float(c_n), _ptr(out),
                                              _ptr(scratch), _stream()), "ren_event_frame_compare")
    return out


# ------------------------------------------------------------------------------- event table
EVENT_TABLE_THREADS = 256            # REN_EVENT_TABLE_THREADS: workgroup size of both kernels
EVENT_TABLE_MAX_N = 2 ** 31 - 1      # N and H * W stay below 2^31
INT64_MAX = 2 ** 63 - 1
_POSITION_BYTES = {torch.uint16: 2, torch.int32: 4, torch.int64: 8}


def event_intervals(pix_sorted: torch.Tensor, order: torch.Tensor, timestamp: torch.Tensor):
    """pix_sorted (N,) int32 pixel keys in stable by-pixel order, order (N,) int64 as `torch.sort(stable=True)` returns it,
    timestamp (N,) int64 in stream order -> valid (N,) uint8 and start_ts (N,) int64 in stream order (start_ts is written
    where valid only) and min_diff (1,) int64: the smallest kept interval, INT64_MAX when none is kept.  An event is kept when
    the slot before it in the by-pixel order holds the same pixel at a different time (data.queue_raw_events)."""
    n = timestamp.shape[0]
    if pix_sorted.shape != (n,) or order.shape != (n,):
        raise ValueError(f"event_intervals: pix_sorted / order must be ({n},); got {tuple(pix_sorted.shape)}, {tuple(order.shape)}")
    dev = timestamp.device
    valid = torch.empty(n, device=dev, dtype=torch.uint8)
    start_ts = torch.empty(n, device=dev, dtype=torch.int64)
    min_diff = torch.full((1,), INT64_MAX, device=dev, dtype=torch.int64)
    if n == 0:
        return valid, start_ts, min_diff
    check(_lib.load().ren_event_intervals(_ptr(pix_sorted, torch.int32), _ptr(order, torch.int64), _ptr(timestamp, torch.int64), n,
                                          _ptr(valid), _ptr(start_ts), _ptr(min_diff), _stream()), "ren_event_intervals")
    return valid, start_ts, min_diff


def event_table_write(valid: torch.Tensor, offsets: torch.Tensor, position: torch.Tensor, timestamp: torch.Tensor,
                      start_ts: torch.Tensor, polarity: torch.Tensor, m: int, height: int, width: int,
                      lut: Optional[torch.Tensor] = None, bayer_channels: Optional[Sequence[int]] = None):
    """the kept events (valid (N,) uint8, offsets (N,) int32 = its exclusive prefix sum, m = its sum) compacted in stream
    order into the training table: position (m, 2) float32 -- `lut` (H * W, 2) float32 gathered at the event's pixel, or the
    stored coordinates cast -- start_ts / end_ts / num_pos / num_neg (m,) int64 and, with `bayer_channels` (the channel of the
    tile positions TL, TR, BL, BR), channel_idx (m,) uint8.  position: (N, 2) uint16 / int32 / int64 as stored, polarity: (N,)
    bool / uint8.  The CALLER has checked 0 <= x < width and 0 <= y < height (data.build_event_table)."""
    n = timestamp.shape[0]
    m = int(m)
    if position.shape != (n, 2) or position.dtype not in _POSITION_BYTES:
        raise ValueError(f"event_table_write: position must be ({n}, 2) uint16 / int32 / int64; got {position.dtype} {tuple(position.shape)}")
    if polarity.shape != (n,) or polarity.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"event_table_write: polarity must be ({n},) bool / uint8; got {polarity.dtype} {tuple(polarity.shape)}")
    if valid.shape != (n,) or offsets.shape != (n,) or start_ts.shape != (n,) or not 0 <= m <= n:
        raise ValueError(f"event_table_write: valid / offsets / start_ts must be ({n},) and 0 <= m <= {n}")
    if lut is not None and lut.shape != (height * width, 2):
        raise ValueError(f"event_table_write: lut must be ({height * width}, 2); got {tuple(lut.shape)}")
    if bayer_channels is not None and len(bayer_channels) != 4:
        raise ValueError("event_table_write: bayer_channels holds the channel of the four tile positions")
    dev = timestamp.device
    out = {"position": torch.empty(m, 2, device=dev, dtype=torch.float32)}
    for k in ("start_ts", "end_ts", "num_pos", "num_neg"):
        out[k] = torch.empty(m, device=dev, dtype=torch.int64)
    code = None
    if bayer_channels is not None:
        out["channel_idx"] = torch.empty(m, device=dev, dtype=torch.uint8)
        code = (ctypes.c_uint8 * 4)(*(int(c) for c in bayer_channels))
    if n == 0 or m == 0:
        return out
    check(_lib.load().ren_event_table_write(
        _ptr(valid, torch.uint8), _ptr(offsets, torch.int32), _ptr(position), _POSITION_BYTES[position.dtype],
        _ptr(timestamp, torch.int64), _ptr(start_ts, torch.int64), _ptr(polarity), n, m, _ptr(lut, torch.float32), height, width,
        None if code is None else ctypes.cast(code, ctypes.c_void_p), _ptr(out["position"]), _ptr(out["start_ts"]),
        _ptr(out["end_ts"]), _ptr(out["num_pos"]), _ptr(out["num_neg"]), _ptr(out.get("channel_idx")), _stream()),
        "ren_event_table_write")
    return out


# ------------------------------------------------------------------------------- event filter
EVENT_FILTER_THREADS = 256           # REN_EVENT_FILTER_THREADS: workgroup size
EVENT_FILTER_MAX_BLOCKS = 2048       # REN_EVENT_FILTER_MAX_BLOCKS: more slots than their product take a second trip of the loop


def event_support(pix_sorted: torch.Tensor, order: torch.Tensor, ts_sorted: torch.Tensor, seg: torch.Tensor,
                  hot: Optional[torch.Tensor], height: int, width: int, dt: Optional[int], include_self: bool = False):
    """keep (N,) uint8 in STREAM order: 1 where the event's pixel is not hot and another event at one of its eight in-sensor,
    non-hot neighbour pixels (its own pixel too with `include_self`) lies 0 .. dt before it (include/ren_amd.h "event filter").
    pix_sorted (N,) int32 keys y * width + x and order (N,) int64 as `torch.sort(stable=True)` returns them, ts_sorted (N,) int64
    = timestamp[order] of a time-ordered stream, seg (height * width + 1,) int32 segment starts of the pixels in the sorted
    stream, hot (height * width,) uint8 or None (no pixel is hot), dt >= 0 or None (every event is supported)."""
    n = ts_sorted.shape[0]
    height, width = int(height), int(width)
    if pix_sorted.shape != (n,) or order.shape != (n,) or ts_sorted.dim() != 1:
        raise ValueError(f"event_support: pix_sorted / order / ts_sorted must be ({n},); got {tuple(pix_sorted.shape)}, "
                         f"{tuple(order.shape)}, {tuple(ts_sorted.shape)}")
    if height < 1 or width < 1 or height * width > EVENT_TABLE_MAX_N or n > EVENT_TABLE_MAX_N:
        raise ValueError(f"event_support: {n} events on {width} x {height} pixels: a sensor of at least one pixel, both counts below 2^31")
    if seg.shape != (height * width + 1,):
        raise ValueError(f"event_support: seg must be ({height * width + 1},); got {tuple(seg.shape)}")
    if hot is not None and hot.shape != (height * width,):
        raise ValueError(f"event_support: hot must be ({height * width},); got {tuple(hot.shape)}")
    want = ((pix_sorted, torch.int32), (order, torch.int64), (ts_sorted, torch.int64), (seg, torch.int32), (hot, torch.uint8))
    for name, (t, dtype) in zip(("pix_sorted", "order", "ts_sorted", "seg", "hot"), want):
        if t is not None and (t.dtype != dtype or t.device != ts_sorted.device):
            raise ValueError(f"event_support: {name} must be {dtype} on {ts_sorted.device}; got {t.dtype} on {t.device}")
    if dt is not None and not 0 <= int(dt) <= INT64_MAX:
        raise ValueError(f"event_support: dt must be in [0, 2^63) or None; got {dt}")
    keep = torch.empty(n, device=ts_sorted.device, dtype=torch.uint8)
    if n == 0:
        return keep
    check(_lib.load().ren_event_support(_ptr(pix_sorted), _ptr(order), _ptr(ts_sorted), _ptr(seg), _ptr(hot), n, height, width,
                                        -1 if dt is None else int(dt), int(bool(include_self)), _ptr(keep), _stream()),
          "ren_event_support")
    return keep


# ------------------------------------------------------------------------------- mesh (level set of a density lattice)
MESH_MAX_POINTS = 2 ** 30            # include/ren_amd.h REN_MESH_MAX_POINTS
MESH_MAX_VERTS = 2 ** 31             # the vertex total must stay below it: faces are int32


def _mesh_lattice(sigma: torch.Tensor, level: float, what: str):
    if sigma.dim() != 3 or min(sigma.shape) < 2:
        raise ValueError(f"{what}: sigma must be (nx, ny, nz) with every extent >= 2; got {tuple(sigma.shape)}")
    if sigma.shape[0] * sigma.shape[1] * sigma.shape[2] > MESH_MAX_POINTS:
        raise ValueError(f"{what}: a lattice of {tuple(sigma.shape)} has more than 2^30 points")
    if math.isnan(float(level)):
        raise ValueError(f"{what}: level is NaN")
    return tuple(int(s) for s in sigma.shape)


def mesh_classify(sigma: torch.Tensor, level: float):
    """sigma (nx, ny, nz) float32 -> mask (n,) uint8: the crossed edges each lattice point owns, vcount (n,) int32 = its
    popcount, fcount ((nx-1)(ny-1)(nz-1),) int32: the triangles of each cube.  A point is inside when sigma >= level
    (include/ren_amd.h "mesh")."""
    nx, ny, nz = _mesh_lattice(sigma, level, "mesh_classify")
    ps = _ptr(sigma, torch.float32)
    dev = sigma.device
    n = nx * ny * nz
    mask = torch.empty(n, device=dev, dtype=torch.uint8)
    vcount = torch.empty(n, device=dev, dtype=torch.int32)
    fcount = torch.empty((nx - 1) * (ny - 1) * (nz - 1), device=dev, dtype=torch.int32)
    check(_lib.load().ren_mesh_classify(ps, nx, ny, nz, _f(level), _ptr(mask), _ptr(vcount), _ptr(fcount), _stream()),
          "ren_mesh_classify")
    return mask, vcount, fcount


def mesh_write(sigma: torch.Tensor, level: float, mask: torch.Tensor, voff: torch.Tensor, foff: torch.Tensor, lo: Sequence[float],
               hi: Sequence[float], n_verts: int, n_faces: int):
    """-> verts (n_verts, 3) float32, faces (n_faces, 3) int32 from mesh_classify's mask and the exclusive prefix sums voff /
    foff (int64, exclusive_scan) of its vcount / fcount, whose totals are n_verts / n_faces.  lo, hi: the world box of the
    lattice; the spacing (hi - lo) / (n - 1) is formed here in float64 and passed as float32.  Zero totals launch nothing."""
    nx, ny, nz = _mesh_lattice(sigma, level, "mesh_write")
    n, cubes = nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)
    n_verts, n_faces = int(n_verts), int(n_faces)
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"mesh_write: the box needs finite lo < hi on every axis; got {lo}, {hi}")
    if mask.shape != (n,) or voff.shape != (n,) or foff.shape != (cubes,):
        raise ValueError(f"mesh_write: mask / voff must be ({n},) and foff ({cubes},)")
    if not 0 <= n_verts < MESH_MAX_VERTS or n_faces < 0:
        raise ValueError(f"mesh_write: {n_verts} vertices: the total must stay below 2^31")
    ptrs = (_ptr(sigma, torch.float32), _ptr(mask, torch.uint8), _ptr(voff, torch.int64), _ptr(foff, torch.int64))
    dev = sigma.device
    verts = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_faces, 3, device=dev, dtype=torch.int32)
    if n_verts == 0 and n_faces == 0:
        return verts, faces
    f3 = ctypes.c_float * 3
    h = [(b - a) / (r - 1) for a, b, r in zip(lo, hi, (nx, ny, nz))]
    check(_lib.load().ren_mesh_write(*ptrs, nx, ny, nz, _f(level), f3(*lo), f3(*hi), f3(*h), n_verts, n_faces, _ptr(verts),
                                     _ptr(faces), _stream()), "ren_mesh_write")
    return verts, faces


def mesh_components(sigma: torch.Tensor, level: float, outside: bool = False):
    """sigma (nx, ny, nz) float32 -> label (nx, ny, nz) int32: the smallest linear index of the point's connected component
    under the marching-tetrahedra edges, -1 for a point that is not selected; size (n,) int32: the points of the component
    rooted there, 0 elsewhere; border (n,) uint8: 1 at the root of a component that touches a face of the lattice.  Selected
    are the inside points (sigma >= level), with `outside` their complement (include/ren_amd.h "mesh components")."""
    nx, ny, nz = _mesh_lattice(sigma, level, "mesh_components")
    ps = _ptr(sigma, torch.float32)
    dev = sigma.device
    n = nx * ny * nz
    label = torch.empty(nx, ny, nz, device=dev, dtype=torch.int32)
    size = torch.empty(n, device=dev, dtype=torch.int32)
    border = torch.empty(n, device=dev, dtype=torch.uint8)
    check(_lib.load().ren_mesh_components(ps, nx, ny, nz, _f(level), 1 if outside else 0, _ptr(label), _ptr(size), _ptr(border),
                                          _stream()), "ren_mesh_components")
    return label, size, border


def mesh_component_apply(sigma: torch.Tensor, label: torch.Tensor, drop: torch.Tensor, value: float,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> a tensor like sigma (float32, any shape): `value` where the point's component is marked (label >= 0 and
    drop[label] != 0; label int32 of sigma's shape, drop (n,) uint8 indexed by root), the bits of sigma elsewhere.  `out`:
    where to write instead of a new tensor; it may be sigma itself."""
    n = sigma.numel()
    if label.shape != sigma.shape or drop.shape != (n,):
        raise ValueError(f"mesh_component_apply: label must be {tuple(sigma.shape)} and drop ({n},)")
    if out is not None and out.shape != sigma.shape:
        raise ValueError(f"mesh_component_apply: out must be {tuple(sigma.shape)}")
    if n > MESH_MAX_POINTS:
        raise ValueError(f"mesh_component_apply: {n} points are more than 2^30")
    if math.isnan(float(value)):
        raise ValueError("mesh_component_apply: value is NaN")
    ptrs = (_ptr(sigma, torch.float32), _ptr(label, torch.int32), _ptr(drop, torch.uint8))
    if out is None:
        out = torch.empty_like(sigma)
    check(_lib.load().ren_mesh_component_apply(*ptrs, n, _f(value), _ptr(out, torch.float32), _stream()),
          "ren_mesh_component_apply")
    return out


# ------------------------------------------------------------------------------- mesh simplify (vertex clustering)
def _simplify_grid(lo: Sequence[float], hi: Sequence[float], grid: Sequence[int], what: str):
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"{what}: the box needs finite lo < hi on every axis; got {lo}, {hi}")
    g = tuple(grid)
    if len(g) != 3 or any(int(v) != v or v < 1 for v in g):
        raise ValueError(f"{what}: the cluster grid is three integers >= 1; got {grid!r}")
    g = tuple(int(v) for v in g)
    if g[0] * g[1] * g[2] > MESH_MAX_POINTS:
        raise ValueError(f"{what}: a cluster grid of {g} has more than 2^30 cells")
    d3 = ctypes.c_double * 3
    return d3(*lo), d3(*hi), g


def _rows(t: torch.Tensor, cols, what: str):
    want = "(n,)" if cols is None else f"(n, {cols})"
    if t.dim() != (1 if cols is None else 2) or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{what} must be {want}; got {tuple(t.shape)}")
    if t.shape[0] >= MESH_MAX_VERTS:
        raise ValueError(f"{what}: {t.shape[0]} rows; the count must stay below 2^31")
    return int(t.shape[0])


def mesh_simplify_cells(verts: torch.Tensor, lo: Sequence[float], hi: Sequence[float], grid: Sequence[int]):
    """verts (V, 3) float32 -> cell (V,) int32: the cluster cell of every vertex, sums (cells, 3) int64 (the bits of uint64)
    and count (cells,) int32 (the bits of uint32): per cell the integer sums of the members' quantised offsets and their
    number (include/ren_amd.h "mesh simplify").  V == 0 launches nothing."""
    plo, phi, g = _simplify_grid(lo, hi, grid, "mesh_simplify_cells")
    pv = _ptr(verts, torch.float32)
    n = _rows(verts, 3, "mesh_simplify_cells: verts")
    dev, cells = verts.device, g[0] * g[1] * g[2]
    cell = torch.empty(n, device=dev, dtype=torch.int32)
    sums = torch.zeros(cells, 3, device=dev, dtype=torch.int64)
    count = torch.zeros(cells, device=dev, dtype=torch.int32)
    check(_lib.load().ren_mesh_simplify_cells(pv, n, plo, phi, *g, _ptr(cell), _ptr(sums), _ptr(count), _stream()),
          "ren_mesh_simplify_cells")
    return cell, sums, count


def mesh_simplify_flags(count: torch.Tensor) -> torch.Tensor:
    """count (cells,) int32 -> flag (cells,) int32: 1 where the cell has a member, for exclusive_scan"""
    pc = _ptr(count, torch.int32)
    n = _rows(count, None, "mesh_simplify_flags: count")
    flag = torch.empty(n, device=count.device, dtype=torch.int32)
    check(_lib.load().ren_mesh_simplify_flags(pc, n, _ptr(flag), _stream()), "ren_mesh_simplify_flags")
    return flag


def mesh_simplify_faces(faces: torch.Tensor, n_verts: int, cell: torch.Tensor, coff: torch.Tensor, clusters: int):
    """faces (F, 3) int32 over n_verts vertices, cell (n_verts,) int32, coff (cells,) int64: the exclusive prefix sum of the
    occupied flags, `clusters` its total -> ids (F, 3) int32: the provisional id of every corner, (-1, -1, -1) for a
    degenerate face; key_a (F,) int32 and key_b (F,) int64: the rotation-invariant key, at their maximum for a degenerate
    face; degenerate (1,) int32: their number.  F == 0 launches nothing."""
    ptrs = (_ptr(faces, torch.int32), _ptr(cell, torch.int32), _ptr(coff, torch.int64))
    n = _rows(faces, 3, "mesh_simplify_faces: faces")
    n_verts, clusters, cells = int(n_verts), int(clusters), _rows(coff, None, "mesh_simplify_faces: coff")
    if cell.shape != (n_verts,) or not 0 <= clusters <= cells:
        raise ValueError(f"mesh_simplify_faces: cell must be ({n_verts},) and clusters in [0, {cells}]")
    dev = faces.device
    ids = torch.empty(n, 3, device=dev, dtype=torch.int32)
    key_a = torch.empty(n, device=dev, dtype=torch.int32)
    key_b = torch.empty(n, device=dev, dtype=torch.int64)
    degenerate = torch.zeros(1, device=dev, dtype=torch.int32)
    check(_lib.load().ren_mesh_simplify_faces(ptrs[0], n, n_verts, ptrs[1], ptrs[2], cells, clusters, _ptr(ids), _ptr(key_a),
                                              _ptr(key_b), _ptr(degenerate), _stream()), "ren_mesh_simplify_faces")
    return ids, key_a, key_b, degenerate


def mesh_simplify_heads(order: torch.Tensor, key_a: torch.Tensor, key_b: torch.Tensor, ids: torch.Tensor, clusters: int):
    """order (F,) int64: the face at every position of the stable lexicographic order by (key_a, key_b) -> keep (F,) int32: 1
    for the first face of every run of equal keys that is not degenerate; used (clusters,) int32: 1 for the provisional ids
    the kept faces reference.  F == 0 launches nothing."""
    ptrs = (_ptr(order, torch.int64), _ptr(key_a, torch.int32), _ptr(key_b, torch.int64), _ptr(ids, torch.int32))
    n = _rows(ids, 3, "mesh_simplify_heads: ids")
    clusters = int(clusters)
    if order.shape != (n,) or key_a.shape != (n,) or key_b.shape != (n,) or not 0 <= clusters <= MESH_MAX_POINTS:
        raise ValueError(f"mesh_simplify_heads: order, key_a and key_b must be ({n},) and clusters in [0, 2^30]")
    keep = torch.zeros(n, device=ids.device, dtype=torch.int32)
    used = torch.zeros(clusters, device=ids.device, dtype=torch.int32)
    check(_lib.load().ren_mesh_simplify_heads(*ptrs, n, clusters, _ptr(keep), _ptr(used), _stream()), "ren_mesh_simplify_heads")
    return keep, used


def mesh_simplify_vertices(sums: torch.Tensor, count: torch.Tensor, coff: torch.Tensor, used: torch.Tensor, uoff: torch.Tensor,
                           lo: Sequence[float], hi: Sequence[float], grid: Sequence[int], n_out: int) -> torch.Tensor:
    """-> verts (n_out, 3) float32: the representative of every used cluster at row uoff[provisional id]; uoff (clusters,)
    int64 the exclusive prefix sum of `used`, n_out its total.  n_out == 0 launches nothing."""
    plo, phi, g = _simplify_grid(lo, hi, grid, "mesh_simplify_vertices")
    ptrs = (_ptr(sums, torch.int64), _ptr(count, torch.int32), _ptr(coff, torch.int64), _ptr(used, torch.int32),
            _ptr(uoff, torch.int64))
    cells, clusters, n_out = g[0] * g[1] * g[2], _rows(used, None, "mesh_simplify_vertices: used"), int(n_out)
    if sums.shape != (cells, 3) or count.shape != (cells,) or coff.shape != (cells,) or uoff.shape != (clusters,):
        raise ValueError(f"mesh_simplify_vertices: sums ({cells}, 3), count / coff ({cells},), uoff ({clusters},) expected")
    if not 0 <= n_out <= clusters <= cells:
        raise ValueError(f"mesh_simplify_vertices: 0 <= n_out <= clusters <= cells; got {n_out}, {clusters}, {cells}")
    verts = torch.empty(n_out, 3, device=sums.device, dtype=torch.float32)
    check(_lib.load().ren_mesh_simplify_vertices(*ptrs, *g, plo, phi, clusters, n_out, _ptr(verts), _stream()),
          "ren_mesh_simplify_vertices")
    return verts


def mesh_simplify_compact_faces(ids: torch.Tensor, keep: torch.Tensor, foff: torch.Tensor, uoff: torch.Tensor,
                                n_out: int) -> torch.Tensor:
    """-> faces (n_out, 3) int32: the kept faces in input order with their final vertex ids uoff[provisional id]; foff (F,)
    int64 the exclusive prefix sum of keep, n_out its total.  n_out == 0 launches nothing."""
    ptrs = (_ptr(ids, torch.int32), _ptr(keep, torch.int32), _ptr(foff, torch.int64), _ptr(uoff, torch.int64))
    n, clusters, n_out = _rows(ids, 3, "mesh_simplify_compact_faces: ids"), _rows(uoff, None, "mesh_simplify_compact_faces: uoff"), int(n_out)
    if keep.shape != (n,) or foff.shape != (n,) or not 0 <= n_out <= n or clusters > MESH_MAX_POINTS:
        raise ValueError(f"mesh_simplify_compact_faces: keep / foff must be ({n},), n_out in [0, {n}], at most 2^30 clusters")
    faces = torch.empty(n_out, 3, device=ids.device, dtype=torch.int32)
    check(_lib.load().ren_mesh_simplify_compact_faces(*ptrs, n, clusters, n_out, _ptr(faces), _stream()),
          "ren_mesh_simplify_compact_faces")
    return faces


# ------------------------------------------------------------------------------- mesh distance (grid nearest neighbour)
NN_MAX_EXTENT = 512                  # include/ren_amd.h REN_NN_MAX_EXTENT


def _nn_grid(lo: Sequence[float], h: float, grid: Sequence[int], what: str):
    """-> (lo as float[3], h and its reciprocal as the float32 values the kernels get, the extents)"""
    lo = [float(v) for v in lo]
    if len(lo) != 3 or not all(math.isfinite(v) and abs(v) <= 3.4028234663852886e38 for v in lo):
        raise ValueError(f"{what}: lo is three finite float32 values; got {lo}")
    g = tuple(grid)
    if len(g) != 3 or any(int(v) != v or not 1 <= v <= NN_MAX_EXTENT for v in g):
        raise ValueError(f"{what}: the grid is three integers in [1, {NN_MAX_EXTENT}]; got {grid!r}")
    h32 = ctypes.c_float(float(h)).value
    if not (math.isfinite(h32) and 2.0 ** -100 <= h32 <= 2.0 ** 100):
        raise ValueError(f"{what}: the cell edge h must be a float32 in [2^-100, 2^100]; got {h!r}")
    return (ctypes.c_float * 3)(*lo), h32, ctypes.c_float(1.0 / h32).value, tuple(int(v) for v in g)


def nn_cells(pts: torch.Tensor, lo: Sequence[float], h: float, grid: Sequence[int]) -> torch.Tensor:
    """pts (n, 3) float32 -> cell (n,) int32: the linear id (z * gy + y) * gx + x of each point's cell in the grid of cubic
    cells of edge h from the corner lo, per axis clamp(floor((p - lo) * float32(1 / h)), 0, g - 1) in float32 (include/ren_amd.h
    "mesh distance").  n == 0 launches nothing."""
    plo, _, inv_h, g = _nn_grid(lo, h, grid, "nn_cells")
    n = _rows(pts, 3, "nn_cells: pts")
    pp = _ptr(pts, torch.float32)
    cell = torch.empty(n, device=pts.device, dtype=torch.int32)
    check(_lib.load().ren_nn_cells(pp, n, plo, _f(inv_h), *g, _ptr(cell), _stream()), "ren_nn_cells")
    return cell


def nn_search(queries: torch.Tensor, ref_records: torch.Tensor, cell_start: torch.Tensor, lo: Sequence[float], h: float,
              grid: Sequence[int]):
    """queries (nq, 3) float32; ref_records (nr, 4) float32: the references grouped by their nn_cells id, row = (x, y, z, the
    bits of the original index); cell_start (gx gy gz + 1,) int32: the records of cell c are [cell_start[c], cell_start[c + 1])
    -> d2 (nq,) float32, idx (nq,) int32: the smallest float32 squared distance to a reference and the smallest original index
    that attains it (include/ren_amd.h "mesh distance"), one query per lane in the given order.  nq == 0 launches nothing."""
    plo, h32, inv_h, g = _nn_grid(lo, h, grid, "nn_search")
    nq, nr = _rows(queries, 3, "nn_search: queries"), _rows(ref_records, 4, "nn_search: ref_records")
    if cell_start.shape != (g[0] * g[1] * g[2] + 1,):
        raise ValueError(f"nn_search: cell_start must be ({g[0] * g[1] * g[2] + 1},) for the grid {g}; got {tuple(cell_start.shape)}")
    ptrs = (_ptr(queries, torch.float32), _ptr(ref_records, torch.float32), _ptr(cell_start, torch.int32))
    d2 = torch.empty(nq, device=queries.device, dtype=torch.float32)
    idx = torch.empty(nq, device=queries.device, dtype=torch.int32)
    check(_lib.load().ren_nn_search(ptrs[0], nq, ptrs[1], ptrs[2], nr, plo, _f(h32), _f(inv_h), *g, _ptr(d2), _ptr(idx), _stream()),
          "ren_nn_search")
    return d2, idx


# ------------------------------------------------------------------------------- tsdf (fusion of depth maps into a lattice)
TSDF_VIEW_BATCH = 16                 # include/ren_amd.h REN_TSDF_VIEW_BATCH
TSDF_MAX_IMAGE = 16384               # include/ren_amd.h REN_TSDF_MAX_IMAGE


def _pos_f32(v, what: str) -> float:
    v32 = ctypes.c_float(float(v)).value
    if not (math.isfinite(v32) and v32 > 0):
        raise ValueError(f"{what} must be a positive finite float32; got {v!r}")
    return v32


def tsdf_integrate(depth: torch.Tensor, cams: torch.Tensor, K, lo: Sequence[float], hi: Sequence[float], res: Sequence[int],
                   trunc: float, z_min: float, sum: torch.Tensor, count: torch.Tensor) -> None:
    """depth (V, H, W) float32 z-depth maps (+inf: nothing met; NaN or <= 0: no information), cams (V, 12) float32 (centre, then
    the camera-to-world rotation row-major), K the 3 x 3 upper-triangular pinhole matrix (a tensor or nested sequence; k00, k01,
    k02, k11, k12 are read), the lattice of `res` = (nx, ny, nz) points over the box [lo, hi] -> sum (nx, ny, nz) float32 and
    count (nx, ny, nz) int32 UPDATED IN PLACE: per point and view, the truncated signed distance D - z over trunc, 1 at and
    beyond trunc, skipped below -trunc, at the nearest pixel (include/ren_amd.h "tsdf").  V == 0 launches nothing."""
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError(f"tsdf_integrate: the box needs finite lo < hi on every axis; got {lo}, {hi}")
    r = tuple(res)
    if len(r) != 3 or any(int(v) != v or v < 2 for v in r):
        raise ValueError(f"tsdf_integrate: the resolution is three integers >= 2; got {res!r}")
    r = tuple(int(v) for v in r)
    if r[0] * r[1] * r[2] > MESH_MAX_POINTS:
        raise ValueError(f"tsdf_integrate: a lattice of {r} has more than 2^30 points")
    if depth.dim() != 3 or cams.dim() != 2 or cams.shape != (depth.shape[0], 12):
        raise ValueError(f"tsdf_integrate: depth must be (V, H, W) and cams (V, 12); got {tuple(depth.shape)}, {tuple(cams.shape)}")
    n_views, height, width = (int(v) for v in depth.shape)
    if height > TSDF_MAX_IMAGE or width > TSDF_MAX_IMAGE or n_views * height * width >= 2 ** 31:
        raise ValueError(f"tsdf_integrate: images of at most {TSDF_MAX_IMAGE} pixels a side and fewer than 2^31 pixels a call; "
                         f"got {tuple(depth.shape)}")
    if tuple(sum.shape) != r or tuple(count.shape) != r:
        raise ValueError(f"tsdf_integrate: sum and count must be {r}; got {tuple(sum.shape)}, {tuple(count.shape)}")
    k = torch.as_tensor(K, dtype=torch.float32).cpu()
    if k.shape != (3, 3):
        raise ValueError(f"tsdf_integrate: K must be 3 x 3; got {tuple(k.shape)}")
    k5 = (ctypes.c_float * 5)(float(k[0, 0]), float(k[0, 1]), float(k[0, 2]), float(k[1, 1]), float(k[1, 2]))
    trunc, z_min = _pos_f32(trunc, "tsdf_integrate: trunc"), _pos_f32(z_min, "tsdf_integrate: z_min")
    ptrs = (_ptr(depth, torch.float32), _ptr(cams, torch.float32), _ptr(sum, torch.float32), _ptr(count, torch.int32))
    d3 = ctypes.c_double * 3
    step = [(b - a) / (n - 1) for a, b, n in zip(lo, hi, r)]
    check(_lib.load().ren_tsdf_integrate(ptrs[0], n_views, height, width, ptrs[1], k5, d3(*lo), d3(*step), *r, _f(trunc), _f(z_min),
                                         ptrs[2], ptrs[3], _stream()), "ren_tsdf_integrate")


# ------------------------------------------------------------------------------- loss / optimiser
ERR_FN ={"l1": 0, "mse": 1, "mape": 2}


PARAM_WEIGHT_POWER = {None: 0, "mean_contrast_reciprocal": 1, "mean_contrast_reciprocal_sq": 2}


def event_prepare(batch, c_p: float, c_n: float, tau: float, *, with_grad_ts: bool = False, with_dtau: bool = False, ep=None):
    """a2-a4 in one launch -> dict(ts (2B,) f64 [start | end], target_diff f32, ts_grad, target_grad, dts_start,
    dts_end, dts_grad) -- the optional entries are None unless asked for.  ep: device-resident event parameters
    (event_params_refresh); c_p / c_n / tau are then ignored."""
    st, en = batch["start_ts"], batch["end_ts"]
    B, dev = st.shape[0], st.device
    ts = torch.empty(2 * B, device=dev, dtype=torch.float64)
    target = torch.empty(B, device=dev, dtype=torch.float32)
    ts_g = torch.empty(B, device=dev, dtype=torch.float64) if with_grad_ts else None
    target_g = torch.empty(B, device=dev, dtype=torch.float32) if with_grad_ts else None
    dts = torch.empty(3 if with_grad_ts else 2, B, device=dev, dtype=torch.float64) if with_dtau else None
    check(_lib.load().ren_event_prepare(
        _ptr(st, torch.int64), _ptr(en, torch.int64), _ptr(batch["num_pos"], torch.int64), _ptr(batch["num_neg"], torch.int64),
        _ptr(batch["u_ts_diff"], torch.float64), _ptr(batch["u_diff_start"], torch.float64),
        _ptr(batch["u_grad"], torch.float64) if with_grad_ts else None, B, _f(c_p), _f(c_n), ctypes.c_double(float(tau)),
        _ptr(ts), _ptr(ts[B:]) if B else None, _ptr(target), _ptr(ts_g), _ptr(target_g),
        _ptr(dts[0]) if with_dtau else None, _ptr(dts[1]) if with_dtau else None,
        _ptr(dts[2]) if (with_dtau and with_grad_ts) else None, _ptr(ep, torch.float64), _stream()), "ren_event_prepare")
    return dict(ts=ts, target_diff=target, ts_grad=ts_g, target_grad=target_g,
                dts_start=dts[0] if with_dtau else None, dts_end=dts[1] if with_dtau else None,
                dts_pair=dts[:2].reshape(-1) if with_dtau else None,          # [d ts_start/d tau | d ts_end/d tau], (2B,) view
                dts_grad=dts[2] if (with_dtau and with_grad_ts) else None)


def event_param_grad(kind: str, err_fn: str, param_weight, pred, valid, batch, c_p: float, c_n: float, raw_ratio: float,
                     tau: float, weight: float, ct_grad=None, tau_grad=None, ep=None):
    """closed-form d(loss term)/d(raw ratio) += ct_grad[0], direct d(loss term)/d(tau) += tau_grad[0] (f64)"""
    check(_lib.load().ren_event_param_grad(
        {"diff": 0, "grad": 1}[kind], ERR_FN[err_fn], PARAM_WEIGHT_POWER[param_weight], _ptr(pred, torch.float32), _ptr(valid),
        _ptr(batch["start_ts"], torch.int64), _ptr(batch["end_ts"], torch.int64), _ptr(batch["num_pos"], torch.int64),
        _ptr(batch["num_neg"], torch.int64), _ptr(batch["u_ts_diff"], torch.float64), pred.shape[0], _f(c_p), _f(c_n),
        _f(raw_ratio), ctypes.c_double(float(tau)), _f(weight), _ptr(ct_grad, torch.float32), _ptr(tau_grad, torch.float64),
        _ptr(ep, torch.float64), _stream()), "ren_event_param_grad")


EP_CP, EP_CN, EP_RAW, EP_TAU, EP_INV_C, EP_INV_C2, EP_TAU_RAW = range(7)     # layout of the device-resident event parameters


def event_params_refresh(ct_raw, c_n: float, tau_raw, tau_max: float, ep):
    """ep (f64[8], device) <- C_p, C_n, raw ratio, tau, 1/C, 1/C^2, clamped raw tau from the raw (trainable) forms"""
    check(_lib.load().ren_event_params_refresh(_ptr(ct_raw, torch.float32), _f(c_n), _ptr(tau_raw, torch.float64),
                                               ctypes.c_double(float(tau_max)), _ptr(ep, torch.float64), _stream()),
          "ren_event_params_refresh")


def tau_adam_step(tau_raw, tau_grad, state, tau_max: float, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, step: int,
                  grad_scale: float = 1.0):
    check(_lib.load().ren_tau_adam_step(_ptr(tau_raw, torch.float64), _ptr(tau_grad, torch.float64), _ptr(state, torch.float64),
                                        ctypes.c_double(float(tau_max)), ctypes.c_double(float(lr)), ctypes.c_double(betas[0]),
                                        ctypes.c_double(betas[1]), ctypes.c_double(eps), int(step), ctypes.c_double(grad_scale),
                                        _stream()), "ren_tau_adam_step")


def event_loss_fwd(i_start, i_end, target, valid, err_fn: str):
    if err_fn not in ERR_FN:
        raise NotImplementedError(err_fn)
    loss_sum = torch.empty(2, device=i_start.device, dtype=torch.float32)
    check(_lib.load().ren_event_loss_fwd(_ptr(i_start, torch.float32), _ptr(i_end, torch.float32),
                                         _ptr(target, torch.float32), _ptr(valid), i_start.shape[0], ERR_FN[err_fn],
                                         _ptr(loss_sum), _stream()), "ren_event_loss_fwd")
    return loss_sum


def event_loss_bwd(i_start, i_end, target, valid, err_fn: str, scale: float, loss_sum):
    g_s = torch.empty_like(i_start)
    g_e = torch.empty_like(i_end)
    check(_lib.load().ren_event_loss_bwd(_ptr(i_start), _ptr(i_end), _ptr(target), _ptr(valid), i_start.shape[0],
                                         ERR_FN[err_fn], _f(scale), _ptr(loss_sum), _ptr(g_s), _ptr(g_e), _stream()),
          "ren_event_loss_bwd")
    return g_s, g_e


def event_diff_loss(colors, opac, channel_idx, target, err_fn: str, scale: float, min_intensity: float, use_validity: bool,
                    want_pred: bool = False, scale_dev=None):
    """Loss + its gradient straight from the batched start / end render: colors (2B, C), opac (2B,) ->
    dict(loss (device scalar), loss_sum, g_colors (2B, C), intensity (2B,), pred (B,) | None, valid (B,) uint8 | None).
    Two launches (ren_event_diff_loss_fwd / _bwd) instead of the intensity epilogue, mask, loss, scatter and scalar glue."""
    if err_fn not in ERR_FN:
        raise NotImplementedError(err_fn)
    dev = colors.device
    B, C = colors.shape[0] // 2, colors.shape[1]
    lib = _lib.load()
    loss_sum = torch.empty(2, device=dev, dtype=torch.float32)
    args = (_ptr(colors, torch.float32), _ptr(opac, torch.float32), _ptr(channel_idx, torch.uint8), C, _f(min_intensity),
            _ptr(target, torch.float32), 1 if use_validity else 0, B, ERR_FN[err_fn])
    check(lib.ren_event_diff_loss_fwd(*args, _ptr(loss_sum), _stream()), "ren_event_diff_loss_fwd")
    g_colors = torch.empty_like(colors)
    inten = torch.empty(2 * B, device=dev, dtype=torch.float32)
    pred = torch.empty(B, device=dev, dtype=torch.float32) if want_pred else None
    valid = torch.empty(B, device=dev, dtype=torch.uint8) if use_validity else None
    loss = torch.empty((), device=dev, dtype=torch.float32)
    check(lib.ren_event_diff_loss_bwd(*args, _f(scale), _ptr(scale_dev, torch.float64), _ptr(loss_sum), _ptr(g_colors), _ptr(inten),
                                      _ptr(pred), _ptr(valid), _ptr(loss), _stream()), "ren_event_diff_loss_bwd")
    return dict(loss=loss, loss_sum=loss_sum, g_colors=g_colors, intensity=inten, pred=pred, valid=valid)


def bkgd_param_fwd(raw: torch.Tensor, C: int) -> torch.Tensor:
    """softplus of the background parameter (models/nerf.py:81-88), one tiny launch"""
    out = torch.empty(C, device=raw.device, dtype=torch.float32)
    check(_lib.load().ren_bkgd_param_fwd(_ptr(raw, torch.float32), C, _ptr(out), _stream()), "ren_bkgd_param_fwd")
    return out


def bkgd_param_grad(d_bkgd_per_ray: torch.Tensor, raw: torch.Tensor, grad_raw: torch.Tensor):
    """grad_raw[:C] += sigmoid(raw[:C]) * column sums of the per-ray background gradient"""
    rows, C = d_bkgd_per_ray.shape
    scratch = torch.empty(512, device=raw.device, dtype=torch.float32)
    check(_lib.load().ren_bkgd_param_grad(_ptr(d_bkgd_per_ray, torch.float32), rows, C, _ptr(raw, torch.float32),
                                          _ptr(grad_raw, torch.float32), _ptr(scratch), _stream()), "ren_bkgd_param_grad")


def adam_step(p, g, m, v, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step: int, grad_scale=1.0,
              zero_grad=True):
    check(_lib.load().ren_adam_step(_ptr(p, torch.float32), _ptr(g, torch.float32), _ptr(m, torch.float32),
                                    _ptr(v, torch.float32), p.numel(), _f(lr), _f(betas[0]), _f(betas[1]), _f(eps),
                                    _f(weight_decay), int(step), _f(grad_scale), 1 if zero_grad else 0, _stream()),
          "ren_adam_step")


# ---- optimiser state on the device (ABI 25): what a captured step (step_graph.StepGraphs) needs -- include/ren_amd.h
HY_STEP, HY_SKIP, HY_BC1, HY_BC2, HY_TAU_STEP, HY_TAU_BC1, HY_TAU_BC2 = range(7)


def step_tick(hyper, betas=(0.9, 0.999), stats=(), tick_tau: bool = False):
    """advance the device-side Adam step(s) -- or raise the sticky skip word when an overflow word of `stats` (up to two
    int64[4] blocks of scan_guard) is set.  Once per optimiser step, before adam_step_dev / tau_adam_step_dev."""
    st = [s for s in stats if s is not None]
    if len(st) > 2:
        raise ValueError("step_tick: at most two renders' stats")
    st += [None] * (2 - len(st))
    check(_lib.load().ren_step_tick(_ptr(hyper, torch.float64), ctypes.c_double(betas[0]), ctypes.c_double(betas[1]),
                                    _ptr(st[0], torch.int64), _ptr(st[1], torch.int64), 1 if tick_tau else 0, _stream()),
          "ren_step_tick")


def adam_step_dev(p, g, m, v, hyper, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, zero_grad=True):
    check(_lib.load().ren_adam_step_dev(_ptr(p, torch.float32), _ptr(g, torch.float32), _ptr(m, torch.float32),
                                        _ptr(v, torch.float32), p.numel(), _f(lr), _f(betas[0]), _f(betas[1]), _f(eps),
                                        _f(weight_decay), _ptr(hyper, torch.float64), _f(grad_scale), 1 if zero_grad else 0,
                                        _stream()), "ren_adam_step_dev")


def tau_adam_step_dev(tau_raw, tau_grad, state, tau_max: float, hyper, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                      grad_scale: float = 1.0):
    check(_lib.load().ren_tau_adam_step_dev(_ptr(tau_raw, torch.float64), _ptr(tau_grad, torch.float64),
                                            _ptr(state, torch.float64), ctypes.c_double(float(tau_max)),
                                            ctypes.c_double(float(lr)), ctypes.c_double(betas[0]), ctypes.c_double(betas[1]),
                                            ctypes.c_double(eps), _ptr(hyper, torch.float64), ctypes.c_double(grad_scale),
                                            _stream()), "ren_tau_adam_step_dev")


# ------------------------------------------------------------------------------- occupancy grid
def occgrid_cell_points(indices, jitter, roi, res, ct):
    m = indices.shape[0]
    x = torch.empty(m, 3, device=indices.device, dtype=torch.float32)
    valid = torch.empty(m, device=indices.device, dtype=torch.uint8)
    roi_c = (ctypes.c_float * 6)(*[float(v) for v in roi])
    res_c = (ctypes.c_int32 * 3)(*[int(v) for v in res])
    check(_lib.load().ren_occgrid_cell_points(_ptr(indices, torch.int64), _ptr(jitter, torch.float32), m, roi_c, res_c,
                                              ct, _ptr(x), _ptr(valid), _stream()), "ren_occgrid_cell_points")
    return x, valid


def occgrid_ema(occs, indices, valid, sigma, step_sizes, step_size: float, decay: float, scratch=None):
    """scratch (one float per cell): deterministic handling of duplicate cells in `indices` (ren_occgrid_ema_unique)"""
    if scratch is not None:
        check(_lib.load().ren_occgrid_ema_unique(_ptr(occs, torch.float32), _ptr(indices, torch.int64), _ptr(valid),
                                                 _ptr(sigma, torch.float32), _ptr(step_sizes), _f(step_size),
                                                 indices.shape[0], _f(decay), _ptr(scratch, torch.float32), _stream()),
              "ren_occgrid_ema_unique")
        return
    check(_lib.load().ren_occgrid_ema(_ptr(occs, torch.float32), _ptr(indices, torch.int64), _ptr(valid),
                                      _ptr(sigma, torch.float32), _ptr(step_sizes), _f(step_size), indices.shape[0],
                                      _f(decay), _stream()), "ren_occgrid_ema")


def occgrid_binarize(occs, occ_thre: float, binary, scratch):
    check(_lib.load().ren_occgrid_binarize(_ptr(occs, torch.float32), occs.numel(), _f(occ_thre),
                                           _ptr(binary, (torch.uint8, torch.bool)), _ptr(scratch, torch.float32),
                                           _stream()), "ren_occgrid_binarize")


# ------------------------------------------------------------------------------- per-kernel timing
# HIP-event timing of individual launches on the stream they are enqueued on (torch's current
# stream, which is the stream handed to the C ABI).  Used by bench.py for the roofline numbers;
# disabled (zero overhead) otherwise.
_PROFILE = None
_TIMED = ("ray_aabb_intersect", "ray_march_count", "ray_march_write", "exclusive_scan", "visibility",
          "compact_samples", "compact_features", "hashgrid_fwd", "hashgrid_bwd", "hashgrid_bwd_input", "hashgrid_bwd_binned", "hashgrid_bwd_binned_begin",
          "hashgrid_bwd_binned_scatter", "hashgrid_bwd_binned_finish", "mlp_fwd", "mlp_bwd", "mlp_fwd_save",
          "mlp_bwd_saved", "mlp_fwd_x", "mlp_bwd_x", "composite_fwd",
          "composite_bwd", "column_sum", "event_loss_fwd", "event_loss_bwd", "adam_step", "trajectory", "raygen",
          "mesh_simplify_cells", "mesh_simplify_flags", "mesh_simplify_faces", "mesh_simplify_heads", "mesh_simplify_vertices",
          "mesh_simplify_compact_faces")


def profile_start():
    global _PROFILE
    _PROFILE = {}


def profile_stop():
    """-> {kernel family: (launches, total milliseconds)}; synchronises once."""
    global _PROFILE
    prof, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in (prof or {}).items()}


def _wrap(name, fn):
    def timed(*a, **kw):
        if _PROFILE is None or torch.cuda.is_current_stream_capturing():    # (events inside a capture become graph nodes)
            return fn(*a, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **kw)
        e1.record()
        _PROFILE.setdefault(name, []).append((e0, e1))
        return out
    timed.__name__ = fn.__name__
    timed.__doc__ = fn.__doc__
    return timed


for _n in _TIMED:
    globals()[_n] = _wrap(_n, globals()[_n])
