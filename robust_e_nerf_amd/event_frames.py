"""Event frames: do the recorded events agree with the brightness change the reconstruction predicts?

A real sequence has no ground-truth intensity image at the event camera's poses, so the L1 / PSNR / SSIM epoch of
``evaluation`` has nothing to score; the evidence is the event stream.  Between the times t0 and t1 a pixel u saw n+
positive and n- negative events, and the sensor model the training uses says

    log I(u, t1) - log I(u, t0)  ~  C_p n+ - C_n n-        (to within one threshold).

``accumulate`` bins the raw stream of ``raw_events.npz`` into per-window count images on the GPU (``ops.event_frames``,
integer atomics: exact and bitwise repeatable), ``predicted_change`` renders the left-hand side at the windows' boundary
poses, ``compare`` scores one against the other per window (``ops.event_frame_compare``: fixed-order fp64 sums) and
``frame_png`` shows measured | predicted | residual side by side.  Nothing is simulated: recorded events are counted and
set against two renders.

Limitation: events that the sensor's refractory period suppressed are not added back.  Where a pixel fires faster than tau
the measured image undercounts, and the residual there is the sensor's doing, not the reconstruction's.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import data, evaluation, ops

SUMS = ("count", "sum_m", "sum_p", "sum_mm", "sum_pp", "sum_mp", "sum_sq_diff", "n_explained", "n_active")
FRAME_SPAN = 4.0          # frame_png: the colour code runs over +- FRAME_SPAN mean thresholds
GREY = 128


def window_edges(t_first: int, t_last: int, n_windows: Optional[int] = None, window_ns: Optional[int] = None,
                 start_ns: Optional[int] = None) -> torch.Tensor:
    """(V + 1,) int64 window boundaries inside the trajectory's time span [t_first, t_last] (nanoseconds), from `start_ns`
    (default t_first):  n_windows alone: [start, t_last] split into V windows of equal length (floor division, the last
    edge is t_last);  window_ns alone: as many whole windows of that length as fit;  both: V windows of window_ns."""
    t_first, t_last = int(t_first), int(t_last)
    start = t_first if start_ns is None else int(start_ns)
    if not t_first <= start < t_last:
        raise ValueError(f"window_edges: start {start} outside the trajectory [{t_first}, {t_last})")
    if n_windows is None and window_ns is None:
        raise ValueError("window_edges: give n_windows, window_ns or both")
    if window_ns is not None and int(window_ns) < 1:
        raise ValueError("window_edges: window_ns must be positive")
    if window_ns is None:
        V = int(n_windows)
        if V < 1:
            raise ValueError("window_edges: n_windows must be at least 1")
        return torch.tensor([start + (t_last - start) * k // V for k in range(V + 1)], dtype=torch.int64)
    V = (t_last - start) // int(window_ns) if n_windows is None else int(n_windows)
    if V < 1 or start + V * int(window_ns) > t_last:
        raise ValueError(f"window_edges: {max(V, 1)} window(s) of {int(window_ns)} ns from {start} do not fit before {t_last}")
    return start + int(window_ns) * torch.arange(V + 1, dtype=torch.int64)


def _check_edges(edges) -> torch.Tensor:
    e = torch.as_tensor(edges).detach().to("cpu", torch.int64).reshape(-1)
    if e.numel() < 2:
        raise ValueError("edges must hold at least two times")
    if bool((e[1:] < e[:-1]).any()):
        raise ValueError("edges must be non-decreasing")
    return e


def _position_words(position) -> torch.Tensor:
    """(N, 2) uint16 (x, y) as raw_events.npz stores it -> (N,) int32 words x | y << 16 (a reinterpretation, no arithmetic)"""
    if torch.is_tensor(position):
        if position.dtype == torch.int32 and position.dim() == 1:
            return position
        position = position.detach().cpu().numpy()
    p = np.ascontiguousarray(np.asarray(position))
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"position must be (N, 2); got {p.shape}")
    if p.dtype != np.uint16:
        if p.size and (p.min() < 0 or p.max() > 65535 or np.any(p != np.floor(p))):
            raise ValueError("position must hold integer pixel coordinates below 65536")
        p = p.astype("<u2")
    return torch.from_numpy(np.ascontiguousarray(p.astype("<u2", copy=False)).view("<i4").reshape(-1))


def accumulate(raw, edges, height: int, width: int, device="cuda") -> torch.Tensor:
    """`raw`: the three arrays of raw_events.npz (a mapping with position (N, 2) uint16 x, y; timestamp (N,) int64 ns in
    time order; polarity (N,) bool), numpy or torch on any device; moved to the GPU once.  `edges`: (V + 1,) non-decreasing
    window boundaries (ValueError otherwise); event e falls into window v iff edges[v] <= t_e < edges[v + 1].
    -> counts (V, 2, H, W) int32 on the GPU, plane 0 positive and plane 1 negative events."""
    e = _check_edges(edges)
    words = _position_words(raw["position"]).to(device)
    ts = torch.as_tensor(np.asarray(raw["timestamp"]) if not torch.is_tensor(raw["timestamp"]) else raw["timestamp"])
    pol = torch.as_tensor(np.asarray(raw["polarity"]) if not torch.is_tensor(raw["polarity"]) else raw["polarity"])
    ts = ts.to(device, torch.int64).contiguous()
    pol = (pol if pol.dtype in (torch.bool, torch.uint8) else pol != 0).to(device).contiguous()
    if not (words.shape[0] == ts.shape[0] == pol.shape[0]):
        raise ValueError(f"raw events: {words.shape[0]} positions, {ts.shape[0]} timestamps, {pol.shape[0]} polarities")
    return ops.event_frames(words, ts, pol, e.to(device), int(height), int(width))


def measured_change(counts: torch.Tensor, c_p: float, c_n: float) -> torch.Tensor:
    """counts (V, 2, H, W) -> float32 (V, H, W): C_p n+ - C_n n-, formed in float64"""
    return (float(c_p) * counts[:, 0].double() - float(c_n) * counts[:, 1].double()).float()


def bayer_channels(height: int, width: int, bayer_pattern: str, device) -> torch.Tensor:
    """(H, W) int64 colour channel of every sensor pixel by the rule of data.colorize_events (pattern: TL, TR, BL, BR)"""
    chan = torch.tensor([data.COLOR_CHANNEL[c] for c in bayer_pattern], dtype=torch.int64, device=device)
    ys, xs = torch.meshgrid(torch.arange(height, device=device), torch.arange(width, device=device), indexing="ij")
    return chan[(xs % 2) + 2 * (ys % 2)]


def _is_distorted(calib) -> bool:
    if calib is None or "distortion_params" not in calib:
        return False
    dist = np.asarray(calib["distortion_params"]).reshape(-1)
    return len(dist) != 0 and bool(np.any(dist != 0))


@torch.no_grad()
def predicted_change(r, Kinv: torch.Tensor, tab_ts, tab_pos, tab_quat, edges, height: int, width: int,
                     bkgd: Optional[torch.Tensor] = None, calib=None, bayer_pattern: str = ""):
    """The model's side: one log-intensity image per DISTINCT edge (contiguous windows share their boundary render), at the
    pose ops.trajectory interpolates for it, through evaluation.render_image -- or, for a distorted sensor (`calib` with
    non-zero distortion_params), through evaluation.render_pixels at data.undistort_points of the integer pixel grid: the
    events stay at their integer sensor pixels, the rays go where those pixels look.  A Bayer sensor (radiance_dim 3,
    `bayer_pattern`) takes each pixel's own colour channel (data.colorize_events).
    -> pred (V, H, W) float32 = log I(edges[v + 1]) - log I(edges[v]);  valid (V, H, W) bool, the AND of both renders'
    is_valid (opacity > 0 without a background colour, everything with one)."""
    e = _check_edges(edges)
    dev = Kinv.device
    uniq, inverse = torch.unique(e, return_inverse=True)
    pos, rot = ops.trajectory(uniq.to(dev, torch.float64), tab_ts.to(dev), tab_pos.to(dev), tab_quat.to(dev))
    C = r.field.C
    if C > 1 and len(bayer_pattern) != 4:
        raise ValueError(f"a field with {C} radiance channels needs the sensor's bayer_pattern")
    chan = bayer_channels(height, width, bayer_pattern, dev) if C > 1 else None
    px = None
    if _is_distorted(calib):
        grid = evaluation.pixel_grid(height, width, "cpu").reshape(-1, 2).numpy().astype(np.float64)
        und = data.undistort_points(grid, np.asarray(calib["intrinsics"], np.float64),
                                    np.asarray(calib["distortion_params"]).reshape(-1), str(calib["distortion_model"]))
        px = torch.from_numpy(und.astype(np.float32)).to(dev).contiguous()
    logs, oks = [], []
    for k in range(uniq.shape[0]):
        if px is None:
            img, opac, _ = evaluation.render_image(r, Kinv, pos[k], rot[k].contiguous(), height, width, bkgd)
            ok = torch.ones_like(opac, dtype=torch.bool) if bkgd is not None else opac > 0
        else:
            n = px.shape[0]
            inten, _, _, _, ok = evaluation.render_pixels(r, Kinv, px, pos[k].reshape(1, 3).expand(n, 3).contiguous(),
                                                          rot[k].reshape(1, 3, 3).expand(n, 3, 3).contiguous(), bkgd)
            img = inten.view(height, width) if C == 1 else inten.view(height, width, C).permute(2, 0, 1)
            ok = ok.view(height, width)
        if C > 1:
            img = img.gather(0, chan[None])[0]
        logs.append(img.log())
        oks.append(ok)
    logs, oks = torch.stack(logs), torch.stack(oks)
    lo, hi = inverse[:-1].to(dev), inverse[1:].to(dev)
    return logs[hi] - logs[lo], oks[hi] & oks[lo]


def scores_from_sums(sums: torch.Tensor, c_p: float, c_n: float) -> dict:
    """(V, 9) float64 sums of ops.event_frame_compare -> the per-window scores of `compare` (CPU tensors, float64):
    corr = cov(m, p) / sqrt(var m var p) with var x = sum x^2 - (sum x)^2 / n, NaN when n_valid == 0 or either variance is
    zero -- a variance not above the round-off of its own sums, 4 n 2^-52 sum x^2, counts as zero."""
    s = sums.detach().to("cpu", torch.float64)
    n, sm, sp, smm, spp, smp, sdd, n_expl, n_act = s.unbind(1)
    nan = torch.full_like(n, float("nan"))
    has = n > 0
    nn = n.clamp_min(1.0)
    var_m, var_p = smm - sm * sm / nn, spp - sp * sp / nn
    floor_m, floor_p = 4 * nn * 2.0 ** -52 * smm, 4 * nn * 2.0 ** -52 * spp
    defined = has & (var_m > floor_m) & (var_p > floor_p)
    den = (var_m.clamp_min(0) * var_p.clamp_min(0)).sqrt()
    corr = torch.where(defined, (smp - sm * sp / nn) / torch.where(defined, den, torch.ones_like(den)), nan)
    mean_c = (float(c_p) + float(c_n)) / 2
    rmse = torch.where(has, (sdd / nn).sqrt() / mean_c, nan)
    expl = torch.where(has, n_expl / nn, nan)

    def mean(x):
        x = x[has]
        x = x[~x.isnan()]
        return float(x.mean()) if x.numel() else float("nan")
    return dict(n_valid=n.to(torch.int64), n_active=n_act.to(torch.int64), corr=corr, rmse_over_c=rmse, explained=expl,
                mean_corr=mean(corr), mean_rmse_over_c=mean(rmse), mean_explained=mean(expl), sums=s)


def compare(counts: torch.Tensor, pred: torch.Tensor, valid: torch.Tensor, c_p: float, c_n: float) -> dict:
    """Per window, over the valid pixels: n_valid; n_active (pixels with at least one event); Pearson `corr` of measured and
    predicted change (NaN when either has no variance or nothing is valid); rmse_over_c = sqrt(mean (p - m)^2) / ((C_p +
    C_n) / 2); `explained`, the share of pixels with |p - m| <= max(C_p, C_n); and mean_corr / mean_rmse_over_c /
    mean_explained over the windows that have valid pixels (windows whose corr is undefined are left out of mean_corr)."""
    return scores_from_sums(ops.event_frame_compare(counts, pred, valid, c_p, c_n), c_p, c_n)


def _diverging(x: torch.Tensor, scale: float) -> torch.Tensor:
    """(H, W) -> uint8 (H, W, 3): 0 white, +scale and above full red, -scale and below full blue, linear between"""
    v = (x.to(torch.float32) / scale).clamp(-1, 1)
    fade = (255 * (1 - v.abs())).round()
    full = torch.full_like(fade, 255.0)
    red, blue = torch.where(v >= 0, full, fade), torch.where(v <= 0, full, fade)
    return torch.stack([red, fade, blue], -1).to(torch.uint8)


def frame_png(measured: torch.Tensor, predicted: torch.Tensor, valid: torch.Tensor, c_mean: float,
              span: float = FRAME_SPAN) -> torch.Tensor:
    """One window as a picture: uint8 (H, 3 W, 3) on the CPU, the panels measured | predicted | residual (predicted -
    measured) in ONE diverging colour code, symmetric about zero: white = no change, red = brighter, blue = darker, full
    colour at +- span x c_mean (default 4 mean thresholds (C_p + C_n) / 2: four events of one sign saturate).  Pixels with
    valid == 0 are grey (128) in all three panels."""
    m, p = measured.detach().cpu().to(torch.float32), predicted.detach().cpu().to(torch.float32)
    ok = valid.detach().cpu().to(torch.bool)
    if not (m.dim() == 2 and m.shape == p.shape == ok.shape):
        raise ValueError(f"frame_png takes three (H, W) images; got {tuple(m.shape)}, {tuple(p.shape)}, {tuple(ok.shape)}")
    scale = float(span) * float(c_mean)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("frame_png: span x c_mean must be positive")
    panels = []
    for x in (m, p, p - m):
        u8 = _diverging(x, scale)
        u8[~ok] = GREY
        panels.append(u8)
    return torch.cat(panels, dim=1).contiguous()
