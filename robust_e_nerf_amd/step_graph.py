"""The training step as ONE hipGraph launch (DESIGN.md "Captured step"; the reference's step: models/robust_e_nerf.py:301-517):
the Trainer's cache of captured steps, each replayed whenever its step shape comes round again."""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass, field

import torch

from . import ops
from .sample_counts import pinned_words

GRAPH_CACHE = 8                          # captured steps kept, oldest evicted first


def pick_key(cached, caps, shape, rays, spr):
    """a cached key of this step shape whose capacities c still fit every render's need m = int(rays * spr * 1.08) + 1024 (`spr`:
    learnt samples per ray) as m <= c <= 3 m + 16384 -- a capture costs ~10 steps: kept while the counts drift -- else (caps,) + shape"""
    need = [tuple(int(n * s * 1.08) + 1024 for s in spr) for n in rays]
    for key in cached:
        if key[1:] == shape and all(m <= c <= 3 * m + 16384 for kc, km in zip(key[0], need) for c, m in zip(kc, km)):
            return key
    return (tuple(caps),) + shape


@dataclass
class Capture:                                    # a step being captured: Renderer._capture for the length of the capture only
    pinned: list                                  # pinned count words allocated before it began, one per render
    passes: list = field(default_factory=list)    # its loss passes' (CountLog, aux): every render of the step is one of them


@dataclass
class CapturedStep:
    graph: torch.cuda.CUDAGraph
    batch: dict                          # static inputs (engine.pack_batch views when the captured batch was packed)
    j0: torch.Tensor | None              # static jitter of the l_diff renders (start | end) and of the third render
    j2: torch.Tensor | None
    loss: torch.Tensor
    aux: dict
    passes: list                         # Capture.passes
    caps: tuple                          # the capacities its renders were captured with (key[0])
    ws: torch.Tensor | None              # the binned-scatter staging pool its launches write: held, so no other tensor gets its address
    ms: tuple | None = None              # (ms per replay, ms per eager step) when the capture was timed

    def __contains__(self, k):           # bench.py reads `"ms" in v` and v["ms"] of the cached steps
        return k == "ms" and self.ms is not None

    def __getitem__(self, k):
        return self.ms if k in self else {}[k]          # (KeyError otherwise, as from a dict)


class StepGraphs:
    """(the Trainer passes itself in: a reference back would be a cycle, and a graph the cycle collector frees in a capture aborts)"""

    def __init__(self):
        self.cache = {}                  # key -> CapturedStep, oldest first
        self.bad = {}                    # step shape -> captures that replayed no faster than the eager steps
        self.pool = None                 # the graph memory pool the cached steps share
        self.last_shape, self.streak = None, 0
        self.eager_ev = None             # (step shape, start, end) events of the last eager step in front of a capture

    def find(self, tr, batch, jitter_start, jitter_end, jitter_grad):
        """-> (key, cached step or None); key None: this step cannot be captured.  The steps whose staging pool was reallocated
        go first (Renderer._binned_workspace): the key is a live step's, or holds the capacities a capture would use now."""
        r, t, sc = tr.r, tr.t, tr.r.counts
        self.cache = {k: rec for k, rec in self.cache.items() if rec.ws is r._bin_ws}
        if tr.use_graph is False or not r.field.flat.is_cuda or not tr.device_counts_ok() or \
                sc.spr is None or sc.host_repeat or (jitter_end is not None and jitter_start is None):
            return None, None
        B = batch["position"].shape[0]
        rays = [2 * B] + ([B] if t.w_grad > 0 else [])
        caps = [sc.capacities(n) for n in rays]
        if any(c is None for c in caps):
            return None, None
        sig = tuple(sorted((k, tuple(v.shape), str(v.dtype)) for k, v in batch.items() if isinstance(v, torch.Tensor)))
        shape = (B, float(tr.lr_scale), tr.grad_sampling_mode(), jitter_start is not None, jitter_grad is not None, sig,
                 t.train_contrast_threshold, t.train_refractory_period, float(t.w_grad))
        key = pick_key(self.cache, caps, shape, rays, sc.spr)
        return key, self.cache.get(key)

    def step(self, tr, batch, jitter_start, jitter_end, jitter_grad):
        """replay (or capture, the third time a step shape occurs in a row) -> (loss, aux), or None: run the step eagerly"""
        key, rec = self.find(tr, batch, jitter_start, jitter_end, jitter_grad)
        if key is None:
            self.last_shape = None
            return None
        if rec is None:
            if tr.use_graph is None:                 # auto: the step SHAPE has to keep repeating before a capture is worth it
                if self.bad.get(key[1:], 0) >= 3:
                    return None                      # (captured three times, never replayed faster than the eager step: stays eager)
                self.streak = self.streak + 1 if self.last_shape == key[1:] else 0
                self.last_shape = key[1:]            # (never, under the reference's dynamic batch size: train.py --batch-size-quantum)
                if self.streak < 2:                  # the eager steps in front of a capture are timed: a graph has to beat them
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = tr._step_passes(batch, jitter_start, jitter_end, jitter_grad, optimizer=tr.world_size == 1)
                    e1.record()                      # (what the graph will contain: under data parallelism the passes only)
                    self.eager_ev = (key[1:], e0, e1)
                    if tr.world_size > 1:
                        tr._optimizer_after_passes(out[1])
                    return out
            rec = self._capture(tr, key, batch, jitter_start if jitter_end is None else torch.cat([jitter_start, jitter_end]), jitter_grad)
            if rec is None:
                return None
        self.last_shape = key[1:]
        # inputs -> the graph's static buffers (skipped for a tensor that already IS the static buffer: Trainer.graph_inputs())
        B = batch["position"].shape[0]
        if "_pack" in batch and "_pack" in rec.batch and batch["_pack"].numel() == rec.batch["_pack"].numel():
            copies = [(rec.batch["_pack"], batch["_pack"])]          # (engine.pack_batch: one launch for all fields)
        else:
            copies = [(dst, batch[k]) for k, dst in rec.batch.items() if k != "_pack"]
        copies += [(rec.j0, jitter_start), (rec.j2, jitter_grad)] if jitter_end is None else \
            [(rec.j0[:B], jitter_start), (rec.j0[B:], jitter_end), (rec.j2, jitter_grad)]
        for dst, src in copies:
            if dst is not None and src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        for log, _ in rec.passes:
            log.arm()
        rec.graph.replay()
        tr.graph_replays += 1
        tr.events.mark_stale()
        if not tr.r.counts.settle(rec.passes):              # (the step's aux is the first pass's)
            if tr.world_size > 1:                    # (data parallelism: the graph ends where the gradient exchange begins)
                tr._optimizer_after_passes(rec.aux)
            else:
                tr.opt.advance_host(tr.t.train_refractory_period)
            return rec.loss, rec.aux
        # a count did not fit: the graph's optimiser launches saw the skip word and changed nothing; its passes' gradients go, and
        # the step runs again with host-side counts (data parallelism: by this rank alone, before the collective)
        tr._clear_grads()
        if tr.world_size == 1:
            tr.opt.sync_hyper()
        return tr.r.counts.repeat(tr, lambda: tr._step_passes(batch, jitter_start, jitter_end, jitter_grad))

    def _capture(self, tr, key, batch, jitter_start, jitter_grad) -> CapturedStep | None:
        from .engine import pack_batch
        r = tr.r
        if len(self.cache) >= GRAPH_CACHE:           # oldest out (its memory stays in the shared pool for the others)
            self.cache.pop(next(iter(self.cache)))
        st_batch = pack_batch(batch) if "_pack" in batch else {k: v.clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
        j0, j2 = (j.to(torch.float32).clone() if j is not None else None for j in (jitter_start, jitter_grad))
        if r.cfg.binned_scatter:
            # sized before the capture (nothing (re)allocates inside), with room to spare for a larger step shape later on
            need = max(max(c) for c in key[0])
            if r._bin_ws is None or r._bin_ws.numel() < ops.hashgrid_bwd_binned_workspace_bytes(need):
                r._binned_workspace(2 * need, r.field.flat.device)
        _ = tr.side_stream
        cap = Capture([pinned_words() for _ in key[0]])
        # (a pool lives as long as a graph captured into it: an empty cache starts a new one -- torch asserts on a dead handle)
        if self.pool is None or not self.cache or os.environ.get("REN_STEP_GRAPH_POOL") == "own":
            self.pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        dump = os.environ.get("REN_STEP_GRAPH_DUMP")             # debugging: <prefix><capture number>.dot of every captured step
        if dump:
            g.enable_debug_mode()
        host_state = tr.opt.host_state()
        r._capture = cap
        tr.fronts.reset()                            # (a front of the eager steps is not part of this one, nor this one's of theirs)
        try:
            with torch.cuda.graph(g, pool=self.pool):
                loss, aux = tr._step_passes(st_batch, j0, None, j2, optimizer=tr.world_size == 1)
        except Exception as e:                       # a capture that cannot be made is not an error of the step
            warnings.warn(f"step capture failed ({type(e).__name__}: {e}); this trainer runs eagerly from here on")
            tr.use_graph = False
            return None
        finally:
            r._capture = None
            tr.fronts.reset()
            tr.opt.restore_host_state(host_state)    # (nothing ran; tr.events may stay marked stale: the replay or eager step that follows marks it anyway)
        tr.graph_captures += 1
        if dump:
            g.debug_dump(f"{dump}{tr.graph_captures}.dot")
        rec = CapturedStep(g, st_batch, j0, j2, loss, aux, cap.passes, key[0], r._bin_ws)
        # kept only if it replays faster than the eager steps just before it: which hardware queue a forked graph lands on can
        # make it 25 % slower (DESIGN.md "Captured step", tools/recapture_probe.py).  Timed: three replays that change nothing
        ev = self.eager_ev
        if tr.use_graph is None and ev is not None and ev[0] == key[1:]:
            t_eager, e0, e1 = ev[1].elapsed_time(ev[2]), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tr.opt.raise_skip()                      # (the optimiser's skip word: parameters and moments stay)
            rec.graph.replay()                       # (first replay of a fresh executable: not timed)
            e0.record()
            for _ in range(3):
                rec.graph.replay()
            e1.record()
            tr._clear_grads()
            tr.opt.sync_hyper()
            if tr.t.train_refractory_period or tr.t.train_contrast_threshold:
                tr.events.refresh()
            torch.cuda.synchronize()
            rec.ms = (e0.elapsed_time(e1) / 3, t_eager)
            if rec.ms[0] > 0.97 * t_eager:
                self.bad[key[1:]] = self.bad.get(key[1:], 0) + 1
                self.streak = 1                      # (the next step tries again: up to three attempts per shape)
                return None
        self.cache[key] = rec
        return rec
