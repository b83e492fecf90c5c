"""The work one training step starts early on the Trainer's side stream (DESIGN.md "Captured step", profiles/NOTES.md), as ONE
owned object: what a front holds, who may take it, and when it is void.

Two fronts, both parameter-independent up to (not including) the first host read of a sample count:
  the l_diff front of the NEXT step (prefetch): void unless the step runs on the very batch / jitter objects it was made from,
      unwritten since, over the occupancy grid it marched (StepFronts.key), with frozen C_p / tau;
  the third (l_grad) render's front of THIS step: announced before forward_backward() (begin_grad_sampling), begun inside it,
      taken by the grad_loss_forward_backward() of the same batch and jitter objects (match_grad); void after reset() -- a
      pass that is repeated with host-side counts, a capture."""
from __future__ import annotations

import contextlib
import dataclasses
import os
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass(slots=True)
class DiffFront:
    """Trainer._front: event correction -> supervision timestamps -> poses -> rays of the start and end renders"""
    prep: dict
    jitter: Optional[torch.Tensor]
    o: Optional[torch.Tensor] = None          # rays of both renders (None under trainable tau: the tangent ray generation
    d: Optional[torch.Tensor] = None          # makes them from `px`, which is None otherwise)
    px: Optional[torch.Tensor] = None
    begun: Optional[dict] = None              # Renderer.sample_begin state, "n0" included once the count has been read back


@dataclass(slots=True)
class GradFront:
    """Trainer._grad_front: the third render up to (not including) the first host read"""
    prep: dict
    o: torch.Tensor
    d: torch.Tensor
    od: torch.Tensor
    dd: torch.Tensor
    ddd: Optional[torch.Tensor]
    jit: Optional[torch.Tensor]
    st: Optional[dict]                        # Renderer.sample_begin state (None until the merged march has made it)
    key: Optional[tuple] = None               # (id(batch), id(jitter_grad)) it was announced for
    merged: bool = False                      # marched together with the l_diff render, in order on the main stream
    n_host: Optional[torch.Tensor] = None     # pinned word the count is copied to ...
    ev: Optional[torch.cuda.Event] = None     # ... and the event after that copy (None: device-side counts, or merged)


def _adopt(v, stream):
    """tensors allocated on another stream's pool that `stream` is about to use (after waiting for their producer): tell the
    caching allocator, so that their memory is not handed out again before `stream` is done with them"""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            v.record_stream(stream)
    elif isinstance(v, dict):
        for x in v.values():
            _adopt(x, stream)
    elif isinstance(v, (tuple, list)):
        for x in v:
            _adopt(x, stream)
    elif dataclasses.is_dataclass(v):                            # (DiffFront, engine.Packed)
        _adopt([getattr(v, f.name) for f in dataclasses.fields(v)], stream)


class StepFronts:
    """(the Trainer passes itself in, as to step_graph.StepGraphs)"""

    def __init__(self):
        self._side = None
        self._n_host = self._n_host_grad = None      # pinned count words of the two fronts
        self.prefetched = None                       # (key, DiffFront, event after the count's copy, the inputs: their ids stay taken)
        self.reset()

    def reset(self):
        """this step's third render: nothing announced, begun or ready (the prefetched l_diff front answers to its key alone)"""
        self.pending = None                          # announced: (batch, jitter_grad, event at the announcement | None = merged)
        self.begun: Optional[GradFront] = None
        self.ready_ev = None                         # start of the last forward_backward() on its stream (early="all")

    @property
    def side_stream(self) -> "torch.cuda.Stream":
        if self._side is None:
            # normal priority (round 6; until then -1 = high): with a HIGH-priority stream in the process every other captured
            # step replayed 25 % slower (small kernels of alternate captures took 45-55 us each: tools/recapture_probe.py,
            # profiles/NOTES.md), and the eager lines and the e2e run are the same at either priority
            self._side = torch.cuda.Stream(priority=int(os.environ.get("REN_SIDE_PRIORITY", 0)))
        return self._side

    # ---- the l_diff front of the next step --------------------------------------------------------------------------
    @staticmethod
    def key(r, batch, jitter_start, jitter_end):
        """identity AND in-place version of every tensor the prefetched front was computed from: a batch or jitter tensor
        mutated between prefetch() and forward_backward() (same object ids, new contents) must not reuse the stale front;
        and what the early march of the occupancy sampler read: the grid tensor's torch version and the refresh epoch"""
        ver = lambda t: (id(t), t._version) if isinstance(t, torch.Tensor) else (id(t), 0)
        return (id(batch), tuple(sorted((k, ver(v)) for k, v in batch.items())), ver(jitter_start), ver(jitter_end),
                r.binary._version, getattr(r, "binary_epoch", 0), r.cfg.sampler)

    def prefetch(self, tr, batch, jitter_start=None, jitter_end=None, next_global_step: Optional[int] = None) -> bool:
        t, r = tr.t, tr.r
        if t.train_contrast_threshold or t.train_refractory_period:
            return False
        if r.cfg.sampler != "uniform" and next_global_step is not None and next_global_step % r.cfg.occ_n == 0:
            return False
        side = self.side_stream
        # Ordered AFTER the work already queued on this stream (round 4): run beside the persistent MLP backward kernels, the
        # pose / ray kernels of this front produced a slightly wrong rotation for an aligned group of 16 rays in ~1 step out
        # of 8 (same inputs, same kernel: tools/prefetch_diag2.py; packed-FP32 code beside matrix-core waves, profiles/NOTES.md:
        # those files are now built without it, and this ordering stays as the second line of defence), which is what made
        # test_prefetched_step_front_gives_the_same_steps fail in 40 % of its stand-alone runs.  What is left of the prefetch:
        # the front shares the chip with the optimiser step only, and the host never enqueues it on the critical path.
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            front = tr._front(batch, jitter_start, jitter_end)
            front.begun = st = r.sample_begin(front.o, front.d, front.jitter, True)
            if self._n_host is None:
                self._n_host = torch.empty(1, dtype=st["total"].dtype).pin_memory()
            self._n_host.copy_(st["total"].reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        self.prefetched = (self.key(r, batch, jitter_start, jitter_end), front, ev, (batch, jitter_start, jitter_end))
        return True

    def match_diff(self, tr, batch, jitter_start, jitter_end):
        """consume the prefetched front -> (DiffFront, event), or None: there is none, or it is void for this call"""
        pf, self.prefetched = self.prefetched, None
        if pf is None or pf[0] != self.key(tr.r, batch, jitter_start, jitter_end) or \
                tr.t.train_contrast_threshold or tr.t.train_refractory_period:        # the guards of prefetch(), re-checked
            return None
        return pf[1], pf[2]

    def take_diff(self, tr, batch, jitter_start, jitter_end) -> DiffFront:
        """the front of this forward_backward(): the prefetched one, its count read, or made now"""
        if tr.r.field.flat.is_cuda:
            # everything enqueued so far (the last optimiser step, the occupancy-grid refresh, the batch) is what the sampling
            # of this step's third render depends on: grad_loss_forward_backward(early="all") waits for this point only
            self.ready_ev = torch.cuda.Event()
            self.ready_ev.record()
        pf = self.match_diff(tr, batch, jitter_start, jitter_end)
        if pf is None:
            return tr._front(batch, jitter_start, jitter_end)
        front, ev = pf
        ev.synchronize()                                               # host: waits for the side stream's few small kernels only
        front.begun["n0"] = int(self._n_host[0])
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        _adopt(front, cur)                                             # side-stream allocations now used on this stream
        return front

    # ---- the third render's front of this step ----------------------------------------------------------------------
    def begin_grad_sampling(self, tr, batch, jitter_grad=None, merged: bool = False) -> bool:
        if not tr.r.field.flat.is_cuda or not (tr.t.w_grad > 0):
            return False
        ready = None
        if not merged:
            ready = torch.cuda.Event()
            ready.record()
        self.begun, self.pending = None, (batch, jitter_grad, ready)
        return True

    def begin_with_grad(self, tr, front: DiffFront, o, d, dc) -> Optional[dict]:
        """the l_diff render's sample_begin() state (None: Renderer.sample runs it), with an announced third render's front
        placed as its mode asks: "begun" -- this render's count pass first, then the third render's front on the side stream;
        "merged" -- both renders' rays through one ray / box test and one march count pass, in order on this stream"""
        if self.pending is None:
            return front.begun
        (batch, jitter_grad, ready), self.pending = self.pending, None
        if ready is None:                                         # "merged"
            fr = tr._grad_front(batch, jitter_grad, rays_only=True)
            if (front.jitter is None) != (fr.jit is None):
                raise ValueError("merged sampling: jitter for both the l_diff renders and the third one, or for neither")
            front.begun, fr.st = tr.r.sample_begin_merged([(o, d, front.jitter), (fr.o, fr.d, fr.jit)], True, device_counts=dc)
            fr.merged = True
        else:                                                     # "begun": `ready` is the event at the announcement
            if front.begun is None:                               # (not prefetched)
                front.begun = tr.r.sample_begin(o, d, front.jitter, True, device_counts=dc)
            side = self.side_stream
            side.wait_event(ready)
            with torch.cuda.stream(side):
                fr = tr._grad_front(batch, jitter_grad)
                if fr.st.get("dc") is None:                       # (device-side counts: nothing to read back)
                    if self._n_host_grad is None:
                        self._n_host_grad = torch.empty(1, dtype=fr.st["total"].dtype).pin_memory()
                    self._n_host_grad.copy_(fr.st["total"].reshape(1), non_blocking=True)
                    fr.ev = torch.cuda.Event()
                    fr.ev.record()
            fr.n_host = self._n_host_grad
        fr.key, self.begun = (id(batch), id(jitter_grad)), fr
        return front.begun

    def match_grad(self, batch, jitter_grad, early):
        """consume this step's state -> (the begun front if it was announced for THIS call, else None; the ready event)"""
        begun, ready = self.begun, self.ready_ev
        self.reset()
        if begun is not None and (not early or begun.key != (id(batch), id(jitter_grad))):
            begun = None                                                  # (begin_grad_sampling was for another call)
        return begun, ready

    def sample_grad(self, tr, batch, jitter_grad, early, dc):
        """-> (GradFront, Packed) of the third render, usable on the current stream: the matching begun front or one made now,
        and the rest of its sampling where `early` and the front's placement put it (Trainer.grad_loss_forward_backward)"""
        r, cuda = tr.r, tr.r.field.flat.is_cuda
        begun, ready = self.match_grad(batch, jitter_grad, early)
        if begun is not None and begun.merged:
            early = False                                                 # merged front: the rest follows in order on this stream
        # no matching front: in order, unless the caller asks for the experimental placement (early="all": everything
        # beside the l_diff forward / backward; wrong rays observed there, see Trainer.grad_sampling_mode)
        early = bool(early) and cuda and (begun is not None or (early == "all" and ready is not None))
        main = torch.cuda.current_stream() if cuda else None
        if early and begun is None:
            self.side_stream.wait_event(ready)
        with (torch.cuda.stream(self.side_stream) if early else contextlib.nullcontext()):
            fr = begun if begun is not None else tr._grad_front(batch, jitter_grad)
            if fr.ev is not None:                                         # count pass already ran: its total is in the pinned buffer
                fr.ev.synchronize()
                fr.st["n0"] = int(fr.n_host[0])
            pk = r.sample(fr.o, fr.d, fr.jit, True, begun=fr.st, device_counts=dc)
            if early:
                done = torch.cuda.Event()
                done.record()
        if early:
            main.wait_event(done)
            _adopt((fr.prep, fr.o, fr.d, fr.od, fr.dd, fr.ddd, fr.jit, pk), main)
        return fr, pk
