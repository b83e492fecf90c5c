"""The device-side sample counts of the occupancy-sampled training renders (RenderCfg.device_counts, DESIGN.md §6 "Device-side
sample counts"), as ONE owned object -- Renderer.counts, which the Trainer and step_graph.StepGraphs use as well:
  capacities: a render's arrays are sized from the samples per ray (marched, kept) learnt from the renders before it;
  logs:       its two counts, and whether they fitted, travel to pinned words behind the sampling kernels (CountLog) -- a ring
              of the Renderer's for eager renders, words of its own for a captured step;
  repeats:    the host looks at them when the pass is in the queue; a pass with a count that did not fit runs again with
              host-side counts."""
from __future__ import annotations

import torch


def pinned_words() -> torch.Tensor:
    """where the host finds one render's (marched, overflowed, kept, overflowed): CountLog's `pinned`"""
    return torch.empty(4, dtype=torch.int64).pin_memory()


def device_words(device):
    """-> (stats, nd): the four words the two guards of one render write (CountLog's `stats`) and its two counts, on the device"""
    return torch.empty(4, device=device, dtype=torch.int64), torch.empty(2, device=device, dtype=torch.int64)


class CountLog:
    """The two sample counts of one render sampled with device-side counts -- marched, kept -- and whether they fitted the
    capacities the arrays were given: copied to pinned memory behind the sampling kernels.  wait() blocks the host until
    THOSE kernels are done (an event), not until the queue is empty.
    polled=True (a render inside a captured step, step_graph.StepGraphs): the copy is a node of the graph and no event can be
    waited for; the host arms the pinned words with -1 before every replay (arm()) and wait() spins until the copy has
    landed -- pinned host memory is coherent, and each of the four words is one aligned 8-byte store."""

    def __init__(self, n_rays: int, caps, stats: torch.Tensor, pinned: torch.Tensor, polled: bool = False):
        self.n_rays, self.caps, self.stats = n_rays, caps, stats
        pinned.copy_(stats, non_blocking=True)
        self._pinned = pinned
        self.ev = None
        if not polled:
            self.ev = torch.cuda.Event()
            self.ev.record()
        self.values = None                       # (marched, overflowed, kept, overflowed)

    def arm(self):
        self._pinned.fill_(-1)
        self.values = None

    def wait(self):
        if self.values is None:
            if self.ev is not None:
                self.ev.synchronize()
                self.values = tuple(int(v) for v in self._pinned.tolist())
            else:
                import time
                t0 = time.monotonic()
                while True:
                    v = self._pinned.tolist()
                    if min(v) >= 0:
                        break
                    if time.monotonic() - t0 > 120.0:         # (a replay that died: fail loudly instead of spinning for ever)
                        torch.cuda.synchronize()
                        raise RuntimeError("captured step: the sample counts of a replay never arrived")
                self.values = tuple(int(x) for x in v)
        return self.values

    @property
    def overflowed(self) -> bool:
        v = self.wait()
        return bool(v[1] or v[3])


class SampleCounts:
    """(the Trainer passes itself in, as to step_graph.StepGraphs)"""

    MARGIN, SLACK, MAX = 1.25, 4096, 1 << 23      # (from 2^23 samples on the chunked two-stream paths take over)

    def __init__(self):
        # samples per ray (marched, kept) the capacities are derived from, learnt from the renders themselves -- the first one
        # reads its counts on the host -- and a ring of pinned buffers (pinned at the first render with device-side counts)
        self.spr = None
        self._ring, self._logs, self._at = None, [None] * 16, 0
        # a pass is being repeated with host-side counts; how many were
        self.host_repeat, self.overflows = False, 0

    def capacities(self, n_rays: int):
        if self.spr is None:
            return None
        def bucket(x):                                   # 8 sizes per octave: the allocator sees repeating sizes while
            q = max(1024, 1 << max(0, x.bit_length() - 4))      # the ray count drifts (update_train_batch_size)
            return (x + q - 1) // q * q
        caps = tuple(bucket(int(n_rays * s * self.MARGIN) + self.SLACK) for s in self.spr)
        return None if max(caps) >= self.MAX else caps

    def learn(self, n_rays: int, marched: int, kept: int):
        """capacities follow the counts: up at once, down slowly (the occupancy grid prunes over the first epochs)"""
        m = (marched / max(n_rays, 1), kept / max(n_rays, 1))
        self.spr = m if self.spr is None else tuple(max(a, 0.75 * b + 0.25 * a) for a, b in zip(m, self.spr))

    def log(self, n_rays: int, caps, stats: torch.Tensor, capture) -> CountLog:
        if capture is not None:                                  # inside a capture: the graph owns its pinned words
            return CountLog(n_rays, caps, stats, capture.pinned.pop(), polled=True)   # (pinned before the capture began)
        if self._ring is None:
            self._ring = [pinned_words() for _ in range(16)]
        k = self._at = (self._at + 1) % 16
        if self._logs[k] is not None:
            self._logs[k].wait()                             # (its pinned buffer is about to be reused)
        log = self._logs[k] = CountLog(n_rays, caps, stats, self._ring[k])
        return log

    def mode(self, ok: bool):
        """what this step's renders pass to Renderer.sample: True (counts stay on the device), "learn" (host counts, but the
        capacities learn from them) or False.  ok: Trainer.device_counts_ok()"""
        if not ok:
            return False
        return "learn" if self.host_repeat else True

    def run_pass(self, tr, fn, args):
        """Run one loss pass (`fn(*args, dc)` -> loss, aux, CountLog | None) with its sample counts on the device, then look
        at them (settle; its field evaluation and backward are still in the queue).  A count that did not fit its arrays left
        the render empty: the scalar parameters' gradient block is put back and the pass runs again with host-side counts."""
        dc, cap = self.mode(tr.device_counts_ok()), tr.r._capture
        snap = tr._gs.clone() if dc is True and cap is None else None
        loss, aux, log = fn(*args, dc)
        if cap is not None:                                  # StepGraphs looks at the counts after every replay
            if log is None:
                raise RuntimeError("a captured step needs every render on device-side counts")
            cap.passes.append((log, aux))
        elif log is not None and self.settle([(log, aux)]):
            tr._gs.copy_(snap)           # (not _clear_grads: this pass added nothing to the table / MLP gradients, earlier ones did)
            loss, aux, _ = self.repeat(tr, lambda: fn(*args, self.mode(tr.device_counts_ok())))
        return loss, aux

    def settle(self, passes) -> bool:
        """wait for the counts of loss passes [(CountLog, aux), ...] -> whether one did not fit; else the capacities and auxes get them"""
        vals = [log.wait() for log, _ in passes]
        if any(v[1] or v[3] for v in vals):
            return True
        for (log, aux), v in zip(passes, vals):
            self.learn(log.n_rays, v[0], v[2])
            aux["n"] = v[2]
            if "n_marched" in aux:
                aux["n_marched"] = v[0]
        return False

    def repeat(self, tr, fn):
        """fn() again with host-side counts (the capacities learn from them), after a device-side count did not fit"""
        self.overflows += 1
        self.host_repeat = True
        tr.fronts.reset()
        try:
            return fn()
        finally:
            self.host_repeat = False
