"""fronts.StepFronts on CPU tensors: when an early front may be used, and when it is void.  No GPU, no library: the key and the
match logic need neither a stream nor a kernel."""
from types import SimpleNamespace as NS

import pytest
import torch

from robust_e_nerf_amd.fronts import DiffFront, GradFront, StepFronts


def _inputs():
    batch = dict(position=torch.zeros(5, 2), start_ts=torch.arange(5), end_ts=torch.arange(5) + 3)
    return batch, torch.rand(5), torch.rand(5)


def _trainer(frozen=True):
    r = NS(binary=torch.zeros(8, dtype=torch.uint8), binary_epoch=0, cfg=NS(sampler="occgrid"))
    return NS(r=r, t=NS(train_contrast_threshold=not frozen, train_refractory_period=False))


def _held(tr, batch, j0, j1):
    """a StepFronts that holds a front made from (batch, j0, j1), as prefetch() leaves it (the event is a stand-in)"""
    sf, front = StepFronts(), DiffFront(prep={}, jitter=None)
    sf.prefetched = (sf.key(tr.r, batch, j0, j1), front, "event", (batch, j0, j1))
    return sf, front


def test_unchanged_inputs_take_the_front_once():
    tr, (batch, j0, j1) = _trainer(), _inputs()
    sf, front = _held(tr, batch, j0, j1)
    assert sf.match_diff(tr, batch, j0, j1) == (front, "event")
    assert sf.prefetched is None and sf.match_diff(tr, batch, j0, j1) is None        # consumed


def _write_batch(tr, batch, j0, j1):
    batch["end_ts"].add_(1)


def _write_jitter(tr, batch, j0, j1):
    j1.mul_(0.5)


def _write_grid(tr, batch, j0, j1):
    tr.r.binary.fill_(1)


def _refresh_grid(tr, batch, j0, j1):
    tr.r.binary_epoch += 1


@pytest.mark.parametrize("change", [_write_batch, _write_jitter, _write_grid, _refresh_grid])
def test_a_write_to_what_the_front_read_voids_it(change):
    tr, (batch, j0, j1) = _trainer(), _inputs()
    sf, _ = _held(tr, batch, j0, j1)
    ids = [id(v) for v in (batch, *batch.values(), j0, j1, tr.r.binary)]
    versions = [v._version for v in (*batch.values(), j0, j1, tr.r.binary)]
    change(tr, batch, j0, j1)
    assert ids == [id(v) for v in (batch, *batch.values(), j0, j1, tr.r.binary)]     # the same objects ...
    if change is not _refresh_grid:
        assert versions != [v._version for v in (*batch.values(), j0, j1, tr.r.binary)]   # ... written in place
    assert sf.match_diff(tr, batch, j0, j1) is None and sf.prefetched is None


def test_another_batch_with_equal_contents_is_refused():
    tr, (batch, j0, j1) = _trainer(), _inputs()
    sf, _ = _held(tr, batch, j0, j1)
    assert sf.match_diff(tr, dict(batch), j0, j1) is None                  # another dict of the same tensors
    sf, _ = _held(tr, batch, j0, j1)
    assert sf.match_diff(tr, {k: v.clone() for k, v in batch.items()}, j0, j1) is None
    sf, _ = _held(tr, batch, j0, j1)
    assert sf.match_diff(tr, batch, j0.clone(), j1) is None


def test_trainable_event_parameters_refuse_any_front():
    tr, (batch, j0, j1) = _trainer(), _inputs()
    sf, _ = _held(tr, batch, j0, j1)
    assert sf.match_diff(_trainer(frozen=False), batch, j0, j1) is None    # (they move the timestamps the front was made from)


def _begun(batch, jitter_grad):
    sf = StepFronts()
    sf.begun = GradFront(*[None] * 8, key=(id(batch), id(jitter_grad)))
    sf.ready_ev = "ready"
    return sf


def test_third_render_front_is_for_one_batch_and_jitter_pair():
    (batch, j2, other) = _inputs()
    sf = _begun(batch, j2)
    fr = sf.begun
    assert sf.match_grad(batch, j2, True) == (fr, "ready")
    assert sf.begun is None and sf.ready_ev is None and sf.match_grad(batch, j2, True) == (None, None)     # consumed
    for b, j in ((batch, other), (dict(batch), j2), (batch, j2.clone())):
        sf = _begun(batch, j2)
        assert sf.match_grad(b, j, True) == (None, "ready")                # dropped, not used ...
        assert sf.pending is None and sf.begun is None and sf.ready_ev is None         # ... and not kept either
    assert _begun(batch, j2).match_grad(batch, j2, False)[0] is None       # an in-order call takes no front


def test_reset_leaves_nothing_announced_begun_or_ready():
    batch, j2, _ = _inputs()
    sf = _begun(batch, j2)
    sf.pending = (batch, j2, None)
    sf.reset()
    assert sf.pending is None and sf.begun is None and sf.ready_ev is None
    assert sf.match_grad(batch, j2, True) == (None, None)
