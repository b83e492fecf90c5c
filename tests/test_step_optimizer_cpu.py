"""optimizer.StepOptimizer on the host: its checkpoint form (the legacy one included), the device block it syncs, and the step
numbers a capture and a replay move.  No GPU, no library: the state lives in CPU tensors, no launch is made."""
import pytest
import torch

from robust_e_nerf_amd import ops
from robust_e_nerf_amd.optimizer import StepOptimizer

KEYS = {"step_count", "exp_avg", "exp_avg_sq", "small_exp_avg", "small_exp_avg_sq", "ct_exp_avg", "ct_exp_avg_sq"}
BUFFERS = ("m", "v", "sm", "sv", "ct_m", "ct_v")


def _make():
    return StepOptimizer(torch.zeros(24), torch.zeros(4), torch.zeros(4))


def _filled(tau_steps=5):
    o = _make()
    gen = torch.Generator().manual_seed(7)
    for name in BUFFERS:
        getattr(o, name).copy_(torch.randn(getattr(o, name).shape, generator=gen))
    o.step_count, o.tau_adam_steps = 11, tau_steps
    o.tau_adam.copy_(torch.tensor([0.1 + 2.0 ** -40, 3.0e-9], dtype=torch.float64))      # (not representable in float32)
    return o


def test_a_new_optimiser_is_at_step_zero_with_zero_moments():
    o = _make()
    assert o.step_count == 0 and o.tau_adam_steps == 0 and o.lr_scale == 1.0
    assert [tuple(getattr(o, n).shape) for n in BUFFERS] == [(24,), (24,), (4,), (4,), (4,), (4,)]
    assert all(getattr(o, n).dtype == torch.float32 and not getattr(o, n).any() for n in BUFFERS)
    assert o.tau_adam.dtype == o.hyper.dtype == torch.float64 and o.tau_adam.shape == (2,) and o.hyper.shape == (8,)
    assert not o.tau_adam.any() and not o.hyper.any()


def test_state_dict_round_trip_is_bit_exact():
    a, b = _filled(), _make()
    sd = a.state_dict()
    assert set(sd) == KEYS | {"tau_adam"} and set(sd["tau_adam"]) == {"step", "exp_avg", "exp_avg_sq"}
    assert all(sd[k].dtype == torch.float32 and sd[k].device.type == "cpu" for k in KEYS - {"step_count"})
    assert sd["exp_avg"].data_ptr() != a.m.data_ptr()                            # copies, not views
    b.load_state_dict(sd)
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in BUFFERS)
    assert (b.step_count, b.tau_adam_steps) == (11, 5) and torch.equal(a.tau_adam, b.tau_adam)


def test_tau_adam_is_absent_while_its_step_is_zero():
    sd = _filled(tau_steps=0).state_dict()
    assert set(sd) == KEYS
    b = _filled(tau_steps=3)
    pair = b.tau_adam.clone()
    b.load_state_dict(sd)                                                        # no "tau_adam": the tau group stays as it is
    assert b.tau_adam_steps == 3 and torch.equal(b.tau_adam, pair) and b.step_count == 11


def test_legacy_tau_adam_in_torch_optim_form():
    sd = _filled(tau_steps=0).state_dict()
    legacy = dict(state={0: dict(step=torch.tensor(7.0), exp_avg=torch.tensor(0.125, dtype=torch.float64),
                                 exp_avg_sq=torch.tensor(2.5e-7, dtype=torch.float64))}, param_groups=[dict(lr=1.0)])
    o = _make()
    o.load_state_dict(dict(sd, tau_adam=legacy))
    assert o.tau_adam_steps == 7 and o.tau_adam.tolist() == [0.125, 2.5e-7]
    assert o.hyper[ops.HY_TAU_STEP] == 7
    o.load_state_dict(dict(sd, tau_adam=dict(state={}, param_groups=[])))        # saved before the first tau step
    assert o.tau_adam_steps == 7 and o.tau_adam.tolist() == [0.125, 2.5e-7]


def test_sync_hyper_writes_the_step_numbers_and_clears_everything_else():
    o = _make()
    o.hyper.fill_(3.0)
    o.load_state_dict(_filled().state_dict())
    hy = o.hyper.tolist()
    assert hy[ops.HY_STEP] == 11 and hy[ops.HY_TAU_STEP] == 5 and hy[ops.HY_SKIP] == 0.0
    assert all(x == 0.0 for i, x in enumerate(hy) if i not in (ops.HY_STEP, ops.HY_TAU_STEP))
    o.raise_skip()
    assert o.hyper[ops.HY_SKIP] == 1.0 and o.hyper[ops.HY_STEP] == 11
    o.sync_hyper()
    assert o.hyper.tolist() == hy


def test_capture_bookkeeping():
    o = _filled()
    s = o.host_state()
    o.advance_host(True)
    assert (o.step_count, o.tau_adam_steps) == (12, 6)
    o.restore_host_state(s)                                                      # a capture: enqueued, did not run
    assert (o.step_count, o.tau_adam_steps) == (11, 5)
    o.advance_host(False)                                                        # a replay with tau frozen
    assert (o.step_count, o.tau_adam_steps) == (12, 5)
    assert not o.hyper.any()                                                     # (the device's own numbers: the tick's business)


@pytest.mark.parametrize("epoch,k", [(0, 0), (19, 0), (20, 1), (30, 2), (36, 3), (99, 3)])
def test_set_epoch_with_the_default_milestones(epoch, k):
    o = _make()
    o.set_epoch(epoch)
    assert o.lr_scale == 0.33 ** k
    o.set_epoch(epoch, milestones=(1000,), gamma=0.5)
    assert o.lr_scale == 1.0
