"""event_params.EventParams on the host: the constructor's values against the oracle, the host mirror's one read-back, the views
the kernels get, and what load() touches.  No GPU, no library: CPU tensors, ops.event_params_refresh replaced by a recorder."""
import pytest
import torch

from oracle import events as oracle_events
from robust_e_nerf_amd import ops
from robust_e_nerf_amd.event_params import EventParams

NEG_CT, TAU_MAX = 0.25, 1e5


def _make(p2n_raw=0.3, tau_raw=torch.tensor(1234.5, dtype=torch.float64)):
    return EventParams(torch.tensor(p2n_raw), torch.tensor(NEG_CT), tau_raw, torch.tensor(TAU_MAX), torch.device("cpu"))


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("tau_raw", [1234.5, -7e4, 50 * TAU_MAX], ids=["inside", "negative", "beyond-the-clamp"])
@pytest.mark.parametrize("p2n_raw", [-2.0, 0.3, 5.0])
def test_constructor_values_match_the_oracle(p2n_raw, tau_raw):
    ev = _make(p2n_raw, torch.tensor(tau_raw, dtype=torch.float64))
    c_p, c_n, mean_c = oracle_events.contrast_thresholds(torch.tensor(p2n_raw), torch.tensor(NEG_CT))
    tmax = torch.tensor(TAU_MAX, dtype=torch.float64)
    raw = oracle_events.clamp_tau_raw(torch.tensor(tau_raw, dtype=torch.float64), tmax)
    tau = oracle_events.refractory_period(raw, tmax)
    for got, ref in ((ev.c_p, c_p), (ev.c_n, c_n), (ev.mean_c, mean_c)):       # float32 through a handful of operations
        assert _rel(got, ref) <= 1e-6
    ep = ev.ep.tolist()
    assert ev.ep.dtype == torch.float64 and ep[ops.EP_CP] == ev.c_p and ep[ops.EP_CN] == ev.c_n and ep[ops.EP_TAU] == ev.tau
    assert _rel(ev.tau, tau) <= 1e-12 and _rel(ep[ops.EP_TAU_RAW], raw) <= 1e-12                # float64
    # 1 / C^k of the mean as the reference forms it, in float32 (the `mean_c` property averages the mirror's C_p and C_n in
    # float64 and may sit one float32 rounding, <= 6e-8, beside it)
    mc = float(mean_c)
    assert _rel(ep[ops.EP_INV_C], 1 / mc) <= 1e-12 and _rel(ep[ops.EP_INV_C2], 1 / mc ** 2) <= 1e-12
    assert _rel(ev.mean_c, mc) <= 6e-8
    assert ev.ct_raw == ep[ops.EP_RAW] == float(ev.ct[0]) == float(torch.tensor(p2n_raw))
    assert float(ev.tau_raw_dev[0]) == ep[ops.EP_TAU_RAW] and float(ev.tau_max) == TAU_MAX
    if tau_raw > TAU_MAX:                                                      # clamped: sigmoid'(raw / tau_max) = 1e-4
        lim = TAU_MAX * abs(float(torch.tensor(1e-4, dtype=torch.float64).logit()))
        assert _rel(ep[ops.EP_TAU_RAW], lim) <= 1e-12 and ep[ops.EP_TAU_RAW] < 10 * TAU_MAX


class _Counting:
    """stands in for `ep`: counts the read-backs"""
    def __init__(self, t):
        self.t, self.reads = t, 0

    def tolist(self):
        self.reads += 1
        return self.t.tolist()


def test_the_mirror_reads_back_once_and_only_when_stale():
    ev = _make()
    tau0 = ev.tau
    block = ev.ep = _Counting(ev.ep)
    assert ev.tau == tau0 and ev.c_p > 0 and ev.mean_c > 0 and block.reads == 0       # a fresh object answers from the mirror
    block.t[ops.EP_TAU] = 42.0
    assert ev.tau == tau0 and block.reads == 0                                   # written on the "device": not seen yet
    ev.mark_stale()
    assert ev.tau == 42.0 and block.reads == 1
    assert ev.tau == 42.0 and ev.ct_raw == ev.ct_raw and ev.mean_c > 0 and block.reads == 1


@pytest.mark.parametrize("shape", [(), (1,)])
def test_tau_raw_keeps_the_constructors_shape_in_float64(shape):
    ev = _make(tau_raw=torch.full(shape, 321.0, dtype=torch.float32))
    assert ev.tau_raw.shape == shape and ev.tau_raw.dtype == torch.float64 and float(ev.tau_raw.reshape(-1)[0]) == 321.0
    assert ev.tau_raw_dev.shape == (1,) and ev.tau_raw_dev.dtype == torch.float64


def test_pw_gives_views_of_the_device_block():
    ev = _make()
    assert ev.pw(None) is None
    for kind, slot in (("mean_contrast_reciprocal", ops.EP_INV_C), ("mean_contrast_reciprocal_sq", ops.EP_INV_C2)):
        w = ev.pw(kind)
        assert w.shape == (1,) and w.data_ptr() == ev.ep[slot:].data_ptr()
        ev.ep[slot] = 7.0 + slot
        assert float(w[0]) == 7.0 + slot
    with pytest.raises(KeyError):
        ev.pw("no_such_weight")


def test_load_writes_the_raw_forms_and_refreshes_once(monkeypatch):
    ev = _make()
    calls = []
    monkeypatch.setattr(ops, "event_params_refresh", lambda *a: calls.append(a))
    block = ev.ep = _Counting(ev.ep)
    ev.load(p2n_raw=torch.tensor([1.5], dtype=torch.float64), tau_raw=torch.tensor(-99.0))
    assert float(ev.ct[0]) == 1.5 and ev.ct.dtype == torch.float32 and ev.ct[1:].abs().sum() == 0
    assert float(ev.tau_raw_dev[0]) == -99.0 and ev.tau_raw_dev.dtype == torch.float64
    assert len(calls) == 1
    ct, c_n, raw, tmax, ep = calls[0]
    assert ct is ev.ct and c_n == ev.c_n and raw is ev.tau_raw_dev and tmax == TAU_MAX and ep is block
    assert block.reads == 0
    _ = ev.tau
    assert block.reads == 1                                                      # left stale: the next look reads back
    ev.load()                                                                    # nothing given: the refresh alone
    assert len(calls) == 2 and float(ev.ct[0]) == 1.5 and float(ev.tau_raw_dev[0]) == -99.0
