"""The event-generation parameters C_p, C_n and tau (event_generation_params.py:51-84,162-203) as ONE owner: the device block
every kernel reads them from (`ep`, ops.EP_*), its host mirror, and the raw trainable forms the optimiser steps."""
import torch

from . import ops


class EventParams:
    def __init__(self, p2n_raw, neg_ct, tau_raw, tau_max, device):
        # evaluated here on the host as the reference does in float32 / float64, then DEVICE-RESIDENT (self.ep): every kernel
        # takes C_p, C_n, tau and the 1 / C^k param weight from that block, and a trainable ratio / refractory period is stepped
        # and re-evaluated on the device (ren_tau_adam_step, ren_event_params_refresh), so no launch of the next step waits for
        # a host read of a parameter.  The host-side attributes (c_p, mean_c, tau, ct_raw, tau_raw) are read back on demand.
        ratio = torch.nn.functional.softplus(p2n_raw.detach().cpu().to(torch.float32))   # event_generation_params.py:51-70
        neg = neg_ct.detach().cpu().to(torch.float32)
        c_p, self.c_n = float(ratio * neg), float(neg)
        mean_c = float((ratio * neg + neg) / 2)
        traw, tmax = tau_raw.detach().cpu().to(torch.float64), tau_max.detach().cpu()
        lim = torch.tensor(1e-4, dtype=torch.float64).logit().abs()
        traw = tmax * (traw / tmax).clamp(-lim, lim)                          # :170-185
        tau = float(tmax * torch.sigmoid(traw / tmax))                        # modules.py:58-74 (float64)
        self.tau_max = tmax.to(torch.float64)
        self._tau_shape = tuple(traw.shape)
        ct_raw = float(p2n_raw.detach().reshape(-1)[0].to(torch.float32))
        self._ep_host = [c_p, self.c_n, ct_raw, tau, 1.0 / mean_c, 1.0 / mean_c ** 2, float(traw.reshape(-1)[0]), 0.0]
        self._ep_stale = False
        self.ep = torch.tensor(self._ep_host, dtype=torch.float64, device=device)
        # trainable refractory period: a float64 scalar (event_generation_params.py:162-164)
        self.tau_raw_dev = traw.reshape(1).clone().to(device)
        # trainable C_p / C_n ratio (softplus-parametrised scalar, its own Adam group with lr 0.1:
        # robust_e_nerf.py:800-803).  Its loss dependence is through the per-event targets and the 1/C^k
        # normalisation only, i.e. O(B) elementwise work on already rendered predictions.
        self.ct = torch.zeros(4, device=device, dtype=torch.float32)
        self.ct[0] = p2n_raw.detach().reshape(-1)[0].to(device, torch.float32)

    # ---- host views of the device block (a read-back when it has moved since the last look) ----
    def _host(self):
        if self._ep_stale:
            self._ep_host, self._ep_stale = self.ep.tolist(), False
        return self._ep_host

    c_p = property(lambda self: self._host()[ops.EP_CP])
    mean_c = property(lambda self: (self._host()[ops.EP_CP] + self._host()[ops.EP_CN]) / 2)
    tau = property(lambda self: self._host()[ops.EP_TAU])
    ct_raw = property(lambda self: self._host()[ops.EP_RAW])

    @property
    def tau_raw(self) -> torch.Tensor:
        """the raw refractory period (float64, host copy, shaped like the constructor's tau_raw)"""
        return self.tau_raw_dev.cpu().reshape(self._tau_shape)

    def mark_stale(self):
        """the device has re-evaluated `ep` (refresh(), or a replayed graph that contains one)"""
        self._ep_stale = True

    def refresh(self):
        """clamp (:170-185), C_p, tau, 1 / C^k from the raw forms, for the next step's kernels"""
        ops.event_params_refresh(self.ct, self.c_n, self.tau_raw_dev, float(self.tau_max), self.ep)
        self.mark_stale()

    def pw(self, kind):
        """device scalar of the param weight 1 / C^k (loss.param_weight.*, robust_e_nerf.py:470-486), None for k = 0"""
        return {None: None, "mean_contrast_reciprocal": self.ep[ops.EP_INV_C: ops.EP_INV_C + 1],
                "mean_contrast_reciprocal_sq": self.ep[ops.EP_INV_C2: ops.EP_INV_C2 + 1]}[kind]

    def load(self, p2n_raw=None, tau_raw=None):
        """restore the learned contrast-threshold ratio / refractory period (checkpoint resume)"""
        if p2n_raw is not None:
            self.ct[0] = p2n_raw.detach().reshape(-1)[0].to(self.ct.device, torch.float32)
        if tau_raw is not None:
            self.tau_raw_dev.copy_(tau_raw.detach().to(torch.float64).reshape(1))
        self.refresh()
