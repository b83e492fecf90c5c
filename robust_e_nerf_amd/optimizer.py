"""The optimiser's own state and its launches (Adam with L2 decay, 4 groups, MultiStepLR: robust_e_nerf.py:782-832): the moment
buffers, the step numbers on the host and on the device (`hyper`, ops.HY_*), the learning-rate factor.  ONE rule lives here:
after the device has advanced the optimiser -- apply(), or a replayed graph of it -- the host step numbers advance too."""
from __future__ import annotations

import torch

from . import ops


class StepOptimizer:
    def __init__(self, flat, small, ct):                     # (the three parameter blocks: for their shapes and device only)
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.sm, self.sv = torch.zeros_like(small), torch.zeros_like(small)
        self.ct_m, self.ct_v = torch.zeros_like(ct), torch.zeros_like(ct)
        # the refractory period's Adam group (float64 scalar; state: exp_avg, exp_avg_sq) lives on the device as well
        self.tau_adam, self.tau_adam_steps = torch.zeros(2, dtype=torch.float64, device=flat.device), 0
        # optimiser state on the device (ABI 25, ops.HY_*): Adam step numbers and bias corrections, and the sticky skip word a
        # captured step raises when one of its device-side counts did not fit (step_graph.StepGraphs)
        self.hyper = torch.zeros(8, dtype=torch.float64, device=flat.device)
        self.step_count = 0
        self.lr_scale = 1.0

    def set_epoch(self, epoch: int, milestones=(20, 30, 36), gamma: float = 0.33):
        """MultiStepLR stepped per epoch (robust_e_nerf.py:818-832, synthetic.yaml:113-128)."""
        self.lr_scale = gamma ** sum(1 for m in milestones if epoch >= m)

    # ---- host step numbers beside the device's ----
    def host_state(self):
        return self.step_count, self.tau_adam_steps

    def restore_host_state(self, s):                         # (a capture enqueues apply() without running it)
        self.step_count, self.tau_adam_steps = s

    def advance_host(self, tick_tau: bool):
        """the device ticked its step numbers (ops.step_tick with this tick_tau, eagerly or in a replayed graph)"""
        self.step_count += 1
        self.tau_adam_steps += int(tick_tau)

    def sync_hyper(self):
        """device-side step numbers <- the host's (after loading a checkpoint, or a repeated step); clears the skip word"""
        h = [0.0] * 8
        h[ops.HY_STEP], h[ops.HY_TAU_STEP] = float(self.step_count), float(self.tau_adam_steps)
        self.hyper.copy_(torch.tensor(h, dtype=torch.float64))

    def raise_skip(self):
        """the sticky skip word: every optimiser launch leaves parameters, moments and gradients alone until sync_hyper()"""
        self.hyper[ops.HY_SKIP: ops.HY_SKIP + 1].fill_(1.0)

    def apply(self, views, t, events, grad_scale: float, stats):
        """one optimiser step.  views: the Trainer's (field, small, small_grad, ct_grad, d loss / d tau); t: its TrainCfg;
        stats: the overflow words of a captured step's renders"""
        f, small, small_grad, ct_grad, tau_grad = views
        gs, hy, lr = grad_scale, self.hyper, t.lr * self.lr_scale
        # step numbers / bias corrections live on the device (ops.HY_*): the same launches serve the eager step and a captured
        # one, whose renders' overflow words raise the skip word instead (step_graph.StepGraphs)
        self.advance_host(t.train_refractory_period)
        ops.step_tick(hy, t.betas, stats=stats, tick_tau=t.train_refractory_period)
        ops.adam_step_dev(f.flat, f.grad, self.m, self.v, hy, lr=lr, betas=t.betas, eps=t.eps,
                          weight_decay=t.weight_decay, grad_scale=gs, zero_grad=True)
        if getattr(f, "n_wn_g", 0):
            f.refresh()
        ops.adam_step_dev(small, small_grad, self.sm, self.sv, hy, lr=lr, betas=t.betas, eps=t.eps,
                          weight_decay=0.0, grad_scale=gs, zero_grad=True)
        if t.train_refractory_period:
            # float64 scalar, Adam group with lr = tau_max * relative lr (robust_e_nerf.py:804-807);
            # tau = tau_max sigmoid(raw / tau_max)  =>  d tau / d raw = sigmoid'(raw / tau_max): one single-thread launch
            ops.tau_adam_step_dev(events.tau_raw_dev, tau_grad, self.tau_adam, float(events.tau_max), hy,
                                  lr=float(events.tau_max) * t.relative_lr_refractory_period * self.lr_scale,
                                  betas=t.betas, eps=t.eps, grad_scale=gs)
        if t.train_contrast_threshold:
            ops.adam_step_dev(events.ct, ct_grad, self.ct_m, self.ct_v, hy, lr=t.lr_contrast_threshold * self.lr_scale,
                              betas=t.betas, eps=t.eps, weight_decay=0.0, grad_scale=gs, zero_grad=True)
        if t.train_refractory_period or t.train_contrast_threshold:
            events.refresh()

    # ---- optimiser state for checkpoints (what ModelCheckpoint keeps under "optimizer_states": scripts/run.py:66-68) ----
    def state_dict(self):
        cpu = lambda t: t.detach().cpu().clone()
        sd = dict(step_count=self.step_count, exp_avg=cpu(self.m), exp_avg_sq=cpu(self.v), small_exp_avg=cpu(self.sm),
                  small_exp_avg_sq=cpu(self.sv), ct_exp_avg=cpu(self.ct_m), ct_exp_avg_sq=cpu(self.ct_v))
        if self.tau_adam_steps:
            m, v = self.tau_adam.tolist()
            sd["tau_adam"] = dict(step=self.tau_adam_steps, exp_avg=m, exp_avg_sq=v)
        return sd

    def load_state_dict(self, sd):
        self.step_count = int(sd["step_count"])
        for dst, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq"), (self.sm, "small_exp_avg"),
                         (self.sv, "small_exp_avg_sq"), (self.ct_m, "ct_exp_avg"), (self.ct_v, "ct_exp_avg_sq")):
            dst.copy_(sd[key].to(dst.device, dst.dtype))
        if "tau_adam" in sd:
            ta = sd["tau_adam"]
            if "state" in ta:                                # round <= 4 checkpoints: a torch.optim.Adam state dict
                st = next(iter(ta["state"].values()), None)
                ta = dict(step=int(st["step"]), exp_avg=float(st["exp_avg"]), exp_avg_sq=float(st["exp_avg_sq"])) if st else None
            if ta:
                self.tau_adam_steps = int(ta["step"])
                self.tau_adam.copy_(torch.tensor([ta["exp_avg"], ta["exp_avg_sq"]], dtype=torch.float64))
        self.sync_hyper()
