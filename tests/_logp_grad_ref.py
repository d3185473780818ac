"""Reference for the log-density gradients (``log_prob_grad``; csrc/ff_mlp_lgrad.hpp): the fixed-grid Hutchinson log-density
as an ordinary differentiable torch function in any dtype, and its gradient from ``torch.autograd.grad``.

The value is the forward row program of ``solvers.plan_ode`` (as ``_pullback_discrete_ref.stage_states`` runs it) on the oracle's
own right-hand side behind ``_pushforward_ref.SolverMap``'s maps (``direction="to_base"``), with the divergence of every row from
``torch.func.jvp``:

    y_e = x + sum_s cin_e[s] k[s];   k[slot_e] = f(t_e, y_e, c);   kl[slot_e] = sum_k w eps_k^T (df/dy)(t_e, y_e, c) eps_k
    FLAG_STEP_END:  x += sum_s cout_e[s] k[s];   lp += sum_s cout_e[s] kl[s]
    log p = div_weight * lp + cot_weight * log prior(x_T) [- sum log target_scale]

Reverse mode over that forward-mode tangent is what the kernel computes, so the two agree to rounding at any step count.
float64 is the truth; float32 gives a case's floor.  ``div_weight=0`` leaves the state path alone (``flow_vjp(adjoint=
"discrete")`` of the prior's gradient); since eps^T J_net eps depends on y only through the slopes SiLU'(z_l), it is also the
gradient with the SiLU'' cross term dropped.  ``cot_weight=0`` leaves the second-order path alone.
"""
from __future__ import annotations

import math

import torch

from flowfusion_amd import solvers

from tests._pullback_ref import Pullback
from tests._pushforward_ref import SolverMap


class LogDensity:
    def __init__(self, smap: SolverMap):
        assert smap.direction == "to_base"
        self.m = smap

    def prior_scale(self):
        m = self.m
        return float(m.oracle.sde.prior_scale()) if m.kind == "score" else 1.0

    def value(self, x, cond, probes, weight, div_weight=1.0, cot_weight=1.0):
        """log p [B] (see the module's docstring) of tensors already in the reference's dtype; differentiable in x and cond."""
        m = self.m
        cont = Pullback(m)
        pre_shift, pre_scale, _, _, _ = cont._maps()
        xs = x if pre_shift is None else (x - pre_shift) / pre_scale
        tab = solvers.plan_ode(m.times.to(torch.float32), m.method, m.options)
        S = solvers.MAX_SLOTS
        k = [torch.zeros_like(xs) for _ in range(S)]
        kl = [xs.new_zeros(xs.shape[0]) for _ in range(S)]
        lp = xs.new_zeros(xs.shape[0])
        for e in range(int(tab.t_eval.numel())):
            y = xs + sum(tab.cin[e, s].to(m.dtype) * k[s] for s in range(S))
            t = tab.t_eval[e].to(m.dtype)
            f = lambda yy: tab.sign * cont.drift(t, yy, cond)
            div = xs.new_zeros(xs.shape[0])
            val = None
            for j in range(probes.shape[1]):
                val, jv = torch.func.jvp(f, (y,), (probes[:, j],))
                div = div + weight * (probes[:, j] * jv).sum(dim=1)
            k[int(tab.slot[e])] = val
            kl[int(tab.slot[e])] = div
            if int(tab.flags[e]) & solvers.FLAG_STEP_END:
                xs = xs + sum(tab.cout[e, s].to(m.dtype) * k[s] for s in range(S))
                lp = lp + sum(tab.cout[e, s].to(m.dtype) * kl[s] for s in range(S))
        sc = self.prior_scale()
        prior = (-0.5 * (xs / sc) ** 2 - math.log(sc) - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
        out = div_weight * lp + cot_weight * prior
        if m.kind == "flow":
            out = out - cot_weight * torch.log(m.oracle.p.target_scale).sum()
        return out

    def __call__(self, x, cond, probes, weight, div_weight=1.0, cot_weight=1.0):
        """(log_p [B], grad_x [B, D], grad_c [B, C] or None): the value and its gradient with respect to ``x`` and the raw
        ``cond`` at fixed ``probes`` [B, K, D], each probe's divergence integral weighted by ``weight``."""
        m = self.m
        x, cond, probes = m.cast(x), m.cast(cond), m.cast(probes)
        x = x.clone().requires_grad_(True)
        if cond is not None:
            cond = cond.clone().requires_grad_(True)
        with torch.enable_grad():
            lp = self.value(x, cond, probes, weight, div_weight, cot_weight)
            wrt = (x,) if cond is None else (x, cond)
            g = torch.autograd.grad(lp.sum(), wrt, allow_unused=True)
        gx = torch.zeros_like(x) if g[0] is None else g[0]
        gc = None if cond is None else (torch.zeros_like(cond) if g[1] is None else g[1])
        return lp.detach(), gx.detach(), (None if gc is None else gc.detach())

    def central_difference(self, x, cond, probes, weight, h=1e-6, **kw):
        """(grad_x, grad_c or None) of the value by central differences of step ``h`` in every coordinate (float64)."""
        m = self.m
        x, cond, probes = m.cast(x), m.cast(cond), m.cast(probes)
        with torch.no_grad():
            gx = torch.zeros_like(x)
            for d in range(x.shape[1]):
                dx = torch.zeros_like(x)
                dx[:, d] = h
                gx[:, d] = (self.value(x + dx, cond, probes, weight, **kw) - self.value(x - dx, cond, probes, weight, **kw)) / (2 * h)
            if cond is None:
                return gx, None
            gc = torch.zeros_like(cond)
            for d in range(cond.shape[1]):
                dc = torch.zeros_like(cond)
                dc[:, d] = h
                gc[:, d] = (self.value(x, cond + dc, probes, weight, **kw) - self.value(x, cond - dc, probes, weight, **kw)) / (2 * h)
        return gx, gc
