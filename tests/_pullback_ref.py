"""Reference for the flow-map pull-backs (``flow_vjp``; csrc/ff_mlp_pull.hpp): the SAME algorithm in any dtype -- the
continuous adjoint of ``odeint_adjoint`` for the inputs of a solve, integrated by the oracle's own fixed-grid solver
(oracle/flowfusion_oracle.py ``odeint_fixed``) over the reversed span with the method and step of the forward solve:

    state [y | alpha | gamma] from [y_T, w, 0]:   dy/dt = f(t, y, c)    dalpha/dt = -(df/dy)^T alpha    dgamma/dt = -(df/dc)^T alpha

with ``f`` = ``ScoreOracle.ode_drift`` / ``FlowOracle.dynamics`` and the products from ``torch.func.vjp``.  It discretises
exactly as the kernel does, so the two agree to rounding; against ``w^T SolverMap.jacobian`` (the derivative of the discrete
map) it differs by the discretisation error of the method.  The maps around the solve are ``_pushforward_ref.SolverMap``'s:
``Pullback(smap)`` pulls back through the map ``smap`` computes, in the units of its ``x``, ``x_out`` and (raw) ``cond``.
"""
from __future__ import annotations

import torch

from oracle import flowfusion_oracle as fo

from tests._pushforward_ref import SolverMap


class Pullback:
    def __init__(self, smap: SolverMap):
        self.m = smap

    def _maps(self):
        """(pre_shift, pre_scale, gain, post_scale, post_shift) of ``SolverMap.__call__``: y0 = (x - pre_shift) / pre_scale *
        gain, x_out = y_T * post_scale + post_shift (None = identity)."""
        m, to_data = self.m, self.m.direction == "to_data"
        if m.kind == "score":
            pre = m.affine if (not to_data and m.affine is not None) else (None, None)
            gain = m.oracle.sde.base_scale if to_data else None
            post = m.affine if (to_data and m.affine is not None) else (None, None)
            return pre[0], pre[1], gain, post[1], post[0]
        p = m.oracle.p
        return (None, None, None, p.target_scale, p.target_shift) if to_data else (p.target_shift, p.target_scale, None, None, None)

    def drift(self, t, y, cond):
        """f(t, y, cond) in the solve's own state, ``cond`` raw (its normalisation is part of what is differentiated)."""
        m = self.m
        if m.kind == "score":
            if cond is not None and m.cond_affine is not None:
                cond = (cond - m.cond_affine[0]) / m.cond_affine[1]
            return m.oracle.ode_drift(t, y, cond)
        return m.oracle.dynamics(t, y, cond)

    def __call__(self, x, cotangents, cond=None):
        """(x_out [B, D], gx [B, K, D], gc [B, K, C] or None, retrace [B])."""
        m = self.m
        x, cond, w = m.cast(x), m.cast(cond), m.cast(cotangents)
        pre_shift, pre_scale, gain, post_scale, post_shift = self._maps()
        y0 = x if pre_shift is None else (x - pre_shift) / pre_scale
        y0 = y0 if gain is None else y0 * gain
        (yT,) = fo.odeint_fixed(lambda t, s: (self.drift(t, s[0], cond),), (y0,), m.times, m.method, m.options)
        x_out = yT if post_scale is None else yT * post_scale + post_shift

        def aug(t, s):
            y, a, g = s
            if cond is None:
                f, pull = torch.func.vjp(lambda yy: self.drift(t, yy, None), y)
                (ay,) = pull(a)
                return f, -ay, torch.zeros_like(g)
            f, pull = torch.func.vjp(lambda yy, cc: self.drift(t, yy, cc), y, cond)
            ay, ac = pull(a)
            return f, -ay, -ac

        back = torch.flip(m.times, dims=(0,))
        gxs, gcs, y_back = [], [], None
        for k in range(w.shape[1]):
            a0 = w[:, k] if post_scale is None else w[:, k] * post_scale
            g0 = torch.zeros_like(x[:, :0]) if cond is None else torch.zeros_like(cond)
            y_back, a, g = fo.odeint_fixed(aug, (yT, a0, g0), back, m.method, m.options)
            a = a if gain is None else a * gain
            gxs.append(a if pre_scale is None else a / pre_scale)
            gcs.append(g)
        xb = y_back if gain is None else y_back / gain
        xb = xb if pre_shift is None else xb * pre_scale + pre_shift
        self.retraced = xb                  # the retraced start, in the units of x
        retrace = (xb - x).abs().amax(dim=1)
        return x_out, torch.stack(gxs, dim=1), (None if cond is None else torch.stack(gcs, dim=1)), retrace
