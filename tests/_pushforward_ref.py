"""Reference for the flow-map sensitivities (``flow_jvp`` / ``flow_jacobian``; csrc/ff_mlp_ode.hpp PUSH): the oracle's own
fixed-grid solver, network and SDE classes (oracle/flowfusion_oracle.py: ``odeint_fixed``, ``mlp_forward`` behind
``ScoreOracle.ode_drift``, ``FlowOracle.dynamics``, ``VP`` / ``VE`` / ``SubVP``) differentiated by ``torch.func.jvp`` /
``jacfwd`` in any dtype.  Differentiating THROUGH the discrete steps is what the kernel's tangent columns do, so the two
agree to rounding, not to the order of the method.

``SolverMap`` is the map  (x [B, D], cond [B, C] or None) -> x_out [B, D]  of one solve, as a pure function:

* score models: ``to_data`` = ``sample_ode_from_base`` (x * sigma_max for VE, t: 1 -> epsilon), ``to_base`` =
  ``solve_odes_forward``'s state (t: epsilon -> 1); ``cond`` is what the network sees;
* flows: ``to_data`` = ``sample`` (t: 1 -> 0, then * target_scale + target_shift), ``to_base`` = the state of ``log_prob``
  ((x - target_shift) / target_scale, t: 0 -> 1); ``cond`` is the RAW conditional (``dynamics`` normalises it);
* ``affine=(shift, scale)`` / ``cond_affine=(cshift, cscale)``: the population wrappers' maps around a score model --
  ``to_data``: x_out * scale + shift, ``to_base``: (x - shift) / scale first; cond = (raw - cshift) / cscale.
"""
from __future__ import annotations

import torch

from oracle import flowfusion_oracle as fo

SDES = {"vp": fo.VP, "ve": fo.VE, "subvp": fo.SubVP}


class SolverMap:
    def __init__(self, kind, params, direction, method, options, dtype=torch.float64, sde="vp", no_sigma=False, affine=None,
                 cond_affine=None):
        assert kind in ("score", "flow") and direction in ("to_data", "to_base")
        self.kind, self.direction, self.method, self.options, self.dtype = kind, direction, method, options, dtype
        cast = lambda pair: None if pair is None else tuple(torch.as_tensor(v).to(dtype) for v in pair)
        self.affine, self.cond_affine = cast(affine), cast(cond_affine)
        if kind == "score":
            self.oracle = fo.ScoreOracle(params, SDES[sde](dtype=dtype), no_sigma=no_sigma, dtype=dtype)
            eps = self.oracle.sde.epsilon.to(torch.float32)
            one = torch.tensor(1.0, dtype=torch.float32)
            self.times = (torch.stack([one, eps]) if direction == "to_data" else torch.stack([eps, one])).to(dtype)
        else:
            self.oracle = fo.FlowOracle(params, dtype=dtype)
            self.times = torch.tensor([1.0, 0.0] if direction == "to_data" else [0.0, 1.0], dtype=torch.float32).to(dtype)

    def __call__(self, x, cond=None):
        o, to_data = self.oracle, self.direction == "to_data"
        if cond is not None and self.cond_affine is not None:
            cond = (cond - self.cond_affine[0]) / self.cond_affine[1]
        if self.kind == "score":
            if not to_data and self.affine is not None:
                x = (x - self.affine[0]) / self.affine[1]
            if to_data and o.sde.base_scale is not None:
                x = x * o.sde.base_scale
            (y,) = fo.odeint_fixed(lambda t, s: (o.ode_drift(t, s[0], cond),), (x,), self.times, self.method, self.options)
            return y * self.affine[1] + self.affine[0] if (to_data and self.affine is not None) else y
        if not to_data:
            x = (x - o.p.target_shift) / o.p.target_scale
        (y,) = fo.odeint_fixed(lambda t, s: (o.dynamics(t, s[0], cond),), (x,), self.times, self.method, self.options)
        return y * o.p.target_scale + o.p.target_shift if to_data else y

    def cast(self, t):
        return None if t is None else t.detach().to("cpu", self.dtype)

    def jvp(self, x, tangents=None, cond=None, cond_tangents=None):
        """(x_out [B, D], dx [B, K, D]): ``torch.func.jvp`` along every (tangents[:, k], cond_tangents[:, k])."""
        x, cond, tangents, cond_tangents = (self.cast(t) for t in (x, cond, tangents, cond_tangents))
        K = (tangents if tangents is not None else cond_tangents).shape[1]
        outs, y = [], None
        for k in range(K):
            vx = torch.zeros_like(x) if tangents is None else tangents[:, k]
            if cond is None:
                y, d = torch.func.jvp(lambda a: self(a), (x,), (vx,))
            else:
                vc = torch.zeros_like(cond) if cond_tangents is None else cond_tangents[:, k]
                y, d = torch.func.jvp(lambda a, c: self(a, c), (x, cond), (vx, vc))
            outs.append(d)
        return y, torch.stack(outs, dim=1)

    def jacobian(self, x, cond=None):
        """(x_out [B, D], J_x [B, D, D], J_c [B, D, C] or None): ``torch.func.jacfwd`` of the one-sample map, per row."""
        x, cond = self.cast(x), self.cast(cond)
        y = self(x, cond)
        if cond is None:
            Jx = torch.stack([torch.func.jacfwd(lambda a: self(a[None])[0])(x[b]) for b in range(x.shape[0])])
            return y, Jx, None
        J = [torch.func.jacfwd(lambda a, c: self(a[None], c[None])[0], argnums=(0, 1))(x[b], cond[b]) for b in range(x.shape[0])]
        return y, torch.stack([j[0] for j in J]), torch.stack([j[1] for j in J])

    def central_difference(self, x, tangents=None, cond=None, cond_tangents=None, h=1e-6):
        """dx [B, K, D] by central differences of step ``h`` along every direction (float64: error ~ h^2 + 1e-16 / h)."""
        x, cond, tangents, cond_tangents = (self.cast(t) for t in (x, cond, tangents, cond_tangents))
        K = (tangents if tangents is not None else cond_tangents).shape[1]
        outs = []
        for k in range(K):
            vx = 0 if tangents is None else tangents[:, k]
            vc = 0 if cond_tangents is None else cond_tangents[:, k]
            up = self(x + h * vx, None if cond is None else cond + h * vc)
            dn = self(x - h * vx, None if cond is None else cond - h * vc)
            outs.append((up - dn) / (2 * h))
        return torch.stack(outs, dim=1)


def score_params(model) -> fo.MLPParams:
    """The oracle's parameter bundle of a ``flowfusion_amd.diffusion.MLP``."""
    sd = {f"model.{k}": v.detach().to("cpu") for k, v in model.state_dict().items()}
    return fo.mlp_params_from_state_dict(sd)


def flow_params(flow) -> fo.FlowParams:
    return fo.flow_params_from_state_dict({k: v.detach().to("cpu") for k, v in flow.state_dict().items()})


def normalised_error(got, ref):
    """max over rows of  max |got - ref| / max |ref|  per sample (rows whose reference is all zero count absolutely)."""
    got, ref = got.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    B = ref.shape[0]
    num = (got - ref).abs().reshape(B, -1).amax(dim=1)
    den = ref.abs().reshape(B, -1).amax(dim=1)
    return float((num / torch.where(den > 0, den, torch.ones_like(den))).max())
