"""Shared host plumbing between the score-model and flow front ends.

``FusedNet`` owns what the kernel needs from a Linear/activation stack: the kernel plan, the
weights repacked into MFMA operand order (cached on the device, refreshed when a parameter
changes) and the launch itself.  The front ends (diffusion.py, flow.py) supply the
time-dependent part: one evaluation table per solve (solvers.py).
"""
from __future__ import annotations

import warnings
from typing import Callable, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _native
from ._native import MODE_EXACT, MODE_HUTCH, MODE_STATE, f32_on  # noqa: F401  (modes re-exported)
from .solvers import ROW_A, ROW_AUX_COEF, ROW_B, ROW_CIN, ROW_HDR, ROW_SLOT, ROW_USE_Y


def activation_spec(act) -> Tuple[int, float, float]:
    """(FF_ACT_* code, parameter 0, parameter 1) of a torch.nn activation module or class -- the
    `activation` argument of the reference constructors (an instance for MLP, diffusion.py:38; a class
    for the flows, flow.py:41,70)."""
    if isinstance(act, type):
        act = act()
    N = _native
    if type(act) is nn.SiLU:
        return (N.ACT_SILU, 0.0, 0.0)
    if type(act) is nn.Tanh:
        return (N.ACT_TANH, 0.0, 0.0)
    if type(act) is nn.Sigmoid:
        return (N.ACT_SIGMOID, 0.0, 0.0)
    if type(act) is nn.ReLU:
        return (N.ACT_RELU, 0.0, 0.0)
    if type(act) is nn.LeakyReLU:
        return (N.ACT_LEAKY_RELU, float(act.negative_slope), 0.0)
    if type(act) is nn.ELU:
        return (N.ACT_ELU, float(act.alpha), 0.0)
    if type(act) is nn.Softplus:
        return (N.ACT_SOFTPLUS, float(act.beta), float(act.threshold))
    if type(act) is nn.GELU:
        return (N.ACT_GELU_TANH if act.approximate == "tanh" else N.ACT_GELU, 0.0, 0.0)
    raise NotImplementedError(
        f"activation {act!r}: the fused gfx950 kernels implement SiLU (the reference default), Tanh, Sigmoid, "
        "ReLU, LeakyReLU, ELU, Softplus and GELU")


class FusedEnvelopeWarning(UserWarning):
    """A network no compiled kernel can hold is evaluated by torch on the GPU (stepping stays native)."""


def within_envelope(owner, key, build: Callable[[], "FusedNet"], modes=(MODE_STATE, MODE_EXACT)) -> bool:
    """True if a compiled kernel holds the network ``build()`` describes (plans exist in every mode of ``modes``: the
    state-only and the divergence-capable kernels, or the state only for the two-network kernels of the symplectic flows).
    The reference puts no limit on width, dimension, conditional inputs or activation (flowfusion/diffusion.py:59-72,
    flow.py:61-74); outside the compiled shapes the front ends keep the
    solve on the GPU by handing the network to ``generic.py`` -- the module evaluated by torch, every Runge-Kutta
    combination, error norm and noise update by the library's kernels -- and say so once per network
    (``FusedEnvelopeWarning``).  The answer is cached on ``owner`` under ``key`` (identity of the layers)."""
    cached = owner.__dict__.get("_envelope")
    if cached is not None and cached[0] == key:
        return cached[1]
    try:
        net = build()
        for mode in modes:
            net.plan(mode)
        ok = True
    except NotImplementedError as e:
        warnings.warn(f"{e} -- outside the fused kernels' envelope: this network is evaluated by torch on the GPU, "
                      "time stepping stays in the library's kernels (flowfusion_amd.generic)",
                      FusedEnvelopeWarning, stacklevel=4)
        ok = False
    object.__setattr__(owner, "_envelope", (key, ok))
    return ok


def exact_trace_passes(dim: int, tile: int) -> List[Tuple[int, int]]:
    """Split the `dim` unit tangents of an exact trace into launches [(first, count), ...].

    A wavefront carries `tile` MFMA columns; a launch with n tangents per sample packs
    floor(tile / (1 + n)) samples into them, so it costs tile / floor(tile / (1 + n)) columns per
    sample (the value column is recomputed by every launch).  The cheapest partition is not always
    the fewest launches: 8 dimensions on 16 columns cost 16 in one launch (9 columns, one sample per
    wavefront) but 8 + 2 as 7 + 1.  Small dynamic programme over the partitions of `dim`."""
    cost = [0.0] + [tile / (tile // (1 + n)) for n in range(1, tile)]
    best = [(0.0, [])] + [None] * dim
    for d in range(1, dim + 1):
        cands = []
        for n in range(1, min(d, tile - 1) + 1):
            c, parts = best[d - n]
            cands.append((c + cost[n] + 1e-9 * (len(parts) + 1), parts + [n]))   # ties: fewer launches
        best[d] = min(cands, key=lambda cp: cp[0])
    out, first = [], 0
    for n in sorted(best[dim][1], reverse=True):
        out.append((first, n))
        first += n
    return out


class FusedNet:
    """Kernel-side view of ``Linear -> SiLU -> ... -> Linear`` with first-layer input
    ``[ time part | x | cond ]`` in any column order."""

    def __init__(self, linears: Sequence[nn.Linear], dim: int, cond_dim: int, x_col0: int, c_col0: int,
                 act: Tuple[int, float, float] = (_native.ACT_SILU, 0.0, 0.0), precision: str = "f32"):
        self.linears = list(linears)
        self.act = (int(act[0]), float(act[1]), float(act[2]))
        if precision not in _native.PRECISIONS:
            raise ValueError(f"precision={precision!r}: expected one of {sorted(_native.PRECISIONS)}")
        self.precision = precision
        if len(self.linears) < 2:
            raise NotImplementedError("the fused path needs at least one hidden layer")
        self.dim = int(dim)
        self.cond_dim = int(cond_dim)
        self.x_col0 = int(x_col0)
        self.c_col0 = int(c_col0)
        self.hidden = [int(l.out_features) for l in self.linears[:-1]]
        if int(self.linears[-1].out_features) != self.dim:
            raise ValueError("last layer must produce `dim` outputs")
        for l in self.linears:
            if l.bias is None:
                raise NotImplementedError("Linear layers without bias are not supported")
        self._plans = {}
        self._wpack = {}            # layout key -> (parameter versions, packed device tensor)
        self._tables = {}           # small cache of evaluation tables already on the device

    def serves(self, linears, act, precision: str = "f32") -> bool:
        """True if this view was built from exactly these Linear modules (identity, in order) and this
        activation.  The front ends rebuild the view otherwise: a layer replaced after the first solve
        (``model.NN[2] = nn.Linear(..)``) must not keep integrating with the old weights."""
        act = (int(act[0]), float(act[1]), float(act[2]))
        return (self.act == act and self.precision == precision and len(linears) == len(self.linears)
                and all(a is b for a, b in zip(linears, self.linears)))

    # -- plan / weights ---------------------------------------------------------------------
    def plan(self, mode: int) -> _native.PlanStruct:
        key = 0 if mode == MODE_STATE else (1 if mode == MODE_HUTCH else 2)
        if key not in self._plans:
            self._plans[key] = _native.make_plan(self.dim, self.cond_dim, self.hidden, mode, self.act,
                                                 _native.PRECISIONS[self.precision])
        return self._plans[key]

    def _param_key(self, device, plan) -> Tuple:
        """(layout key, parameter versions).  The packed layout is a function of (tile, width, dregs, cregs,
        n_hidden) -- ff_layout.h make_layout -- and not of the kernel instantiation: the state-only and the
        divergence-capable kernels of one shape share a buffer."""
        vers = tuple((p.data_ptr(), p._version) for l in self.linears for p in (l.weight, l.bias))
        # (a pull plan's buffer holds the transposed network too: a key of its own)
        return (str(device), plan.precision, plan.tile, plan.width, plan.dregs, plan.cregs, plan.n_hidden) + \
            (("pull",) if _native.is_pull_plan(plan) else ()), vers

    def _pack(self, plan) -> torch.Tensor:
        return _native.pack_weights(plan, [l.weight for l in self.linears], [l.bias for l in self.linears],
                                    self.hidden, self.x_col0, self.c_col0)

    def push_plan(self) -> _native.PlanStruct:
        """The push-forward unit of this network (ff_mlp_push_plan); NotImplementedError with the envelope if none holds it."""
        if "push" not in self._plans:
            self._plans["push"] = _native.make_push_plan(self.dim, self.cond_dim, self.hidden, self.act,
                                                         _native.PRECISIONS[self.precision])
        return self._plans["push"]

    def pull_plan(self) -> _native.PlanStruct:
        """The pull-back unit of this network (ff_mlp_pull_plan); NotImplementedError with the envelope if none holds it."""
        if "pull" not in self._plans:
            self._plans["pull"] = _native.make_pull_plan(self.dim, self.cond_dim, self.hidden, self.act,
                                                         _native.PRECISIONS[self.precision])
        return self._plans["pull"]

    def wpack(self, device, mode: int, plan=None) -> torch.Tensor:
        plan = self.plan(mode) if plan is None else plan
        layout, vers = self._param_key(device, plan)
        hit = self._wpack.get(layout)
        if hit is None or hit[0] != vers:
            hit = (vers, self._pack(plan).to(device))
            self._wpack[layout] = hit
        return hit[1]

    # -- launch -----------------------------------------------------------------------------
    def integrate(self, x: torch.Tensor, etab: torch.Tensor, mode: int = MODE_STATE,
                  cond: Optional[torch.Tensor] = None, probe: Optional[torch.Tensor] = None,
                  noise: Optional[torch.Tensor] = None,
                  in_shift=None, in_scale=None, out_scale=None, out_shift=None,
                  rng: Optional[Tuple[int, int, int]] = None, stage_slots: int = 0, plan=None, per_probe: bool = False):
        """Run the fused integration.  Returns (y_final [B,D], dlogp [B] or empty, status [1]) -- with ``per_probe=True``
        (MODE_HUTCH, fp32 kernels, no noise rows) (y_final, dlogp, per-probe divergences [B, K], status): the first two
        bitwise what the call without it returns, column k of the third the integral of p_k^T J p_k of probe k as given.
        ``rng = (seed, global index of row 0, noise index of table row 0)`` selects in-kernel noise for
        tables with noise rows (instead of a ``noise`` buffer).  ``plan``: another plan of this network that shares the
        mode's packed weights (``FusedPair``'s select plan); default ``self.plan(mode)``."""
        if not x.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {x.device}); there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(x.shape)}")
        dev = x.device
        plan = self.plan(mode) if plan is None else plan
        if self.cond_dim > 0:
            if cond is None:
                raise ValueError("this network has conditional inputs; `conditional` is required")
            cond = f32_on(cond, dev)
            if cond.dim() != 2 or cond.shape != (x.shape[0], self.cond_dim):
                raise ValueError(f"conditional must be [batch, {self.cond_dim}], got {tuple(cond.shape)}")
        else:
            cond = None
        args = (f32_on(x, dev), cond, f32_on(probe, dev), f32_on(noise, dev), self.wpack(dev, mode), f32_on(etab, dev),
                f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
                _native.plan_words(plan, stage_slots), mode)
        if per_probe:
            if mode != MODE_HUTCH or noise is not None or rng is not None or args[2] is None:
                raise ValueError("per_probe=True: a Hutchinson solve (MODE_HUTCH with a probe, no noise rows)")
            return torch.ops.flowfusion_amd.mlp_ode_probes(*args[:3], *args[4:11], _native.probe_count(args[2]))
        if rng is not None:
            if mode != MODE_STATE or noise is not None:
                raise ValueError("in-kernel noise applies to state-only integration without a noise buffer")
            return torch.ops.flowfusion_amd.mlp_ode(*args, 0, 0, int(rng[0]), int(rng[1]), int(rng[2]))
        if mode == MODE_HUTCH and _native.probe_count(args[2]):      # K probes per sample: probe [B, K, D]
            return torch.ops.flowfusion_amd.mlp_ode(*args, 0, _native.probe_count(args[2]))
        if mode != MODE_EXACT:
            return torch.ops.flowfusion_amd.mlp_ode(*args)
        # exact trace = sum over dimensions of unit-tangent contributions: integrate it in the
        # cheapest set of launches (each carries at most tile - 1 tangents per sample) and add up
        total = status = None
        for first, count in exact_trace_passes(self.dim, plan.tile):
            y, dl, st = torch.ops.flowfusion_amd.mlp_ode(*args, first, count)
            total = dl if total is None else total + dl
            status = st if status is None else (status | st)
        return y, total, status

    def pushforward(self, x: torch.Tensor, etab: torch.Tensor, tangents: Optional[torch.Tensor] = None,
                    cond: Optional[torch.Tensor] = None, cond_tangents: Optional[torch.Tensor] = None,
                    unit: Optional[Tuple[int, int]] = None, in_shift=None, in_scale=None, out_scale=None, out_shift=None,
                    stage_slots: int = 0):
        """The fused fixed-grid solve of ``integrate`` with K tangents per sample pushed through it, on the push-forward
        unit (``push_plan``; ``etab`` has ITS width).  Returns (y_final [B, D], dy [B, K, D], status [1]):
        ``dy[b, k] = d y_final[b] / d (x[b], cond[b]) . (tangents[b, k], cond_tangents[b, k])``, the exact derivative of
        the discrete solver map (either part may be None = zero), or with ``unit = (first, count)`` its columns for the
        unit vectors ``first .. first + count - 1`` of the combined space [0, D + C).  The affine maps act on tangents
        by their linear parts (``/ in_scale``, ``* out_scale``); ``cond`` and ``cond_tangents`` are taken as given.
        ``y_final`` is bitwise the state of a ``num_probes=K`` Hutchinson ``integrate`` of the same rows."""
        if not x.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {x.device}); there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(x.shape)}")
        dev = x.device
        plan = self.push_plan()
        B = x.shape[0]
        if self.cond_dim > 0:
            if cond is None:
                raise ValueError("this network has conditional inputs; `conditional` is required")
            cond = f32_on(cond, dev)
            if cond.dim() != 2 or cond.shape != (B, self.cond_dim):
                raise ValueError(f"conditional must be [batch, {self.cond_dim}], got {tuple(cond.shape)}")
        else:
            cond = None
        if unit is not None:
            first, K = int(unit[0]), int(unit[1])
            tangents = cond_tangents = None
        else:
            first = 0
            given = tangents if tangents is not None else cond_tangents
            if given is None or given.dim() != 3:
                raise ValueError("pushforward: tangents [batch, K, dim] and / or cond_tangents [batch, K, cond_dim], or unit=(first, count)")
            K = int(given.shape[1])
        return torch.ops.flowfusion_amd.mlp_ode_push(
            f32_on(x, dev), cond, f32_on(tangents, dev), f32_on(cond_tangents, dev), self.wpack(dev, MODE_HUTCH, plan),
            f32_on(etab, dev), f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), unit is not None, first, K)

    def pullback(self, x: torch.Tensor, etab: torch.Tensor, cotangents: torch.Tensor, cond: Optional[torch.Tensor] = None,
                 want_cond: bool = False, in_shift=None, in_scale=None, out_scale=None, out_shift=None, stage_slots: int = 0):
        """The fused continuous-adjoint solve on the pull-back unit (``pull_plan``; ``etab`` has ITS width and holds the
        rows of the REVERSED span of the solve that produced ``x``).  Returns (retraced state [B, D], gx [B, K, D],
        gc [B, K, C] or None, status [1]): ``gx[b, k] = cotangents[b, k]^T d x[b] / d (retraced state)[b]`` and ``gc``
        likewise for ``cond`` as given -- the continuous adjoint integrated with the table's method, not the transpose of
        ``pushforward``'s discrete derivative.  The affine maps are this launch's own: ``in_*`` undo the output map of the
        forward solve, ``out_*`` redo its input map; cotangents come in the units of ``x`` and leave in those of the
        retraced state."""
        if not x.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {x.device}); there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(x.shape)}")
        dev = x.device
        plan = self.pull_plan()
        B = x.shape[0]
        if self.cond_dim > 0:
            if cond is None:
                raise ValueError("this network has conditional inputs; `conditional` is required")
            cond = f32_on(cond, dev)
            if cond.dim() != 2 or cond.shape != (B, self.cond_dim):
                raise ValueError(f"conditional must be [batch, {self.cond_dim}], got {tuple(cond.shape)}")
        else:
            cond = None
        if cotangents is None or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, self.dim):
            raise ValueError(f"pullback: cotangents [batch, K, {self.dim}]")
        want = bool(want_cond and self.cond_dim > 0)
        y, gx, gc, status = torch.ops.flowfusion_amd.mlp_ode_pull(
            f32_on(x, dev), cond, f32_on(cotangents, dev).contiguous(), self.wpack(dev, MODE_HUTCH, plan), f32_on(etab, dev),
            f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), want)
        return y, gx, (gc if want else None), status

    def _pull_cond(self, cond: Optional[torch.Tensor], B: int, dev) -> Optional[torch.Tensor]:
        """``cond`` as the record and discrete-adjoint launches take it: [B, cond_dim] fp32 on ``dev``, None without inputs."""
        if self.cond_dim == 0:
            return None
        if cond is None:
            raise ValueError("this network has conditional inputs; `conditional` is required")
        cond = f32_on(cond, dev)
        if cond.dim() != 2 or cond.shape != (B, self.cond_dim):
            raise ValueError(f"conditional must be [batch, {self.cond_dim}], got {tuple(cond.shape)}")
        return cond

    def record(self, x: torch.Tensor, etab: torch.Tensor, cond: Optional[torch.Tensor] = None, stage_slots: int = 0,
               in_shift=None, in_scale=None, out_scale=None, out_shift=None):
        """The fused fixed-grid solve of the state on the record unit (the sibling of ``pull_plan``'s; ``etab`` has ITS width
        and holds the rows of the FORWARD span) that writes every stage state down.  Returns (x_out [B, D], record
        [n_evals, B, D], status [1]): ``record[e, b]`` = the stage state y_e of row e in the integrated state's units --
        what ``pullback_discrete`` reads backwards."""
        if not x.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {x.device}); there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(x.shape)}")
        dev = x.device
        plan = self.pull_plan()
        cond = self._pull_cond(cond, x.shape[0], dev)
        return torch.ops.flowfusion_amd.mlp_ode_record(
            f32_on(x, dev), cond, self.wpack(dev, MODE_HUTCH, plan), f32_on(etab, dev),
            f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots))

    def pullback_discrete(self, record: torch.Tensor, etab: torch.Tensor, cotangents: torch.Tensor,
                          cond: Optional[torch.Tensor] = None, want_cond: bool = False, in_shift=None, in_scale=None,
                          out_scale=None, out_shift=None, stage_slots: int = 0):
        """The exact discrete adjoint on the discrete-adjoint unit (the sibling of ``pull_plan``'s): the transposed row program
        of the FORWARD rows ``etab``, run backwards over ``record`` (``record`` of the same table, conditional and maps --
        the maps here are the FORWARD solve's, unlike ``pullback``'s).  Returns (gx [B, K, D], gc [B, K, C] or None, status
        [1]): ``gx[b, k] = cotangents[b, k]^T d x_out[b] / d x[b]`` and ``gc`` likewise for ``cond`` as given -- the transpose
        of ``pushforward``'s derivative."""
        if not record.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {record.device}); there is no CPU fallback")
        if record.dim() != 3 or record.shape[2] != self.dim or record.shape[0] != etab.shape[0]:
            raise ValueError(f"expected a [{int(etab.shape[0])}, batch, {self.dim}] record, got {tuple(record.shape)}")
        dev = record.device
        plan = self.pull_plan()
        B = int(record.shape[1])
        cond = self._pull_cond(cond, B, dev)
        if cotangents is None or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, self.dim):
            raise ValueError(f"pullback_discrete: cotangents [batch, K, {self.dim}]")
        want = bool(want_cond and self.cond_dim > 0)
        gx, gc, status = torch.ops.flowfusion_amd.mlp_ode_pull_discrete(
            f32_on(record, dev), cond, f32_on(cotangents, dev).contiguous(), self.wpack(dev, MODE_HUTCH, plan), f32_on(etab, dev),
            f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), want)
        return gx, (gc if want else None), status

    def logp_grad(self, rec: torch.Tensor, table: torch.Tensor, probe: torch.Tensor, cot: torch.Tensor,
                  weight: Optional[torch.Tensor] = None, cond: Optional[torch.Tensor] = None, want_cond: bool = False,
                  stage_slots: int = 0, in_shift=None, in_scale=None, out_scale=None, out_shift=None):
        """The gradient of a fixed-grid Hutchinson log-density on the log-density gradient unit (the sibling of
        ``pull_plan``'s): the transposed row program of the FORWARD rows ``table`` with the divergence integral in it, run
        backwards over ``rec`` (``record`` of the same table, conditional and maps).  ``probe`` [B, D]: each row's probe;
        ``cot`` [B, D]: the cotangent of its final state; ``weight`` [B] or None (= 1): that of its divergence integral.
        Returns (gx [B, D], gc [B, C] or None, status [1]): the gradient of ``weight * lp + <cot, x_out>`` with respect to the
        record launch's ``x`` and ``cond`` as given, at fixed probes."""
        if not rec.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {rec.device}); there is no CPU fallback")
        if rec.dim() != 3 or rec.shape[2] != self.dim or rec.shape[0] != table.shape[0]:
            raise ValueError(f"expected a [{int(table.shape[0])}, batch, {self.dim}] record, got {tuple(rec.shape)}")
        dev = rec.device
        plan = self.pull_plan()
        B = int(rec.shape[1])
        cond = self._pull_cond(cond, B, dev)
        for name, t in (("probe", probe), ("cot", cot)):
            if t is None or tuple(t.shape) != (B, self.dim):
                raise ValueError(f"logp_grad: {name} [batch, {self.dim}]")
        if weight is not None and tuple(weight.shape) != (B,):
            raise ValueError("logp_grad: weight [batch]")
        want = bool(want_cond and self.cond_dim > 0)
        gx, gc, status = torch.ops.flowfusion_amd.mlp_ode_logp_grad(
            f32_on(rec, dev), cond, f32_on(probe, dev), f32_on(weight, dev), f32_on(cot, dev), self.wpack(dev, MODE_HUTCH, plan),
            f32_on(table, dev), f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), want)
        return gx, (gc if want else None), status

    def vjp_products(self, x: torch.Tensor, etab: torch.Tensor, seeds: torch.Tensor, per_row: bool = False,
                     cond: Optional[torch.Tensor] = None, stage_slots: int = 0, in_shift=None, in_scale=None, out_scale=None,
                     out_shift=None):
        """The fused fixed-grid solve of the state on the products unit (the sibling of ``pull_plan``'s; ``etab`` has ITS
        width and holds the rows of the FORWARD span) with K products per evaluation row.  ``seeds`` [B, K, D] (the same on
        every row) or, with ``per_row``, [n_evals, B, K, D].  Returns (x_out [B, D], prod [n_evals, B, K, D], status [1]):
        ``prod[e, b, k] = a_e seed + b_e J_net(y_e)^T seed`` at the stage state of row e -- row e of
        ``mlp_ode_jacobians``' record applied to the seed, without the record.  Seeds and products are in the units of the
        integrated state; the state never depends on them."""
        if not x.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {x.device}); there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(x.shape)}")
        dev = x.device
        plan = self.pull_plan()
        B, n = x.shape[0], int(etab.shape[0])
        if self.cond_dim > 0:
            if cond is None:
                raise ValueError("this network has conditional inputs; `conditional` is required")
            cond = f32_on(cond, dev)
            if cond.dim() != 2 or cond.shape != (B, self.cond_dim):
                raise ValueError(f"conditional must be [batch, {self.cond_dim}], got {tuple(cond.shape)}")
        else:
            cond = None
        want = ((n, B) if per_row else (B,))
        if seeds is None or seeds.dim() != len(want) + 2 or tuple(seeds.shape[:-2]) != want or seeds.shape[-1] != self.dim:
            raise ValueError(f"vjp_products: seeds {list(want) + ['K', self.dim]}, got {None if seeds is None else tuple(seeds.shape)}")
        K = int(seeds.shape[-2])
        if not 1 <= K <= _native.MAX_VJP_SEEDS:
            raise ValueError(f"vjp_products: 1 <= K <= {_native.MAX_VJP_SEEDS} seed columns beside the value column, got {K}")
        return torch.ops.flowfusion_amd.mlp_ode_vjp_products(
            f32_on(x, dev), cond, f32_on(seeds, dev), self.wpack(dev, MODE_HUTCH, plan), f32_on(etab, dev),
            f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots))

    def cached_table(self, key, device, build):
        """Evaluation tables depend only on (time span, method, options, schedule parameters, first-layer
        weights): keep the last few on the device so repeated solves skip the host work."""
        l0 = self.linears[0]
        full = (key, str(device), l0.weight.data_ptr(), l0.weight._version, l0.bias._version)
        hit = self._tables.get(full)
        if hit is None:
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            hit = build().to(device)
            self._tables[full] = hit
        return hit

    # -- adaptive stepping under the HOST controller: one launch per attempted step (flowfusion_amd/adaptive.py) -----------
    def make_step(self, schedule, sign: float, mode: int, device, cond=None, probe=None, launcher=None):
        """Step function for ``adaptive.Dopri5``.  ``schedule(t_real fp32 [n]) -> (a, b, c1)`` supplies
        the time-dependent scalars and first-layer bias; ``sign`` = -1 for a decreasing span (solved
        in reversed time with the right-hand side negated).  ``launcher`` replaces the GPU launch in
        the CPU tests (kernel-semantics emulator)."""
        plan = self.plan(mode)
        width = self.width(mode)        # first-layer bias words per row (two networks' worth on a pair plan)
        cond_d = f32_on(cond, device) if self.cond_dim > 0 else None
        probe_d = f32_on(probe, device)
        own = launcher is None
        if own:
            wpack = self.wpack(device, mode)
            launcher = lambda y, k1, kl1, lp0, etab, n_aux, first, count, used=0: torch.ops.flowfusion_amd.mlp_ode_step(
                y, cond_d, probe_d, k1, kl1, lp0, wpack, etab.to(device), _native.plan_words(plan, used), mode, n_aux, first, count)
        # (Hutchinson with a [B, K, D] probe: the count of the launch is K)
        passes = [(0, _native.probe_count(probe_d) if mode == MODE_HUTCH else 0)] if mode != MODE_EXACT else \
            exact_trace_passes(self.dim, plan.tile)

        def step(y, k1, lp0, kl1, t_rows, cin, slots, tail, use_y, n_aux):
            n = int(t_rows.numel())
            used = int(slots.max()) + 1
            self.require_slots(used, mode, "this adaptive method")
            hint = {"used": used} if own else {}
            a, b, c1 = schedule(sign * t_rows)
            rows = torch.zeros(n + 2, ROW_HDR + width, dtype=torch.float32)
            rows[:n, ROW_A] = sign * a
            rows[:n, ROW_B] = sign * b
            ints = rows.view(torch.int32)
            ints[:n, ROW_SLOT] = slots
            rows[:n, ROW_CIN] = cin
            rows[:n, ROW_HDR:ROW_HDR + c1.shape[1]] = c1
            rows[n, ROW_CIN], rows[n, ROW_AUX_COEF] = tail[0], tail[1]
            rows[n + 1, ROW_CIN], rows[n + 1, ROW_AUX_COEF] = tail[2], tail[3]
            ints[n, ROW_USE_Y] = use_y
            aux = aux_lp = None
            for i, (first, count) in enumerate(passes):
                o, olp = launcher(y, k1, kl1 if i == 0 else None, lp0 if i == 0 else None, rows, n_aux, first, count, **hint)
                aux = o if aux is None else aux
                aux_lp = olp if aux_lp is None else aux_lp + olp
            return aux, (aux_lp if mode != MODE_STATE else None)

        return step

    # -- first layer pieces used by the table builders ---------------------------------------
    def time_columns(self, device, c0: int, c1: int):
        """(W1[:, c0:c1] contiguous, bias) of the first layer as fp32 device tensors -- what the device-side adaptive
        controller multiplies the time features with (ff_adapt_config.w0t / b0).  Cached until a parameter changes."""
        l0 = self.linears[0]
        key = (str(device), c0, c1, l0.weight.data_ptr(), l0.weight._version, l0.bias.data_ptr(), l0.bias._version)
        hit = self.__dict__.get("_time_cols")
        if hit is None or hit[0] != key:
            w = l0.weight.detach()[:, c0:c1].to(device, torch.float32).contiguous()
            b = l0.bias.detach().to(device, torch.float32).contiguous()
            hit = (key, w, b)
            self._time_cols = hit
        return hit[1], hit[2]

    def first_layer_cpu(self):
        l0 = self.linears[0]
        return (l0.weight.detach().to("cpu", torch.float32), l0.bias.detach().to("cpu", torch.float32))

    def width(self, mode: int = MODE_STATE) -> int:
        return int(self.plan(mode).width)

    def stage_slots(self, mode: int = MODE_STATE) -> int:
        """Runge-Kutta stage slots the selected kernel keeps on chip: 7 (FF_MAX_SLOTS) everywhere except the split-precision
        kernels for states of 17-32 dimensions, which keep 4 (csrc/ff_split_layout.h slots_on_chip)."""
        plan = self.plan(mode)
        return 4 if (plan.precision != _native.PREC_F32 and plan.dregs == 16) else 7

    def require_slots(self, used: int, mode: int, what: str):
        if used > self.stage_slots(mode):
            raise NotImplementedError(
                f"precision={self.precision!r} with {self.dim} state dimensions keeps {self.stage_slots(mode)} Runge-Kutta stage "
                f"slots on chip and {what} needs {used}: use euler / midpoint / heun3 / rk4 / rk4_classic (or bosh3 / fehlberg2 "
                "/ adaptive_heun), or precision='f32'")


class FusedPair(FusedNet):
    """Kernel-side view of the two networks of a symplectic flow (flowfusion_amd/symplectic.py): ``mlp_q`` reading the p
    half of the state [q | p] and ``mlp_p`` reading the q half, each ``Linear -> SiLU -> ... -> Linear`` with first-layer
    input ``[state half | cond | time features]``, on one two-network kernel (csrc/ff_mlp_pair.hpp).  State-only: the
    field is divergence-free by construction.  ``dim`` is the whole state (2D); evaluation rows carry the c1 of net A
    (mlp_q), then net B's (mlp_p), ``width`` words each.

    A second plan kind, ``select=True`` (``ff_mlp_pair_select_plan``, the leapfrog route): the same shape and the same
    packed weights on the row-select kernel, whose rows run one network each and carry that network's c1 only."""

    def __init__(self, q_linears: Sequence[nn.Linear], p_linears: Sequence[nn.Linear], dim: int, cond_dim: int,
                 x_col0: int, c_col0: int):
        super().__init__(q_linears, dim // 2, cond_dim, x_col0, c_col0)
        self.p_linears = list(p_linears)
        if [int(l.out_features) for l in self.p_linears] != [int(l.out_features) for l in self.linears] or \
                len(self.p_linears) != len(self.linears):
            raise NotImplementedError("the two networks of a pair must have the same shape")
        for l in self.p_linears:
            if l.bias is None:
                raise NotImplementedError("Linear layers without bias are not supported")
        self.dim = int(dim)

    def serves(self, linears, act, precision: str = "f32", p_linears=()) -> bool:
        return (super().serves(linears, act, precision) and len(p_linears) == len(self.p_linears)
                and all(a is b for a, b in zip(p_linears, self.p_linears)))

    def plan(self, mode: int, select: bool = False) -> _native.PlanStruct:
        if mode != MODE_STATE:
            raise NotImplementedError("the two-network kernels integrate the state only (the field is divergence-free)")
        key = "select" if select else 0
        if key not in self._plans:
            self._plans[key] = _native.make_pair_plan(self.dim, self.cond_dim, self.hidden, select=select)
        return self._plans[key]

    def integrate_select(self, x, etab, cond=None, **maps):
        """``integrate`` of a table of select rows (solvers.plan_leapfrog): on the select plan, and on nothing else."""
        plan = self.plan(MODE_STATE, select=True)
        if not _native.is_select_plan(plan):
            raise RuntimeError("select rows need a select plan")
        return self.integrate(x, etab, MODE_STATE, cond=cond, stage_slots=1, plan=plan, **maps)

    def pull_select_plan(self) -> _native.PlanStruct:
        """The row-select pull-back unit of this pair (ff_mlp_pull_select_plan); NotImplementedError with the envelope if
        none holds it."""
        if "pull_select" not in self._plans:
            self._plans["pull_select"] = _native.make_pull_select_plan(self.dim, self.cond_dim, self.hidden)
        return self._plans["pull_select"]

    def pullback_select(self, z: torch.Tensor, etab: torch.Tensor, cotangents: torch.Tensor, cond: Optional[torch.Tensor] = None,
                        want_cond: bool = False, stage_slots: int = 1, in_shift=None, in_scale=None, out_scale=None,
                        out_shift=None):
        """The pull-back of K cotangents through select rows, on the row-select pull-back unit (``pull_select_plan``): ``etab``
        has ITS width (``width(MODE_STATE, pull_select=True)``) and holds the rows of the REVERSED grid of the leapfrog that
        produced ``z`` [B, 2D].  Returns (z_back [B, 2D], gz [B, K, 2D], gc [B, K, C] or None, status [1]): ``z_back`` the
        retraced start state, ``gz[b, k] = cotangents[b, k]^T d z[b] / d z_back[b]`` and ``gc`` likewise for ``cond`` as
        given -- on shear rows the exact transpose of the forward rows.  The affine maps are this launch's own, as
        ``pullback``'s are."""
        if not z.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {z.device}); there is no CPU fallback")
        if z.dim() != 2 or z.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(z.shape)}")
        dev = z.device
        plan = self.pull_select_plan()
        B = z.shape[0]
        cond = self._pull_cond(cond, B, dev)
        if cotangents is None or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, self.dim):
            raise ValueError(f"pullback_select: cotangents [batch, K, {self.dim}]")
        want = bool(want_cond and self.cond_dim > 0)
        y, gz, gc, status = torch.ops.flowfusion_amd.mlp_ode_pull_select(
            f32_on(z, dev), cond, f32_on(cotangents, dev).contiguous(), self.wpack(dev, MODE_STATE, plan), f32_on(etab, dev),
            f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), want)
        return y, gz, (gc if want else None), status

    def push_select_plan(self) -> _native.PlanStruct:
        """The row-select push-forward unit of this pair (ff_mlp_push_select_plan); NotImplementedError with the envelope if
        none holds it."""
        if "push_select" not in self._plans:
            self._plans["push_select"] = _native.make_push_select_plan(self.dim, self.cond_dim, self.hidden)
        return self._plans["push_select"]

    def pushforward_select(self, z: torch.Tensor, etab: torch.Tensor, tangents: Optional[torch.Tensor] = None,
                           cond: Optional[torch.Tensor] = None, cond_tangents: Optional[torch.Tensor] = None,
                           unit: Optional[Tuple[int, int]] = None, stage_slots: int = 1, in_shift=None, in_scale=None,
                           out_scale=None, out_shift=None):
        """K tangents per sample pushed through select rows, on the row-select push-forward unit (``push_select_plan``):
        ``etab`` has ITS width (``width(MODE_STATE, push_select=True)``) and holds the rows of a leapfrog grid.  Returns
        (z_out [B, 2D], dz [B, K, 2D], status [1]): ``z_out`` the state ``integrate_select`` gives on the same rows,
        ``dz[b, k] = d z_out[b] / d (z[b], cond[b]) . (tangents[b, k], cond_tangents[b, k])``, the exact derivative of the
        discrete leapfrog (either part may be None = zero), or with ``unit = (first, count)`` its columns for the unit vectors
        ``first .. first + count - 1`` of the combined space [0, 2D + C).  The affine maps act on tangents by their linear
        parts, as ``pushforward``'s do; ``cond`` and ``cond_tangents`` are taken as given."""
        if not z.is_cuda:
            raise RuntimeError(
                "flowfusion_amd integrates on the GPU only: move the model and its inputs to 'cuda' "
                f"(got a tensor on {z.device}); there is no CPU fallback")
        if z.dim() != 2 or z.shape[1] != self.dim:
            raise ValueError(f"expected a [batch, {self.dim}] state, got {tuple(z.shape)}")
        dev = z.device
        plan = self.push_select_plan()
        cond = self._pull_cond(cond, z.shape[0], dev)
        if unit is not None:
            first, K = int(unit[0]), int(unit[1])
            tangents = cond_tangents = None
        else:
            first = 0
            given = tangents if tangents is not None else cond_tangents
            if given is None or given.dim() != 3:
                raise ValueError("pushforward_select: tangents [batch, K, dim] and / or cond_tangents [batch, K, cond_dim], or "
                                 "unit=(first, count)")
            K = int(given.shape[1])
        return torch.ops.flowfusion_amd.mlp_ode_push_select(
            f32_on(z, dev), cond, f32_on(tangents, dev), f32_on(cond_tangents, dev), self.wpack(dev, MODE_STATE, plan),
            f32_on(etab, dev), f32_on(in_shift, dev), f32_on(in_scale, dev), f32_on(out_scale, dev), f32_on(out_shift, dev),
            _native.plan_words(plan, stage_slots), unit is not None, first, K)

    def _param_key(self, device, plan) -> Tuple:
        vers = tuple((p.data_ptr(), p._version) for l in self.linears + self.p_linears for p in (l.weight, l.bias))
        # (a pull-select plan's buffer holds two pull packs, a push-select plan's two forward packs of ITS unit: keys of their own)
        return (str(device), plan.tile, plan.width, plan.dregs, plan.cregs, plan.n_hidden) + \
            (("pull_select",) if _native.is_pull_select_plan(plan) else ()) + \
            (("push_select",) if _native.is_push_select_plan(plan) else ()), vers

    def _pack(self, plan) -> torch.Tensor:
        if _native.is_pull_select_plan(plan):
            return _native.pack_pull_select_weights(plan, self.linears, self.p_linears, self.hidden, self.x_col0, self.c_col0)
        if _native.is_push_select_plan(plan):
            return _native.pack_push_select_weights(plan, self.linears, self.p_linears, self.hidden, self.x_col0, self.c_col0)
        return _native.pack_pair_weights(plan, self.linears, self.p_linears, self.hidden, self.x_col0, self.c_col0)

    def cached_table(self, key, device, build):
        q0, p0 = self.linears[0], self.p_linears[0]
        key = (key, p0.weight.data_ptr(), p0.weight._version, p0.bias._version)
        return super().cached_table(key, device, build)

    def first_layers_cpu(self):
        """Host copies of both first layers: ((W_q, b_q), (W_p, b_p))."""
        return tuple((l.weight.detach().to("cpu", torch.float32), l.bias.detach().to("cpu", torch.float32))
                     for l in (self.linears[0], self.p_linears[0]))

    def time_columns(self, device, c0: int, c1: int):
        """Both first layers' columns [c0, c1) and biases, stacked as the device controller takes them for a pair plan:
        ``[net A rows | zero pad | net B rows | zero pad]``, ``width`` rows each."""
        layers = (self.linears[0], self.p_linears[0])
        key = (str(device), c0, c1) + tuple((l.weight.data_ptr(), l.weight._version, l.bias.data_ptr(), l.bias._version)
                                            for l in layers)
        hit = self.__dict__.get("_time_cols")
        if hit is None or hit[0] != key:
            H = int(self.plan(MODE_STATE).width)
            w = torch.zeros(2 * H, c1 - c0, dtype=torch.float32)
            b = torch.zeros(2 * H, dtype=torch.float32)
            for i, l in enumerate(layers):
                h = int(l.out_features)
                w[i * H:i * H + h] = l.weight.detach()[:, c0:c1].to("cpu", torch.float32)
                b[i * H:i * H + h] = l.bias.detach().to("cpu", torch.float32)
            hit = (key, w.to(device).contiguous(), b.to(device).contiguous())
            self._time_cols = hit
        return hit[1], hit[2]

    def width(self, mode: int = MODE_STATE, select: bool = False, pull_select: bool = False, push_select: bool = False) -> int:
        """First-layer bias words per evaluation row: two networks' worth; one network's on the select plan; one network's of
        the pull-select / push-select plan's width with ``pull_select=True`` / ``push_select=True`` (their units may be wider
        than the pair plan's)."""
        if pull_select:
            return int(self.pull_select_plan().width)
        if push_select:
            return int(self.push_select_plan().width)
        return (1 if select else 2) * int(self.plan(mode).width)

    def stage_slots(self, mode: int = MODE_STATE) -> int:
        return 7


def require_fp32(module, *tensors, what="this solve"):
    """The kernels compute in fp32, the dtype the reference's constructors create (and every BASELINE configuration uses).
    The reference itself follows the dtype of its parameters and inputs -- a ``.double()`` model solves in float64 there --
    so anything else is refused here rather than rounded to fp32 behind the caller's back."""
    for p in module.parameters():
        if p.dtype != torch.float32:
            raise TypeError(f"flowfusion_amd: {what} computes in float32; the model holds {p.dtype} parameters (the reference "
                            "would solve in that dtype) -- cast the model with .float()")
    for t in tensors:
        if t is not None and torch.is_tensor(t) and t.is_floating_point() and t.dtype != torch.float32:
            raise TypeError(f"flowfusion_amd: {what} computes in float32; got a {t.dtype} input (the reference would "
                            "solve in that dtype) -- cast it with .float()")
