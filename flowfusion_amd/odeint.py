"""The one place where an ODE solve of a score model (diffusion.py) or a flow (flow.py) picks its route.

* **generic**: a network no compiled kernel holds is evaluated by torch, the library steps around it (generic.py);
* **fixed grid**: one fused launch per solve, the PopulationModel / flow affine maps in its prologue and epilogue;
* **device controller**: the adaptive loop on the GPU (device_adaptive.py);
* **host controller**: the adaptive loop in Python (adaptive.py), for what the device controller cannot describe.

Hutch++ / XTrace solves take the same routes with the Jacobian of every evaluation row recorded (host_stepper.py).  The
front ends supply only what differs between them: ``_fusable()`` / ``_net()``, ``_device_schedule(device)``,
``_host_schedule()``, ``_ode_table(...)`` with ``_schedule_key()``, and ``_module_rhs(mode, cond, probe)`` for the generic
route.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _native, adaptive, device_adaptive, solvers, trace_estimators
from ._native import MODE_EXACT, MODE_HUTCH, MODE_STATE
from .fused import require_fp32
from .generic import ModuleStepper, _need_gpu
from .host_stepper import RowStepper


def _fixed_grid(front, net, x, t_span, method, options, mode, **launch):
    """The fused fixed-grid solve: the evaluation table (cached on the device; built per call where a ``grid_constructor``
    may make it depend on y0), then ONE ``net.integrate(x, table, mode, **launch)``, whose result it returns."""
    if (options or {}).get("grid_constructor") is not None:
        table = front._ode_table(t_span, method, options, mode, y0=x).to(x.device)
    else:
        key = (tuple(float(v) for v in t_span), method, repr(sorted((options or {}).items())), mode) + front._schedule_key()
        table = net.cached_table(key, x.device, lambda: front._ode_table(t_span, method, options, mode))
    return net.integrate(x, table, mode, stage_slots=solvers.resolve_method(method).stages, **launch)


ESTIMATOR_MIN_BYTES = 1 << 30      # a fixed-grid estimator solve cuts its batch no finer than this many bytes per chunk
PRODUCTS = ("jacobian", "vjp")
MAX_PRODUCT_SEEDS = _native.MAX_VJP_SEEDS      # seed columns of the second sweep: r + m (Hutch++) or m (XTrace)


def check_products(front, products, method, options, kind=None, r=0, m=0):
    """The refusals of ``products="vjp"`` (``solve``), raised before the device is touched; each names the way out.
    ``kind`` None: the front end is not an estimator model."""
    if products not in PRODUCTS:
        raise ValueError(f"products={products!r}: expected 'jacobian' (the recorded-Jacobian route, the default) or 'vjp'")
    if products == "jacobian":
        return
    if kind is None:
        raise ValueError("products='vjp' is a route of the Hutch++ / XTrace estimators: construct the model with hutchpp=True "
                         "or xtrace=True (hutchinson=True and the exact trace have their own fused launches)")
    if method in solvers.ALL_ADAPTIVE or method in solvers.ADAPTIVE_METHODS:
        raise ValueError(f"products='vjp' with the adaptive method={method!r}: the two sweeps run over a fixed grid; use "
                         "method=\"rk4\" / \"dopri5_fixed\" with options={\"step_size\": h}, or products=\"jacobian\"")
    solvers.resolve_method(method)
    for name in ("grid_constructor", "perturb"):
        if (options or {}).get(name) not in (None, False):
            raise ValueError(f"products='vjp' with options[{name!r}]: the grid is the uniform one of "
                             "options={\"step_size\": h} (or the nodes of t_span); or use products=\"jacobian\"")
    prec = getattr(front, "precision", "f32")
    if prec != "f32":
        raise ValueError(f"products='vjp' with precision={prec!r}: the products kernels compute in f32; use precision='f32'")
    seeds = r + m if kind == "hutchpp" else r
    if seeds > MAX_PRODUCT_SEEDS:
        what = f"hpp_rank + hpp_vecs = {r} + {m}" if kind == "hutchpp" else f"xt_vecs = {r}"
        raise ValueError(f"products='vjp' with {what} > {MAX_PRODUCT_SEEDS}: a sample and the second sweep's seeds share the "
                         "16 columns of one tile; use products=\"jacobian\"")
    try:
        if not front._fusable():
            raise NotImplementedError("products='vjp' needs the library's MLP (a ``model=`` module has no products kernel)")
        front._net().pull_plan()
    except NotImplementedError as e:
        msg = str(e)
        raise NotImplementedError(msg if _native.PULL_ENVELOPE in msg else
                                  f"{msg} -- {_native.PULL_ENVELOPE}; there is no module-path fallback: use "
                                  "products=\"jacobian\"") from None


def solve(front, x, t_span, method, options, mode, atol, rtol, cond=None, probe=None, norm_only=(), estimator=None,
          div_fn=None, in_shift=None, in_scale=None, out_scale=None, out_shift=None, products="jacobian"):
    """``odeint(front, x, t_span, method=, atol=, rtol=, options=)``; returns (y [B, D], dlogp [B] or None) and sets
    ``front.last_solver_stats`` (fused fixed-grid solves leave it alone).

    ``norm_only``: state components the reference carries with a zero derivative (a flow's raw conditional), seen by the
    adaptive error norm only.  ``estimator = (kind, probes)``: a Hutch++ / XTrace solve in MODE_EXACT (``div_fn(A)`` is its
    estimate on the host controller; on the generic route the front end's module estimates by itself).  The affine maps
    (PopulationModel*, flow sampling): ``(x - in_shift) / in_scale`` before the solve, ``y * out_scale + out_shift`` after
    it -- on the host around the adaptive and generic routes, in the kernel's prologue / epilogue on fixed grids.

    ``products`` (estimator solves): ``"jacobian"`` (default) records the Jacobian of every evaluation row
    (``RowStepper.run_table_recorded``, ``n_evals * B * D * D`` floats through memory, D + 1 tile columns per sample);
    ``"vjp"`` (opt-in, fixed grids, the pull-back units' networks) computes the estimators as the reference does, from
    J^T v products: two sweeps of the products unit and two streaming launches (``RowStepper.run_table_products``),
    ``(2r + m) D`` or ``2m D`` floats per evaluation and sample.  The two agree to rounding, not bitwise.  At small D the
    Jacobian route is the cheaper one (D + 1 columns undercut two sweeps of two networks).  ``check_products`` lists what
    ``"vjp"`` refuses; adaptive solves -- the reference's defaults -- always take the Jacobian route."""
    if products != "jacobian":
        if estimator is None:
            check_products(front, products, method, options)
        else:
            check_products(front, products, method, options, estimator[0], *_native.trace_kind_and_probes(*estimator)[3:])
    if estimator is None:           # (the estimator solves have never refused other dtypes: they cast the state to fp32)
        require_fp32(front, x, cond, probe, what="an ODE solve")
    fused = front._fusable()
    net = front._net() if fused else None
    adaptive_method = method in solvers.ALL_ADAPTIVE
    if fused and estimator is None and not adaptive_method:
        out = _fixed_grid(front, net, x, t_span, method, options, mode, cond=cond, probe=probe, in_shift=in_shift,
                          in_scale=in_scale, out_scale=out_scale, out_shift=out_shift)
        return out[0], (out[1] if mode != MODE_STATE else None)
    if in_shift is not None:
        x = (x - in_shift) / in_scale
    if fused and estimator is not None:
        x = x.detach().to(torch.float32).contiguous()
    if adaptive_method:
        t = t_span.detach().to("cpu", torch.float32).double()
        sign = -1.0 if bool(t[0] > t[-1]) else 1.0        # a decreasing span is solved in reversed time
        norm_only = tuple(c.detach().to(x.device, torch.float32) for c in norm_only)
    if not fused:
        # generic: the front end's module evaluated by torch, every stage combination one ff_stage_combine launch
        _need_gpu(x)
        stepper = ModuleStepper(front._module_rhs(mode, cond, probe), mode != MODE_STATE)
        if adaptive_method:
            y, lp = _host_adaptive(front, stepper.make_step(sign), x, t, sign, method, options, mode, atol, rtol, norm_only)
            front.last_solver_stats["evaluations"] = stepper.n_evals
        else:
            y, lp = stepper.run_plan(x, solvers.plan_ode(t_span, method, options, y0=x))
            front.last_solver_stats = {"evaluations": stepper.n_evals}
    elif not adaptive_method:
        # Hutch++ / XTrace on a fixed grid: one launch per tangent pass records every row's Jacobian, one launch estimates
        # all of them (the recorded Jacobians of a chunk of samples may take a quarter of the free device memory: cutting a
        # batch into many small launches leaves their last rounds of tiles mostly empty)
        kind, probes = estimator
        budget = max(ESTIMATOR_MIN_BYTES, _estimator_budget(x.device) // 2)
        if products == "vjp":
            # the same estimates from J^T v products: two sweeps of the products unit over the pull plan's table, the basis
            # between them and the combination after them (no Jacobian leaves the chip)
            grid = solvers.plan_ode(t_span, method, options)
            table = solvers.build_table(grid, *front._host_schedule()(grid.t_eval), int(net.pull_plan().width))
            y, lp = RowStepper(net, x.device, cond, None).run_table_products(
                x, table, kind, probes, cond=cond, max_bytes=budget, stage_slots=solvers.resolve_method(method).stages)
        else:
            div_rows = lambda A, lo, hi: _native.trace_estimate(A, kind, tuple(P[:, lo:hi] for P in probes))
            y, lp = RowStepper(net, x.device, cond, None).run_table_recorded(
                x, front._ode_table(t_span, method, options, MODE_EXACT), div_rows, cond=cond, max_bytes=budget)
    else:
        spec = front._device_schedule(x.device) if (x.is_cuda and method in solvers.NATIVE_ADAPTIVE) else None
        if device_adaptive.supported(spec, x, net, mode, options) and (estimator is None or device_adaptive.estimator_bytes(
                net, method, x.shape[0], *estimator) <= _estimator_budget(x.device)):
            # the whole loop on the device: attempts, error norms, step control, the next attempt's table rows
            y, lp, front.last_solver_stats = device_adaptive.solve(
                net, spec, sign, mode, x, float(sign * t[0]), float(sign * t[-1]), rtol, atol, options, method, cond=cond,
                probe=probe, norm_only=norm_only, estimator=estimator)
        else:
            # the host controller: one launch per attempted step, or per right-hand side for the estimators
            step = (net.make_step(front._host_schedule(), sign, mode, x.device, cond=cond, probe=probe) if estimator is None
                    else RowStepper(net, x.device, cond, div_fn).make_step(front._host_schedule(), sign))
            y, lp = _host_adaptive(front, step, x, t, sign, method, options, mode, atol, rtol, norm_only)
    if out_scale is not None:
        y = y * out_scale + out_shift
    return y, lp


PROBE_BUFFER_FLOATS = 1 << 28      # a K-probe device buffer [rows, K, D] holds FEWER floats than this (under 1 GiB): fixed-grid solves cut their rows to fit


def solve_hutchinson(front, x, t_span, method, options, atol, rtol, num_probes, probe_rng=None, keep=None, per_probe=False,
                     cond=None, norm_only=(), in_shift=None, in_scale=None):
    """``solve`` in MODE_HUTCH with ``num_probes`` = K >= 1 independent +-1 probes per sample, averaged; every Hutchinson
    log-density solve of the front ends.  Returns (y, dlogp, d): ``d`` [B, K] with ``per_probe``, else None.
    ``probe_rng``: None = torch's generator, or (seed, global row of row 0) = the counter-based stream
    (trace_estimators.hutchinson_probe).  ``keep(e)`` receives the +-1 probes -- before the solve where it is one
    launch sequence (ScoreModel.forward reads them on the generic route), after it where the rows were cut.

    K = 1 is the reference's single probe: ``hutchinson_probe(x, probe_rng)`` [B, D] handed to ``solve`` as it is (states
    of any rank that route takes, every precision, never cut).  What follows is K > 1 (extension), probes [B, K, D].

    The fused kernel carries the K probes of a sample in K tangent columns of its tile (ff_ode_args.tangent_count) and
    returns the SUM of their p^T J p, so it gets the probes times 1/sqrt(K).  On fixed grids the rows are cut so that a
    probe buffer on the device stays under ``PROBE_BUFFER_FLOATS`` floats (1 GiB); rows are independent, so the result
    does not depend on the cut.  Adaptive solves control the step over the whole batch and take it whole; so does a fixed
    grid from ``options["grid_constructor"]``, which may depend on the batch it is given.  The rule
    bounds device buffers only: torch's probes are drawn as ONE ``sign(randn(B, K, D))`` on the host (a row cut must
    not change which numbers a seed gives), and ``keep`` is handed the whole [B, K, D] set.

    ``per_probe=True`` (fixed grids, K >= 2; the front ends' ``return_stderr``): y and dlogp are bitwise those of the call
    without it and ``d[b, k]`` is what a single-probe solve with probe k alone gives.  Fused: the
    same launch also stores every tangent column's own integral (ff_mlp_ode_launch_probes); the kernel sees the probes
    times 1/sqrt(K), so its output is scaled by K.  Where the rows are cut the pieces are concatenated.  A network on the
    generic route (torch evaluates the module) makes the K-probe pass as before and then K single-probe passes over the
    same state and grid, one per probe -- K + 1 passes instead of one; the module's right-hand side keeps returning one
    divergence per row."""
    K = int(num_probes)
    if K < 1 or (per_probe and K < 2):
        raise ValueError(f"num_probes={num_probes}: at least one probe per sample, two for per_probe=True")
    if per_probe and method in solvers.ALL_ADAPTIVE:
        raise ValueError(f"per_probe=True with the adaptive method={method!r}: per-probe divergences are carried by fixed-grid "
                         "solves only (method=\"rk4\" / \"dopri5_fixed\" with options={\"step_size\": h})")
    if K > 1 and x.dim() != 2:
        raise NotImplementedError("num_probes > 1: only [batch, dim] states")
    fused = front._fusable()
    net = front._net() if fused else None
    if fused and K > 1:
        if net.precision != "f32":
            raise ValueError(f"num_probes={K} with precision={net.precision!r}: the split-precision kernels carry one probe per "
                             "sample; use precision='f32'")
        tile = int(net.plan(MODE_HUTCH).tile)
        if K > tile - 1:
            raise ValueError(f"num_probes={K}: the kernel of this network holds a sample and its probes in the {tile} columns of "
                             f"one tile, so at most {tile - 1} probes; use num_probes <= {tile - 1} (or the exact trace)")
    B = x.shape[0]
    rows = max(1, B)
    # (a grid_constructor may build the grid from y0 -- the batch it is handed: such a solve is not cut either)
    if K > 1 and fused and method not in solvers.ALL_ADAPTIVE and (options or {}).get("grid_constructor") is None:
        rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * x.shape[1]))
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    scale = K ** -0.5
    whole_cpu = torch.sign(torch.randn(B, K, x.shape[1])) if K > 1 and probe_rng is None else None      # (the reference's draw, with a K axis)

    def draw(r0, r1):
        """(+-1 probes or None, the kernel's probes) of rows [r0, r1)."""
        if K == 1:
            e = trace_estimators.hutchinson_probe(x, probe_rng)
            return e, e
        if probe_rng is None:
            e = whole_cpu[r0:r1].to(x.device)
        elif keep is None and (fused or not per_probe):      # nobody asks for the +-1 form: fill the scaled probes directly
            return None, _native.probe_fill(r1 - r0, K, x.shape[1], probe_rng[0], probe_rng[1] + r0, x.device, scale=scale)
        else:
            e = trace_estimators.hutchinson_probe(x[r0:r1], (probe_rng[0], probe_rng[1] + r0), K)
        return e, e * scale

    whole = len(pieces) == 1
    outs, es = [], []
    for r0, r1 in pieces:
        e, p = draw(r0, r1)
        if whole and keep is not None:
            keep(e)
        kw = dict(cond=cond if whole or cond is None else cond[r0:r1], in_shift=in_shift, in_scale=in_scale)
        xs = x if whole else x[r0:r1]
        if not per_probe:
            outs.append(solve(front, xs, t_span, method, options, MODE_HUTCH, atol, rtol, probe=p, norm_only=norm_only, **kw)
                        + (None,))
        elif fused:                 # the same launch stores every tangent column's own integral
            require_fp32(front, xs, kw["cond"], p, what="an ODE solve")
            y, lp, d, _ = _fixed_grid(front, net, xs, t_span, method, options, MODE_HUTCH, probe=p, per_probe=True, **kw)
            outs.append((y, lp, d * float(K)))
        else:
            outs.append(_generic_per_probe(front, xs, t_span, method, options, atol, rtol, e, p, keep, norm_only, kw))
        es.append(e)
    if not whole and keep is not None:
        keep(torch.cat(es))
    cat = (lambda ts: ts[0]) if whole else torch.cat
    y, lp, d = zip(*outs)
    return cat(y), cat(lp), (cat(d) if per_probe else None)


def _generic_per_probe(front, x, t_span, method, options, atol, rtol, e, p, keep, norm_only, kw):
    """Per-probe divergences of a network on the generic route: the K-probe pass (probes ``p``), then one single-probe pass
    per +-1 probe ``e[:, k]`` (a front end that reads the probe from its own attribute -- ScoreModel.forward -- is handed
    each probe through ``keep``, and the whole set again at the end); returns (y, dlogp, d [B, K])."""
    y, lp = solve(front, x, t_span, method, options, MODE_HUTCH, atol, rtol, probe=p, norm_only=norm_only, **kw)
    cols = []
    try:
        for k in range(e.shape[1]):
            ek = e[:, k].contiguous()
            if keep is not None:
                keep(ek)
            cols.append(solve(front, x, t_span, method, options, MODE_HUTCH, atol, rtol, probe=ek, norm_only=norm_only, **kw)[1])
    finally:                    # whatever a pass raised, the front end holds the whole [B, K, D] set again
        if keep is not None:
            keep(e)
    return y, lp, torch.stack(cols, dim=1)


def solve_push(front, x, t_span, method, options, tangents=None, cond=None, cond_tangents=None, unit=None, in_shift=None,
               in_scale=None, out_scale=None, out_shift=None, tangent_gain=None, cond_tangent_scale=None):
    """Flow-map sensitivities (extension): the fixed-grid solve of ``solve`` in MODE_STATE with K tangents per sample pushed
    through it.  Returns ``(y [B, D], dy [B, K, D])`` with ``dy[b, k] = d y[b] / d (x[b], cond[b]) . (tangents[b, k],
    cond_tangents[b, k])`` -- forward mode through the SAME discrete steps, so the exact derivative of the solver map, not
    of the continuous flow (they agree to the order of the method).  ``tangents`` [B, K, D] / ``cond_tangents`` [B, K, C]:
    either may be None (zero); ``unit = (first, count)`` instead of both: the unit vectors ``first .. first + count - 1`` of
    the combined space [0, D + C), K = count.  ``cond`` and ``cond_tangents`` are the network's (normalised) conditional
    inputs; the affine maps of ``solve`` act on the tangents by their linear parts, in the kernel.  What a front end did to
    its inputs on the host follows here, after the checks: ``x * tangent_gain`` and ``tangents * tangent_gain`` (a VE
    model's solve starts from the base samples times sigma_max; a tensor or None), ``cond_tangents / cond_tangent_scale``
    (``cond`` is the caller's, normalised by that scale).

    One launch of a push-forward unit per piece of rows (FusedNet.pushforward): the K tangents of a sample ride in K
    columns of its tile beside its value column, as the probes of ``solve_hutchinson`` do, K <= 15.  Rows are cut by that
    function's rule (a [rows, K, D] device buffer stays under ``PROBE_BUFFER_FLOATS`` floats); rows are independent, so the
    result is bitwise the same for any cut.

    Refused with ValueError before the device is touched: adaptive methods (the step control would have to be
    differentiated too), ``grid_constructor`` / ``perturb``, K > 15, shapes that do not match, ``precision`` other than
    f32.  NotImplementedError: a network outside the push-forward units, or a ``model=`` module (there is no module-path
    fallback).  Out of scope: parameter gradients and torch.autograd integration, Euler-Maruyama, sharded entry points
    (rows are independent: slice), split precision, activations other than SiLU."""
    if method in solvers.ALL_ADAPTIVE or method in solvers.ADAPTIVE_METHODS:
        raise ValueError(f"flow-map sensitivities with the adaptive method={method!r}: the tangents ride through the steps of a "
                         "fixed grid (an adaptive solve would have to differentiate its step control); use method=\"rk4\" / "
                         "\"dopri5_fixed\" with options={\"step_size\": h}")
    solvers.resolve_method(method)
    for name in ("grid_constructor", "perturb"):
        if (options or {}).get(name) not in (None, False):
            raise ValueError(f"flow-map sensitivities with options[{name!r}]: the grid is the uniform one of "
                             "options={\"step_size\": h} (or the nodes of t_span)")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("flow-map sensitivities: x must be a [batch, dim] tensor")
    B, D = int(x.shape[0]), int(x.shape[1])
    prec = getattr(front, "precision", "f32")
    if prec != "f32":
        raise ValueError(f"flow-map sensitivities with precision={prec!r}: the push-forward kernels compute in f32; use "
                         "precision='f32'")
    try:
        net = front._net()                  # (a ``model=`` module that is not the library's MLP raises here)
        plan = net.push_plan()
    except NotImplementedError as e:
        msg = str(e)
        raise NotImplementedError(msg if _native.PUSH_ENVELOPE in msg else
                                  f"{msg} -- {_native.PUSH_ENVELOPE}; there is no module-path fallback") from None
    if D != net.dim:
        raise ValueError(f"flow-map sensitivities: x has {D} columns, the model has {net.dim} dimensions")
    C = net.cond_dim
    if C > 0 and (cond is None or cond.dim() != 2 or tuple(cond.shape) != (B, C)):
        raise ValueError(f"flow-map sensitivities: conditional must be [{B}, {C}], got "
                         f"{None if cond is None else tuple(cond.shape)}")
    if C == 0 and (cond is not None or cond_tangents is not None):
        raise ValueError("flow-map sensitivities: this model has no conditional inputs")
    if unit is not None:
        if tangents is not None or cond_tangents is not None:
            raise ValueError("flow-map sensitivities: unit tangents take no tangent tensors")
        first, K = int(unit[0]), int(unit[1])
        if first < 0 or K < 1 or first + K > D + C:
            raise ValueError(f"flow-map sensitivities: unit tangents [{first}, {first + K}) outside [0, {D + C})")
    else:
        if tangents is None and cond_tangents is None:
            raise ValueError("flow-map sensitivities: tangents [batch, K, dim] and / or conditional_tangents [batch, K, cond_dim]")
        given = tangents if tangents is not None else cond_tangents
        if given.dim() != 3:
            raise ValueError(f"flow-map sensitivities: tangents must be [batch, K, dim], got {tuple(given.shape)}")
        K = int(given.shape[1])
        if tangents is not None and tuple(tangents.shape) != (B, K, D):
            raise ValueError(f"flow-map sensitivities: tangents has shape {tuple(tangents.shape)}, expected {(B, K, D)}")
        if cond_tangents is not None and tuple(cond_tangents.shape) != (B, K, C):
            raise ValueError(f"flow-map sensitivities: conditional_tangents has shape {tuple(cond_tangents.shape)}, "
                             f"expected {(B, K, C)}")
        if K < 1:
            raise ValueError("flow-map sensitivities: at least one tangent per sample")
    if K > _native.MAX_PUSH_TANGENTS or K + 1 > int(plan.tile):
        raise ValueError(f"flow-map sensitivities: K={K} tangents per sample; a sample and its tangents share the "
                         f"{int(plan.tile)} columns of one tile, so at most {_native.MAX_PUSH_TANGENTS} per call (flow_jacobian "
                         "makes as many calls as it needs)")
    require_fp32(front, x, cond, tangents, cond_tangents, what="a flow-map sensitivity solve")
    _need_gpu(x)
    if tangent_gain is not None:
        x = x * tangent_gain
        tangents = None if tangents is None else tangents * tangent_gain
    if cond_tangent_scale is not None and cond_tangents is not None:
        cond_tangents = cond_tangents / cond_tangent_scale
    tab = solvers.plan_ode(t_span, method, options)          # (rows of a fixed-grid ODE method: none carries a noise flag)
    width = int(plan.width)
    key = ("push", tuple(float(v) for v in t_span), method, repr(sorted((options or {}).items()))) + front._schedule_key()
    table = net.cached_table(key, x.device, lambda: solvers.build_table(tab, *front._host_schedule()(tab.t_eval), width))
    rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * D))
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    ys, dys = [], []
    for r0, r1 in pieces:
        y, dy, _ = net.pushforward(cut(x, r0, r1), table, tangents=cut(tangents, r0, r1), cond=cut(cond, r0, r1),
                                   cond_tangents=cut(cond_tangents, r0, r1), unit=None if unit is None else (first, K),
                                   in_shift=in_shift, in_scale=in_scale, out_scale=out_scale, out_shift=out_shift,
                                   stage_slots=solvers.resolve_method(method).stages)
        ys.append(y)
        dys.append(dy)
    return (ys[0], dys[0]) if whole else (torch.cat(ys), torch.cat(dys))


def solve_push_jacobian(front, x, t_span, method, options, cond=None, tangent_gain=None, cond_tangent_scale=None, **maps):
    """The whole Jacobian of the flow map from ``solve_push`` with unit tangents: ``(y [B, D], J_x [B, D, D], J_c [B, D, C]
    or None)``, ``J_x[b, i, j] = d y_i / d x_j``, ``J_c[b, i, j] = d y_i / d cond_j``, in ceil((D + C) / 15) launches per piece
    of rows; ``y`` is the first launch's (every launch computes the same one, bit for bit).  ``tangent_gain`` /
    ``cond_tangent_scale``: as in ``solve_push`` (the start is ``x * tangent_gain``), and applied to the columns of the
    result (the chain rule's factors)."""
    D = int(x.shape[1]) if torch.is_tensor(x) and x.dim() == 2 else 0
    C = 0 if cond is None else int(cond.shape[-1])
    y, cols = None, []
    for first in range(0, max(D + C, 1), _native.MAX_PUSH_TANGENTS):
        yk, dy = solve_push(front, x, t_span, method, options, cond=cond,
                            unit=(first, min(_native.MAX_PUSH_TANGENTS, D + C - first)), **maps)
        y = yk if y is None else y
        cols.append(dy)
    J = torch.cat(cols, dim=1).transpose(1, 2).contiguous()          # [B, D, D + C]: column j = the derivative along unit j
    Jx, Jc = J[:, :, :D].contiguous(), (J[:, :, D:].contiguous() if C > 0 else None)
    if tangent_gain is not None:
        Jx = Jx * tangent_gain
    if cond_tangent_scale is not None and Jc is not None:
        Jc = Jc / cond_tangent_scale
    return y, Jx, Jc


def _pull_checks(front, x, method, options, cotangents, cond, what="flow-map pull-backs", tile_limit=True):
    """What ``solve_pull`` and ``solve_pull_discrete`` refuse, in one order and with one set of messages, before the device is
    touched; returns ``(net, plan, B, D, K, C)``.  ``solve_logp_grad`` refuses the same, under its own name ``what``; its K
    probes are rows of their own, not columns of a tile (``tile_limit=False``)."""
    if method in solvers.ALL_ADAPTIVE or method in solvers.ADAPTIVE_METHODS:
        raise ValueError(f"{what} with the adaptive method={method!r}: the adjoint sweep runs over the reversed "
                         "fixed grid of the forward solve; use method=\"rk4\" / \"dopri5_fixed\" with "
                         "options={\"step_size\": h}")
    solvers.resolve_method(method)
    for name in ("grid_constructor", "perturb"):
        if (options or {}).get(name) not in (None, False):
            raise ValueError(f"{what} with options[{name!r}]: the grid is the uniform one of "
                             "options={\"step_size\": h} (or the nodes of t_span)")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a [batch, dim] tensor")
    B, D = int(x.shape[0]), int(x.shape[1])
    prec = getattr(front, "precision", "f32")
    if prec != "f32":
        raise ValueError(f"{what} with precision={prec!r}: the pull-back kernels compute in f32; use "
                         "precision='f32'")
    if not torch.is_tensor(cotangents) or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, D) or cotangents.shape[1] < 1:
        raise ValueError(f"{what}: cotangents must be [{B}, K >= 1, {D}], got "
                         f"{tuple(cotangents.shape) if torch.is_tensor(cotangents) else type(cotangents).__name__}")
    K = int(cotangents.shape[1])
    if tile_limit and K > _native.MAX_PULL_COTANGENTS:
        raise ValueError(f"{what}: K={K} cotangents per sample; a sample and its cotangents share the 16 columns "
                         f"of one tile, so at most {_native.MAX_PULL_COTANGENTS} per call")
    try:
        net = front._net()                  # (a ``model=`` module that is not the library's MLP raises here)
        plan = net.pull_plan()
    except NotImplementedError as e:
        msg = str(e)
        raise NotImplementedError(msg if _native.PULL_ENVELOPE in msg else
                                  f"{msg} -- {_native.PULL_ENVELOPE}; there is no module-path fallback") from None
    if D != net.dim:
        raise ValueError(f"{what}: x has {D} columns, the model has {net.dim} dimensions")
    C = net.cond_dim
    if C > 0 and (cond is None or cond.dim() != 2 or tuple(cond.shape) != (B, C)):
        raise ValueError(f"{what}: conditional must be [{B}, {C}], got "
                         f"{None if cond is None else tuple(cond.shape)}")
    if C == 0 and cond is not None:
        raise ValueError(f"{what}: this model has no conditional inputs")
    require_fp32(front, x, cond, cotangents, what="a flow-map pull-back solve" if tile_limit else "a log-density gradient solve")
    _need_gpu(x)
    return net, plan, B, D, K, C


def solve_pull(front, x, t_span, method, options, cotangents, cond=None, in_shift=None, in_scale=None, out_scale=None,
               out_shift=None, tangent_gain=None, cond_tangent_scale=None, return_retrace=False):
    """Flow-map pull-backs (extension): K cotangents per sample pulled back through the fixed-grid solve of ``solve`` in
    MODE_STATE, by the CONTINUOUS adjoint, as torchdiffeq's ``odeint_adjoint`` does.  Returns ``(y [B, D], gx [B, K, D],
    gc [B, K, C] or None)`` -- and ``retrace [B]`` with ``return_retrace`` -- where ``gx[b, k] = cotangents[b, k]^T d y[b] /
    d x[b]`` and ``gc`` likewise for ``cond`` (times ``1 / cond_tangent_scale``: the caller's raw conditional).

    Two launches per piece of rows: the ordinary state-only solve ``x -> y`` (``y`` is bitwise what ``solve`` returns), then
    ONE launch of a pull-back unit (FusedNet.pullback) over the REVERSED span, same method and step, on the augmented state
    ``[y | alpha_k | gamma_k]`` from ``[y, w_k, 0]``: ``dalpha/dt = -(df/dy)^T alpha``, ``dgamma/dt = -(df/dc)^T alpha``.
    This is NOT the transpose of the discrete map ``solve_push`` differentiates: the two differ by the discretisation
    error of the method (order p in the step), and the backward sweep retraces ``y`` instead of storing it.
    ``retrace[b] = max_d |y_back - x|`` in the units of ``x`` says how far the retraced trajectory ended from where the
    forward one began: read it, use rk4 or better, and raise the step count until it is small.  (An Euler sweep of a VP
    score model with 128 steps retraces to 0.4 and its gradient is off by 0.7; rk4 with 128 steps is off by 4e-6.)

    The affine maps are those of the forward solve, as in ``solve_push``; ``tangent_gain``: the solve starts from
    ``x * tangent_gain`` (a VE model's sigma_max), and ``gx`` carries the factor.  Rows are cut so that a [rows, K, D]
    device buffer stays under ``PROBE_BUFFER_FLOATS`` floats; rows are independent, so any cut gives bitwise the same.

    Refused with ValueError before the device is touched: adaptive methods, ``grid_constructor`` / ``perturb``, K > 15,
    shapes that do not match, ``precision`` other than f32.  NotImplementedError: a network outside the pull-back units
    (``_native.PULL_ENVELOPE``), or a ``model=`` module.  Out of scope: parameter gradients and torch.autograd
    integration, adaptive control, sharded entry points.  The exact discrete adjoint is ``solve_pull_discrete``."""
    net, plan, B, D, K, C = _pull_checks(front, x, method, options, cotangents, cond)
    x0 = x if tangent_gain is None else x * tangent_gain
    y, _ = solve(front, x0, t_span, method, options, MODE_STATE, 0.0, 0.0, cond=cond, in_shift=in_shift, in_scale=in_scale,
                 out_scale=out_scale, out_shift=out_shift)
    t_back = torch.flip(torch.as_tensor(t_span), dims=(0,))
    tab = solvers.plan_ode(t_back, method, options)           # (rows of a fixed-grid ODE method: none carries a noise flag)
    width = int(plan.width)
    key = ("pull", tuple(float(v) for v in t_back), method, repr(sorted((options or {}).items()))) + front._schedule_key()
    table = net.cached_table(key, x.device, lambda: solvers.build_table(tab, *front._host_schedule()(tab.t_eval), width))
    rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * D))
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    backs, gxs, gcs = [], [], []
    for r0, r1 in pieces:
        # the backward launch's maps: undo the forward solve's output map on the way in, redo its input map on the way out
        yb, gx, gc, _ = net.pullback(cut(y, r0, r1), table, cut(cotangents, r0, r1), cond=cut(cond, r0, r1), want_cond=C > 0,
                                     in_shift=out_shift, in_scale=out_scale, out_scale=in_scale, out_shift=in_shift,
                                     stage_slots=solvers.resolve_method(method).stages)
        backs.append(yb)
        gxs.append(gx)
        gcs.append(gc)
    yb, gx = (backs[0], gxs[0]) if whole else (torch.cat(backs), torch.cat(gxs))
    gc = None if C == 0 else (gcs[0] if whole else torch.cat(gcs))
    if tangent_gain is not None:
        gx = gx * tangent_gain
        yb = yb / tangent_gain
    if cond_tangent_scale is not None and gc is not None:
        gc = gc / cond_tangent_scale
    if not return_retrace:
        return y, gx, gc
    return y, gx, gc, (yb - x).abs().amax(dim=1)


def discrete_piece_rows(B, K, E, D):
    """Rows per piece of ``solve_pull_discrete``: neither a [rows, K, D] buffer nor the [E, rows, D] record reaches
    ``PROBE_BUFFER_FLOATS`` floats.  Even pieces, whole tiles where the bound allows: a long piece and a short one would each
    end on a part-filled round of wavefronts (at 2^16 rows of a 400-row record, 6 + 3 rounds of the chip where two halves
    take 4 + 4)."""
    most = max(1, (PROBE_BUFFER_FLOATS - 1) // (max(K, E, 1) * D))
    rows = -(-max(B, 1) // -(-max(B, 1) // most))
    return min(most, -(-rows // 16) * 16) if most >= 16 else rows


def solve_pull_discrete(front, x, t_span, method, options, cotangents, cond=None, in_shift=None, in_scale=None, out_scale=None,
                        out_shift=None, tangent_gain=None, cond_tangent_scale=None):
    """Flow-map pull-backs by the exact DISCRETE adjoint (extension): K cotangents per sample pulled back through the
    fixed-grid solve of ``solve`` in MODE_STATE by the transpose of the map that solve applies -- the transpose of what
    ``solve_push`` differentiates, so ``<w, solve_push(v)> = <solve_pull_discrete(w), v>`` up to rounding at ANY step
    count, one Euler step included.  Returns ``(y [B, D], gx [B, K, D], gc [B, K, C] or None)`` as ``solve_pull`` does.

    Two launches per piece of rows over the SAME forward table: the record unit (FusedNet.record) integrates ``x -> y`` and
    writes the stage state of every evaluation row down, [E, rows, D]; the discrete-adjoint unit
    (FusedNet.pullback_discrete) runs the transposed row program from the last row to the first on those states.  Nothing
    is retraced: there is no ``retrace`` to read.  ``y`` is the record launch's state: it does not depend on K, on the
    cotangents or on the cut, and is bitwise what ``solve`` returns (the record unit runs the state kernels' fp32 chains in
    their order).

    The affine maps, ``tangent_gain`` and ``cond_tangent_scale`` are as in ``solve_pull``.  Rows are cut so that neither a
    [rows, K, D] buffer nor the [E, rows, D] record reaches ``PROBE_BUFFER_FLOATS`` floats; rows are independent, so any
    cut gives bitwise the same.  Refusals: ``solve_pull``'s, with its messages.  Out of scope: parameter gradients and
    torch.autograd integration, adaptive control, ``grid_constructor`` grids, sharded entry points."""
    net, plan, B, D, K, C = _pull_checks(front, x, method, options, cotangents, cond)
    x0 = x if tangent_gain is None else x * tangent_gain
    tab = solvers.plan_ode(t_span, method, options)          # (rows of a fixed-grid ODE method: none carries a noise flag)
    width = int(plan.width)
    key = ("pull_discrete", tuple(float(v) for v in torch.as_tensor(t_span)), method,
           repr(sorted((options or {}).items()))) + front._schedule_key()
    table = net.cached_table(key, x.device, lambda: solvers.build_table(tab, *front._host_schedule()(tab.t_eval), width))
    E = max(1, int(table.shape[0]))
    rows = discrete_piece_rows(B, K, E, D)
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    slots = solvers.resolve_method(method).stages
    ys, gxs, gcs = [], [], []
    for r0, r1 in pieces:
        maps = dict(in_shift=in_shift, in_scale=in_scale, out_scale=out_scale, out_shift=out_shift)
        yp, rec, _ = net.record(cut(x0, r0, r1), table, cond=cut(cond, r0, r1), stage_slots=slots, **maps)
        gx, gc, _ = net.pullback_discrete(rec, table, cut(cotangents, r0, r1), cond=cut(cond, r0, r1), want_cond=C > 0,
                                          stage_slots=slots, **maps)
        del rec
        ys.append(yp)
        gxs.append(gx)
        gcs.append(gc)
    y, gx = (ys[0], gxs[0]) if whole else (torch.cat(ys), torch.cat(gxs))
    gc = None if C == 0 else (gcs[0] if whole else torch.cat(gcs))
    if tangent_gain is not None:
        gx = gx * tangent_gain
    if cond_tangent_scale is not None and gc is not None:
        gc = gc / cond_tangent_scale
    return y, gx, gc


def solve_pull_by(adjoint, front, x, t_span, method, options, cotangents, return_retrace=False, **kw):
    """``flow_vjp``'s choice of route: ``adjoint="continuous"`` is ``solve_pull``, ``"discrete"`` ``solve_pull_discrete``
    (which retraces nothing: ``return_retrace`` raises); anything else raises ValueError."""
    if adjoint == "continuous":
        return solve_pull(front, x, t_span, method, options, cotangents, return_retrace=return_retrace, **kw)
    if adjoint != "discrete":
        raise ValueError(f"flow-map pull-backs: adjoint={adjoint!r}; \"continuous\" (the adjoint ODE over the reversed grid) or "
                         "\"discrete\" (the transpose of the discrete solver map, from recorded stage states)")
    if return_retrace:
        raise ValueError("flow-map pull-backs: return_retrace with adjoint=\"discrete\": the discrete adjoint reads recorded "
                         "stage states and retraces nothing")
    return solve_pull_discrete(front, x, t_span, method, options, cotangents, **kw)


def check_logp_grad(front, x, method, options, cond):
    """The refusals of ``solve_logp_grad`` that need no probes: the front ends call it before the value solve, so that a
    ``log_prob_grad`` that cannot run raises before the device is touched."""
    stand_in = x.unsqueeze(1) if torch.is_tensor(x) and x.dim() == 2 else None       # (a view: the probes' shape, no device work)
    _pull_checks(front, x, method, options, stand_in, cond, what="log-density gradients", tile_limit=False)


def solve_logp_grad(front, x, t_span, method, options, probes, probe_weight, cond=None, in_shift=None, in_scale=None,
                    cond_tangent_scale=None, prior_grad=None):
    """Log-density gradients (extension): the gradient of the fixed-grid Hutchinson log-density
    ``sum_k probe_weight * lp(x, cond; probes[:, k]) + log prior(y)`` with respect to ``x`` and ``cond`` at FIXED probes, by
    the exact discrete adjoint with the divergence integral in it (csrc/ff_mlp_lgrad.hpp) -- reverse mode over the
    forward-mode tangent, so exact for the discrete sum that ``solve`` in MODE_HUTCH evaluates, at any step count.  Returns
    ``(y [B, D], gx [B, D], gc [B, C] or None)``.  ``probes`` [B, K, D]: K >= 1 probes per point, every one a row of its own
    (the kernel carries two columns per row: no tile limit on K); ``probe_weight``: 1 / K for a probe average, 1 for the D
    unit probes of an exact trace.  ``prior_grad(y)``: the gradient of the log prior at the final state (default ``-y``: a
    standard normal).

    Per piece of rows, cut by ``discrete_piece_rows`` on the expanded B K rows (whole points): the record launch on the
    repeated rows, the prior's gradient at its state as the final cotangent of replica 0 of each point (zero on the
    others), ONE launch of the log-density gradient unit (FusedNet.logp_grad), and the sum over a point's K replicas in the
    order k = 0 .. K - 1.  Rows are independent, so any cut gives bitwise the same.  ``y`` is the record launch's state:
    bitwise the fixed-grid solve's.  The affine input map and ``cond_tangent_scale`` are as in ``solve_pull_discrete``.

    Refusals: ``_pull_checks``', under the name "log-density gradients".  Out of scope: parameter gradients and
    torch.autograd integration, adaptive control, a multi-probe column layout, twins, split precision, non-SiLU units, a
    module-path fallback, sharded entry points (rows are independent: slice).  The gradient of ``log_prob_noisy`` is
    ``log_prob_noisy_grad`` below, around this function."""
    net, plan, B, D, K, C = _pull_checks(front, x, method, options, probes, cond, what="log-density gradients", tile_limit=False)
    tab = solvers.plan_ode(t_span, method, options)          # (rows of a fixed-grid ODE method: none carries a noise flag)
    width = int(plan.width)
    key = ("pull_discrete", tuple(float(v) for v in torch.as_tensor(t_span)), method,
           repr(sorted((options or {}).items()))) + front._schedule_key()
    table = net.cached_table(key, x.device, lambda: solvers.build_table(tab, *front._host_schedule()(tab.t_eval), width))
    E = max(1, int(table.shape[0]))
    points = max(1, discrete_piece_rows(B * K, 1, E, D) // K)
    pieces = [(r0, min(B, r0 + points)) for r0 in range(0, B, points)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    rep = lambda t: t if (t is None or K == 1) else t.repeat_interleave(K, dim=0)
    slots = solvers.resolve_method(method).stages
    maps = dict(in_shift=in_shift, in_scale=in_scale)
    ys, gxs, gcs = [], [], []
    for r0, r1 in pieces:
        n = r1 - r0
        ck = rep(cut(cond, r0, r1))
        yp, rec, _ = net.record(rep(cut(x, r0, r1)), table, cond=ck, stage_slots=slots, **maps)
        y0 = yp if K == 1 else yp[::K].contiguous()
        cot = torch.zeros(n * K, D, dtype=torch.float32, device=x.device)
        cot[::K] = -y0 if prior_grad is None else prior_grad(y0)
        weight = torch.full((n * K,), float(probe_weight), dtype=torch.float32, device=x.device)
        gx, gc, _ = net.logp_grad(rec, table, cut(probes, r0, r1).reshape(n * K, D), cot, weight, cond=ck, want_cond=C > 0,
                                  stage_slots=slots, **maps)
        del rec
        gx, gc = gx.view(n, K, D), (None if gc is None else gc.view(n, K, C))
        sx, sc = gx[:, 0].clone(), (None if gc is None else gc[:, 0].clone())
        for k in range(1, K):                   # a fixed order: the sum does not depend on the cut
            sx += gx[:, k]
            if sc is not None:
                sc += gc[:, k]
        ys.append(y0)
        gxs.append(sx)
        gcs.append(sc)
    y, gx = (ys[0], gxs[0]) if whole else (torch.cat(ys), torch.cat(gxs))
    gc = None if C == 0 else (gcs[0] if whole else torch.cat(gcs))
    if cond_tangent_scale is not None and gc is not None:
        gc = gc / cond_tangent_scale
    return y, gx, gc


def solve_leapfrog(front, x, grid, cond=None):
    """Kick-drift-kick leapfrog of a separable front end (symplectic.py) over the nodes ``grid``; returns the state
    [B, 2D] and sets ``front.last_solver_stats``.  Compiled shapes: ONE fused launch of the row-select kernel on the table
    of ``solvers.plan_leapfrog``.  Everything else: the same rows stepped by the library around torch (generic.py), one
    network -- or the needed half of a foreign module's output -- per row."""
    require_fp32(front, x, cond, what="an ODE solve")
    if front._fusable():
        net = front._net()
        key = ("leapfrog", tuple(float(v) for v in grid)) + front._schedule_key()
        table = net.cached_table(key, x.device, lambda: front._leapfrog_table(grid))
        y, _, _ = net.integrate_select(x, table, cond=cond)
        front.last_solver_stats = {"evaluations": int(table.shape[0]), "launches": 1}
        return y
    _need_gpu(x)
    stepper = ModuleStepper(front._module_half_rhs(cond), False)
    y = stepper.run_leapfrog(x, solvers.plan_leapfrog(grid))
    front.last_solver_stats = {"evaluations": stepper.n_evals}
    return y


def _leapfrog_pull_checks(front, z, cotangents, cond, num_cotangents):
    """What ``solve_leapfrog_pull`` refuses before the device is touched, in ``_pull_checks``' style: shapes, K, dtypes,
    CPU tensors, the envelope.  Returns ``(net, B, D2, K, C)``."""
    what = "leapfrog pull-backs"
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] % 2 != 0 or z.shape[1] < 2:
        raise ValueError(f"{what}: z must be a [batch, 2 dim] tensor, the joint state [q | p]")
    B, D2 = int(z.shape[0]), int(z.shape[1])
    if callable(cotangents):
        K = int(num_cotangents)
        if K < 1:
            raise ValueError(f"{what}: num_cotangents={num_cotangents}: at least one cotangent per sample")
    else:
        if not torch.is_tensor(cotangents) or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, D2) or cotangents.shape[1] < 1:
            raise ValueError(f"{what}: cotangents must be [{B}, K >= 1, {D2}], got "
                             f"{tuple(cotangents.shape) if torch.is_tensor(cotangents) else type(cotangents).__name__}")
        K = int(cotangents.shape[1])
    if K > _native.MAX_PULL_COTANGENTS:
        raise ValueError(f"{what}: K={K} cotangents per sample; a sample and its cotangents share the 16 columns "
                         f"of one tile, so at most {_native.MAX_PULL_COTANGENTS} per call")
    if cond is not None and (not torch.is_tensor(cond) or cond.dim() != 2 or cond.shape[0] != B):
        raise ValueError(f"{what}: conditional must be [{B}, cond_dim], got "
                         f"{tuple(cond.shape) if torch.is_tensor(cond) else type(cond).__name__}")
    require_fp32(front, z, cond, None if callable(cotangents) else cotangents, what="a leapfrog pull-back solve")
    _need_gpu(z)
    try:
        if not front._fusable():
            raise NotImplementedError("the model's two networks are outside the compiled two-network shapes (or not a SymplecticMLP "
                                      "with SiLU)")
        net = front._net()
        net.pull_select_plan()
    except NotImplementedError as e:
        msg = str(e)
        raise NotImplementedError(msg if _native.PULL_SELECT_ENVELOPE in msg else
                                  f"{msg} -- {_native.PULL_SELECT_ENVELOPE}; there is no module-path fallback") from None
    if D2 != net.dim:
        raise ValueError(f"{what}: z has {D2} columns, the model's joint state has {net.dim}")
    C = net.cond_dim
    if C > 0 and (cond is None or tuple(cond.shape) != (B, C)):
        raise ValueError(f"{what}: conditional must be [{B}, {C}], got {None if cond is None else tuple(cond.shape)}")
    if C == 0 and cond is not None:
        raise ValueError(f"{what}: this model has no conditional inputs")
    return net, B, D2, K, C


def solve_leapfrog_pull(front, z, grid, cotangents, cond=None, return_retrace=False):
    """Leapfrog pull-backs (extension): K cotangents per sample pulled back through ``solve_leapfrog(front, z, grid, cond)``,
    exactly.  Returns ``(z_out [B, 2D], gz [B, K, 2D], gc [B, K, C] or None)`` -- and ``retrace [B]`` with ``return_retrace``
    -- where ``gz[b, k] = cotangents[b, k]^T d z_out[b] / d z[b]`` and ``gc`` likewise for ``cond`` as given.

    A leapfrog row is a shear ``q' = q + w f(p, c, t)``, ``p' = p`` (or the kick, its mirror image); its transpose is
    ``lambda_q = lambda_q'``, ``lambda_p = lambda_p' + w J_f(p)^T lambda_q'``, ``gamma += w (df/dc)^T lambda_q'``.  The row
    leaves the network's input half alone, so the backward sweep recomputes ``f(p)`` from the state it holds, un-shears, and
    takes the slopes for ``J^T`` from that same evaluation: the retracing sweep IS the discrete adjoint, and no stage state
    is recorded.  Per piece of rows: ``solve_leapfrog`` for ``z_out`` (the existing launch: bitwise what ``sample_leapfrog`` /
    ``log_prob_leapfrog`` see), then ONE launch of the row-select pull-back unit (``FusedPair.pullback_select``) from
    ``z_out`` on the table of ``solvers.plan_leapfrog(grid.flip(0))``, which holds bitwise the forward table's times and
    weights in reverse order.  Rows are cut so that a [rows, K, 2D] buffer stays under ``PROBE_BUFFER_FLOATS`` floats; rows
    are independent, so any cut gives bitwise the same.

    ``cotangents``: [B, K, 2D].  ``retrace[b] = max_d |z_back - z|``: within rounding by construction (the
    un-shear subtracts what the forward row added, recomputed from the same input half); it exists to show a non-finite or
    exploding trajectory.

    Refused before the device is touched: shapes that do not match and K > 15 (ValueError), non-fp32 tensors (TypeError), CPU
    tensors (RuntimeError), a model outside ``_native.PULL_SELECT_ENVELOPE`` or not on the fused route
    (NotImplementedError: there is no module-path fallback).  Out of scope: parameter gradients and torch.autograd
    integration, Euler and dopri5 solves (not shears: they need a record), twins, sharded entry points (rows are
    independent: slice)."""
    if callable(cotangents):
        raise ValueError("leapfrog pull-backs: cotangents must be a [batch, K, 2 dim] tensor")
    return _solve_leapfrog_pull(front, z, grid, cotangents, cond, return_retrace, 1)


def _leapfrog_pull_from(front, z_out, grid, cotangents, cond):
    """The backward half of ``_solve_leapfrog_pull``, for a caller that already holds ``z_out`` = ``solve_leapfrog(front, z,
    grid, cond)`` [n, 2D] (``log_prob_marginal_grad``: its one forward solve serves the weights and this): the pull-back of
    ``cotangents`` [n, K, 2D] from ``z_out`` by ``FusedPair.pullback_select`` on the table of the flipped grid -- under
    ``_solve_leapfrog_pull``'s cache key, its rows cut by the same rule under ``PROBE_BUFFER_FLOATS``.  Returns ``(z_back [n,
    2D], gz [n, K, 2D], gc [n, K, C] or None)`` and sets ``front.last_solver_stats`` to this half's ``evaluations`` and
    ``launches``.  Checks nothing: ``_leapfrog_pull_checks`` is the caller's."""
    net = front._net()
    n, K, D2 = (int(v) for v in cotangents.shape)
    C = net.cond_dim
    grid = torch.as_tensor(grid).detach().to("cpu", torch.float32).reshape(-1)
    back = torch.flip(grid, dims=(0,))
    key = ("leapfrog_pull", tuple(float(v) for v in back)) + front._schedule_key()
    table = net.cached_table(key, z_out.device, lambda: front._leapfrog_table(back, pull_select=True))
    rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * D2))
    pieces = [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    backs, gzs, gcs = [], [], []
    for r0, r1 in pieces:
        zb, gz, gc, _ = net.pullback_select(cut(z_out, r0, r1), table, cut(cotangents, r0, r1), cond=cut(cond, r0, r1),
                                            want_cond=C > 0, stage_slots=1)
        backs.append(zb)
        gzs.append(gz)
        gcs.append(gc)
    front.last_solver_stats = {"evaluations": int(table.shape[0]), "launches": len(pieces)}
    zb, gz = (backs[0], gzs[0]) if whole else (torch.cat(backs), torch.cat(gzs))
    return zb, gz, (None if C == 0 else (gcs[0] if whole else torch.cat(gcs)))


def _solve_leapfrog_pull(front, z, grid, cotangents, cond, return_retrace, num_cotangents):
    """``solve_leapfrog_pull`` whose ``cotangents`` may also be a function ``z_out piece [rows, 2D] -> [rows, num_cotangents,
    2D]``, evaluated per piece of rows between the two launches: how ``log_prob_leapfrog_grad`` hands over ``-z1``."""
    net, B, D2, K, C = _leapfrog_pull_checks(front, z, cotangents, cond, num_cotangents)
    grid = torch.as_tensor(grid).detach().to("cpu", torch.float32).reshape(-1)
    rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * D2))
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    outs, backs, gzs, gcs = [], [], [], []
    evals = 0
    for r0, r1 in pieces:
        zo = solve_leapfrog(front, cut(z, r0, r1), grid, cond=cut(cond, r0, r1))
        evals = front.last_solver_stats["evaluations"]
        w = cotangents(zo) if callable(cotangents) else cut(cotangents, r0, r1)
        if callable(cotangents) and (w.dim() != 3 or tuple(w.shape) != (r1 - r0, K, D2)):
            raise ValueError(f"leapfrog pull-backs: the cotangent function returned {tuple(w.shape)}, expected {(r1 - r0, K, D2)}")
        zb, gz, gc = _leapfrog_pull_from(front, zo, grid, w, cut(cond, r0, r1))        # (a piece is within its cut: one launch)
        evals += front.last_solver_stats["evaluations"]
        outs.append(zo)
        backs.append(zb)
        gzs.append(gz)
        gcs.append(gc)
    front.last_solver_stats = {"evaluations": evals, "launches": 2 * len(pieces)}
    zo, zb, gz = (outs[0], backs[0], gzs[0]) if whole else (torch.cat(outs), torch.cat(backs), torch.cat(gzs))
    gc = None if C == 0 else (gcs[0] if whole else torch.cat(gcs))
    if not return_retrace:
        return zo, gz, gc
    return zo, gz, gc, (zb - z).abs().amax(dim=1)


def _leapfrog_push_checks(front, z, tangents, cond, cond_tangents, unit):
    """What ``solve_leapfrog_push`` refuses before the device is touched, in ``_leapfrog_pull_checks``' style and order:
    shapes, the tangents and K, dtypes, CPU tensors, the envelope, the conditional against the model.  Returns
    ``(net, B, D2, K, C)``."""
    what = "leapfrog push-forwards"
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] % 2 != 0 or z.shape[1] < 2:
        raise ValueError(f"{what}: z must be a [batch, 2 dim] tensor, the joint state [q | p]")
    B, D2 = int(z.shape[0]), int(z.shape[1])
    shape_of = lambda t: tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
    if cond is not None and (not torch.is_tensor(cond) or cond.dim() != 2 or cond.shape[0] != B):
        raise ValueError(f"{what}: conditional must be [{B}, cond_dim], got {shape_of(cond)}")
    if tangents is not None and (not torch.is_tensor(tangents) or tangents.dim() != 3 or tuple(tangents.shape[::2]) != (B, D2)):
        raise ValueError(f"{what}: tangents must be [{B}, K >= 1, {D2}], got {shape_of(tangents)}")
    if cond_tangents is not None and (not torch.is_tensor(cond_tangents) or cond_tangents.dim() != 3 or cond is None or
                                      tuple(cond_tangents.shape[::2]) != (B, int(cond.shape[1]))):
        raise ValueError(f"{what}: conditional_tangents must be [{B}, K >= 1, cond_dim] beside a conditional, got "
                         f"{shape_of(cond_tangents)}")
    if tangents is not None and cond_tangents is not None and tangents.shape[1] != cond_tangents.shape[1]:
        raise ValueError(f"{what}: tangents and conditional_tangents hold {tangents.shape[1]} and {cond_tangents.shape[1]} "
                         "tangents per sample")
    if unit is not None:
        if tangents is not None or cond_tangents is not None:
            raise ValueError(f"{what}: unit tangents take no tangent tensors")
        first, K = int(unit[0]), int(unit[1])
        span = D2 + (0 if cond is None else int(cond.shape[1]))
        if first < 0 or K < 1 or first + K > span:
            raise ValueError(f"{what}: unit tangents [{first}, {first + K}) outside [0, {span})")
    else:
        if tangents is None and cond_tangents is None:
            raise ValueError(f"{what}: tangents [batch, K, 2 dim] and / or conditional_tangents [batch, K, cond_dim]")
        K = int((tangents if tangents is not None else cond_tangents).shape[1])
        if K < 1:
            raise ValueError(f"{what}: at least one tangent per sample")
    if K > _native.MAX_PUSH_TANGENTS:
        raise ValueError(f"{what}: K={K} tangents per sample; a sample and its tangents share the 16 columns "
                         f"of one tile, so at most {_native.MAX_PUSH_TANGENTS} per call")
    require_fp32(front, z, cond, tangents, cond_tangents, what="a leapfrog push-forward solve")
    _need_gpu(z)
    try:
        if not front._fusable():
            raise NotImplementedError("the model's two networks are outside the compiled two-network shapes (or not a SymplecticMLP "
                                      "with SiLU)")
        net = front._net()
        net.push_select_plan()
    except NotImplementedError as e:
        msg = str(e)
        raise NotImplementedError(msg if _native.PUSH_SELECT_ENVELOPE in msg else
                                  f"{msg} -- {_native.PUSH_SELECT_ENVELOPE}; there is no module-path fallback") from None
    if D2 != net.dim:
        raise ValueError(f"{what}: z has {D2} columns, the model's joint state has {net.dim}")
    C = net.cond_dim
    if C > 0 and (cond is None or tuple(cond.shape) != (B, C)):
        raise ValueError(f"{what}: conditional must be [{B}, {C}], got {None if cond is None else tuple(cond.shape)}")
    if C == 0 and cond is not None:
        raise ValueError(f"{what}: this model has no conditional inputs")
    return net, B, D2, K, C


def solve_leapfrog_push(front, z, grid, tangents=None, cond=None, cond_tangents=None, unit=None):
    """Leapfrog push-forwards (extension): K tangents per sample pushed through ``solve_leapfrog(front, z, grid, cond)``,
    exactly.  Returns ``(z_out [B, 2D], dz [B, K, 2D])`` with ``dz[b, k] = d z_out[b] / d (z[b], cond[b]) . (tangents[b, k],
    cond_tangents[b, k])`` -- forward mode through the SAME shears, so the derivative of the discrete leapfrog map on ANY
    leapfrog grid: ``linspace(1, 0, n + 1)`` is the sampler's direction, its flip the log-density's.  ``tangents``
    [B, K, 2D] / ``cond_tangents`` [B, K, C]: either may be None (zero); ``unit = (first, count)`` instead of both: the unit
    vectors ``first .. first + count - 1`` of the combined space [0, 2D + C).  ``cond`` and ``cond_tangents`` are the
    networks' (normalised) conditional inputs.

    A leapfrog row is a shear ``q' = q + w f(p, c, t)``, ``p' = p`` (or the kick, its mirror image); its forward-mode form
    is ``dq' = dq + w (J_f(p) dp + df/dc dc)``, ``dp' = dp``.  ONE launch of the row-select push-forward unit per piece of rows
    (``FusedPair.pushforward_select``) on the table of ``solvers.plan_leapfrog(grid)`` at that unit's row width: the K
    tangents of a sample ride in K columns of its tile beside its value column, K <= 15, and nothing is stashed, so there is
    no depth ceiling.  ``z_out`` is bitwise ``solve_leapfrog``'s: the value column runs the row-select kernel's FMA chains
    wherever that kernel works on the 16-column tile; for the networks it serves on its 32-column tile (hidden widths up to
    64) ``z_out`` comes from a ``solve_leapfrog`` launch of its own.  Rows are cut by ``solve_push``'s rule (a [rows, K, 2D]
    buffer stays under ``PROBE_BUFFER_FLOATS`` floats); rows are independent, so any cut gives bitwise the same.

    Refused before the device is touched: shapes that do not match, no tangents at all and K > 15 (ValueError), non-fp32
    tensors (TypeError), CPU tensors (RuntimeError), a model outside ``_native.PUSH_SELECT_ENVELOPE`` or not on the fused
    route (NotImplementedError: there is no module-path fallback).  Out of scope: parameter gradients and torch.autograd
    integration, Euler and dopri5 solves, twins, sharded entry points (rows are independent: slice)."""
    return _solve_leapfrog_push(front, z, grid, tangents, cond, cond_tangents, unit, None)


def _solve_leapfrog_push(front, z, grid, tangents, cond, cond_tangents, unit, cond_tangent_scale):
    """``solve_leapfrog_push`` for a front end that normalised ``cond`` on the host: after the checks, ``cond_tangents /
    cond_tangent_scale`` (a tensor or None), as ``solve_push`` does."""
    net, B, D2, K, C = _leapfrog_push_checks(front, z, tangents, cond, cond_tangents, unit)
    if cond_tangent_scale is not None and cond_tangents is not None:
        cond_tangents = cond_tangents / cond_tangent_scale
    grid = torch.as_tensor(grid).detach().to("cpu", torch.float32).reshape(-1)
    key = ("leapfrog_push", tuple(float(v) for v in grid)) + front._schedule_key()
    table = net.cached_table(key, z.device, lambda: front._leapfrog_table(grid, push_select=True))
    own_state = int(net.plan(MODE_STATE, select=True).tile) == int(net.push_select_plan().tile)
    rows = max(1, (PROBE_BUFFER_FLOATS - 1) // (K * D2))
    pieces = [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)] or [(0, 0)]
    whole = len(pieces) == 1
    cut = lambda t, r0, r1: t if (whole or t is None) else t[r0:r1]
    outs, dzs = [], []
    for r0, r1 in pieces:
        zo, dz, _ = net.pushforward_select(cut(z, r0, r1), table, tangents=cut(tangents, r0, r1), cond=cut(cond, r0, r1),
                                           cond_tangents=cut(cond_tangents, r0, r1),
                                           unit=None if unit is None else (int(unit[0]), K), stage_slots=1)
        if not own_state:
            zo = solve_leapfrog(front, cut(z, r0, r1), grid, cond=cut(cond, r0, r1))
        outs.append(zo)
        dzs.append(dz)
    front.last_solver_stats = {"evaluations": int(table.shape[0]), "launches": (1 if own_state else 2) * len(pieces)}
    return (outs[0], dzs[0]) if whole else (torch.cat(outs), torch.cat(dzs))


def solve_leapfrog_push_jacobian(front, z, grid, cond=None):
    """The whole Jacobian of the leapfrog map from ``solve_leapfrog_push`` with unit tangents: ``(z_out [B, 2D], J_z
    [B, 2D, 2D], J_c [B, 2D, C] or None)``, ``J_z[b, i, j] = d z_out_i / d z_j``, ``J_c[b, i, j] = d z_out_i / d cond_j``, in
    ceil((2D + C) / 15) launches per piece of rows; ``z_out`` is the first launch's (every launch computes the same one, bit
    for bit)."""
    D2 = int(z.shape[1]) if torch.is_tensor(z) and z.dim() == 2 else 0
    C = 0 if cond is None or not torch.is_tensor(cond) or cond.dim() != 2 else int(cond.shape[1])
    zo, cols = None, []
    for first in range(0, max(D2 + C, 1), _native.MAX_PUSH_TANGENTS):
        zk, dz = solve_leapfrog_push(front, z, grid, cond=cond, unit=(first, min(_native.MAX_PUSH_TANGENTS, D2 + C - first)))
        zo = zk if zo is None else zo
        cols.append(dz)
    J = torch.cat(cols, dim=1).transpose(1, 2).contiguous()          # [B, 2D, 2D + C]: column j = the derivative along unit j
    return zo, J[:, :, :D2].contiguous(), (J[:, :, D2:].contiguous() if C > 0 else None)


# ---- extension: the log-density of noisy observations over K noise draws (the front ends' ``log_prob_noisy``) -----------
OBSERVE_CHUNK_ROWS = 1 << 22        # rows (data points x noise draws) in flight by default on a fixed grid


def noise_std_tensor(noise_std, x):
    """``noise_std`` of a ``log_prob_noisy`` as the contiguous fp32 tensor ff_observe_expand takes, on ``x``'s device: [B, D]
    or [D] as given, a Python or 0-dim scalar expanded to [D] on the host.  Finite and >= 0, else ValueError."""
    B, D = x.shape
    if torch.is_tensor(noise_std) and noise_std.dim() > 0:
        if tuple(noise_std.shape) not in ((D,), (B, D)):
            raise ValueError(f"noise_std has shape {tuple(noise_std.shape)}: [{B}, {D}] (per object and dimension), [{D}] (one "
                             "vector for every object) or a scalar")
        std = _native.f32_on(noise_std, x.device)
    else:
        std = torch.full((D,), float(noise_std), dtype=torch.float32).to(x.device)
    if not bool((torch.isfinite(std) & (std >= 0)).all()):
        raise ValueError("noise_std must be finite and >= 0 everywhere (0: that coordinate was measured exactly)")
    return std


def log_prob_noisy(log_prob_rows, randomised, x, noise_std, cond, num_draws, method, seed, sample_offset, chunk_points,
                   return_ess):
    """What every front end's ``log_prob_noisy`` does: ``log p_obs(x | noise_std) = log E_{z ~ N(0, I)} p(x - noise_std z)``
    [B] from K = ``num_draws`` draws per point (with ``return_ess`` also the effective sample size of the K weights [B]).
    Per chunk of points: ff_observe_expand writes the K rows ``x[r] - noise_std[r] * z_k`` (and repeats ``cond``), the
    model's own log-density runs on them -- ``log_prob_rows(y, cond_rows, extra)`` -> [rows] or [rows, 1], ``extra`` the
    keywords that key the probes of a ``randomised`` (Hutchinson) model by ``seed`` and the expanded GLOBAL row,
    ``probe="philox"`` with ``sample_offset = (sample_offset + lo) K``: a host draw would depend on the chunking --
    and ff_logmeanexp combines them in double.  The draws come from the counter-based stream keyed by ``seed`` and the
    global row ``sample_offset + r`` (noise indices FF_OBS_NOISE_BASE + k); ``seed=None`` draws a 63-bit one from torch's
    default generator.  On a fixed-grid ``method`` the points go through in chunks of ``chunk_points`` (default:
    ``chunk_points * K <= OBSERVE_CHUNK_ROWS``) with bitwise the same result whatever the chunking; an adaptive method
    takes its step from the whole batch, so all B K rows are one solve and ``chunk_points`` raises."""
    out, ess, _ = _observe_chunks(log_prob_rows, randomised, x, noise_std, cond, num_draws, method, seed, sample_offset,
                                  chunk_points, return_ess, None)
    return (out, ess) if return_ess else out


def _observe_args(what, x, num_draws, num_samples, method, chunk_points):
    """The checks of ``log_prob_noisy``, ``posterior_noisy`` and ``log_prob_noisy_grad`` that touch no device, and the chunk
    rule: ``(K, M or None, points per chunk)``."""
    K = int(num_draws)
    if not 1 <= K <= _native.MAX_OBS_DRAWS:
        raise ValueError(f"num_draws={num_draws}: 1 .. {_native.MAX_OBS_DRAWS} noise draws per data point")
    M = None if num_samples is None else int(num_samples)
    if M is not None and not 0 <= M <= _native.MAX_OBS_SAMPLES:
        raise ValueError(f"num_samples={num_samples}: 0 .. {_native.MAX_OBS_SAMPLES} posterior draws per data point")
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: x must be a [batch, dim] float32 tensor")
    B = int(x.shape[0])
    if method not in solvers.FIXED_METHODS:
        if chunk_points is not None:
            raise ValueError(f"chunk_points with method={method!r}: an adaptive solve takes its step size from the error "
                             "norm of the whole batch, so chunks would change every row's steps; all B * num_draws rows "
                             "are one solve.  A fixed-grid method (method='rk4' with options={'step_size': h}) processes "
                             "chunks with bitwise the same result")
        chunk = max(B, 1)
    elif chunk_points is None:
        chunk = max(1, OBSERVE_CHUNK_ROWS // K)
    else:
        chunk = int(chunk_points)
        if chunk < 1:
            raise ValueError(f"chunk_points={chunk_points}: at least one data point per chunk")
    return K, M, chunk


def _observe_seed(seed):
    """``seed`` of the noise draws; None draws a 63-bit one from torch's default generator."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) if seed is None else int(seed)


def _observe_chunks(log_prob_rows, randomised, x, noise_std, cond, num_draws, method, seed, sample_offset, chunk_points,
                    want_ess, num_samples):
    """The loop over chunks of ``log_prob_noisy`` and ``posterior_noisy``: its checks, the chunk rule and the seed draw,
    then per chunk expand -> the model's ``log_prob`` -> the reductions.  Returns ``(log_p [B], ess [B] or None,
    posterior)``; with ``num_samples`` = M not None the chunk's particles and log-densities also go through
    ff_weighted_resample before they are dropped, ``posterior`` = (samples [B, M, D], index [B, M], mean, var [B, D]) --
    else None."""
    what = "log_prob_noisy" if num_samples is None else "posterior_noisy"
    K, M, chunk = _observe_args(what, x, num_draws, num_samples, method, chunk_points)
    B = int(x.shape[0])
    std = noise_std_tensor(noise_std, x)
    seed, first = _observe_seed(seed), int(sample_offset)
    x = x.detach().contiguous()
    cond = _native.f32_on(cond, x.device)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    ess = torch.empty(B, dtype=torch.float32, device=x.device) if want_ess else None
    parts = []
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        y, ck = _native.observe_expand(x[lo:hi], std if std.dim() == 1 else std[lo:hi], K, seed, first + lo,
                                       None if cond is None else cond[lo:hi])
        extra = {"probe": "philox", "seed": seed, "sample_offset": (first + lo) * K} if randomised else {}
        lp = log_prob_rows(y, ck, extra)
        del ck
        lp = lp.detach().to(torch.float32).contiguous()
        _native.logmeanexp(lp, K, out[lo:hi], None if ess is None else ess[lo:hi])
        if M is not None:
            parts.append(_native.weighted_resample(y, lp, K, M, seed, first + lo))
        del y, lp
    if M is None:
        return out, ess, None
    if len(parts) == 1:
        return out, ess, parts[0]
    if not parts:
        parts = [_native.weighted_resample(x.new_empty(0, x.shape[1]), x.new_empty(0), K, M, seed, first)]
    return out, ess, tuple(torch.cat(cols) for cols in zip(*parts))


class NoisyPosterior(NamedTuple):
    """What ``posterior_noisy`` returns about the per-object posterior ``p(x | x_obs, noise_std)``."""
    samples: torch.Tensor       # [B, M, D]: M draws per object, in the units of x
    log_prob: torch.Tensor      # what log_prob_noisy returns for the same arguments and seed
    ess: torch.Tensor           # [B]: the effective sample size of the K weights
    mean: torch.Tensor          # [B, D]: the weighted mean of the K particles
    var: torch.Tensor           # [B, D]: their weighted variance about it
    index: torch.Tensor         # [B, M] int32: samples[r, m] is particle index[r, m] of object r


def posterior_noisy(log_prob_rows, randomised, x, noise_std, cond, num_draws, num_samples, method, seed, sample_offset,
                    chunk_points):
    """What every front end's ``posterior_noisy`` does: the loop of ``log_prob_noisy`` (same arguments, checks, chunk rule
    and seed), keeping what that one throws away.  The K rows ``y_k = x - noise_std z_k`` of a point with weights
    ``w_k ~ p(y_k)`` are a self-normalised importance sample of its posterior ``p(x | x_obs, noise_std) ~ p(x)
    N(x_obs; x, diag noise_std^2)``: ff_weighted_resample draws ``num_samples`` = M of them per point by their weights
    (uniforms of the counter-based stream under the same ``seed`` and global row, FF_OBS_RESAMPLE_NOISE_INDEX) and forms
    the weighted mean and variance, in double.  Returns a ``NoisyPosterior`` whose ``log_prob`` [B] and ``ess`` are the
    ff_logmeanexp results of ``log_prob_noisy(..., return_ess=True)``, bit for bit; every field is bitwise independent of
    the chunking on a fixed grid."""
    out, ess, (samples, index, mean, var) = _observe_chunks(log_prob_rows, randomised, x, noise_std, cond, num_draws, method,
                                                            seed, sample_offset, chunk_points, True, num_samples)
    return NoisyPosterior(samples, out, ess, mean, var, index)


def log_prob_noisy_grad(value_rows, grad_rows, randomised, x, noise_std, cond, num_draws, method, seed, sample_offset,
                        chunk_points, min_weight, return_ess, return_noise_grad, checks=None, stats=None):
    """What every front end's ``log_prob_noisy_grad`` does: ``log_prob_noisy`` on a fixed grid with its gradient, ``(log_p
    [B], grad_x [B, D], grad_c [B, C] or None [, ess [B]] [, grad_noise_std [B, D]])``.  With ``lp_k`` the log-density of row
    ``y_k = x - noise_std z_k`` and ``wn_k = exp(lp_k - max lp) / W`` its normalised weight (double), the gradient of
    ``logsumexp_k lp_k - log K`` at fixed draws is ``sum_k wn_k grad lp_k`` for ``x`` and ``cond`` and ``-sum_k wn_k z_k
    grad_y lp_k`` for ``noise_std`` (per object and dimension, whatever the shape of ``noise_std``).

    Per chunk of points (the chunk rule, checks and seed of ``log_prob_noisy``): ff_observe_expand -> ``value_rows(y,
    cond_rows, extra)`` -> ``(lp [rows], probes [rows, P, D] or None)``, the model's fixed-grid log-density of the rows and, on
    a ``randomised`` (Hutchinson) model, the probes it took (``extra`` keys them as in ``log_prob_noisy``) -> ff_logmeanexp
    (``log_p`` and ``ess``: bitwise ``log_prob_noisy``'s) -> ff_observe_keep -> the kept rows, their conditionals and probes
    gathered in order -> ``grad_rows(y_kept, cond_kept, probes_kept)`` -> ``(gx [n, D], gc [n, C] or None, rows launched)``,
    the record and gradient launches of ``solve_logp_grad`` in the user's units -> ff_observe_grad_reduce.  Only kept rows
    reach the gradient launches: draw k is kept iff ``wn_k > 0`` and ``wn_k >= min_weight``, and the sums take the weights of
    the FULL ``W``, not renormalised, so a ``min_weight`` = m > 0 truncates by at most ``sum_skipped wn_k |grad lp_k| <= K m
    max |grad lp|``.  A point with a NaN or +inf among its ``lp``, or with ``W = 0``, has NaN gradients.  Rows and points are
    independent: any chunking, and any slice of the batch at its ``sample_offset``, gives bitwise the same.

    ``checks()``: the front end's refusals, run after the host-only argument checks and before the device is touched.
    ``stats``: a dict that receives ``rows``, ``rows_kept`` and ``gradient_rows`` (what ``grad_rows`` launched)."""
    m = float(min_weight)
    if not 0.0 <= m < 1.0:
        raise ValueError(f"min_weight={min_weight}: a normalised weight, 0 <= min_weight < 1 (0 keeps every draw of non-zero "
                         "weight)")
    K, _, chunk = _observe_args("log_prob_noisy_grad", x, num_draws, None, method, chunk_points)
    if checks is not None:
        checks()
    B, D = int(x.shape[0]), int(x.shape[1])
    std = noise_std_tensor(noise_std, x)
    seed, first = _observe_seed(seed), int(sample_offset)
    x = x.detach().contiguous()
    cond = _native.f32_on(cond, x.device)
    C = 0 if cond is None else int(cond.shape[1])
    new = lambda cols: torch.empty(B, cols, dtype=torch.float32, device=x.device)
    out, ess = new(1).view(B), (new(1).view(B) if return_ess else None)
    gx, gc, gs = new(D), (new(C) if C > 0 else None), (new(D) if return_noise_grad else None)
    kept = launched = 0
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        std_c = std if std.dim() == 1 else std[lo:hi]
        y, ck = _native.observe_expand(x[lo:hi], std_c, K, seed, first + lo, None if cond is None else cond[lo:hi])
        extra = {"probe": "philox", "seed": seed, "sample_offset": (first + lo) * K} if randomised else {}
        lp, probes = value_rows(y, ck, extra)
        lp = lp.detach().to(torch.float32).contiguous().view(-1)
        _native.logmeanexp(lp, K, out[lo:hi], None if ess is None else ess[lo:hi])
        keep = _native.observe_keep(lp, K, m)
        rows = torch.nonzero(keep).view(-1)                 # the kept rows in order: row_of is their rank
        n = int(rows.numel())
        row_of = torch.where(keep > 0, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
        if n == 0:
            gxr, gcr = y.new_zeros(0, D), (None if C == 0 else y.new_zeros(0, C))
        else:
            take = lambda t: None if t is None else (t if n == t.shape[0] else t.index_select(0, rows))
            gxr, gcr, ran = grad_rows(take(y), take(ck), take(probes))
            launched += int(ran)
        kept += n
        _native.observe_grad_reduce(lp, row_of, gxr, gcr, std_c, K, seed, first + lo, return_noise_grad, gx[lo:hi],
                                    None if gc is None else gc[lo:hi], None if gs is None else gs[lo:hi])
        del y, ck, lp, probes, gxr, gcr
    if stats is not None:
        stats.update(rows=B * K, rows_kept=kept, gradient_rows=launched)
    return (out, gx, gc) + ((ess,) if return_ess else ()) + ((gs,) if return_noise_grad else ())


def _host_adaptive(front, step, x, t, sign, method, options, mode, atol, rtol, norm_only):
    """The host controller around any of the three step functions (``FusedNet`` / ``RowStepper`` / ``ModuleStepper``)."""
    has_lp = mode != MODE_STATE
    solver = adaptive.make_solver(step, has_lp, rtol, atol, options, norm_only=norm_only, method=method, sign=sign)
    lp0 = torch.zeros(x.shape[0], device=x.device) if has_lp else None
    y, lp = solver.integrate(float(sign * t[0]), float(sign * t[-1]), x.detach().to(torch.float32).contiguous(), lp0)
    front.last_solver_stats = {"attempts": solver.n_attempts, "accepted": solver.n_accepted}
    return y, lp


def _estimator_budget(device) -> int:
    """Bytes the recorded Jacobians of an attempted step may take: half of what the device has free right now."""
    free, _ = torch.cuda.mem_get_info(device)
    return free // 2
