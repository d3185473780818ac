"""Flow-matching continuous normalising flows on MI355X: the reference's ``flowfusion.flow`` API
(``ODEFlow`` flow.py:9-438, ``ConditionalODEFlow`` flow.py:441-941) with ``sample`` and
``log_prob`` / ``solve_ode_forward`` running as one fused HIP launch.

The velocity network takes ``[x, t]`` (``[x, t, (cond - shift)/scale]`` when conditional,
flow.py:112-115, 583-586).  ``state_dict`` keys match the reference: ``twopi``,
``target_shift``/``target_scale`` (+ ``conditional_*``), and the Linear parameters under both
``layers.{0,2,..}`` and ``velocity.{0,2,..}`` (the same modules registered twice).

Native: ``sample`` (t: 1 -> 0) and ``solve_ode_forward`` / ``log_prob`` (t: 0 -> 1, exact
divergence by forward-mode tangents, or a Hutchinson probe as an opt-in extension) for SiLU
networks and fixed-grid methods.  The reference's ``sample`` exposes no solver arguments and
always runs adaptive dopri5 at torchdiffeq's default tolerances (flow.py:299-303); here ``sample``
takes optional ``method``/``options`` keywords.  Nothing on these methods falls back to eager
PyTorch or the CPU: unsupported requests raise.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from . import _native, device_adaptive, odeint, solvers, trace_estimators
from .fused import FusedNet, MODE_EXACT, MODE_HUTCH, MODE_STATE, activation_spec, within_envelope
from .odeint import NoisyPosterior  # noqa: F401  (what ``posterior_noisy`` returns)

_DEFAULT_SAMPLE_METHOD = "dopri5"     # what odeint() picks when the reference passes no method


def _build_layers(sizes, activation):
    layers = nn.ModuleList()
    for n_in, n_out in zip(sizes[:-2], sizes[1:-1]):
        layers.append(nn.Linear(n_in, n_out))
        layers.append(activation())
    layers.append(nn.Linear(sizes[-2], sizes[-1]))
    return layers


class _FlowBase(nn.Module):
    """Common fused plumbing of the two flow classes."""

    def _linears(self):
        return [m for m in self.layers if isinstance(m, nn.Linear)]

    def _net(self) -> FusedNet:
        specs = {activation_spec(m) for m in self.layers if not isinstance(m, nn.Linear)}
        if len(specs) != 1:
            raise NotImplementedError("the fused gfx950 path needs one activation shared by all hidden layers")
        act = next(iter(specs))
        lin = self._linears()
        cached = getattr(self, "_fused", None)
        prec = getattr(self, "precision", "f32")       # extension: "bf16x3" = split-precision kernels (see ScoreModel)
        if cached is None or not cached.serves(lin, act, prec):
            D = self.target_dimension
            C = getattr(self, "conditional_dimension", 0)
            # first-layer columns: [x (D) | t (1) | cond (C)]
            object.__setattr__(self, "_fused", FusedNet(lin, D, C, x_col0=0, c_col0=D + 1, act=act, precision=prec))
        return self._fused

    def _fusable(self) -> bool:
        """A compiled kernel holds the velocity network (shape and activation).  The reference has no limit on
        either (flow.py:61-74, 494-508); outside the compiled shapes the solve goes through generic.py.  An explicit
        ``precision=`` other than f32 never switches arithmetic silently: ``_net()`` raises instead."""
        if getattr(self, "precision", "f32") != "f32":
            return True
        key = tuple(id(m) for m in self.layers) + tuple(repr(m) for m in self.layers if not isinstance(m, nn.Linear))
        return within_envelope(self, key, self._net)

    def _module_rhs(self, mode, cond, probe):
        """``self.velocity`` evaluated by torch for the generic route (odeint.py): stage combinations, error norms and step
        control by the library (generic.py), divergences by autograd as in the reference (flow.py:122-166, 598-652)."""
        D = self.target_dimension

        def velocity(t, y):
            cols = [y, t.reshape(1, 1).to(y.dtype).expand(y.shape[0], 1)]
            if cond is not None:
                cols.append(cond)
            return self.velocity(torch.cat(cols, dim=1))

        def rhs(t, y):
            if mode == MODE_STATE:
                with torch.no_grad():
                    return velocity(t, y), None
            with torch.enable_grad():
                y = y.detach().requires_grad_(True)
                v = velocity(t, y)
                if mode == MODE_HUTCH and probe.dim() == 3:      # K probes (already times 1/sqrt(K)): the sum is their mean
                    div = sum((torch.autograd.grad(v, y, probe[:, k], retain_graph=True)[0] * probe[:, k]).sum(dim=1)
                              for k in range(probe.shape[1]))
                elif mode == MODE_HUTCH:
                    div = (torch.autograd.grad(v, y, probe)[0] * probe).sum(dim=1)
                else:
                    div = sum(torch.autograd.grad(v[:, i].sum(), y, retain_graph=True)[0][:, i] for i in range(D))
            return v.detach(), div.detach()

        return rhs

    def _schedule(self, t, first=None):
        """(a, b, c1) for real times t (fp32, CPU): xdot = NET([x, t, cond]) -> a = 0, b = 1,
        c1 = w_t * t + bias of the first layer (flow.py:112-118).  ``first`` = host copy of the first layer,
        taken once per solve by the adaptive path (a device-to-host copy per step would wait for the kernel)."""
        w0, b0 = first if first is not None else self._net().first_layer_cpu()
        D = self.target_dimension
        with solvers.host_threads():
            c1 = t[:, None] * w0[:, D][None, :] + b0[None, :]
            return torch.zeros_like(t), torch.ones_like(t), c1

    def _host_schedule(self):
        """``_schedule`` for the host controller, with the host copy of the first layer taken once per solve."""
        first = self._net().first_layer_cpu()
        return lambda tr: self._schedule(tr, first)

    def _device_schedule(self, device):
        """``device_adaptive.ScheduleSpec`` of the device controller: xdot = NET([x, t, cond]) -> a = 0, b = 1,
        c1 = w_t t + b1."""
        D = self.target_dimension
        w0t, b0 = self._net().time_columns(device, D, D + 1)
        return device_adaptive.ScheduleSpec(_native.SCHED_FLOW, (0.0, 0.0, 0.0), True, None, 0.0, w0t, b0)

    def _ode_table(self, t_span, method, options, mode, y0=None):
        plan = solvers.plan_ode(t_span, method, options, y0=y0)
        self._net().require_slots(int(plan.slot.max()) + 1, mode, f"method={method!r}")
        a, b, c1 = self._schedule(plan.t_eval)
        return solvers.build_table(plan, a, b, c1, self._net().width(mode))

    _table = _ode_table       # the flows' older name, still used by the tests and scratch/

    def _schedule_key(self):
        """Everything besides the first layer that the evaluation table depends on: nothing."""
        return ()

    def _norm_cond(self, conditional):
        return (conditional - self.conditional_shift) / self.conditional_scale

    def _cond_args(self, conditional):
        """(normalised conditional, ``norm_only``) of a public method's raw ``conditional``; None: the unconditional flow."""
        return (None, ()) if conditional is None else (self._norm_cond(conditional), (conditional,))

    def _solve(self, x, t_span, method, options, mode, atol, rtol, **kw):
        """``odeint(self, x, t_span, ...)``: the flow's solve through the shared dispatcher (odeint.py)."""
        return odeint.solve(self, x, t_span, method, options, mode, atol, rtol, **kw)

    def _fused_sample(self, xT, conditional, method, options, atol, rtol, norm_only=()):
        if torch.is_grad_enabled() and xT.requires_grad:
            raise NotImplementedError("gradients through the fused solve are not available; detach the input")
        method = _DEFAULT_SAMPLE_METHOD if method is None else method
        t_span = torch.tensor([1.0, 0.0], dtype=torch.float32)
        x, _ = self._solve(xT, t_span, method, options, MODE_STATE, atol, rtol, cond=conditional, norm_only=norm_only,
                           out_scale=self.target_scale, out_shift=self.target_shift)
        return x

    def _probe_rng(self, probe, seed, sample_offset, hutchinson):
        """``probe="torch"`` (default): the +-1 probe is drawn on the CPU and moved; ``probe="philox"`` (keyword-only
        extension, as on ScoreModel.log_prob): the signs of the library's counter-based normals keyed by ``seed`` and the
        GLOBAL row ``sample_offset + r`` -- drawn on the device and independent of how a batch is cut into shards
        (``distributed.flow_log_prob_sharded``)."""
        return trace_estimators.probe_rng(probe, seed, sample_offset, hutchinson,
                                          "probe='philox' is the Hutchinson probe: pass hutchinson=True")

    def _fused_forward(self, x, conditional, method, options, hutchinson, atol, rtol, norm_only=(), probe_rng=None,
                       num_probes=1, return_stderr=False):
        """Returns ``(xT, log_jacobian [B,1], stderr [B,1] or None)``.
        ``norm_only``: the raw conditional, which the reference keeps in the solver state (flow.py:779-796, 855-881).
        ``num_probes`` (keyword-only extension of ``solve_ode_forward`` / ``log_prob``, with ``hutchinson=True``): the
        divergence is the mean over that many independent +-1 probes per sample, carried by one launch
        (``odeint.solve_hutchinson``); 1 = the reference's single probe.
        ``return_stderr=True`` (keyword-only extension; ``hutchinson=True``, ``num_probes=K >= 2``, a fixed-grid ``method``):
        the public methods return ``(xT, log_jacobian, stderr [B,1])``, the first two bitwise those of the call without it; ``stderr`` is
        ``trace_estimators.hutchinson_stderr`` of the K single-probe estimates, which stay in ``self.dlogp_probes`` [B, K]
        (column k: the log-Jacobian a single-probe solve with probe k alone returns) next to the probes ``self.e``
        [B, K, D].  Same launch, one more store per tangent column (ff_mlp_ode_launch_probes).  Only this path sets
        ``self.e`` and ``self.dlogp_probes``, and both stay on the device until the next such call: the plain
        ``num_probes=K`` solve keeps no probes on the flows (a [B, K, D] tensor held for nobody), and with
        ``probe="philox"`` it fills the scaled probes directly, without the +-1 form."""
        t_span = torch.tensor([0.0, 1.0], dtype=torch.float32)
        K = trace_estimators.check_num_probes(num_probes, hutchinson, "pass hutchinson=True")
        stderr = trace_estimators.check_stderr(return_stderr, K, method)
        if not hutchinson:
            xT, logj = self._solve(x, t_span, method, options, MODE_EXACT, atol, rtol, cond=conditional, norm_only=norm_only)
            return xT, logj.view(-1, 1), None
        xT, logj, d = odeint.solve_hutchinson(self, x, t_span, method, options, atol, rtol, K, probe_rng,
                                              keep=(lambda e: setattr(self, "e", e)) if stderr else None, per_probe=stderr,
                                              cond=conditional, norm_only=norm_only)
        if stderr:
            self.dlogp_probes = d
        return xT, logj.view(-1, 1), (trace_estimators.hutchinson_stderr(d).view(-1, 1) if stderr else None)

    # -- flow-map sensitivities (extension) -------------------------------------------------------------------------------
    def _push_args(self, x, conditional, direction):
        """(t_span, keywords of ``odeint.solve_push``) of a sensitivity solve: ``to_data`` is ``sample``'s solve (base point
        -> target space, ``* target_scale + target_shift`` in the kernel), ``to_base`` is ``log_prob``'s (target-space point
        -> base, ``(x - target_shift) / target_scale`` in the kernel); the raw ``conditional`` is normalised as everywhere."""
        if direction not in ("to_data", "to_base"):
            raise ValueError(f"direction={direction!r}: 'to_data' (the solve of sample) or 'to_base' (the solve of log_prob)")
        C = getattr(self, "conditional_dimension", 0)
        kw = {}
        if conditional is not None:
            if C == 0:
                raise ValueError("flow-map sensitivities: this flow has no conditional inputs")
            if not torch.is_tensor(conditional) or conditional.dim() != 2 or conditional.shape[1] != C:
                raise ValueError(f"flow-map sensitivities: conditional must be [batch, {C}]")
            kw = {"cond": self._norm_cond(conditional), "cond_tangent_scale": self.conditional_scale}
        if direction == "to_data":
            return torch.tensor([1.0, 0.0], dtype=torch.float32), dict(kw, out_scale=self.target_scale, out_shift=self.target_shift)
        return torch.tensor([0.0, 1.0], dtype=torch.float32), dict(kw, in_shift=self.target_shift, in_scale=self.target_scale)

    @torch.no_grad()
    def flow_jvp(self, x, tangents=None, conditional=None, conditional_tangents=None, *, direction="to_data", method="rk4",
                 options=None):
        """Extension: the solve of ``sample`` (``direction="to_data"``, ``x`` = base points) or of ``log_prob``
        (``"to_base"``, ``x`` = target-space points) with K directions pushed through it, forward mode, in ONE launch:
        returns ``(x_out [B, D], dx [B, K, D])`` with ``dx[b, k] = d x_out[b] / d (x[b], conditional[b]) . (tangents[b, k],
        conditional_tangents[b, k])`` -- the exact derivative of the DISCRETE solver map (fixed grids only: ``method="rk4"``
        / ``"dopri5_fixed"`` / ``"euler"`` ... with ``options={"step_size": h}``), in the units of ``x``, ``x_out`` and the
        raw ``conditional``.  ``tangents`` [B, K, D] and ``conditional_tangents`` [B, K, C]: either may be None (zero);
        K <= 15.  No parameter gradients, no torch.autograd integration (the call runs under ``no_grad``), no adaptive step
        control: see ``odeint.solve_push``."""
        t_span, kw = self._push_args(x, conditional, direction)
        return odeint.solve_push(self, x, t_span, method, options, tangents=tangents, cond_tangents=conditional_tangents, **kw)

    @torch.no_grad()
    def flow_jacobian(self, x, conditional=None, *, direction="to_data", method="rk4", options=None):
        """Extension: the whole Jacobian of the solver map of ``flow_jvp``: ``(x_out [B, D], J_x [B, D, D], J_c [B, D, C] or
        None)``, ``J_x[b, i, j] = d x_out_i / d x_j``, ``J_c[b, i, j] = d x_out_i / d conditional_j``, from unit tangents
        in ceil((D + C) / 15) launches."""
        t_span, kw = self._push_args(x, conditional, direction)
        return odeint.solve_push_jacobian(self, x, t_span, method, options, **kw)

    @torch.no_grad()
    def flow_vjp(self, x, cotangents, conditional=None, *, direction="to_data", method="rk4", options=None,
                 return_retrace=False, adjoint="continuous"):
        """Extension: K cotangents pulled back through the solve of ``sample`` (``direction="to_data"``, ``x`` = base points)
        or of ``log_prob`` (``"to_base"``, ``x`` = target-space points), reverse mode: returns ``(x_out [B, D], gx [B, K, D],
        gc [B, K, C] or None)`` -- plus ``retrace [B]`` with ``return_retrace`` -- with ``gx[b, k] = cotangents[b, k]^T
        d x_out[b] / d x[b]`` and ``gc`` likewise for the raw ``conditional``, in the units of ``x``, ``x_out`` and the raw
        ``conditional`` (``flow_jvp``'s conventions).  ``cotangents`` is [B, K, D], K <= 15.  ``x_out`` is bitwise the
        fixed-grid ``sample`` / forward solve.

        It integrates the CONTINUOUS adjoint over the reversed grid, as the reference's ``odeint_adjoint`` does
        (``sample(gradients=True)``, ``adjoint=True``) -- not the transpose of the discrete map ``flow_jvp``
        differentiates.  The two differ by the discretisation error, and the backward sweep retraces the state instead of
        storing it: use rk4 or better, read ``retrace[b] = max_d |y_back - x|`` (how far the retraced trajectory ended
        from ``x``, in its units), and raise the step count until it is small.  (Measured in float64 on a small flow: gap to
        ``w^T flow_jacobian`` 6e-11 with 16 rk4 steps, 9e-3 with 128 euler steps.)

        ``adjoint="discrete"`` (keyword only) takes the exact discrete adjoint instead (``odeint.solve_pull_discrete``): a
        forward launch records the stage state of every evaluation row and a second one runs the transposed row program
        backwards over them, so ``gx`` and ``gc`` are the transpose of what ``flow_jvp`` differentiates up to rounding at ANY
        step count -- the gradient of the function that is actually evaluated.  ``x_out`` is then the record launch's state
        (bitwise the fixed-grid solve's, as on the default route), nothing is retraced (``return_retrace`` raises), and
        the record costs ``n_evals * B * D`` floats of device memory per piece of rows.  Any other value raises ValueError.

        No parameter gradients, no torch.autograd integration (the call runs under ``no_grad``), no adaptive step
        control: see ``odeint.solve_pull`` and ``odeint.solve_pull_discrete``."""
        t_span, kw = self._push_args(x, conditional, direction)
        return odeint.solve_pull_by(adjoint, self, x, t_span, method, options, cotangents, return_retrace=return_retrace, **kw)

    @torch.no_grad()
    def _log_prob_grad(self, x, conditional, method, options, hutchinson, probe, seed, sample_offset, num_probes):
        """``log_prob_grad`` of both flows (extension): ``log_prob`` on a fixed grid with its gradient, ``(log_p [B, 1],
        grad_x [B, D], grad_c [B, C] or None)`` in the units of the target-space ``x`` and the raw ``conditional``.  ``log_p`` is
        bitwise ``log_prob(x, [conditional,] method=method, options=options, hutchinson=hutchinson, probe=..., ...)`` (as a
        column).  ``hutchinson=True``: the gradient launches take the very probes of that solve, and the gradient is exact for
        that value at FIXED probes -- the discrete adjoint with the divergence integral in it (``odeint.solve_logp_grad``),
        exact at any step count.  ``hutchinson=False``: the value comes from the exact-trace solve, the gradient from the D
        unit probes with weight 1 -- the gradient of the same discrete sum, to rounding.  ``- sum log target_scale`` is a
        constant; ``(x - target_shift) / target_scale`` contributes ``1 / target_scale``.

        Fixed grids only (``method="rk4"`` / ``"dopri5_fixed"`` / ``"euler"`` with ``options={"step_size": h}``; the default
        grid is ONE step): adaptive methods, ``grid_constructor`` / ``perturb`` and ``precision`` other than f32 raise
        before the device is touched.  No parameter gradients, no torch.autograd integration; the gradient of
        ``log_prob_noisy`` is ``log_prob_noisy_grad``."""
        cond, kw = self._logp_grad_cond(conditional)
        K = trace_estimators.check_num_probes(num_probes, hutchinson, "pass hutchinson=True")
        rng = self._probe_rng(probe, seed, sample_offset, hutchinson)
        odeint.check_logp_grad(self, x, method, options, cond)
        logp, probes = self._logp_value(x, conditional, cond, method, options, hutchinson, K, rng)
        gx, gc = self._logp_grad_rows(x, cond, method, options, probes, kw)
        return logp.view(-1, 1), gx, gc

    def _logp_grad_cond(self, conditional):
        """(normalised conditional, keywords of ``odeint.solve_logp_grad``) of a raw ``conditional``, checked."""
        C = getattr(self, "conditional_dimension", 0)
        if conditional is None:
            return None, {}
        if C == 0:
            raise ValueError("log-density gradients: this model has no conditional inputs")
        if not torch.is_tensor(conditional) or conditional.dim() != 2 or conditional.shape[1] != C:
            raise ValueError(f"log-density gradients: conditional must be [batch, {C}]")
        return self._norm_cond(conditional), {"cond_tangent_scale": self.conditional_scale}

    def _logp_value(self, x, conditional, cond, method, options, hutchinson, K, rng):
        """The value half of ``_log_prob_grad``: ``(log_p [B], probes [B, K, D] or None)``, the fixed-grid ``log_prob`` of the
        rows ``x`` and the Hutchinson probes it took (None: the exact trace).  ``cond``: ``conditional`` normalised."""
        xn = (x - self.target_shift) / self.target_scale
        t_span = torch.tensor([0.0, 1.0], dtype=torch.float32)
        norm_only = () if conditional is None else (conditional,)
        if hutchinson:
            kept = []
            xT, logj, _ = odeint.solve_hutchinson(self, xn, t_span, method, options, 1e-5, 1e-5, K, rng, keep=kept.append,
                                                  cond=cond, norm_only=norm_only)
            probes = kept[-1] if K > 1 else kept[-1].unsqueeze(1)
        else:
            xT, logj = self._solve(xn, t_span, method, options, MODE_EXACT, 1e-5, 1e-5, cond=cond, norm_only=norm_only)
            probes = None
        base = torch.sum(-0.5 * xT ** 2 - 0.5 * torch.log(self.twopi), dim=1)
        return base + logj.view(-1, 1).squeeze(1) - torch.sum(torch.log(self.target_scale)), probes

    def _logp_grad_rows(self, x, cond, method, options, probes, kw):
        """The gradient half of ``_log_prob_grad``: ``(gx [B, D], gc [B, C] or None)`` of the rows ``x`` with the probes of
        their value solve, or with the D unit probes of the exact trace (``probes`` None)."""
        B, D = x.shape
        xn = (x - self.target_shift) / self.target_scale
        t_span = torch.tensor([0.0, 1.0], dtype=torch.float32)
        if probes is not None:
            weight = 1.0 / probes.shape[1]
        else:
            probes, weight = torch.eye(D, dtype=torch.float32, device=x.device).expand(B, D, D), 1.0
        _, gx, gc = odeint.solve_logp_grad(self, xn, t_span, method, options, probes.contiguous(), weight, cond=cond, **kw)
        return gx / self.target_scale, gc

    @torch.no_grad()
    def _log_prob_noisy_grad(self, x, noise_std, conditional, num_draws, method, options, hutchinson, seed, sample_offset,
                             chunk_points, num_probes, min_weight, return_ess, return_noise_grad):
        """``log_prob_noisy_grad`` of both flows (extension): ``log_prob_noisy`` on a fixed grid with its gradient, ``(log_p
        [B, 1], grad_x [B, D], grad_c [B, C] or None)`` -- then ``ess [B]`` with ``return_ess`` and ``grad_noise_std [B, D]``
        with ``return_noise_grad`` -- in the units of the target-space ``x``, its ``noise_std`` and the raw ``conditional``:
        what HMC / NUTS or L-BFGS over the population hyper-parameters of a catalogue of measured objects needs.  ``log_p``
        (as a column) and ``ess`` are bitwise ``log_prob_noisy(x, noise_std, [conditional,] num_draws, method=method,
        options=options, hutchinson=hutchinson, seed=seed, ..., return_ess=True)``.  With ``wn_k`` the normalised weight of
        draw k (double), ``grad_x = sum_k wn_k grad_y lp_k``, ``grad_c = sum_k wn_k grad_c lp_k`` and ``grad_noise_std = -sum_k
        wn_k z_k grad_y lp_k`` (per object and dimension, whatever the shape of ``noise_std``), ``grad lp_k`` the discrete
        adjoint of ``_log_prob_grad`` on row k: the exact gradient of the value returned at fixed draws -- and, with
        ``hutchinson=True``, at fixed probes (the very probes of the value solve of those rows, ``probe="philox"`` under the
        same ``seed``) -- at any step count.  ``hutchinson=False``: the value comes from the exact-trace solve and the
        gradient from the D unit probes with weight 1, D gradient rows per kept draw: ``min_weight`` is the lever.

        ``min_weight`` = m (0 <= m < 1): only draws with ``wn_k > 0`` and ``wn_k >= m`` go through the record and gradient
        launches.  The sums keep the weights of the full sum, not renormalised, so the truncation error is at most
        ``sum_skipped wn_k |grad lp_k| <= K m max |grad lp|``; m = 0 keeps every draw of non-zero weight.
        ``self.last_noisy_grad_stats`` = ``{"rows": B K, "rows_kept": n, "gradient_rows": rows that reached the gradient
        launch}`` after the call.  A point with a NaN or +inf among its rows' log-densities, or with no weight at all, has
        NaN gradients; its ``log_p`` is what ``log_prob_noisy`` gives.

        Fixed grids only: every refusal of ``log_prob_grad`` applies, before the device is touched.  ``noise_std``,
        ``num_draws``, ``seed``, ``sample_offset``, ``chunk_points``: as in ``log_prob_noisy``; any chunking and any slice of
        the batch at its ``sample_offset`` give bitwise the same.  Out of scope: sharded entry points (slice), adaptive
        methods, gradients of ``posterior_noisy``, parameter gradients and torch.autograd integration."""
        hutchinson = bool(hutchinson)
        K = 1

        def checks():
            nonlocal K
            cond, _ = self._logp_grad_cond(conditional)
            K = trace_estimators.check_num_probes(num_probes, hutchinson, "pass hutchinson=True")
            odeint.check_logp_grad(self, x, method, options, cond)

        def value_rows(y, c, extra):
            rng = (extra["seed"], extra["sample_offset"]) if extra else None
            return self._logp_value(y, c, None if c is None else self._norm_cond(c), method, options, hutchinson, K, rng)

        def grad_rows(y, c, probes):
            cond, kw = self._logp_grad_cond(c)
            gx, gc = self._logp_grad_rows(y, cond, method, options, probes, kw)
            return gx, gc, y.shape[0] * (K if hutchinson else y.shape[1])

        self.last_noisy_grad_stats = {}
        out = odeint.log_prob_noisy_grad(value_rows, grad_rows, hutchinson, x, noise_std, conditional, num_draws, method, seed,
                                         sample_offset, chunk_points, min_weight, return_ess, return_noise_grad, checks=checks,
                                         stats=self.last_noisy_grad_stats)
        return (out[0].view(-1, 1),) + out[1:]

    # -- the public methods' bodies, written once (``conditional=None``: the unconditional flow) -----------------------------
    def compute_linear_velocity_field(self, x0, xT, t):
        x0 = (x0 - self.target_shift) / self.target_scale
        return (1 - t) * x0 + t * xT, xT - x0

    def _sample(self, xT, conditional, gradients, method, options, atol, rtol):
        if gradients:
            raise NotImplementedError("sample(gradients=True) uses odeint_adjoint in the reference "
                                      f"(flow.py:{'286-295' if conditional is None else '779-788'}); differentiable solves are "
                                      "out of scope (flow_vjp pulls cotangents back through a fixed-grid solve, for x and "
                                      "the conditional; parameter gradients are not built)")
        cond, norm_only = self._cond_args(conditional)
        return self._fused_sample(xT, cond, method, options, atol, rtol, norm_only=norm_only)

    def _solve_ode_forward(self, x, conditional, atol, rtol, method, options, adjoint, hutchinson, probe, seed, sample_offset,
                           num_probes, return_stderr):
        """``(xT, log_jacobian [B,1], stderr [B,1] or None)`` of the normalised points ``x``."""
        if adjoint:
            raise NotImplementedError("adjoint=True (odeint_adjoint) is out of scope for the fused path (flow_vjp is the "
                                      "continuous adjoint of a fixed-grid solve with respect to x and the conditional)")
        cond, norm_only = self._cond_args(conditional)
        return self._fused_forward(x, cond, method, options, hutchinson, atol, rtol, norm_only=norm_only,
                                   probe_rng=self._probe_rng(probe, seed, sample_offset, hutchinson), num_probes=num_probes,
                                   return_stderr=return_stderr)

    def _log_prob(self, x, conditional, *solver):
        """``(log_p [B], stderr [B] or None)`` of target-space points; ``solver``: the rest of ``_solve_ode_forward``."""
        x = (x - self.target_shift) / self.target_scale
        xT, logj, se = self._solve_ode_forward(x, conditional, *solver)
        base = torch.sum(-0.5 * xT ** 2 - 0.5 * torch.log(self.twopi), dim=1)
        logp = base + logj.squeeze(1) - torch.sum(torch.log(self.target_scale))
        return logp, (None if se is None else se.squeeze(1))

    @torch.no_grad()
    def _log_prob_noisy(self, x, noise_std, conditional, num_draws, atol, rtol, method, options, hutchinson, seed,
                        sample_offset, chunk_points, return_ess, num_probes):
        """``log_prob_noisy`` of both flows (extension): target-space points ``x`` [B, D] (fp32, on the GPU) were measured
        with Gaussian errors of known standard deviation ``noise_std`` ([B, D], [D] or a scalar; finite, >= 0, in the units
        of ``x``: before ``(x - target_shift) / target_scale``), and a likelihood needs the convolved density
        ``p_obs(x | noise_std) = E_{z ~ N(0, I)}[p(x - noise_std z)]``.  Returns ``logsumexp_k log p(x - noise_std z_k) -
        log K`` [B] from ``num_draws`` = K draws per point; with ``return_ess=True`` ``(log_p [B], ess [B])``, ess the
        effective sample size of the K weights, in (0, K].  The flow's own ``log_prob`` runs on the B K expanded rows
        (its affine map and ``- sum log target_scale`` apply unchanged; the raw ``conditional`` is repeated for the draws);
        ``seed`` / ``sample_offset`` / ``chunk_points`` and the chunking rules: ``odeint.log_prob_noisy``.  With
        ``noise_std = 0, num_draws = 1`` this is ``log_prob`` bit for bit.

        ``hutchinson=True`` takes the probes of the expanded rows from ``probe="philox"`` under the same ``seed``, keyed by
        the expanded global row.  Mind what it estimates: the Hutchinson divergence is unbiased for log p, but here it sits
        inside an exponent, and E[exp(noisy)] > exp(E[noisy]) -- the estimate of p_obs is biased upwards by about half the
        variance of the divergence estimate (``num_probes`` shrinks it).  The exact trace is the clean case."""
        rows = lambda y, c, extra: self.log_prob(y, *(() if c is None else (c,)), atol=atol, rtol=rtol, method=method,
                                                 options=options, hutchinson=hutchinson, num_probes=num_probes, **extra)
        return odeint.log_prob_noisy(rows, bool(hutchinson), x, noise_std, conditional, num_draws, method, seed,
                                     sample_offset, chunk_points, return_ess)

    @torch.no_grad()
    def _posterior_noisy(self, x, noise_std, conditional, num_draws, num_samples, atol, rtol, method, options, hutchinson,
                         seed, sample_offset, chunk_points, num_probes):
        """``posterior_noisy`` of both flows (extension): the per-object posterior ``p(x_true | x, noise_std) ~ p(x_true)
        N(x; x_true, diag noise_std^2)`` of target-space observations ``x`` [B, D], from the same ``num_draws`` = K draws
        that ``_log_prob_noisy`` makes (arguments, seed and chunking rules as there).  The K candidates ``x - noise_std z_k``
        with weights ``w_k ~ p(candidate k)`` are a self-normalised importance sample of it.  Returns a ``NoisyPosterior``:
        ``samples`` [B, M, D] (M = ``num_samples`` multinomial draws of the candidates by their weights, in the units of
        ``x``), ``log_prob`` [B] and ``ess`` [B] (bit for bit ``log_prob_noisy(..., return_ess=True)`` under the same
        seed), ``mean`` and ``var`` [B, D] (the weighted mean -- the denoised estimate -- and variance of the candidates)
        and ``index`` [B, M] (int32: which candidate each sample is).

        The samples are a RESAMPLE of K particles: only as many distinct points as the effective sample size allows.  Read
        ``ess`` before trusting ``samples``, and raise ``num_draws``, not ``num_samples``, to get more of them.  With
        ``hutchinson=True`` the weights carry the noise of the divergence estimate (see ``_log_prob_noisy``); the exact
        trace is the clean case."""
        rows = lambda y, c, extra: self.log_prob(y, *(() if c is None else (c,)), atol=atol, rtol=rtol, method=method,
                                                 options=options, hutchinson=hutchinson, num_probes=num_probes, **extra)
        return odeint.posterior_noisy(rows, bool(hutchinson), x, noise_std, conditional, num_draws, num_samples, method, seed,
                                      sample_offset, chunk_points)


class ODEFlow(_FlowBase):
    """Unconditional flow-matching CNF (reference: flow.py:9-438)."""

    def __init__(self, target_dimension: int = 1, hidden_units: List[int] = [128, 128],
                 activation: nn.Module = nn.SiLU, target_shift: Optional[torch.Tensor] = None,
                 target_scale: Optional[torch.Tensor] = None):
        super().__init__()
        self.target_dimension = target_dimension
        self.layers = _build_layers([target_dimension + 1] + list(hidden_units) + [target_dimension], activation)
        self.velocity = nn.Sequential(*self.layers)
        self.register_buffer("twopi", torch.tensor(2.0 * 3.14159265358979323846))
        self.register_buffer("target_shift", target_shift if target_shift is not None else torch.zeros(target_dimension))
        self.register_buffer("target_scale", target_scale if target_scale is not None else torch.ones(target_dimension))

    # -- pointwise (plain torch) ----------------------------------------------------------------
    def dynamics(self, t: torch.Tensor, states: Tuple[torch.Tensor]):
        x = states[0]
        return self.velocity(torch.cat([x, t.view(-1, 1).expand(x.shape[0], 1)], dim=1))

    def dynamics_with_jacobian(self, t, states):
        x, logj = states
        with torch.set_grad_enabled(True):
            x.requires_grad_(True)
            v = self.dynamics(t, (x,))
            div = torch.zeros_like(logj)
            for i in range(x.shape[-1]):
                div = div + torch.autograd.grad(v[:, i].sum(), x, create_graph=True, retain_graph=True)[0][:, i:i + 1]
        return v, div

    def forward(self, t, states):
        return self.dynamics(t, states)

    # -- fused ------------------------------------------------------------------------------------
    def sample(self, xT: torch.Tensor, gradients: bool = False, method: Optional[str] = None,
               options: Optional[dict] = None, atol: float = 1e-9, rtol: float = 1e-7):
        """Transport base samples xT (t=1) to the target (t=0), then ``* target_scale + target_shift``."""
        return self._sample(xT, None, gradients, method, options, atol, rtol)

    def solve_ode_forward(self, x, atol: float = 1e-5, rtol: float = 1e-5, method: str = "dopri5",
                          options: Optional[dict] = None, adjoint: bool = False, hutchinson: bool = False, *,
                          probe: str = "torch", seed: Optional[int] = None, sample_offset: int = 0, num_probes: int = 1,
                          return_stderr: bool = False):
        """Integrate t: 0 -> 1 with the divergence; returns ``(xT, log_jacobian[B,1])`` (flow.py:308-384).
        ``probe`` / ``seed`` / ``sample_offset``: see ``_probe_rng``; ``num_probes`` / ``return_stderr``: see
        ``_fused_forward``."""
        out = self._solve_ode_forward(x, None, atol, rtol, method, options, adjoint, hutchinson, probe, seed, sample_offset,
                                      num_probes, return_stderr)
        return out if return_stderr else out[:2]

    def log_prob(self, x, atol: float = 1e-5, rtol: float = 1e-5, method: str = "dopri5",
                 options: Optional[dict] = None, adjoint: bool = False, hutchinson: bool = False, *,
                 probe: str = "torch", seed: Optional[int] = None, sample_offset: int = 0, num_probes: int = 1,
                 return_stderr: bool = False):
        """Log-density of target-space points, shape [B] (flow.py:386-438); with ``return_stderr=True`` (see
        ``_fused_forward``) ``(log_p [B], stderr [B])``."""
        out = self._log_prob(x, None, atol, rtol, method, options, adjoint, hutchinson, probe, seed, sample_offset,
                             num_probes, return_stderr)
        return out if return_stderr else out[0]

    def log_prob_grad(self, x, conditional=None, *, method: str = "rk4", options: Optional[dict] = None,
                      hutchinson: bool = False, probe: str = "torch", seed: Optional[int] = None, sample_offset: int = 0,
                      num_probes: int = 1):
        """Extension: ``(log_p [B, 1], grad_x [B, D], None)``: ``log_prob`` on a fixed grid and its gradient with respect to
        ``x`` (see ``_log_prob_grad``).  ``conditional`` must stay None (the signature is the conditional flow's)."""
        if conditional is not None:
            raise ValueError("log-density gradients: this model has no conditional inputs")
        return self._log_prob_grad(x, None, method, options, hutchinson, probe, seed, sample_offset, num_probes)

    def log_prob_noisy_grad(self, x, noise_std, num_draws: int = 16, *, method: str = "rk4", options: Optional[dict] = None,
                            hutchinson: bool = False, seed: Optional[int] = None, sample_offset: int = 0,
                            chunk_points: Optional[int] = None, num_probes: int = 1, min_weight: float = 0.0,
                            return_ess: bool = False, return_noise_grad: bool = False):
        """Extension: ``(log_p [B, 1], grad_x [B, D], None [, ess [B]] [, grad_noise_std [B, D]])``: ``log_prob_noisy`` on a
        fixed grid and its gradient with respect to the observations and their error bars (see ``_log_prob_noisy_grad``)."""
        return self._log_prob_noisy_grad(x, noise_std, None, num_draws, method, options, hutchinson, seed, sample_offset,
                                         chunk_points, num_probes, min_weight, return_ess, return_noise_grad)

    def log_prob_noisy(self, x, noise_std, num_draws: int = 16, atol: float = 1e-5, rtol: float = 1e-5,
                       method: str = "dopri5", options: Optional[dict] = None, *, hutchinson: bool = False,
                       seed: Optional[int] = None, sample_offset: int = 0, chunk_points: Optional[int] = None,
                       return_ess: bool = False, num_probes: int = 1):
        """Log-density [B] of target-space observations with Gaussian errors ``noise_std``, from ``num_draws`` noise draws
        per point (extension; see ``_log_prob_noisy``)."""
        return self._log_prob_noisy(x, noise_std, None, num_draws, atol, rtol, method, options, hutchinson, seed,
                                    sample_offset, chunk_points, return_ess, num_probes)

    def posterior_noisy(self, x, noise_std, num_draws: int = 16, num_samples: int = 1, atol: float = 1e-5,
                        rtol: float = 1e-5, method: str = "dopri5", options: Optional[dict] = None, *,
                        hutchinson: bool = False, seed: Optional[int] = None, sample_offset: int = 0,
                        chunk_points: Optional[int] = None, num_probes: int = 1):
        """Posterior draws, mean and variance of target-space observations with Gaussian errors ``noise_std``, from the
        ``num_draws`` candidates of ``log_prob_noisy``: a ``NoisyPosterior`` (extension; see ``_posterior_noisy`` -- read
        ``ess`` before trusting ``samples``)."""
        return self._posterior_noisy(x, noise_std, None, num_draws, num_samples, atol, rtol, method, options, hutchinson,
                                     seed, sample_offset, chunk_points, num_probes)


class ConditionalODEFlow(_FlowBase):
    """Conditional flow-matching CNF (reference: flow.py:441-941)."""

    def __init__(self, target_dimension: int = 1, conditional_dimension: int = 1,
                 hidden_units: List[int] = [128, 128], activation: nn.Module = nn.SiLU,
                 target_shift: Optional[torch.Tensor] = None, target_scale: Optional[torch.Tensor] = None,
                 conditional_shift: Optional[torch.Tensor] = None,
                 conditional_scale: Optional[torch.Tensor] = None):
        super().__init__()
        self.target_dimension = target_dimension
        self.conditional_dimension = conditional_dimension
        self.layers = _build_layers(
            [target_dimension + 1 + conditional_dimension] + list(hidden_units) + [target_dimension], activation)
        self.velocity = nn.Sequential(*self.layers)
        self.register_buffer("twopi", torch.tensor(2.0 * 3.14159265358979323846))
        self.register_buffer("target_shift", target_shift if target_shift is not None else torch.zeros(target_dimension))
        self.register_buffer("target_scale", target_scale if target_scale is not None else torch.ones(target_dimension))
        self.register_buffer("conditional_shift",
                             conditional_shift if conditional_shift is not None else torch.zeros(conditional_dimension))
        self.register_buffer("conditional_scale",
                             conditional_scale if conditional_scale is not None else torch.ones(conditional_dimension))

    # -- pointwise (plain torch) ----------------------------------------------------------------
    def dynamics(self, t, states):
        x, conditional = states
        c = self._norm_cond(conditional)
        v = self.velocity(torch.cat([x, t.view(-1, 1).expand(x.shape[0], 1), c], dim=1))
        return v, torch.zeros_like(c)

    def dynamics_with_jacobian(self, t, states):
        x, conditional, logj = states
        with torch.set_grad_enabled(True):
            x.requires_grad_(True)
            v = self.dynamics(t, (x, conditional))[0]
            div = torch.zeros_like(logj)
            for i in range(x.shape[-1]):
                div = div + torch.autograd.grad(v[:, i].sum(), x, create_graph=True, retain_graph=True)[0][:, i:i + 1]
        return v, torch.zeros_like(conditional), div

    def forward(self, t, states):
        return self.dynamics(t, states)

    # -- fused ------------------------------------------------------------------------------------
    def sample(self, xT, conditional, gradients: bool = False, method: Optional[str] = None,
               options: Optional[dict] = None, atol: float = 1e-9, rtol: float = 1e-7):
        return self._sample(xT, conditional, gradients, method, options, atol, rtol)

    def solve_ode_forward(self, x, conditional, atol: float = 1e-5, rtol: float = 1e-5,
                          method: str = "dopri5", options: Optional[dict] = None, adjoint: bool = False,
                          hutchinson: bool = False, *, probe: str = "torch", seed: Optional[int] = None,
                          sample_offset: int = 0, num_probes: int = 1, return_stderr: bool = False):
        out = self._solve_ode_forward(x, conditional, atol, rtol, method, options, adjoint, hutchinson, probe, seed,
                                      sample_offset, num_probes, return_stderr)
        return out if return_stderr else out[:2]

    def log_prob(self, x, conditional, atol: float = 1e-5, rtol: float = 1e-5, method: str = "dopri5",
                 options: Optional[dict] = None, adjoint: bool = False, hutchinson: bool = False, *,
                 probe: str = "torch", seed: Optional[int] = None, sample_offset: int = 0, num_probes: int = 1,
                 return_stderr: bool = False):
        """With ``return_stderr=True`` (see ``_fused_forward``) ``(log_p [B], stderr [B])``."""
        out = self._log_prob(x, conditional, atol, rtol, method, options, adjoint, hutchinson, probe, seed, sample_offset,
                             num_probes, return_stderr)
        return out if return_stderr else out[0]

    def log_prob_grad(self, x, conditional=None, *, method: str = "rk4", options: Optional[dict] = None,
                      hutchinson: bool = False, probe: str = "torch", seed: Optional[int] = None, sample_offset: int = 0,
                      num_probes: int = 1):
        """Extension: ``(log_p [B, 1], grad_x [B, D], grad_c [B, C])``: ``log_prob`` on a fixed grid and its gradient with
        respect to ``x`` and the raw ``conditional`` (see ``_log_prob_grad``)."""
        return self._log_prob_grad(x, conditional, method, options, hutchinson, probe, seed, sample_offset, num_probes)

    def log_prob_noisy_grad(self, x, noise_std, conditional, num_draws: int = 16, *, method: str = "rk4",
                            options: Optional[dict] = None, hutchinson: bool = False, seed: Optional[int] = None,
                            sample_offset: int = 0, chunk_points: Optional[int] = None, num_probes: int = 1,
                            min_weight: float = 0.0, return_ess: bool = False, return_noise_grad: bool = False):
        """Extension: ``(log_p [B, 1], grad_x [B, D], grad_c [B, C] [, ess [B]] [, grad_noise_std [B, D]])``: ``log_prob_noisy``
        on a fixed grid and its gradient with respect to the observations, the raw ``conditional`` (the population
        hyper-parameters: ``grad_c.sum(0)`` is the gradient of the hierarchical likelihood of a catalogue that shares them)
        and the error bars (see ``_log_prob_noisy_grad``)."""
        return self._log_prob_noisy_grad(x, noise_std, conditional, num_draws, method, options, hutchinson, seed,
                                         sample_offset, chunk_points, num_probes, min_weight, return_ess, return_noise_grad)

    def log_prob_noisy(self, x, noise_std, conditional, num_draws: int = 16, atol: float = 1e-5, rtol: float = 1e-5,
                       method: str = "dopri5", options: Optional[dict] = None, *, hutchinson: bool = False,
                       seed: Optional[int] = None, sample_offset: int = 0, chunk_points: Optional[int] = None,
                       return_ess: bool = False, num_probes: int = 1):
        """Log-density [B] of target-space observations with Gaussian errors ``noise_std``, from ``num_draws`` noise draws
        per point (extension; see ``_log_prob_noisy``)."""
        return self._log_prob_noisy(x, noise_std, conditional, num_draws, atol, rtol, method, options, hutchinson, seed,
                                    sample_offset, chunk_points, return_ess, num_probes)

    def posterior_noisy(self, x, noise_std, conditional, num_draws: int = 16, num_samples: int = 1, atol: float = 1e-5,
                        rtol: float = 1e-5, method: str = "dopri5", options: Optional[dict] = None, *,
                        hutchinson: bool = False, seed: Optional[int] = None, sample_offset: int = 0,
                        chunk_points: Optional[int] = None, num_probes: int = 1):
        """Posterior draws, mean and variance of target-space observations with Gaussian errors ``noise_std`` given the raw
        ``conditional``, from the ``num_draws`` candidates of ``log_prob_noisy``: a ``NoisyPosterior`` (extension; see
        ``_posterior_noisy`` -- read ``ess`` before trusting ``samples``)."""
        return self._posterior_noisy(x, noise_std, conditional, num_draws, num_samples, atol, rtol, method, options,
                                     hutchinson, seed, sample_offset, chunk_points, num_probes)
