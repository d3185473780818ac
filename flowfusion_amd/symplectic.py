"""Symplectic flows on MI355X: the reference's ``flowfusion.symplectic`` API (``SymplecticMLP`` symplectic.py:11-122,
``SymplecticFlowModel`` :124-253) with ``sample`` and ``log_prob`` running on the library's two-network kernel.

The dynamics of a state ``[q | p]`` (2D dimensions) are ``v = [mlp_q(p, cond, t), -mlp_p(q, cond, t)]`` (:80-122): two
networks of one shape on complementary halves, so the field is divergence-free by construction and ``log_prob`` is a
state-only solve.  Each right-hand side is ONE evaluation of ``mlp_pair_kernel`` (csrc/ff_mlp_pair.hpp): net A = mlp_q,
net B = mlp_p with its output negated, both per evaluation inside one launch; the symplectic structure lives in the host
packer (``ff_mlp_pair_wpack``).  ``state_dict`` keys match the reference: ``shift``, ``scale``, ``conditional_shift``,
``conditional_scale`` (buffers, any of them may be None), ``model.W``, ``model.mlp_{q,p}_dynamics.{0,2,..}.*``.

Routes (odeint.py): ``sample`` is torchdiffeq-style fixed-grid Euler on the reference's ``linspace(1, 0, num_steps + 1)``
grid (one fused launch); ``log_prob`` is adaptive dopri5 on the device controller.  ``sample_leapfrog`` / ``log_prob_leapfrog`` (extensions;
``method="leapfrog"`` of ``_sample_from`` / ``_log_prob_from`` / ``_integrate``) integrate the same grid with
kick-drift-kick leapfrog on the row-select kernel: every sub-step moves one half of the state under the network that reads
the other half, so the discrete map preserves volume and ``log_prob_leapfrog(x, num_steps=n)`` -- the flipped grid, one
launch, no step controller -- is the exact density of what ``sample_leapfrog(shape, num_steps=n)`` applies.
``log_prob_marginal`` (extension) averages the importance weights of K momentum draws per data point -- the marginal over
the momentum that ``log_prob`` estimates from one draw -- with a streaming kernel at each end of the solve
(csrc/ff_marginal.hip); ``log_prob_marginal_grad`` (extension) adds its exact gradient with respect to the data and the
raw conditional: one forward solve, one backward launch on the rows that carry weight.  ``log_prob_marginal_noisy`` / ``log_prob_marginal_noisy_grad`` (extensions) are
the same two for an observation with known Gaussian errors: the noise is drawn jointly with the momentum
(csrc/ff_marginal_observe.hip at the two ends, the same launches between), and the gradient gains ``noise_std``.  Networks outside the compiled pair
shapes, non-SiLU activations and any other ``model`` with the same ``forward(t, state, conditional)`` are evaluated by
torch with the stepping in the library (generic.py; ``FusedEnvelopeWarning`` for the first two).  GPU only: CPU tensors
raise.  The reference draws a tqdm progress bar in ``sample``; this module does not.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from . import _native, device_adaptive, odeint, solvers
from .fused import FusedPair, MODE_STATE, activation_spec, within_envelope


class SymplecticMLP(nn.Module):
    """Two networks for the position and momentum dynamics (reference: symplectic.py:11-122).

    ``mlp_q_dynamics`` / ``mlp_p_dynamics``: ``Linear(D + C + E -> units[0])``, activation, ..., ``Linear(-> D)``, the
    same ``activation`` instance in every hidden layer of both; buffer ``W = randn(E // 2) * 16``.  Parameters are drawn
    in the reference's order (mlp_q, mlp_p, then W), so a seeded construction gives the reference's weights."""

    def __init__(self, n_data_dims, n_conditionals, embedding_dimensions, units, activation=nn.SiLU()):
        super().__init__()
        input_dim = n_data_dims + n_conditionals + embedding_dimensions
        self.mlp_q_dynamics = self._create_mlp(input_dim, n_data_dims, units, activation)
        self.mlp_p_dynamics = self._create_mlp(input_dim, n_data_dims, units, activation)
        self.register_buffer("W", torch.randn(embedding_dimensions // 2) * 16.0)

    def _create_mlp(self, input_dim, output_dim, units, activation):
        layers = []
        current = input_dim
        for unit_count in units:
            layers.append(nn.Linear(current, unit_count))
            layers.append(activation)
            current = unit_count
        layers.append(nn.Linear(current, output_dim))
        return nn.Sequential(*layers)

    def forward(self, t, state, conditional):
        """(dq/dt, dp/dt) = (mlp_q([p, cond, emb]), -mlp_p([q, cond, emb])), emb = [sin | cos]((t W) 2 pi); a 0-dim ``t``
        is expanded to the batch (plain torch, symplectic.py:80-122)."""
        q, p = torch.chunk(state, 2, dim=-1)
        if t.dim() == 0:
            t = t.expand(q.shape[0])
        t_projected = t[:, None] * self.W[None, :] * 2 * math.pi
        t_embedded = torch.cat([torch.sin(t_projected), torch.cos(t_projected)], dim=1)
        if conditional is not None:
            input_q = torch.cat([p, conditional, t_embedded], dim=1)
            input_p = torch.cat([q, conditional, t_embedded], dim=1)
        else:
            input_q = torch.cat([p, t_embedded], dim=1)
            input_p = torch.cat([q, t_embedded], dim=1)
        v_q = self.mlp_q_dynamics(input_q)
        v_p = -self.mlp_p_dynamics(input_p)
        return torch.cat([v_q, v_p], dim=-1)


class SymplecticFlowModel(nn.Module):
    """Symplectic flow: a fast sampler and an exact log-density without a divergence term (reference:
    symplectic.py:124-253).  ``shift`` / ``scale`` / ``conditional_shift`` / ``conditional_scale`` are buffers (None
    allowed, as in the reference)."""

    def __init__(self, model, shift, scale, conditional_shift, conditional_scale):
        super().__init__()
        self.model = model
        self.register_buffer("shift", shift)
        self.register_buffer("scale", scale)
        self.register_buffer("conditional_shift", conditional_shift)
        self.register_buffer("conditional_scale", conditional_scale)

    # -- public API (the reference's signatures) ------------------------------------------------
    @torch.no_grad()
    def sample(self, shape, conditional=None, num_steps=1):
        """``num_steps`` Euler steps from t = 1 to t = 0 of the joint state [q | p], started from ``randn(shape[0],
        2 shape[1])`` on the model's device; returns ``q * scale + shift`` [B, D] (symplectic.py:166-202).  No progress
        bar (the reference draws one with tqdm)."""
        device = next(self.model.parameters()).device
        x = torch.randn(shape[0], shape[1] * 2, device=device)
        return self._sample_from(x, conditional, num_steps)

    def flow_jvp(self, *args, **kwargs):
        """Flow-map sensitivities (``ODEFlow.flow_jvp``) are not built for the two-network kernels."""
        raise NotImplementedError("flow_jvp / flow_jacobian of a SymplecticFlowModel: the two-network kernels carry no tangent "
                                  f"columns -- {_native.PUSH_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")

    flow_jacobian = flow_jvp

    def flow_vjp(self, *args, **kwargs):
        """Flow-map pull-backs (``ODEFlow.flow_vjp``) are not built for the two-network kernels."""
        raise NotImplementedError("flow_vjp of a SymplecticFlowModel: the two-network kernels carry no cotangent columns -- "
                                  f"{_native.PULL_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")

    def log_prob_grad(self, *args, **kwargs):
        """Log-density gradients (``ODEFlow.log_prob_grad``) are not built for the two-network kernels."""
        raise NotImplementedError("log_prob_grad of a SymplecticFlowModel: the two-network kernels carry no adjoint columns -- "
                                  f"{_native.PULL_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")

    @torch.no_grad()
    def log_prob(self, x, conditional=None, atol=1e-5, rtol=1e-5):
        """``log N(z1) - log N(p0) - sum log scale`` with z1 the dopri5 solution over t: 0 -> 1 of [q0 | p0],
        q0 = (x - shift) / scale, p0 = randn_like(q0) (symplectic.py:204-253)."""
        p0 = torch.randn_like(x)
        return self._log_prob_from(x, p0, conditional, atol, rtol)

    # -- extensions: kick-drift-kick leapfrog.  Methods of their own: the signatures of ``sample`` / ``log_prob`` are the
    # reference's, and the golden fixtures pin them ------------------------------------------------------------------------
    @torch.no_grad()
    def sample_leapfrog(self, shape, conditional=None, num_steps=1):
        """``sample`` with ``num_steps`` leapfrog steps instead of Euler steps: the same prior draw, the same grid
        ``linspace(1, 0, num_steps + 1)``, the same return value; second order, volume-preserving and exactly invertible
        (``log_prob_leapfrog`` with the same ``num_steps`` is the density of this map)."""
        device = next(self.model.parameters()).device
        x = torch.randn(shape[0], shape[1] * 2, device=device)
        return self._sample_from(x, conditional, num_steps, method="leapfrog")

    @torch.no_grad()
    def log_prob_leapfrog(self, x, conditional=None, num_steps=None):
        """``log_prob`` with z1 the leapfrog solution on ``linspace(1, 0, num_steps + 1).flip(0)`` -- the exact inverse of
        what ``sample_leapfrog(..., num_steps)`` applies -- in one launch: no tolerances, no step controller."""
        p0 = torch.randn_like(x)
        return self._log_prob_from(x, p0, conditional, method="leapfrog", num_steps=num_steps)

    # -- extensions: derivatives through the leapfrog (odeint.solve_leapfrog_pull).  Methods of their own, as sample_leapfrog /
    # log_prob_leapfrog are: flow_jvp / flow_jacobian / flow_vjp / log_prob_grad above keep raising -------------------------
    @torch.no_grad()
    def sample_leapfrog_vjp(self, z, cotangents, conditional=None, num_steps=1, *, return_retrace=False):
        """K cotangents per sample pulled back through ``sample_leapfrog``'s map, exactly (the transpose of the discrete
        leapfrog: every row is a shear, so nothing is recorded).

        ``z`` [B, 2D] is the prior draw (the ``x`` of ``_sample_from``), ``cotangents`` [B, K, D] are in the units of the
        returned sample, K <= 15.  Returns ``(x [B, D], gz [B, K, 2D], gc [B, K, C] or None)`` -- and ``retrace [B]`` with
        ``return_retrace``: ``x`` is bitwise ``_sample_from(z, conditional, num_steps, method="leapfrog")``,
        ``gz[b, k] = cotangents[b, k]^T dx / dz`` and ``gc`` the same with respect to the raw ``conditional`` (the
        population hyper-parameters), i.e. divided by ``conditional_scale``.  The joint cotangent handed to the launch is
        ``[w * scale | 0]``.  Two launches per piece of rows; fused route only (``_native.PULL_SELECT_ENVELOPE``), no
        module-path fallback.  ``retrace``: see ``log_prob_leapfrog_grad``."""
        if int(num_steps) < 1:
            raise ValueError(f"num_steps={num_steps}: sample_leapfrog_vjp differentiates at least one leapfrog step")
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] % 2 != 0:
            raise ValueError("sample_leapfrog_vjp: z must be the prior draw [batch, 2 dim]")
        B, D = int(z.shape[0]), int(z.shape[1]) // 2
        if not torch.is_tensor(cotangents) or cotangents.dim() != 3 or tuple(cotangents.shape[::2]) != (B, D) or cotangents.shape[1] < 1:
            raise ValueError(f"sample_leapfrog_vjp: cotangents must be [{B}, K >= 1, {D}], got "
                             f"{tuple(cotangents.shape) if torch.is_tensor(cotangents) else type(cotangents).__name__}")
        cond = self._norm_cond(conditional)
        w = cotangents if self.scale is None else cotangents * self.scale
        joint = torch.cat([w, torch.zeros_like(w)], dim=-1)
        grid = torch.linspace(1.0, 0.0, int(num_steps) + 1, device=z.device).cpu()      # (built as _sample_from builds it)
        out = odeint.solve_leapfrog_pull(self, z, grid, joint, cond=cond, return_retrace=return_retrace)
        q, _ = torch.chunk(out[0], 2, dim=-1)
        x = q * self.scale + self.shift
        gc = out[2]
        if gc is not None and self.conditional_scale is not None:
            gc = gc / self.conditional_scale
        return (x, out[1], gc) + tuple(out[3:])

    @torch.no_grad()
    def log_prob_leapfrog_grad(self, x, conditional=None, num_steps=None, *, momentum=None, return_momentum_grad=False,
                               return_retrace=False):
        """``log_prob_leapfrog`` and its gradient with respect to ``x`` and the raw ``conditional`` -- what HMC / NUTS,
        L-BFGS and MAP ask of this model class.  Returns ``(log_p [B], grad_x [B, D], grad_c [B, C] or None)``, then
        ``grad_momentum [B, D]`` with ``return_momentum_grad`` and ``retrace [B]`` with ``return_retrace``.

        ``momentum=None`` draws ``torch.randn_like(x)`` as ``log_prob_leapfrog`` does; ``log_p`` is bitwise
        ``_log_prob_from(x, momentum, conditional, method="leapfrog", num_steps=num_steps)``.  The backward launch takes the
        one cotangent ``-z1`` (the gradient of ``log N(z1)``) through the transpose of the discrete leapfrog: ``grad_x =
        g_q / scale``, ``grad_momentum = g_p + momentum``, ``grad_c = gamma / conditional_scale`` -- the exact gradient of
        the returned value at fixed momentum, at any step count (no discretisation error between value and gradient).

        ``retrace[b] = max_d |z_back - z0|``, z0 = [q0 | momentum]: the backward sweep un-shears with the same network
        evaluation that gave it its slopes, so the retrace is within rounding BY CONSTRUCTION; it says nothing about the
        step count.  It exists to show a non-finite or exploding trajectory.

        Fused route only (``_native.PULL_SELECT_ENVELOPE``); Euler ``sample`` and dopri5 ``log_prob`` pull-backs, parameter
        gradients and torch.autograd integration are out of scope (the gradient of the K-draw marginal:
        ``log_prob_marginal_grad``)."""
        self._check_log_prob_method("leapfrog", num_steps)
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError("log_prob_leapfrog_grad: x must be a [batch, dim] tensor")
        if momentum is None:
            momentum = torch.randn_like(x)
        elif not torch.is_tensor(momentum) or tuple(momentum.shape) != tuple(x.shape):
            raise ValueError(f"log_prob_leapfrog_grad: momentum must be {tuple(x.shape)}, got "
                             f"{tuple(momentum.shape) if torch.is_tensor(momentum) else type(momentum).__name__}")
        D = int(x.shape[1])
        q0 = (x - self.shift) / self.scale
        cond = self._norm_cond(conditional)
        z0 = torch.cat([q0, momentum], dim=-1)
        grid = torch.linspace(1.0, 0.0, int(num_steps) + 1).flip(0)                     # (as _solve_forward builds it)
        out = odeint._solve_leapfrog_pull(self, z0, grid, lambda z1: (-z1)[:, None, :], cond, return_retrace, 1)
        z1, gz, gc = out[0], out[1][:, 0], out[2]
        normal = torch.distributions.Normal(0, 1)
        log_p = normal.log_prob(z1).sum(dim=-1) - normal.log_prob(momentum).sum(dim=-1) - torch.sum(torch.log(self.scale))
        grad_x = gz[:, :D] / self.scale
        grad_c = None
        if gc is not None:
            grad_c = gc[:, 0] if self.conditional_scale is None else gc[:, 0] / self.conditional_scale
        res = (log_p, grad_x, grad_c)
        if return_momentum_grad:
            res += (gz[:, D:] + momentum,)
        return res + tuple(out[3:])

    # -- extensions: forward-mode derivatives through the leapfrog (odeint.solve_leapfrog_push).  Methods of their own again:
    # flow_jvp / flow_jacobian above keep raising ------------------------------------------------------------------------------
    def _leapfrog_push_front_checks(self, name, z, conditional, num_steps, tangents=None, conditional_tangents=None, unit=None):
        """What both push-forward methods refuse, in one order, before anything is computed: ``num_steps``, the prior draw's
        shape, then everything ``odeint.solve_leapfrog_push`` refuses (the raw conditional has the normalised one's shape and
        dtype, so the checks see it as it is; the launch re-checks the normalised tensors).  Returns D."""
        if int(num_steps) < 1:
            raise ValueError(f"num_steps={num_steps}: {name} differentiates at least one leapfrog step")
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] % 2 != 0 or z.shape[1] < 2:
            raise ValueError(f"{name}: z must be the prior draw [batch, 2 dim]")
        odeint._leapfrog_push_checks(self, z, tangents, conditional, conditional_tangents, unit)
        return int(z.shape[1]) // 2

    @torch.no_grad()
    def sample_leapfrog_jvp(self, z, tangents=None, conditional=None, conditional_tangents=None, num_steps=1):
        """K tangents per sample pushed through ``sample_leapfrog``'s map, exactly (forward mode through the discrete
        leapfrog): the sensitivity of a sample to its prior draw and to the raw ``conditional`` (the population
        hyper-parameters) -- what a Fisher forecast or a delta-method error bar asks of this model class.

        ``z`` [B, 2D] is the prior draw (the ``x`` of ``_sample_from``); ``tangents`` [B, K, 2D] are in its units,
        ``conditional_tangents`` [B, K, C] in the units of the raw ``conditional`` (divided by ``conditional_scale`` on the
        way in); either may be None (zero), K <= 15.  Returns ``(x [B, D], dx [B, K, D])``: ``x`` is bitwise
        ``_sample_from(z, conditional, num_steps, method="leapfrog")``, ``dx[b, k] = dx / d(z, conditional) . (tangents[b, k],
        conditional_tangents[b, k])`` in the units of the sample (``dq * scale``).  One launch per piece of rows; fused route
        only (``_native.PUSH_SELECT_ENVELOPE``), no module-path fallback, no depth ceiling."""
        D = self._leapfrog_push_front_checks("sample_leapfrog_jvp", z, conditional, num_steps, tangents, conditional_tangents)
        cond = self._norm_cond(conditional)
        grid = torch.linspace(1.0, 0.0, int(num_steps) + 1, device=z.device).cpu()      # (built as _sample_from builds it)
        zo, dz = odeint._solve_leapfrog_push(self, z, grid, tangents, cond, conditional_tangents, None, self.conditional_scale)
        q, _ = torch.chunk(zo, 2, dim=-1)
        return q * self.scale + self.shift, dz[:, :, :D] * self.scale

    @torch.no_grad()
    def sample_leapfrog_jacobian(self, z, conditional=None, num_steps=1):
        """The whole Jacobian of ``sample_leapfrog``'s map: ``(x [B, D], J_z [B, D, 2D], J_c [B, D, C] or None)``,
        ``J_z[b, i, j] = dx_i / dz_j`` and ``J_c[b, i, j] = dx_i / d conditional_j`` for the raw ``conditional``, from unit
        tangents in ceil((2D + C) / 15) launches per piece of rows (``sample_leapfrog_vjp`` needs D cotangents for the same:
        see README for which route to use when).  ``x`` is bitwise ``_sample_from(z, conditional, num_steps,
        method="leapfrog")``."""
        D = self._leapfrog_push_front_checks("sample_leapfrog_jacobian", z, conditional, num_steps, unit=(0, 1))
        cond = self._norm_cond(conditional)
        grid = torch.linspace(1.0, 0.0, int(num_steps) + 1, device=z.device).cpu()
        zo, Jz, Jc = odeint.solve_leapfrog_push_jacobian(self, z, grid, cond=cond)
        q, _ = torch.chunk(zo, 2, dim=-1)
        scale = self.scale if self.scale.dim() == 0 else self.scale[:, None]
        Jz = Jz[:, :D] * scale
        if Jc is not None:
            Jc = Jc[:, :D] * scale
            if self.conditional_scale is not None:
                Jc = Jc / self.conditional_scale
        return q * self.scale + self.shift, Jz, Jc

    # -- with the random draws supplied (tests feed the reference's draws) ----------------------------
    def _norm_cond(self, conditional):
        if conditional is None:
            return None
        return (conditional - self.conditional_shift) / self.conditional_scale

    SAMPLE_METHODS = ("euler", "leapfrog")

    @torch.no_grad()
    def _integrate(self, z, time_steps, conditional_normalised=None, method="euler"):
        """The whole state [B, 2D] after integrating ``z`` over the nodes ``time_steps`` (either direction) with the
        fixed-grid ``method``: ``"euler"`` (torchdiffeq's, on the pair kernel) or ``"leapfrog"`` (kick-drift-kick on the
        row-select kernel; odeint.solve_leapfrog)."""
        if method not in self.SAMPLE_METHODS:
            raise ValueError(f"method={method!r}: the fixed-grid methods of a symplectic flow are 'euler' and 'leapfrog'")
        time_steps = time_steps.detach().to("cpu", torch.float32)
        if method == "leapfrog":
            return odeint.solve_leapfrog(self, z, time_steps, cond=conditional_normalised)
        z, _ = odeint.solve(self, z, time_steps, "euler", None, MODE_STATE, None, None, cond=conditional_normalised)
        return z

    @torch.no_grad()
    def _sample_from(self, x, conditional=None, num_steps=1, *, method="euler"):
        """``sample`` from the prior draw ``x`` [B, 2D]: the reference's grid ``linspace(1, 0, num_steps + 1)`` built on the
        state's device, ``x + v(t_k, x) (t_{k+1} - t_k)`` per step -- torchdiffeq's fixed-grid Euler on that grid -- or
        leapfrog steps on the same grid."""
        if method not in self.SAMPLE_METHODS:
            raise ValueError(f"method={method!r}: sample takes 'euler' or 'leapfrog'")
        conditional = self._norm_cond(conditional)
        time_steps = torch.linspace(1.0, 0.0, num_steps + 1, device=x.device)
        if num_steps > 0:
            x = self._integrate(x, time_steps.cpu(), conditional, method)
        q, _ = torch.chunk(x, 2, dim=-1)
        return q * self.scale + self.shift

    def _check_log_prob_method(self, method, num_steps):
        if method == "leapfrog":
            if num_steps is None or int(num_steps) < 1:
                raise ValueError("method='leapfrog' needs num_steps >= 1 (the steps of the sample it inverts)")
        elif num_steps is not None:
            raise ValueError(f"num_steps belongs to method='leapfrog'; method={method!r} chooses its own steps")
        elif method not in solvers.FIXED_METHODS and method not in solvers.ADAPTIVE_METHODS:
            raise ValueError(f"method={method!r}: log_prob takes 'dopri5' (the default), 'leapfrog' with num_steps, or another "
                             f"torchdiffeq method ({sorted(solvers.FIXED_METHODS)}, {solvers.ALL_ADAPTIVE})")

    def _solve_forward(self, z0, conditional_normalised, atol, rtol, method, options, num_steps):
        """z1 [B, 2D]: the solve of ``log_prob`` over t: 0 -> 1 from ``z0`` (``method`` already checked): the flipped grid
        of ``sample`` under leapfrog, ``odeint.solve`` on t_span = [0, 1] otherwise."""
        if method == "leapfrog":
            grid = torch.linspace(1.0, 0.0, int(num_steps) + 1).flip(0)
            return self._integrate(z0, grid, conditional_normalised, "leapfrog")
        t_span = torch.tensor([0.0, 1.0])
        z1, _ = odeint.solve(self, z0, t_span, method, options, MODE_STATE, atol, rtol, cond=conditional_normalised)
        return z1

    @torch.no_grad()
    def _log_prob_from(self, x, p0, conditional=None, atol=1e-5, rtol=1e-5, method="dopri5", options=None, *,
                       num_steps=None):
        """``log_prob`` with the momentum draw ``p0`` supplied; ``method`` / ``options`` as torchdiffeq takes them (the
        reference always runs its default, dopri5), or ``method="leapfrog"`` with ``num_steps``: the flipped grid of
        ``sample``, no tolerances."""
        self._check_log_prob_method(method, num_steps)
        q0 = (x - self.shift) / self.scale
        conditional = self._norm_cond(conditional)
        z0 = torch.cat([q0, p0], dim=-1)
        z1 = self._solve_forward(z0, conditional, atol, rtol, method, options, num_steps)
        normal = torch.distributions.Normal(0, 1)
        log_p_z1 = normal.log_prob(z1).sum(dim=-1)
        log_p_p0 = normal.log_prob(p0).sum(dim=-1)
        return log_p_z1 - log_p_p0 - torch.sum(torch.log(self.scale))

    # -- extension: the marginal over K momentum draws ------------------------------------------------------------------
    MARGINAL_CHUNK_ROWS = 1 << 22        # rows (data points x momenta) in flight by default on a fixed grid

    @torch.no_grad()
    def log_prob_marginal(self, x, conditional=None, num_momenta=16, atol=1e-5, rtol=1e-5, *, method="dopri5",
                          num_steps=None, options=None, seed=None, sample_offset=0, chunk_points=None, return_ess=False):
        """The data log-density as the marginal over the momentum, from ``num_momenta`` = K draws per point.

        The flow preserves volume in [q | p], so p(q0) = E_{p0 ~ N}[N(z1(q0, p0)) / N(p0)]; ``log_prob`` returns the
        one-draw estimate of it in log space (a different value on every call), this returns
        ``logsumexp_k(log N(z1_k) - log N(p0_k)) - log K - sum log scale`` [B]: ff_marginal_expand writes the K starting
        states of every point, the solve of ``log_prob`` (``method`` / ``num_steps`` / ``options`` / ``atol`` / ``rtol`` as
        in ``_log_prob_from``; compiled shapes and the module route alike) runs on the B K rows, ff_marginal_reduce
        combines them in double.  The momenta come from the library's counter-based stream keyed by ``seed`` and the global
        row ``sample_offset + r`` (noise indices FF_MOMENTUM_NOISE_BASE + k): an explicit ``seed`` makes the call
        reproducible, ``seed=None`` draws a 63-bit one from torch's default generator (``torch.manual_seed`` governs it).
        ``return_ess=True`` returns ``(log_p, ess)``, ess [B] the effective sample size of the K weights, in (0, K].

        Memory: on a fixed grid (``method="leapfrog"`` or a fixed-grid torchdiffeq method) the points are processed in
        chunks of ``chunk_points`` (default: ``chunk_points * K <= 2**22`` rows), each expand -> solve -> reduce into the
        one output; rows do not depend on the batch they sit in, so the result is bitwise independent of ``chunk_points``
        (and of a sharding that passes ``sample_offset`` = its first row).  An adaptive method controls its step from the
        whole batch it is handed: all B K rows are one solve, and ``chunk_points`` raises."""
        K = int(num_momenta)
        if not 1 <= K <= _native.MAX_MOMENTA:
            raise ValueError(f"num_momenta={num_momenta}: 1 .. {_native.MAX_MOMENTA} momentum draws per data point")
        self._check_log_prob_method(method, num_steps)
        chunk = self._marginal_chunk(int(x.shape[0]), K, method, chunk_points, "num_momenta")
        return self._marginal_value(x, None, conditional, K, atol, rtol, method, num_steps, options, seed, sample_offset, chunk,
                                    return_ess)

    def _marginal_chunk(self, B, K, method, chunk_points, draws):
        """Data points per chunk of ``log_prob_marginal`` / ``log_prob_marginal_noisy`` (``method`` already checked): the whole
        batch under an adaptive method, where ``chunk_points`` raises; ``draws``: the caller's name for K."""
        if method != "leapfrog" and method not in solvers.FIXED_METHODS:
            if chunk_points is not None:
                raise ValueError(f"chunk_points with method={method!r}: an adaptive solve takes its step size from the error "
                                 f"norm of the whole batch, so chunks would change every row's steps; all B * {draws} rows "
                                 "are one solve.  method='leapfrog' with num_steps (a fixed grid) processes chunks with "
                                 "bitwise the same result")
            return max(B, 1)
        if chunk_points is None:
            return max(1, self.MARGINAL_CHUNK_ROWS // K)
        chunk = int(chunk_points)
        if chunk < 1:
            raise ValueError(f"chunk_points={chunk_points}: at least one data point per chunk")
        return chunk

    def _marginal_value(self, x, std, conditional, K, atol, rtol, method, num_steps, options, seed, sample_offset, chunk,
                        return_ess):
        """The chunk loop of ``log_prob_marginal`` (``std`` None: ff_marginal_expand) and ``log_prob_marginal_noisy`` (``std``
        the tensor of ``odeint.noise_std_tensor``: ff_marginal_observe_expand): expand -> solve -> ff_marginal_reduce."""
        B = int(x.shape[0])
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed, first = int(seed), int(sample_offset)
        x = x.contiguous()
        cond = self._norm_cond(conditional)
        cond = None if cond is None else cond.contiguous()
        log_det = 0.0 if self.scale is None else float(torch.log(self.scale.double()).sum())
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        ess = torch.empty(B, dtype=torch.float32, device=x.device) if return_ess else None
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            ck = None if cond is None else cond[lo:hi]
            if std is None:
                z0, ck = _native.marginal_expand(x[lo:hi], K, seed, first + lo, self.shift, self.scale, ck)
            else:
                z0, ck = _native.marginal_observe_expand(x[lo:hi], std if std.dim() == 1 else std[lo:hi], K, seed, first + lo,
                                                         _native.f32_on(self.shift, x.device), _native.f32_on(self.scale, x.device), ck)
            z1 = self._solve_forward(z0, ck, atol, rtol, method, options, num_steps)
            del z0
            _native.marginal_reduce(z1, K, seed, first + lo, log_det, out[lo:hi], None if ess is None else ess[lo:hi])
            del z1
        return (out, ess) if return_ess else out

    @torch.no_grad()
    def log_prob_marginal_grad(self, x, conditional=None, num_momenta=16, *, method="leapfrog", num_steps=None, seed=None,
                               sample_offset=0, chunk_points=None, min_weight=0.0, return_ess=False):
        """``log_prob_marginal(..., method="leapfrog")`` and its gradient with respect to ``x`` and the raw ``conditional``
        (the population hyper-parameters): what a hierarchical fit asks of this model class.  Returns ``(log_p [B], grad_x
        [B, D], grad_c [B, C] or None)``, then ``ess [B]`` with ``return_ess``; ``log_p`` and ``ess`` are bitwise
        ``log_prob_marginal(x, conditional, num_momenta, method="leapfrog", num_steps=num_steps, seed=seed,
        sample_offset=sample_offset, return_ess=True)``.

        With the momenta ``p_k`` of the counter-based stream fixed, ``lw_k = log N(z1_k) - log N(p_k)`` and ``wn_k = exp(lw_k -
        max lw) / W`` (double), the gradient of ``logsumexp_k lw_k - log K - sum log scale`` is ``sum_k wn_k g_q,k / scale`` for
        ``x`` and ``sum_k wn_k gamma_k / conditional_scale`` for ``conditional``, ``(g_q,k | g_p,k)`` and ``gamma_k`` the
        pull-back of the one cotangent ``-z1_k`` through the transpose of the discrete leapfrog (``g_p`` is not needed: the
        momenta are constants of the estimate) -- the exact gradient of the returned value at that seed, at any step count.

        Per chunk of points (the chunk rule and the seed rule of ``log_prob_marginal``): ff_marginal_expand -> ONE forward
        ``solve_leapfrog`` of the rows -> ff_marginal_weigh (``log_p``, ``ess``, the rows' ``lw`` in double and which rows are
        kept) -> the kept rows of ``z1`` and the conditional gathered in order -> ``odeint._leapfrog_pull_from`` from ``z1``
        itself (no second forward solve) -> ff_marginal_grad_reduce.  Draw k is kept iff ``wn_k > 0`` and ``wn_k >=
        min_weight``; the sums take the weights of the FULL ``W``, not renormalised, so ``min_weight`` = m > 0 truncates the
        gradient by at most ``K m max |grad lw|``.  A point with a NaN among its ``lw``, or with ``W = 0``, has NaN gradients.
        Rows and points are independent: any ``chunk_points``, and any slice of the batch at its ``sample_offset``, gives
        bitwise the same.  ``self.last_marginal_grad_stats``: ``rows`` (B K), ``rows_kept`` (what reached the backward
        launch) and ``launches`` (``{"forward", "backward"}``: one each per piece of rows).

        Refused before the device is touched, in this order: ``num_momenta``, ``min_weight``, ``chunk_points`` (ValueError);
        a ``method`` other than ``"leapfrog"`` (ValueError); ``num_steps`` missing or < 1 (ValueError); then every refusal of
        the leapfrog pull-backs (``odeint._leapfrog_pull_checks``).  Fused route only (``_native.PULL_SELECT_ENVELOPE``), no
        module-path fallback; adaptive, Euler and dopri5 marginals, a momentum gradient, parameter gradients and torch.autograd
        integration are out of scope."""
        K = int(num_momenta)
        if not 1 <= K <= _native.MAX_MOMENTA:
            raise ValueError(f"num_momenta={num_momenta}: 1 .. {_native.MAX_MOMENTA} momentum draws per data point")
        m = float(min_weight)
        if not 0.0 <= m < 1.0:
            raise ValueError(f"min_weight={min_weight}: a normalised weight, 0 <= min_weight < 1 (0 keeps every draw of non-zero "
                             "weight)")
        if chunk_points is not None and int(chunk_points) < 1:
            raise ValueError(f"chunk_points={chunk_points}: at least one data point per chunk")
        if method != "leapfrog":
            raise ValueError(f"log_prob_marginal_grad: method={method!r}: Euler and dopri5 rows are not shears, so their pull-back "
                             "needs a record of the stage states, which the two-network kernels do not keep; use "
                             "method=\"leapfrog\" with num_steps (every row a shear: the exact gradient of the value it returns)")
        self._check_log_prob_method("leapfrog", num_steps)
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError("log_prob_marginal_grad: x must be a [batch, dim] tensor")
        B, D = int(x.shape[0]), int(x.shape[1])
        # (shapes, dtypes and devices only: the raw conditional and an unwritten joint state stand in for the rows)
        _, _, _, _, C = odeint._leapfrog_pull_checks(self, x.new_empty((B, 2 * D)), lambda z1: None, conditional, 1)
        out, gx, gcond, ess, _, stats = self._marginal_grad_chunks(x, None, conditional, K, m, num_steps, seed, sample_offset,
                                                                   chunk_points, C, return_ess, False)
        self.last_marginal_grad_stats = stats
        return (out, gx, gcond) + ((ess,) if return_ess else ())

    def _marginal_grad_chunks(self, x, std, conditional, K, m, num_steps, seed, sample_offset, chunk_points, C, return_ess,
                              return_noise_grad):
        """The chunk loop of ``log_prob_marginal_grad`` (``std`` None: ff_marginal_expand, ff_marginal_grad_reduce) and
        ``log_prob_marginal_noisy_grad`` (``std`` the tensor of ``odeint.noise_std_tensor``: ff_marginal_observe_expand, and
        ff_marginal_observe_grad_reduce where the gradient with respect to it is wanted), everything checked by the caller:
        expand -> one forward ``solve_leapfrog`` -> ff_marginal_weigh -> the kept rows gathered -> one
        ``odeint._leapfrog_pull_from`` from ``z1`` itself -> reduce.  Returns ``(log_p, grad_x, grad_c or None, ess or None,
        grad_noise_std or None, stats)``."""
        B, D = int(x.shape[0]), int(x.shape[1])
        chunk = max(1, self.MARGINAL_CHUNK_ROWS // K) if chunk_points is None else int(chunk_points)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed, first = int(seed), int(sample_offset)
        x = x.contiguous()
        cond = self._norm_cond(conditional)
        cond = None if cond is None else cond.contiguous()
        log_det = 0.0 if self.scale is None else float(torch.log(self.scale.double()).sum())
        scale = _native.f32_on(self.scale, x.device)
        shift = None if std is None else _native.f32_on(self.shift, x.device)
        cscale = _native.f32_on(self.conditional_scale, x.device) if C > 0 else None
        new = lambda cols: torch.empty(B, cols, dtype=torch.float32, device=x.device)
        out, ess = new(1).view(B), (new(1).view(B) if return_ess else None)
        gx, gcond = new(D), (new(C) if C > 0 else None)
        gstd = new(D) if (std is not None and return_noise_grad) else None
        grid = torch.linspace(1.0, 0.0, int(num_steps) + 1).flip(0)                     # (as _solve_forward builds it)
        kept = forward = backward = 0
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            ck = None if cond is None else cond[lo:hi]
            std_c = None if std is None else (std if std.dim() == 1 else std[lo:hi])
            if std is None:
                z0, ck = _native.marginal_expand(x[lo:hi], K, seed, first + lo, self.shift, self.scale, ck)
            else:
                z0, ck = _native.marginal_observe_expand(x[lo:hi], std_c, K, seed, first + lo, shift, scale, ck)
            z1 = self._solve_forward(z0, ck, None, None, "leapfrog", None, num_steps)
            forward += int(self.last_solver_stats["launches"])
            del z0
            _, lw, keep = _native.marginal_weigh(z1, K, seed, first + lo, log_det, m, out[lo:hi],
                                                 None if ess is None else ess[lo:hi])
            rows = torch.nonzero(keep).view(-1)                 # the kept rows in order: row_of is their rank
            n = int(rows.numel())
            row_of = torch.where(keep > 0, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
            if n == 0:
                gz, gc = z1.new_zeros(0, 2 * D), (None if C == 0 else z1.new_zeros(0, C))
            else:
                take = lambda t: None if t is None else (t if n == t.shape[0] else t.index_select(0, rows))
                zk = take(z1)
                _, gz, gc = odeint._leapfrog_pull_from(self, zk, grid, (-zk)[:, None, :], take(ck))
                backward += int(self.last_solver_stats["launches"])
                gz, gc = gz[:, 0], (None if gc is None else gc[:, 0])
                del zk
            kept += n
            if gstd is None:
                _native.marginal_grad_reduce(lw, row_of, gz, gc, K, scale, cscale, gx[lo:hi],
                                             None if gcond is None else gcond[lo:hi])
            else:
                _native.marginal_observe_grad_reduce(lw, row_of, gz, gc, std_c, K, seed, first + lo, scale, cscale, True,
                                                     gx[lo:hi], None if gcond is None else gcond[lo:hi], gstd[lo:hi])
            del z1, ck, lw, keep, gz, gc
        stats = {"rows": B * K, "rows_kept": kept, "launches": {"forward": forward, "backward": backward}}
        return out, gx, gcond, ess, gstd, stats

    # -- extension: the marginal of NOISY observations, K joint (noise, momentum) draws per point -------------------------------
    # Names of their own: ``log_prob_noisy`` / ``posterior_noisy`` / ``log_prob_noisy_grad`` of the single-network classes
    # wrap a model's own log-density; here the noise draw joins the momentum draw of the marginal itself.
    def _marginal_noisy_front_checks(self, what, x, noise_std, num_draws, chunk_points, method, num_steps, grad, min_weight=0.0):
        """What both noisy-marginal methods refuse before the device is touched, in one order: ``num_draws``, ``min_weight``,
        ``chunk_points``; the gradient's ``method``; ``num_steps``; ``x``; ``noise_std``.  Returns ``(K, min_weight, std)``."""
        K = int(num_draws)
        if not 1 <= K <= _native.MAX_MOMENTA:
            raise ValueError(f"num_draws={num_draws}: 1 .. {_native.MAX_MOMENTA} joint (noise, momentum) draws per data point")
        m = float(min_weight)
        if not 0.0 <= m < 1.0:
            raise ValueError(f"min_weight={min_weight}: a normalised weight, 0 <= min_weight < 1 (0 keeps every draw of non-zero "
                             "weight)")
        if chunk_points is not None and int(chunk_points) < 1:
            raise ValueError(f"chunk_points={chunk_points}: at least one data point per chunk")
        if grad and method != "leapfrog":
            raise ValueError(f"{what}: method={method!r}: Euler and dopri5 rows are not shears, so their pull-back "
                             "needs a record of the stage states, which the two-network kernels do not keep; use "
                             "method=\"leapfrog\" with num_steps (every row a shear: the exact gradient of the value it returns)")
        self._check_log_prob_method(method, num_steps)
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError(f"{what}: x must be a [batch, dim] float32 tensor")
        return K, m, odeint.noise_std_tensor(noise_std, x)

    @torch.no_grad()
    def log_prob_marginal_noisy(self, x, noise_std, conditional=None, num_draws=16, atol=1e-5, rtol=1e-5, *, method="dopri5",
                                num_steps=None, options=None, seed=None, sample_offset=0, chunk_points=None, return_ess=False):
        """The log-density of a NOISY observation ``x = x_true + n``, ``n ~ N(0, diag noise_std^2)``, as the marginal over
        noise and momentum, from ``num_draws`` = K joint draws per point: ``log_p [B]`` (``(log_p, ess)`` with ``return_ess``).

        Draw k of point r is the noise ``z_k`` and the momentum ``p_k`` of the counter-based stream, both keyed by ``seed`` and
        the global row ``sample_offset + r`` (noise indices FF_OBS_NOISE_BASE + k and FF_MOMENTUM_NOISE_BASE + k); its row
        starts at ``[((x - noise_std z_k) - shift) / scale | p_k]`` (ff_marginal_observe_expand).  The flow preserves volume
        in [q | p], so ``p_obs(x | noise_std) = E_{z,p}[N(z1) / N(p)] / prod scale`` and the estimate is ``logsumexp_k(log
        N(z1_k) - log N(p_k)) - log K - sum log scale``: ff_marginal_reduce, unchanged.  ``noise_std``: [B, D], [D] or a
        scalar, in the units of ``x``, finite and >= 0 (``odeint.noise_std_tensor``); with ``noise_std = 0`` the result is
        bitwise ``log_prob_marginal`` at the same seed.  The loop, chunk rule, seed rule and adaptive rule are
        ``log_prob_marginal``'s: on a fixed grid (``method="leapfrog"`` with ``num_steps``) any ``chunk_points`` and any slice
        of the batch at its ``sample_offset`` give bitwise the same; an adaptive method solves all B K rows at once and
        ``chunk_points`` raises."""
        K, _, std = self._marginal_noisy_front_checks("log_prob_marginal_noisy", x, noise_std, num_draws, chunk_points, method,
                                                      num_steps, False)
        chunk = self._marginal_chunk(int(x.shape[0]), K, method, chunk_points, "num_draws")
        return self._marginal_value(x, std, conditional, K, atol, rtol, method, num_steps, options, seed, sample_offset, chunk,
                                    return_ess)

    @torch.no_grad()
    def log_prob_marginal_noisy_grad(self, x, noise_std, conditional=None, num_draws=16, *, method="leapfrog", num_steps=None,
                                     seed=None, sample_offset=0, chunk_points=None, min_weight=0.0, return_ess=False,
                                     return_noise_grad=False):
        """``log_prob_marginal_noisy(..., method="leapfrog")`` and its gradient with respect to the observation ``x``, the raw
        ``conditional`` (the population hyper-parameters) and, with ``return_noise_grad``, ``noise_std``: what a hierarchical
        fit of data with error bars differentiates.  Returns ``(log_p [B], grad_x [B, D], grad_c [B, C] or None)``, then
        ``ess [B]`` with ``return_ess``, then ``grad_noise_std [B, D]`` with ``return_noise_grad`` (per object and dimension,
        whatever the layout of ``noise_std``); ``log_p`` and ``ess`` are bitwise the value method's.

        With the draws fixed, ``wn_k = exp(lw_k - max lw) / W`` (double) and ``(g_q,k | g_p,k)``, ``gamma_k`` the pull-back of
        the one cotangent ``-z1_k`` through the transposed leapfrog: ``grad_x = sum_k wn_k g_q,k / scale``, ``grad_c = sum_k
        wn_k gamma_k / conditional_scale``, ``grad_noise_std = -sum_k wn_k z_k g_q,k / scale`` -- the exact gradient of the
        returned value at that seed, at any step count.  Per chunk of points: ff_marginal_observe_expand -> ONE forward
        ``solve_leapfrog`` -> ff_marginal_weigh -> the kept rows gathered in order -> ONE ``odeint._leapfrog_pull_from`` from
        ``z1`` itself -> ff_marginal_grad_reduce, or ff_marginal_observe_grad_reduce with ``return_noise_grad`` (the same
        ``grad_x`` and ``grad_c`` bit for bit).  ``min_weight``, the kept rows, degenerate points and the independence of
        chunks and slices are ``log_prob_marginal_grad``'s; with ``noise_std = 0`` every output it shares with that method is
        bitwise that method's.  ``self.last_marginal_noisy_grad_stats``: ``rows`` (B K), ``rows_kept`` and ``launches``
        (``{"forward", "backward"}``).

        Refused before the device is touched, in this order: ``num_draws``, ``min_weight``, ``chunk_points`` (ValueError); a
        ``method`` other than ``"leapfrog"`` (ValueError); ``num_steps`` missing or < 1; ``x`` not [B, D] float32;
        ``noise_std`` (shape, finite, >= 0); then every refusal of the leapfrog pull-backs
        (``odeint._leapfrog_pull_checks``).  Fused route only (``_native.PULL_SELECT_ENVELOPE``), no module-path fallback;
        adaptive, Euler and dopri5 gradients, a momentum gradient, a posterior, parameter gradients and torch.autograd
        integration are out of scope."""
        K, m, std = self._marginal_noisy_front_checks("log_prob_marginal_noisy_grad", x, noise_std, num_draws, chunk_points,
                                                      method, num_steps, True, min_weight)
        B, D = int(x.shape[0]), int(x.shape[1])
        # (shapes, dtypes and devices only: the raw conditional and an unwritten joint state stand in for the rows)
        _, _, _, _, C = odeint._leapfrog_pull_checks(self, x.new_empty((B, 2 * D)), lambda z1: None, conditional, 1)
        out, gx, gcond, ess, gstd, stats = self._marginal_grad_chunks(x, std, conditional, K, m, num_steps, seed, sample_offset,
                                                                      chunk_points, C, return_ess, return_noise_grad)
        self.last_marginal_noisy_grad_stats = stats
        return (out, gx, gcond) + ((ess,) if return_ess else ()) + ((gstd,) if return_noise_grad else ())

    @torch.no_grad()
    def posterior_marginal_noisy(self, x, noise_std, conditional=None, num_draws=16, num_samples=1, atol=1e-5, rtol=1e-5, *,
                                 method="dopri5", num_steps=None, options=None, seed=None, sample_offset=0, chunk_points=None):
        """The per-object posterior ``p(x_true | x, noise_std) ~ p(x_true) N(x; x_true, diag noise_std^2)`` of NOISY
        observations ``x`` [B, D], from the ``num_draws`` = K joint draws that ``log_prob_marginal_noisy`` makes and drops: an
        ``odeint.NoisyPosterior(samples [B, M, D], log_prob [B], ess [B], mean [B, D], var [B, D], index [B, M])``.

        Candidate k of point r is ``y_k = x - noise_std z_k`` and its weight ``w_k = N(z1_k) / N(p_k)``.  The flow preserves
        volume in [q | p], so ``w_k`` is an unbiased ONE-MOMENTUM estimate of ``p(y_k)``, not ``p(y_k)`` itself: the K rows are
        a pseudo-marginal, self-normalised importance sample of the posterior (the momentum is integrated out by the same
        average that integrates out the noise).  ``samples`` are M = ``num_samples`` multinomial draws of the candidates by
        their weights, in the units of ``x``; ``index`` [B, M] int32 says which candidate each is; ``mean`` -- the de-noised
        ("shrunk") value of each object under the learned population -- and ``var`` are the weighted mean and variance of the
        candidates, in double; ``log_prob`` and ``ess`` are bitwise ``log_prob_marginal_noisy(..., return_ess=True)`` at the same
        seed.

        The samples are a RESAMPLE of K particles: only as many distinct points as the effective sample size allows.  Read
        ``ess`` before trusting ``samples``, and raise ``num_draws``, not ``num_samples``, to get more of them.

        Arguments, chunk rule, seed rule and adaptive rule are ``log_prob_marginal_noisy``'s.  Per chunk of points:
        ff_marginal_observe_expand -> the solve of ``log_prob`` -> ff_marginal_weigh with ``min_weight = 0`` (``log_prob``,
        ``ess`` and the rows' ``lw`` in double) -> ff_marginal_observe_resample, which regenerates the candidates from the
        counter-based stream instead of reading a particle buffer (uniforms under the same ``seed`` and global row,
        FF_OBS_RESAMPLE_NOISE_INDEX).  On a fixed grid (``method="leapfrog"`` with ``num_steps``) every field is bitwise
        independent of ``chunk_points`` and of slicing the batch at its ``sample_offset``; an adaptive method solves all B K
        rows at once and ``chunk_points`` raises.  A point with a NaN among its ``lw``, or with no draw above -inf, has
        ``index = -1`` and NaN in ``samples``, ``mean`` and ``var``.

        Refused before the device is touched, in this order: ``num_draws``, ``num_samples`` (0 .. 4096), ``chunk_points``
        (ValueError); ``method`` / ``num_steps``; ``x`` not [B, D] float32; ``noise_std`` (shape, finite, >= 0).  A posterior over
        the momentum, gradients of the posterior and MCMC refinement of low-ESS objects are out of scope."""
        M = int(num_samples)
        # (a bad num_draws is the front checks' to refuse, first)
        if 1 <= int(num_draws) <= _native.MAX_MOMENTA and not 0 <= M <= _native.MAX_OBS_SAMPLES:
            raise ValueError(f"num_samples={num_samples}: 0 .. {_native.MAX_OBS_SAMPLES} posterior draws per data point")
        K, _, std = self._marginal_noisy_front_checks("posterior_marginal_noisy", x, noise_std, num_draws, chunk_points, method,
                                                      num_steps, False)
        B, D = int(x.shape[0]), int(x.shape[1])
        chunk = self._marginal_chunk(B, K, method, chunk_points, "num_draws")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        seed, first = int(seed), int(sample_offset)
        x = x.contiguous()
        cond = self._norm_cond(conditional)
        cond = None if cond is None else cond.contiguous()
        log_det = 0.0 if self.scale is None else float(torch.log(self.scale.double()).sum())
        shift, scale = _native.f32_on(self.shift, x.device), _native.f32_on(self.scale, x.device)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
        out, ess, mean, var, samples = new(B), new(B), new(B, D), new(B, D), new(B, M, D)
        index = torch.empty(B, M, dtype=torch.int32, device=x.device)
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            std_c = std if std.dim() == 1 else std[lo:hi]
            z0, ck = _native.marginal_observe_expand(x[lo:hi], std_c, K, seed, first + lo, shift, scale,
                                                     None if cond is None else cond[lo:hi])
            z1 = self._solve_forward(z0, ck, atol, rtol, method, options, num_steps)
            del z0, ck
            _, lw, _ = _native.marginal_weigh(z1, K, seed, first + lo, log_det, 0.0, out[lo:hi], ess[lo:hi])
            del z1
            _native.marginal_observe_resample(x[lo:hi], std_c, lw, K, M, seed, first + lo, samples[lo:hi], index[lo:hi],
                                              mean[lo:hi], var[lo:hi])
            del lw
        return odeint.NoisyPosterior(samples, out, ess, mean, var, index)

    # -- what odeint.solve asks of a front end -------------------------------------------------------
    def _layers(self):
        m = self.model
        return list(m.mlp_q_dynamics), list(m.mlp_p_dynamics)

    def _fusable(self) -> bool:
        """The dynamics are a SymplecticMLP whose two networks a compiled pair kernel holds (shape, SiLU).  Another
        module with the same ``forward(t, state, conditional)`` is stepped by generic.py; so is a SymplecticMLP outside
        the compiled shapes or with another activation (with a ``FusedEnvelopeWarning``)."""
        if not isinstance(self.model, SymplecticMLP):
            return False
        q, p = self._layers()
        key = tuple(id(l) for l in q + p) + tuple(repr(l) for l in q + p if not isinstance(l, nn.Linear))
        return within_envelope(self, key, self._net, modes=(MODE_STATE,))

    def _net(self) -> FusedPair:
        m = self.model
        q, p = self._layers()
        acts = {activation_spec(l) for l in q + p if not isinstance(l, nn.Linear)}
        if acts != {(_native.ACT_SILU, 0.0, 0.0)}:
            raise NotImplementedError(f"activations {sorted(acts)}: the two-network kernels are compiled for SiLU only")
        ql = [l for l in q if isinstance(l, nn.Linear)]
        pl = [l for l in p if isinstance(l, nn.Linear)]
        cached = self.__dict__.get("_fused")
        if cached is None or not cached.serves(ql, (_native.ACT_SILU, 0.0, 0.0), "f32", pl):
            D = int(ql[-1].out_features)
            E = 2 * int(m.W.numel())
            C = int(ql[0].in_features) - D - E
            # first-layer columns of each network: [its half of the state (D) | cond (C) | time features (E)]
            cached = FusedPair(ql, pl, 2 * D, C, x_col0=0, c_col0=D)
            object.__setattr__(self, "_fused", cached)
        return cached

    def _time_cols(self):
        net = self._net()
        D, C = net.dim // 2, net.cond_dim
        return D + C, D + C + 2 * int(self.model.W.numel())

    def _device_schedule(self, device):
        """``device_adaptive.ScheduleSpec`` of the device controller: a = 0, b = 1, c1 = [sin | cos]((t W) 2 pi) through
        both first layers' time columns (FF_SCHED_FOURIER), stacked [net A | net B]."""
        m = self.model
        if m.W.numel() == 0:
            return None
        c0, c1 = self._time_cols()
        w0t, b0 = self._net().time_columns(device, c0, c1)
        emb_w = m.W.detach().to(device, torch.float32).contiguous()
        return device_adaptive.ScheduleSpec(_native.SCHED_FOURIER, (0.0, 0.0, 0.0), True, emb_w, math.pi, w0t, b0)

    def _schedule_inputs(self):
        """Host copies of what ``_schedule`` reads: W and both first layers (taken once per solve)."""
        return (self.model.W.detach().to("cpu", torch.float32),) + self._net().first_layers_cpu()

    def _schedule(self, t: torch.Tensor, host=None):
        """(a, b, c1) for real times ``t`` (fp32, CPU): a = 0, b = 1, c1 = [c1 of mlp_q | c1 of mlp_p], each the first
        layer's time columns times [sin | cos]((t W) 2 pi) plus its bias, zero-padded to the on-chip width."""
        W, (wq, bq), (wp, bp) = host if host is not None else self._schedule_inputs()
        c0, c1c = self._time_cols()
        H = int(self._net().plan(MODE_STATE).width)
        with solvers.host_threads():
            arg = t[:, None] * W[None, :] * 2 * math.pi
            emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
            c1 = torch.zeros(t.numel(), 2 * H, dtype=torch.float32)
            for i, (w0, b0) in enumerate(((wq, bq), (wp, bp))):
                # products rounded, summed in column order, then the bias (the device controller's order)
                acc = torch.zeros(t.numel(), w0.shape[0], dtype=torch.float32)
                for k in range(c1c - c0):
                    acc = acc + emb[:, k:k + 1] * w0[None, :, c0 + k]
                c1[:, i * H:i * H + w0.shape[0]] = acc + b0
            return torch.zeros_like(t), torch.ones_like(t), c1

    def _host_schedule(self):
        host = self._schedule_inputs()
        return lambda tr: self._schedule(tr, host)

    def _ode_table(self, t_span, method, options, mode, y0=None):
        plan = solvers.plan_ode(t_span, method, options, y0=y0)
        a, b, c1 = self._schedule(plan.t_eval)
        return solvers.build_table(plan, a, b, c1, self._net().width(mode))

    def _leapfrog_table(self, grid, pull_select=False, push_select=False):
        """The select plan's table of ``solvers.plan_leapfrog(grid)``: every row carries the c1 of the network it runs.
        ``pull_select`` / ``push_select``: the same rows at the row width of the pull-select / push-select plan (their units may
        be wider than the pair plan's)."""
        plan = solvers.plan_leapfrog(grid)
        a, b, c1 = self._schedule(plan.t_eval)
        H = self._net().width(MODE_STATE, select=True)
        net_b = (plan.flags & solvers.FLAG_NET_B) != 0
        own = torch.where(net_b[:, None], c1[:, H:], c1[:, :H])
        if pull_select or push_select:
            h0 = self._net().hidden[0]
            return solvers.build_table(plan, a, b, own[:, :h0],
                                       self._net().width(MODE_STATE, pull_select=pull_select, push_select=push_select))
        return solvers.build_table(plan, a, b, own, H)

    def _schedule_key(self):
        """Besides the first layers: the embedding frequencies."""
        W = self.model.W
        return (W.data_ptr(), W._version)

    def _module_half_rhs(self, cond):
        """One half of the field for the generic leapfrog (generic.ModuleStepper.run_leapfrog): ``rhs(t, y, net_b)`` is
        ``[0 | -mlp_p(q)]`` for a kick, ``[mlp_q(p) | 0]`` for a drift.  A SymplecticMLP evaluates only that network; any
        other module is evaluated whole and the needed half taken."""
        m = self.model

        def rhs(t, y, net_b):
            with torch.no_grad():
                tb = t.reshape(()).to(y.dtype).expand(y.shape[0])
                D = y.shape[1] // 2
                out = torch.zeros_like(y)
                if isinstance(m, SymplecticMLP):
                    q, p = torch.chunk(y, 2, dim=-1)
                    arg = tb[:, None] * m.W[None, :] * 2 * math.pi
                    tail = [torch.sin(arg), torch.cos(arg)] if cond is None else [cond, torch.sin(arg), torch.cos(arg)]
                    if net_b:
                        out[:, D:] = -m.mlp_p_dynamics(torch.cat([q] + tail, dim=1))
                    else:
                        out[:, :D] = m.mlp_q_dynamics(torch.cat([p] + tail, dim=1))
                else:
                    v = m(tb, y, cond)
                    if net_b:
                        out[:, D:] = v[:, D:]
                    else:
                        out[:, :D] = v[:, :D]
                return out
        return rhs

    def _module_rhs(self, mode, cond, probe):
        """``self.model`` evaluated by torch for the generic route: ``t`` expanded to the batch as the reference's
        callers do (symplectic.py:192, 236-238); no divergence (the field is divergence-free)."""
        def rhs(t, y):
            with torch.no_grad():
                return self.model(t.reshape(()).to(y.dtype).expand(y.shape[0]), y, cond), None
        return rhs
