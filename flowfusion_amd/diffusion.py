"""Score-based diffusion models on MI355X: the reference's ``flowfusion.diffusion`` API with the
sampling / log-density solves running as one fused HIP launch.

Class names, constructor arguments, method signatures, return shapes and ``state_dict`` keys
follow ``flowfusion/diffusion.py`` (MLP :9-121, ScoreModel :124-815, VESDE :818-1003,
VPSDE :1006-1180, SUBVPSDE :1183-1366, PopulationModelDiffusion[Conditional] :1466-1848) so a
model trained with the reference loads with ``load_state_dict`` and samples here.

What is native (csrc/ff_mlp_ode.hpp through the C ABI in include/flowfusion_amd.h):
``ScoreModel.sample_ode_from_base``, ``solve_odes_forward`` / ``log_prob`` (Hutchinson probe or
exact trace) and ``sample_sde``, for an ``MLP`` score network with SiLU activations and a
fixed-grid ``method`` (``euler``, ``midpoint``, ``heun3``, ``rk4`` + ``options={"step_size": h}``) or
the reference's default adaptive ``dopri5`` (step control on the device, device_adaptive.py; host controller: adaptive.py),
the divergence by Hutchinson probe, exact trace or the Hutch++ / XTrace estimators (csrc/ff_trace.hip).
CPU tensors raise: there is no eager/CPU fallback behind these methods.  The small pointwise members (``MLP.forward``, ``score``,
``ode_drift``, the SDE schedule functions) are ordinary torch code, used by training code and to
build the per-evaluation tables on the host.  Training losses and the adjoint branches of the
reference are out of scope.
"""
from __future__ import annotations

import copy
import math
import os
from typing import Optional

import torch
from torch import nn
from torch.distributions import Normal

from . import _native, device_adaptive, generic, odeint, solvers, trace_estimators
from .fused import FusedNet, MODE_EXACT, MODE_HUTCH, MODE_STATE, activation_spec, require_fp32, within_envelope
from .generic import _need_gpu
from .odeint import NoisyPosterior  # noqa: F401  (what ``posterior_noisy`` returns)


# ------------------------------------------------------------------------------------------------
# score network
# ------------------------------------------------------------------------------------------------
class MLP(nn.Module):
    """Score network: Gaussian-Fourier time features, then Linear/activation layers.

    Same parameters and buffers as the reference (diffusion.py:32-80): ``NN`` (ModuleList of
    Linear), ``W`` (frozen embedding frequencies, ``embedding_dimensions // 2`` of them drawn as
    ``randn * sigma_initialization``) and ``pi``.  Input column order of the first layer is
    ``[sin, cos, x, conditional]`` (diffusion.py:109-113).
    """

    def __init__(self, n_dimensions=2, n_conditionals=1, embedding_dimensions=8, units=[128],
                 activation=nn.SiLU(), sigma_initialization=16):
        super().__init__()
        self.n_dimensions = n_dimensions
        self.n_conditionals = n_conditionals
        self.architecture = [n_dimensions + n_conditionals + embedding_dimensions] + list(units) + [n_dimensions]
        self.n_layers = len(self.architecture) - 1
        self.NN = nn.ModuleList(
            nn.Linear(n_in, n_out) for n_in, n_out in zip(self.architecture[:-1], self.architecture[1:]))
        self.W = nn.Parameter(torch.randn(embedding_dimensions // 2) * sigma_initialization, requires_grad=False)
        self.activation = activation
        self.register_buffer("pi", torch.tensor(math.pi, dtype=torch.float32))

    def time_features(self, t):
        """[sin(2 pi W t), cos(2 pi W t)] with the reference's fp32 operation order (diffusion.py:109-110)."""
        arg = t[:, None] * self.W[None, :] * 2 * self.pi
        return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)

    def forward(self, t, x, conditional=None):
        if conditional is not None:
            x = torch.cat([x, conditional], dim=1)
        if t.dim() == 0:
            t = t * torch.ones(x.shape[:-1], device=x.device)
        h = torch.cat([self.time_features(t), x], dim=1)
        for layer in self.NN[:-1]:
            h = self.activation(layer(h))
        return self.NN[-1](h)


# ------------------------------------------------------------------------------------------------
# SDEs (closed-form schedules; reference: diffusion.py:818-1366)
# ------------------------------------------------------------------------------------------------
def _col(v, x):
    return v.view(-1, *[1] * (x.dim() - 1))


class VESDE(nn.Module):
    """Variance-exploding SDE: sigma(t) = sigma_min (sigma_max/sigma_min)^(t/T), zero drift."""

    def __init__(self, sigma_min=1e-2, sigma_max=10.0, T=1.0, epsilon=1e-5):
        super().__init__()
        for name, val in (("T", T), ("epsilon", epsilon), ("sigma_min", sigma_min), ("sigma_max", sigma_max)):
            self.register_buffer(name, torch.tensor(val, dtype=torch.float32))

    def sigma(self, t):
        return self.sigma_min * (self.sigma_max / self.sigma_min) ** (t / self.T)

    def diffusion(self, t, x):
        return _col(self.sigma(t), x) * torch.sqrt(2 * (torch.log(self.sigma_max) - torch.log(self.sigma_min)) / self.T)

    def drift(self, t, x):
        return torch.zeros_like(x)

    def marginal_prob_scalars(self, t):
        return torch.ones_like(t), self.sigma(t)

    def marginal_prob(self, t, x):
        m, s = self.marginal_prob_scalars(t)
        return _col(m, x) * x, _col(s, x)

    def sample_marginal(self, t, x0):
        m, s = self.marginal_prob_scalars(t)
        return _col(m, x0) * x0 + _col(s, x0) * torch.randn_like(x0)

    def prior(self, shape, mu=None):
        if mu is None:
            mu = torch.zeros(shape, device=self.T.device)
        else:
            assert mu.shape == shape
        return Normal(loc=mu, scale=self.sigma_max)


class VPSDE(nn.Module):
    """Variance-preserving SDE with linear beta(t); ``beta_min/beta_max/T`` are plain floats and
    ``epsilon`` a buffer, as in the reference (diffusion.py:1042-1045)."""

    def __init__(self, beta_min=0.1, beta_max=20, T=1.0, epsilon=1e-3):
        super().__init__()
        self.beta_min = beta_min
        self.beta_max = beta_max
        self.T = T
        self.register_buffer("epsilon", torch.tensor(epsilon, dtype=torch.float32))

    def beta(self, t):
        return self.beta_min + (self.beta_max - self.beta_min) * (t / self.T)

    def _log_coeff(self, t):
        return 0.5 * (self.beta_max - self.beta_min) * t ** 2 / self.T + self.beta_min * t

    def marginal_prob_scalars(self, t):
        lc = self._log_coeff(t)
        return torch.exp(-0.5 * lc), torch.sqrt(1.0 - torch.exp(-lc))

    def sigma(self, t):
        return self.marginal_prob_scalars(t)[1]

    def prior(self, shape):
        return Normal(loc=torch.zeros(shape, device=self.epsilon.device), scale=1.0)

    def diffusion(self, t, x):
        return _col(torch.sqrt(self.beta(t)), x)

    def drift(self, t, x):
        return -0.5 * _col(self.beta(t), x) * x

    def marginal_prob(self, t, x):
        m, s = self.marginal_prob_scalars(t)
        return _col(m, x) * x, _col(s, x)


class SUBVPSDE(VPSDE):
    """Sub-VP SDE: same drift as VP, g^2 = beta (1 - exp(-2 int beta)), std = 1 - exp(-int beta)."""

    def diffusion(self, t, x):
        decay = torch.exp(-2 * self.beta_min * t - (self.beta_max - self.beta_min) * t ** 2 / self.T)
        return _col(torch.sqrt(self.beta(t) * (1.0 - decay)), x)

    def marginal_prob_scalars(self, t):
        lc = self._log_coeff(t)
        return torch.exp(-0.5 * lc), 1.0 - torch.exp(-lc)


# ------------------------------------------------------------------------------------------------
# score model
# ------------------------------------------------------------------------------------------------
class ScoreModel(nn.Module):
    """Sampler / density evaluator for a score network and an SDE (reference: diffusion.py:124-815)."""

    def __init__(self, model=None, sde=None, conditional=None, no_sigma=False, hutchinson=False,
                 hutchpp=False, hpp_rank=1, hpp_vecs=1, xtrace=False, xt_vecs=1, *, precision="f32"):
        """Arguments as in the reference (diffusion.py:158-170).  Extension, keyword only: ``precision`` (also an
        attribute that can be flipped later) selects the arithmetic of the Linear layers in the fused solves:
        ``"f32"`` (default) is exact fp32, what the reference computes; ``"bf16x3"`` runs them on the bf16 matrix cores
        with every operand split into three bf16 parts and six products per term -- fp32-class accuracy (1e-7
        relative per layer) at about twice the speed, for the state-only solves (sampling on fixed grids and with the
        adaptive methods, ``sample_sde``) of SiLU networks with 1-4 hidden layers up to 256 wide, dim <= 16.
        ``"bf16x2"``: two bf16 parts by round-to-nearest (operands to 16 significand bits, unbiased) and three products per
        term -- half the matrix work of ``"bf16x3"``; a layer's error is ~4e-7 relative in the mean (fp32: 2e-8), end to
        end the sampler and the log-density of the headline configuration stay at the fp32 kernel's distance from the
        float64 oracle; same networks, also the Hutchinson and exact-trace log-densities and, state-only, dim <= 32.
        Anything else -- the Hutch++ / XTrace estimators, other activations, wider or deeper networks -- raises with these
        settings (round 3 froze the family at what the BASELINE configurations and the reference's demos reach)."""
        super().__init__()
        self.precision = precision
        self.model = model
        self.sde = sde
        self.conditional = conditional
        self.no_sigma = no_sigma
        self.prob = False
        self.hutch = hutchinson
        self.hutchpp = hutchpp
        self.hpp_rank = hpp_rank
        self.hpp_vector = hpp_vecs
        self.xtrace = xtrace
        self.xt_vector = xt_vecs
        self._fused = None

    # -- pointwise pieces (plain torch) -------------------------------------------------------
    def score(self, t, x, conditional=None):
        out = self.model(t, x, conditional=conditional)
        if self.no_sigma:
            return out
        return out / _col(self.sde.sigma(t), x)

    def ode_drift(self, t, x, conditional=None):
        g = self.sde.diffusion(t, x)
        return self.sde.drift(t, x) - 0.5 * g ** 2 * self.score(t, x, conditional=conditional)

    def forward(self, t, states):
        """ODE right-hand side in torchdiffeq's calling convention: ``states = (x,)`` or
        ``(x, dlogp)``; returns the matching tuple of time derivatives (reference :281-508).
        Autograd-based and differentiable; the fused solves do not call it."""
        x = states[0]
        if not self.prob:
            with torch.set_grad_enabled(True):
                x.requires_grad_(True)
                return self.ode_drift(t, x, conditional=self.conditional)
        n = x.shape[0]
        with torch.set_grad_enabled(True):
            x.requires_grad_(True)
            xdot = self.ode_drift(t, x, conditional=self.conditional)
            if self.hutch and self.e.dim() == 3:      # num_probes = K > 1 (extension): the mean over the K probes [B, K, D]
                div = sum((torch.autograd.grad(xdot, x, self.e[:, k], create_graph=True, retain_graph=True)[0] * self.e[:, k]).sum(dim=1)
                          for k in range(self.e.shape[1])) / self.e.shape[1]
            elif self.hutch:
                vjp = torch.autograd.grad(xdot, x, self.e, create_graph=True, retain_graph=True)[0]
                div = (vjp * self.e).sum(dim=1)
            elif self.hutchpp or self.xtrace:
                # the reference detaches the estimator's products (diffusion.py:375-396): not differentiable
                rows = [torch.autograd.grad(xdot[:, i].sum(), x, retain_graph=True)[0] for i in range(x.shape[1])]
                A = torch.stack(rows, dim=1).transpose(1, 2).contiguous()          # A[b] = J[b]^T
                div = self._estimate_divergence(A.detach(), x)
            else:
                div = x.new_zeros(n)
                for i in range(x.shape[1]):
                    div = div + torch.autograd.grad(xdot[:, i].sum(), x, create_graph=True, retain_graph=True)[0][:, i]
        return xdot, div.view(n, 1)

    # -- Hutch++ / XTrace (reference :336-481) ---------------------------------------------------
    def _probe_counts(self, D):
        """(r, m) of Hutch++ and m of XTrace with the reference's clamps (:343-344, :409)."""
        return (int(min(self.hpp_rank, D)), int(max(1, self.hpp_vector))), int(min(max(1, self.xt_vector), D))

    def _estimate_divergence(self, A, x):
        """Divergence estimate [B] from A[b] = J[b]^T with the stored probes (drawn afresh, like the reference's
        fallback :350-353, :415-416, when none of the right shape are stored).  On the GPU the estimate is one launch of
        ff_trace_estimate (csrc/ff_trace.hip); CPU tensors -- ``forward`` in training code, the tests' emulator -- and
        ``FF_TORCH_ESTIMATOR=1`` (A/B runs) take the torch statement of the same formulas (trace_estimators.py)."""
        B, D = x.shape
        (r, m), mx = self._probe_counts(D)
        native = A.is_cuda and A.dtype == torch.float32 and os.environ.get("FF_TORCH_ESTIMATOR", "") in ("", "0")
        if self.hutchpp:
            S, G = getattr(self, "S", None), getattr(self, "G", None)
            if S is None or tuple(S.shape) != (r, B, D):
                S = trace_estimators.draw_probes(r, x)
            if G is None or tuple(G.shape) != (m, B, D):
                G = trace_estimators.draw_probes(m, x)
            if native:
                return _native.trace_estimate(A.unsqueeze(0), "hutchpp", (S, G))[0]
            return trace_estimators.hutchpp(A, S.to(A.device), G.to(A.device))
        O = getattr(self, "O", None)
        if O is None or tuple(O.shape) != (mx, B, D):
            O = trace_estimators.draw_probes(mx, x)
        if native:
            return _native.trace_estimate(A.unsqueeze(0), "xtrace", (O,))[0]
        return trace_estimators.xtrace(A, O.to(A.device))

    # -- any other `model=` module: native stepping around the module's own forward (generic.py) -------------
    def _fusable(self) -> bool:
        """The score network is the reference's MLP and a compiled kernel holds its shape and activation.  Anything
        else -- a user module, or an MLP wider / higher-dimensional than the compiled shapes or with an activation
        the kernels do not implement -- is stepped by generic.py (the reference has no such limit, diffusion.py:59-72).
        An explicit ``precision=`` other than f32 never switches arithmetic silently: ``_net()`` raises instead."""
        m = self.model
        if not (hasattr(m, "NN") and hasattr(m, "W") and hasattr(m, "pi") and hasattr(m, "n_dimensions")):
            return False
        if getattr(self, "precision", "f32") != "f32":
            return True
        key = tuple(id(l) for l in m.NN) + (repr(m.activation),)
        return within_envelope(self, key, self._net)

    def _module_rhs(self, mode, cond, probe):
        """ODE right-hand side through ``self.forward`` (the reference's own RHS, diffusion.py:281-508) for the generic
        route (odeint.py): the user's module evaluates the score; divergences come from autograd exactly as in the
        reference (``self.prob`` / ``self.conditional`` and the probes are set by the caller)."""
        def rhs(t, y):
            if not self.prob:
                return self.forward(t, (y,)), None
            xdot, div = self.forward(t, (y, None))
            return xdot, div.reshape(-1)
        return rhs

    # -- fused path -----------------------------------------------------------------------------
    def _net(self) -> FusedNet:
        m = self.model
        if not (hasattr(m, "NN") and hasattr(m, "W") and hasattr(m, "pi") and hasattr(m, "n_dimensions")):
            raise NotImplementedError(
                "the fused gfx950 path needs a flowfusion MLP score network "
                f"(NN/W/pi attributes); got {type(m).__name__}")
        act = activation_spec(m.activation)
        prec = getattr(self, "precision", "f32")
        if self._fused is None or not self._fused.serves(list(m.NN), act, prec):
            E = 2 * m.W.numel()
            self._fused = FusedNet(list(m.NN), m.n_dimensions, m.n_conditionals, x_col0=E,
                                   c_col0=E + m.n_dimensions, act=act, precision=prec)
        return self._fused

    def _device_schedule(self, device):
        """What the device-side adaptive controller needs to evaluate this model's time-dependent terms itself
        (``device_adaptive.ScheduleSpec``), or None when it cannot: an SDE class other than the reference's three, or a
        score network without the MLP's Fourier features.  Scalars that live in buffers are read once per value."""
        sde, m = self.sde, self.model
        kind = {VESDE: _native.SCHED_VE, VPSDE: _native.SCHED_VP, SUBVPSDE: _native.SCHED_SUBVP}.get(type(sde))
        if kind is None or not (hasattr(m, "W") and hasattr(m, "pi") and hasattr(m, "NN")):
            return None
        names = ("sigma_min", "sigma_max", "T") if kind == _native.SCHED_VE else ("beta_min", "beta_max", "T")
        vals = [getattr(sde, n) for n in names] + [m.pi]
        key = tuple((v.data_ptr(), v._version) if torch.is_tensor(v) else v for v in vals)
        hit = self.__dict__.get("_dev_sched_scalars")
        if hit is None or hit[0] != key:
            hit = (key, [float(v) for v in vals])
            object.__setattr__(self, "_dev_sched_scalars", hit)
        p0, p1, p2, pi = hit[1]
        E = 2 * m.W.numel()
        w0t, b0 = self._net().time_columns(device, 0, E)
        emb_w = m.W.detach().to(device, torch.float32).contiguous()
        return device_adaptive.ScheduleSpec(kind, (p0, p1, p2), bool(self.no_sigma), emb_w, pi, w0t, b0)

    def _schedule_inputs(self):
        """Host copies of everything `_schedule` reads (SDE, embedding frequencies, first layer).  Taken once
        per solve: the adaptive driver calls `_schedule` at every attempted step, and each device-to-host copy
        would wait for the kernel in flight."""
        m = self.model
        w0, b0 = self._net().first_layer_cpu()
        return (copy.deepcopy(self.sde).to("cpu"), m.W.detach().to("cpu", torch.float32),
                m.pi.detach().to("cpu", torch.float32), w0, b0)

    def _host_schedule(self):
        """``(a, b, c1)`` of the probability-flow ODE for the host controller, from one set of host copies per solve."""
        host = self._schedule_inputs()
        return lambda tr: self._schedule(tr, "ode", host)[:3]

    def _schedule(self, t: torch.Tensor, sde_form: str, host=None):
        """Per-evaluation scalars (a, b) and first-layer bias c1 for real times ``t`` (fp32, CPU).

        ODE (diffusion.py:276-278): xdot = f - 0.5 g^2 score  ->  a = f/x, b = -0.5 g^2 [/ sigma]
        reverse SDE (:553):         f - g^2 score             ->  b = -g^2 [/ sigma]
        with f = a(t) x for all three SDEs (:905, :1131, :1316).  Returns also g (for the noise).
        """
        sde, W, pi, w0, b0 = host if host is not None else self._schedule_inputs()
        with solvers.host_threads():
            return self._schedule_on_host(t, sde_form, sde, W, pi, w0, b0)

    def _schedule_on_host(self, t, sde_form, sde, W, pi, w0, b0):
        one = torch.ones(t.numel(), 1, dtype=torch.float32)
        a = sde.drift(t, one).reshape(-1)
        g = sde.diffusion(t, one).reshape(-1)
        b = -(0.5 * g ** 2) if sde_form == "ode" else -(g ** 2)
        if not self.no_sigma:
            b = b / sde.sigma(t).reshape(-1)
        arg = t[:, None] * W[None, :] * 2 * pi
        emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        # broadcast product + sum rather than a matmul: a BLAS call this small costs ~0.5-8 ms when it wakes a
        # 128-thread pool on a many-core host (measured), the elementwise form stays on the calling thread
        c1 = (emb[:, None, :] * w0[None, :, : emb.shape[1]]).sum(-1) + b0
        return a, b, c1, g

    def _check_inputs(self, x, what):
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError(
                f"{what}: gradients through the fused solve are not available (the reference's "
                "odeint_adjoint branch, diffusion.py:620-629, is out of scope); detach the input")

    def _ode_table(self, t_span, method, options, mode, y0=None):
        plan = solvers.plan_ode(t_span, method, options, y0=y0)
        self._net().require_slots(int(plan.slot.max()) + 1, mode, f"method={method!r}")
        a, b, c1, _ = self._schedule(plan.t_eval, "ode")
        return solvers.build_table(plan, a, b, c1, self._net().width(mode))

    def _schedule_key(self):
        """Everything besides the first layer that the evaluation table depends on."""
        sde = self.sde
        vals = [self.no_sigma, type(sde).__name__]
        for name in ("beta_min", "beta_max", "T", "epsilon", "sigma_min", "sigma_max"):
            if hasattr(sde, name):
                vals.append(float(getattr(sde, name)))
        m = self.model
        return tuple(vals) + (m.W.data_ptr(), m.W._version)

    @torch.no_grad()
    def sample_sde(self, shape, conditional=None, steps=100, *, noise="torch", seed=None, sample_offset=0,
                   progress=None, progress_every=None):
        """Euler-Maruyama sampling of the reverse SDE; returns the last *mean* state, like the
        reference (diffusion.py:510-563).  By default random numbers are drawn exactly as the reference
        draws them on the model's device (one prior draw, then one ``randn_like`` per step), so a given
        ``torch.manual_seed`` reproduces the reference's stream on that device.  If a step produces a NaN the
        reference prints a message, stops and returns that step's mean (:560-563); so does this method (the
        step is located after the fact, by re-running a prefix of the launch that reported it).  One difference after
        such a stop: the reference stops DRAWING at the failing step, here the normals of the whole chunk (and, with two
        chunks in flight, of the next one) have been drawn by then, so torch's generator is further along than the
        reference's would be -- the returned tensor is the reference's, the generator state afterwards is not.

        Extensions: ``noise="philox"`` draws the per-step normals inside the kernel (counter-based, keyed by
        ``seed`` and the global sample index ``sample_offset + row``; include/flowfusion_amd.h): no noise
        buffers, no random-number kernels, and the result for a sample does not depend on how the batch is
        split over launches or GPUs (``flowfusion_amd.distributed.sample_sde_sharded``).  ``seed=None``
        takes one from torch's default generator, so ``torch.manual_seed`` still fixes the run.
        ``progress(done, total)`` is called after every ``progress_every`` steps (default: a tenth of the
        run) -- the reference's tqdm bar (:543-547) at launch granularity instead of three host syncs per
        step."""
        batch, *dims = shape
        dev = next(self.model.parameters()).device
        x = self.sde.prior(dims).sample([batch]).to(dev)
        kw = dict(progress=progress, progress_every=progress_every)
        if noise == "torch":
            return self._sample_sde_from(x, lambda like: torch.randn_like(like), conditional, steps, **kw)
        if noise != "philox":
            raise ValueError(f"noise={noise!r}: expected 'torch' or 'philox'")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return self._sample_sde_from(x, None, conditional, steps, rng=(int(seed), int(sample_offset)), **kw)

    @torch.no_grad()
    def _sample_sde_from(self, x, draw, conditional=None, steps=100, rng=None, progress=None, progress_every=None):
        """The Euler-Maruyama loop proper: ``x`` is the prior draw, ``draw(like)`` supplies the i-th
        standard-normal slab (tests inject the reference's captured stream here); with
        ``rng = (seed, global index of row 0)`` the kernel draws the normals itself.  The steps run in as few
        launches as the noise memory and the progress granularity allow (one, normally)."""
        require_fp32(self, x, conditional, what="sample_sde")
        if not self._fusable():
            if rng is not None:
                raise NotImplementedError("noise='philox' lives in the fused kernel; a custom score module samples with noise='torch'")
            host = copy.deepcopy(self.sde).to("cpu")
            drift = lambda t, xx: self.sde.drift(t, xx) - self.sde.diffusion(t, xx) ** 2 * self.score(t, xx, conditional=conditional)
            g_of_t = lambda ts: host.diffusion(ts, torch.ones(ts.numel(), 1))
            return generic.euler_maruyama(drift, g_of_t, x, draw, torch.as_tensor(self.sde.T, dtype=torch.float32).cpu(),
                                          self.sde.epsilon.detach().cpu(), steps, progress)
        net = self._net()
        if x.dim() != 2:
            raise NotImplementedError("sample_sde: only [batch, dim] states are supported")
        dev = x.device
        batch = x.shape[0]
        T = torch.as_tensor(self.sde.T, dtype=torch.float32).cpu()
        eps = self.sde.epsilon.detach().cpu()
        ts, dt = solvers.plan_euler_maruyama(T, eps, steps)
        n = int(ts.numel())
        if n == 0:
            raise RuntimeError("sample_sde: T < epsilon, no step to take")
        a, b, c1, g = self._schedule(ts, "sde")
        gn = g * (-dt) ** (1.0 / 2.0)                 # g * sqrt(-dt)  (:554-558)
        cout = torch.zeros(n, 8)
        cout[:, 0] = dt                               # x_mean = x + f dt  (:557)
        zeros8 = torch.zeros(n, 8)
        slot = torch.zeros(n, dtype=torch.int32)
        width = net.width(MODE_STATE)

        def table(start, stop, mean_last):
            """Rows of steps [start, stop); with `mean_last` the last one returns x_mean (no noise added, :563)."""
            flags = torch.full((stop - start,), solvers.FLAG_STEP_END | solvers.FLAG_NOISE, dtype=torch.int32)
            if mean_last:
                flags[-1] = solvers.FLAG_STEP_END
            sub = solvers.EvalPlan(t_eval=ts[start:stop], sign=1.0, slot=slot[start:stop], flags=flags,
                                   cin=zeros8[start:stop], cout=cout[start:stop], n_steps=stop - start)
            return solvers.build_table(sub, a[start:stop], b[start:stop], c1[start:stop], width,
                                       gn=gn[start:stop], noise_idx=torch.arange(stop - start)).to(dev)

        def launch(x_in, start, stop, mean_last, buf):
            if rng is not None:
                return net.integrate(x_in, table(start, stop, mean_last), MODE_STATE, cond=conditional,
                                     rng=(rng[0] & 0x7FFFFFFFFFFFFFFF, rng[1], start), stage_slots=1)
            return net.integrate(x_in, table(start, stop, mean_last), MODE_STATE, cond=conditional,
                                 noise=buf[: stop - start], stage_slots=1)

        def first_nan_mean(x_in, start, stop, buf):
            """A launch over steps [start, stop) reported NaN: the reference would have stopped at the first
            step whose state x (noise included, :558-560) has one and returned that step's mean.  NaN is
            absorbing, so bisect on the number of full steps (each probe = one launch of a prefix), then
            re-run that prefix with a mean-only last row."""
            lo, hi = 1, stop - start                  # smallest m with a NaN in x after m steps
            while lo < hi:
                mid = (lo + hi) // 2
                if int(launch(x_in, start, start + mid, False, buf)[2].item()) & 1:
                    hi = mid
                else:
                    lo = mid + 1
            return launch(x_in, start, start + lo, True, buf)[0]

        # chunk boundaries: noise slabs are drawn per step, in order, at most 2^28 floats (1 GiB) per buffer;
        # a progress callback adds boundaries of its own
        per_step = max(batch * x.shape[1], 1)
        chunk = n if rng is not None else max(1, min(n, (1 << 28) // per_step))
        if progress is not None:
            every = int(progress_every) if progress_every else max(1, n // 10)
            chunk = max(1, min(chunk, every))
        bounds = [(s0, min(n, s0 + chunk)) for s0 in range(0, n, chunk)]
        bufs = [] if rng is not None else [
            torch.empty(min(chunk, n), batch, x.shape[1], device=dev, dtype=torch.float32)
            for _ in range(min(2, len(bounds)))]
        # The draws of chunk c+1 are enqueued on a side stream while the kernel integrates chunk c (two
        # buffers), so the random-number kernels stay off the critical path; the host-side generator is
        # advanced in the same order either way, so the stream of numbers is unchanged.
        overlap = rng is None and len(bounds) > 1
        main = torch.cuda.current_stream(dev) if x.is_cuda else None
        side = torch.cuda.Stream(device=dev) if overlap else None
        ready = [None] * len(bounds)
        freed = [None] * len(bufs)

        def fill(c):
            start, stop = bounds[c]
            buf = bufs[c % len(bufs)]
            if not overlap:
                for i in range(stop - start):                   # one draw per executed step, the last included (:554)
                    buf[i] = draw(x)
                return
            with torch.cuda.stream(side):
                if freed[c % len(bufs)] is not None:
                    side.wait_event(freed[c % len(bufs)])       # the kernel that read this buffer is done
                else:
                    side.wait_stream(main)
                for i in range(stop - start):
                    buf[i] = draw(x)
                ready[c] = side.record_event()

        if rng is None:
            fill(0)
        for c, (start, stop) in enumerate(bounds):
            if overlap and c + 1 < len(bounds):
                fill(c + 1)
            if overlap:
                main.wait_event(ready[c])
            buf = bufs[c % len(bufs)] if bufs else None
            x_in = x
            x, _, status = launch(x_in, start, stop, stop == n, buf)
            if overlap:
                freed[c % len(bufs)] = main.record_event()
            if int(status.item()) & 1:
                print("Diffusion is not stable, NaN were produced. Stopped sampling.")
                return first_nan_mean(x_in, start, stop, buf)
            if progress is not None:
                progress(stop, n)
        return x

    def sample_ode_from_base(self, base_samples, conditional=None, atol=1e-4, rtol=1e-4,
                             method="dopri5", options=None):
        """Probability-flow ODE from t=1 down to epsilon; returns ``(samples, [])`` like the
        reference (diffusion.py:566-640).  ``atol``/``rtol`` are accepted for signature
        compatibility and unused by the fixed-grid methods."""
        return self._sample_ode(base_samples, conditional, atol, rtol, method, options), []

    def _sample_ode(self, base_samples, conditional, atol, rtol, method, options, out_scale=None, out_shift=None):
        """sample_ode_from_base proper; ``x * out_scale + out_shift`` (PopulationModel*.forward,
        diffusion.py:1575-1585, 1772-1784) is applied by the kernel's epilogue."""
        self._check_inputs(base_samples, "sample_ode_from_base")
        if self._fusable():
            self._net()
        z = base_samples * self.sde.sigma_max if hasattr(self.sde, "sigma_max") else base_samples
        self.prob = False
        self.conditional = conditional
        t_span = torch.tensor([1.0, float(self.sde.epsilon)], dtype=torch.float32)
        x, _ = odeint.solve(self, z, t_span, method, options, MODE_STATE, atol, rtol, cond=conditional,
                            out_scale=out_scale, out_shift=out_shift)
        return x

    # -- flow-map sensitivities (extension) -------------------------------------------------------------------------------
    def _push_args(self, x, direction):
        """(t_span, start gain) of a sensitivity solve: ``to_data`` is ``sample_ode_from_base``'s solve (``x`` = base samples,
        started from ``x * sigma_max`` where the SDE has one, t: 1 -> epsilon; the tangents follow with the same factor --
        ``odeint.solve_push`` applies it behind its checks), ``to_base`` is ``solve_odes_forward``'s (t: epsilon -> 1)."""
        if direction not in ("to_data", "to_base"):
            raise ValueError(f"direction={direction!r}: 'to_data' (the solve of sample_ode_from_base) or 'to_base' (the solve "
                             "of solve_odes_forward)")
        eps = float(self.sde.epsilon)
        if direction == "to_base":
            return torch.tensor([eps, 1.0], dtype=torch.float32), None
        return torch.tensor([1.0, eps], dtype=torch.float32), getattr(self.sde, "sigma_max", None)

    @torch.no_grad()
    def flow_jvp(self, x, tangents=None, conditional=None, conditional_tangents=None, *, direction="to_data", method="rk4",
                 options=None):
        """Extension: the probability-flow solve of ``sample_ode_from_base`` (``direction="to_data"``, ``x`` = base samples)
        or of ``solve_odes_forward`` (``"to_base"``) with K directions pushed through it, forward mode, in ONE launch:
        returns ``(x_out [B, D], dx [B, K, D])`` with ``dx[b, k] = d x_out[b] / d (x[b], conditional[b]) . (tangents[b, k],
        conditional_tangents[b, k])`` -- the exact derivative of the DISCRETE solver map, so fixed grids only
        (``method="rk4"`` / ``"dopri5_fixed"`` / ``"euler"`` ... with ``options={"step_size": h}``).  ``tangents`` [B, K, D]
        and ``conditional_tangents`` [B, K, C]: either may be None (zero); K <= 15.  The tangent columns ride beside the
        value column of a sample like the probes of ``num_probes=K``; measured, a launch costs 2 % more than that solve on an
        unconditional model (the push-forward kernels always carry conditional registers; profiles/pushforward.txt).
        No parameter gradients, no torch.autograd integration (the call runs under ``no_grad``), no adaptive step control,
        no Euler-Maruyama, f32 SiLU networks within the push-forward kernels only: see ``odeint.solve_push``."""
        return self._flow_jvp(x, tangents, conditional, conditional_tangents, direction, method, options)

    def _flow_jvp(self, x, tangents, conditional, conditional_tangents, direction, method, options, **maps):
        """``flow_jvp`` proper; ``maps``: the affine maps and the conditional scale of the population wrappers
        (``odeint.solve_push``)."""
        t_span, gain = self._push_args(x, direction)
        return odeint.solve_push(self, x, t_span, method, options, tangents=tangents, cond=conditional,
                                 cond_tangents=conditional_tangents, tangent_gain=gain, **maps)

    @torch.no_grad()
    def flow_jacobian(self, x, conditional=None, *, direction="to_data", method="rk4", options=None):
        """Extension: the whole Jacobian of the solver map of ``flow_jvp``: ``(x_out [B, D], J_x [B, D, D], J_c [B, D, C] or
        None)``, ``J_x[b, i, j] = d x_out_i / d x_j``, ``J_c[b, i, j] = d x_out_i / d conditional_j``, from unit tangents
        in ceil((D + C) / 15) launches (``x_out`` is the first launch's)."""
        return self._flow_jacobian(x, conditional, direction, method, options)

    @torch.no_grad()
    def flow_vjp(self, x, cotangents, conditional=None, *, direction="to_data", method="rk4", options=None,
                 return_retrace=False, adjoint="continuous"):
        """Extension: K cotangents pulled back through the probability-flow solve of ``flow_jvp``, reverse mode: returns
        ``(x_out [B, D], gx [B, K, D], gc [B, K, C] or None)`` -- plus ``retrace [B]`` with ``return_retrace`` -- with
        ``gx[b, k] = cotangents[b, k]^T d x_out[b] / d x[b]`` and ``gc`` likewise for ``conditional``; ``cotangents`` is
        [B, K, D], K <= 15; ``x_out`` is bitwise the fixed-grid state-only solve (for a VE model ``to_data`` starts from
        ``x * sigma_max``, and ``gx`` carries the factor).

        It integrates the CONTINUOUS adjoint over the reversed grid, as the reference's ``odeint_adjoint`` does -- not the
        transpose of the discrete map ``flow_jvp`` differentiates.  The two differ by the discretisation error, and the
        backward sweep retraces the state instead of storing it.  A score model's Fourier time features (sigma = 16) are
        under-resolved below about 100 steps: use rk4 or better, read ``retrace[b] = max_d |y_back - x|``, and raise the step
        count until it is small.  (Measured in float64 on a VP model: gap to ``w^T flow_jacobian`` 4e-4 with 32 rk4 steps,
        4e-6 with 128; with 128 EULER steps ``to_base`` the gap is 0.7 and the retrace 0.4.)

        ``adjoint="discrete"`` (keyword only) takes the exact discrete adjoint instead (``odeint.solve_pull_discrete``): a
        forward launch records the stage state of every evaluation row and a second one runs the transposed row program
        backwards over them, so ``gx`` and ``gc`` are the transpose of what ``flow_jvp`` differentiates up to rounding at ANY
        step count -- the gradient of the function that is actually evaluated.  ``x_out`` is then the record launch's state
        (bitwise the fixed-grid solve's, as on the default route), nothing is retraced (``return_retrace`` raises), and
        the record costs ``n_evals * B * D`` floats of device memory per piece of rows.  Any other value raises ValueError.

        No parameter gradients, no torch.autograd integration, no adaptive step control: see ``odeint.solve_pull`` and
        ``odeint.solve_pull_discrete``."""
        return self._flow_vjp(x, cotangents, conditional, direction, method, options, return_retrace, adjoint)

    def _flow_vjp(self, x, cotangents, conditional, direction, method, options, return_retrace, adjoint="continuous", **maps):
        t_span, gain = self._push_args(x, direction)
        return odeint.solve_pull_by(adjoint, self, x, t_span, method, options, cotangents, cond=conditional, tangent_gain=gain,
                                    return_retrace=return_retrace, **maps)

    def _flow_jacobian(self, x, conditional, direction, method, options, **maps):
        t_span, gain = self._push_args(x, direction)
        return odeint.solve_push_jacobian(self, x, t_span, method, options, cond=conditional, tangent_gain=gain, **maps)

    @torch.no_grad()
    def solve_odes_forward(self, x0_samples, conditional=None, atol=1e-5, rtol=1e-5,
                           method="dopri5", options=None, *, probe="torch", seed=None, sample_offset=0, num_probes=1,
                           return_stderr=False, products="jacobian"):
        """Probability-flow ODE from epsilon up to t=1 with the divergence integrated alongside;
        returns ``(xT, delta_logp[B,1])`` (reference: diffusion.py:642-754).

        ``return_stderr=True`` (keyword only, extension; ``num_probes=K >= 2`` on a fixed grid): returns
        ``(xT, delta_logp, stderr[B,1])`` -- the first two bitwise what the call without it returns, ``stderr`` the
        standard error of ``delta_logp`` as the mean of K single-probe estimates (``trace_estimators.hutchinson_stderr``:
        their sample standard deviation over sqrt(K)).  The K estimates stay in ``self.dlogp_probes`` [B, K], next to the
        probes ``self.e`` [B, K, D]: column k is what a single-probe solve with probe k alone returns as ``delta_logp``.
        They come out of the same launch (ff_mlp_ode_launch_probes: one more store per tangent column), so the solve costs
        what it costs without them; a ``model=`` module on the generic route pays K more single-probe passes.  Adaptive
        methods -- the default here -- are refused with the way out: ``method="rk4"`` / ``"dopri5_fixed"`` with
        ``options={"step_size": h}``.

        Extension, keyword only (Hutchinson models): ``probe="torch"`` (default) draws the +-1 probe on the CPU and
        moves it, exactly as the reference does (:701), so ``torch.manual_seed`` reproduces its stream;
        ``probe="philox"`` takes the signs of the library's counter-based normals keyed by ``seed`` and the GLOBAL row
        ``sample_offset + r`` (``ff_normal_fill`` with the reserved probe index): drawn on the device (no host draw, no
        upload) and independent of how a batch is cut into shards (``distributed.log_prob_sharded``).
        ``num_probes=K`` (Hutchinson models): the divergence is the mean over K independent +-1 probes per sample, all
        carried by ONE launch -- a sample and its K probes share the columns of a kernel tile, so K <= tile - 1 (15, or 31 on
        the 32-column kernels); a tile holds tile // (1 + K) samples, and the cost follows that occupancy (measured, profiles/hutch_multi.txt:
        1.99x / 3.97x / 7.93x a single-probe solve at K = 3 / 7 / 15 on 16 columns); the variance falls as 1 / K.  ``self.e`` then holds the
        probes as [B, K, D]; probe 0 of ``probe="philox"`` is the single-probe stream's, probe k >= 1 lives under the noise
        index FF_HUTCH_PROBE_NOISE_BASE + k.  On fixed grids the rows are cut so that a probe buffer on the device stays
        under 1 GiB (``odeint.solve_hutchinson``; ``probe="torch"`` still draws the whole [B, K, D] set on the host, and
        ``self.e`` holds it whole).  f32 kernels only.

        ``products`` (keyword only, extension; ``hutchpp=True`` / ``xtrace=True`` models): how a Hutch++ / XTrace solve gets
        its matrix-vector products.  ``"jacobian"`` (default): today's route, bit for bit -- the Jacobian of every
        evaluation row is recorded in forward mode (D + 1 tile columns per sample, ``n_evals B D D`` floats through memory)
        and ``ff_trace_estimate`` reads it.  ``"vjp"`` (opt-in): the reference's own route (diffusion.py:356-398,
        :419-455), J^T v products in reverse mode -- two sweeps of the products unit over the fixed grid
        (``ff_mlp_ode_launch_vjp``; r, then r + m seed columns per sample for Hutch++, m and m for XTrace) with
        ``ff_trace_basis`` between and ``ff_trace_combine`` after them; ``(2r + m) D`` or ``2m D`` floats per evaluation and
        sample, no Jacobian.  Same probes (``probe="torch"`` / ``"philox"``), same ``self.S`` / ``self.G`` / ``self.O``, same
        shapes.  The two routes agree to rounding, not bitwise.  When the Jacobian route is the cheaper one: at small D,
        where D + 1 columns undercut two sweeps that each run two networks, and at many seed columns (a tile holds
        16 // (1 + K) samples).  Measured (one MI355X, 100-step rk4, 2^16 rows, 4x256, whole calls against the parent
        commit's in the same run; profiles/estimator_products.txt): 16-d 0.62x at r = m = 1, 0.75x at XTrace m = 2, 2.36x
        (slower) at r = m = 4; 32-d 0.30x, 0.39x, 1.17x (slower).  ``"vjp"`` refuses, with ValueError before the device is touched:
        adaptive methods -- the default here: pass ``method="rk4"`` / ``"dopri5_fixed"`` with
        ``options={"step_size": h}``, or stay with ``"jacobian"`` --, ``grid_constructor`` / ``perturb``, a model without
        ``hutchpp=True`` / ``xtrace=True``, ``hpp_rank + hpp_vecs > 15`` or ``xt_vecs > 15``, ``precision`` other than f32;
        with NotImplementedError naming ``_native.PULL_ENVELOPE``: a network outside the pull-back units, a ``model=``
        module.  Out of scope: the adaptive / device-controller hook-up (adaptive solves, the reference's defaults, still
        take the Jacobian route), a single-sweep kernel with the QR in it, sharded entry points (rows are independent:
        slice), the flows (no estimators), split precision and non-SiLU activations, a module-path fallback,
        ``num_probes``; ``log_prob_noisy`` / ``posterior_noisy`` keep their signatures and the Jacobian route."""
        philox_ok = self.hutch or self.hutchpp or self.xtrace
        out = self._solve_forward(x0_samples, conditional, atol, rtol, method, options, probe_rng=trace_estimators.probe_rng(
            probe, seed, sample_offset, philox_ok, "probe='philox' draws the probes of a Hutchinson / Hutch++ / XTrace model: "
            "construct it with hutchinson=True, hutchpp=True or xtrace=True"), num_probes=num_probes, return_stderr=return_stderr,
            products=products)
        return out if return_stderr else out[:2]

    @torch.no_grad()
    def _solve_forward(self, x0_samples, conditional, atol, rtol, method, options, in_shift=None, in_scale=None,
                       probe_rng=None, num_probes=1, return_stderr=False, products="jacobian"):
        """solve_odes_forward proper; returns ``(xT, delta_logp [B,1], stderr [B,1] or None)``.  ``(x - in_shift) / in_scale``
        (PopulationModel*.log_prob, diffusion.py:1633, 1837) is applied by the kernel's prologue."""
        K = trace_estimators.check_num_probes(num_probes, bool(self.hutch), "construct the model with hutchinson=True",
                                              estimator=bool((self.hutchpp or self.xtrace) and not self.hutch))
        stderr = trace_estimators.check_stderr(return_stderr, K, method)
        estimator = bool((self.hutchpp or self.xtrace) and not self.hutch)
        if products != "jacobian" and not estimator:
            odeint.check_products(self, products, method, options)      # (raises: no estimator, or no such route)
        fused = self._fusable()
        if fused:
            self._net()
        self.prob = True
        self.conditional = conditional
        if (self.hutchpp or self.xtrace) and not self.hutch:
            if in_shift is not None:
                x0_samples = (x0_samples - in_shift) / in_scale
            return self._solve_with_estimator(x0_samples, conditional, atol, rtol, method, options, fused, probe_rng,
                                              products) + (None,)
        t_span = torch.tensor([float(self.sde.epsilon), 1.0], dtype=torch.float32)
        if not self.hutch:
            xT, dlogp = odeint.solve(self, x0_samples, t_span, method, options, MODE_EXACT, atol, rtol, cond=conditional,
                                     in_shift=in_shift, in_scale=in_scale)
            return xT, dlogp.view(-1, 1), None
        if probe_rng is not None and x0_samples.dim() != 2:
            raise NotImplementedError("probe='philox': only [batch, dim] states")
        xT, dlogp, d = odeint.solve_hutchinson(self, x0_samples, t_span, method, options, atol, rtol, K, probe_rng,
                                               keep=lambda e: setattr(self, "e", e), per_probe=stderr, cond=conditional,
                                               in_shift=in_shift, in_scale=in_scale)
        if stderr:
            self.dlogp_probes = d
        return xT, dlogp.view(-1, 1), (trace_estimators.hutchinson_stderr(d).view(-1, 1) if stderr else None)

    def _solve_with_estimator(self, x0, conditional, atol, rtol, method, options, fused, probe_rng=None, products="jacobian"):
        """Hutch++ / XTrace log-density solve.  The state never depends on the divergence, so the fused launches are those
        of the exact trace with the Jacobian of every evaluation row recorded (ff_ode_args.jac_all); the estimates of all
        rows come from ONE launch (ff_trace_estimate, csrc/ff_trace.hip) and are combined with the tableau's weights
        (odeint.py picks the route).  Any other module: forward() runs the estimator itself (reverse mode, like the
        reference).  Probes are drawn once per solve on the state's device, as the reference does (:703-719).
        ``products="vjp"``: the same estimates from J^T v products (``solve_odes_forward``; odeint.check_products)."""
        if products != "jacobian":
            (r, m), mx = self._probe_counts(x0.shape[1])
            odeint.check_products(self, products, method, options, *(("hutchpp", r, m) if self.hutchpp else ("xtrace", mx, 0)))
        if fused:
            net = self._net()
            if net.precision != "f32":
                raise NotImplementedError(f"precision={net.precision!r}: the Hutch++ / XTrace estimators need the Jacobian output of the "
                                          "f32 kernels (bf16x2 serves hutchinson=True and the exact trace)")
            _need_gpu(x0)
        elif probe_rng is not None:
            raise NotImplementedError("probe='philox' lives on the fused path; a custom score module draws its probes with torch")
        (r, m), mx = self._probe_counts(x0.shape[1])
        if probe_rng is not None:       # probe="philox": keyed by (seed, global row), independent of the sharding
            draw = lambda n, second=False: trace_estimators.draw_probes_philox(n, x0, probe_rng[0], probe_rng[1], second)
        else:
            draw = lambda n, second=False: trace_estimators.draw_probes(n, x0)
        if self.hutchpp:
            self.S = draw(r)
            self.G = draw(m, True)
            kind, probes = "hutchpp", (self.S, self.G)
        else:
            # the reference stores max(1, xt_vecs) probes and redraws inside forward when that exceeds D (:719, :409-416)
            self.O = draw(mx)
            kind, probes = "xtrace", (self.O,)
        t_span = torch.tensor([float(self.sde.epsilon), 1.0], dtype=torch.float32)
        y, lp = odeint.solve(self, x0, t_span, method, options, MODE_EXACT, atol, rtol, cond=conditional,
                             estimator=(kind, probes), div_fn=lambda A: self._estimate_divergence(A, x0), products=products)
        return y, lp.view(-1, 1)

    @torch.no_grad()
    def log_prob(self, x0_samples, conditional=None, atol=1e-4, rtol=1e-4, method="dopri5",
                 options={"min_step": 1e-6}, *, probe="torch", seed=None, sample_offset=0, num_probes=1, return_stderr=False,
                 products="jacobian"):
        """log p(x0) = delta_logp + log prior(xT), shape [B,1] (reference: diffusion.py:756-815).  ``probe`` / ``seed`` /
        ``sample_offset`` / ``num_probes`` / ``return_stderr`` / ``products``: see ``solve_odes_forward``; with ``return_stderr=True``
        returns ``(log_p [B,1], stderr [B,1])`` (the prior term is exact, so the standard error is ``delta_logp``'s)."""
        out = self.solve_odes_forward(x0_samples, conditional=conditional, atol=atol, rtol=rtol,
                                      method=method, options=options, probe=probe, seed=seed,
                                      sample_offset=sample_offset, num_probes=num_probes, return_stderr=return_stderr,
                                      products=products)
        xT, lp = out[0], out[1]
        logp = lp + torch.sum(self.sde.prior(xT.shape).log_prob(xT), dim=1, keepdim=True)
        return (logp, out[2]) if return_stderr else logp

    @torch.no_grad()
    def log_prob_grad(self, x, conditional=None, *, method="rk4", options=None, probe="torch", seed=None, sample_offset=0,
                      num_probes=1):
        """Extension: ``log_prob`` on a fixed grid together with its gradient: returns ``(log_p [B, 1], grad_x [B, D],
        grad_c [B, C] or None)`` -- what HMC / NUTS or L-BFGS over ``x`` or over the conditional inputs needs.  ``log_p`` is
        bitwise ``log_prob(x, conditional, method=method, options=options, probe=..., ...)``.  On a ``hutchinson=True``
        model the gradient launches take the very probes of that solve (``self.e``), and ``grad_x`` / ``grad_c`` are the
        exact gradient of that value as a function of ``(x, conditional)`` at FIXED probes -- the discrete adjoint with the
        divergence integral in it (reverse mode over the forward-mode tangent, ``odeint.solve_logp_grad``), exact at any
        step count.  On an exact-trace model the value comes from the exact-trace solve and the gradient from the D unit
        probes with weight 1: the gradient of the same discrete sum, to rounding.  Three launches per piece of rows: the
        value solve, the record launch, the gradient launch; K probes are K rows each.

        Fixed grids only (``method="rk4"`` / ``"dopri5_fixed"`` / ``"euler"`` with ``options={"step_size": h}``; the default
        grid is ONE step): adaptive methods, ``grid_constructor`` / ``perturb``, ``precision`` other than f32 and Hutch++ /
        XTrace models raise before the device is touched.  No parameter gradients, no torch.autograd integration (the call
        runs under ``no_grad``): see ``odeint.solve_logp_grad``; the gradient of ``log_prob_noisy`` is ``log_prob_noisy_grad``."""
        return self._log_prob_grad(x, conditional, method, options, probe, seed, sample_offset, num_probes)

    def _log_prob_grad(self, x, conditional, method, options, probe, seed, sample_offset, num_probes, in_shift=None,
                       in_scale=None, cond_tangent_scale=None):
        """``log_prob_grad`` proper; the affine input map and the conditional scale of the population wrappers as in
        ``_flow_vjp``."""
        rng = self._logp_grad_checks(x, conditional, method, options, probe, seed, sample_offset, num_probes)
        logp = self._logp_value(x, conditional, method, options, rng, num_probes, in_shift, in_scale)
        gx, gc = self._logp_grad_rows(x, conditional, method, options, self.e if self.hutch else None, in_shift=in_shift,
                                      in_scale=in_scale, cond_tangent_scale=cond_tangent_scale)
        return logp, gx, gc

    def _logp_grad_checks(self, x, conditional, method, options, probe, seed, sample_offset, num_probes):
        """What ``log_prob_grad`` and ``log_prob_noisy_grad`` refuse, before the device is touched; returns the probes' key."""
        if (self.hutchpp or self.xtrace) and not self.hutch:
            raise ValueError("log-density gradients of a Hutch++ / XTrace model: the estimators' products are not differentiated "
                             "(the reference detaches them too); construct the model with hutchinson=True, or without an "
                             "estimator (the exact trace)")
        trace_estimators.check_num_probes(num_probes, bool(self.hutch), "construct the model with hutchinson=True")
        rng = trace_estimators.probe_rng(probe, seed, sample_offset, bool(self.hutch),
                                         "probe='philox' draws the probes of a Hutchinson model: construct it with hutchinson=True")
        odeint.check_logp_grad(self, x, method, options, conditional)
        return rng

    def _logp_value(self, x, conditional, method, options, rng, num_probes, in_shift=None, in_scale=None):
        """The value half of ``log_prob_grad``: the fixed-grid ``log_prob`` [B, 1] of the rows ``x``; a Hutchinson model's
        probes stay in ``self.e``."""
        xT, lp, _ = self._solve_forward(x, conditional, 0.0, 0.0, method, options, in_shift=in_shift, in_scale=in_scale,
                                        probe_rng=rng, num_probes=num_probes)
        return lp + torch.sum(self.sde.prior(xT.shape).log_prob(xT), dim=1, keepdim=True)

    def _logp_grad_rows(self, x, conditional, method, options, e, in_shift=None, in_scale=None, cond_tangent_scale=None):
        """The gradient half of ``log_prob_grad``: ``(gx [B, D], gc [B, C] or None)`` of the rows ``x`` with the Hutchinson
        probes ``e`` ([B, D] or [B, K, D]) of their value solve, or with the D unit probes of the exact trace (``e`` None)."""
        B, D = x.shape
        if e is not None:
            probes = e if e.dim() == 3 else e.unsqueeze(1)
            weight = 1.0 / probes.shape[1]
        else:
            probes, weight = torch.eye(D, dtype=torch.float32, device=x.device).expand(B, D, D), 1.0
        var = float(getattr(self.sde, "sigma_max", 1.0)) ** 2          # the prior: N(0, sigma_max^2) on a VE model, else N(0, 1)
        t_span = torch.tensor([float(self.sde.epsilon), 1.0], dtype=torch.float32)
        _, gx, gc = odeint.solve_logp_grad(self, x, t_span, method, options, probes.contiguous(), weight, cond=conditional,
                                           in_shift=in_shift, in_scale=in_scale, cond_tangent_scale=cond_tangent_scale,
                                           prior_grad=lambda y: -y / var)
        return gx, gc

    @torch.no_grad()
    def log_prob_noisy_grad(self, x, noise_std, conditional=None, num_draws=16, *, method="rk4", options=None, seed=None,
                            sample_offset=0, chunk_points=None, num_probes=1, min_weight=0.0, return_ess=False,
                            return_noise_grad=False):
        """Extension: ``log_prob_noisy`` on a fixed grid together with its gradient: returns ``(log_p [B, 1], grad_x [B, D],
        grad_c [B, C] or None)`` -- then ``ess [B]`` with ``return_ess`` and ``grad_noise_std [B, D]`` with
        ``return_noise_grad`` -- what HMC / NUTS or L-BFGS over the population hyper-parameters (``conditional``) of a
        catalogue of measured objects needs: ``sum_r log_p[r]`` is the hierarchical likelihood, ``grad_c`` its gradient per
        object.  ``log_p`` and ``ess`` are bitwise ``log_prob_noisy(x, noise_std, conditional, num_draws, method=method,
        options=options, seed=seed, ..., return_ess=True)``.  With ``wn_k`` the normalised weight of draw k (double),
        ``grad_x = sum_k wn_k grad_y lp_k``, ``grad_c = sum_k wn_k grad_c lp_k`` and ``grad_noise_std = -sum_k wn_k z_k
        grad_y lp_k`` (per object and dimension, whatever the shape of ``noise_std``), ``grad lp_k`` the discrete adjoint of
        ``log_prob_grad`` on row k: the exact gradient of the value returned at fixed draws -- and, on a ``hutchinson=True``
        model, at fixed probes (the very probes of the value solve of those rows, ``probe="philox"`` under the same
        ``seed``) -- at any step count.  On an exact-trace model the value comes from the exact-trace solve and the
        gradient from the D unit probes with weight 1: D gradient rows per kept draw, and ``min_weight`` is the lever.

        ``min_weight`` = m (0 <= m < 1): only draws with ``wn_k > 0`` and ``wn_k >= m`` go through the record and gradient
        launches (typically most draws carry no weight: ess is a small fraction of K).  The sums keep the weights of the
        full sum, not renormalised, so the truncation error is at most ``sum_skipped wn_k |grad lp_k| <= K m max |grad
        lp|``; m = 0 keeps every draw of non-zero weight.  ``self.last_noisy_grad_stats`` = ``{"rows": B K, "rows_kept": n,
        "gradient_rows": rows that reached the gradient launch}`` after the call.  A point with a NaN or +inf among its
        rows' log-densities, or with no weight at all, has NaN gradients; its ``log_p`` is what ``log_prob_noisy`` gives.

        Fixed grids only (``method="rk4"`` / ``"dopri5_fixed"`` / ``"euler"`` with ``options={"step_size": h}``; the default
        grid is ONE step): every refusal of ``log_prob_grad`` applies, before the device is touched.  ``noise_std``,
        ``num_draws``, ``seed``, ``sample_offset``, ``chunk_points``: as in ``log_prob_noisy``; any chunking and any slice of
        the batch at its ``sample_offset`` give bitwise the same.  Out of scope: sharded entry points (slice), adaptive
        methods, gradients of ``posterior_noisy``, parameter gradients and torch.autograd integration."""
        return self._log_prob_noisy_grad(x, noise_std, conditional, num_draws, method, options, seed, sample_offset,
                                         chunk_points, num_probes, min_weight, return_ess, return_noise_grad)

    def _log_prob_noisy_grad(self, x, noise_std, conditional, num_draws, method, options, seed, sample_offset, chunk_points,
                             num_probes, min_weight, return_ess, return_noise_grad, **maps):
        """``log_prob_noisy_grad`` proper (``odeint.log_prob_noisy_grad`` around the two halves of ``log_prob_grad``);
        ``maps``: the affine input map and the conditional scale of the population wrappers."""
        value_maps = {k: v for k, v in maps.items() if k != "cond_tangent_scale"}
        hutch = bool(self.hutch)

        def checks():
            self._logp_grad_checks(x, conditional, method, options, "philox" if hutch else "torch", 0 if hutch else None, 0,
                                   num_probes)

        def value_rows(y, c, extra):
            rng = (extra["seed"], extra["sample_offset"]) if extra else None
            lp = self._logp_value(y, c, method, options, rng, num_probes, **value_maps)
            return lp, ((self.e if self.e.dim() == 3 else self.e.unsqueeze(1)) if hutch else None)

        def grad_rows(y, c, probes):
            gx, gc = self._logp_grad_rows(y, c, method, options, probes, **maps)
            return gx, gc, y.shape[0] * (probes.shape[1] if hutch else y.shape[1])

        self.last_noisy_grad_stats = {}
        out = odeint.log_prob_noisy_grad(value_rows, grad_rows, hutch, x, noise_std, conditional, num_draws, method, seed,
                                         sample_offset, chunk_points, min_weight, return_ess, return_noise_grad, checks=checks,
                                         stats=self.last_noisy_grad_stats)
        return (out[0].view(-1, 1),) + out[1:]

    @torch.no_grad()
    def log_prob_noisy(self, x, noise_std, conditional=None, num_draws=16, atol=1e-4, rtol=1e-4, method="dopri5",
                       options={"min_step": 1e-6}, *, seed=None, sample_offset=0, chunk_points=None, return_ess=False,
                       num_probes=1):
        """Extension: the log-density of noisy observations.  ``x`` [B, D] (fp32, on the GPU) was measured with Gaussian
        errors of known standard deviation ``noise_std`` ([B, D], [D] or a scalar; finite, >= 0), so what a likelihood
        needs is the convolved density ``p_obs(x | noise_std) = E_{z ~ N(0, I)}[p(x - noise_std z)]``.  Returns its estimate
        from ``num_draws`` = K draws per point, ``logsumexp_k log p(x - noise_std z_k) - log K`` [B, 1]; with
        ``return_ess=True`` ``(log_p [B, 1], ess [B])``, ess the effective sample size of the K weights, in (0, K].
        ``log_prob`` itself (``conditional``, ``atol``, ``rtol``, ``method``, ``options``, ``num_probes`` as there) runs on
        the B K expanded rows; ``seed`` / ``sample_offset`` / ``chunk_points`` and the chunking rules:
        ``odeint.log_prob_noisy``.  With ``noise_std = 0, num_draws = 1`` this is ``log_prob`` bit for bit.

        A model built with ``hutchinson=True`` takes the probes of the expanded rows from ``probe="philox"`` under the same
        ``seed``, keyed by the expanded global row.  Mind what it estimates: the Hutchinson divergence is unbiased for
        log p, but here it sits inside an exponent, and E[exp(noisy)] > exp(E[noisy]) -- the estimate of p_obs is biased
        upwards by about half the variance of the divergence estimate (``num_probes`` shrinks it).  Exact-trace models are
        the clean case.  Hutch++ / XTrace models go through their ``log_prob`` as they are (probes from torch's generator
        per chunk)."""
        rows = lambda y, c, extra: self.log_prob(y, conditional=c, atol=atol, rtol=rtol, method=method, options=options,
                                                 num_probes=num_probes, **extra)
        out = odeint.log_prob_noisy(rows, bool(self.hutch), x, noise_std, conditional, num_draws, method, seed,
                                    sample_offset, chunk_points, return_ess)
        return (out[0].view(-1, 1), out[1]) if return_ess else out.view(-1, 1)

    @torch.no_grad()
    def posterior_noisy(self, x, noise_std, conditional=None, num_draws=16, num_samples=1, atol=1e-4, rtol=1e-4,
                        method="dopri5", options={"min_step": 1e-6}, *, seed=None, sample_offset=0, chunk_points=None,
                        num_probes=1):
        """Extension: the per-object posterior ``p(x_true | x, noise_std) ~ p(x_true) N(x; x_true, diag noise_std^2)``
        of observations ``x`` [B, D] under the learned population, from the same ``num_draws`` = K draws that
        ``log_prob_noisy`` makes (arguments, seed and chunking rules as there).  The K candidates ``x - noise_std z_k``
        with weights ``w_k ~ p(candidate k)`` are a self-normalised importance sample of it.  Returns a
        ``NoisyPosterior``: ``samples`` [B, M, D] (M = ``num_samples`` multinomial draws of the K candidates by their
        weights, in the units of ``x``), ``log_prob`` [B, 1] and ``ess`` [B] (bit for bit
        ``log_prob_noisy(..., return_ess=True)`` under the same seed), ``mean`` and ``var`` [B, D] (the weighted mean --
        the denoised, "shrunk" estimate -- and variance of the candidates) and ``index`` [B, M] (int32: which candidate
        each sample is).

        The samples are a RESAMPLE of K particles: only as many distinct points as the effective sample size allows.
        Read ``ess`` before trusting ``samples`` (an ess near 1: every draw is the same candidate, ``var`` near 0), and
        raise ``num_draws``, not ``num_samples``, to get more of them.  With a ``hutchinson=True`` model the weights carry
        the noise of the divergence estimate (see ``log_prob_noisy``); exact-trace models are the clean case."""
        rows = lambda y, c, extra: self.log_prob(y, conditional=c, atol=atol, rtol=rtol, method=method, options=options,
                                                 num_probes=num_probes, **extra)
        post = odeint.posterior_noisy(rows, bool(self.hutch), x, noise_std, conditional, num_draws, num_samples, method, seed,
                                      sample_offset, chunk_points)
        return post._replace(log_prob=post.log_prob.view(-1, 1))


# ------------------------------------------------------------------------------------------------
# population-model wrappers (affine pre/post-processing; reference: diffusion.py:1466-1848)
# ------------------------------------------------------------------------------------------------
class _PopulationModel(nn.Module):
    """What the two wrappers share: a ``ScoreModel`` between ``(x - shift) / scale`` and ``x * scale + shift``."""

    def __init__(self, model, sde, score_model, shift, scale, method, options):
        super().__init__()
        self.model = model
        self.sde = sde
        self.score_model = score_model
        n = self.model.n_dimensions
        self.register_buffer("shift", shift if shift is not None else torch.zeros(n, dtype=torch.float32))
        self.register_buffer("scale", scale if scale is not None else torch.ones(n, dtype=torch.float32))
        self.method = method
        self.options = options

    def _cond(self, conditional):
        return None

    def _forward(self, base_samples, conditional):
        kernel_maps = self.scale.dtype == torch.float32 and self.shift.dtype == torch.float32
        x = self.score_model._sample_ode(base_samples, self._cond(conditional), 1e-5, 1e-5, self.method, self.options,
                                         **({"out_scale": self.scale, "out_shift": self.shift} if kernel_maps else {}))
        # (e.g. float64 statistics from numpy: the reference's `* scale + shift` then promotes the result -- so does this)
        return x if kernel_maps else x * self.scale + self.shift

    def _sample_sde(self, shape, conditional):
        # the reference ignores `steps` here and always takes 100 (diffusion.py:1608)
        return self.score_model.sample_sde(shape, conditional=self._cond(conditional), steps=100) * self.scale + self.shift

    def _log_prob(self, x, conditional, atol, rtol, num_probes, probe_rng=None):
        # the reference does not forward self.method here: the solver default applies (diffusion.py:1633-1635)
        xT, lp, _ = self.score_model._solve_forward(x, self._cond(conditional), atol, rtol, "dopri5", self.options,
                                                    in_shift=self.shift, in_scale=self.scale, num_probes=num_probes,
                                                    probe_rng=probe_rng)
        return lp + torch.sum(self.sde.prior(xT.shape).log_prob(xT), 1, keepdim=True)

    def _push_maps(self, conditional, direction):
        """(normalised conditional, keywords of ``odeint.solve_push``) of the wrappers' sensitivity solves, in the units of
        the user's ``x`` and ``conditional``: ``to_data`` is ``forward``'s solve (``* scale + shift`` in the kernel),
        ``to_base`` is ``log_prob``'s (``(x - shift) / scale`` in the kernel); tangents of the raw conditional are divided
        by ``conditional_scale`` on the host."""
        maps = {"out_scale": self.scale, "out_shift": self.shift} if direction == "to_data" else \
            {"in_shift": self.shift, "in_scale": self.scale}
        if conditional is None:
            return None, maps
        C = int(self.model.n_conditionals)
        if not hasattr(self, "conditional_scale") or not torch.is_tensor(conditional) or conditional.dim() != 2 or \
                conditional.shape[1] != C:
            raise ValueError(f"flow-map sensitivities: conditional must be [batch, {C}] (and the wrapper a conditional one)")
        return self._cond(conditional), dict(maps, cond_tangent_scale=self.conditional_scale)

    @torch.no_grad()
    def _flow_jvp(self, x, tangents, conditional, conditional_tangents, direction, method, options):
        """``flow_jvp`` of the two wrappers: ``ScoreModel.flow_jvp`` of the inner score model between the wrappers' affine
        maps, so that ``x``, ``x_out``, ``conditional`` and every tangent are in the user's units."""
        cond, maps = self._push_maps(conditional, direction)
        return self.score_model._flow_jvp(x, tangents, cond, conditional_tangents, direction, method, options, **maps)

    @torch.no_grad()
    def _flow_jacobian(self, x, conditional, direction, method, options):
        cond, maps = self._push_maps(conditional, direction)
        return self.score_model._flow_jacobian(x, cond, direction, method, options, **maps)

    @torch.no_grad()
    def _flow_vjp(self, x, cotangents, conditional, direction, method, options, return_retrace, adjoint="continuous"):
        """``flow_vjp`` of the two wrappers: ``ScoreModel.flow_vjp`` of the inner score model between the wrappers' affine
        maps, so that ``x``, ``x_out``, ``conditional`` and every cotangent are in the user's units."""
        cond, maps = self._push_maps(conditional, direction)
        return self.score_model._flow_vjp(x, cotangents, cond, direction, method, options, return_retrace, adjoint, **maps)

    @torch.no_grad()
    def _log_prob_grad(self, x, conditional, method, options, probe, seed, sample_offset, num_probes):
        """``log_prob_grad`` of the two wrappers: ``ScoreModel.log_prob_grad`` of the inner score model behind ``(x - shift) /
        scale`` (in the kernel), so that ``grad_x`` is in the units of the user's ``x`` and ``grad_c`` in those of the RAW
        conditional.  ``log_p`` is this wrapper's ``log_prob`` formula on the fixed grid of ``method`` / ``options`` (its
        ``log_prob`` itself is hard-wired to adaptive dopri5, which has no discrete adjoint)."""
        cond, maps = self._logp_grad_maps(conditional)
        return self.score_model._log_prob_grad(x, cond, method, options, probe, seed, sample_offset, num_probes, **maps)

    def _logp_grad_maps(self, conditional):
        """(normalised conditional, the maps of the inner score model's log-density gradients) in the user's units."""
        cond, maps = None, {"in_shift": self.shift, "in_scale": self.scale}
        if conditional is not None:
            C = int(self.model.n_conditionals)
            if not hasattr(self, "conditional_scale") or not torch.is_tensor(conditional) or conditional.dim() != 2 or \
                    conditional.shape[1] != C:
                raise ValueError(f"log-density gradients: conditional must be [batch, {C}] (and the wrapper a conditional one)")
            cond, maps = self._cond(conditional), dict(maps, cond_tangent_scale=self.conditional_scale)
        return cond, maps

    @torch.no_grad()
    def _log_prob_noisy_grad(self, x, noise_std, conditional, num_draws, method, options, seed, sample_offset, chunk_points,
                             num_probes, min_weight, return_ess, return_noise_grad):
        """``log_prob_noisy_grad`` of the two wrappers: ``ScoreModel.log_prob_noisy_grad`` of the inner score model behind
        ``(x - shift) / scale`` (in the kernel).  The noise lives in the data space of ``x``, so ``grad_x`` and
        ``grad_noise_std`` are in the units of the user's ``x`` and ``noise_std``, ``grad_c`` in those of the RAW conditional
        (normalised per point, then repeated for the draws).  ``log_p`` is ff_logmeanexp of this wrapper's ``log_prob``
        formula on the fixed grid of ``method`` / ``options``, as in ``_log_prob_grad`` (its ``log_prob_noisy`` itself is
        hard-wired to adaptive dopri5, which has no discrete adjoint)."""
        cond, maps = self._logp_grad_maps(conditional)
        out = self.score_model._log_prob_noisy_grad(x, noise_std, cond, num_draws, method, options, seed, sample_offset,
                                                    chunk_points, num_probes, min_weight, return_ess, return_noise_grad, **maps)
        self.last_noisy_grad_stats = self.score_model.last_noisy_grad_stats
        return out

    @torch.no_grad()
    def _log_prob_noisy(self, x, noise_std, conditional, num_draws, atol, rtol, seed, sample_offset, chunk_points,
                        return_ess, num_probes):
        """``log_prob_noisy`` of the two wrappers: ``ScoreModel.log_prob_noisy`` around this wrapper's own ``log_prob`` --
        the noise lives in the data space of ``x``, before ``(x - shift) / scale``, and the expanded rows take the affine
        map where every row of ``log_prob`` does.  The solve is hard-wired to adaptive dopri5, like
        ``log_prob``'s: all B K rows are one solve, and ``chunk_points`` raises."""
        def rows(y, c, extra):
            rng = (extra["seed"], extra["sample_offset"]) if extra else None
            return self._log_prob(y, c, atol, rtol, num_probes, probe_rng=rng)
        out = odeint.log_prob_noisy(rows, bool(self.score_model.hutch), x, noise_std, conditional, num_draws, "dopri5",
                                    seed, sample_offset, chunk_points, return_ess)
        return (out[0].view(-1, 1), out[1]) if return_ess else out.view(-1, 1)

    @torch.no_grad()
    def _posterior_noisy(self, x, noise_std, conditional, num_draws, num_samples, atol, rtol, seed, sample_offset,
                         chunk_points, num_probes):
        """``posterior_noisy`` of the two wrappers, around this wrapper's own ``log_prob`` like ``_log_prob_noisy``: the
        candidates, and so ``samples``, ``mean`` and ``var``, are in the data space of ``x`` (before ``(x - shift) /
        scale``)."""
        def rows(y, c, extra):
            rng = (extra["seed"], extra["sample_offset"]) if extra else None
            return self._log_prob(y, c, atol, rtol, num_probes, probe_rng=rng)
        post = odeint.posterior_noisy(rows, bool(self.score_model.hutch), x, noise_std, conditional, num_draws, num_samples,
                                      "dopri5", seed, sample_offset, chunk_points)
        return post._replace(log_prob=post.log_prob.view(-1, 1))


class PopulationModelDiffusion(_PopulationModel):
    def __init__(self, model=None, sde=None, shift=None, scale=None, method="dopri5", no_sigma=False,
                 hutchinson=False, options=None, *, precision="f32"):
        """Arguments as in the reference (diffusion.py:1466-1530); ``precision`` (keyword only, extension) is handed to the
        inner ``ScoreModel`` (see there)."""
        score_model = ScoreModel(model=model, sde=sde, hutchinson=hutchinson, no_sigma=no_sigma, precision=precision)
        super().__init__(model, sde, score_model, shift, scale, method, options)

    def forward(self, base_samples):
        return self._forward(base_samples, None)

    def sample_sde(self, shape, steps=100):
        return self._sample_sde(shape, None)

    def log_prob(self, x, atol=1e-5, rtol=1e-5, *, num_probes=1):
        """(No ``return_stderr`` here: like the reference's, this solve is hard-wired to adaptive dopri5, and per-probe
        divergences are carried by fixed-grid solves only -- ``self.score_model.log_prob(..., method="rk4",
        options={"step_size": h}, num_probes=K, return_stderr=True)`` on the normalised points is the route.)
        ``num_probes`` (extension): see ``ScoreModel.solve_odes_forward``; a model built with ``hutchinson=True``."""
        return self._log_prob(x, None, atol, rtol, num_probes)

    def log_prob_grad(self, x, conditional=None, *, method="rk4", options=None, probe="torch", seed=None, sample_offset=0,
                      num_probes=1):
        """Extension: ``ScoreModel.log_prob_grad`` in the units of this wrapper: ``(log_p [B, 1], grad_x [B, D], None)`` on
        the fixed grid of ``method`` / ``options`` (the default grid is ONE rk4 step: pass ``options={"step_size": h}``).
        ``conditional`` must stay None (the signature is the conditional wrapper's).  See ``_log_prob_grad``."""
        if conditional is not None:
            raise ValueError("log-density gradients: this model has no conditional inputs")
        return self._log_prob_grad(x, None, method, options, probe, seed, sample_offset, num_probes)

    def log_prob_noisy_grad(self, x, noise_std, num_draws=16, *, method="rk4", options=None, seed=None, sample_offset=0,
                            chunk_points=None, num_probes=1, min_weight=0.0, return_ess=False, return_noise_grad=False):
        """Extension: ``ScoreModel.log_prob_noisy_grad`` in the units of this wrapper: ``(log_p [B, 1], grad_x [B, D], None
        [, ess [B]] [, grad_noise_std [B, D]])`` of observations ``x`` measured with Gaussian errors ``noise_std``, on the
        fixed grid of ``method`` / ``options`` (the default grid is ONE rk4 step: pass ``options={"step_size": h}``).
        ``min_weight`` and ``self.last_noisy_grad_stats``: as there.  See ``_log_prob_noisy_grad``."""
        return self._log_prob_noisy_grad(x, noise_std, None, num_draws, method, options, seed, sample_offset, chunk_points,
                                         num_probes, min_weight, return_ess, return_noise_grad)

    def flow_jvp(self, x, tangents, *, direction="to_data", method="rk4", options=None):
        """Extension: ``ScoreModel.flow_jvp`` in the units of this wrapper: ``to_data`` differentiates ``forward(x)``
        (``x`` = base samples), ``to_base`` the map of ``log_prob`` from data ``x`` to the base; ``(x_out [B, D],
        dx [B, K, D])``.  The default grid is one rk4 step: pass ``options={"step_size": h}``."""
        return self._flow_jvp(x, tangents, None, None, direction, method, options)

    def flow_jacobian(self, x, *, direction="to_data", method="rk4", options=None):
        """Extension: ``ScoreModel.flow_jacobian`` in the units of this wrapper: ``(x_out [B, D], J_x [B, D, D], None)``."""
        return self._flow_jacobian(x, None, direction, method, options)

    def flow_vjp(self, x, cotangents, *, direction="to_data", method="rk4", options=None, return_retrace=False,
                 adjoint="continuous"):
        """Extension: ``ScoreModel.flow_vjp`` in the units of this wrapper: ``(x_out [B, D], gx [B, K, D], None)`` (and
        ``retrace [B]``), ``gx[b, k] = cotangents[b, k]^T d x_out[b] / d x[b]`` -- the continuous adjoint: use rk4 or
        better, read ``retrace``, raise the step count (``options={"step_size": h}``; the default grid is ONE step).
        ``adjoint="discrete"``: the exact discrete adjoint from recorded stage states instead -- the transpose of
        ``flow_jvp`` at any step count, the default one-step grid included; nothing is retraced."""
        return self._flow_vjp(x, cotangents, None, direction, method, options, return_retrace, adjoint)

    def log_prob_noisy(self, x, noise_std, num_draws=16, atol=1e-5, rtol=1e-5, *, seed=None, sample_offset=0,
                       chunk_points=None, return_ess=False, num_probes=1):
        """Extension: ``log_prob`` of observations ``x`` measured with Gaussian errors ``noise_std`` (in the units of ``x``),
        from ``num_draws`` noise draws per point: [B, 1], with ``return_ess=True`` ``(log_p [B, 1], ess [B])``.  See
        ``ScoreModel.log_prob_noisy`` (a ``hutchinson=True`` model: the bias of a noisy divergence inside an exponent)
        and ``_log_prob_noisy``."""
        return self._log_prob_noisy(x, noise_std, None, num_draws, atol, rtol, seed, sample_offset, chunk_points,
                                    return_ess, num_probes)

    def posterior_noisy(self, x, noise_std, num_draws=16, num_samples=1, atol=1e-5, rtol=1e-5, *, seed=None,
                        sample_offset=0, chunk_points=None, num_probes=1):
        """Extension: the per-object posterior of observations ``x`` measured with Gaussian errors ``noise_std`` under this
        population model, from the ``num_draws`` candidates of ``log_prob_noisy``: a ``NoisyPosterior`` whose ``samples``
        [B, ``num_samples``, D], ``mean`` and ``var`` are in the units of ``x``.  Read ``ess`` before trusting ``samples``
        and raise ``num_draws``, not ``num_samples``: see ``ScoreModel.posterior_noisy`` and ``_posterior_noisy``."""
        return self._posterior_noisy(x, noise_std, None, num_draws, num_samples, atol, rtol, seed, sample_offset,
                                     chunk_points, num_probes)


class PopulationModelDiffusionConditional(_PopulationModel):
    def __init__(self, model=None, sde=None, shift=None, scale=None, conditional_shift=None,
                 conditional_scale=None, no_sigma=False, method="dopri5", options=None, *, precision="f32"):
        score_model = ScoreModel(model=model, sde=sde, no_sigma=no_sigma, precision=precision)
        super().__init__(model, sde, score_model, shift, scale, method, options)
        c = self.model.n_conditionals
        self.register_buffer("conditional_shift",
                             conditional_shift if conditional_shift is not None else torch.zeros(c, dtype=torch.float32))
        self.register_buffer("conditional_scale",
                             conditional_scale if conditional_scale is not None else torch.ones(c, dtype=torch.float32))

    def _cond(self, conditional):
        return (conditional - self.conditional_shift) / self.conditional_scale

    def forward(self, base_samples, conditional=None):
        return self._forward(base_samples, conditional)

    def sample_sde(self, shape, conditional=None, steps=100):
        return self._sample_sde(shape, conditional)

    def log_prob(self, x, conditional=None, atol=1e-5, rtol=1e-5, *, num_probes=1):
        """(No ``return_stderr`` here: like the reference's, this solve is hard-wired to adaptive dopri5 -- and this
        wrapper's score model takes the exact trace, which has no probes to spread; ``num_probes`` > 1 is refused there.)"""
        return self._log_prob(x, conditional, atol, rtol, num_probes)

    def log_prob_grad(self, x, conditional=None, *, method="rk4", options=None, probe="torch", seed=None, sample_offset=0,
                      num_probes=1):
        """Extension: ``ScoreModel.log_prob_grad`` in the units of this wrapper: ``(log_p [B, 1], grad_x [B, D],
        grad_c [B, C])`` with ``grad_c`` the gradient with respect to the RAW conditional (the population
        hyper-parameters), on the fixed grid of ``method`` / ``options`` (the default grid is ONE rk4 step: pass
        ``options={"step_size": h}``).  This wrapper's score model takes the exact trace.  See ``_log_prob_grad``."""
        return self._log_prob_grad(x, conditional, method, options, probe, seed, sample_offset, num_probes)

    def log_prob_noisy_grad(self, x, noise_std, conditional=None, num_draws=16, *, method="rk4", options=None, seed=None,
                            sample_offset=0, chunk_points=None, num_probes=1, min_weight=0.0, return_ess=False,
                            return_noise_grad=False):
        """Extension: ``ScoreModel.log_prob_noisy_grad`` in the units of this wrapper: ``(log_p [B, 1], grad_x [B, D],
        grad_c [B, C] [, ess [B]] [, grad_noise_std [B, D]])`` of observations ``x`` measured with Gaussian errors
        ``noise_std``, ``grad_c`` with respect to the RAW conditional (the population hyper-parameters: ``grad_c.sum(0)`` is
        the gradient of the hierarchical likelihood of a catalogue that shares them), on the fixed grid of ``method`` /
        ``options`` (the default grid is ONE rk4 step: pass ``options={"step_size": h}``).  This wrapper's score model takes
        the exact trace: D gradient rows per kept draw, ``min_weight`` is the lever.  See ``_log_prob_noisy_grad``."""
        return self._log_prob_noisy_grad(x, noise_std, conditional, num_draws, method, options, seed, sample_offset,
                                         chunk_points, num_probes, min_weight, return_ess, return_noise_grad)

    def flow_jvp(self, x, tangents=None, conditional=None, conditional_tangents=None, *, direction="to_data", method="rk4",
                 options=None):
        """Extension: ``ScoreModel.flow_jvp`` in the units of this wrapper: ``to_data`` differentiates ``forward(x,
        conditional)``, ``to_base`` the map of ``log_prob`` from data ``x`` to the base, along ``tangents`` [B, K, D] in ``x``
        and ``conditional_tangents`` [B, K, C] in the RAW conditional (the population hyper-parameters); ``(x_out [B, D],
        dx [B, K, D])``.  The default grid is one rk4 step: pass ``options={"step_size": h}``."""
        return self._flow_jvp(x, tangents, conditional, conditional_tangents, direction, method, options)

    def flow_jacobian(self, x, conditional=None, *, direction="to_data", method="rk4", options=None):
        """Extension: ``ScoreModel.flow_jacobian`` in the units of this wrapper: ``(x_out [B, D], J_x [B, D, D],
        J_c [B, D, C])``, ``J_c`` with respect to the RAW conditional."""
        return self._flow_jacobian(x, conditional, direction, method, options)

    def flow_vjp(self, x, cotangents, conditional=None, *, direction="to_data", method="rk4", options=None,
                 return_retrace=False, adjoint="continuous"):
        """Extension: ``ScoreModel.flow_vjp`` in the units of this wrapper: ``(x_out [B, D], gx [B, K, D], gc [B, K, C])``
        (and ``retrace [B]``), ``gc`` with respect to the RAW conditional (the population hyper-parameters) -- the
        continuous adjoint: use rk4 or better, read ``retrace``, raise the step count (``options={"step_size": h}``; the
        default grid is ONE step).  ``adjoint="discrete"``: the exact discrete adjoint from recorded stage states instead
        -- the transpose of ``flow_jvp`` at any step count, the default one-step grid included; nothing is retraced."""
        return self._flow_vjp(x, cotangents, conditional, direction, method, options, return_retrace, adjoint)

    def log_prob_noisy(self, x, noise_std, conditional=None, num_draws=16, atol=1e-5, rtol=1e-5, *, seed=None,
                       sample_offset=0, chunk_points=None, return_ess=False, num_probes=1):
        """Extension: ``log_prob`` of observations ``x`` measured with Gaussian errors ``noise_std`` (in the units of ``x``),
        from ``num_draws`` noise draws per point; the raw ``conditional`` [B, C] is repeated for the draws.  See
        ``PopulationModelDiffusion.log_prob_noisy``."""
        return self._log_prob_noisy(x, noise_std, conditional, num_draws, atol, rtol, seed, sample_offset, chunk_points,
                                    return_ess, num_probes)

    def posterior_noisy(self, x, noise_std, conditional=None, num_draws=16, num_samples=1, atol=1e-5, rtol=1e-5, *,
                        seed=None, sample_offset=0, chunk_points=None, num_probes=1):
        """Extension: the per-object posterior of observations ``x`` measured with Gaussian errors ``noise_std`` given the
        raw ``conditional`` [B, C] (repeated for the draws): a ``NoisyPosterior`` in the units of ``x``.  Read ``ess`` before
        trusting ``samples`` and raise ``num_draws``, not ``num_samples``: see ``PopulationModelDiffusion.posterior_noisy``."""
        return self._posterior_noisy(x, noise_std, conditional, num_draws, num_samples, atol, rtol, seed, sample_offset,
                                     chunk_points, num_probes)
