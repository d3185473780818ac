"""Reference for the leapfrog pull-backs (``FusedPair.pullback_select``, ``odeint.solve_leapfrog_pull``,
``SymplecticFlowModel.sample_leapfrog_vjp`` / ``log_prob_leapfrog_grad``; csrc/ff_mlp_pullsel.hpp), in the style of
tests/_symplectic_ref.py: the library's ``SymplecticMLP`` restated in plain torch in float64 or fp32, the rows of
``solvers.plan_leapfrog`` (or of a hand-built plan) stepped one by one with every state kept, and ``torch.autograd.grad``
through them.

A table row ``(t, w, net_b)`` is the shear the kernels apply: ``p += w (-mlp_p(q, c, t))`` if ``net_b`` else
``q += w mlp_q(p, c, t)``, with ``w = sign * cout[0]`` of the row (``b = sign`` and ``x += cout[0] * b * NET``).

``pull_ref``     what the raw launch computes, by autograd: from ``z`` (the END of a forward leapfrog) the retraced start
                 ``z_back`` = the backward rows applied to ``z``, then the gradient of ``cot . F(z_back, c)`` with respect to
                 ``z_back`` and ``c``, F = the backward rows undone in reverse order (weights negated): the forward leapfrog.
``sweep_ref``    the kernel's own algorithm, written out: per backward row ONE network evaluation at the held state gives the
                 un-shear and, through ``torch.func.vjp``, the transposed-Jacobian products of the same evaluation.
``Damage``       the wrong-weight-path variants the host file holds every case against.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from flowfusion_amd import solvers
from flowfusion_amd import symplectic as Sm
from tests._deep_models import apply_gain

E_DIMS = 4          # time-embedding features of every test model


def make_model(D, C, units, gain=1.0, seed=5, affine=False):
    """A seeded ``SymplecticFlowModel`` on the CPU with the hidden-to-hidden weights of BOTH networks multiplied by ``gain``
    (tests/_deep_models.py).  ``affine``: shift / scale / conditional shift / conditional scale that are not the identity."""
    torch.manual_seed(seed)
    mlp = Sm.SymplecticMLP(D, C, E_DIMS, list(units))
    for seq in (mlp.mlp_q_dynamics, mlp.mlp_p_dynamics):
        apply_gain([l for l in seq if isinstance(l, torch.nn.Linear)], float(gain))
    if affine:
        shift, scale = torch.linspace(-1.0, 1.0, D), torch.linspace(0.5, 2.0, D)
        cshift, cscale = (torch.linspace(-0.5, 0.5, C), torch.linspace(0.75, 1.5, C)) if C else (None, None)
    else:
        shift, scale = torch.zeros(D), torch.ones(D)
        cshift, cscale = (torch.zeros(C), torch.ones(C)) if C else (None, None)
    return Sm.SymplecticFlowModel(mlp, shift, scale, cshift, cscale).eval()


@dataclass(frozen=True)
class Damage:
    """A wrong weight path: ``swap = (network 0 = mlp_q / 1 = mlp_p, hidden layer, (i, j))`` exchanges two output rows of the
    weight matrix that produces that hidden layer (biases stay); ``exchange`` runs mlp_p where mlp_q belongs and the other
    way round; ``drop_gamma = network`` leaves that network's contribution to the conditional's gradient out."""
    swap: Optional[Tuple[int, int, Tuple[int, int]]] = None
    exchange: bool = False
    drop_gamma: Optional[int] = None


def plan_rows(plan):
    """[(t, w, net_b)] of an ``EvalPlan`` of select rows: fp32 time, signed fp32 weight, bool."""
    w = plan.sign * plan.cout[:, 0]
    nb = (plan.flags & solvers.FLAG_NET_B) != 0
    return [(plan.t_eval[i].clone(), w[i].clone(), bool(nb[i])) for i in range(int(plan.t_eval.numel()))]


def undo_rows(rows):
    """The rows that undo ``rows``: reverse order, weights negated."""
    return [(t, -w, nb) for (t, w, nb) in reversed(rows)]


class LeapfrogRef:
    """The two networks of a ``SymplecticFlowModel`` in ``dtype`` on the CPU, and shears built from them."""

    def __init__(self, front, dtype=torch.float64, damage: Damage = Damage()):
        self.dtype, self.damage = dtype, damage
        m = front.model
        self.W = m.W.detach().to("cpu", dtype)
        cp = lambda seq: [[l.weight.detach().to("cpu", dtype).clone(), l.bias.detach().to("cpu", dtype).clone()]
                          for l in seq if isinstance(l, torch.nn.Linear)]
        self.nets = [cp(m.mlp_q_dynamics), cp(m.mlp_p_dynamics)]
        if damage.swap is not None:
            n, layer, (i, j) = damage.swap
            w = self.nets[n][layer][0]
            w[[i, j]] = w[[j, i]]
        if damage.exchange:
            self.nets = self.nets[::-1]
        self.D = int(self.nets[0][-1][0].shape[0])

    def net(self, which, half, cond, t):
        """mlp_q (``which`` 0) or mlp_p (1) at ``[half | cond | emb(t)]``; ``t`` an fp32 scalar tensor (the table's time)."""
        tt = t.to(self.dtype).expand(half.shape[0])
        arg = tt[:, None] * self.W[None, :] * 2 * math.pi
        emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        if cond is not None and self.damage.drop_gamma == which:
            cond = cond.detach()
        h = torch.cat([half] + ([cond] if cond is not None else []) + [emb], dim=1)
        layers = self.nets[which]
        for i, (w, b) in enumerate(layers):
            h = h @ w.T + b
            if i < len(layers) - 1:
                h = h * torch.sigmoid(h)
        return h

    def run(self, z, cond, rows):
        """The state after the shears ``rows``."""
        D = self.D
        q, p = z[:, :D], z[:, D:]
        for t, w, nb in rows:
            w = w.to(self.dtype)
            if nb:
                p = p + w * (-self.net(1, q, cond, t))
            else:
                q = q + w * self.net(0, p, cond, t)
        return torch.cat([q, p], dim=1)

    def cast(self, t):
        return None if t is None else t.detach().to("cpu", self.dtype)

    def vjp(self, z0, cond, rows, cot):
        """(z_out, gz [B, K, 2D], gc [B, K, C] or None) of ``run`` at (z0, cond), by ``torch.autograd.grad``."""
        z0 = self.cast(z0).requires_grad_(True)
        cond = None if cond is None else self.cast(cond).requires_grad_(True)
        cot = self.cast(cot)
        out = self.run(z0, cond, rows)
        gz, gc = [], []
        for k in range(cot.shape[1]):
            g = torch.autograd.grad((out * cot[:, k]).sum(), [z0] + ([cond] if cond is not None else []), retain_graph=True,
                                    allow_unused=True)
            gz.append(g[0])
            if cond is not None:
                gc.append(torch.zeros_like(cond) if g[1] is None else g[1])
        return out.detach(), torch.stack(gz, dim=1), (torch.stack(gc, dim=1) if cond is not None else None)

    def pull_ref(self, z, cond, back_rows, cot):
        """What the raw launch returns: (z_back, gz, gc), the derivatives by autograd through the kept states."""
        with torch.no_grad():
            z_back = self.run(self.cast(z), self.cast(cond), back_rows)
        _, gz, gc = self.vjp(z_back, cond, undo_rows(back_rows), cot)
        return z_back, gz, gc

    def sweep_ref(self, z, cond, back_rows, cot):
        """The kernel's algorithm: one retracing sweep over the backward rows, nothing kept."""
        D = self.D
        y, c = self.cast(z).clone(), self.cast(cond)
        alpha = self.cast(cot).clone()
        B, K = alpha.shape[0], alpha.shape[1]
        gamma = None if c is None else torch.zeros(B, K, c.shape[1], dtype=self.dtype)
        for t, w, nb in back_rows:
            w = w.to(self.dtype)
            src = slice(0, D) if nb else slice(D, 2 * D)       # the half the network reads
            dst = slice(D, 2 * D) if nb else slice(0, D)       # the half the row moves
            sgn = -1.0 if nb else 1.0
            if c is None:
                f, pull = torch.func.vjp(lambda h: sgn * self.net(int(nb), h, None, t), y[:, src])
            else:
                f, pull = torch.func.vjp(lambda h, cc: sgn * self.net(int(nb), h, cc, t), y[:, src], c)
            for k in range(K):
                g = pull(alpha[:, k, dst].contiguous())
                alpha[:, k, src] = alpha[:, k, src] - w * g[0]
                if c is not None and self.damage.drop_gamma != int(nb):
                    gamma[:, k] = gamma[:, k] - w * g[1]
            y[:, dst] = y[:, dst] + w * f
        return y, alpha, gamma


def normalised_pair(gz, gc, rz, rc):
    """One normalised error for a (gz, gc) pair against its reference: the larger of the two."""
    from tests._pushforward_ref import normalised_error
    e = normalised_error(gz, rz)
    if rc is not None:
        e = max(e, normalised_error(gc, rc))
    return e


# ---- the raw cases: the smallest at which each thing can go wrong --------------------------------------------------------------
# (D, C, units, gain, steps, K, B[, "maps"]); steps = leapfrog steps of the BACKWARD grid linspace(0, 1, steps + 1).flip(0)
# (2 steps + 1 rows, first and last on net B), or "hand" for the hand-built table whose rows select A, A, B, B, A.
# B = samples per tile + 1 for the K of the case (a tile holds 16 // (1 + K)), or 1 / 17.  Gains: hidden-to-hidden weights
# x 1 .. 3 (seed 5), chosen on the CPU so that every damage misses the bar by 100 x (tests/test_leapfrog_pull_host.py).
RAW_CASES = [
    (1, 0, [128], 1.0, 1, 1, 9),
    (4, 1, [128, 128], 2.0, 2, 2, 6),
    (5, 16, [128] * 4, 2.0, 3, 4, 4),
    (8, 0, [128] * 5, 2.0, 1, 7, 3),
    (9, 0, [128, 128], 2.0, 2, 15, 2),
    (16, 16, [256] * 2, 1.5, 2, 1, 9),
    (8, 1, [256] * 7, 2.0, 1, 1, 1),
    (4, 0, [256] * 8, 2.5, 1, 2, 17),
    (5, 1, [256, 192, 256], 2.0, 3, 1, 9),
    (4, 1, [128] * 2, 2.0, "hand", 2, 6),
    (4, 1, [128, 128], 2.0, 2, 2, 6, "maps"),
]
# the deepest depth the plan accepts per unit, K = 1
DEEP_CASES = [
    (4, 1, [128] * 36, 2.1, 1, 1, 9),
    (8, 0, [256] * 18, 2.85, 1, 1, 9),
    (16, 1, [256] * 17, 2.0, 1, 1, 9),
]
UNIT_OF = {0: "mlp_pullsel_m16_h128_d4_c4", 1: "mlp_pullsel_m16_h128_d4_c4", 2: "mlp_pullsel_m16_h128_d4_c4",
           3: "mlp_pullsel_m16_h128_d4_c4", 4: "mlp_pullsel_m16_h256_d8_c4", 5: "mlp_pullsel_m16_h256_d8_c4",
           6: "mlp_pullsel_m16_h256_d4_c4", 7: "mlp_pullsel_m16_h256_d4_c4", 8: "mlp_pullsel_m16_h256_d4_c4",
           9: "mlp_pullsel_m16_h128_d4_c4", 10: "mlp_pullsel_m16_h128_d4_c4"}


def case_id(case):
    D, C, units, gain, steps, K, B = case[:7]
    return f"D{D}-C{C}-{len(units)}x{max(units)}{'r' if len(set(units)) > 1 else ''}-g{gain}-s{steps}-K{K}-B{B}" + \
        ("-maps" if len(case) > 7 else "")


def hand_plan():
    """Five select rows that choose A, A, B, B, A: a wrong next-row prefetch shows."""
    t = torch.tensor([0.9, 0.7, 0.55, 0.3, 0.1], dtype=torch.float32)
    w = torch.tensor([0.2, 0.15, 0.25, 0.1, 0.3], dtype=torch.float32)
    flags = torch.full((5,), solvers.FLAG_STEP_END, dtype=torch.int32)
    flags[2:4] |= solvers.FLAG_NET_B
    cout = torch.zeros(5, 8, dtype=torch.float32)
    cout[:, 0] = w
    return solvers.EvalPlan(t_eval=t, sign=-1.0, slot=torch.zeros(5, dtype=torch.int32), flags=flags,
                            cin=torch.zeros(5, 8, dtype=torch.float32), cout=cout, n_steps=5)


def case_plan(case):
    steps = case[4]
    if steps == "hand":
        return hand_plan()
    return solvers.plan_leapfrog(torch.linspace(0.0, 1.0, int(steps) + 1).flip(0))


def case_maps(case):
    """The affine maps of the raw launch of a case (None, or the four vectors over the joint state)."""
    if len(case) <= 7:
        return {}
    D2 = 2 * case[0]
    return dict(in_shift=torch.linspace(-0.3, 0.3, D2), in_scale=torch.linspace(0.8, 1.25, D2),
                out_scale=torch.linspace(0.9, 1.6, D2), out_shift=torch.linspace(0.2, -0.2, D2))


_SETUPS = {}


def case_setup(case):
    """(front, plan, rows, z, cot, cond) of a case, computed once: seeded inputs, the model on the CPU."""
    key = case_id(case)
    if key not in _SETUPS:
        D, C, units, gain, steps, K, B = case[:7]
        front = make_model(D, C, units, gain)
        g = torch.Generator().manual_seed(1234)
        z = torch.randn(B, 2 * D, generator=g)
        cot = torch.randn(B, K, 2 * D, generator=g)
        cond = torch.randn(B, C, generator=g) if C else None
        plan = case_plan(case)
        _SETUPS[key] = (front, plan, plan_rows(plan), z, cot, cond)
    return _SETUPS[key]


def raw_reference(case, dtype=torch.float64, damage=Damage()):
    """(z_back, gz, gc) of a raw case as the launch defines them, maps included: the launch integrates
    ``y = (z - in_shift) / in_scale``, takes cotangents times ``in_scale``, returns ``y_back * out_scale + out_shift`` and
    cotangents over ``out_scale``."""
    front, plan, rows, z, cot, cond = case_setup(case)
    ref = LeapfrogRef(front, dtype, damage)
    m = {k: v.to(dtype) for k, v in case_maps(case).items()}
    zz, cc = z.to(dtype), cot.to(dtype)
    if m:
        zz, cc = (zz - m["in_shift"]) / m["in_scale"], cc * m["in_scale"]
    zb, gz, gc = ref.pull_ref(zz, cond, rows, cc)
    if m:
        zb, gz = zb * m["out_scale"] + m["out_shift"], gz / m["out_scale"]
    return zb, gz, gc


_REFS = {}


def raw_floor_and_reference(case):
    """(floor, (z_back, gz, gc) in float64) of a case, computed once and shared: the floor is the fp32 reference's normalised
    error against float64 (tests/test_gpu_pushforward.py ``fp32_floor``)."""
    key = case_id(case)
    if key not in _REFS:
        from tests.test_gpu_pushforward import fp32_floor
        r64 = raw_reference(case, torch.float64)
        r32 = raw_reference(case, torch.float32)
        floor = fp32_floor(r32[1], r64[1])
        if r64[2] is not None:
            floor = max(floor, fp32_floor(r32[2], r64[2]))
        _REFS[key] = (floor, r64)
    return _REFS[key]


# ---- the front ends ---------------------------------------------------------------------------------------------------------
def _affine(front, dtype):
    cast = lambda t: None if t is None else t.detach().to("cpu", dtype)
    return cast(front.shift), cast(front.scale), cast(front.conditional_shift), cast(front.conditional_scale)


def sample_map(front, dtype=torch.float64):
    """(z [B, 2D], raw conditional, num_steps) -> x [B, D]: ``_sample_from(.., method="leapfrog")`` in ``dtype``."""
    ref = LeapfrogRef(front, dtype)
    shift, scale, cshift, cscale = _affine(front, dtype)

    def f(z, cond, num_steps):
        rows = plan_rows(solvers.plan_leapfrog(torch.linspace(1.0, 0.0, int(num_steps) + 1)))
        cn = None if cond is None else (cond - cshift) / cscale
        return ref.run(z, cn, rows)[:, :ref.D] * scale + shift
    return f


def sample_vjp_ref(front, z, cot, cond, num_steps, dtype=torch.float64):
    """(x, gz [B, K, 2D], gc [B, K, C] or None) of ``sample_leapfrog_vjp`` by autograd, gc for the RAW conditional."""
    f = sample_map(front, dtype)
    z = z.detach().to("cpu", dtype).requires_grad_(True)
    cond = None if cond is None else cond.detach().to("cpu", dtype).requires_grad_(True)
    cot = cot.detach().to("cpu", dtype)
    x = f(z, cond, num_steps)
    gz, gc = [], []
    for k in range(cot.shape[1]):
        g = torch.autograd.grad((x * cot[:, k]).sum(), [z] + ([cond] if cond is not None else []), retain_graph=True)
        gz.append(g[0])
        if cond is not None:
            gc.append(g[1])
    return x.detach(), torch.stack(gz, dim=1), (torch.stack(gc, dim=1) if cond is not None else None)


def logp_map(front, dtype=torch.float64):
    """(x [B, D], momentum [B, D], raw conditional, num_steps) -> log_p [B]: ``_log_prob_from(.., method="leapfrog")``."""
    ref = LeapfrogRef(front, dtype)
    shift, scale, cshift, cscale = _affine(front, dtype)

    def f(x, p0, cond, num_steps):
        rows = plan_rows(solvers.plan_leapfrog(torch.linspace(1.0, 0.0, int(num_steps) + 1).flip(0)))
        cn = None if cond is None else (cond - cshift) / cscale
        z1 = ref.run(torch.cat([(x - shift) / scale, p0], dim=1), cn, rows)
        logn = lambda v: (-0.5 * v ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
        return logn(z1) - logn(p0) - torch.log(scale).sum()
    return f


def logp_grad_ref(front, x, p0, cond, num_steps, dtype=torch.float64):
    """(log_p, grad_x, grad_c or None, grad_momentum) of ``log_prob_leapfrog_grad`` by autograd."""
    f = logp_map(front, dtype)
    x = x.detach().to("cpu", dtype).requires_grad_(True)
    p0 = p0.detach().to("cpu", dtype).requires_grad_(True)
    cond = None if cond is None else cond.detach().to("cpu", dtype).requires_grad_(True)
    lp = f(x, p0, cond, num_steps)
    g = torch.autograd.grad(lp.sum(), [x, p0] + ([cond] if cond is not None else []))
    return lp.detach(), g[0], (g[2] if cond is not None else None), g[1]


def logp_central_difference(front, x, p0, cond, num_steps, direction_x, direction_c=None, h=1e-6):
    """d log_p along (direction_x, direction_c) [B] by central differences of the float64 map (error ~ h^2 + 1e-16 / h)."""
    f = logp_map(front, torch.float64)
    d = lambda t: None if t is None else t.detach().to("cpu", torch.float64)
    x, p0, cond, dx, dc = d(x), d(p0), d(cond), d(direction_x), d(direction_c)
    up = f(x + h * dx, p0, None if cond is None else cond + h * (0 if dc is None else dc), num_steps)
    dn = f(x - h * dx, p0, None if cond is None else cond - h * (0 if dc is None else dc), num_steps)
    return (up - dn) / (2 * h)


# (D, C, units, gain, num_steps, B, affine): the front-end cases
SAMPLE_CASES = [
    (4, 3, [64, 64], 2.0, 2, 9, True),
    (9, 0, [128], 1.0, 1, 5, False),
]
LOGP_CASES = [
    (4, 3, [64, 64], 2.0, 2, 9, True),
    (16, 0, [256] * 3, 1.5, 4, 9, False),
    (5, 1, [128] * 2, 2.0, 1, 17, True),
]


def front_id(case):
    D, C, units, gain, steps, B, affine = case
    return f"D{D}-C{C}-{len(units)}x{max(units)}-g{gain}-n{steps}-B{B}" + ("-affine" if affine else "")


def front_inputs(case, K=3):
    """(front, z [B, 2D], x [B, D], momentum [B, D], cotangents [B, K, D], raw conditional or None), seeded."""
    D, C, units, gain, steps, B, affine = case
    front = make_model(D, C, units, gain, affine=affine)
    g = torch.Generator().manual_seed(4321)
    z = torch.randn(B, 2 * D, generator=g)
    x = torch.randn(B, D, generator=g)
    p0 = torch.randn(B, D, generator=g)
    cot = torch.randn(B, K, D, generator=g)
    cond = torch.randn(B, C, generator=g) if C else None
    return front, z, x, p0, cot, cond
