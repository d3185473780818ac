"""Reference for the leapfrog push-forwards (``FusedPair.pushforward_select``, ``odeint.solve_leapfrog_push`` /
``solve_leapfrog_push_jacobian``, ``SymplecticFlowModel.sample_leapfrog_jvp`` / ``sample_leapfrog_jacobian``;
csrc/ff_mlp_pushsel.hpp): the plain-torch restatement of tests/_leapfrog_pull_ref.py (``LeapfrogRef``: the library's
``SymplecticMLP`` in float64 or fp32, the rows of ``solvers.plan_leapfrog`` or of the hand-built plan stepped one by one) with
``torch.func.jvp`` through ``LeapfrogRef.run``, one call per tangent.

The cases are the first ten raw cases of the pull file -- the same networks, gains, step counts, K and batch sizes -- run on
the FORWARD rows, ``plan_leapfrog(linspace(1, 0, steps + 1))`` or the hand plan A, A, B, B, A, plus one "maps" case that
exercises the four affine vectors of the raw launch (tangents ``/ in_scale`` on the way in, ``* out_scale`` on the way out, no
shift).  Inputs are seeded (4321): ``z``, ``tangents [B, K, 2D]``, ``cond``, ``cond_tangents [B, K, C]``.

Error measure and bar are the derivative families': ``normalised_error`` of tests/_pushforward_ref.py; the floor of a case is
the fp32 CPU run's error against float64; the device is held to ``FACTOR = 22`` floors.  The pull file's ``DEEP_CASES`` are not
reused: at one forward step their mid-layer swaps miss the bar by 0-3 x, and the push units have no LDS depth ceiling to pin.
"""
from __future__ import annotations

import torch

from flowfusion_amd import solvers
from tests import _leapfrog_pull_ref as P
from tests._leapfrog_pull_ref import Damage, LeapfrogRef, case_id, hand_plan, make_model, plan_rows      # noqa: F401
from tests._pushforward_ref import normalised_error

FACTOR = 22.0
ULP = 2.0 ** -23
SEED = 4321

# (D, C, units, gain, steps, K, B[, "maps"]): steps = leapfrog steps of the FORWARD grid linspace(1, 0, steps + 1), or "hand"
RAW_CASES = [tuple(c[:7]) for c in P.RAW_CASES[:10]] + [(4, 1, [128, 128], 2.0, 2, 2, 6, "maps")]
UNIT_OF = {i: P.UNIT_OF[i].replace("mlp_pullsel_", "mlp_pushsel_") + ("_w3" if "_h128_" in P.UNIT_OF[i] else "_w2")
           for i in range(len(RAW_CASES))}


def fp32_floor(r32, r64):
    """The fp32 floor: the fp32 reference's normalised error against float64, as measured (an exact zero, the luck of a tiny
    case, is replaced by one ulp of fp32: tests/test_gpu_pushforward.py ``fp32_floor``)."""
    f = normalised_error(r32, r64)
    return f if f > 0.0 else ULP


def case_plan(case):
    steps = case[4]
    if steps == "hand":
        return hand_plan()
    return solvers.plan_leapfrog(torch.linspace(1.0, 0.0, int(steps) + 1))


def case_maps(case):
    """The affine maps of the raw launch of a case (none, or the four vectors over the joint state)."""
    if len(case) <= 7:
        return {}
    D2 = 2 * case[0]
    return dict(in_shift=torch.linspace(-0.3, 0.3, D2), in_scale=torch.linspace(0.8, 1.25, D2),
                out_scale=torch.linspace(0.9, 1.6, D2), out_shift=torch.linspace(0.2, -0.2, D2))


_SETUPS = {}


def case_setup(case):
    """(front, plan, rows, z, tangents, cond, cond_tangents) of a case, computed once: seeded inputs, the model on the CPU."""
    key = case_id(case)
    if key not in _SETUPS:
        D, C, units, gain, steps, K, B = case[:7]
        front = make_model(D, C, units, gain)
        g = torch.Generator().manual_seed(SEED)
        z = torch.randn(B, 2 * D, generator=g)
        v = torch.randn(B, K, 2 * D, generator=g)
        cond = torch.randn(B, C, generator=g) if C else None
        vc = torch.randn(B, K, C, generator=g) if C else None
        plan = case_plan(case)
        _SETUPS[key] = (front, plan, plan_rows(plan), z, v, cond, vc)
    return _SETUPS[key]


def jvp_rows(ref: LeapfrogRef, z, cond, rows, v, vc):
    """(z_out [B, 2D], dz [B, K, 2D]) of ``ref.run`` over ``rows`` at (z, cond) along the K tangents (v[:, k], vc[:, k]), by
    ``torch.func.jvp``, one call per tangent; ``v`` / ``vc`` None = zero."""
    z, cond = ref.cast(z), ref.cast(cond)
    given = v if v is not None else vc
    K = int(given.shape[1])
    out, cols = None, []
    for k in range(K):
        vk = torch.zeros_like(z) if v is None else ref.cast(v[:, k])
        if cond is None:
            out, d = torch.func.jvp(lambda zz: ref.run(zz, None, rows), (z,), (vk,))
        else:
            ck = torch.zeros_like(cond) if vc is None else ref.cast(vc[:, k])
            out, d = torch.func.jvp(lambda zz, cc: ref.run(zz, cc, rows), (z, cond), (vk, ck))
        cols.append(d)
    return out.detach(), torch.stack(cols, dim=1).detach()


def raw_reference(case, dtype=torch.float64, damage=Damage()):
    """(z_out, dz) of a raw case as the launch defines them, maps included: the launch integrates ``y = (z - in_shift) /
    in_scale`` with tangents ``v / in_scale`` and returns ``y_out * out_scale + out_shift`` and ``dy * out_scale``."""
    front, plan, rows, z, v, cond, vc = case_setup(case)
    ref = LeapfrogRef(front, dtype, damage)
    m = {k: t.to(dtype) for k, t in case_maps(case).items()}
    zz, vv = z.to(dtype), v.to(dtype)
    if m:
        zz, vv = (zz - m["in_shift"]) / m["in_scale"], vv / m["in_scale"]
    zo, dz = jvp_rows(ref, zz, cond, rows, vv, vc)
    if m:
        zo, dz = zo * m["out_scale"] + m["out_shift"], dz * m["out_scale"]
    return zo, dz


_REFS = {}


def raw_floor_and_reference(case):
    """(floor of dz, floor of z_out, (z_out, dz) in float64) of a case, computed once and shared."""
    key = case_id(case)
    if key not in _REFS:
        r64 = raw_reference(case, torch.float64)
        r32 = raw_reference(case, torch.float32)
        _REFS[key] = (fp32_floor(r32[1], r64[1]), fp32_floor(r32[0], r64[0]), r64)
    return _REFS[key]


def jacobian_rows(ref: LeapfrogRef, z, cond, rows):
    """d run / d z [B, 2D, 2D] in the reference's dtype: column j from the unit tangent e_j."""
    z = ref.cast(z)
    D2 = int(z.shape[1])
    eye = torch.eye(D2, dtype=ref.dtype)[None].expand(z.shape[0], D2, D2)
    return jvp_rows(ref, z, cond, rows, eye, None)[1].transpose(1, 2)


# ---- the front ends ---------------------------------------------------------------------------------------------------------
# (D, C, units, gain, num_steps, B, affine): one per unit; the first is served by the 32-column row-select kernel (64 wide)
SAMPLE_CASES = [
    (4, 3, [64, 64], 2.0, 2, 9, True),
    (9, 0, [128], 1.0, 1, 5, False),
    (5, 1, [256, 256], 1.5, 3, 6, False),
]
front_id = P.front_id


def front_inputs(case, K=3):
    """(front, z [B, 2D], tangents [B, K, 2D], raw conditional or None, conditional tangents [B, K, C] or None, cotangents
    [B, K, D]), seeded."""
    D, C, units, gain, steps, B, affine = case
    front = make_model(D, C, units, gain, affine=affine)
    g = torch.Generator().manual_seed(SEED)
    z = torch.randn(B, 2 * D, generator=g)
    v = torch.randn(B, K, 2 * D, generator=g)
    cond = torch.randn(B, C, generator=g) if C else None
    vc = torch.randn(B, K, C, generator=g) if C else None
    w = torch.randn(B, K, D, generator=g)
    return front, z, v, cond, vc, w


def sample_jvp_ref(front, z, v, cond, vc, num_steps, dtype=torch.float64):
    """(x [B, D], dx [B, K, D]) of ``sample_leapfrog_jvp`` by ``torch.func.jvp`` of the whole method (``sample_map`` of the
    pull file: raw conditional in, ``q * scale + shift`` out); ``v`` / ``vc`` None = zero."""
    f = P.sample_map(front, dtype)
    cast = lambda t: None if t is None else t.detach().to("cpu", dtype)
    z, cond = cast(z), cast(cond)
    K = int((v if v is not None else vc).shape[1])
    x, cols = None, []
    for k in range(K):
        vk = torch.zeros_like(z) if v is None else cast(v[:, k])
        if cond is None:
            x, d = torch.func.jvp(lambda zz: f(zz, None, num_steps), (z,), (vk,))
        else:
            ck = torch.zeros_like(cond) if vc is None else cast(vc[:, k])
            x, d = torch.func.jvp(lambda zz, cc: f(zz, cc, num_steps), (z, cond), (vk, ck))
        cols.append(d)
    return x.detach(), torch.stack(cols, dim=1).detach()


def sample_jacobian_ref(front, z, cond, num_steps, dtype=torch.float64):
    """(x, J_z [B, D, 2D], J_c [B, D, C] or None) of ``sample_leapfrog_jacobian``: unit tangents through ``sample_jvp_ref``."""
    B, D2 = z.shape
    C = 0 if cond is None else int(cond.shape[1])
    eye = torch.eye(D2 + C)[None].expand(B, D2 + C, D2 + C)
    x, d = sample_jvp_ref(front, z, eye[:, :, :D2], cond, eye[:, :, D2:] if C else None, num_steps, dtype)
    J = d.transpose(1, 2)
    return x, J[:, :, :D2], (J[:, :, D2:] if C else None)


def adjoint_gap(w, dx, gz, v, gc=None, vc=None):
    """The adjoint identity of a push-forward against a pull-back of the same map, per (sample, k) and then the worst:
    ``|<w, dx> - <gz, v> - <gc, vc>|`` over the sum of the absolute terms, in float64."""
    d = lambda t: t.detach().to("cpu", torch.float64)
    a, b = d(w) * d(dx), d(gz) * d(v)
    num = a.sum(-1) - b.sum(-1)
    den = a.abs().sum(-1) + b.abs().sum(-1)
    if gc is not None:
        c = d(gc) * d(vc)
        num, den = num - c.sum(-1), den + c.abs().sum(-1)
    return float((num.abs() / den).max())


_ADJ = {}


def adjoint_floor(case):
    """The floor of ``adjoint_gap`` of a front-end case: the same quantity from the fp32 CPU restatement of both legs (jvp and
    autograd of the whole method), an exact zero replaced by one ulp; computed once."""
    key = front_id(case)
    if key not in _ADJ:
        front, z, v, cond, vc, w = front_inputs(case)
        n = case[4]
        _, dx = sample_jvp_ref(front, z, v, cond, vc, n, torch.float32)
        _, gz, gc = P.sample_vjp_ref(front, z, w, cond, n, torch.float32)
        gap = adjoint_gap(w, dx, gz, v, gc, vc)
        _ADJ[key] = gap if gap > 0.0 else ULP
    return _ADJ[key]
