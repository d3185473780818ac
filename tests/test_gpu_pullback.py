"""GPU tier of the flow-map pull-backs (csrc/ff_mlp_pull.hpp, ff_mlp_ode_launch_pull, ``flow_vjp``): raw launches of the three
pull-back units between guard words on NaN-prefilled outputs against the float64 reference (tests/_pullback_ref.py: the same
continuous adjoint through the oracle's fixed-grid solver), the bitwise properties (the state of the front end, the retraced
state's independence of the cotangents, zeros, columns, cuts, slices, re-runs, a noise row), the adjoint identity against
``flow_jvp`` and the population wrappers' chain rule.

Tolerance: the push-forward tests' rule and factor (tests/test_gpu_pushforward.py).  Per case the reference runs twice on
the CPU, in fp32 and in float64; the fp32 run's error per sample, normalised by the sample's largest reference entry, is the
case's fp32 floor, as measured, and the bar is that floor times FACTOR = 22.  profiles/pullback.txt lists the floors and the
device's errors.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from flowfusion_amd import diffusion as Dm
from tests import _pullback_ref as P
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import (FACTOR, GUARD, W128, W256, _guarded, _payload, affine_of, fp32_floor, make_front, options_of,
                                        span_of)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def inputs(B, D, C, K, seed=29):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * D + K)
    x = torch.randn(B, D, generator=g)
    w = torch.randn(B, K, D, generator=g)
    c = torch.randn(B, C, generator=g) if C else None
    return x, w, c


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


def forward_state(front, x_in, t_span, method, opts, cond, maps):
    """The ordinary state-only solve on the device: what a pull launch starts from."""
    y, _ = odeint.solve(front, _dev(x_in), t_span, method, opts, _native.MODE_STATE, 0.0, 0.0, cond=_dev(cond), **maps)
    return y


def raw_pull(front, y, t_span, method, options, cotangents, cond=None, maps=None, want_cond=True, noise_row=None, status_is=0,
             slots=None):
    """ff_mlp_ode_launch_pull on buffers of the test's own, over the REVERSED span of the solve that gave ``y``, with the
    forward solve's ``maps`` turned round: (retraced state [B, D], cot_x [B, K, D], cot_cond [B, K, C] or None), guards
    checked.  ``noise_row``: that row of the table gets the FF_ROW_NOISE flag; ``status_is``: what the status word must read;
    ``slots``: the stage slots kept in LDS (default: the method's stages)."""
    net = front.to(DEV)._net()
    plan = net.pull_plan()
    tab = solvers.plan_ode(torch.flip(t_span, dims=(0,)), method, options)
    table = solvers.build_table(tab, *front._host_schedule()(tab.t_eval), int(plan.width))
    if noise_row is not None:
        table.view(torch.int32)[noise_row, solvers.ROW_FLAGS] |= solvers.FLAG_NOISE
    table = table.to(DEV)
    wp = net.wpack(torch.device(DEV), _native.MODE_HUTCH, plan)
    y, w, cond = _dev(y), _dev(cotangents), _dev(cond)
    turned = {"in_shift": "out_shift", "in_scale": "out_scale", "out_scale": "in_scale", "out_shift": "in_shift"}
    keep = {turned[k]: _dev(v) for k, v in (maps or {}).items()}
    B, D = y.shape
    K, C = w.shape[1], (0 if cond is None else cond.shape[1])
    xo, gx = _guarded(B * D), _guarded(B * K * D)
    gc = _guarded(B * K * C) if (C and want_cond) else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab, a.status = y.data_ptr(), xo.data_ptr() + 4 * GUARD, wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if cond is None else cond.data_ptr()
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    a.batch, a.n_evals, a.tangent_count, a.mode = B, table.shape[0], K, _native.MODE_HUTCH
    a.stage_slots = solvers.resolve_method(method).stages if slots is None else slots
    rc = _native.lib().ff_mlp_ode_launch_pull(ctypes.byref(plan), ctypes.byref(a), w.data_ptr(), gx.data_ptr() + 4 * GUARD,
                                              0 if gc is None else gc.data_ptr() + 4 * GUARD,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    return (_payload(xo, (B, D)), _payload(gx, (B, K, D)), None if gc is None else _payload(gc, (B, K, C)),
            _native.kernel_name(plan))


# (unit's kernel, model, D, C, K, B, hidden layers, method, steps, direction, affine); B = 1, samples per tile + 1, 37
RAW_CASES = [
    ("h128_d4", "vp", 1, 0, 1, 1, 1, "euler", 1, "to_data", False),
    ("h128_d4", "ve", 4, 1, 2, 16 // 3 + 1, 2, "rk4", 2, "to_base", True),
    ("h128_d4", "subvp", 16, 16, 15, 37, 1, "dopri5_fixed", 5, "to_data", True),
    ("h128_d4", "flow", 5, 0, 7, 16 // 8 + 1, 4, "rk4", 5, "to_base", False),
    ("h128_d4", "flow", 16, 1, 1, 37, 2, "dopri5_fixed", 2, "to_data", True),
    ("h256_d4", "vp", 1, 16, 15, 16 // 16 + 1, 4, "dopri5_fixed", 1, "to_base", False),
    ("h256_d4", "ve", 16, 0, 2, 37, 1, "euler", 5, "to_data", True),
    ("h256_d4", "subvp", 4, 1, 1, 16 // 2 + 1, 4, "rk4", 2, "to_base", True),
    ("h256_d4", "flow", 16, 16, 7, 16 // 8 + 1, 2, "rk4", 1, "to_data", False),
    ("h256_d4", "vp", 5, 0, 15, 37, 4, "rk4", 5, "to_base", False),
    ("h256_d8", "vp", 17, 0, 1, 1, 1, "rk4", 1, "to_data", False),
    ("h256_d8", "ve", 32, 16, 15, 37, 4, "dopri5_fixed", 2, "to_base", True),
    ("h256_d8", "subvp", 17, 1, 2, 16 // 3 + 1, 2, "euler", 5, "to_data", True),
    ("h256_d8", "flow", 32, 0, 7, 16 // 8 + 1, 1, "rk4", 2, "to_base", True),
    ("h256_d8", "flow", 17, 16, 1, 37, 4, "dopri5_fixed", 5, "to_data", False),
]


def case_setup(case):
    """The front end, the inputs, what the launches take (the start of the forward solve, the network's conditional, the
    forward solve's maps) and the reference in fp32 / float64, which works in the user's units."""
    unit, kind, D, C, K, B, nh, method, nsteps, direction, affine = case
    width = W128 if unit.startswith("h128") else W256
    front, ref_kw = make_front(kind, D, C, width, nh, affine=affine)
    x, w, c = inputs(B, D, C, K)
    opts = options_of(front, direction, nsteps)
    maps, ref_aff = {}, {}
    if affine:
        shift, scale = affine_of(D)
        maps = dict(out_scale=scale, out_shift=shift) if direction == "to_data" else dict(in_shift=shift, in_scale=scale)
        if kind != "flow":
            ref_aff = dict(affine=(shift, scale))
    refs = {dt: P.Pullback(R.SolverMap(direction=direction, method=method, options=opts, dtype=dt, **ref_kw, **ref_aff))
            for dt in (torch.float32, torch.float64)}
    # a score model's to_data solve starts from x * sigma_max: the chain rule's factor on cot_x, and on the retraced state
    gain = float(front.sde.sigma_max) if (kind != "flow" and direction == "to_data" and hasattr(front.sde, "sigma_max")) else 1.0
    # a flow's network sees the normalised conditional: the chain rule's factor on cot_cond
    c_net, c_scale = c, None
    if kind == "flow" and C:
        c_net, c_scale = front._norm_cond(c), front.conditional_scale.detach().cpu()
    return front, refs, (x, w, c), (x * gain, c_net, gain, c_scale), span_of(front, direction), method, opts, maps


def _id(case):
    return "-".join(str(p) for p in case)


def run_case(case, cotangents=None, **kw):
    """(retraced state, cot_x, cot_cond) of a raw case in the USER's units, its forward state, the kernel's name."""
    front, refs, (x, w, c), (x_in, c_net, gain, c_scale), t_span, method, opts, maps = case_setup(case)
    w = w if cotangents is None else cotangents
    y = forward_state(front, x_in, t_span, method, opts, c_net, maps)
    xb, gx, gc, name = raw_pull(front, y, t_span, method, opts, w, cond=c_net, maps=maps, **kw)
    xb, gx, gc = xb.cpu() / gain, gx.cpu() * gain, (None if gc is None else gc.cpu())
    if gc is not None and c_scale is not None:
        gc = gc / c_scale
    return (xb, gx, gc), y, name


@pytest.mark.parametrize("case", RAW_CASES, ids=_id)
def test_raw_launch_against_float64_reference(case):
    _, refs, (x, w, c), *_ = case_setup(case)
    (xb, gx, gc), y, name = run_case(case)
    assert f"mlp_pull_m16_{case[0]}_c4" == name, name             # the unit the case is meant for
    r64, r32 = refs[torch.float64], refs[torch.float32]
    y64, gx64, gc64, _ = r64(x, w, c)
    y32, gx32, gc32, _ = r32(x, w, c)
    line = f"\n[pullback] {_id(case)}:"
    checks = [("x_out", y, y64, y32), ("retraced", xb, r64.retraced, r32.retraced), ("cot_x", gx, gx64, gx32)]
    if c is not None:
        checks.append(("cot_cond", gc, gc64, gc32))
    worst = []
    for what, got, ref64, ref32 in checks:
        floor, err = fp32_floor(ref32, ref64), R.normalised_error(got, ref64)
        line += f" {what} err {err:.3e} floor {floor:.3e};"
        worst.append((what, err, floor))
    print(line)
    for what, err, floor in worst:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


# ---- bitwise properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (1, 8, 11, 12)], ids=_id)
def test_retraced_state_ignores_the_cotangents_and_zero_cotangents_give_zeros(case):
    _, _, (x, w, c), *_ = case_setup(case)
    (xb, gx, gc), _, _ = run_case(case)
    (xb2, gx2, gc2), _, _ = run_case(case, cotangents=3.0 * w + 1.0)
    assert torch.equal(xb, xb2) and not torch.equal(gx, gx2)
    (xb0, gx0, gc0), _, _ = run_case(case, cotangents=torch.zeros_like(w))
    assert torch.equal(xb0, xb) and bool((gx0 == 0).all()) and (gc0 is None or bool((gc0 == 0).all()))
    # without the conditional output the rest is the same, bit for bit
    (xbn, gxn, gcn), _, _ = run_case(case, want_cond=False)
    assert gcn is None and torch.equal(xbn, xb) and torch.equal(gxn, gx)


@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (2, 3, 9, 11)], ids=_id)
def test_column_k_of_a_k_launch_is_the_single_launch_of_that_cotangent(case):
    _, _, (x, w, c), *_ = case_setup(case)
    (xb, gx, gc), _, _ = run_case(case)
    for k in (0, w.shape[1] - 1):
        (xb1, gx1, gc1), _, _ = run_case(case, cotangents=w[:, k:k + 1])
        assert torch.equal(xb1, xb) and torch.equal(gx1[:, 0], gx[:, k])
        assert gc is None or torch.equal(gc1[:, 0], gc[:, k])


def test_a_noise_row_is_left_out_and_reported_in_the_status_word():
    case = RAW_CASES[1]
    (xb, gx, gc), _, _ = run_case(case)
    for row in (0, 7):                                       # a stage row and a step-end row (rk4, two steps: rows 0 .. 7)
        (xn, gn, cn), _, _ = run_case(case, noise_row=row, status_is=_native.STATUS_NOISE_ROW)
        assert torch.equal(xn, xb) and torch.equal(gn, gx) and torch.equal(cn, gc)


# ---- the front ends -----------------------------------------------------------------------------------------------------------------
def test_front_end_state_is_bitwise_the_state_only_solve_and_matches_the_raw_launch():
    D, C, B, K = 5, 3, 21, 3
    front, ref_kw = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, w, c = (t.to(DEV) for t in inputs(B, D, C, K))
    for direction in ("to_data", "to_base"):
        kw = dict(direction=direction, method="rk4", options={"step_size": 0.25})
        y, gx, gc, retrace = front.flow_vjp(x, w, c, return_retrace=True, **kw)
        assert y.shape == (B, D) and gx.shape == (B, K, D) and gc.shape == (B, K, C) and retrace.shape == (B,)
        if direction == "to_data":
            assert torch.equal(y, front.sample(x, c, method="rk4", options=kw["options"]))
        else:
            solo, _ = odeint.solve(front, x, span_of(front, direction), "rk4", kw["options"], _native.MODE_STATE, 0.0, 0.0,
                                   cond=front._norm_cond(c), in_shift=front.target_shift, in_scale=front.target_scale)
            assert torch.equal(y, solo)
        three = front.flow_vjp(x, w, c, **kw)
        assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, (y, gx, gc)))
        refs = {dt: P.Pullback(R.SolverMap(direction=direction, method="rk4", options=kw["options"], dtype=dt, **ref_kw))
                for dt in (torch.float32, torch.float64)}
        (y64, gx64, gc64, rt64), (y32, gx32, gc32, rt32) = (refs[dt](x, w, c) for dt in (torch.float64, torch.float32))
        for got, r64, r32 in ((y, y64, y32), (gx, gx64, gx32), (gc, gc64, gc32)):
            assert R.normalised_error(got, r64) <= FACTOR * fp32_floor(r32, r64)
        # retrace = max_d |y_back - x|: a difference of two nearby fp32 states, so its error is that of the retraced state
        back64, back32 = refs[torch.float64].retraced, refs[torch.float32].retraced
        slack = FACTOR * fp32_floor(back32, back64) * float(back64.abs().max())
        assert bool(((retrace.cpu().double() - rt64).abs() <= slack).all())


def test_row_cuts_slices_and_reruns_are_bitwise(monkeypatch):
    D, C, B, K = 4, 1, 37, 7
    front, _ = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, w, c = (t.to(DEV) for t in inputs(B, D, C, K))
    kw = dict(direction="to_base", method="dopri5_fixed", options={"step_size": 0.5}, return_retrace=True)
    whole = front.flow_vjp(x, w, c, **kw)
    again = front.flow_vjp(x, w, c, **kw)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    part = front.flow_vjp(x[5:20], w[5:20], c[5:20], **kw)
    assert all(torch.equal(a, b[5:20]) for a, b in zip(part, whole))
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 5 * K * D + 1)       # five rows per launch: eight pieces
    cut = front.flow_vjp(x, w, c, **kw)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(whole, cut))


def test_adjoint_identity_against_the_pushed_tangents():
    """<w, flow_jvp(v, vc)> = <flow_vjp(w), (v, vc)> on a flow with rk4, where the discretisation gap between the discrete
    derivative (jvp) and the continuous adjoint (vjp) -- 1e-10 at 16 steps -- sits far under fp32 rounding.  Bar: every entry
    of dx is off by at most FACTOR x its fp32 floor x the sample's largest |dx|, every entry of (gx, gc) likewise, so the two
    inner products differ by at most  FACTOR (floor_push max|dx| sum|w| + floor_pull max|g| sum|(v, vc)|)  plus the float64
    references' own gap."""
    D, C, B, K = 4, 2, 11, 3
    front, ref_kw = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, w, c = inputs(B, D, C, K)
    g = torch.Generator().manual_seed(77)
    v, vc = torch.randn(B, K, D, generator=g), torch.randn(B, K, C, generator=g)
    for direction in ("to_data", "to_base"):
        kw = dict(direction=direction, method="rk4", options={"step_size": 1.0 / 16})
        _, dx = front.flow_jvp(_dev(x), _dev(v), _dev(c), _dev(vc), **kw)
        _, gx, gc = front.flow_vjp(_dev(x), _dev(w), _dev(c), **kw)
        maps = {dt: R.SolverMap(direction=direction, method="rk4", options=kw["options"], dtype=dt, **ref_kw)
                for dt in (torch.float32, torch.float64)}
        dx64, dx32 = (maps[dt].jvp(x, v, c, vc)[1] for dt in (torch.float64, torch.float32))
        (_, gx64, gc64, _), (_, gx32, gc32, _) = (P.Pullback(maps[dt])(x, w, c) for dt in (torch.float64, torch.float32))
        g64, g32 = torch.cat([gx64, gc64], dim=2), torch.cat([gx32, gc32], dim=2)
        floor_push, floor_pull = fp32_floor(dx32, dx64), fp32_floor(g32, g64)
        u = torch.cat([v, vc], dim=2).double()
        lhs = (w.double() * dx.cpu().double()).sum(dim=2)
        rhs = (torch.cat([gx, gc], dim=2).cpu().double() * u).sum(dim=2)
        gap64 = ((w.double() * dx64).sum(dim=2) - (g64 * u).sum(dim=2)).abs()
        bound = FACTOR * (floor_push * dx64.abs().reshape(B, -1).amax(dim=1)[:, None] * w.double().abs().sum(dim=2)
                          + floor_pull * g64.abs().reshape(B, -1).amax(dim=1)[:, None] * u.abs().sum(dim=2)) + gap64
        print(f"\n[pullback] adjoint identity {direction}: |lhs - rhs| {float((lhs - rhs).abs().max()):.3e}, float64 gap "
              f"{float(gap64.max()):.3e}, smallest bound {float(bound.min()):.3e}, floors {floor_push:.3e} {floor_pull:.3e}")
        assert bool(((lhs - rhs).abs() <= bound).all()), ((lhs - rhs).abs(), bound)


@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_population_wrappers_apply_the_chain_rule(direction):
    torch.manual_seed(21)
    D, C, B, K = 5, 3, 9, 4
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=[100, 100])
    shift, scale = torch.linspace(-0.5, 0.5, D), torch.linspace(0.5, 1.5, D)
    cshift, cscale = torch.linspace(0.2, -0.2, C), torch.linspace(0.7, 1.9, C)
    pm = Dm.PopulationModelDiffusionConditional(model=m, sde=Dm.VPSDE(), shift=shift, scale=scale, conditional_shift=cshift,
                                                conditional_scale=cscale, method="rk4").to(DEV).eval()
    x, w, c = inputs(B, D, C, K)
    opts = options_of(pm.score_model, direction, 2)
    kw = dict(direction=direction, method="rk4", options=opts)
    refs = {dt: P.Pullback(R.SolverMap("score", R.score_params(m), direction, "rk4", opts, dtype=dt, sde="vp",
                                       affine=(shift, scale), cond_affine=(cshift, cscale)))
            for dt in (torch.float32, torch.float64)}
    y, gx, gc, retrace = pm.flow_vjp(_dev(x), _dev(w), _dev(c), return_retrace=True, **kw)
    (y64, gx64, gc64, _), (y32, gx32, gc32, _) = (refs[dt](x, w, c) for dt in (torch.float64, torch.float32))
    for got, r64, r32 in ((y, y64, y32), (gx, gx64, gx32), (gc, gc64, gc32)):
        assert R.normalised_error(got, r64) <= FACTOR * fp32_floor(r32, r64)
    # the unconditional wrapper, on a VE model: to_data starts from x * sigma_max, and gx carries the factor
    torch.manual_seed(22)
    mu = Dm.MLP(n_dimensions=D, n_conditionals=0, embedding_dimensions=8, units=[64, 64])
    pu = Dm.PopulationModelDiffusion(model=mu, sde=Dm.VESDE(), shift=shift, scale=scale, method="rk4").to(DEV).eval()
    optu = options_of(pu.score_model, direction, 2)
    refu = {dt: P.Pullback(R.SolverMap("score", R.score_params(mu), direction, "rk4", optu, dtype=dt, sde="ve",
                                       affine=(shift, scale))) for dt in (torch.float32, torch.float64)}
    yu, gu, none, rtu = pu.flow_vjp(_dev(x), _dev(w), direction=direction, method="rk4", options=optu, return_retrace=True)
    (yu64, gu64, _, rt64), (yu32, gu32, _, _) = (refu[dt](x, w) for dt in (torch.float64, torch.float32))
    assert none is None
    assert R.normalised_error(yu, yu64) <= FACTOR * fp32_floor(yu32, yu64)
    assert R.normalised_error(gu, gu64) <= FACTOR * fp32_floor(gu32, gu64)
    back64, back32 = refu[torch.float64].retraced, refu[torch.float32].retraced
    slack = FACTOR * fp32_floor(back32, back64) * float(back64.abs().max())
    assert bool(((rtu.cpu().double() - rt64).abs() <= slack).all())
