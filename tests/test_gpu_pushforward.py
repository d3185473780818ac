"""GPU tier of the flow-map sensitivities (csrc/ff_mlp_ode.hpp PUSH, ff_mlp_ode_launch_push, ``flow_jvp`` /
``flow_jacobian``): raw launches of the three push-forward units between guard words against the float64 reference
(tests/_pushforward_ref.py), the state against a K-probe Hutchinson launch bit for bit, linearity, unit tangents against
one-hot buffers, the front ends (Jacobian times vector, row cuts, slices, re-runs, the population wrappers' chain rule)
and the to_base / to_data round trip.

Tolerance.  Nothing is fixed in advance but one factor.  Per case the test runs the reference twice on the CPU, in fp32 and
in float64, and takes the fp32 run's error per sample, normalised by the sample's max |reference tangent|: the fp32 floor,
as measured (``fp32_floor``: only a floor of exactly zero -- the fp32 run hit the rounded float64 values bit for bit, which
says nothing about another fp32 run -- is replaced, by one fp32 ulp).  The bar
is that floor times FACTOR, the factor by which the parity tests' state bar (tests/test_gpu_parity.py STATE_TOL = 2e-5)
exceeds the same floor measured for the STATE on these shapes.  The floors of RAW_CASES span four decades (3e-8 .. 2e-4:
one rk4 step over the whole VP span amplifies rounding by hundreds, and there the fp32 reference itself misses 2e-5), so
the factor is taken where the parity bar is at home: the case of RAW_CASES with the parity tests' own model (their config
c2: 16-d VP, 4 x 256, rk4; here 5 steps, B = 37).  Its fp32 state floor is 8.82e-7 (profiles/pushforward.txt lists all
fifteen), so FACTOR = 2e-5 / 8.82e-7 = 22.7, rounded down to 22.  The state of a raw case is held to the same rule, its own
floor times FACTOR.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from flowfusion_amd import diffusion as Dm
from flowfusion_amd import flow as Fm
from tests import _pushforward_ref as R
from tests._deep_models import apply_gain

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23
FACTOR = 22.0
GUARD = 64
MAGIC = 12345.6789
SDE = {"vp": "VPSDE", "ve": "VESDE", "subvp": "SUBVPSDE"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


# ---- models and their references ---------------------------------------------------------------------------------------------
def make_front(kind, D, C, width, nh, seed=5, affine=False, gain=1.0):
    """(front end on the CPU, SolverMap keywords) of a seeded model: kind in vp / ve / subvp (ScoreModel) or flow.  ``width``: one
    width for all ``nh`` hidden layers, or the sequence of their widths.  ``gain`` multiplies the hidden-to-hidden weight
    matrices in place before the reference reads the parameters (tests/_deep_models.py: at default init a deep stack's
    Jacobian vanishes); 1.0 leaves the seeded model as it is, bit for bit."""
    torch.manual_seed(seed)
    units = [width] * nh if isinstance(width, int) else list(width)
    if kind == "flow":
        kw = {}
        if affine:
            kw = dict(target_shift=torch.linspace(-1.0, 1.0, D), target_scale=torch.linspace(0.5, 2.0, D))
        f = Fm.ODEFlow(D, units, **kw) if C == 0 else Fm.ConditionalODEFlow(D, C, units, **kw)
        apply_gain(f._linears(), gain)
        return f.eval(), dict(kind="flow", params=R.flow_params(f))
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=units)
    apply_gain(list(m.NN), gain)
    sm = Dm.ScoreModel(m, getattr(Dm, SDE[kind])(), no_sigma=False).eval()
    return sm, dict(kind="score", params=R.score_params(m), sde=kind)


def fp32_floor(r32, r64):
    """The fp32 floor of a case: the fp32 reference's normalised error against float64, as measured.  Exactly zero means the
    fp32 run reproduced the rounded float64 result, by luck of a tiny case; a bar of zero would then ask any other order of
    the same fp32 operations for the same luck, so that one value is replaced by one ulp of fp32."""
    f = R.normalised_error(r32, r64)
    return f if f > 0.0 else ULP


def affine_of(D):
    return torch.linspace(-1.0, 1.0, D), torch.linspace(0.5, 2.0, D)


def span_of(front, direction):
    if isinstance(front, Dm.ScoreModel):
        eps = float(front.sde.epsilon)
        return torch.tensor([1.0, eps] if direction == "to_data" else [eps, 1.0], dtype=torch.float32)
    return torch.tensor([1.0, 0.0] if direction == "to_data" else [0.0, 1.0], dtype=torch.float32)


def options_of(front, direction, nsteps):
    t = span_of(front, direction)
    return {"step_size": float(abs(t[1] - t[0])) / nsteps}


def inputs(B, D, C, K, seed=17):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * D + K)
    x = torch.randn(B, D, generator=g)
    v = torch.randn(B, K, D, generator=g)
    c = torch.randn(B, C, generator=g) if C else None
    vc = torch.randn(B, K, C, generator=g) if C else None
    return x, v, c, vc


# ---- the raw launch, between guard words -------------------------------------------------------------------------------------
def _guarded(n):
    buf = torch.full((GUARD + n + GUARD,), MAGIC, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    return buf


def _payload(buf, shape):
    n = buf.numel() - 2 * GUARD
    assert bool((buf[:GUARD] == MAGIC).all()) and bool((buf[GUARD + n:] == MAGIC).all()), "a guard word was overwritten"
    out = buf[GUARD:GUARD + n].clone().view(*shape)
    assert not bool(torch.isnan(out).any()), "an output word was not written"
    return out


def raw_push(front, x, t_span, method, options, K, tangents=None, cond=None, cond_tangents=None, unit_first=None, maps=None,
             noise_row=None, status_is=0):
    """ff_mlp_ode_launch_push on buffers of the test's own: (x_out [B, D], tangent_out [B, K, D]), guards checked.
    ``noise_row``: that row of the table gets the FF_ROW_NOISE flag; ``status_is``: what the status word must read."""
    net = front.to(DEV)._net()
    plan = net.push_plan()
    tab = solvers.plan_ode(t_span, method, options)
    table = solvers.build_table(tab, *front._host_schedule()(tab.t_eval), int(plan.width))
    if noise_row is not None:
        table.view(torch.int32)[noise_row, solvers.ROW_FLAGS] |= solvers.FLAG_NOISE
    table = table.to(DEV)
    wp = net.wpack(torch.device(DEV), _native.MODE_HUTCH, plan)
    dev = lambda t: None if t is None else t.detach().to(DEV, torch.float32).contiguous()
    x, tangents, cond, cond_tangents = dev(x), dev(tangents), dev(cond), dev(cond_tangents)
    keep = {k: dev(v) for k, v in (maps or {}).items()}
    B, D = x.shape
    xo, to = _guarded(B * D), _guarded(B * K * D)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab, a.status = x.data_ptr(), xo.data_ptr() + 4 * GUARD, wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if cond is None else cond.data_ptr()
    a.probe = 0 if tangents is None else tangents.data_ptr()
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    a.batch, a.n_evals, a.tangent_count = B, table.shape[0], K
    a.mode = _native.MODE_HUTCH if unit_first is None else _native.MODE_EXACT
    a.tangent_first = 0 if unit_first is None else unit_first
    a.stage_slots = solvers.resolve_method(method).stages
    rc = _native.lib().ff_mlp_ode_launch_push(ctypes.byref(plan), ctypes.byref(a), 0 if cond_tangents is None else cond_tangents.data_ptr(),
                                              to.data_ptr() + 4 * GUARD, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    return _payload(xo, (B, D)), _payload(to, (B, K, D)), _native.kernel_name(plan)


# (unit's kernel, model, D, C, K, B, hidden layers, method, steps, direction, affine, conditional tangents given)
W128, W256 = 128, 256
RAW_CASES = [
    ("h128_d4", "vp", 1, 0, 1, 1, 1, "euler", 1, "to_data", False, False),
    ("h128_d4", "ve", 3, 1, 2, 16 // 3 + 1, 4, "rk4", 2, "to_base", True, True),
    ("h128_d4", "subvp", 16, 16, 15, 37, 1, "dopri5_fixed", 5, "to_data", True, False),
    ("h128_d4", "flow", 3, 0, 7, 16 // 8 + 1, 4, "rk4", 5, "to_base", False, False),
    ("h128_d4", "flow", 16, 1, 7, 37, 1, "dopri5_fixed", 2, "to_data", True, True),
    ("h256_d4", "vp", 1, 16, 15, 16 // 16 + 1, 4, "dopri5_fixed", 1, "to_base", False, True),
    ("h256_d4", "ve", 16, 0, 2, 37, 1, "euler", 5, "to_data", True, False),
    ("h256_d4", "subvp", 3, 1, 1, 1, 4, "rk4", 2, "to_base", True, False),
    ("h256_d4", "flow", 16, 16, 7, 16 // 8 + 1, 4, "rk4", 1, "to_data", False, True),
    ("h256_d4", "vp", 16, 0, 15, 37, 4, "rk4", 5, "to_base", False, False),
    ("h256_d8", "vp", 17, 0, 1, 1, 1, "rk4", 1, "to_data", False, False),
    ("h256_d8", "ve", 32, 16, 15, 37, 4, "dopri5_fixed", 2, "to_base", True, True),
    ("h256_d8", "subvp", 17, 1, 2, 16 // 3 + 1, 4, "euler", 5, "to_data", True, False),
    ("h256_d8", "flow", 32, 0, 7, 16 // 8 + 1, 1, "rk4", 2, "to_base", True, False),
    ("h256_d8", "flow", 17, 16, 7, 37, 4, "dopri5_fixed", 5, "to_data", False, True),
]


def case_setup(case):
    """Everything a raw case needs: the front end, the launch's inputs and maps, and the reference maps in fp32 / float64."""
    unit, kind, D, C, K, B, nh, method, nsteps, direction, affine, ct = case
    width = W128 if unit.startswith("h128") else W256
    front, ref_kw = make_front(kind, D, C, width, nh, affine=affine)
    x, v, c, vc = inputs(B, D, C, K)
    if not ct:
        vc = None
    opts = options_of(front, direction, nsteps)
    maps, ref_aff = {}, {}
    if affine:
        shift, scale = affine_of(D)
        maps = dict(out_scale=scale, out_shift=shift) if direction == "to_data" else dict(in_shift=shift, in_scale=scale)
        if kind != "flow":
            ref_aff = dict(affine=(shift, scale))
    refs = {dt: R.SolverMap(direction=direction, method=method, options=opts, dtype=dt, **ref_kw, **ref_aff)
            for dt in (torch.float32, torch.float64)}
    # the start of the launch: a score model's to_data solve starts from x * sigma_max, and so do its tangents
    gain = float(front.sde.sigma_max) if (kind != "flow" and direction == "to_data" and hasattr(front.sde, "sigma_max")) else None
    x_in, v_in = (x, v) if gain is None else (x * front.sde.sigma_max, v * gain)
    return front, refs, (x, v, c, vc), (x_in, v_in), span_of(front, direction), method, opts, K, maps


def _id(case):
    return "-".join(str(p) for p in case)


@pytest.mark.parametrize("case", RAW_CASES, ids=_id)
def test_raw_launch_against_float64_reference(case):
    front, refs, (x, v, c, vc), (x_in, v_in), t_span, method, opts, K, maps = case_setup(case)
    y, dy, name = raw_push(front, x_in, t_span, method, opts, K, tangents=v_in, cond=c, cond_tangents=vc, maps=maps)
    assert f"_{case[0]}_c4" in name, name             # the unit the case is meant for
    y64, d64 = refs[torch.float64].jvp(x, v, c, vc)
    y32, d32 = refs[torch.float32].jvp(x, v, c, vc)
    floor, sfloor = fp32_floor(d32, d64), fp32_floor(y32, y64)
    err, serr = R.normalised_error(dy, d64), R.normalised_error(y, y64)
    print(f"\n[pushforward] {_id(case)} {name}: tangent err {err:.3e} floor {floor:.3e} bar {FACTOR * floor:.3e}; "
          f"state err {serr:.3e} floor {sfloor:.3e}")
    assert serr <= FACTOR * sfloor, (serr, sfloor)
    assert err <= FACTOR * floor, (err, floor)


# ---- the state is the Hutchinson launch's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (2, 5, 9, 11, 14)], ids=_id)
def test_state_is_bitwise_the_k_probe_hutchinson_launch(case):
    front, _, (x, v, c, vc), (x_in, v_in), t_span, method, opts, K, maps = case_setup(case)
    y, _, _ = raw_push(front, x_in, t_span, method, opts, K, tangents=v_in, cond=c, cond_tangents=vc, maps=maps)
    net = front._net()
    table = front._ode_table(t_span, method, opts, _native.MODE_HUTCH)
    yh, _, _ = net.integrate(x_in.to(DEV), table, _native.MODE_HUTCH, cond=None if c is None else c.to(DEV),
                             probe=v_in.to(DEV).contiguous(), stage_slots=solvers.resolve_method(method).stages, **maps)
    assert torch.equal(y, yh)


# ---- linearity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (1, 8, 11, 12)], ids=_id)
def test_zero_tangents_give_zero_and_doubled_tangents_double(case):
    front, _, (x, v, c, vc), (x_in, v_in), t_span, method, opts, K, maps = case_setup(case)
    run = lambda tv, tc: raw_push(front, x_in, t_span, method, opts, K, tangents=tv, cond=c, cond_tangents=tc, maps=maps)
    y1, d1, _ = run(v_in, vc)
    y0, d0, _ = run(torch.zeros_like(v_in), None if vc is None else torch.zeros_like(vc))
    assert torch.equal(y0, y1) and bool((d0 == 0).all())
    if c is not None:                       # no state tangents at all (NULL): zero as well, and the conditional part alone
        _, dn, _ = run(None, None if vc is None else torch.zeros_like(vc))
        assert bool((dn == 0).all())
    y2, d2, _ = run(2.0 * v_in, None if vc is None else 2.0 * vc)
    assert torch.equal(y2, y1) and torch.equal(d2, 2.0 * d1)


def test_a_noise_row_is_left_out_and_reported_in_the_status_word():
    """The table is device memory, so the launcher cannot refuse a row with FF_ROW_NOISE; the kernel does: the noise is left
    out (the outputs are those of the table without the flag, bit for bit) and FF_STATUS_NOISE_ROW is set."""
    front, _, (x, v, c, vc), (x_in, v_in), t_span, method, opts, K, maps = case_setup(RAW_CASES[1])
    run = lambda **kw: raw_push(front, x_in, t_span, method, opts, K, tangents=v_in, cond=c, cond_tangents=vc, maps=maps, **kw)
    y, dy, _ = run()
    for row in (0, 7):                                       # a stage row and a step-end row (rk4, two steps: rows 0 .. 7)
        yn, dn, _ = run(noise_row=row, status_is=_native.STATUS_NOISE_ROW)
        assert torch.equal(yn, y) and torch.equal(dn, dy)


# ---- unit tangents ----------------------------------------------------------------------------------------------------------------
def test_unit_tangents_are_bitwise_the_one_hot_buffers():
    D, C, B = 16, 4, 9
    front, _ = make_front("vp", D, C, W256, 4)
    x, _, c, _ = inputs(B, D, C, 1)
    t_span, opts = span_of(front, "to_base"), options_of(front, "to_base", 2)
    shift, scale = affine_of(D)
    maps = dict(in_shift=shift, in_scale=scale)
    eye = torch.eye(D + C)
    for first, K in ((0, 15), (15, 5)):
        hot = eye[first:first + K].unsqueeze(0).expand(B, K, D + C)
        yu, du, _ = raw_push(front, x, t_span, "rk4", opts, K, cond=c, unit_first=first, maps=maps)
        yh, dh, _ = raw_push(front, x, t_span, "rk4", opts, K, tangents=hot[:, :, :D], cond=c, cond_tangents=hot[:, :, D:], maps=maps)
        assert torch.equal(yu, yh) and torch.equal(du, dh), first
        assert bool((du != 0).any())


# ---- the front ends -----------------------------------------------------------------------------------------------------------------
def _bar(ref, x, v=None, c=None, vc=None):
    d64, d32 = ref[torch.float64].jvp(x, v, c, vc)[1], ref[torch.float32].jvp(x, v, c, vc)[1]
    return FACTOR * fp32_floor(d32, d64), d64


def _conditional_model(D=5, C=3, width=100, nh=2):
    torch.manual_seed(21)
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=[width] * nh)
    return m, torch.linspace(-0.5, 0.5, D), torch.linspace(0.5, 1.5, D), torch.linspace(0.2, -0.2, C), torch.linspace(0.7, 1.9, C)


def test_jacobian_times_vector_is_the_jvp():
    D, C, B, K = 16, 4, 11, 3                        # D + C = 20 unit tangents: two launches
    front, ref_kw = make_front("subvp", D, C, 200, 2)
    front = front.to(DEV)
    x, v, c, vc = inputs(B, D, C, K)
    kw = dict(direction="to_data", method="rk4", options=options_of(front, "to_data", 2))
    y, dx = front.flow_jvp(x.to(DEV), v.to(DEV), c.to(DEV), vc.to(DEV), **kw)
    yj, Jx, Jc = front.flow_jacobian(x.to(DEV), c.to(DEV), **kw)
    assert torch.equal(y, yj) and Jx.shape == (B, D, D) and Jc.shape == (B, D, C)
    refs = {dt: R.SolverMap(direction="to_data", method="rk4", options=kw["options"], dtype=dt, **ref_kw)
            for dt in (torch.float32, torch.float64)}
    bar, d64 = _bar(refs, x, v, c, vc)
    assert R.normalised_error(dx, d64) <= bar
    J = torch.cat([Jx, Jc], dim=2).cpu().double()
    w = torch.cat([v, vc], dim=2).double()                              # [B, K, D + C]
    Jv = torch.einsum("bij,bkj->bki", J, w)
    # every entry of J carries at most `bar` of its column's scale; the product sums |J| |w| of them
    scale = torch.einsum("bij,bkj->bki", J.abs(), w.abs()).reshape(B, -1).amax(dim=1)
    assert bool(((Jv - dx.cpu().double()).abs().reshape(B, -1).amax(dim=1) <= 2 * bar * scale).all())
    J64, J32 = (torch.cat(refs[dt].jacobian(x, c)[1:], dim=2) for dt in (torch.float64, torch.float32))
    assert R.normalised_error(J.float(), J64) <= FACTOR * fp32_floor(J32, J64)


def test_row_cuts_slices_and_reruns_are_bitwise(monkeypatch):
    D, C, B, K = 3, 1, 37, 7
    front, _ = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, v, c, vc = (t.to(DEV) for t in inputs(B, D, C, K))
    kw = dict(direction="to_base", method="dopri5_fixed", options={"step_size": 0.5})
    whole = front.flow_jvp(x, v, c, vc, **kw)
    again = front.flow_jvp(x, v, c, vc, **kw)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))
    part = front.flow_jvp(x[5:20], v[5:20], c[5:20], vc[5:20], **kw)
    assert torch.equal(part[0], whole[0][5:20]) and torch.equal(part[1], whole[1][5:20])
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 5 * K * D + 1)       # five rows per launch: eight pieces
    cut = front.flow_jvp(x, v, c, vc, **kw)
    cutj = front.flow_jacobian(x, c, **kw)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(whole, cut))
    assert all(torch.equal(a, b) for a, b in zip(front.flow_jacobian(x, c, **kw), cutj))


@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_population_wrappers_apply_the_chain_rule(direction):
    m, shift, scale, cshift, cscale = _conditional_model()
    D, C, B, K = 5, 3, 9, 4
    pm = Dm.PopulationModelDiffusionConditional(model=m, sde=Dm.VPSDE(), shift=shift, scale=scale, conditional_shift=cshift,
                                                conditional_scale=cscale, method="rk4").to(DEV).eval()
    x, v, c, vc = inputs(B, D, C, K)
    opts = options_of(pm.score_model, direction, 2)
    kw = dict(direction=direction, method="rk4", options=opts)
    refs = {dt: R.SolverMap("score", R.score_params(m), direction, "rk4", opts, dtype=dt, sde="vp", affine=(shift, scale),
                            cond_affine=(cshift, cscale)) for dt in (torch.float32, torch.float64)}
    y, dx = pm.flow_jvp(x.to(DEV), v.to(DEV), c.to(DEV), vc.to(DEV), **kw)
    bar, d64 = _bar(refs, x, v, c, vc)
    assert R.normalised_error(dx, d64) <= bar
    y64, y32 = (refs[dt](x.to(dt), c.to(dt)) for dt in (torch.float64, torch.float32))
    assert R.normalised_error(y, y64) <= FACTOR * fp32_floor(y32, y64)
    # the conditional part alone: d x_out / d (raw conditional), the derivative inference over the hyper-parameters takes
    _, dc = pm.flow_jvp(x.to(DEV), None, c.to(DEV), vc.to(DEV), **kw)
    barc, dc64 = _bar(refs, x, None, c, vc)
    assert R.normalised_error(dc, dc64) <= barc
    _, Jx, Jc = pm.flow_jacobian(x.to(DEV), c.to(DEV), **kw)
    _, Jx64, Jc64 = refs[torch.float64].jacobian(x, c)
    _, Jx32, Jc32 = refs[torch.float32].jacobian(x, c)
    for got, r64, r32 in ((Jx, Jx64, Jx32), (Jc, Jc64, Jc32)):
        assert R.normalised_error(got, r64) <= FACTOR * fp32_floor(r32, r64)
    # the unconditional wrapper
    torch.manual_seed(22)
    mu = Dm.MLP(n_dimensions=D, n_conditionals=0, embedding_dimensions=8, units=[64, 64])
    pu = Dm.PopulationModelDiffusion(model=mu, sde=Dm.VESDE(), shift=shift, scale=scale, method="rk4").to(DEV).eval()
    optu = options_of(pu.score_model, direction, 2)
    refu = {dt: R.SolverMap("score", R.score_params(mu), direction, "rk4", optu, dtype=dt, sde="ve", affine=(shift, scale))
            for dt in (torch.float32, torch.float64)}
    _, du = pu.flow_jvp(x.to(DEV), v.to(DEV), direction=direction, method="rk4", options=optu)
    baru, du64 = _bar(refu, x, v)
    assert R.normalised_error(du, du64) <= baru


def test_round_trip_jacobians_multiply_to_the_identity():
    # (a flow: its velocity field is smooth over t in [0, 1], so five rk4 steps invert each other to ~1e-6 and the identity
    # is a real check; the score models' schedules are stiff on such a grid -- the reference's own residual there is 0.9)
    D, B = 6, 8
    front, ref_kw = make_front("flow", D, 0, 128, 2, affine=True)
    front = front.to(DEV)
    x = inputs(B, D, 0, 1)[0]
    opts = {"step_size": 0.2}
    y, J1, _ = front.flow_jacobian(x.to(DEV), direction="to_base", method="rk4", options=opts)
    _, J2, _ = front.flow_jacobian(y, direction="to_data", method="rk4", options=opts)
    ref = lambda d, dt: R.SolverMap(direction=d, method="rk4", options=opts, dtype=dt, **ref_kw)
    y64, A64, _ = ref("to_base", torch.float64).jacobian(x)
    _, B64, _ = ref("to_data", torch.float64).jacobian(y64)
    _, A32, _ = ref("to_base", torch.float32).jacobian(x)
    _, B32, _ = ref("to_data", torch.float32).jacobian(y64)
    eye = torch.eye(D, dtype=torch.float64)
    # the discrete map is not exactly its own inverse at finite h: the float64 reference's own residual on this grid is the
    # bound, plus what fp32 Jacobians carry into the product.  An entry of J2 is off by at most e2 max |J2| and one of J1 by
    # e1 max |J1| (e = the factor's bar, normalised as everywhere by the sample's largest entry), so entry (i, j) of the product
    # is off by at most  e2 max |J2| sum_k |J1_kj|  +  e1 max |J1| sum_k |J2_ik|  (and a second-order term, left out)
    residual = (B64 @ A64 - eye).abs().amax(dim=(1, 2))
    e1, e2 = FACTOR * fp32_floor(A32, A64), FACTOR * fp32_floor(B32, B64)
    carried = (e2 * B64.abs().amax(dim=(1, 2)) * A64.abs().sum(dim=1).amax(dim=1)
               + e1 * A64.abs().amax(dim=(1, 2)) * B64.abs().sum(dim=2).amax(dim=1))
    got = (J2.cpu().double() @ J1.cpu().double() - eye).abs().amax(dim=(1, 2))
    print(f"\n[pushforward] round trip: |J2 J1 - I| {float(got.max()):.3e}, float64 reference {float(residual.max()):.3e}, "
          f"bound {float((residual + carried).min()):.3e}")
    assert bool((got <= residual + carried).all()), (got, residual, carried)
