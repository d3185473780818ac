"""GPU tier of the exact discrete adjoint (csrc/ff_mlp_dadj.hpp, ff_mlp_ode_launch_record, ff_mlp_ode_launch_pull_discrete,
``flow_vjp(adjoint="discrete")``): raw launches of the three record and the three discrete-adjoint units between guard words on
NaN-prefilled outputs against the float64 reference (tests/_pullback_discrete_ref.py: ``torch.func.vjp`` of the discrete solver
map), the record against the float64 stage states, the state against ``solve``, the adjoint identity with ``flow_jvp`` on grids
where the continuous route misses it, the bitwise properties, the two status bits, the wrappers' chain rule, and the default
route unchanged.

Tolerance: the push and pull tests' rule and factor (tests/test_gpu_pushforward.py).  Per case the reference runs twice on the
CPU, in fp32 and in float64; the fp32 run's error per sample, normalised by the sample's largest reference entry, is the case's
fp32 floor, as measured, and the bar is that floor times FACTOR = 22.  Every case of RAW_CASES is one at which the float64
CONTINUOUS adjoint misses that bar by at least 100x and whose floor is at most 5e-5 (tests/test_pullback_discrete_host.py
checks both on the CPU), so a kernel that computed the continuous adjoint -- or anything between the two -- fails here.
profiles/pullback_discrete.txt lists the floors and the device's errors.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from flowfusion_amd import diffusion as Dm
from tests import _pullback_discrete_ref as DP
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import FACTOR, GUARD, _guarded, _payload, affine_of, fp32_floor, make_front, options_of, span_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE_TOL = 2e-5        # relative to max |reference state|: the state tests' bar (tests/test_gpu_parity.py)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def inputs(B, D, C, K, seed=31):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * D + K)
    x = torch.randn(B, D, generator=g)
    w = torch.randn(B, K, D, generator=g)
    c = torch.randn(B, C, generator=g) if C else None
    return x, w, c


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


def forward_table(front, plan, t_span, method, options, noise_row=None):
    tab = solvers.plan_ode(t_span, method, options)
    table = solvers.build_table(tab, *front._host_schedule()(tab.t_eval), int(plan.width))
    if noise_row is not None:
        table.view(torch.int32)[noise_row, solvers.ROW_FLAGS] |= solvers.FLAG_NOISE
    return table.to(DEV)


def _launch_args(front, t_span, method, options, cond, maps, slots, noise_row):
    net = front.to(DEV)._net()
    plan = net.pull_plan()
    table = forward_table(front, plan, t_span, method, options, noise_row)
    wp = net.wpack(torch.device(DEV), _native.MODE_HUTCH, plan)
    keep = {k: _dev(v) for k, v in (maps or {}).items()}
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.wpack, a.etab, a.status = wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if cond is None else cond.data_ptr()
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    a.n_evals = table.shape[0]
    a.stage_slots = solvers.resolve_method(method).stages if slots is None else slots
    return plan, a, status, (table, wp, keep)


def raw_record(front, x_in, t_span, method, options, cond=None, maps=None, slots=None, noise_row=None, status_is=0):
    """ff_mlp_ode_launch_record on buffers of the test's own over the FORWARD span: (x_out [B, D], record [E, B, D], the
    unit's name), guards checked."""
    x, cond = _dev(x_in), _dev(cond)
    plan, a, status, hold = _launch_args(front, t_span, method, options, cond, maps, slots, noise_row)
    B, D = x.shape
    E = int(a.n_evals)
    xo, rec = _guarded(B * D), _guarded(E * B * D)
    a.x_in, a.x_out, a.batch, a.mode = x.data_ptr(), xo.data_ptr() + 4 * GUARD, B, _native.MODE_STATE
    rc = _native.lib().ff_mlp_ode_launch_record(ctypes.byref(plan), ctypes.byref(a), rec.data_ptr() + 4 * GUARD,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    index = int(plan.kernel_id) - _native.PULL_KERNEL_BASE
    return _payload(xo, (B, D)), _payload(rec, (E, B, D)), _native.lib().ff_rec_kernel_name(index).decode()


def raw_discrete(front, rec, t_span, method, options, cotangents, cond=None, maps=None, want_cond=True, slots=None,
                 noise_row=None, status_is=0):
    """ff_mlp_ode_launch_pull_discrete over the SAME forward table and maps, on the record ``rec``: (cot_x [B, K, D], cot_cond
    [B, K, C] or None, the unit's name), guards checked."""
    rec, w, cond = _dev(rec), _dev(cotangents), _dev(cond)
    plan, a, status, hold = _launch_args(front, t_span, method, options, cond, maps, slots, noise_row)
    E, B, D = rec.shape
    assert E == int(a.n_evals)
    K, C = w.shape[1], (0 if cond is None else cond.shape[1])
    gx = _guarded(B * K * D)
    gc = _guarded(B * K * C) if (C and want_cond) else None
    a.batch, a.tangent_count, a.mode = B, K, _native.MODE_HUTCH
    rc = _native.lib().ff_mlp_ode_launch_pull_discrete(ctypes.byref(plan), ctypes.byref(a), rec.data_ptr(), w.data_ptr(),
                                                       gx.data_ptr() + 4 * GUARD, 0 if gc is None else gc.data_ptr() + 4 * GUARD,
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    index = int(plan.kernel_id) - _native.PULL_KERNEL_BASE
    return (_payload(gx, (B, K, D)), None if gc is None else _payload(gc, (B, K, C)),
            _native.lib().ff_dadj_kernel_name(index).decode())


# (unit, model, D, C, K, B, width, hidden layers, method, steps, direction, affine); B = 1, samples per tile + 1, 37.
# Which (model, method, steps, direction) discriminate between the two adjoints is measured, not guessed: Euler on any field,
# the higher orders on the score models where test_pullback_discrete_host finds the continuous gap >= 100 bars.
RAW_CASES = [
    ("h128_d4", "vp", 1, 0, 1, 1, 32, 1, "euler", 1, "to_data", False),
    ("h128_d4", "ve", 4, 1, 2, 16 // 3 + 1, 128, 4, "midpoint", 2, "to_data", True),
    ("h128_d4", "subvp", 16, 16, 15, 37, 128, 1, "heun3", 5, "to_data", True),
    ("h128_d4", "flow", 5, 0, 7, 16 // 8 + 1, 32, 4, "euler", 2, "to_base", False),
    ("h128_d4", "flow", 16, 1, 1, 37, 128, 2, "euler", 5, "to_data", True),
    ("h256_d4", "vp", 1, 16, 15, 16 // 16 + 1, 256, 4, "dopri5_fixed", 1, "to_data", False),
    ("h256_d4", "ve", 16, 0, 2, 37, 256, 1, "euler", 5, "to_base", True),
    ("h256_d4", "vp", 4, 1, 1, 16 // 2 + 1, 256, 4, "rk4", 5, "to_base", True),
    ("h256_d4", "flow", 16, 16, 7, 16 // 8 + 1, 256, 1, "euler", 1, "to_data", False),
    ("h256_d4", "vp", 5, 0, 15, 37, 256, 4, "rk4_classic", 2, "to_data", False),
    ("h256_d8", "vp", 17, 0, 1, 1, 256, 1, "rk4", 1, "to_data", False),
    ("h256_d8", "vp", 32, 16, 15, 37, 256, 4, "dopri5_fixed", 5, "to_base", True),
    ("h256_d8", "subvp", 17, 1, 2, 16 // 3 + 1, 256, 2, "euler", 5, "to_data", True),
    ("h256_d8", "flow", 32, 0, 7, 16 // 8 + 1, 256, 1, "euler", 2, "to_base", True),
    ("h256_d8", "ve", 17, 16, 1, 37, 256, 4, "heun3", 1, "to_data", False),
]


def case_setup(case):
    """The front end, the inputs, what the launches take (the start of the forward solve, the network's conditional, the
    chain rule's factors, the forward solve's maps) and the SolverMap in fp32 / float64, which works in the user's units."""
    unit, kind, D, C, K, B, width, nh, method, nsteps, direction, affine = case
    front, ref_kw = make_front(kind, D, C, width, nh, affine=affine)
    x, w, c = inputs(B, D, C, K)
    opts = options_of(front, direction, nsteps)
    maps, ref_aff = {}, {}
    if affine:
        shift, scale = affine_of(D)
        maps = dict(out_scale=scale, out_shift=shift) if direction == "to_data" else dict(in_shift=shift, in_scale=scale)
        if kind != "flow":
            ref_aff = dict(affine=(shift, scale))
    smaps = {dt: R.SolverMap(direction=direction, method=method, options=opts, dtype=dt, **ref_kw, **ref_aff)
             for dt in (torch.float32, torch.float64)}
    # a score model's to_data solve starts from x * sigma_max: the chain rule's factor on cot_x
    gain = float(front.sde.sigma_max) if (kind != "flow" and direction == "to_data" and hasattr(front.sde, "sigma_max")) else 1.0
    # a flow's network sees the normalised conditional: the chain rule's factor on cot_cond
    c_net, c_scale = c, None
    if kind == "flow" and C:
        c_net, c_scale = front._norm_cond(c), front.conditional_scale.detach().cpu()
    return front, smaps, (x, w, c), (x * gain, c_net, gain, c_scale), span_of(front, direction), method, opts, maps


def _id(case):
    return "-".join(str(p) for p in case)


def run_case(case, cotangents=None, rows=None, slots=None, noise_row=None, status_is=0, want_cond=True):
    """((x_out, record), (cot_x, cot_cond) in the USER's units, the two units' names) of a raw case; ``rows``: a slice of the
    batch."""
    front, _, (x, w, c), (x_in, c_net, gain, c_scale), t_span, method, opts, maps = case_setup(case)
    w = w if cotangents is None else cotangents
    if rows is not None:
        x_in, w, c_net = x_in[rows], w[rows], (None if c_net is None else c_net[rows])
    kw = dict(cond=c_net, maps=maps, slots=slots, noise_row=noise_row, status_is=status_is)
    y, rec, rec_name = raw_record(front, x_in, t_span, method, opts, **kw)
    gx, gc, dadj_name = raw_discrete(front, rec, t_span, method, opts, w, want_cond=want_cond, **kw)
    gx, gc = gx.cpu() * gain, (None if gc is None else gc.cpu())
    if gc is not None and c_scale is not None:
        gc = gc / c_scale
    return (y.cpu(), rec.cpu()), (gx, gc), (rec_name, dadj_name)


_REFS = {}


def references(case):
    """The fp32 and float64 discrete references of a case and the float64 stage states, computed once and shared."""
    if case not in _REFS:
        _, smaps, (x, w, c), *_ = case_setup(case)
        r64, r32 = DP.DiscretePullback(smaps[torch.float64]), DP.DiscretePullback(smaps[torch.float32])
        _REFS[case] = (r64(x, w, c), r32(x, w, c), r64.stage_states(x, c))
    return _REFS[case]


@pytest.mark.parametrize("case", RAW_CASES, ids=_id)
def test_raw_launches_against_float64_reference(case):
    (y, rec), (gx, gc), names = run_case(case)
    assert names == (f"mlp_rec_m16_{case[0]}_c4", f"mlp_dadj_m16_{case[0]}_c4"), names       # the units the case is meant for
    (y64, gx64, gc64), (y32, gx32, gc32), (rec64, _) = references(case)
    line = f"\n[pullback_discrete] {_id(case)}:"
    # the record: every stage state at the state tests' bar
    rec_err = float(((rec.double() - rec64).abs().amax(dim=(1, 2)) / rec64.abs().amax(dim=(1, 2)).clamp_min(1e-30)).max())
    line += f" record err {rec_err:.3e};"
    checks = [("x_out", y, y64, y32), ("cot_x", gx, gx64, gx32)]
    if gc64 is not None:
        checks.append(("cot_cond", gc, gc64, gc32))
    worst = []
    for what, got, ref64, ref32 in checks:
        floor, err = fp32_floor(ref32, ref64), R.normalised_error(got, ref64)
        line += f" {what} err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors);"
        worst.append((what, err, floor))
    print(line)
    assert rec_err <= STATE_TOL, rec_err
    for what, err, floor in worst:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (1, 7, 11, 12)], ids=_id)
def test_state_is_the_state_only_solve_and_ignores_the_cotangent_side(case):
    front, _, (x, w, c), (x_in, c_net, gain, c_scale), t_span, method, opts, maps = case_setup(case)
    (y, rec), (gx, gc), _ = run_case(case)
    solo, _ = odeint.solve(front.to(DEV), _dev(x_in), t_span, method, opts, _native.MODE_STATE, 0.0, 0.0, cond=_dev(c_net),
                           **{k: _dev(v) for k, v in maps.items()})
    err = float((y - solo.cpu()).abs().max() / solo.abs().max())
    print(f"\n[pullback_discrete] {_id(case)}: record launch's x_out against solve {err:.3e}, bitwise {torch.equal(y, solo.cpu())}")
    assert torch.equal(y, solo.cpu())               # (the same fp32 chains in the same order as the state kernels: measured bitwise)
    # other cotangents, one cotangent, no conditional output: the state and the record do not move, bit for bit
    (y2, rec2), (gx2, _), _ = run_case(case, cotangents=3.0 * w + 1.0)
    assert torch.equal(y2, y) and torch.equal(rec2, rec) and not torch.equal(gx2, gx)
    (y1, rec1), _, _ = run_case(case, cotangents=w[:, :1])
    assert torch.equal(y1, y) and torch.equal(rec1, rec)
    (_, _), (gxn, gcn), _ = run_case(case, want_cond=False)
    assert gcn is None and torch.equal(gxn, gx)


# ---- bitwise properties, linearity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (2, 5, 9, 11)], ids=_id)
def test_reruns_columns_and_batch_slices_are_bitwise_and_the_map_is_linear(case):
    _, _, (x, w, c), *_ = case_setup(case)
    (y, rec), (gx, gc), _ = run_case(case)
    (ya, reca), (gxa, gca), _ = run_case(case)
    assert torch.equal(ya, y) and torch.equal(reca, rec) and torch.equal(gxa, gx) and (gc is None or torch.equal(gca, gc))
    for k in (0, w.shape[1] - 1):                   # column k of the K launch = the K = 1 launch of that cotangent
        _, (gx1, gc1), _ = run_case(case, cotangents=w[:, k:k + 1])
        assert torch.equal(gx1[:, 0], gx[:, k]) and (gc is None or torch.equal(gc1[:, 0], gc[:, k]))
    B = x.shape[0]
    rows = slice(B // 3, B // 3 + max(1, B // 2))
    (ys, recs), (gxs, gcs), _ = run_case(case, rows=rows)
    assert torch.equal(ys, y[rows]) and torch.equal(recs, rec[:, rows]) and torch.equal(gxs, gx[rows])
    assert gc is None or torch.equal(gcs, gc[rows])
    # linearity: zero gives zero exactly; w -> 2 w doubles bit for bit (a power of two); w + w' adds up to rounding
    _, (gx0, gc0), _ = run_case(case, cotangents=torch.zeros_like(w))
    assert bool((gx0 == 0).all()) and (gc0 is None or bool((gc0 == 0).all()))
    _, (gx2, gc2), _ = run_case(case, cotangents=2.0 * w)
    assert torch.equal(gx2, 2.0 * gx) and (gc is None or torch.equal(gc2, 2.0 * gc))
    other = torch.flip(w, dims=(1,)) * 0.5 + 0.25
    _, (gxo, _), _ = run_case(case, cotangents=other)
    _, (gxs_, _), _ = run_case(case, cotangents=w + other)
    floor = fp32_floor(references(case)[1][1], references(case)[0][1])
    scale = (gx.abs() + gxo.abs()).reshape(B, -1).amax(dim=1).clamp_min(1e-30)
    assert float(((gxs_ - (gx + gxo)).abs().reshape(B, -1).amax(dim=1) / scale).max()) <= FACTOR * floor


def test_row_cuts_slices_and_reruns_of_the_front_end_are_bitwise(monkeypatch):
    D, C, B, K = 4, 1, 37, 7
    front, _ = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, w, c = (t.to(DEV) for t in inputs(B, D, C, K))
    kw = dict(direction="to_base", method="dopri5_fixed", options={"step_size": 0.5}, adjoint="discrete")
    whole = front.flow_vjp(x, w, c, **kw)
    again = front.flow_vjp(x, w, c, **kw)
    assert len(whole) == 3 and all(torch.equal(a, b) for a, b in zip(whole, again))
    part = front.flow_vjp(x[5:20], w[5:20], c[5:20], **kw)
    assert all(torch.equal(a, b[5:20]) for a, b in zip(part, whole))
    one = front.flow_vjp(x, w[:, 2:3], c, **kw)                              # the state does not depend on K
    assert torch.equal(one[0], whole[0]) and torch.equal(one[1][:, 0], whole[1][:, 2])
    # 14 evaluation rows: the record [14, rows, D] is what bounds the piece -- two rows per launch, nineteen pieces
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 2 * 14 * D + 1)
    cut = front.flow_vjp(x, w, c, **kw)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(whole, cut))
    # a K-bound cut: euler, one row, K * D floats per sample
    kw1 = dict(kw, method="euler", options={"step_size": 1.0})
    whole1 = front.flow_vjp(x, w, c, **kw1)
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 5 * K * D + 1)
    cut1 = front.flow_vjp(x, w, c, **kw1)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(whole1, cut1))


# ---- the status word ---------------------------------------------------------------------------------------------------------------
def test_a_slot_beyond_the_kept_ones_is_reported_and_contributes_nothing():
    """rk4, two steps, ``stage_slots`` one short: the rows of slot 3 store nothing forward (FF_STATUS_BAD_SLOT from the
    record launch) and contribute nothing backward (the same bit from the discrete launch).  Every output word is written
    and finite; what they hold is the map without that stage, which nobody should use."""
    case = RAW_CASES[7]
    (y, rec), (gx, gc), _ = run_case(case, slots=3, status_is=_native.STATUS_BAD_SLOT)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all()) and bool(torch.isfinite(rec).all())
    (y_ok, _), (gx_ok, _), _ = run_case(case)
    assert not torch.equal(y, y_ok) and not torch.equal(gx, gx_ok)


def test_a_noise_row_is_left_out_and_reported_in_the_status_word():
    case = RAW_CASES[7]
    (y, rec), (gx, gc), _ = run_case(case)
    for row in (0, 7):                                       # a stage row and a step-end row (rk4: rows 0 .. 19)
        (yn, recn), (gn, cn), _ = run_case(case, noise_row=row, status_is=_native.STATUS_NOISE_ROW)
        assert torch.equal(yn, y) and torch.equal(recn, rec) and torch.equal(gn, gx) and torch.equal(cn, gc)


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
def _vp_model(D=4, C=2, units=(64, 64), seed=5):
    torch.manual_seed(seed)
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=list(units))
    return Dm.ScoreModel(m, Dm.VPSDE(), no_sigma=False).eval(), dict(kind="score", params=R.score_params(m), sde="vp")


@pytest.mark.parametrize("method, nsteps", [("euler", 1), ("rk4", 2)])
@pytest.mark.parametrize("direction", ["to_data"])
def test_adjoint_identity_with_flow_jvp_where_the_continuous_route_misses_it(method, nsteps, direction):
    """<w, flow_jvp(v, vc)> = <flow_vjp(w, adjoint="discrete"), (v, vc)> per sample on a VP score model at one Euler step
    and at two rk4 steps.  Bar, as in tests/test_gpu_pullback.py: every entry of dx is off by at most FACTOR x its fp32 floor
    x the sample's largest |dx|, every entry of (gx, gc) likewise, so the two inner products differ by at most
    FACTOR (floor_push max|dx| sum|w| + floor_pull max|g| sum|(v, vc)|); the float64 references' own gap is rounding.  The
    same call with ``adjoint="continuous"`` must MISS that bar on some sample: there the two adjoints are far apart."""
    D, C, B, K = 4, 2, 11, 3
    front, ref_kw = _vp_model(D, C)
    front = front.to(DEV)
    x, w, c = inputs(B, D, C, K)
    g = torch.Generator().manual_seed(77)
    v, vc = torch.randn(B, K, D, generator=g), torch.randn(B, K, C, generator=g)
    kw = dict(direction=direction, method=method, options=options_of(front, direction, nsteps))
    _, dx = front.flow_jvp(_dev(x), _dev(v), _dev(c), _dev(vc), **kw)
    maps = {dt: R.SolverMap(direction=direction, method=method, options=kw["options"], dtype=dt, **ref_kw)
            for dt in (torch.float32, torch.float64)}
    dx64, dx32 = (maps[dt].jvp(x, v, c, vc)[1] for dt in (torch.float64, torch.float32))
    (_, gx64, gc64), (_, gx32, gc32) = (DP.DiscretePullback(maps[dt])(x, w, c) for dt in (torch.float64, torch.float32))
    g64, g32 = torch.cat([gx64, gc64], dim=2), torch.cat([gx32, gc32], dim=2)
    floor_push, floor_pull = fp32_floor(dx32, dx64), fp32_floor(g32, g64)
    u = torch.cat([v, vc], dim=2).double()
    lhs = (w.double() * dx.cpu().double()).sum(dim=2)
    gap64 = ((w.double() * dx64).sum(dim=2) - (g64 * u).sum(dim=2)).abs()
    bound = FACTOR * (floor_push * dx64.abs().reshape(B, -1).amax(dim=1)[:, None] * w.double().abs().sum(dim=2)
                      + floor_pull * g64.abs().reshape(B, -1).amax(dim=1)[:, None] * u.abs().sum(dim=2)) + gap64
    miss = {}
    for adjoint in ("discrete", "continuous"):
        _, gx, gc = front.flow_vjp(_dev(x), _dev(w), _dev(c), adjoint=adjoint, **kw)
        rhs = (torch.cat([gx, gc], dim=2).cpu().double() * u).sum(dim=2)
        miss[adjoint] = (lhs - rhs).abs() / bound
        print(f"\n[pullback_discrete] adjoint identity {method} x{nsteps} {direction} adjoint={adjoint}: worst |lhs - rhs| / bound "
              f"{float(miss[adjoint].max()):.3e}, float64 gap {float(gap64.max()):.3e}, floors {floor_push:.3e} {floor_pull:.3e}")
    assert float(gap64.max()) <= 1e-12 * float((w.double() * dx64).sum(dim=2).abs().max())
    assert bool((miss["discrete"] <= 1.0).all()), miss["discrete"]
    assert float(miss["continuous"].max()) > 1.0, miss["continuous"]


@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_population_wrappers_apply_the_chain_rule(direction):
    """The two wrappers against float64.  to_data: midpoint, two steps, and the default ONE-step grid of the wrappers; to_base:
    rk4 / dopri5_fixed with five steps (the grids at which a score model's to_base floor is small)."""
    torch.manual_seed(21)
    D, C, B, K = 5, 3, 9, 4
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=[100, 100])
    shift, scale = torch.linspace(-0.5, 0.5, D), torch.linspace(0.5, 1.5, D)
    cshift, cscale = torch.linspace(0.2, -0.2, C), torch.linspace(0.7, 1.9, C)
    pm = Dm.PopulationModelDiffusionConditional(model=m, sde=Dm.VPSDE(), shift=shift, scale=scale, conditional_shift=cshift,
                                                conditional_scale=cscale, method="rk4").to(DEV).eval()
    x, w, c = inputs(B, D, C, K)
    method, nsteps = ("midpoint", 2) if direction == "to_data" else ("rk4", 5)
    opts = options_of(pm.score_model, direction, nsteps)
    refs = {dt: DP.DiscretePullback(R.SolverMap("score", R.score_params(m), direction, method, opts, dtype=dt, sde="vp",
                                                affine=(shift, scale), cond_affine=(cshift, cscale)))
            for dt in (torch.float32, torch.float64)}
    y, gx, gc = pm.flow_vjp(_dev(x), _dev(w), _dev(c), direction=direction, method=method, options=opts, adjoint="discrete")
    (y64, gx64, gc64), (y32, gx32, gc32) = (refs[dt](x, w, c) for dt in (torch.float64, torch.float32))
    for got, r64, r32 in ((y, y64, y32), (gx, gx64, gx32), (gc, gc64, gc32)):
        assert R.normalised_error(got, r64) <= FACTOR * fp32_floor(r32, r64)
    # the unconditional wrapper, on a VE model: to_data starts from x * sigma_max, and gx carries the factor
    torch.manual_seed(22)
    mu = Dm.MLP(n_dimensions=D, n_conditionals=0, embedding_dimensions=8, units=[64, 64])
    pu = Dm.PopulationModelDiffusion(model=mu, sde=Dm.VESDE(), shift=shift, scale=scale, method="rk4").to(DEV).eval()
    methodu, nu = ("rk4", 1) if direction == "to_data" else ("dopri5_fixed", 5)
    optu = None if direction == "to_data" else options_of(pu.score_model, direction, nu)      # None: the default ONE-step grid
    refu = {dt: DP.DiscretePullback(R.SolverMap("score", R.score_params(mu), direction, methodu, optu, dtype=dt, sde="ve",
                                                affine=(shift, scale))) for dt in (torch.float32, torch.float64)}
    yu, gu, none = pu.flow_vjp(_dev(x), _dev(w), direction=direction, method=methodu, options=optu, adjoint="discrete")
    (yu64, gu64, _), (yu32, gu32, _) = (refu[dt](x, w) for dt in (torch.float64, torch.float32))
    assert none is None
    assert R.normalised_error(yu, yu64) <= FACTOR * fp32_floor(yu32, yu64)
    assert R.normalised_error(gu, gu64) <= FACTOR * fp32_floor(gu32, gu64)


def test_the_default_route_is_the_continuous_one_bit_for_bit():
    D, C, B, K = 5, 3, 21, 3
    front, _ = make_front("flow", D, C, 128, 2, affine=True)
    front = front.to(DEV)
    x, w, c = (t.to(DEV) for t in inputs(B, D, C, K))
    sm, _ = _vp_model(4, 2)
    sm = sm.to(DEV)
    xs, ws, cs = (t.to(DEV) for t in inputs(B, 4, 2, K))
    for direction in ("to_data", "to_base"):
        kw = dict(direction=direction, method="rk4", options={"step_size": 0.25}, return_retrace=True)
        default, explicit = front.flow_vjp(x, w, c, **kw), front.flow_vjp(x, w, c, adjoint="continuous", **kw)
        assert len(default) == 4 and all(torch.equal(a, b) for a, b in zip(default, explicit))
        t_span, pkw = front._push_args(x, c, direction)
        direct = odeint.solve_pull(front, x, t_span, "rk4", kw["options"], w, return_retrace=True, **pkw)
        assert all(torch.equal(a, b) for a, b in zip(default, direct))
        ds, es = sm.flow_vjp(xs, ws, cs, **kw), sm.flow_vjp(xs, ws, cs, adjoint="continuous", **kw)
        assert all(torch.equal(a, b) for a, b in zip(ds, es))
        # and the discrete route's state is the continuous route's, which is the state-only solve's, bit for bit
        yd = front.flow_vjp(x, w, c, direction=direction, method="rk4", options={"step_size": 0.25}, adjoint="discrete")[0]
        assert torch.equal(yd, default[0])
