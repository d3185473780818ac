"""GPU tier of the log-density gradients (csrc/ff_mlp_lgrad.hpp, ff_mlp_ode_launch_logp_grad, ``log_prob_grad``): raw launches of
the three log-density gradient units between guard words on NaN-prefilled outputs against the float64 reference
(tests/_logp_grad_ref.py: ``torch.autograd.grad`` of the fixed-grid Hutchinson log-density, the divergence of every row from
``torch.func.jvp``), the two paths in isolation, the bitwise properties, and the front ends.

Tolerance: the derivative families' rule and factor (tests/test_gpu_pushforward.py).  Per case the reference runs twice on the
CPU, in fp32 and in float64; the fp32 run's error per sample, normalised by the sample's largest reference entry, is the case's
fp32 floor, as measured, and the bar is that floor times FACTOR = 22.  tests/test_logp_grad_host.py checks on the CPU, for every
case of CASES, that the floor is at most 5e-5, that the float64 reference without the SiLU'' cross term misses the bar by at
least 100x, that a pair of swapped weight rows in the first, a middle or the last hidden layer does too, and that the
second-order share of the gradient is not negligible -- so a kernel that dropped or mis-addressed the second-order path fails
here.  Default-initialised networks are blind to all of that: every case carries a gain (tests/_deep_models.py), found on the CPU
in float64 and written here as a literal.  profiles/logp_grad.txt lists the floors and the device's errors.
"""
import ctypes
from collections import namedtuple

import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import diffusion as Dm
from tests import _deep_models as DM
from tests import _logp_grad_ref as LG
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import FACTOR, GUARD, _guarded, _payload, affine_of, fp32_floor, make_front, options_of, span_of

pytestmark = pytest.mark.gpu
DEV = "cuda"

Case = namedtuple("Case", "unit kind D C B width nh method steps affine gain")

# Units: each of the three.  D: 1, 16, 17 / 32 (the d8 unit).  C: 0, 1, 16.  Hidden layers: 1, 2, 4, 5 (the phases of the weight
# ring's wrap) and the deepest each unit accepts (19 x 128, 9 x 256: 64 n_hidden width bytes of stash under 160 KiB).  B: 1, 8
# (one full tile), 9, 17.  Methods: euler (one slot), rk4, dopri5_fixed (seven slots, FSAL); 1 to 3 steps.  A VP score model and a
# flow: the VP cases keep to three rk4 steps, the grid at which a score model's fp32 floor is under the host file's cap (with
# euler or fewer steps the Fourier time features and 1 / sigma(t) near epsilon put it at 1e-4 .. 1e-3); the flows carry the
# other methods and step counts.  The gains: tests/test_logp_grad_host.py.
CASES = [
    Case("h128_d4", "vp", 1, 0, 1, 128, 1, "rk4", 3, False, 1.0),
    Case("h128_d4", "flow", 16, 1, 9, 128, 2, "euler", 1, False, 6.0),
    Case("h128_d4", "vp", 5, 16, 17, 128, 4, "rk4", 3, True, 1.5),
    Case("h128_d4", "flow", 16, 0, 8, 128, 5, "dopri5_fixed", 3, True, 3.0),
    Case("h128_d4", "flow", 16, 1, 9, 128, 19, "rk4", 1, False, 2.6),
    Case("h256_d4", "vp", 16, 0, 17, 256, 1, "rk4", 3, False, 1.0),
    Case("h256_d4", "flow", 1, 16, 8, 256, 2, "dopri5_fixed", 1, False, 6.0),
    Case("h256_d4", "vp", 4, 1, 9, 256, 4, "rk4", 3, True, 1.25),
    Case("h256_d4", "flow", 16, 16, 1, 256, 5, "euler", 2, False, 3.0),
    Case("h256_d4", "flow", 16, 0, 9, 256, 9, "dopri5_fixed", 1, False, 2.8),
    Case("h256_d8", "vp", 17, 0, 9, 256, 1, "rk4", 3, False, 1.0),
    Case("h256_d8", "flow", 32, 16, 17, 256, 2, "dopri5_fixed", 1, True, 6.0),
    Case("h256_d8", "vp", 32, 1, 8, 256, 4, "rk4", 3, False, 2.0),
    Case("h256_d8", "flow", 17, 0, 1, 256, 5, "euler", 3, False, 3.0),
    Case("h256_d8", "vp", 32, 16, 9, 256, 9, "rk4", 3, False, 2.0),
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _id(case):
    return "-".join(str(p) for p in case)


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


def case_inputs(case, seed=43):
    """(x [B, D], +-1 probes [B, D], cond [B, C] or None) of a case."""
    g = torch.Generator().manual_seed(seed + 1000 * case.B + 10 * case.D + case.C)
    x = torch.randn(case.B, case.D, generator=g)
    e = torch.sign(torch.randn(case.B, case.D, generator=g))
    c = torch.randn(case.B, case.C, generator=g) if case.C else None
    return x, e, c


def case_setup(case, damage=None):
    """(front end, {dtype: LogDensity}, what the launches take: the network's conditional, the chain rule's factor on grad_c,
    the span, the options, the forward solve's maps).  ``damage``: a hidden layer whose first two weight rows the references
    swap (the host file's discrimination check)."""
    front, ref_kw = make_front(case.kind, case.D, case.C, case.width, case.nh, affine=case.affine, gain=case.gain)
    if damage is not None:
        ref_kw = dict(ref_kw, params=DM.swap_rows(ref_kw["params"], damage))
    opts = options_of(front, "to_base", case.steps)
    maps, ref_aff = {}, {}
    if case.affine:
        shift, scale = affine_of(case.D)
        maps = dict(in_shift=shift, in_scale=scale)
        if case.kind != "flow":
            ref_aff = dict(affine=(shift, scale))
    refs = {dt: LG.LogDensity(R.SolverMap(direction="to_base", method=case.method, options=opts, dtype=dt, **ref_kw, **ref_aff))
            for dt in (torch.float32, torch.float64)}
    _, _, c = case_inputs(case)
    c_net, c_scale = c, None
    if case.kind == "flow" and case.C:
        c_net, c_scale = front._norm_cond(c), front.conditional_scale.detach().cpu()
    return front, refs, (c_net, c_scale), span_of(front, "to_base"), opts, maps


_REFS = {}


def references(case, **weights):
    """{dtype: (log_p, grad_x, grad_c)} of a case's fp32 and float64 references (``weights``: ``div_weight`` / ``cot_weight`` of
    the reference), computed once and shared."""
    key = (case, tuple(sorted(weights.items())))
    if key not in _REFS:
        _, refs, *_ = case_setup(case)
        x, e, c = case_inputs(case)
        _REFS[key] = {dt: refs[dt](x, c, e[:, None], 1.0, **weights) for dt in refs}
    return _REFS[key]


def floors_and_errors(case, gx, gc, **weights):
    """[(what, error of the device against float64, the case's fp32 floor)] for grad_x and, where there is one, grad_c."""
    r = references(case, **weights)
    (_, gx64, gc64), (_, gx32, gc32) = r[torch.float64], r[torch.float32]
    out = [("grad_x", R.normalised_error(gx, gx64), fp32_floor(gx32, gx64))]
    if gc64 is not None:
        out.append(("grad_c", R.normalised_error(gc, gc64), fp32_floor(gc32, gc64)))
    return out


def raw_logp_grad(front, rec, t_span, method, options, probes, weight, cot, cond=None, maps=None, want_cond=True, slots=None,
                  status_is=0):
    """ff_mlp_ode_launch_logp_grad over the record launch's table and maps, on the record ``rec``: (grad_x [B, D], grad_c
    [B, C] or None, the unit's name), guards checked."""
    from tests.test_gpu_pullback_discrete import _launch_args
    rec, probes, weight, cot, cond = _dev(rec), _dev(probes), _dev(weight), _dev(cot), _dev(cond)
    plan, a, status, hold = _launch_args(front, t_span, method, options, cond, maps, slots, None)
    E, B, D = rec.shape
    assert E == int(a.n_evals)
    C = 0 if cond is None else cond.shape[1]
    gx = _guarded(B * D)
    gc = _guarded(B * C) if (C and want_cond) else None
    a.batch, a.tangent_count, a.mode = B, 1, _native.MODE_HUTCH
    rc = _native.lib().ff_mlp_ode_launch_logp_grad(ctypes.byref(plan), ctypes.byref(a), rec.data_ptr(), probes.data_ptr(),
                                                   0 if weight is None else weight.data_ptr(), cot.data_ptr(),
                                                   gx.data_ptr() + 4 * GUARD, 0 if gc is None else gc.data_ptr() + 4 * GUARD,
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    index = int(plan.kernel_id) - _native.PULL_KERNEL_BASE
    return _payload(gx, (B, D)), None if gc is None else _payload(gc, (B, C)), _native.lib().ff_lgrad_kernel_name(index).decode()


def run_case(case, weight=None, prior=True, rows=None, want_cond=True):
    """(grad_x, grad_c in the USER's units, the unit's name, the record launch's state and the final cotangent) of a raw case:
    the record launch, the prior's gradient at its state (``prior=False``: a zero cotangent), the gradient launch with the
    per-row ``weight`` (None: the launch's NULL = 1).  ``rows``: a slice of the batch."""
    from tests.test_gpu_pullback_discrete import raw_record
    front, refs, (c_net, c_scale), t_span, opts, maps = case_setup(case)
    x, e, _ = case_inputs(case)
    if rows is not None:
        x, e, c_net = x[rows], e[rows], (None if c_net is None else c_net[rows])
        weight = None if weight is None else weight[rows]
    y, rec, _ = raw_record(front, x, t_span, case.method, opts, cond=c_net, maps=maps)
    var = refs[torch.float64].prior_scale() ** 2
    cot = -y / var if prior else torch.zeros_like(y)
    gx, gc, name = raw_logp_grad(front, rec, t_span, case.method, opts, e, weight, cot, cond=c_net, maps=maps, want_cond=want_cond)
    gx, gc = gx.cpu(), (None if gc is None else gc.cpu())
    if gc is not None and c_scale is not None:
        gc = gc / c_scale
    return gx, gc, name, (y, rec, cot)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_raw_launch_against_float64_reference(case):
    gx, gc, name, _ = run_case(case)
    assert name == f"mlp_lgrad_m16_{case.unit}_c4", name             # the unit the case is meant for
    line = f"\n[logp_grad] {_id(case)}:"
    results = floors_and_errors(case, gx, gc)
    for what, err, floor in results:
        line += f" {what} err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors);"
    print(line)
    for what, err, floor in results:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


@pytest.mark.parametrize("case", [CASES[i] for i in (1, 4, 7, 9, 12, 14)], ids=_id)
def test_a_zero_final_cotangent_isolates_the_second_order_path(case):
    gx, gc, _, _ = run_case(case, prior=False)
    line = f"\n[logp_grad] second-order path alone {_id(case)}:"
    results = floors_and_errors(case, gx, gc, cot_weight=0.0)
    for what, err, floor in results:
        line += f" {what} err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors);"
    print(line)
    for what, err, floor in results:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


@pytest.mark.parametrize("case", [CASES[i] for i in (2, 4, 8, 9, 11, 14)], ids=_id)
def test_a_zero_weight_isolates_the_state_path_and_agrees_with_the_discrete_adjoint(case):
    """``dlogp_cotangent = 0``: what is left is ``flow_vjp(adjoint="discrete")`` at K = 1 of the same final cotangent, over the same
    record.  Tolerance: the case's bar for the state path alone (the float64 reference at ``div_weight = 0``)."""
    from tests.test_gpu_pullback_discrete import raw_discrete
    front, _, (c_net, c_scale), t_span, opts, maps = case_setup(case)
    gx, gc, _, (y, rec, cot) = run_case(case, weight=torch.zeros(case.B))
    dx, dc, _ = raw_discrete(front, rec, t_span, case.method, opts, cot[:, None], cond=c_net, maps=maps)
    dx, dc = dx[:, 0].cpu(), (None if dc is None else dc[:, 0].cpu())
    if dc is not None and c_scale is not None:
        dc = dc / c_scale
    results = floors_and_errors(case, gx, gc, div_weight=0.0)
    pairs = [("grad_x", gx, dx)] + ([("grad_c", gc, dc)] if gc is not None else [])
    for (what, err, floor), (_, got, other) in zip(results, pairs):
        gap = R.normalised_error(got, other)
        print(f"\n[logp_grad] state path alone {_id(case)} {what}: err {err:.3e} floor {floor:.3e}, against the discrete adjoint "
              f"{gap:.3e}, bitwise {torch.equal(got, other)}")
        assert err <= FACTOR * floor and gap <= FACTOR * floor, (what, err, gap, floor)


@pytest.mark.parametrize("case", [CASES[i] for i in (2, 5, 9, 11)], ids=_id)
def test_reruns_batch_slices_and_the_null_weight_are_bitwise(case):
    gx, gc, _, _ = run_case(case)
    gxa, gca, _, _ = run_case(case)
    assert torch.equal(gxa, gx) and (gc is None or torch.equal(gca, gc))
    gx1, gc1, _, _ = run_case(case, weight=torch.ones(case.B))       # NULL weights are ones
    assert torch.equal(gx1, gx) and (gc is None or torch.equal(gc1, gc))
    B = case.B
    rows = slice(B // 3, B // 3 + max(1, B // 2))
    gxs, gcs, _, _ = run_case(case, rows=rows)
    assert torch.equal(gxs, gx[rows]) and (gc is None or torch.equal(gcs, gc[rows]))
    if gc is not None:                                                # no conditional output: grad_x does not move
        gxn, gcn, _, _ = run_case(case, want_cond=False)
        assert gcn is None and torch.equal(gxn, gx)


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
def _front_case(kind, D, C, width, nh, gain, B, seed=71):
    front, ref_kw = make_front(kind, D, C, width, nh, affine=True, gain=gain)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    c = torch.randn(B, C, generator=g) if C else None
    return front.to(DEV), ref_kw, x, c


def _check(what, got, r64, r32):
    err, floor = R.normalised_error(got, r64), fp32_floor(r32, r64)
    print(f"\n[logp_grad] {what}: err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors)")
    assert err <= FACTOR * floor, (what, err, floor)


def test_score_model_log_p_is_log_prob_bitwise_and_the_gradient_is_that_of_its_probes(monkeypatch):
    D, C, B = 5, 2, 21
    front, ref_kw, x, c = _front_case("vp", D, C, 128, 2, 2.0, B)
    front.hutch = True
    kw = dict(method="rk4", options=options_of(front, "to_base", 3), probe="philox", seed=11)
    lp, gx, gc = front.log_prob_grad(_dev(x), _dev(c), **kw)
    e = front.e.clone()
    assert lp.shape == (B, 1) and gx.shape == (B, D) and gc.shape == (B, C)
    assert torch.equal(lp, front.log_prob(_dev(x), _dev(c), **kw)) and torch.equal(front.e, e)
    refs = {dt: LG.LogDensity(R.SolverMap(direction="to_base", method="rk4", options=kw["options"], dtype=dt, **ref_kw))
            for dt in (torch.float32, torch.float64)}
    (lp64, gx64, gc64), (_, gx32, gc32) = (refs[dt](x, c, e[:, None], 1.0) for dt in (torch.float64, torch.float32))
    assert float((lp.cpu().double()[:, 0] - lp64).abs().max()) <= 1e-4 * float(lp64.abs().max().clamp_min(1.0))
    _check("ScoreModel grad_x", gx, gx64, gx32)
    _check("ScoreModel grad_c", gc, gc64, gc32)
    # a re-run, a batch slice (philox probes are keyed by the global row) and any cut of the rows: bitwise
    again = front.log_prob_grad(_dev(x), _dev(c), **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, (lp, gx, gc)))
    part = front.log_prob_grad(_dev(x[5:14]), _dev(c[5:14]), sample_offset=5, **kw)
    assert all(torch.equal(a, b[5:14]) for a, b in zip(part, (lp, gx, gc)))
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 3 * 12 * D + 1)          # twelve evaluation rows: three points per piece
    cut = front.log_prob_grad(_dev(x), _dev(c), **kw)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(cut[1:], (gx, gc)))


def test_three_probes_are_the_weighted_sum_of_three_single_probe_calls():
    """K = 3 probes with weight 1 / 3 each = the mean of the three single-probe gradients (every one of which carries the whole
    prior term), to rounding; and both are the float64 reference's."""
    D, C, B, K = 16, 1, 9, 3
    front, ref_kw, x, c = _front_case("flow", D, C, 128, 2, 6.0, B)
    method, opts = "rk4", {"step_size": 0.5}
    torch.manual_seed(3)
    probes = torch.sign(torch.randn(B, K, D))
    xn, cn = (_dev(x) - front.target_shift) / front.target_scale, front._norm_cond(_dev(c))
    t_span = torch.tensor([0.0, 1.0])
    _, gx3, gc3 = odeint.solve_logp_grad(front, xn, t_span, method, opts, _dev(probes), 1.0 / K, cond=cn)
    parts = [odeint.solve_logp_grad(front, xn, t_span, method, opts, _dev(probes[:, k:k + 1]), 1.0, cond=cn) for k in range(K)]
    mx, mc = sum(p[1] for p in parts) / K, sum(p[2] for p in parts) / K
    refs = {dt: LG.LogDensity(R.SolverMap(direction="to_base", method=method, options=opts, dtype=dt, **ref_kw))
            for dt in (torch.float32, torch.float64)}
    (_, gx64, gc64), (_, gx32, gc32) = (refs[dt](x, c, probes, 1.0 / K) for dt in (torch.float64, torch.float32))
    # (the reference works in the user's units, the solve above in the normalised ones: the chain rule's factors)
    _check("K = 3 grad_x", gx3 / front.target_scale, gx64, gx32)
    _check("K = 3 grad_c", gc3 / front.conditional_scale, gc64, gc32)
    assert R.normalised_error(mx, gx3) <= FACTOR * fp32_floor(gx32, gx64)
    assert R.normalised_error(mc, gc3) <= FACTOR * fp32_floor(gc32, gc64)
    # the front end with num_probes = 3: log_p is log_prob's under the same torch seed, bit for bit
    kw = dict(method=method, options=opts, hutchinson=True, num_probes=K)
    torch.manual_seed(9)
    lp, gx, gc = front.log_prob_grad(_dev(x), _dev(c), **kw)
    torch.manual_seed(9)
    assert torch.equal(lp[:, 0], front.log_prob(_dev(x), _dev(c), **kw))
    torch.manual_seed(9)
    e = torch.sign(torch.randn(B, K, D))                  # (the draw of ``solve_hutchinson``)
    (_, fx64, fc64), (_, fx32, fc32) = (refs[dt](x, c, e, 1.0 / K) for dt in (torch.float64, torch.float32))
    _check("num_probes = 3 grad_x", gx, fx64, fx32)
    _check("num_probes = 3 grad_c", gc, fc64, fc32)


@pytest.mark.parametrize("kind, D, C", [("flow", 17, 0), ("vp", 4, 16)])
def test_exact_trace_model_against_the_reference_with_unit_probes(kind, D, C):
    B = 9
    # (a VP model's fp32 floor is small at three steps and a moderate gain: the module's docstring)
    front, ref_kw, x, c = _front_case(kind, D, C, 256 if D > 16 else 128, 2, 6.0 if kind == "flow" else 2.0, B)
    method, opts = "dopri5_fixed", options_of(front, "to_base", 1 if kind == "flow" else 3)
    args = (_dev(x),) + (() if c is None else (_dev(c),))
    if kind == "flow":
        lp, gx, gc = front.log_prob_grad(*args, method=method, options=opts)
        assert torch.equal(lp[:, 0], front.log_prob(*args, method=method, options=opts))
    else:
        lp, gx, gc = front.log_prob_grad(*args, method=method, options=opts)
        assert torch.equal(lp, front.log_prob(*args, method=method, options=opts))
    refs = {dt: LG.LogDensity(R.SolverMap(direction="to_base", method=method, options=opts, dtype=dt, **ref_kw))
            for dt in (torch.float32, torch.float64)}
    eye = torch.eye(D).expand(B, D, D)
    (lp64, gx64, gc64), (_, gx32, gc32) = (refs[dt](x, c, eye, 1.0) for dt in (torch.float64, torch.float32))
    assert float((lp.cpu().double()[:, 0] - lp64).abs().max()) <= 1e-4 * float(lp64.abs().max().clamp_min(1.0))
    _check(f"exact trace {kind} grad_x", gx, gx64, gx32)
    if C:
        _check(f"exact trace {kind} grad_c", gc, gc64, gc32)
    else:
        assert gc is None


def test_population_wrappers_apply_the_chain_rule():
    torch.manual_seed(21)
    D, C, B = 5, 3, 9
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=[128, 128])
    DM.apply_gain(list(m.NN), 2.0)
    shift, scale = torch.linspace(-0.5, 0.5, D), torch.linspace(0.5, 1.5, D)
    cshift, cscale = torch.linspace(0.2, -0.2, C), torch.linspace(0.7, 1.9, C)
    pm = Dm.PopulationModelDiffusionConditional(model=m, sde=Dm.VPSDE(), shift=shift, scale=scale, conditional_shift=cshift,
                                                conditional_scale=cscale, method="rk4").to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    x, c = torch.randn(B, D, generator=g), torch.randn(B, C, generator=g)
    opts = options_of(pm.score_model, "to_base", 3)
    lp, gx, gc = pm.log_prob_grad(_dev(x), _dev(c), method="rk4", options=opts)
    refs = {dt: LG.LogDensity(R.SolverMap("score", R.score_params(m), "to_base", "rk4", opts, dtype=dt, sde="vp",
                                          affine=(shift, scale), cond_affine=(cshift, cscale)))
            for dt in (torch.float32, torch.float64)}
    eye = torch.eye(D).expand(B, D, D)
    (lp64, gx64, gc64), (_, gx32, gc32) = (refs[dt](x, c, eye, 1.0) for dt in (torch.float64, torch.float32))
    assert lp.shape == (B, 1)
    assert float((lp.cpu().double()[:, 0] - lp64).abs().max()) <= 1e-4 * float(lp64.abs().max().clamp_min(1.0))
    _check("conditional wrapper grad_x", gx, gx64, gx32)
    _check("conditional wrapper grad_c", gc, gc64, gc32)
    # the unconditional wrapper on a VE model with a Hutchinson probe: the prior is N(0, sigma_max^2)
    torch.manual_seed(22)
    mu = Dm.MLP(n_dimensions=D, n_conditionals=0, embedding_dimensions=8, units=[128, 128])
    DM.apply_gain(list(mu.NN), 2.0)
    pu = Dm.PopulationModelDiffusion(model=mu, sde=Dm.VESDE(), shift=shift, scale=scale, method="rk4", hutchinson=True).to(DEV).eval()
    optu = options_of(pu.score_model, "to_base", 3)
    lpu, gu, none = pu.log_prob_grad(_dev(x), method="rk4", options=optu, probe="philox", seed=4)
    assert none is None
    e = pu.score_model.e.clone()
    refu = {dt: LG.LogDensity(R.SolverMap("score", R.score_params(mu), "to_base", "rk4", optu, dtype=dt, sde="ve",
                                          affine=(shift, scale))) for dt in (torch.float32, torch.float64)}
    (_, gu64, _), (_, gu32, _) = (refu[dt](x, None, e[:, None], 1.0) for dt in (torch.float64, torch.float32))
    _check("unconditional VE wrapper grad_x", gu, gu64, gu32)
