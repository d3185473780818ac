"""GPU tier of the Hutch++ / XTrace products route (csrc/ff_mlp_vjp.hpp, ff_mlp_ode_launch_vjp, csrc/ff_trace_prod.hip,
``products="vjp"``): raw launches of the three products units between guard words on NaN-prefilled outputs against the
float64 reference (tests/_estimator_products_ref.py: the table's rows stepped with the kernel's slot semantics, reverse-mode
products of the oracle's drift at every stage state), the bitwise structure of the launch, the products against the
Jacobians the library already records, the two streaming kernels against their host twins and the float64 torch statement,
and the front end against the reference's fixtures.

Tolerance: the push-forward tests' rule and factor (tests/test_gpu_pushforward.py).  Per case the reference runs twice on the
CPU, in fp32 and in float64; the fp32 run's error per sample, normalised by the sample's largest reference entry over the
launch, is the case's fp32 floor, as measured, and the bar is that floor times FACTOR = 22.  profiles/estimator_products.txt
lists the floors and the device's errors.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers, trace_estimators as TE
from flowfusion_amd import diffusion as Dm
from flowfusion_amd.fused import exact_trace_passes
from oracle import flowfusion_oracle as fo
from tests import _estimator_products_ref as EP
from tests import _pushforward_ref as R
from tests._util import load_golden, max_rel, score_model
from tests.test_gpu_pushforward import FACTOR, GUARD, SDE, _guarded, _payload, fp32_floor
from tests.test_trace_estimators import well_posed

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


# ---- models, inputs, the reference ---------------------------------------------------------------------------------------------
SHAPES = {"h128_d4": (5, 3, [64, 100]), "h256_d4": (16, 0, [256] * 4), "h256_d8": (32, 8, [96, 96])}


def make_model(unit, sde, no_sigma, seed=5):
    """(ScoreModel on the CPU, dtype -> drift(t, y, cond) of the oracle) of a seeded model of the unit's shape."""
    D, C, units = SHAPES[unit]
    torch.manual_seed(seed)
    m = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=units)
    sm = Dm.ScoreModel(m, getattr(Dm, SDE[sde])(), no_sigma=no_sigma).eval()
    params = R.score_params(m)
    oracle = lambda dt: fo.ScoreOracle(params, R.SDES[sde](dtype=dt), no_sigma=no_sigma, dtype=dt)
    return sm, oracle


def grid_of(sm, method, nsteps):
    eps = float(sm.sde.epsilon)
    span = torch.tensor([eps, 1.0], dtype=torch.float32)
    opts = {"step_size": float(span[1] - span[0]) / nsteps}
    return span, opts, solvers.plan_ode(span, method, opts)


def inputs(unit, B, K, n, per_row, seed=31):
    D, C, _ = SHAPES[unit]
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * D + K)
    x = torch.randn(B, D, generator=g)
    c = torch.randn(B, C, generator=g) if C else None
    seeds = torch.randn(*((n, B, K, D) if per_row else (B, K, D)), generator=g)
    return x, c, seeds


def reference(oracle, plan, x, c, seeds, per_row, dt):
    o = oracle(dt)
    cc = None if c is None else c.to(dt)
    xo, prod, _ = EP.table_products(lambda t, y: o.ode_drift(t, y, cc), plan, x.to(dt), seeds.to(dt), per_row)
    return xo, prod


def per_sample(prod):
    """[n, B, K, D] -> [B, n, K, D]: the normalisation runs over everything a sample's launch wrote."""
    return prod.permute(1, 0, 2, 3)


# ---- the raw launch, between guard words -------------------------------------------------------------------------------------
def raw_vjp(sm, plan_rows, method, x, seeds, per_row, cond=None, noise_row=None, status_is=0, slots=None):
    """ff_mlp_ode_launch_vjp on buffers of the test's own over the forward table of ``plan_rows``: (x_out [B, D],
    prod [n, B, K, D], the kernel's name), guards checked.  ``noise_row``: that row gets the FF_ROW_NOISE flag;
    ``slots``: the stage slots kept in LDS (default: the method's stages)."""
    net = sm.to(DEV)._net()
    plan = net.pull_plan()
    table = solvers.build_table(plan_rows, *sm._host_schedule()(plan_rows.t_eval), int(plan.width))
    if noise_row is not None:
        table.view(torch.int32)[noise_row, solvers.ROW_FLAGS] |= solvers.FLAG_NOISE
    table = table.to(DEV)
    wp = net.wpack(torch.device(DEV), _native.MODE_HUTCH, plan)
    x, seeds, cond = _dev(x), _dev(seeds), _dev(cond)
    B, D = x.shape
    K, n = seeds.shape[-2], table.shape[0]
    assert tuple(seeds.shape) == ((n, B, K, D) if per_row else (B, K, D))
    xo, prod = _guarded(B * D), _guarded(n * B * K * D)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab, a.status = x.data_ptr(), xo.data_ptr() + 4 * GUARD, wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if cond is None else cond.data_ptr()
    a.batch, a.n_evals, a.tangent_count, a.mode = B, n, K, _native.MODE_HUTCH
    a.stage_slots = solvers.resolve_method(method).stages if slots is None else slots
    rc = _native.lib().ff_mlp_ode_launch_vjp(ctypes.byref(plan), ctypes.byref(a), seeds.data_ptr(), B * K * D if per_row else 0,
                                             prod.data_ptr() + 4 * GUARD, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == status_is
    name = _native.lib().ff_vjp_kernel_name(int(plan.kernel_id) - _native.PULL_KERNEL_BASE).decode()
    return _payload(xo, (B, D)).cpu(), _payload(prod, (n, B, K, D)).cpu(), name


# (unit, sde, no_sigma, K, B, method, steps, seeds per row): every unit, VP with sigma / VP no_sigma / VE, B = 37 and 1 (ragged
# tiles), K = 1, 2, 4, 15 (8 / 5 / 3 / 1 samples per tile; dead columns at K = 2, 4), euler / rk4 / dopri5_fixed (all seven
# slots), both seed_row_stride forms
RAW_CASES = [
    ("h128_d4", "vp", False, 1, 37, "rk4", 3, False),
    ("h128_d4", "vp", True, 2, 1, "euler", 2, True),
    ("h128_d4", "ve", False, 15, 37, "dopri5_fixed", 2, True),
    ("h256_d4", "vp", False, 4, 37, "dopri5_fixed", 2, False),
    ("h256_d4", "ve", False, 1, 1, "rk4", 3, True),
    ("h256_d4", "vp", True, 15, 37, "euler", 2, False),
    ("h256_d8", "vp", False, 2, 37, "rk4", 3, True),
    ("h256_d8", "vp", True, 4, 1, "dopri5_fixed", 2, False),
    ("h256_d8", "ve", False, 1, 37, "euler", 2, True),
]


def _id(case):
    return "-".join(str(p) for p in case)


def case_setup(case):
    unit, sde, no_sigma, K, B, method, nsteps, per_row = case
    sm, oracle = make_model(unit, sde, no_sigma)
    span, opts, plan = grid_of(sm, method, nsteps)
    x, c, seeds = inputs(unit, B, K, int(plan.t_eval.numel()), per_row)
    return sm, oracle, plan, method, x, c, seeds, per_row


@pytest.mark.parametrize("case", RAW_CASES, ids=_id)
def test_raw_launch_against_float64_reference(case):
    sm, oracle, plan, method, x, c, seeds, per_row = case_setup(case)
    xo, prod, name = raw_vjp(sm, plan, method, x, seeds, per_row, cond=c)
    assert name == f"mlp_vjp_m16_{case[0]}_c4", name               # the unit the case is meant for
    x64, p64 = reference(oracle, plan, x, c, seeds, per_row, torch.float64)
    x32, p32 = reference(oracle, plan, x, c, seeds, per_row, torch.float32)
    line, worst = f"\n[estimator_products] {_id(case)}:", []
    for what, got, r64, r32 in (("x_out", xo, x64, x32), ("prod", per_sample(prod), per_sample(p64), per_sample(p32))):
        floor, err = fp32_floor(r32, r64), R.normalised_error(got, r64)
        line += f" {what} err {err:.3e} floor {floor:.3e};"
        worst.append((what, err, floor))
    print(line)
    for what, err, floor in worst:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


# ---- the structure of the launch, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (0, 3, 6)], ids=_id)
def test_state_ignores_the_seeds_columns_are_independent_and_reruns_are_bitwise(case):
    unit, sde, no_sigma, K, B, method, nsteps, per_row = case
    sm, oracle, plan, method, x, c, _, _ = case_setup(case)
    n = int(plan.t_eval.numel())
    _, _, flat = inputs(unit, B, 4, n, False, seed=41)              # [B, 4, D]
    _, _, rows = inputs(unit, B, 4, n, True, seed=43)               # [n, B, 4, D]
    xo, prod, _ = raw_vjp(sm, plan, method, x, flat, False, cond=c)
    again = raw_vjp(sm, plan, method, x, flat, False, cond=c)
    assert torch.equal(again[0], xo) and torch.equal(again[1], prod)                       # a re-run
    # the state: bitwise independent of K, of the seeds and of the form they come in (a sweep-1- and a sweep-2-shaped launch)
    xr, prod_rows, _ = raw_vjp(sm, plan, method, x, rows, True, cond=c)
    assert torch.equal(xr, xo) and not torch.equal(prod_rows, prod)
    for k_other in (1, 2, 15):
        _, _, other = inputs(unit, B, k_other, n, False, seed=47)
        assert torch.equal(raw_vjp(sm, plan, method, x, other, False, cond=c)[0], xo), k_other
    # column k of a K-launch is the single-column launch of that seed
    for k in (0, 3):
        x1, p1, _ = raw_vjp(sm, plan, method, x, flat[:, k:k + 1].contiguous(), False, cond=c)
        assert torch.equal(x1, xo) and torch.equal(p1[:, :, 0], prod[:, :, k]), k
        x1, p1, _ = raw_vjp(sm, plan, method, x, rows[:, :, k:k + 1].contiguous(), True, cond=c)
        assert torch.equal(p1[:, :, 0], prod_rows[:, :, k]), k
    # zero seeds give exact zeros
    x0, p0, _ = raw_vjp(sm, plan, method, x, torch.zeros_like(flat), False, cond=c)
    assert torch.equal(x0, xo) and bool((p0 == 0).all())
    # seed_row_stride = 0 is the per-row form with the seeds repeated
    xs, ps, _ = raw_vjp(sm, plan, method, x, flat.unsqueeze(0).expand(n, *flat.shape).contiguous(), True, cond=c)
    assert torch.equal(xs, xo) and torch.equal(ps, prod)


def test_a_noise_row_is_left_out_and_reported_in_the_status_word():
    case = RAW_CASES[0]
    sm, oracle, plan, method, x, c, seeds, per_row = case_setup(case)
    xo, prod, _ = raw_vjp(sm, plan, method, x, seeds, per_row, cond=c)
    for row in (0, 7):                                       # a stage row and a step-end row (rk4: rows 3, 7, 11 end a step)
        xn, pn, _ = raw_vjp(sm, plan, method, x, seeds, per_row, cond=c, noise_row=row, status_is=_native.STATUS_NOISE_ROW)
        assert torch.equal(xn, xo) and torch.equal(pn, prod)


# ---- against the Jacobian the library already records ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RAW_CASES[i] for i in (0, 3, 6)], ids=_id)
def test_products_are_the_recorded_jacobian_times_the_seeds(case):
    """prod[e, b, k] against A[e, b] seed with A from ``mlp_ode_jacobians`` on the same grid.  Bar: the sum of the two routes'
    fp32 floors -- the products', and that of A seed with A from the fp32 / float64 reference's unit-seed products -- x FACTOR."""
    unit, sde, no_sigma, K, B, method, nsteps, _ = case
    sm, oracle, plan, method, x, c, _, _ = case_setup(case)
    D = x.shape[1]
    n = int(plan.t_eval.numel())
    _, _, seeds = inputs(unit, B, K, n, False)
    _, prod, _ = raw_vjp(sm, plan, method, x, seeds, False, cond=c)
    net = sm.to(DEV)._net()
    eplan = net.plan(_native.MODE_EXACT)
    span, opts, _ = grid_of(sm, method, nsteps)
    table = sm._ode_table(span, method, opts, _native.MODE_EXACT).to(DEV)
    jac = torch.empty(n, B, D, D, dtype=torch.float32, device=DEV)
    for first, count in exact_trace_passes(D, eplan.tile):
        torch.ops.flowfusion_amd.mlp_ode_jacobians(_dev(x), _dev(c), net.wpack(torch.device(DEV), _native.MODE_EXACT), table,
                                                   _native.plan_words(eplan), first, count, jac)
    times = lambda A, s: torch.einsum("ebji,bki->ebkj", A.double(), s.double())
    got = times(jac.cpu(), seeds)
    eye = torch.eye(D).unsqueeze(0).expand(B, D, D).contiguous()
    refs = {}
    for dt in (torch.float32, torch.float64):
        _, p = reference(oracle, plan, x, c, seeds, False, dt)
        _, A = reference(oracle, plan, x, c, eye, False, dt)            # A[e, b, j, :] = J^T e_j
        refs[dt] = (p, torch.einsum("ebji,bki->ebkj", A, seeds.to(dt)))
    floor_p = fp32_floor(per_sample(refs[torch.float32][0]), per_sample(refs[torch.float64][0]))
    floor_j = fp32_floor(per_sample(refs[torch.float32][1]), per_sample(refs[torch.float64][1]))
    err = R.normalised_error(per_sample(prod), per_sample(got))
    print(f"\n[estimator_products] {_id(case)} against the recorded Jacobian: err {err:.3e} floors {floor_p:.3e} + {floor_j:.3e}")
    assert err <= FACTOR * (floor_p + floor_j), (err, floor_p, floor_j)


# ---- the streaming kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, r, m, B, n", [(16, 1, 1, 300, 6), (5, 2, 3, 77, 2), (32, 3, 2, 65, 1), (8, 3, 2, 100, 3)])
def test_basis_and_combine_kernels_against_their_host_twins_and_the_torch_statement(D, r, m, B, n):
    """ff_trace_basis / ff_trace_combine on the device: random Jacobians, products computed in float64 and rounded, against
    the host twins and against trace_estimators.py in float64 at the bar of
    test_trace_estimate_kernel_against_the_torch_statement, 2e-6 x scale.  B is no multiple of 64 and the items span the
    rows.  Probes: seed 23, +-1 by coin flips."""
    g = torch.Generator().manual_seed(23)
    S = torch.randint(0, 2, (r, B, D), generator=g).float() * 2 - 1
    G = torch.randint(0, 2, (m, B, D), generator=g).float() * 2 - 1
    A = torch.randn(n, B, D, D, generator=g)
    ok1 = well_posed(S)
    if D >= 8:
        assert bool(ok1.all())
    else:
        assert int(ok1.sum()) * 3 >= 2 * B
    ok = ok1.repeat(n)
    A64 = A.double()
    times = lambda V: torch.einsum("ebik,ebck->ebci", A64, V.double()).float()              # [n, B, K, D] -> A V, rounded
    rep = lambda P: P.unsqueeze(1).expand(P.shape[0], n, B, D).reshape(P.shape[0], n * B, D).double()
    scale = max(1.0, float(A.abs().sum(dim=(2, 3)).max()))
    flat = A64.reshape(n * B, D, D)
    P = S.permute(1, 0, 2).unsqueeze(0).expand(n, B, r, D)
    Y = times(P)
    for kind, probes, want, bar in (("hutchpp", (S, G), TE.hutchpp(flat, rep(S), rep(G)), 2e-6 * scale),
                                    ("xtrace", (S,), TE.xtrace(flat, rep(S)), 2e-6 * scale * max(1, r))):
        hb, hr = _native.trace_basis(Y, kind, probes, host=True)
        db, dr = _native.trace_basis(Y.to(DEV), kind, tuple(p.to(DEV) for p in probes))
        torch.cuda.synchronize()
        assert db.shape == hb.shape and ((dr is None) == (hr is None))
        assert float((db.cpu() - hb)[ok.view(n, B)].abs().max()) <= bar, kind
        host = _native.trace_combine(hb, hr, times(hb), kind, probes, host=True).reshape(-1).double()
        dev = _native.trace_combine(db, dr, times(db.cpu()).to(DEV), kind, tuple(p.to(DEV) for p in probes))
        dev = dev.cpu().reshape(-1).double()
        e_host, e_ref, h_ref = (float(v[ok].abs().max()) for v in (dev - host, dev - want, host - want))
        print(f"\n[estimator_products] streaming {kind} D={D} r={r} m={m} B={B} n={n}: device-host {e_host:.3e} device-f64 {e_ref:.3e} "
              f"host-f64 {h_ref:.3e} bar {bar:.3e}")
        assert e_host <= bar and e_ref <= bar and h_ref <= bar, (kind, e_host, e_ref, h_ref, bar)


# ---- the front end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trace_vp_nosigma_16d", "trace_vp_sigma_cond", "trace_ve_nosigma_cond32"])
def test_log_prob_with_products_against_reference_fixtures(name, monkeypatch):
    """log_prob(..., method="rk4", products="vjp") with the fixture's probes (the draw is intercepted) against the
    log-densities the reference's forward produced under the oracle's RK4, at the bar of
    test_hutchpp_and_xtrace_log_prob_against_reference_fixtures -- and products="jacobian" beside it, same bar."""
    meta, a = load_golden(name)
    x, cond = a["x"].to(DEV), (a["cond"].to(DEV) if "cond" in a else None)
    opts = {"step_size": meta["step_size"]}
    for kind, kw, probes, want in (("hutchpp", dict(hutchpp=True, hpp_rank=meta["hpp_rank"], hpp_vecs=meta["hpp_vecs"]),
                                    [a["S"], a["G"]], a["lp_hpp_rk4"]),
                                   ("xtrace", dict(xtrace=True, xt_vecs=meta["xt_vecs"]), [a["O"]], a["lp_xt_rk4"])):
        sm = score_model(meta, a, DEV, **kw)
        ok = well_posed(probes[0])
        for route in ("vjp", "jacobian"):
            queue = [p.to(DEV) for p in probes]
            monkeypatch.setattr(TE, "draw_probes", lambda n, like: queue.pop(0))
            lp = sm.log_prob(x, conditional=cond, method="rk4", options=opts, products=route)
            assert not queue and lp.shape == (x.shape[0], 1)
            err = max_rel(lp.cpu()[ok], want[ok], floor=1.0)
            print(f"\n[estimator_products] {name} {kind} products={route}: err {err:.3e}")
            assert err < 5e-5, (name, kind, route, err)
        with pytest.raises(ValueError, match="adaptive"):
            sm.log_prob(x, conditional=cond, products="vjp")                       # default arguments: adaptive dopri5


def test_philox_probes_chunks_and_halves_are_bitwise(monkeypatch):
    meta, a = load_golden("trace_vp_sigma_cond")
    x, cond = a["x"].to(DEV), a["cond"].to(DEV)
    kw = dict(method="rk4", options={"step_size": meta["step_size"]}, products="vjp", probe="philox", seed=77)
    for mk in (dict(hutchpp=True, hpp_rank=2, hpp_vecs=3), dict(xtrace=True, xt_vecs=3)):
        sm = score_model(meta, a, DEV, **mk)
        whole = sm.log_prob(x, conditional=cond, **kw)
        again = sm.log_prob(x, conditional=cond, **kw)
        bits = lambda t: t.view(torch.int32)
        assert torch.equal(bits(whole), bits(again))
        # a chunk budget of three samples: four chunks
        n = solvers.plan_ode(torch.tensor([float(sm.sde.epsilon), 1.0]), "rk4", kw["options"]).t_eval.numel()
        K1, K2 = (2, 5) if "hutchpp" in mk else (3, 3)
        calls = []
        orig = sm._net().vjp_products
        monkeypatch.setattr(sm._net(), "vjp_products", lambda xx, *p, **k: (calls.append(xx.shape[0]), orig(xx, *p, **k))[1])
        monkeypatch.setattr(odeint, "ESTIMATOR_MIN_BYTES", 3 * n * (K1 + 2 * K2) * x.shape[1] * 4)
        monkeypatch.setattr(odeint, "_estimator_budget", lambda device: 0)
        cut = sm.log_prob(x, conditional=cond, **kw)
        monkeypatch.undo()
        assert calls == [3, 3, 3, 3, 3, 3, 1, 1] and torch.equal(bits(cut), bits(whole))
        # the batch in two halves, the second keyed by its global rows
        lo = sm.log_prob(x[:4], conditional=cond[:4], **kw)
        hi = sm.log_prob(x[4:], conditional=cond[4:], **dict(kw, sample_offset=4))
        assert torch.equal(bits(torch.cat([lo, hi])), bits(whole))


def test_full_rank_hutchpp_from_products_is_the_exact_trace():
    meta, a = load_golden("trace_vp_sigma_cond")
    assert meta["D"] == 5
    x, cond = a["x"].to(DEV), a["cond"].to(DEV)
    kw = dict(method="rk4", options={"step_size": meta["step_size"]})
    sm = score_model(meta, a, DEV, hutchpp=True, hpp_rank=meta["D"], hpp_vecs=1)
    lp_pp = sm.log_prob(x, conditional=cond, products="vjp", **kw)
    sm.hutchpp = False
    lp_exact = sm.log_prob(x, conditional=cond, **kw)
    # rank = D: the sketch spans everything, the estimate IS the trace
    assert max_rel(lp_pp.cpu(), lp_exact.cpu(), floor=1.0) < 2e-3
