"""CPU tier of ``log_prob_noisy_grad`` (csrc/ff_observe.hip: ff_observe_keep, ff_observe_grad_reduce; odeint.log_prob_noisy_grad):
the host twins of the two kernels against a float64 numpy restatement (tests/_observe_grad_ref.py) to one fp32 ulp -- double
sums rounded once can differ only at a rounding tie --, degenerate points, the keep rule at ``min_weight`` = 0 and with a weight
exactly on the threshold, the C entry points' refusals, every refusal of the five front ends, and, for every front-end case of
tests/test_gpu_observe_grad.py, the conditions that make a pass on the device mean something:

* the fp32 floor of grad_x, grad_c and grad_noise_std is at most 5e-5;
* every point has 1.5 <= ess <= K - 0.5: the weights are neither uniform nor one-hot;
* a wrong reference with uniform weights 1 / K misses the bar (22 floors) by at least 100x;
* a wrong reference that drops the z_k factor from grad_noise_std misses it by at least 100x;
* in the cut-off case at least a third of the draws fall below ``min_weight`` = 1e-3.
"""
import ctypes
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd import symplectic as S
from tests import _observe_grad_ref as OG
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import FACTOR, fp32_floor

ROOT = Path(__file__).resolve().parents[1]
OK, BAD = _native.FF_OK, _native.FF_ERR_BADARG
FRONTS = (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional)
CAP = 5e-5
NB = 37
GRID = [(K, Dd, C, per_point) for K in (1, 3, 16, 65, 130) for Dd in (1, 5, 16, 32) for C in (0, 3) for per_point in (True, False)]


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


def ulps(got, ref64):
    """max |got - ref| in units of the fp32 spacing at the reference (NaN must meet NaN)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert (np.isnan(got) == np.isnan(ref64)).all()
    ok = ~np.isnan(ref64)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - ref64[ok]) / np.spacing(np.abs(ref64[ok]).astype(np.float32)).astype(np.float64)).max())


def raw_inputs(K, Dd, C, per_point, seed=0, spread=3.0, min_weight=1e-3):
    """(lp [NB K], keep, row_of, gx_rows [n, D], gc_rows [n, C] or None, noise_std) of one cell of the kernels' grid: log-weights
    wide enough that some draws fall below ``min_weight``, a -inf among them."""
    g = torch.Generator().manual_seed(seed + 1000 * K + 10 * Dd + C)
    lp = spread * torch.randn(NB * K, generator=g)
    if K > 1:
        lp[K + 1] = float("-inf")
    keep = torch.from_numpy(OG.keep64(lp.numpy(), K, min_weight))
    rows, n = OG.row_of(keep), int(keep.sum())
    gx = torch.randn(n, Dd, generator=g)
    gc = torch.randn(n, C, generator=g) if C else None
    std = torch.rand(NB, Dd, generator=g) if per_point else torch.rand(Dd, generator=g)
    return lp, keep, rows, gx, gc, std


# ---- the kernels' host twins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, Dd, C, per_point", GRID)
def test_grad_reduce_host_is_the_float64_restatement_to_one_ulp(K, Dd, C, per_point):
    lp, keep, rows, gx, gc, std = raw_inputs(K, Dd, C, per_point)
    assert 0 < int(keep.sum()) and (K < 16 or int(keep.sum()) < NB * K)         # some rows are skipped
    got = _native.observe_grad_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET)
    z = OG.draws(OG.SEED, OG.OFFSET, NB, Dd, K).numpy()
    ref = OG.grad_reduce64(lp.numpy(), rows.numpy(), gx.numpy(), None if gc is None else gc.numpy(), K, z)
    assert got[0].shape == (NB, Dd) and got[2].shape == (NB, Dd) and (got[1] is None) == (C == 0)
    for what, a, b in zip(("grad_x", "grad_c", "grad_noise_std"), got, ref):
        if b is not None:
            assert ulps(a.numpy(), b) <= 1.0, (what, ulps(a.numpy(), b))
    # without the noise gradient the other two do not move; the layout of noise_std changes nothing
    gx2, gc2, none = _native.observe_grad_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET, want_noise_grad=False)
    assert none is None and torch.equal(gx2, got[0]) and (gc is None or torch.equal(gc2, got[1]))


def test_a_point_is_fixed_by_its_own_data():
    """Any cut of the batch at its sample_offset: bitwise (the host twin; the device's is tests/test_gpu_observe_grad.py)."""
    K, Dd, C = 16, 5, 3
    lp, keep, rows, gx, gc, std = raw_inputs(K, Dd, C, True)
    whole = _native.observe_grad_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET)
    lo, hi = 11, 22
    first = int(rows[:lo * K].max()) + 1
    part_rows = torch.where(rows[lo * K:hi * K] >= 0, rows[lo * K:hi * K] - first, -1).to(torch.int32).contiguous()
    n = int(part_rows.max()) + 1
    part = _native.observe_grad_reduce(lp[lo * K:hi * K].contiguous(), part_rows, gx[first:first + n].contiguous(),
                                       gc[first:first + n].contiguous(), std[lo:hi].contiguous(), K, OG.SEED, OG.OFFSET + lo)
    assert all(torch.equal(a, b[lo:hi]) for a, b in zip(part, whole))


def test_degenerate_points_have_nan_gradients_and_a_lone_minus_inf_is_not_read():
    K, Dd, C = 4, 5, 3
    inf, nan = float("inf"), float("nan")
    lp = torch.tensor([[0.0, nan, 1.0, 2.0], [0.0, inf, 1.0, 2.0], [-inf] * 4, [0.5, -inf, 1.0, -0.25], [0.0, 0.0, 0.0, 0.0]]).view(-1)
    keep = _native.observe_keep(lp, K, 0.0)
    assert keep.view(5, K).tolist() == [[0] * 4, [0] * 4, [0] * 4, [1, 0, 1, 1], [1] * 4]
    rows = OG.row_of(keep)
    g = torch.Generator().manual_seed(3)
    full_x, full_c = torch.randn(5 * K, Dd, generator=g), torch.randn(5 * K, C, generator=g)
    full_x[3 * K + 1], full_c[3 * K + 1] = nan, inf                           # the row of the lone -inf: never read
    kept = torch.nonzero(keep).view(-1)
    std = torch.rand(Dd, generator=g)
    gx, gc, gs = _native.observe_grad_reduce(lp, rows, full_x[kept], full_c[kept], std, K, 1, 0)
    for t in (gx, gc, gs):
        assert bool(torch.isnan(t[:3]).all()) and bool(torch.isfinite(t[3:]).all())
    z = OG.draws(1, 0, 5, Dd, K).numpy()
    ref = OG.grad_reduce64(lp.numpy(), rows.numpy(), full_x[kept].numpy(), full_c[kept].numpy(), K, z)
    for a, b in zip((gx, gc, gs), ref):
        assert ulps(a.numpy(), b) <= 1.0
    # ... and with every row handed over (row_of = the row itself) the NaN row of zero weight would poison the point
    every = torch.arange(5 * K, dtype=torch.int32)
    bad = _native.observe_grad_reduce(lp, every, full_x, full_c, std, K, 1, 0)[0]
    assert bool(torch.isnan(bad[3]).any())


@pytest.mark.parametrize("K", [1, 3, 16, 65, 130])
def test_keep_host_at_zero_keeps_exactly_the_rows_of_positive_weight(K):
    g = torch.Generator().manual_seed(K)
    lp = 200.0 * torch.randn(NB * K, generator=g)              # exp(lp - max) underflows to 0 in double for many rows
    lp[::7] = float("-inf")
    keep = _native.observe_keep(lp, K, 0.0)
    wn, bad = OG.weights64(lp.numpy(), K)
    want = (wn > 0) & ~bad[:, None]
    assert keep.dtype == torch.int32 and (keep.numpy().reshape(NB, K) == want).all()
    assert K == 1 or 0 < int(keep.sum()) < NB * K


@pytest.mark.parametrize("K", [3, 16, 65, 130])
def test_keep_host_keeps_exactly_the_rows_at_or_above_min_weight(K):
    lp, _, _, _, _, _ = raw_inputs(K, 1, 0, False, spread=4.0)
    for m in (1e-4, 1e-2, 0.3):
        keep = _native.observe_keep(lp, K, m)
        assert (keep.numpy() == OG.keep64(lp.numpy(), K, m)).all(), m
    assert 0 < int(_native.observe_keep(lp, K, 1e-2).sum()) < int(_native.observe_keep(lp, K, 0.0).sum())


def test_a_weight_exactly_on_min_weight_is_kept():
    """Two-valued lp: four draws at one value and the rest at -inf have normalised weights of exactly 1 / 4 in any order of the
    sum; m = 0.25 keeps them, the next double above drops them all."""
    K = 9
    lp = torch.full((3, K), float("-inf"))
    lp[0, [0, 3, 4, 8]] = -1.25
    lp[1, [1, 2, 5, 6]] = 3.5
    lp[2, :5] = 0.0                                            # five draws: 0.2 each, below m
    keep = _native.observe_keep(lp.view(-1), K, 0.25).view(3, K)
    assert keep[0].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 1] and keep[1].tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 0]
    assert keep[2].tolist() == [0] * K
    assert int(_native.observe_keep(lp.view(-1), K, float(np.nextafter(0.25, 1.0))).sum()) == 0
    assert (keep.view(-1).numpy() == OG.keep64(lp.view(-1).numpy(), K, 0.25)).all()


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures_and_refuse_bad_arguments():
    L = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    for proto in ("int ff_observe_keep(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep, void* hip_stream);",
                  "int ff_observe_keep_host(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep);",
                  "int ff_observe_grad_reduce(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows, "
                  "const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed, "
                  "int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std, void* hip_stream);",
                  "int ff_observe_grad_reduce_host(const float* lp, const int32_t* row_of, const float* gx_rows, "
                  "const float* gc_rows, const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, "
                  "int32_t K, uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std);"):
        assert proto in header, proto
    K, Dd, C = 3, 5, 2
    lp, rows = torch.zeros(2 * K), torch.arange(2 * K, dtype=torch.int32)
    gx, gc, std = torch.zeros(2 * K, Dd), torch.zeros(2 * K, C), torch.zeros(Dd)
    ox, oc, os_, keep = torch.zeros(2, Dd), torch.zeros(2, C), torch.zeros(2, Dd), torch.zeros(2 * K, dtype=torch.int32)
    p = lambda t: t.data_ptr()
    kp = lambda **kw: L.ff_observe_keep_host(*[kw.get(n, v) for n, v in
                                               (("lp", p(lp)), ("B", 2), ("K", K), ("m", 0.0), ("keep", p(keep)))])
    assert kp() == OK and kp(B=0) == OK
    for kw in (dict(lp=0), dict(keep=0), dict(B=-1), dict(K=0), dict(K=_native.MAX_OBS_DRAWS + 1), dict(m=-1e-9), dict(m=1.0),
               dict(m=float("nan"))):
        assert kp(**kw) == BAD, kw
    base = (("lp", p(lp)), ("rows", p(rows)), ("gx", p(gx)), ("gc", p(gc)), ("std", p(std)), ("stride", 0), ("B", 2), ("D", Dd),
            ("C", C), ("K", K), ("seed", 1), ("off", 0), ("ox", p(ox)), ("oc", p(oc)), ("os", p(os_)))
    gr = lambda **kw: L.ff_observe_grad_reduce_host(*[kw.get(n, v) for n, v in base])
    assert gr() == OK and gr(B=0) == OK and gr(gc=0, C=0, oc=0) == OK and gr(os=0) == OK
    for kw in (dict(lp=0), dict(rows=0), dict(gx=0), dict(std=0), dict(ox=0), dict(B=-1), dict(D=0), dict(K=0),
               dict(K=_native.MAX_OBS_DRAWS + 1), dict(stride=1), dict(C=0), dict(oc=0)):
        assert gr(**kw) == BAD, kw
    # the device entry points refuse the same before anything is enqueued: no device is needed to ask
    assert L.ff_observe_keep(0, 2, K, 0.0, p(keep), None) == BAD
    assert L.ff_observe_grad_reduce(p(lp), p(rows), p(gx), p(gc), p(std), 1, 2, Dd, C, K, 1, 0, p(ox), p(oc), p(os_), None) == BAD
    assert L.ff_observe_keep(p(lp), 0, K, 0.0, p(keep), None) == OK           # B == 0: FF_OK without a launch
    # the binding's own checks
    with pytest.raises(ValueError, match="min_weight"):
        _native.observe_keep(lp, K, 1.0)
    with pytest.raises(RuntimeError, match="row_of points at row"):
        _native.observe_grad_reduce(lp, rows, gx[:4].contiguous(), None, std, K, 1)


# ---- the conditions on the GPU file's cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OG.CASES, ids=lambda c: c.name)
def test_every_gpu_case_has_a_low_floor_spread_weights_and_tells_wrong_weights_and_a_dropped_z(case):
    r = OG.references(case)
    r64, r32 = r[torch.float64], r[torch.float32]
    ess = r64.ess
    print(f"\n[observe_grad] {case.name}: ess {float(ess.min()):.2f} .. {float(ess.max()):.2f} of K = {case.K}")
    assert float(ess.min()) >= 1.5 and float(ess.max()) <= case.K - 0.5
    # the reference's own identity: autograd through the logsumexp is the weighted sum of the rows' gradients
    assert R.normalised_error((r64.wn[..., None] * r64.g).sum(1), r64.gx) <= 1e-12
    assert R.normalised_error(-(r64.wn[..., None] * r64.z * r64.g).sum(1), r64.gs) <= 1e-12
    uniform = {"gx": r64.g.mean(1), "gs": -(r64.z * r64.g).mean(1), "gc": None if r64.gc is None else r64.h.mean(1)}
    no_z = -(r64.wn[..., None] * r64.g).sum(1)
    for what in ("gx", "gc", "gs"):
        ref = getattr(r64, what)
        if ref is None:
            assert case.C == 0
            continue
        floor = fp32_floor(getattr(r32, what), ref)
        miss = R.normalised_error(uniform[what], ref) / (FACTOR * floor)
        line = f"[observe_grad] {case.name} {what}: floor {floor:.3e}; uniform weights miss the bar by {miss:.0f}x"
        assert floor <= CAP, (what, floor)
        assert miss >= 100.0, (what, miss)
        if what == "gs":
            dropped = R.normalised_error(no_z, ref) / (FACTOR * floor)
            line += f"; without z by {dropped:.0f}x"
            assert dropped >= 100.0, dropped
        print(line)


def test_the_cut_off_case_puts_a_third_of_the_draws_below_min_weight():
    r64 = OG.references(OG.CUT_CASE)[torch.float64]
    below = float((r64.wn < OG.CUT).double().mean())
    print(f"\n[observe_grad] {OG.CUT_CASE.name}: {below:.3f} of the draws below {OG.CUT}")
    assert below >= 1.0 / 3.0


def test_the_cases_are_the_ones_the_issue_names():
    by = {c.name: c for c in OG.CASES}
    assert OG.B == 24 and OG.STEPS == 3
    assert (by["vp_hutch"].D, by["vp_hutch"].C, by["vp_hutch"].K, by["vp_hutch"].P, by["vp_hutch"].width) == (16, 0, 8, 1, (128, 128))
    assert (by["ve_exact"].kind, by["ve_exact"].D, by["ve_exact"].C, by["ve_exact"].K, by["ve_exact"].P) == ("ve", 5, 3, 4, 0)
    c = by["cflow_hutch3"]
    assert (c.kind, c.D, c.C, c.K, c.P) == ("flow", 8, 2, 16, 3) and len(set(c.width)) > 1
    assert {(by[n].wrap, by[n].D, by[n].K) for n in ("pop_hutch", "popc_exact")} == {("pop", 4, 4), ("popc", 4, 4)}


# ---- the front ends' signatures and refusals ----------------------------------------------------------------------------------------
def test_the_five_front_ends_have_the_method_and_the_symplectic_flow_does_not():
    for cls in FRONTS:
        sig = inspect.signature(cls.log_prob_noisy_grad)
        names = list(sig.parameters)
        noisy = list(inspect.signature(cls.log_prob_noisy).parameters)
        prefix = noisy[:noisy.index("num_draws") + 1]
        assert names[:len(prefix)] == prefix, (cls.__name__, names)          # the positional prefix of its log_prob_noisy
        kwonly = {n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
        want = {"method", "options", "seed", "sample_offset", "chunk_points", "num_probes", "min_weight", "return_ess",
                "return_noise_grad"}
        assert want <= kwonly, (cls.__name__, want - kwonly)
        assert ("hutchinson" in kwonly) == (cls in (F.ODEFlow, F.ConditionalODEFlow))
        d = {n: p.default for n, p in sig.parameters.items()}
        assert (d["num_draws"], d["method"], d["options"], d["min_weight"], d["return_ess"], d["return_noise_grad"]) == \
            (16, "rk4", None, 0.0, False, False)
    assert not hasattr(S.SymplecticFlowModel, "log_prob_noisy_grad")


def _fronts():
    """[(front end on the CPU, positional arguments after noise_std)] of the five classes, small."""
    torch.manual_seed(0)
    Dd, C, B = 4, 2, 3
    x, c = torch.randn(B, Dd), torch.randn(B, C)
    mu = D.MLP(n_dimensions=Dd, n_conditionals=0, embedding_dimensions=8, units=[128, 128])
    mc = D.MLP(n_dimensions=Dd, n_conditionals=C, embedding_dimensions=8, units=[128, 128])
    return x, [(D.ScoreModel(mc, D.VPSDE()).eval(), (c,)), (F.ODEFlow(Dd, [128, 128]).eval(), ()),
               (F.ConditionalODEFlow(Dd, C, [128, 128]).eval(), (c,)),
               (D.PopulationModelDiffusion(model=mu, sde=D.VPSDE()).eval(), ()),
               (D.PopulationModelDiffusionConditional(model=mc, sde=D.VPSDE()).eval(), (c,))]


def test_every_refusal_of_the_five_front_ends_names_the_way_out():
    x, fronts = _fronts()
    step = {"step_size": 0.5}
    for front, rest in fronts:
        call = lambda *a, x=x, std=0.1, **kw: front.log_prob_noisy_grad(x, std, *rest, *a, **kw)
        name = type(front).__name__
        for m in (-0.1, 1.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match="0 <= min_weight < 1"):
                call(min_weight=m)
        with pytest.raises(ValueError, match=r"adaptive method='dopri5'.*method=\"rk4\" / \"dopri5_fixed\""):
            call(method="dopri5", options=step)
        for opt in ("grid_constructor", "perturb"):
            with pytest.raises(ValueError, match=r"options=\{\"step_size\": h\}"):
                call(options={opt: (lambda *a: None) if opt == "grid_constructor" else True})
        with pytest.raises(ValueError, match="1 .. 4096 noise draws"):
            call(0, options=step)
        with pytest.raises(ValueError, match="1 .. 4096 noise draws"):
            call(_native.MAX_OBS_DRAWS + 1, options=step)
        with pytest.raises(ValueError, match="at least one data point per chunk"):
            call(options=step, chunk_points=0)
        with pytest.raises(ValueError, match=r"x must be a \[batch, dim\] float32 tensor"):
            call(x=x.double(), options=step)
        with pytest.raises(ValueError, match="num_probes=2 averages Hutchinson probes"):
            call(options=step, num_probes=2)
        # (after the refusals: a CPU tensor cannot be solved -- and nothing above touched a device)
        with pytest.raises(RuntimeError, match="GPU|cuda|device"):
            call(options=step)
        assert getattr(front, "last_noisy_grad_stats", {}) == {}, name       # no call got as far as a launch
    score, (c,) = fronts[0]
    for flag in ("hutchpp", "xtrace"):
        setattr(score, flag, True)
        with pytest.raises(ValueError, match="Hutch\\+\\+ / XTrace model.*hutchinson=True"):
            score.log_prob_noisy_grad(x, 0.1, c, options=step)
        setattr(score, flag, False)
    score.precision = "bf16x2"
    with pytest.raises(ValueError, match="precision='f32'"):
        score.log_prob_noisy_grad(x, 0.1, c, options=step)
    score.precision = "f32"
    with pytest.raises(ValueError, match=r"conditional must be \[3, 2\]"):
        score.log_prob_noisy_grad(x, 0.1, None, options=step)
    with pytest.raises(ValueError, match="no conditional inputs"):
        fronts[1][0]._log_prob_noisy_grad(x, 0.1, c, 4, "rk4", step, False, None, 0, None, 1, 0.0, False, False)
    # a network outside the log-density gradient units: no module-path fallback
    wide = F.ODEFlow(4, [512, 512]).eval()
    with pytest.raises(NotImplementedError, match="no module-path fallback|" + _native.PULL_ENVELOPE[:20]):
        wide.log_prob_noisy_grad(x, 0.1, options=step)
