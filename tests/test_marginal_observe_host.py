"""CPU tier of ``SymplecticFlowModel.log_prob_marginal_noisy`` / ``log_prob_marginal_noisy_grad`` (csrc/ff_marginal_observe.hip:
ff_marginal_observe_expand, ff_marginal_observe_grad_reduce): the host twins of the two kernels against the kernels they extend
(bitwise: the q half is ``marginal_expand(observe_expand(x, sigma, K), 1)``'s, the p half and ``cond_out`` ``marginal_expand(x,
K)``'s, ``grad_x`` and ``grad_c`` ``marginal_grad_reduce``'s) and a float64 numpy restatement (one fp32 ulp), guard words around
every output, K = 1, degenerate points, the C entry points' refusals, the methods' signatures and every refusal in its order with
the device calls replaced by ones that raise, and, for every front-end case of tests/test_gpu_marginal_observe.py, the conditions
that make a pass on the device mean something:

* the fp32 floor of grad_x, grad_c and grad_noise_std is at most 5e-5, and no point is degenerate;
* a wrong reference with uniform weights 1 / K, and one with the neighbouring point's weights, misses the bar (22 floors) by at
  least 100x on every gradient;
* d / d sigma with z dropped, and with z taken from the momentum index, misses it by at least 100x;
* in the cut-off case between a quarter and three quarters of the draws are kept, and no weight is within 1e-3 of the threshold.

These conditions and the pin of the four older methods' messages run no new code and pass without the feature; every other test
here needs it.
"""
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import symplectic as S
from tests import _leapfrog_pull_ref as L
from tests import _marginal_grad_ref as M
from tests import _marginal_observe_ref as O
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import FACTOR

ROOT = Path(__file__).resolve().parents[1]
OK, BAD = _native.FF_OK, _native.FF_ERR_BADARG
CAP = 5e-5
CPU = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the kernels' host twins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D, K", M.KERNEL_SHAPES)
def test_expand_twin_is_its_two_parents_bitwise(D, K, B):
    O.check_expand(CPU, D, K, B, M.KERNEL_C[D], "BD")
    O.check_expand(CPU, D, K, B, M.KERNEL_C[D], "D")


def test_expand_twin_one_float_off_alignment_and_keyed_by_the_global_row():
    O.check_expand(CPU, 16, 17, 5, 4, "BD", offset=1)
    x, std, shift, scale, cond = O.expand_inputs(16, 17, 5, 4, "BD")
    whole, wc = O.raw_expand(CPU, x, std, shift, scale, cond, 17)
    part, pc = O.raw_expand(CPU, x[2:4], std[2:4], shift, scale, cond[2:4], 17, sample_offset=O.OFFSET + 2)
    assert torch.equal(O.bits(part), O.bits(whole[2 * 17:4 * 17])) and torch.equal(O.bits(pc), O.bits(wc[2 * 17:4 * 17]))
    # the composition of the existing kernels keys the momenta by the EXPANDED row: not this kernel's rows
    y, _ = _native.observe_expand(x, std, 17, O.SEED, O.OFFSET)
    via, _ = _native.marginal_expand(y, 1, O.SEED, O.OFFSET, shift, scale)
    assert not torch.equal(via[:, 16:], whole[:, 16:])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D, K", M.KERNEL_SHAPES)
def test_reduce_twin_is_marginal_grad_reduce_bitwise_and_the_float64_restatement(D, K, B):
    for mode in ("partial", "full", "empty"):
        O.check_reduce(O.run_reduce(CPU, D, K, B, M.KERNEL_C[D], keep_mode=mode), K, (D, K, B, mode))


def test_reduce_twin_one_float_off_alignment_the_vector_layout_and_the_case_of_the_second_grid_trip():
    O.check_reduce(O.run_reduce(CPU, 16, 17, 5, 4, offset=1), 17)
    O.check_reduce(O.run_reduce(CPU, 4, 65, 5, 4, std_layout="D"), 65)
    D, K, B = M.BIG
    O.check_reduce(O.run_reduce(CPU, D, K, B, 0), K, M.BIG)


def test_one_draw_is_minus_z_g_over_scale_rounded_once():
    D, C, B = 5, 3, 7
    _, gz, gc, scale, cscale = M.kernel_inputs(D, 1, B, C)
    lw = torch.linspace(-30.0, 4.0, B, dtype=torch.float64)
    rows = torch.arange(B, dtype=torch.int32)
    z, _ = O.draws(B, D, 1)
    gx, gcond, gs = _native.marginal_observe_grad_reduce(lw, rows, gz, gc, torch.ones(D), 1, O.SEED, O.OFFSET, scale, cscale)
    want = (-(z[:, 0].double() * gz[:, :D].double()) / scale.double()).float()
    assert torch.equal(O.bits(gs), O.bits(want))
    assert torch.equal(O.bits(gx), O.bits(gz[:, :D] / scale)) and torch.equal(O.bits(gcond), O.bits(gc / cscale))
    _, _, gs = _native.marginal_observe_grad_reduce(lw, rows, gz, None, torch.ones(D), 1, O.SEED, O.OFFSET)
    assert torch.equal(O.bits(gs), O.bits((-(z[:, 0].double() * gz[:, :D].double())).float()))


def test_degenerate_points_write_nan_to_all_three_while_their_neighbours_are_untouched():
    D, K, B, C = 5, 4, 5, 3
    clean = O.run_reduce(CPU, D, K, B, C, min_weight=0.0)
    z1 = M.kernel_inputs(D, K, B, C)[0].clone()
    z1[1 * K + 2, 3] = float("nan")                            # point 1: a NaN row
    z1[3 * K:4 * K, 0] = float("inf")                          # point 3: every lw is -inf
    r = O.run_reduce(CPU, D, K, B, C, min_weight=0.0, z1=z1)
    assert r.keep.view(B, K).tolist() == [[1] * K, [0] * K, [1] * K, [0] * K, [1] * K]
    for got, ref in ((r.gx, clean.gx), (r.gcond, clean.gcond), (r.gs, clean.gs)):
        assert bool(torch.isnan(got[[1, 3]]).all())
        assert torch.equal(O.bits(got[[0, 2, 4]]), O.bits(ref[[0, 2, 4]]))
    assert torch.equal(O.bits(r.gx), O.bits(r.px)) and torch.equal(O.bits(r.gcond), O.bits(r.pc))


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures_and_refuse_bad_arguments():
    Lb = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    expand = ("const float* x, const float* noise_std, int32_t std_row_stride, const float* shift, const float* scale, "
              "const float* cond, int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0, "
              "float* cond_out")
    grad = ("const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows, const float* scale, "
            "const float* cond_scale, const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K, "
            "uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std")
    for proto in (f"int ff_marginal_observe_expand({expand}, void* hip_stream);", f"int ff_marginal_observe_expand_host({expand});",
                  f"int ff_marginal_observe_grad_reduce({grad}, void* hip_stream);",
                  f"int ff_marginal_observe_grad_reduce_host({grad});"):
        assert proto in header, proto
    K, Dd, C = 3, 5, 2
    x, std, sh, sc, cond = torch.zeros(2, Dd), torch.ones(2, Dd), torch.zeros(Dd), torch.ones(Dd), torch.zeros(2, C)
    z0, co = torch.zeros(2 * K, 2 * Dd), torch.zeros(2 * K, C)
    p = lambda t: t.data_ptr()
    ebase = (("x", p(x)), ("std", p(std)), ("stride", Dd), ("sh", p(sh)), ("sc", p(sc)), ("cond", p(cond)), ("B", 2), ("D", Dd),
             ("C", C), ("K", K), ("seed", 1), ("off", 0), ("z0", p(z0)), ("co", p(co)))
    ex = lambda **kw: Lb.ff_marginal_observe_expand_host(*[kw.get(n, v) for n, v in ebase])
    assert ex() == OK and ex(B=0) == OK and ex(stride=0) == OK and ex(sh=0, sc=0) == OK and ex(cond=0, C=0, co=0) == OK
    assert ex(K=_native.MAX_MOMENTA, B=0) == OK
    for kw in (dict(x=0), dict(std=0), dict(z0=0), dict(B=-1), dict(D=0), dict(K=0), dict(K=_native.MAX_MOMENTA + 1),
               dict(stride=1), dict(stride=Dd + 1), dict(C=0), dict(co=0)):
        assert ex(**kw) == BAD, kw
    lw, rows = torch.zeros(2 * K, dtype=torch.float64), torch.arange(2 * K, dtype=torch.int32)
    gz, gc, cs = torch.zeros(2 * K, 2 * Dd), torch.zeros(2 * K, C), torch.ones(C)
    ox, oc, os_ = torch.zeros(2, Dd), torch.zeros(2, C), torch.zeros(2, Dd)
    gbase = (("lw", p(lw)), ("rows", p(rows)), ("gz", p(gz)), ("gc", p(gc)), ("sc", p(sc)), ("cs", p(cs)), ("std", p(std)),
             ("stride", Dd), ("B", 2), ("D", Dd), ("C", C), ("K", K), ("seed", 1), ("off", 0), ("ox", p(ox)), ("oc", p(oc)),
             ("os", p(os_)))
    gr = lambda **kw: Lb.ff_marginal_observe_grad_reduce_host(*[kw.get(n, v) for n, v in gbase])
    assert gr() == OK and gr(B=0) == OK and gr(gc=0, C=0, oc=0, cs=0) == OK and gr(sc=0, cs=0) == OK and gr(os=0) == OK
    assert gr(stride=0) == OK
    for kw in (dict(lw=0), dict(rows=0), dict(gz=0), dict(std=0), dict(ox=0), dict(B=-1), dict(D=0), dict(K=0),
               dict(K=_native.MAX_MOMENTA + 1), dict(stride=1), dict(C=0), dict(oc=0)):
        assert gr(**kw) == BAD, kw
    # the device entry points refuse the same before anything is enqueued: no device is needed to ask
    dev_ex = lambda **kw: Lb.ff_marginal_observe_expand(*[kw.get(n, v) for n, v in ebase], None)
    dev_gr = lambda **kw: Lb.ff_marginal_observe_grad_reduce(*[kw.get(n, v) for n, v in gbase], None)
    assert dev_ex(stride=1) == BAD and dev_ex(z0=0) == BAD and dev_ex(K=0) == BAD and dev_ex(B=0) == OK
    assert dev_gr(stride=1) == BAD and dev_gr(std=0) == BAD and dev_gr(C=0) == BAD and dev_gr(B=0) == OK
    # the binding's own checks
    with pytest.raises(ValueError, match="joint draws"):
        _native.marginal_observe_expand(x, std, 0, 1)
    with pytest.raises(RuntimeError, match=r"noise_std has shape \(3,\)"):
        _native.marginal_observe_expand(x, torch.ones(3), K, 1)
    with pytest.raises(RuntimeError, match="scale has 3 elements"):
        _native.marginal_observe_expand(x, std, K, 1, scale=torch.ones(3))
    with pytest.raises(RuntimeError, match=r"cond has shape"):
        _native.marginal_observe_expand(x, std, K, 1, cond=torch.zeros(3, C))
    with pytest.raises(RuntimeError, match="contiguous float32"):
        _native.marginal_observe_expand(x.double(), std, K, 1)
    with pytest.raises(RuntimeError, match="row_of points at row"):
        _native.marginal_observe_grad_reduce(lw, rows, gz[:4].contiguous(), None, std, K, 1)
    with pytest.raises(RuntimeError, match="row_of must be a contiguous int32"):
        _native.marginal_observe_grad_reduce(lw, rows.long(), gz, None, std, K, 1)
    with pytest.raises(RuntimeError, match="float64"):
        _native.marginal_observe_grad_reduce(lw.float(), rows, gz, None, std, K, 1)
    with pytest.raises(RuntimeError, match=r"noise_std has shape \(2, 3\)"):
        _native.marginal_observe_grad_reduce(lw, rows, gz, None, torch.ones(2, 3), K, 1)
    with pytest.raises(RuntimeError, match="grad_noise_std has 3 elements"):
        _native.marginal_observe_grad_reduce(lw, rows, gz, None, std, K, 1, grad_noise_std=torch.zeros(3))


# ---- the conditions on the GPU file's cases (reference only: they pass without the feature) -----------------------------------------
@pytest.mark.parametrize("ck", O.CASES, ids=O.case_id)
def test_every_gpu_case_has_low_floors_no_degenerate_point_and_tells_every_damaged_reference(ck):
    r = O.references(ck)
    r32, r64 = r[torch.float32], r[torch.float64]
    K = ck[1]
    assert bool(torch.isfinite(r64.lw).all()) and bool(torch.isfinite(r32.lw).all())             # no point is degenerate
    own = O.weighted(r64, r64.wn)
    for got, ref in zip(own, (r64.gx, r64.gc, r64.gs)):        # autograd through the logsumexp is the weighted sum, z included
        assert ref is None or R.normalised_error(got, ref) <= 1e-12
    damaged = {"uniform weights": O.weighted(r64, torch.full_like(r64.wn, 1.0 / K)),
               "the neighbour's weights": O.weighted(r64, r64.wn.roll(1, 0)),
               "z dropped": O.weighted(r64, r64.wn, None), "z from the momentum index": O.weighted(r64, r64.wn, "p")}
    fl = O.floors(r32, r64)
    for i, what in enumerate(("gx", "gc", "gs")):
        if what not in fl:
            continue
        assert fl[what] <= CAP, (what, fl[what])
        for name, dm in damaged.items():
            if what != "gs" and name.startswith("z "):
                continue                                       # (those two damage d / d sigma alone)
            miss = R.normalised_error(dm[i], getattr(r64, what)) / (FACTOR * fl[what])
            print(f"\n[marginal_observe] {O.case_id(ck)} {what}: floor {fl[what]:.3e}; {name} miss the bar by {miss:.0f}x")
            assert miss >= 100.0, (what, name, miss)


def test_the_cut_off_case_keeps_between_a_quarter_and_three_quarters_and_no_weight_is_near_the_threshold():
    wn = O.references((O.CUT_CASE, O.CUT_K))[torch.float64].wn
    frac = float((wn >= O.CUT).double().mean())
    gap = float(((wn - O.CUT).abs() / O.CUT).min())
    print(f"\n[marginal_observe] cut-off case: {frac:.3f} of the draws at or above {O.CUT}, the nearest weight {gap:.3e} away")
    assert 0.25 <= frac <= 0.75 and gap >= 1e-3
    assert O.CUT_CASE in L.LOGP_CASES and O.CUT_K in O.KS


def test_the_cases_are_the_ones_the_issue_names():
    assert [c for c, _ in O.CASES[::2]] == L.LOGP_CASES and O.KS == (2, 4) and len(O.CASES) == 6
    assert M.KERNEL_SHAPES == [(1, 1), (4, 65), (5, 3), (16, 17), (17, 4), (32, 9)] and M.BIG == (4, 64, 1 << 14)
    assert FACTOR == 22.0 and all(0 < s for s in O.SIGMA.values()) and len(O.SIGMA) == 3


# ---- the methods: signatures, refusals and their order ----------------------------------------------------------------------------------
def test_the_methods_have_the_signatures_of_the_issue_and_the_old_names_stay_absent():
    sig = inspect.signature(S.SymplecticFlowModel.log_prob_marginal_noisy)
    names = list(sig.parameters)
    assert names == ["self", "x", "noise_std", "conditional", "num_draws", "atol", "rtol", "method", "num_steps", "options", "seed",
                     "sample_offset", "chunk_points", "return_ess"]
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == names[7:]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert [d[n] for n in names[3:]] == [None, 16, 1e-5, 1e-5, "dopri5", None, None, None, 0, None, False]
    sig = inspect.signature(S.SymplecticFlowModel.log_prob_marginal_noisy_grad)
    names = list(sig.parameters)
    assert names == ["self", "x", "noise_std", "conditional", "num_draws", "method", "num_steps", "seed", "sample_offset",
                     "chunk_points", "min_weight", "return_ess", "return_noise_grad"]
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == names[5:]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert [d[n] for n in names[3:]] == [None, 16, "leapfrog", None, None, 0, None, 0.0, False, False]
    for old in ("log_prob_noisy", "posterior_noisy", "log_prob_noisy_grad"):
        assert not hasattr(S.SymplecticFlowModel, old)


DEVICE_CALLS = [(_native, "marginal_expand"), (_native, "marginal_observe_expand"), (_native, "marginal_reduce"),
                (_native, "marginal_weigh"), (_native, "marginal_grad_reduce"), (_native, "marginal_observe_grad_reduce"),
                (odeint, "solve_leapfrog"), (odeint, "solve"), (odeint, "_leapfrog_pull_from")]


class Touched(Exception):
    pass


def _no_device(monkeypatch):
    def touched(*a, **kw):
        raise Touched
    for mod, name in DEVICE_CALLS:
        monkeypatch.setattr(mod, name, touched)


def test_every_refusal_of_the_gradient_comes_in_its_order_before_the_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    front, x, std, cond = O.case_inputs(L.LOGP_CASES[0])                         # D 4, C 3, on the CPU
    call = lambda *a, x=x, std=std, cond=cond, **kw: front.log_prob_marginal_noisy_grad(x, std, cond, *a, **kw)
    nan_std = torch.full_like(std, float("nan"))
    # 1. num_draws, min_weight, chunk_points -- each ahead of everything behind it
    for K in (0, -3, _native.MAX_MOMENTA + 1):
        with pytest.raises(ValueError, match=f"num_draws={K}: 1 .. {_native.MAX_MOMENTA} joint"):
            call(K, method="dopri5", min_weight=2.0, chunk_points=0)
    for m in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= min_weight < 1"):
            call(4, method="dopri5", min_weight=m, chunk_points=0)
    with pytest.raises(ValueError, match="at least one data point per chunk"):
        call(4, method="dopri5", chunk_points=0)
    # 2. the method -- ahead of num_steps and of the tensors; log_prob_marginal_grad's wording
    for method in ("dopri5", "euler", "rk4"):
        with pytest.raises(ValueError, match=r"log_prob_marginal_noisy_grad: method=.*not shears.*record.*"
                                             r"method=\"leapfrog\" with num_steps"):
            call(4, method=method, x=x.double(), std=nan_std)
    # 3. num_steps
    for n in (None, 0, -1):
        with pytest.raises(ValueError, match="method='leapfrog' needs num_steps >= 1"):
            call(4, num_steps=n, x=x.double(), std=nan_std)
    # 4. x
    for bad in (x[0], x.double(), x.numpy()):
        with pytest.raises(ValueError, match=r"log_prob_marginal_noisy_grad: x must be a \[batch, dim\] float32 tensor"):
            call(4, num_steps=2, x=bad, std=nan_std)
    # 5. noise_std: noise_std_tensor's errors, ahead of the conditional's
    with pytest.raises(ValueError, match=r"noise_std has shape \(9, 3\)"):
        call(4, num_steps=2, std=std[:, :3], cond=cond[:4])
    for bad in (nan_std, -std, float("inf"), -1.0):
        with pytest.raises(ValueError, match="noise_std must be finite and >= 0 everywhere"):
            call(4, num_steps=2, std=bad, cond=cond[:4])
    # 6. the leapfrog pull-backs' refusals, with their types and messages
    with pytest.raises(ValueError, match=r"conditional must be \[9, cond_dim\]"):
        call(4, num_steps=2, cond=cond[:4])
    with pytest.raises(TypeError):
        call(4, num_steps=2, cond=cond.double())
    with pytest.raises(RuntimeError, match="GPU|cuda|device"):
        call(4, num_steps=2)
    monkeypatch.setattr(odeint, "_need_gpu", lambda t: None)                   # (the checks behind the device check)
    with pytest.raises(ValueError, match=r"conditional must be \[9, 3\]"):
        call(4, num_steps=2, cond=None)
    with pytest.raises(ValueError, match="z has 10 columns, the model's joint state has 8"):
        call(4, num_steps=2, x=torch.zeros(9, 5), std=0.1)
    plain, x1, std1, _ = O.case_inputs(L.LOGP_CASES[1])
    with pytest.raises(ValueError, match="no conditional inputs"):
        plain.log_prob_marginal_noisy_grad(x1, std1, torch.zeros(9, 2), 4, num_steps=2)
    wide = L.make_model(4, 0, [512, 512])
    with pytest.raises(NotImplementedError, match="no module-path fallback"):
        wide.log_prob_marginal_noisy_grad(torch.zeros(3, 4), 0.1, None, 4, num_steps=2)
    # ... and a call that nothing refuses gets as far as the first device call, no further -- in every layout of noise_std
    for s in (std, std[0].clone(), 0.25, torch.tensor(0.25)):
        with pytest.raises(Touched):
            call(4, num_steps=2, std=s, return_noise_grad=True)
    assert not hasattr(front, "last_marginal_noisy_grad_stats")


def test_every_refusal_of_the_value_comes_in_its_order_before_the_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    front, x, std, cond = O.case_inputs(L.LOGP_CASES[0])
    call = lambda *a, x=x, std=std, cond=cond, **kw: front.log_prob_marginal_noisy(x, std, cond, *a, **kw)
    nan_std = torch.full_like(std, float("nan"))
    for K in (0, _native.MAX_MOMENTA + 1):
        with pytest.raises(ValueError, match=f"num_draws={K}: 1 .. {_native.MAX_MOMENTA} joint"):
            call(K, method="nonsense", chunk_points=0)
    with pytest.raises(ValueError, match="at least one data point per chunk"):
        call(4, method="nonsense", chunk_points=0)
    with pytest.raises(ValueError, match="method='nonsense': log_prob takes 'dopri5'"):
        call(4, method="nonsense", x=x.double())
    with pytest.raises(ValueError, match="num_steps belongs to method='leapfrog'"):
        call(4, num_steps=3, x=x.double())
    with pytest.raises(ValueError, match="method='leapfrog' needs num_steps >= 1"):
        call(4, method="leapfrog", x=x.double())
    with pytest.raises(ValueError, match=r"log_prob_marginal_noisy: x must be a \[batch, dim\] float32 tensor"):
        call(4, x=x.double(), std=nan_std)
    with pytest.raises(ValueError, match="noise_std must be finite and >= 0 everywhere"):
        call(4, std=nan_std, chunk_points=3)
    # an adaptive method solves all B K rows at once: chunk_points raises and names the way out
    with pytest.raises(ValueError, match=r"chunk_points with method='dopri5'.*all B \* num_draws rows.*method='leapfrog' with num_steps"):
        call(4, chunk_points=3)
    with pytest.raises(Touched):
        call(4)
    with pytest.raises(Touched):
        call(4, method="leapfrog", num_steps=2, chunk_points=3)


def test_log_prob_marginal_still_names_its_own_draws_when_it_refuses_chunks(monkeypatch):
    _no_device(monkeypatch)
    front, x, _, cond = O.case_inputs(L.LOGP_CASES[0])
    with pytest.raises(ValueError, match=r"all B \* num_momenta rows are one solve"):
        front.log_prob_marginal(x, cond, 4, chunk_points=3)
    with pytest.raises(Touched):
        front.log_prob_marginal(x, cond, 4, method="leapfrog", num_steps=2, chunk_points=3)
    assert hasattr(front, "_marginal_grad_chunks")             # (the loop the two gradients share)


def test_the_four_older_methods_keep_raising_with_their_messages():
    front, x, _, cond = O.case_inputs(L.LOGP_CASES[0])
    for name, what in (("flow_jvp", "carry no tangent columns"), ("flow_jacobian", "carry no tangent columns"),
                       ("flow_vjp", "carry no cotangent columns"), ("log_prob_grad", "carry no adjoint columns")):
        with pytest.raises(NotImplementedError, match=f"of a SymplecticFlowModel: the two-network kernels {what}"):
            getattr(front, name)(x, cond)
