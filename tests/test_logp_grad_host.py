"""CPU tier of the log-density gradients (csrc/ff_mlp_lgrad.hpp; ``log_prob_grad``): the signatures of the five front ends, every
front-end refusal and every refusal of ff_mlp_ode_launch_logp_grad, the LDS formula restated and held against the launch's own
refusal one layer past each ceiling, the float64 reference against central differences -- and, for every case of
tests/test_gpu_logp_grad.py, the conditions that make a pass on the device mean something:

* the fp32 floor of grad_x and grad_c is at most 5e-5 (the depth tests' cap);
* the float64 reference WITHOUT the SiLU'' cross term (eps^T J_net eps depends on the state only through the slopes, so this is
  the reference at ``div_weight = 0``) misses the case's bar (22 floors) by at least 100x;
* a float64 reference whose parameters have two output rows of ONE hidden layer's weight matrix swapped -- the first, a middle
  and the last hidden layer in turn -- misses the bar by at least 100x;
* the second-order share of the gradient, max |grad - grad at div_weight = 0| over max |grad| per sample, is at least 1e-3.

At torch's default initialisation none of that holds (tests/_deep_models.py): the cases carry gains, written next to them as
literals in the GPU file; the VP cases keep to three rk4 steps, where a score model's fp32 floor is under the cap."""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd import symplectic as S
from tests import _logp_grad_ref as LG
from tests import _pushforward_ref as R
from tests import test_gpu_logp_grad as G
from tests.test_gpu_pushforward import FACTOR

ROOT = Path(__file__).resolve().parents[1]
OK, BAD, UNS = _native.FF_OK, _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED
UNITS = ("m16_h128_d4_c4", "m16_h256_d4_c4", "m16_h256_d8_c4")
FRONTS = (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional)
CAP = 5e-5
KIB = 1024


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the reference on its own (the one test of this file that may pass without the feature) --------------------------------------
@pytest.mark.parametrize("kind, method, nsteps", [("flow", "euler", 1), ("flow", "dopri5_fixed", 2), ("vp", "rk4", 3)])
def test_reference_gradient_is_the_central_difference_of_its_value(kind, method, nsteps):
    """float64: ``torch.autograd.grad`` through ``torch.func.jvp`` against central differences of the same value, for x and the
    conditional, with three probes of weight 1 / 3 -- and the two isolated paths add up to the whole."""
    from tests.test_gpu_pushforward import make_front, options_of
    front, ref_kw = make_front(kind, 4, 2, 32, 2, gain=4.0)
    ref = LG.LogDensity(R.SolverMap(direction="to_base", method=method, options=options_of(front, "to_base", nsteps),
                                    dtype=torch.float64, **ref_kw))
    g = torch.Generator().manual_seed(1)
    x, c = torch.randn(3, 4, generator=g), torch.randn(3, 2, generator=g)
    e = torch.sign(torch.randn(3, 3, 4, generator=g))
    lp, gx, gc = ref(x, c, e, 1.0 / 3)
    fx, fc = ref.central_difference(x, c, e, 1.0 / 3)
    assert lp.dtype == torch.float64 and gx.shape == (3, 4) and gc.shape == (3, 2)
    assert R.normalised_error(gx, fx) <= 1e-7 and R.normalised_error(gc, fc) <= 1e-7
    _, sx, sc = ref(x, c, e, 1.0 / 3, div_weight=0.0)
    _, dx, dc = ref(x, c, e, 1.0 / 3, cot_weight=0.0)
    assert R.normalised_error(sx + dx, gx) <= 1e-12 and R.normalised_error(sc + dc, gc) <= 1e-12
    assert R.normalised_error(dx, gx) > 1e-3                      # (the second-order path is there)


# ---- the conditions on the GPU file's cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=G._id(c)) for c in G.CASES])
def test_every_gpu_case_has_a_low_floor_and_tells_the_cross_term_and_a_swapped_weight_row_pair(case):
    x, e, c = G.case_inputs(case)
    r = G.references(case)
    r64, r32 = r[torch.float64], r[torch.float32]
    n64 = G.references(case, div_weight=0.0)[torch.float64]
    bad = {}
    for layer in sorted({0, case.nh // 2, case.nh - 1}):
        _, refs, *_ = G.case_setup(case, damage=layer)
        bad[layer] = refs[torch.float64](x, c, e[:, None], 1.0)
    for i, what in ((1, "grad_x"), (2, "grad_c")):
        if r64[i] is None:
            continue
        floor = G.fp32_floor(r32[i], r64[i])
        share = R.normalised_error(n64[i], r64[i])
        cross = share / (FACTOR * floor)
        swaps = {layer: R.normalised_error(b[i], r64[i]) / (FACTOR * floor) for layer, b in bad.items()}
        print(f"\n[logp_grad] {G._id(case)} {what}: floor {floor:.3e}; second-order share {share:.3e}; without the cross term the "
              f"bar is missed by {cross:.0f}x; swapped rows miss it by " + " ".join(f"layer {l}: {v:.0f}x" for l, v in swaps.items()))
        assert floor <= CAP, (what, floor)
        assert cross >= 100.0, (what, cross)
        assert share >= 1e-3, (what, share)
        for layer, ratio in swaps.items():
            assert ratio >= 100.0, (what, layer, ratio)


def test_the_cases_cover_the_axes():
    cs = G.CASES
    assert {c.unit for c in cs} == {"h128_d4", "h256_d4", "h256_d8"}
    assert {1, 16, 17, 32} <= {c.D for c in cs} and {0, 1, 16} <= {c.C for c in cs}
    assert {1, 8, 9, 17} <= {c.B for c in cs} and {"euler", "rk4", "dopri5_fixed"} <= {c.method for c in cs}
    assert {1, 2, 3} <= {c.steps for c in cs} and {"vp", "flow"} <= {c.kind for c in cs}
    for unit, deepest in (("h128_d4", 19), ("h256_d4", 9), ("h256_d8", 9)):
        assert {1, 2, 4, 5, deepest} <= {c.nh for c in cs if c.unit == unit}, unit
    for c in cs:                       # the unit a case names is the one the planner picks for its shape
        assert _native.kernel_name(_native.make_pull_plan(c.D, c.C, [c.width] * c.nh)) == f"mlp_pull_m16_{c.unit}_c4", c


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    L = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    for proto in ("int ff_lgrad_kernel_count(void);", "const char* ff_lgrad_kernel_name(int index);",
                  "int ff_mlp_ode_launch_logp_grad(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* record_in, "
                  "const float* probe_in /* [batch, dim] */, const float* dlogp_cotangent /* [batch] or NULL */, "
                  "const float* cotangent_in /* [batch, dim] */, float* grad_x_out /* [batch, dim] */, "
                  "float* grad_cond_out /* [batch, cond_dim] or NULL */, void* hip_stream);",
                  "#define FF_LGRAD_KERNEL_BASE 0x90000"):
        assert proto in header, proto
    assert _native.LGRAD_KERNEL_BASE == 0x90000
    assert L.ff_mlp_ode_launch_logp_grad.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs)] + \
        [ctypes.c_void_p] * 7
    assert [f[0] for f in _native.OdeArgs._fields_][-1] == "gate"          # the new pointers are arguments, not fields
    assert L.ff_lgrad_kernel_count() == 3
    names = [L.ff_lgrad_kernel_name(i).decode() for i in range(3)]
    assert names == [f"mlp_lgrad_{u}" for u in UNITS]
    assert L.ff_lgrad_kernel_name(3) is None and L.ff_lgrad_kernel_name(-1) is None
    # a family of its own: the other tables keep their counts and do not hold the new names
    assert (L.ff_pull_kernel_count(), L.ff_vjp_kernel_count(), L.ff_rec_kernel_count(), L.ff_dadj_kernel_count()) == (3, 3, 3, 3)
    table = {L.ff_kernel_name(i).decode() for i in range(L.ff_kernel_count())}
    table |= {L.ff_push_kernel_name(i).decode() for i in range(L.ff_push_kernel_count())}
    for fam in ("pull", "vjp", "rec", "dadj"):
        table |= {getattr(L, f"ff_{fam}_kernel_name")(i).decode() for i in range(3)}
    assert not table & set(names) and not any("lgrad" in n for n in table)
    assert _native.kernel_name(_native.make_pull_plan(16, 4, [256] * 4)) == "mlp_pull_m16_h256_d4_c4"


def _args(buf, mode=_native.MODE_HUTCH, count=1):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of the
    empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count = 0, 1, mode, count
    return a


def test_every_refusal_of_the_launch_without_a_gpu():
    L = _native.lib()
    buf = torch.zeros(64)
    ptr = buf.data_ptr()
    pull = _native.make_pull_plan(16, 4, [256] * 4)
    plain = _native.make_pull_plan(16, 0, [128])
    H, ST = _native.MODE_HUTCH, _native.MODE_STATE
    lg = lambda plan, a, rec=ptr, probe=ptr, wgt=None, cot=ptr, gx=ptr, gc=None: L.ff_mlp_ode_launch_logp_grad(
        ctypes.byref(plan), ctypes.byref(a), rec, probe, wgt, cot, gx, gc, None)
    # what passes: NULL or given weights, with and without the conditional output, tangent_count 0 or 1
    for count in (0, 1):
        assert lg(pull, _args(buf, H, count)) == OK and lg(pull, _args(buf, H, count), wgt=ptr, gc=ptr) == OK
        assert lg(plain, _args(buf, H, count)) == OK
    a = _args(buf)
    a.x_in = a.x_out = 0                                                   # x_in / x_out are ignored
    assert lg(pull, a) == OK
    # more than one probe per row; the wrong mode
    for count in (2, 15, 16, -1):
        assert lg(pull, _args(buf, H, count)) == BAD, count
    for mode in (ST, _native.MODE_EXACT, 7):
        assert lg(pull, _args(buf, mode, 1)) == BAD, mode
    # NULL required pointers (a missing probe_in among them); no arguments; grad_cond_out without conditional inputs
    for null in ("rec", "probe", "cot", "gx"):
        assert lg(pull, _args(buf), **{null: None}) == BAD, null
    assert L.ff_mlp_ode_launch_logp_grad(ctypes.byref(pull), None, ptr, ptr, None, ptr, ptr, None, None) == BAD
    assert lg(plain, _args(buf), gc=ptr) == BAD
    # the divergence side, attempt launches, the Jacobian output, noise, probes of the caller's own
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out", "probe"):
        a = _args(buf)
        setattr(a, field, ptr)
        assert lg(pull, a) == BAD, field
    a = _args(buf)
    a.n_aux = 1
    a.aux_out[0] = ptr
    assert lg(pull, a) == BAD
    for field in ("wpack", "etab", "cond"):
        a = _args(buf)
        setattr(a, field, 0)
        assert lg(pull, a) == BAD, field
    a = _args(buf)
    a.stage_slots = 8
    assert lg(pull, a) == BAD
    # a plan that is not a pull plan; a split-precision plan; forged indices
    for mode in (H, ST, _native.MODE_EXACT):
        assert lg(_native.make_plan(16, 4, [256] * 4, mode), _args(buf)) == BAD
    assert lg(_native.make_push_plan(16, 4, [256] * 4), _args(buf)) == BAD
    for select in (False, True):
        assert lg(_native.make_pair_plan(8, 0, [128, 128], select=select), _args(buf)) == BAD
    assert lg(_native.make_plan(16, 0, [256] * 4, H, precision=_native.PREC_BF16X2), _args(buf)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(pull)
    for kid in (_native.PULL_KERNEL_BASE + 3, _native.LGRAD_KERNEL_BASE, _native.DADJ_KERNEL_BASE):
        forged.kernel_id = kid
        assert lg(forged, _args(buf)) == BAD, kid
    # handing a pull plan to the existing launches behaves as before
    assert L.ff_mlp_ode_launch_pull_discrete(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), ptr, ptr, ptr, None, None) == OK
    assert L.ff_mlp_ode_launch_record(ctypes.byref(pull), ctypes.byref(_args(buf, ST, 0)), ptr, None) == OK


def lds_bytes(dregs, width, nh, slots, tile=16):
    """csrc/ff_api.cpp lgrad_lds_bytes, restated: adjoint slots of dregs words per lane, then two words per hidden unit for each of
    the tile's tile / 2 rows -- 64 n_hidden width bytes at 16 columns."""
    return slots * (dregs // 4) * 64 * 16 + (tile // 2) * nh * width * 2 * 4


@pytest.mark.parametrize("unit, D_, width, dregs, ceiling", [("h128_d4", 16, 128, 4, 19), ("h256_d4", 16, 256, 4, 9), ("h256_d8", 32, 256, 8, 9)])
def test_the_launch_accepts_the_ceiling_depth_and_refuses_one_layer_more(unit, D_, width, dregs, ceiling):
    """Per unit and slot count (euler 1, rk4 4, dopri5_fixed 7, 0 = all seven): the restated request stays under 160 KiB up to the
    ceiling -- 19 x 128, 9 x 256 -- and passes it one layer later, exactly where the launch answers FF_ERR_UNSUPPORTED."""
    L, buf = _native.lib(), torch.zeros(64)
    ptr = buf.data_ptr()
    base = _native.make_pull_plan(D_, 4, [width] * 4)
    assert _native.kernel_name(base) == f"mlp_pull_m16_{unit}_c4" and int(base.dregs) == dregs
    assert lds_bytes(4, 256, 4, 4) == 68 * KIB and lds_bytes(8, 256, 4, 7) == 78 * KIB      # 4 x 256: 64 KiB of stash and the slots
    for slots in (1, 4, 7, 0):
        kept = slots or 7
        for nh in range(1, ceiling + 3):
            plan = _native.PlanStruct.from_buffer_copy(base)
            plan.n_hidden = nh
            a = _args(buf)
            a.stage_slots = slots
            rc = L.ff_mlp_ode_launch_logp_grad(ctypes.byref(plan), ctypes.byref(a), ptr, ptr, None, ptr, ptr, None, None)
            fits = lds_bytes(dregs, width, nh, kept) <= 160 * KIB
            assert rc == (OK if fits else UNS), (slots, nh, rc)
            assert fits == (nh <= ceiling), (slots, nh)
    assert lds_bytes(dregs, width, ceiling, 7) > 64 * KIB


# ---- the op ----------------------------------------------------------------------------------------------------------------------------
def test_the_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_logp_grad
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_pull_plan(16, 4, [256] * 4), 4)
    with FakeTensorMode():
        rec, c, etab = torch.empty(12, 9, 16), torch.empty(9, 4), torch.empty(12, 32 + 256)
        e, w, cot = torch.empty(9, 16), torch.empty(9), torch.empty(9, 16)
        gx, gc, st = op(rec, c, e, w, cot, torch.empty(10), etab, None, None, None, None, plan, True)
        assert gx.shape == (9, 16) and gc.shape == (9, 4) and st.shape == (1,)
        gx, gc, st = op(rec, c, e, None, cot, torch.empty(10), etab, None, None, None, None, plan, False)
        assert gx.shape == (9, 16) and gc.shape == (9, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(12, 2, 16), torch.zeros(2, 4), torch.zeros(2, 16), None, torch.zeros(2, 16), torch.zeros(10),
           torch.zeros(12, 288), None, None, None, None, plan, True)


# ---- the front ends ------------------------------------------------------------------------------------------------------------------
def test_signatures_on_the_five_classes():
    for cls in FRONTS:
        prm = inspect.signature(cls.log_prob_grad).parameters
        names = list(prm)
        assert names[:3] == ["self", "x", "conditional"] and prm["conditional"].default is None, cls
        want = {"method": "rk4", "options": None, "probe": "torch", "seed": None, "sample_offset": 0, "num_probes": 1}
        if cls in (F.ODEFlow, F.ConditionalODEFlow):
            want["hutchinson"] = False                            # the flows take hutchinson= as their log_prob does
        assert set(names[3:]) == set(want), (cls, names)
        for k, v in want.items():
            assert prm[k].kind is inspect.Parameter.KEYWORD_ONLY and prm[k].default == v, (cls, k)
        doc = " ".join(cls.log_prob_grad.__doc__.split())
        assert "log_p [B, 1]" in doc and "grad_x [B, D]" in doc, cls
    prm = inspect.signature(odeint.solve_logp_grad).parameters
    assert list(prm)[:11] == ["front", "x", "t_span", "method", "options", "probes", "probe_weight", "cond", "in_shift", "in_scale",
                             "cond_tangent_scale"]
    doc = " ".join(odeint.solve_logp_grad.__doc__.split()).lower()
    for piece in ("fixed probes", "discrete_piece_rows", "bitwise", "replica 0", "parameter gradients", "torch.autograd", "adaptive",
                  "multi-probe column layout", "twins", "split precision", "non-silu", "module-path fallback", "sharded",
                  "log_prob_noisy"):
        assert piece in doc, piece
    prm = inspect.signature(odeint._pull_checks).parameters                # the pull-backs' checks keep their name by default
    assert prm["what"].default == "flow-map pull-backs" and prm["tile_limit"].default is True
    from flowfusion_amd.fused import FusedNet
    assert list(inspect.signature(FusedNet.logp_grad).parameters)[:9] == ["self", "rec", "table", "probe", "cot", "weight", "cond",
                                                                         "want_cond", "stage_slots"]


def _score_model(D_=4, C=0, units=(64, 64), **kw):
    torch.manual_seed(3)
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=C, embedding_dimensions=8, units=list(units)), D.VPSDE(), **kw).eval()


def _fronts():
    torch.manual_seed(4)
    m, mc = _score_model().model, _score_model(C=2).model
    return [(_score_model(hutchinson=True), 0), (_score_model(C=2), 2), (F.ODEFlow(4, [64, 64]), 0),
            (F.ConditionalODEFlow(4, 2, [64, 64]), 2), (D.PopulationModelDiffusion(model=m, sde=D.VPSDE(), method="rk4"), 0),
            (D.PopulationModelDiffusionConditional(model=mc, sde=D.VPSDE(), method="rk4"), 2)]


def _grad(front, C, x, **kw):
    return front.log_prob_grad(x, **kw) if C == 0 else front.log_prob_grad(x, torch.randn(x.shape[0], C), **kw)


def test_front_end_refusals_come_before_the_device():
    """Everything here runs on CPU tensors: a refusal that came after the device was touched would raise the GPU-only
    RuntimeError instead of the error under test."""
    x = torch.randn(5, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    for front, C in _fronts():
        for method in solvers.ALL_ADAPTIVE:
            with pytest.raises(ValueError) as info:
                _grad(front, C, x, method=method)
            for piece in ("log-density gradients", "adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}'):
                assert piece in str(info.value), (piece, str(info.value))
        with pytest.raises(ValueError, match="log-density gradients.*grid_constructor"):
            _grad(front, C, x, method="rk4", options={"grid_constructor": lambda f, y, t: t})
        with pytest.raises(ValueError, match="log-density gradients.*perturb"):
            _grad(front, C, x, method="rk4", options={"step_size": 0.5, "perturb": True})
        with pytest.raises(ValueError, match="log-density gradients"):
            _grad(front, C, torch.randn(5, 3), **fixed)                  # the wrong number of columns
        with pytest.raises(ValueError, match="log-density gradients"):
            _grad(front, C, torch.randn(5), **fixed)
        if C:
            with pytest.raises(ValueError, match="log-density gradients"):
                front.log_prob_grad(x, torch.randn(5, C + 1), **fixed)
            with pytest.raises(ValueError, match="log-density gradients"):
                front.log_prob_grad(x, **fixed)                         # the conditional is missing
        else:
            with pytest.raises(ValueError, match="log-density gradients.*no conditional"):
                front.log_prob_grad(x, torch.randn(5, 2), **fixed)
        inner = getattr(front, "score_model", front)
        inner.precision = "bf16x2"
        try:
            with pytest.raises(ValueError, match="log-density gradients with precision='bf16x2'.*precision='f32'"):
                _grad(front, C, x, **fixed)
        finally:
            inner.precision = "f32"
        with pytest.raises(RuntimeError, match="GPU|cuda"):                 # and a run that passes every check needs the device
            _grad(front, C, x, **fixed)
    # Hutch++ / XTrace models; more probes than an exact-trace model has; philox probes without a Hutchinson model
    for kw in (dict(hutchpp=True), dict(xtrace=True)):
        with pytest.raises(ValueError, match="Hutch\\+\\+ / XTrace.*hutchinson=True"):
            _score_model(**kw).log_prob_grad(x, **fixed)
    with pytest.raises(ValueError, match="num_probes"):
        _score_model().log_prob_grad(x, num_probes=3, **fixed)
    with pytest.raises(ValueError, match="num_probes"):
        F.ODEFlow(4, [64, 64]).log_prob_grad(x, num_probes=3, **fixed)
    with pytest.raises(ValueError, match="philox"):
        _score_model().log_prob_grad(x, probe="philox", seed=1, **fixed)
    with pytest.raises(ValueError, match="philox"):
        F.ODEFlow(4, [64, 64]).log_prob_grad(x, probe="philox", seed=1, **fixed)
    # networks outside the pull-back units, and the two-network flows: NotImplementedError naming the envelope
    with pytest.raises(NotImplementedError) as info:
        F.ODEFlow(4, [64, 64], activation=torch.nn.Tanh).log_prob_grad(x, **fixed)
    assert _native.PULL_ENVELOPE in str(info.value)
    sym = S.SymplecticFlowModel.__new__(S.SymplecticFlowModel)
    with pytest.raises(NotImplementedError) as info:
        S.SymplecticFlowModel.log_prob_grad(sym, x)
    assert _native.PULL_ENVELOPE in str(info.value) and "log_prob_grad" in str(info.value)


def test_the_pull_backs_keep_their_messages():
    x, w = torch.randn(5, 4), torch.randn(5, 3, 4)
    with pytest.raises(ValueError, match="flow-map pull-backs with the adaptive"):
        F.ODEFlow(4, [64, 64]).flow_vjp(x, w, method="dopri5", adjoint="discrete")
    with pytest.raises(ValueError, match="flow-map pull-backs: K=16"):
        F.ODEFlow(4, [64, 64]).flow_vjp(x, torch.randn(5, 16, 4), method="rk4", adjoint="discrete")
