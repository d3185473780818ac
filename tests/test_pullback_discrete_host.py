"""CPU tier of the exact discrete adjoint (csrc/ff_mlp_dadj.hpp; ``flow_vjp(adjoint="discrete")``): the exported entry points,
the two new kernel tables, every refusal of the two launches' argument check without a GPU, ``ff_mlp_record_floats``, the two
ops' fake registration, the front ends' errors ahead of the device, the keyword on the five classes, the transposed row
program emulated on the host in float64 against ``torch.func.vjp`` of the forward row program (with its two negative
controls), the float64 reference against ``w^T SolverMap.jacobian``, and the discrimination condition of every case of the GPU
file's table: the continuous adjoint misses the case's bar by at least 100x and the case's fp32 floor is at most 5e-5."""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch

from flowfusion_amd import _native, solvers
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd import symplectic as S
from tests import _pullback_discrete_ref as DP
from tests import _pullback_ref as P
from tests import _pushforward_ref as R

ROOT = Path(__file__).resolve().parent.parent
BAD, UNS, OK = _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED, _native.FF_OK
FRONTS = (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional)
UNITS = ["m16_h128_d4_c4", "m16_h256_d4_c4", "m16_h256_d8_c4"]


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the reference on its own (the one test of this file that needs nothing the library adds) ------------------------------
def _cflow():
    torch.manual_seed(5)
    fl = F.ConditionalODEFlow(4, 2, [32, 32])
    x, c, w = torch.randn(5, 4), torch.randn(5, 2), torch.randn(5, 2, 4)
    return R.flow_params(fl), x, c, w


@pytest.mark.parametrize("method, nsteps", [("euler", 1), ("midpoint", 2), ("rk4", 1), ("dopri5_fixed", 3)])
@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_reference_is_the_transposed_jacobian_of_the_discrete_map(method, nsteps, direction):
    """float64: ``DiscretePullback`` equals ``w^T SolverMap.jacobian`` to 1e-12 at grids where the continuous adjoint is far
    off, and its stage states end in the map's own result."""
    prm, x, c, w = _cflow()
    sm = R.SolverMap("flow", prm, direction, method, {"step_size": 1.0 / nsteps}, dtype=torch.float64)
    y, Jx, Jc = sm.jacobian(x, c)
    ref = DP.DiscretePullback(sm)
    x_out, gx, gc = ref(x, w, c)
    assert x_out.dtype == torch.float64 and gx.shape == (5, 2, 4) and gc.shape == (5, 2, 2)
    assert torch.equal(x_out, y)
    wJx, wJc = torch.einsum("bki,bij->bkj", w.double(), Jx), torch.einsum("bki,bij->bkj", w.double(), Jc)
    assert R.normalised_error(gx, wJx) <= 1e-12 and R.normalised_error(gc, wJc) <= 1e-12
    rec, end = ref.stage_states(x, c)
    assert rec.shape == (nsteps * solvers.resolve_method(method).stages, 5, 4)
    # (the row table carries its times and tableau coefficients in fp32, the oracle's solver in the map's dtype: 2^-24 relative
    # per coefficient, a few rows deep -- 1e-6, a twentieth of the 2e-5 bar the record is held to)
    assert R.normalised_error(end, y) <= 1e-6
    if method == "euler":
        cont = P.Pullback(sm)(x, w, c)
        gap = max(R.normalised_error(cont[1], gx), R.normalised_error(cont[2], gc))
        assert gap > 1e-3, gap                                  # (the continuous adjoint is another function here: nine orders off)


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    L = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    for proto in ("int ff_rec_kernel_count(void);", "const char* ff_rec_kernel_name(int index);",
                  "int ff_dadj_kernel_count(void);", "const char* ff_dadj_kernel_name(int index);",
                  "size_t ff_mlp_record_floats(int64_t batch, int32_t n_evals, int32_t dim);",
                  "int ff_mlp_ode_launch_record(const ff_mlp_plan_t* plan, const ff_ode_args* args, float* record_out "
                  "/* [n_evals, batch, dim] */, void* hip_stream);",
                  "int ff_mlp_ode_launch_pull_discrete(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* record_in, "
                  "const float* cotangent_in /* [batch, K, dim] */, float* cot_x_out /* [batch, K, dim] */, float* cot_cond_out "
                  "/* [batch, K, cond_dim] or NULL */, void* hip_stream);",
                  "#define FF_REC_KERNEL_BASE 0x70000", "#define FF_DADJ_KERNEL_BASE 0x80000"):
        assert proto in header, proto
    assert (_native.REC_KERNEL_BASE, _native.DADJ_KERNEL_BASE) == (0x70000, 0x80000)
    assert L.ff_mlp_ode_launch_record.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs),
                                                   ctypes.c_void_p, ctypes.c_void_p]
    assert L.ff_mlp_ode_launch_pull_discrete.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs)] + \
        [ctypes.c_void_p] * 5
    # the new pointers are arguments, not fields of ff_ode_args (tests/test_abi.py pins the struct itself)
    assert [f[0] for f in _native.OdeArgs._fields_][-1] == "gate"
    # two families of their own, one sibling per pull unit; the other tables keep their counts
    assert L.ff_rec_kernel_count() == 3 and L.ff_dadj_kernel_count() == 3
    rec = [L.ff_rec_kernel_name(i).decode() for i in range(3)]
    dadj = [L.ff_dadj_kernel_name(i).decode() for i in range(3)]
    assert rec == [f"mlp_rec_{u}" for u in UNITS] and dadj == [f"mlp_dadj_{u}" for u in UNITS]
    for name in (L.ff_rec_kernel_name, L.ff_dadj_kernel_name):
        assert name(3) is None and name(-1) is None
    assert L.ff_pull_kernel_count() == 3 and L.ff_vjp_kernel_count() == 3
    table = {L.ff_kernel_name(i).decode() for i in range(L.ff_kernel_count())}
    table |= {L.ff_push_kernel_name(i).decode() for i in range(L.ff_push_kernel_count())}
    table |= {L.ff_pull_kernel_name(i).decode() for i in range(3)} | {L.ff_vjp_kernel_name(i).decode() for i in range(3)}
    assert not table & set(rec + dadj) and not any("_rec_" in n or "dadj" in n for n in table)
    # a pull plan still names its pull unit
    assert _native.kernel_name(_native.make_pull_plan(16, 4, [256] * 4)) == "mlp_pull_m16_h256_d4_c4"


def test_record_floats():
    L = _native.lib()
    assert L.ff_mlp_record_floats(37, 20, 5) == 37 * 20 * 5
    assert L.ff_mlp_record_floats(1 << 16, 400, 16) == (1 << 16) * 400 * 16          # 1.7 GB: past 2^31 bytes, no wrap
    assert L.ff_mlp_record_floats(0, 4, 4) == 0 and L.ff_mlp_record_floats(3, 0, 4) == 0
    assert L.ff_mlp_record_floats(-1, 4, 4) == 0 and L.ff_mlp_record_floats(3, -2, 4) == 0 and L.ff_mlp_record_floats(3, 2, -4) == 0


def _args(buf, mode, count=0):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of
    the empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count = 0, 1, mode, count
    return a


def test_every_refusal_of_the_two_launches_without_a_gpu():
    L = _native.lib()
    buf = torch.zeros(64)
    ptr = buf.data_ptr()
    pull = _native.make_pull_plan(16, 4, [256] * 4)
    plain = _native.make_pull_plan(16, 0, [128])
    H, ST = _native.MODE_HUTCH, _native.MODE_STATE
    record = lambda plan, a, rec=ptr: L.ff_mlp_ode_launch_record(ctypes.byref(plan), ctypes.byref(a), rec, None)
    disc = lambda plan, a, rec=ptr, w=ptr, gx=ptr, gc=None: L.ff_mlp_ode_launch_pull_discrete(
        ctypes.byref(plan), ctypes.byref(a), rec, w, gx, gc, None)
    # what passes
    assert record(pull, _args(buf, ST)) == OK and record(plain, _args(buf, ST)) == OK
    for count in (1, 2, 7, 15):
        assert disc(pull, _args(buf, H, count)) == OK, count
        assert disc(pull, _args(buf, H, count), gc=ptr) == OK, count
        assert disc(plain, _args(buf, H, count)) == OK, count
    # the discrete launch ignores x_in / x_out
    a = _args(buf, H, 3)
    a.x_in = a.x_out = 0
    assert disc(pull, a) == OK
    # K < 1 or K > tile - 1; the wrong mode
    for count in (0, -1, 16, 40):
        assert disc(pull, _args(buf, H, count)) == BAD, count
    for mode in (ST, _native.MODE_EXACT, 7):
        assert disc(pull, _args(buf, mode, 3)) == BAD, mode
    for mode in (H, _native.MODE_EXACT, 7):
        assert record(pull, _args(buf, mode, 1)) == BAD, mode
    # NULL required pointers; no arguments; cot_cond_out without conditional inputs
    assert record(pull, _args(buf, ST), rec=None) == BAD
    for null in ("rec", "w", "gx"):
        assert disc(pull, _args(buf, H, 3), **{null: None}) == BAD, null
    assert L.ff_mlp_ode_launch_record(ctypes.byref(pull), None, ptr, None) == BAD
    assert L.ff_mlp_ode_launch_pull_discrete(ctypes.byref(pull), None, ptr, ptr, ptr, None, None) == BAD
    assert disc(plain, _args(buf, H, 3), gc=ptr) == BAD
    # the divergence side, attempt launches, the Jacobian output, noise, probes
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out", "probe"):
        a, b = _args(buf, H, 3), _args(buf, ST)
        setattr(a, field, ptr)
        setattr(b, field, ptr)
        assert disc(pull, a) == BAD and record(pull, b) == BAD, field
    a, b = _args(buf, H, 3), _args(buf, ST)
    for args in (a, b):
        args.n_aux = 1
        args.aux_out[0] = ptr
    assert disc(pull, a) == BAD and record(pull, b) == BAD
    # missing inputs
    for field in ("wpack", "etab", "cond"):
        a, b = _args(buf, H, 3), _args(buf, ST)
        setattr(a, field, 0)
        setattr(b, field, 0)
        assert disc(pull, a) == BAD and record(pull, b) == BAD, field
    for field in ("x_in", "x_out"):
        b = _args(buf, ST)
        setattr(b, field, 0)
        assert record(pull, b) == BAD, field
    # a depth whose stash does not fit at this K: a plan the planner would have refused, forged.  The adjoint slots hold dregs
    # words, not dregs + cregs, so the depth the pull launch refuses at K = 1 (19) still fits here and 20 does not: 8 samples x
    # 20 x 256 words = 160 KiB of stash alone.  (The record launch keeps no stash: it takes any depth.)
    deep = _native.PlanStruct.from_buffer_copy(pull)
    deep.n_hidden = 19
    assert L.ff_mlp_ode_launch_pull(ctypes.byref(deep), ctypes.byref(_args(buf, H, 1)), ptr, ptr, None, None) == UNS
    assert disc(deep, _args(buf, H, 1)) == OK
    deep.n_hidden = 20
    assert disc(deep, _args(buf, H, 1)) == UNS
    assert disc(deep, _args(buf, H, 3)) == OK                           # (4 samples per tile: half the stash)
    assert record(deep, _args(buf, ST)) == OK
    # a plan that is not a pull plan; a split-precision plan; a forged index
    for mode in (H, ST, _native.MODE_EXACT):
        plan = _native.make_plan(16, 4, [256] * 4, mode)
        assert disc(plan, _args(buf, H, 3)) == BAD and record(plan, _args(buf, ST)) == BAD
    push = _native.make_push_plan(16, 4, [256] * 4)
    assert disc(push, _args(buf, H, 3)) == BAD and record(push, _args(buf, ST)) == BAD
    for select in (False, True):
        pair = _native.make_pair_plan(8, 0, [128, 128], select=select)
        assert disc(pair, _args(buf, H, 3)) == BAD and record(pair, _args(buf, ST)) == BAD
    split = _native.make_plan(16, 0, [256] * 4, H, precision=_native.PREC_BF16X2)
    assert disc(split, _args(buf, H, 1)) == UNS and record(split, _args(buf, ST)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(pull)
    forged.kernel_id = _native.PULL_KERNEL_BASE + 3
    assert disc(forged, _args(buf, H, 3)) == BAD and record(forged, _args(buf, ST)) == BAD
    for base in (_native.REC_KERNEL_BASE, _native.DADJ_KERNEL_BASE):    # no plan carries the new ids
        forged.kernel_id = base
        assert disc(forged, _args(buf, H, 3)) == BAD and record(forged, _args(buf, ST)) == BAD
    # handing a pull plan to the existing launches behaves as before
    a = _args(buf, H, 3)
    a.dlogp_out = a.probe = ptr
    assert L.ff_mlp_ode_launch(ctypes.byref(pull), ctypes.byref(a), None) == BAD
    assert L.ff_mlp_ode_launch(ctypes.byref(pull), ctypes.byref(_args(buf, ST)), None) == BAD
    assert L.ff_mlp_ode_launch_pull(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), ptr, ptr, None, None) == OK
    assert L.ff_mlp_ode_launch_vjp(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), ptr, 0, ptr, None) == OK


# ---- the ops ---------------------------------------------------------------------------------------------------------------------
def test_the_two_ops_are_registered_with_fakes():
    rec_op, disc_op = torch.ops.flowfusion_amd.mlp_ode_record, torch.ops.flowfusion_amd.mlp_ode_pull_discrete
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_pull_plan(16, 4, [256] * 4), 4)
    with FakeTensorMode():
        x, c, etab = torch.empty(9, 16), torch.empty(9, 4), torch.empty(12, 32 + 256)
        y, rec, st = rec_op(x, c, torch.empty(10), etab, None, None, None, None, plan)
        assert y.shape == (9, 16) and rec.shape == (12, 9, 16) and st.shape == (1,)
        gx, gc, st = disc_op(rec, c, torch.empty(9, 3, 16), torch.empty(10), etab, None, None, None, None, plan, True)
        assert gx.shape == (9, 3, 16) and gc.shape == (9, 3, 4) and st.shape == (1,)
        gx, gc, st = disc_op(rec, c, torch.empty(9, 5, 16), torch.empty(10), etab, None, None, None, None, plan, False)
        assert gx.shape == (9, 5, 16) and gc.shape == (9, 5, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        rec_op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(10), torch.zeros(12, 288), None, None, None, None, plan)
    with pytest.raises(RuntimeError, match="GPU"):
        disc_op(torch.zeros(12, 2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), torch.zeros(10), torch.zeros(12, 288), None, None,
                None, None, plan, True)


# ---- the front ends ----------------------------------------------------------------------------------------------------------------
def _score_model(D_=4, C=0, units=(64, 64), **kw):
    torch.manual_seed(3)
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=C, embedding_dimensions=8, units=list(units)), D.VPSDE(), **kw).eval()


def _fronts():
    torch.manual_seed(4)
    m, mc = _score_model().model, _score_model(C=2).model
    return [(_score_model(), 0), (_score_model(C=2), 2), (F.ODEFlow(4, [64, 64]), 0), (F.ConditionalODEFlow(4, 2, [64, 64]), 2),
            (D.PopulationModelDiffusion(model=m, sde=D.VPSDE(), method="rk4"), 0),
            (D.PopulationModelDiffusionConditional(model=mc, sde=D.VPSDE(), method="rk4"), 2)]


def _vjp(front, C, x, w, **kw):
    return front.flow_vjp(x, w, **kw) if C == 0 else front.flow_vjp(x, w, torch.randn(x.shape[0], C), **kw)


def test_the_keyword_is_keyword_only_defaults_to_continuous_and_is_documented():
    for cls in FRONTS:
        prm = inspect.signature(cls.flow_vjp).parameters
        assert prm["adjoint"].kind is inspect.Parameter.KEYWORD_ONLY and prm["adjoint"].default == "continuous", cls
        doc = " ".join(cls.flow_vjp.__doc__.split()).lower()
        for piece in ("continuous adjoint", "rk4 or better", "retrace", "step count", 'adjoint="discrete"', "exact discrete adjoint"):
            assert piece in doc, (cls, piece)
    from flowfusion_amd import odeint
    doc = " ".join(odeint.solve_pull_discrete.__doc__.split()).lower()
    for piece in ("discrete", "record", "probe_buffer_floats", "bitwise"):
        assert piece in doc, piece
    prm = inspect.signature(odeint.solve_pull_discrete).parameters
    assert list(prm)[:6] == ["front", "x", "t_span", "method", "options", "cotangents"] and "return_retrace" not in prm


def test_front_end_errors_of_the_discrete_route_come_before_the_device():
    x, w = torch.randn(5, 4), torch.randn(5, 3, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25}, adjoint="discrete")
    for front, C in _fronts():
        for adjoint in ("exact", "", None, True, "Discrete"):
            with pytest.raises(ValueError, match="adjoint"):
                _vjp(front, C, x, w, method="rk4", options={"step_size": 0.25}, adjoint=adjoint)
        with pytest.raises(ValueError, match="retrace"):
            _vjp(front, C, x, w, return_retrace=True, **fixed)
        for method in solvers.ALL_ADAPTIVE:
            with pytest.raises(ValueError) as info:
                _vjp(front, C, x, w, method=method, adjoint="discrete")
            for piece in ("adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}'):
                assert piece in str(info.value), (piece, str(info.value))
        with pytest.raises(ValueError, match="grid_constructor"):
            _vjp(front, C, x, w, method="rk4", options={"grid_constructor": lambda f, y, t: t}, adjoint="discrete")
        with pytest.raises(ValueError, match="perturb"):
            _vjp(front, C, x, w, method="rk4", options={"step_size": 0.5, "perturb": True}, adjoint="discrete")
        with pytest.raises(ValueError, match="at most 15"):
            _vjp(front, C, x, torch.randn(5, 16, 4), **fixed)
        for bad_w in (torch.randn(5, 3, 5), torch.randn(4, 3, 4), torch.randn(5, 4), torch.randn(5, 0, 4), None):
            with pytest.raises(ValueError):
                _vjp(front, C, x, bad_w, **fixed)
        with pytest.raises(ValueError, match="direction"):
            _vjp(front, C, x, w, direction="sideways", **fixed)
        if C:
            with pytest.raises(ValueError):
                front.flow_vjp(x, w, torch.randn(5, C + 1), **fixed)
            with pytest.raises(ValueError):
                front.flow_vjp(x, w, None, **fixed)
        # what passes the checks stops at the device: CPU tensors
        with pytest.raises(RuntimeError, match="GPU"):
            _vjp(front, C, x, w, **fixed)
        # ... on the default one-step grid too
        with pytest.raises(RuntimeError, match="GPU"):
            _vjp(front, C, x, w, adjoint="discrete")
    for prec in ("bf16x3", "bf16x2"):
        with pytest.raises(ValueError, match="precision='f32'"):
            _score_model(precision=prec).flow_vjp(x, w, **fixed)
    with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
        _score_model(units=(512, 512)).flow_vjp(x, w, **fixed)
    # what still raises, whatever the keyword
    torch.manual_seed(5)
    sym = S.SymplecticFlowModel(S.SymplecticMLP(2, 0, 8, [64, 64]), torch.zeros(2), torch.ones(2), None, None)
    with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
        sym.flow_vjp(torch.randn(5, 2), torch.randn(5, 3, 2), adjoint="discrete")
    fl = F.ODEFlow(4, [64, 64])
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        fl.sample(torch.randn(3, 4), gradients=True)
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        fl.solve_ode_forward(torch.randn(3, 4), adjoint=True)


# ---- the transposed row program, emulated on the host ------------------------------------------------------------------------------
class _Field:
    """A small float64 right-hand side in the kernels' form, rhs_e(y, c) = a_e y + b_e NET(y, c), with per-row a_e, b_e."""

    def __init__(self, n_rows, D_=3, C=2, H=7, seed=11):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        self.W1, self.Wc, self.b1, self.W2, self.b2 = rnd(D_, H), rnd(C, H), rnd(H), rnd(H, D_), rnd(D_)
        self.a, self.b = rnd(n_rows), rnd(n_rows)

    def net(self, y, c):
        return torch.nn.functional.silu(y @ self.W1 + c @ self.Wc + self.b1) @ self.W2 + self.b2


def _forward_rows(tab, field, x, c):
    """The forward row program of the issue on the rows of ``solvers.plan_ode``; returns (x_out, the stage states)."""
    k = [torch.zeros_like(x) for _ in range(solvers.MAX_SLOTS)]
    ys = []
    for e in range(int(tab.t_eval.numel())):
        y = x + sum(tab.cin[e, s].double() * k[s] for s in range(solvers.MAX_SLOTS))
        ys.append(y)
        k[int(tab.slot[e])] = field.a[e] * y + field.b[e] * field.net(y, c)
        if int(tab.flags[e]) & solvers.FLAG_STEP_END:
            x = x + sum(tab.cout[e, s].double() * k[s] for s in range(solvers.MAX_SLOTS))
    return x, ys


def _transposed_rows(tab, field, ys, c, w, clear_slot=True, step_end=True):
    """The four steps of the transposed program, last row first, on the recorded stage states ``ys``.  ``clear_slot`` /
    ``step_end``: the negative controls drop step 2's ``kb[slot] = 0`` / step 1."""
    xb = w.clone()
    kb = [torch.zeros_like(w) for _ in range(solvers.MAX_SLOTS)]
    gamma = torch.zeros_like(c)
    for e in reversed(range(int(tab.t_eval.numel()))):
        slot = int(tab.slot[e])
        if step_end and int(tab.flags[e]) & solvers.FLAG_STEP_END:                  # 1
            for s in range(solvers.MAX_SLOTS):
                kb[s] = kb[s] + tab.cout[e, s].double() * xb
        rb = kb[slot]                                                                # 2
        if clear_slot:
            kb[slot] = torch.zeros_like(rb)
        _, pull = torch.func.vjp(field.net, ys[e], c)                                # 3
        jy, jc = pull(rb)
        yb = field.a[e] * rb + field.b[e] * jy
        gamma = gamma + field.b[e] * jc
        xb = xb + yb                                                                 # 4
        for s in range(solvers.MAX_SLOTS):
            kb[s] = kb[s] + tab.cin[e, s].double() * yb
    return xb, gamma


@pytest.mark.parametrize("method", sorted(solvers.FIXED_METHODS))
@pytest.mark.parametrize("nsteps", [1, 2, 3])
@pytest.mark.parametrize("span", [(0.0, 1.0), (1.0, 0.001)])
def test_transposed_row_program_is_the_vjp_of_the_forward_row_program(method, nsteps, span):
    t_span = torch.tensor(span, dtype=torch.float32)
    tab = solvers.plan_ode(t_span, method, {"step_size": abs(span[1] - span[0]) / nsteps})
    E = int(tab.t_eval.numel())
    assert E == nsteps * solvers.resolve_method(method).stages
    field = _Field(E)
    g = torch.Generator().manual_seed(3)
    x, c, w = (torch.randn(4, n, generator=g, dtype=torch.float64) for n in (3, 2, 3))
    (x_out, ys), pull = torch.func.vjp(lambda xx, cc: _forward_rows(tab, field, xx, cc), x, c)
    gx, gc = pull((w, [torch.zeros_like(y) for y in ys]))
    ex, ec = _transposed_rows(tab, field, [y.detach() for y in ys], c, w)
    assert R.normalised_error(ex, gx) <= 1e-12 and R.normalised_error(ec, gc) <= 1e-12
    # the negative controls: each step left out misses by far more than rounding
    for drop in (dict(clear_slot=False), dict(step_end=False)):
        bx, bc = _transposed_rows(tab, field, [y.detach() for y in ys], c, w, **drop)
        if "clear_slot" in drop and nsteps == 1:
            continue                                # (one step: no row overwrites a slot that held an older value)
        assert max(R.normalised_error(bx, gx), R.normalised_error(bc, gc)) > 1e-6, (drop, method, nsteps)


# ---- the discrimination condition of the GPU file's cases --------------------------------------------------------------------------
def _gpu_cases():
    from tests.test_gpu_pullback_discrete import RAW_CASES, _id
    return [pytest.param(case, id=_id(case)) for case in RAW_CASES]


@pytest.mark.parametrize("case", _gpu_cases())
def test_every_gpu_case_tells_the_two_adjoints_apart(case):
    """Computed on the CPU with the GPU file's own set-up: the float64 CONTINUOUS reference misses the case's bar (22 fp32 floors
    of the discrete reference) by at least 100x on cot_x and on cot_cond, and every floor is at most 5e-5."""
    from tests.test_gpu_pullback_discrete import case_setup
    from tests.test_gpu_pushforward import FACTOR, fp32_floor
    _, smaps, (x, w, c), *_ = case_setup(case)
    d64, d32 = (DP.DiscretePullback(smaps[dt])(x, w, c) for dt in (torch.float64, torch.float32))
    cont = P.Pullback(smaps[torch.float64])(x, w, c)
    for i, what in ((1, "cot_x"), (2, "cot_cond")):
        if d64[i] is None:
            continue
        floor, gap = fp32_floor(d32[i], d64[i]), R.normalised_error(cont[i], d64[i])
        print(f"{what}: floor {floor:.2e}, continuous gap {gap:.2e} = {gap / (FACTOR * floor):.0f} bars")
        assert floor <= 5e-5, (what, floor)
        assert gap >= 100.0 * FACTOR * floor, (what, gap, floor)
