"""CPU tier of the flow-map sensitivities (ff_mlp_push_plan, ff_mlp_ode_launch_push; ``flow_jvp`` / ``flow_jacobian``):
the two entry points and their signatures, every refusal of the launch's argument check without a GPU, the planner at the
corners of its three units and one step past them, the front ends' ValueErrors / NotImplementedErrors from CPU-resident
models, the sixth op's fake registration, and the float64 reference on its own: jvp against jacfwd against central
differences."""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch
from torch import nn

from flowfusion_amd import _native, solvers
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd import symplectic as S
from tests import _pushforward_ref as R

ROOT = Path(__file__).resolve().parent.parent
BAD, UNS, OK = _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED, _native.FF_OK


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    L = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert ("int ff_mlp_push_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision, "
            "ff_mlp_plan_t* plan_out);") in header
    assert ("int ff_mlp_ode_launch_push(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cond_tangent "
            "/* [batch, K, cond_dim] or NULL */, float* tangent_out /* [batch, K, dim] */, void* hip_stream);") in header
    assert "#define FF_PUSH_KERNEL_BASE 0x40000" in header and "#define FF_STATUS_NOISE_ROW 4u" in header
    assert L.ff_mlp_push_plan.argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(_native.PlanStruct)]
    assert L.ff_mlp_ode_launch_push.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs),
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # the new pointers are arguments, not fields of ff_ode_args (tests/test_abi.py pins the struct itself)
    assert [f[0] for f in _native.OdeArgs._fields_][-1] == "gate"
    # a family of its own: three units, none of them in the ff_kernel_count / ff_kernel_name table
    assert L.ff_push_kernel_count() == 3
    names = [L.ff_push_kernel_name(i).decode() for i in range(3)]
    assert names == ["mlp_push_m16_h128_d4_c4_w3", "mlp_push_m16_h256_d4_c4_w2", "mlp_push_m16_h256_d8_c4_w2"]
    assert L.ff_push_kernel_name(3) is None and L.ff_push_kernel_name(-1) is None
    table = {L.ff_kernel_name(i).decode() for i in range(L.ff_kernel_count())}
    assert not table & set(names) and not any("push" in n for n in table)


def _plan(dim, cond, hidden, act=_native.ACT_SILU, prec=_native.PREC_F32):
    p = _native.PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = _native.lib().ff_mlp_push_plan(dim, cond, len(hidden), arr, act, prec, ctypes.byref(p))
    return rc, p


@pytest.mark.parametrize("dim, cond, hidden, index", [
    (1, 0, [1], 0), (16, 16, [128] * 4, 0),                 # width <= 128, dim <= 16, cond <= 16
    (1, 0, [129], 1), (16, 16, [256] * 4, 1), (3, 1, [64, 200], 1),
    (17, 0, [1], 2), (32, 16, [256] * 4, 2), (17, 16, [128], 2),
])
def test_planner_picks_the_smallest_unit_at_its_corners(dim, cond, hidden, index):
    rc, p = _plan(dim, cond, hidden)
    assert rc == OK
    assert p.kernel_id == _native.PUSH_KERNEL_BASE + index and p.tile == 16 and p.precision == _native.PREC_F32
    assert (p.width, p.dregs, p.cregs) == [(128, 4, 4), (256, 4, 4), (256, 8, 4)][index]
    assert (p.dim, p.cond_dim, p.n_hidden, p.activation) == (dim, cond, len(hidden), _native.ACT_SILU)
    assert _native.kernel_name(p) == _native.lib().ff_push_kernel_name(index).decode()
    assert _native.is_push_plan(p) and not _native.is_pair_plan(p) and not _native.is_select_plan(p)
    # the packed weights and the rows are those of any fp32 plan of the shape
    assert _native.row_width(p) == p.width and _native.lib().ff_mlp_wpack_floats(ctypes.byref(p)) > 0


def test_planner_refuses_one_step_past_the_envelope():
    for args in ((33, 0, [64]), (1, 17, [64]), (1, 0, [257]), (16, 0, [128, 257])):
        assert _plan(*args)[0] == UNS, args
    for act in range(1, 9):
        assert _plan(4, 0, [64], act=act)[0] == UNS, act
    for prec in (_native.PREC_BF16X3, _native.PREC_BF16X2):
        assert _plan(4, 0, [64], prec=prec)[0] == UNS
    for args in ((0, 0, [64]), (4, -1, [64]), (4, 0, [0])):
        assert _plan(*args)[0] == BAD, args
    assert _plan(4, 0, [64], act=9)[0] == BAD and _plan(4, 0, [64], prec=7)[0] == BAD
    arr = (ctypes.c_int * 1)(64)
    assert _native.lib().ff_mlp_push_plan(4, 0, 1, arr, 0, 0, None) == BAD
    with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
        _native.make_push_plan(33, 0, [64])


def _args(buf, mode=_native.MODE_HUTCH, count=0, first=0):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of
    the empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.probe = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count, a.tangent_first = 0, 1, mode, count, first
    return a


def test_every_refusal_of_the_launch_without_a_gpu():
    L = _native.lib()
    buf = torch.zeros(64)
    out = buf.data_ptr()
    push = _native.make_push_plan(16, 4, [256] * 4)                  # D + C = 20 unit directions
    plain = _native.make_push_plan(16, 0, [128])
    H, E = _native.MODE_HUTCH, _native.MODE_EXACT
    call = lambda plan, a, ct=None, to=out: L.ff_mlp_ode_launch_push(ctypes.byref(plan), ctypes.byref(a), ct, to, None)
    # what passes: every K a tile holds, tangents as given or unit ranges inside [0, D + C), NULL state tangents
    for count in (0, 1, 2, 7, 15):
        assert call(push, _args(buf, H, count)) == OK, count
        assert call(push, _args(buf, H, count), out) == OK, count
    for first, count in ((0, 15), (15, 5), (19, 1), (16, 4)):
        assert call(push, _args(buf, E, count, first)) == OK, (first, count)
    assert call(_native.make_push_plan(8, 4, [64]), _args(buf, E)) == OK       # count 0 = all 12 unit directions, which fit
    assert call(plain, _args(buf, E)) == BAD                             # ... all 16 do not: 16 + 1 > tile
    a = _args(buf, H, 3)
    a.probe = 0
    assert call(push, a, out) == OK
    # tangent_out NULL; no arguments
    assert call(push, _args(buf, H, 3), None, None) == BAD
    assert L.ff_mlp_ode_launch_push(ctypes.byref(push), None, None, out, None) == BAD
    # K < 1 or K + 1 > tile
    for mode, count in ((H, -1), (H, 16), (H, 40), (E, 16), (E, -1)):
        assert call(push, _args(buf, mode, count)) == BAD, (mode, count)
    assert call(push, _args(buf, E)) == BAD                             # count 0 = all 20 unit directions: more than a tile holds
    assert call(push, _args(buf, _native.MODE_STATE)) == BAD and call(push, _args(buf, 7)) == BAD
    # the divergence side, attempt launches, the Jacobian output, noise
    for field in ("dlogp_out", "k1_in", "kl1_in", "dlogp_in", "jac_out", "noise"):
        a = _args(buf, H, 3)
        setattr(a, field, buf.data_ptr())
        assert call(push, a) == BAD, field
    a = _args(buf, H, 3)
    a.n_aux = 1
    a.aux_out[0] = buf.data_ptr()
    assert call(push, a) == BAD
    # a unit range that reaches past D + C
    for first, count in ((20, 1), (15, 6), (-1, 2), (6, 15)):
        assert call(push, _args(buf, E, count, first)) == BAD, (first, count)
    assert call(plain, _args(buf, E, 1, 16)) == BAD                     # no conditional inputs: the space ends at D
    # conditional tangents without conditional inputs, or beside unit tangents
    assert call(plain, _args(buf, H, 3), out) == BAD
    assert call(push, _args(buf, E, 5, 15), out) == BAD
    # missing inputs
    for field in ("x_in", "x_out", "wpack", "etab", "cond"):
        a = _args(buf, H, 3)
        setattr(a, field, 0)
        assert call(push, a) == BAD, field
    # a plan that is not a push plan; a split-precision plan
    for mode in (_native.MODE_HUTCH, _native.MODE_STATE, _native.MODE_EXACT):
        assert call(_native.make_plan(16, 4, [256] * 4, mode), _args(buf, H, 3)) == BAD
    for select in (False, True):
        assert call(_native.make_pair_plan(8, 0, [128, 128], select=select), _args(buf, H, 3)) == BAD
    split = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH, precision=_native.PREC_BF16X2)
    assert call(split, _args(buf, H, 1)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(push)
    forged.kernel_id = _native.PUSH_KERNEL_BASE + 3
    assert call(forged, _args(buf, H, 3)) == BAD
    # a push plan launches through its own entry point only
    a = _args(buf, H, 3)
    a.dlogp_out = buf.data_ptr()
    assert L.ff_mlp_ode_launch(ctypes.byref(push), ctypes.byref(a), None) == BAD
    assert L.ff_mlp_ode_launch_probes(ctypes.byref(push), ctypes.byref(a), out, None) == BAD
    assert L.ff_mlp_ode_launch(ctypes.byref(push), ctypes.byref(_args(buf, _native.MODE_STATE)), None) == BAD


# ---- the op ----------------------------------------------------------------------------------------------------------------------
def test_sixth_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_push
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_push_plan(16, 4, [256] * 4), 4)
    with FakeTensorMode():
        x, c = torch.empty(9, 16), torch.empty(9, 4)
        y, dy, st = op(x, c, torch.empty(9, 3, 16), torch.empty(9, 3, 4), torch.empty(10), torch.empty(12, 32 + 256), None, None,
                       None, None, plan, False, 0, 3)
        assert y.shape == (9, 16) and dy.shape == (9, 3, 16) and st.shape == (1,)
        y, dy, st = op(x, c, None, None, torch.empty(10), torch.empty(12, 288), None, None, None, None, plan, True, 15, 5)
        assert dy.shape == (9, 5, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), None, torch.zeros(10), torch.zeros(12, 288), None, None,
           None, None, plan, False, 0, 3)


# ---- the front ends' refusals ------------------------------------------------------------------------------------------------------
def _score_model(D_=4, C=0, units=(64, 64), act=None, **kw):
    torch.manual_seed(3)
    mk = {} if act is None else {"activation": act}
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=C, embedding_dimensions=8, units=list(units), **mk), D.VPSDE(),
                        **kw).eval()


def _fronts():
    """(front end, its conditional dimension) of every class that carries the two methods."""
    torch.manual_seed(4)
    m, mc = _score_model().model, _score_model(C=2).model
    return [(_score_model(), 0), (_score_model(C=2), 2), (F.ODEFlow(4, [64, 64]), 0), (F.ConditionalODEFlow(4, 2, [64, 64]), 2),
            (D.PopulationModelDiffusion(model=m, sde=D.VPSDE(), method="rk4"), 0),
            (D.PopulationModelDiffusionConditional(model=mc, sde=D.VPSDE(), method="rk4"), 2)]


def _jvp(front, C, x, v, vc=None, **kw):
    if C == 0:
        return front.flow_jvp(x, v, **kw)
    return front.flow_jvp(x, v, torch.randn(x.shape[0], C), vc, **kw)


def _jac(front, C, x, **kw):
    return front.flow_jacobian(x, **kw) if C == 0 else front.flow_jacobian(x, torch.randn(x.shape[0], C), **kw)


def test_methods_exist_with_keyword_only_solver_arguments():
    for cls in (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional):
        for name in ("flow_jvp", "flow_jacobian"):
            prm = inspect.signature(getattr(cls, name)).parameters
            for key, default in (("direction", "to_data"), ("method", "rk4"), ("options", None)):
                assert prm[key].kind is inspect.Parameter.KEYWORD_ONLY and prm[key].default == default, (cls, name, key)
            assert list(prm)[1] == "x"


def test_front_end_value_errors_come_before_the_device():
    x, v = torch.randn(5, 4), torch.randn(5, 3, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    for front, C in _fronts():
        vc = torch.randn(5, 3, C) if C else None
        # adaptive methods: the message names the way out
        for method in solvers.ALL_ADAPTIVE:
            for call in (lambda: _jvp(front, C, x, v, vc, method=method), lambda: _jac(front, C, x, method=method)):
                with pytest.raises(ValueError) as info:
                    call()
                for piece in ("adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}'):
                    assert piece in str(info.value), (piece, str(info.value))
        # grid_constructor / perturb
        with pytest.raises(ValueError, match="grid_constructor"):
            _jvp(front, C, x, v, vc, method="rk4", options={"grid_constructor": lambda f, y, t: t})
        with pytest.raises(ValueError, match="perturb"):
            _jac(front, C, x, method="rk4", options={"step_size": 0.5, "perturb": True})
        # more tangents than a tile holds
        with pytest.raises(ValueError, match="at most 15"):
            _jvp(front, C, x, torch.randn(5, 16, 4), None, **fixed)
        # shapes that do not match
        for bad_v in (torch.randn(5, 3, 5), torch.randn(4, 3, 4), torch.randn(5, 4)):
            with pytest.raises(ValueError):
                _jvp(front, C, x, bad_v, None, **fixed)
        with pytest.raises(ValueError):
            _jvp(front, C, torch.randn(5, 3), torch.randn(5, 3, 3), None, **fixed)
        with pytest.raises(ValueError):
            _jvp(front, C, x, None, None, **fixed)                    # no direction at all
        with pytest.raises(ValueError, match="direction"):
            _jvp(front, C, x, v, vc, direction="sideways", **fixed)
        if C:
            with pytest.raises(ValueError):
                front.flow_jvp(x, v, torch.randn(5, C), torch.randn(5, 2, C), **fixed)      # K differs
            with pytest.raises(ValueError):
                front.flow_jvp(x, v, torch.randn(5, C + 1), None, **fixed)
            with pytest.raises(ValueError):
                front.flow_jvp(x, v, None, None, **fixed)                                    # the conditional is required
        # what passes the checks stops at the device: CPU tensors
        with pytest.raises(RuntimeError, match="GPU"):
            _jvp(front, C, x, v, vc, **fixed)
        with pytest.raises(RuntimeError, match="GPU"):
            _jac(front, C, x, **fixed)
    # an unconditional model handed a conditional
    with pytest.raises(ValueError, match="conditional"):
        _score_model().flow_jvp(x, v, torch.randn(5, 2), None, **fixed)
    with pytest.raises(ValueError, match="conditional"):
        F.ODEFlow(4, [64, 64]).flow_jacobian(x, torch.randn(5, 2), **fixed)
    # split precision
    for prec in ("bf16x3", "bf16x2"):
        with pytest.raises(ValueError, match="precision='f32'"):
            _score_model(precision=prec).flow_jvp(x, v, **fixed)
    # unknown method names keep their own error
    with pytest.raises(ValueError, match="unknown ODE method"):
        _score_model().flow_jvp(x, v, method="rk5")


class _Foreign(nn.Module):
    def forward(self, t, x, conditional=None):
        return -x


def test_models_outside_the_envelope_raise_not_implemented():
    x, v = torch.randn(5, 4), torch.randn(5, 3, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    outside = [_score_model(units=(512, 512)), _score_model(act=nn.Tanh()), _score_model(D_=40),
               F.ODEFlow(4, [300]), F.ODEFlow(4, [64, 64], activation=nn.Tanh), F.ConditionalODEFlow(4, 17, [64])]
    for front in outside:
        d = front.model.n_dimensions if hasattr(front, "model") else front.target_dimension
        c = getattr(front, "conditional_dimension", 0)
        xs, vs = torch.randn(5, d), torch.randn(5, 3, d)
        with pytest.raises(NotImplementedError, match="hidden widths up to 256") as info:
            front.flow_jvp(xs, vs, **fixed) if c == 0 else front.flow_jvp(xs, vs, torch.randn(5, c), **fixed)
        assert "up to 32 state dimensions" in str(info.value) and "15 tangents" in str(info.value)
    with pytest.raises(NotImplementedError, match="hidden widths up to 256") as info:
        D.ScoreModel(_Foreign(), D.VPSDE()).flow_jvp(x, v, **fixed)
    assert "no module-path fallback" in str(info.value)
    torch.manual_seed(5)
    sym = S.SymplecticFlowModel(S.SymplecticMLP(2, 0, 8, [64, 64]), torch.zeros(2), torch.ones(2), None, None)
    for call in (lambda: sym.flow_jvp(torch.randn(5, 2), torch.randn(5, 3, 2)), lambda: sym.flow_jacobian(torch.randn(5, 2))):
        with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
            call()


# ---- the reference on its own --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_reference_jvp_is_jacfwd_is_a_central_difference(direction):
    """float64, a 2-step rk4 VP model with conditional inputs: three routes to the same derivative."""
    torch.manual_seed(9)
    Dn, C, B, K = 3, 2, 4, 3
    m = D.MLP(n_dimensions=Dn, n_conditionals=C, embedding_dimensions=8, units=[32, 32])
    opts = {"step_size": (1.0 - 1e-3) / 2}
    ref = R.SolverMap("score", R.score_params(m), direction, "rk4", opts, dtype=torch.float64, sde="vp")
    x, v, c, vc = torch.randn(B, Dn), torch.randn(B, K, Dn), torch.randn(B, C), torch.randn(B, K, C)
    y, d = ref.jvp(x, v, c, vc)
    yj, Jx, Jc = ref.jacobian(x, c)
    assert y.dtype == torch.float64 and d.shape == (B, K, Dn) and Jx.shape == (B, Dn, Dn) and Jc.shape == (B, Dn, C)
    assert torch.allclose(y, yj, rtol=0, atol=1e-14 * float(y.abs().max()))
    Jv = torch.einsum("bij,bkj->bki", Jx, v.double()) + torch.einsum("bij,bkj->bki", Jc, vc.double())
    # two forward-mode evaluations of one float64 computation: rounding only (1e-16 per operation over a few hundred of them)
    assert R.normalised_error(Jv, d) < 1e-12
    # central differences of step h = 1e-6: truncation h^2 |f'''| / 6 ~ 1e-12 and rounding 1e-16 |f| / h ~ 1e-10 of the scale;
    # 1e-7 leaves three decades for the third derivative and the conditioning of a two-step solve
    assert R.normalised_error(ref.central_difference(x, v, c, vc, h=1e-6), d) < 1e-7
    # the parts alone, and the wrappers' maps: the chain rule's factors
    _, dx_only = ref.jvp(x, v, c, None)
    _, dc_only = ref.jvp(x, None, c, vc)
    assert R.normalised_error(dx_only + dc_only, d) < 1e-12
    shift, scale, cshift, cscale = torch.randn(Dn), torch.rand(Dn) + 0.5, torch.randn(C), torch.rand(C) + 0.5
    wrapped = R.SolverMap("score", R.score_params(m), direction, "rk4", opts, dtype=torch.float64, sde="vp",
                          affine=(shift, scale), cond_affine=(cshift, cscale))
    raw_c = c.double() * cscale.double() + cshift.double()
    xw = x.double() if direction == "to_data" else x.double() * scale.double() + shift.double()
    _, Jxw, Jcw = wrapped.jacobian(xw, raw_c)
    if direction == "to_data":
        want_x, want_c = Jx * scale.double()[None, :, None], Jc * scale.double()[None, :, None] / cscale.double()[None, None, :]
    else:
        want_x, want_c = Jx / scale.double()[None, None, :], Jc / cscale.double()[None, None, :]
    assert R.normalised_error(Jxw, want_x) < 1e-10 and R.normalised_error(Jcw, want_c) < 1e-10
