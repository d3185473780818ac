"""CPU tier of the flow-map pull-backs (ff_mlp_pull_plan, ff_mlp_pull_wpack, ff_mlp_ode_launch_pull; ``flow_vjp``): the entry
points and their signatures, every refusal of the launch's argument check without a GPU, the planner at the corners of its
three units and one step past them (a depth that overflows the slope stash included), the front ends' ValueErrors /
NotImplementedErrors from CPU-resident models, the seventh op's fake registration, the transposed pack emulated on the
host against ``torch.func.vjp`` of the network, and the float64 reference on its own: its gap to the discrete Jacobian
falls with the order of the method, and it matches central differences."""
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
from tests import _emulator as E
from tests import _pushforward_ref as R
from tests._deep_models import apply_gain

ROOT = Path(__file__).resolve().parent.parent
BAD, UNS, OK = _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED, _native.FF_OK
FRONTS = (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional)


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the reference on its own (the one test of this file that needs nothing the library adds) ------------------------------
def _cflow():
    torch.manual_seed(5)
    fl = F.ConditionalODEFlow(4, 2, [32, 32])
    x, c, w = torch.randn(5, 4), torch.randn(5, 2), torch.randn(5, 2, 4)
    return R.flow_params(fl), x, c, w


@pytest.mark.parametrize("method, order", [("euler", 1), ("rk4", 4)])
@pytest.mark.parametrize("direction", ["to_data", "to_base"])
def test_reference_converges_to_the_discrete_jacobian_and_matches_central_differences(method, order, direction):
    """float64, ConditionalODEFlow D = 4, C = 2, [32, 32], seed 5, B = 5.  The continuous adjoint and the derivative of the
    discrete map differ by the discretisation error, O(h^p): the gap must fall by at least 2^(p - 0.25) per halving of the
    step between 16, 32 and 64 steps (>= 1.68 for euler, >= 13.4 for rk4; measured 1.99-2.01 and 16.05-16.16)."""
    from tests import _pullback_ref as P
    prm, x, c, w = _cflow()
    gaps = []
    for n in (16, 32, 64):
        sm = R.SolverMap("flow", prm, direction, method, {"step_size": 1.0 / n}, dtype=torch.float64)
        y, Jx, Jc = sm.jacobian(x, c)
        x_out, gx, gc, retrace = P.Pullback(sm)(x, w, c)
        assert x_out.dtype == torch.float64 and gx.shape == (5, 2, 4) and gc.shape == (5, 2, 2) and retrace.shape == (5,)
        assert torch.allclose(x_out, y, rtol=0, atol=1e-14 * float(y.abs().max()))
        wJx, wJc = torch.einsum("bki,bij->bkj", w.double(), Jx), torch.einsum("bki,bij->bkj", w.double(), Jc)
        gaps.append(max(R.normalised_error(gx, wJx), R.normalised_error(gc, wJc)))
    print(f"{method} {direction}: gaps {gaps}")
    for coarse, fine in zip(gaps[:-1], gaps[1:]):
        assert coarse / fine >= 2.0 ** (order - 0.25), (method, direction, gaps)
    if method == "rk4":
        # 64 rk4 steps: central differences of sum(w * x_out), step 1e-6 (truncation 1e-12, rounding 1e-10 of the scale;
        # the discretisation gap above is 2.5e-13): 1e-7 as in the push-forward reference's own check
        smap, k = sm, 0
        f = lambda xx, cc: (smap(xx, cc) * w[:, k].double()).sum(dim=1)
        h, xd, cd = 1e-6, x.double(), c.double()
        fx = torch.stack([(f(xd + h * e, cd) - f(xd - h * e, cd)) / (2 * h) for e in torch.eye(4, dtype=torch.float64)], dim=1)
        fc = torch.stack([(f(xd, cd + h * e) - f(xd, cd - h * e)) / (2 * h) for e in torch.eye(2, dtype=torch.float64)], dim=1)
        assert R.normalised_error(gx[:, k], fx) < 1e-7 and R.normalised_error(gc[:, k], fc) < 1e-7


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    L = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert ("int ff_mlp_pull_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision, "
            "ff_mlp_plan_t* plan_out);") in header
    assert "size_t ff_mlp_pull_wpack_floats(const ff_mlp_plan_t* plan);" in header
    assert ("int ff_mlp_pull_wpack(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b, const int* hidden_widths, "
            "int in_features0, int x_col0, int c_col0, float* out);") in header
    assert ("int ff_mlp_ode_launch_pull(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cotangent_in "
            "/* [batch, K, dim] */, float* cot_x_out /* [batch, K, dim] */, float* cot_cond_out /* [batch, K, cond_dim] or NULL */, "
            "void* hip_stream);") in header
    assert "#define FF_PULL_KERNEL_BASE 0x50000" in header
    assert L.ff_mlp_ode_launch_pull.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs),
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # the new pointers are arguments, not fields of ff_ode_args (tests/test_abi.py pins the struct itself)
    assert [f[0] for f in _native.OdeArgs._fields_][-1] == "gate"
    # a family of its own: three units, none of them in the ff_kernel_count / ff_kernel_name table or in the push table
    assert L.ff_pull_kernel_count() == 3
    names = [L.ff_pull_kernel_name(i).decode() for i in range(3)]
    assert names == ["mlp_pull_m16_h128_d4_c4", "mlp_pull_m16_h256_d4_c4", "mlp_pull_m16_h256_d8_c4"]
    assert L.ff_pull_kernel_name(3) is None and L.ff_pull_kernel_name(-1) is None
    table = {L.ff_kernel_name(i).decode() for i in range(L.ff_kernel_count())}
    table |= {L.ff_push_kernel_name(i).decode() for i in range(L.ff_push_kernel_count())}
    assert not table & set(names) and not any("pull" in n for n in table)


def _plan(dim, cond, hidden, act=_native.ACT_SILU, prec=_native.PREC_F32):
    p = _native.PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    rc = _native.lib().ff_mlp_pull_plan(dim, cond, len(hidden), arr, act, prec, ctypes.byref(p))
    return rc, p


@pytest.mark.parametrize("dim, cond, hidden, index", [
    (1, 0, [1], 0), (16, 16, [128] * 4, 0), (4, 0, [128] * 36, 0),
    (1, 0, [129], 1), (16, 16, [256] * 4, 1), (3, 1, [64, 200], 1), (16, 0, [256] * 18, 1),
    (17, 0, [1], 2), (32, 16, [256] * 4, 2), (17, 16, [128], 2), (32, 0, [256] * 17, 2),
])
def test_planner_picks_the_smallest_unit_at_its_corners(dim, cond, hidden, index):
    rc, p = _plan(dim, cond, hidden)
    assert rc == OK
    assert p.kernel_id == _native.PULL_KERNEL_BASE + index and p.tile == 16 and p.precision == _native.PREC_F32
    assert (p.width, p.dregs, p.cregs) == [(128, 4, 4), (256, 4, 4), (256, 8, 4)][index]
    assert (p.dim, p.cond_dim, p.n_hidden, p.activation) == (dim, cond, len(hidden), _native.ACT_SILU)
    assert _native.kernel_name(p) == _native.lib().ff_pull_kernel_name(index).decode()
    assert _native.is_pull_plan(p) and not _native.is_push_plan(p) and not _native.is_pair_plan(p) and not _native.is_select_plan(p)
    L = _native.lib()
    # two packs: the forward network's (the push plan's of the shape) and the transposed network's, which is larger where the
    # output layer of dregs + cregs registers needs more chunks
    rcp, push = R_push_plan(dim, cond, hidden)
    fwd = L.ff_mlp_wpack_floats(ctypes.byref(push))
    assert rcp == OK and L.ff_mlp_pull_wpack_floats(ctypes.byref(p)) >= 2 * fwd and L.ff_mlp_wpack_floats(ctypes.byref(p)) == 0
    assert L.ff_mlp_pull_wpack_floats(ctypes.byref(push)) == 0
    assert _native.row_width(p) == p.width


def R_push_plan(dim, cond, hidden):
    p = _native.PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    return _native.lib().ff_mlp_push_plan(dim, cond, len(hidden), arr, 0, 0, ctypes.byref(p)), p


def test_planner_refuses_one_step_past_the_envelope():
    for args in ((33, 0, [64]), (1, 17, [64]), (1, 0, [257]), (16, 0, [128, 257])):
        assert _plan(*args)[0] == UNS, args
    # a depth whose K = 1 stash (8 samples x n_hidden x width x 4 bytes) and stage slots overflow 160 KiB of LDS
    for args in ((4, 0, [128] * 37), (16, 0, [256] * 19), (32, 0, [256] * 18), (17, 0, [128] * 35 + [129])):
        assert _plan(*args)[0] == UNS, args
    for act in range(1, 9):
        assert _plan(4, 0, [64], act=act)[0] == UNS, act
    for prec in (_native.PREC_BF16X3, _native.PREC_BF16X2):
        assert _plan(4, 0, [64], prec=prec)[0] == UNS
    for args in ((0, 0, [64]), (4, -1, [64]), (4, 0, [0])):
        assert _plan(*args)[0] == BAD, args
    assert _plan(4, 0, [64], act=9)[0] == BAD and _plan(4, 0, [64], prec=7)[0] == BAD
    arr = (ctypes.c_int * 1)(64)
    assert _native.lib().ff_mlp_pull_plan(4, 0, 1, arr, 0, 0, None) == BAD
    with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
        _native.make_pull_plan(33, 0, [64])
    with pytest.raises(NotImplementedError, match="160 KiB of LDS: 18 at width 256"):
        _native.make_pull_plan(4, 0, [256] * 19)


def _args(buf, mode=_native.MODE_HUTCH, count=1):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of
    the empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
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
    H = _native.MODE_HUTCH
    call = lambda plan, a, w=ptr, gx=ptr, gc=None: L.ff_mlp_ode_launch_pull(ctypes.byref(plan), ctypes.byref(a), w, gx, gc, None)
    # what passes: every K a tile holds, with and without the conditional output
    for count in (1, 2, 7, 15):
        assert call(pull, _args(buf, H, count)) == OK, count
        assert call(pull, _args(buf, H, count), gc=ptr) == OK, count
        assert call(plain, _args(buf, H, count)) == OK, count
    # K < 1 or K > tile - 1; a mode other than FF_MODE_HUTCH
    for count in (0, -1, 16, 40):
        assert call(pull, _args(buf, H, count)) == BAD, count
    for mode in (_native.MODE_STATE, _native.MODE_EXACT, 7):
        assert call(pull, _args(buf, mode, 3)) == BAD, mode
    # NULL cotangent_in / cot_x_out; no arguments; cot_cond_out without conditional inputs
    assert call(pull, _args(buf, H, 3), w=None) == BAD and call(pull, _args(buf, H, 3), gx=None) == BAD
    assert L.ff_mlp_ode_launch_pull(ctypes.byref(pull), None, ptr, ptr, None, None) == BAD
    assert call(plain, _args(buf, H, 3), gc=ptr) == BAD
    # the divergence side, attempt launches, the Jacobian output, noise, probes
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out", "probe"):
        a = _args(buf, H, 3)
        setattr(a, field, ptr)
        assert call(pull, a) == BAD, field
    a = _args(buf, H, 3)
    a.n_aux = 1
    a.aux_out[0] = ptr
    assert call(pull, a) == BAD
    # missing inputs
    for field in ("x_in", "x_out", "wpack", "etab", "cond"):
        a = _args(buf, H, 3)
        setattr(a, field, 0)
        assert call(pull, a) == BAD, field
    # a depth whose stash does not fit: a plan the planner would have refused, forged
    deep = _native.PlanStruct.from_buffer_copy(pull)
    deep.n_hidden = 19
    assert call(deep, _args(buf, H, 1)) == UNS
    assert call(deep, _args(buf, H, 3)) == OK                           # (4 samples per tile: half the stash)
    # a plan that is not a pull plan; a split-precision plan; a forged index
    for mode in (_native.MODE_HUTCH, _native.MODE_STATE, _native.MODE_EXACT):
        assert call(_native.make_plan(16, 4, [256] * 4, mode), _args(buf, H, 3)) == BAD
    assert call(_native.make_push_plan(16, 4, [256] * 4), _args(buf, H, 3)) == BAD
    for select in (False, True):
        assert call(_native.make_pair_plan(8, 0, [128, 128], select=select), _args(buf, H, 3)) == BAD
    split = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH, precision=_native.PREC_BF16X2)
    assert call(split, _args(buf, H, 1)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(pull)
    forged.kernel_id = _native.PULL_KERNEL_BASE + 3
    assert call(forged, _args(buf, H, 3)) == BAD
    # a pull plan launches through its own entry point only
    a = _args(buf, H, 3)
    a.dlogp_out = a.probe = ptr
    assert L.ff_mlp_ode_launch(ctypes.byref(pull), ctypes.byref(a), None) == BAD
    assert L.ff_mlp_ode_launch_probes(ctypes.byref(pull), ctypes.byref(a), ptr, None) == BAD
    assert L.ff_mlp_ode_launch_push(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), None, ptr, None) == BAD
    assert L.ff_mlp_ode_launch(ctypes.byref(pull), ctypes.byref(_args(buf, _native.MODE_STATE)), None) == BAD
    # ... and is packed by its own packer only
    one = (ctypes.c_void_p * 2)(ptr, ptr)
    hw = (ctypes.c_int * 1)(128)
    assert L.ff_mlp_wpack(ctypes.byref(plain), one, one, hw, 16, 0, 0, ptr) == BAD
    assert L.ff_mlp_pull_wpack(ctypes.byref(_native.make_push_plan(16, 0, [128])), one, one, hw, 16, 0, 0, ptr) == BAD


# ---- the op ----------------------------------------------------------------------------------------------------------------------
def test_seventh_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_pull
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_pull_plan(16, 4, [256] * 4), 4)
    with FakeTensorMode():
        x, c = torch.empty(9, 16), torch.empty(9, 4)
        y, gx, gc, st = op(x, c, torch.empty(9, 3, 16), torch.empty(10), torch.empty(12, 32 + 256), None, None, None, None, plan, True)
        assert y.shape == (9, 16) and gx.shape == (9, 3, 16) and gc.shape == (9, 3, 4) and st.shape == (1,)
        y, gx, gc, st = op(x, c, torch.empty(9, 5, 16), torch.empty(10), torch.empty(12, 288), None, None, None, None, plan, False)
        assert gx.shape == (9, 5, 16) and gc.shape == (9, 5, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), torch.zeros(10), torch.zeros(12, 288), None, None, None, None,
           plan, True)


# ---- the transposed pack, emulated on the host -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Dn, C, hidden", [
    (1, 0, [32]), (16, 1, [128] * 4), (17, 16, [256]), (32, 0, [256] * 4), (16, 16, [128, 32, 256, 32]), (32, 1, [32]),
    (1, 16, [128, 32, 32, 128]),
])
def test_forward_pack_then_transposed_pack_reproduce_the_vjp_of_the_network(Dn, C, hidden, gain=1.0):
    """What the kernel reads, decoded (tests/_emulator.py) and run in float64 the way the kernel runs it: net A from the
    first pack gives the slopes, net B from the second pack -- first layer on [alpha | 0], a multiply by the slope after
    every layer, output rows = the state dimensions and the conditional inputs at the places of net A's registers -- must
    give J_net^T alpha and (dNET/dc)^T alpha of the network itself (torch.func.vjp).  ``gain`` (tests/_deep_models.py): the
    hidden-to-hidden weights times it, for the deep shapes of tests/test_derivative_depth_host.py."""
    torch.manual_seed(Dn * 100 + C)
    sizes = [Dn + C + 3] + list(hidden) + [Dn]                       # first layer input: [3 time columns | x | cond]
    lin = [nn.Linear(a, b) for a, b in zip(sizes[:-1], sizes[1:])]
    apply_gain(lin, gain)
    x_col0, c_col0 = 3, 3 + Dn
    plan = _native.make_pull_plan(Dn, C, list(hidden))
    pack = _native.pack_weights(plan, [l.weight for l in lin], [l.bias for l in lin], list(hidden), x_col0, c_col0)
    assert pack.numel() == _native.lib().ff_mlp_pull_wpack_floats(ctypes.byref(plan))
    words = _native.plan_words(plan, 0)
    push_words = _native.plan_words(_native.make_push_plan(Dn, C, list(hidden)), 0)
    nA = _native.lib().ff_mlp_wpack_floats(ctypes.byref(_native.make_push_plan(Dn, C, list(hidden))))
    tile, dregs, cregs = plan.tile, plan.dregs, plan.cregs
    NQ = 64 // tile
    W1, hid, Wo, bo, dx = E.decode_wpack(push_words, pack[:nA])
    wordsB = list(words)
    wordsB[0], wordsB[1], wordsB[4], wordsB[5] = NQ * (dregs + cregs), 0, dregs + cregs, 0
    T1, thid, To, tb, _ = E.decode_wpack(wordsB, pack[nA:])
    assert tb.abs().sum() == 0 and all(b.abs().sum() == 0 for _, b in thid)         # no biases
    # the place of conditional input j in net B's combined feature space
    cplace = {E.feat_of_reg(tile, r, q): E.feat_of_reg(tile, dregs + r, q) for r in range(cregs) for q in range(NQ)}
    B = 3
    y, c, alpha = torch.randn(B, Dn).double(), torch.randn(B, C).double(), torch.randn(B, Dn).double()
    tcols = torch.randn(3).double()
    c1 = lin[0].bias.double() + lin[0].weight.double()[:, :3] @ tcols                # what an evaluation row carries
    H = plan.width
    c1p = torch.zeros(H, dtype=torch.float64)
    c1p[:hidden[0]] = c1
    # net A, as the kernel: pre-activations, values, slopes
    silu = lambda a: a * torch.sigmoid(a)
    slope = lambda a: torch.sigmoid(a) * (1 + a * (1 - torch.sigmoid(a)))
    pre = y @ W1[:, :Dn].T + (c @ W1[:, dx:dx + C].T if C else 0.0) + c1p
    slopes, h = [slope(pre)], silu(pre)
    for Wl, bl in hid:
        pre = h @ Wl.T + bl
        slopes.append(slope(pre))
        h = silu(pre)
    net = (h @ Wo.T + bo)[:, :Dn]
    # net B on [alpha | 0]
    op = torch.zeros(B, T1.shape[1], dtype=torch.float64)
    op[:, :Dn] = alpha
    v = (op @ T1.T) * slopes[-1]
    for (Wl, _), s in zip(thid, reversed(slopes[:-1])):
        v = (v @ Wl.T) * s
    out = v @ To.T
    # the network itself
    def f(yy, cc):
        t = tcols.expand(B, 3)
        hcur = torch.cat([t, yy, cc], dim=1)
        for l in lin[:-1]:
            hcur = nn.functional.silu(hcur @ l.weight.double().T + l.bias.double())
        return hcur @ lin[-1].weight.double().T + lin[-1].bias.double()
    want, pull = torch.func.vjp(f, y, c)
    gy, gc = pull(alpha)
    scale = float(gy.detach().abs().max())
    assert torch.allclose(net, want.detach(), rtol=0, atol=1e-6 * float(want.detach().abs().max()))     # (fp32 weights in a float64 run)
    assert torch.allclose(out[:, :Dn], gy.detach(), rtol=0, atol=1e-6 * scale)
    if C:
        got_c = torch.stack([out[:, cplace[j]] for j in range(C)], dim=1)
        assert torch.allclose(got_c, gc.detach(), rtol=0, atol=1e-6 * max(scale, float(gc.detach().abs().max())))
    # every other row of net B's output is a structural zero
    used = set(range(Dn)) | {cplace[j] for j in range(C)}
    rest = [i for i in range(out.shape[1]) if i not in used]
    assert out[:, rest].abs().sum() == 0


# ---- the front ends' refusals ------------------------------------------------------------------------------------------------------
def _score_model(D_=4, C=0, units=(64, 64), act=None, **kw):
    torch.manual_seed(3)
    mk = {} if act is None else {"activation": act}
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=C, embedding_dimensions=8, units=list(units), **mk), D.VPSDE(),
                        **kw).eval()


def _fronts():
    torch.manual_seed(4)
    m, mc = _score_model().model, _score_model(C=2).model
    return [(_score_model(), 0), (_score_model(C=2), 2), (F.ODEFlow(4, [64, 64]), 0), (F.ConditionalODEFlow(4, 2, [64, 64]), 2),
            (D.PopulationModelDiffusion(model=m, sde=D.VPSDE(), method="rk4"), 0),
            (D.PopulationModelDiffusionConditional(model=mc, sde=D.VPSDE(), method="rk4"), 2)]


def _vjp(front, C, x, w, **kw):
    return front.flow_vjp(x, w, **kw) if C == 0 else front.flow_vjp(x, w, torch.randn(x.shape[0], C), **kw)


def test_method_exists_with_keyword_only_solver_arguments():
    for cls in FRONTS:
        prm = inspect.signature(cls.flow_vjp).parameters
        for key, default in (("direction", "to_data"), ("method", "rk4"), ("options", None), ("return_retrace", False)):
            assert prm[key].kind is inspect.Parameter.KEYWORD_ONLY and prm[key].default == default, (cls, key)
        assert list(prm)[1:3] == ["x", "cotangents"]
        doc = " ".join(cls.flow_vjp.__doc__.split())
        for piece in ("continuous adjoint", "rk4 or better", "retrace", "step count"):
            assert piece in doc.lower(), (cls, piece)


def test_front_end_value_errors_come_before_the_device():
    x, w = torch.randn(5, 4), torch.randn(5, 3, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    for front, C in _fronts():
        for method in solvers.ALL_ADAPTIVE:
            with pytest.raises(ValueError) as info:
                _vjp(front, C, x, w, method=method)
            for piece in ("adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}'):
                assert piece in str(info.value), (piece, str(info.value))
        with pytest.raises(ValueError, match="grid_constructor"):
            _vjp(front, C, x, w, method="rk4", options={"grid_constructor": lambda f, y, t: t})
        with pytest.raises(ValueError, match="perturb"):
            _vjp(front, C, x, w, method="rk4", options={"step_size": 0.5, "perturb": True})
        with pytest.raises(ValueError, match="at most 15"):
            _vjp(front, C, x, torch.randn(5, 16, 4), **fixed)
        for bad_w in (torch.randn(5, 3, 5), torch.randn(4, 3, 4), torch.randn(5, 4), torch.randn(5, 0, 4), None):
            with pytest.raises(ValueError):
                _vjp(front, C, x, bad_w, **fixed)
        with pytest.raises(ValueError):
            _vjp(front, C, torch.randn(5, 3), torch.randn(5, 3, 3), **fixed)
        with pytest.raises(ValueError, match="direction"):
            _vjp(front, C, x, w, direction="sideways", **fixed)
        if C:
            with pytest.raises(ValueError):
                front.flow_vjp(x, w, torch.randn(5, C + 1), **fixed)
            with pytest.raises(ValueError):
                front.flow_vjp(x, w, None, **fixed)                                          # the conditional is required
        # what passes the checks stops at the device: CPU tensors
        with pytest.raises(RuntimeError, match="GPU"):
            _vjp(front, C, x, w, **fixed)
    with pytest.raises(ValueError, match="conditional"):
        _score_model().flow_vjp(x, w, torch.randn(5, 2), **fixed)
    with pytest.raises(ValueError, match="conditional"):
        F.ODEFlow(4, [64, 64]).flow_vjp(x, w, torch.randn(5, 2), **fixed)
    for prec in ("bf16x3", "bf16x2"):
        with pytest.raises(ValueError, match="precision='f32'"):
            _score_model(precision=prec).flow_vjp(x, w, **fixed)
    with pytest.raises(ValueError, match="unknown ODE method"):
        _score_model().flow_vjp(x, w, method="rk5")


class _Foreign(nn.Module):
    def forward(self, t, x, conditional=None):
        return -x


def test_models_outside_the_envelope_raise_not_implemented():
    x, w = torch.randn(5, 4), torch.randn(5, 3, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    outside = [_score_model(units=(512, 512)), _score_model(act=nn.Tanh()), _score_model(D_=40), F.ODEFlow(4, [300]),
               F.ODEFlow(4, [64, 64], activation=nn.Tanh), F.ConditionalODEFlow(4, 17, [64]), F.ODEFlow(4, [256] * 19)]
    for front in outside:
        d = front.model.n_dimensions if hasattr(front, "model") else front.target_dimension
        c = getattr(front, "conditional_dimension", 0)
        xs, ws = torch.randn(5, d), torch.randn(5, 3, d)
        with pytest.raises(NotImplementedError, match="hidden widths up to 256") as info:
            front.flow_vjp(xs, ws, **fixed) if c == 0 else front.flow_vjp(xs, ws, torch.randn(5, c), **fixed)
        assert "up to 32 state dimensions" in str(info.value) and "15 cotangents" in str(info.value)
        assert "160 KiB of LDS" in str(info.value)
    with pytest.raises(NotImplementedError, match="hidden widths up to 256") as info:
        D.ScoreModel(_Foreign(), D.VPSDE()).flow_vjp(x, w, **fixed)
    assert "no module-path fallback" in str(info.value)
    torch.manual_seed(5)
    sym = S.SymplecticFlowModel(S.SymplecticMLP(2, 0, 8, [64, 64]), torch.zeros(2), torch.ones(2), None, None)
    with pytest.raises(NotImplementedError, match="hidden widths up to 256"):
        sym.flow_vjp(torch.randn(5, 2), torch.randn(5, 3, 2))


def test_the_reference_branches_that_still_raise_name_flow_vjp():
    fl, cf = F.ODEFlow(4, [64, 64]), F.ConditionalODEFlow(4, 2, [64, 64])
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        fl.sample(torch.randn(3, 4), gradients=True)
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        cf.sample(torch.randn(3, 4), torch.randn(3, 2), gradients=True)
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        fl.solve_ode_forward(torch.randn(3, 4), adjoint=True)
    with pytest.raises(NotImplementedError, match="flow_vjp"):
        cf.log_prob(torch.randn(3, 4), torch.randn(3, 2), adjoint=True)
