"""CPU tier of the leapfrog push-forwards (ff_mlp_push_select_plan, ff_mlp_push_select_wpack, ff_mlp_ode_launch_push_select;
``FusedPair.pushforward_select``, ``odeint.solve_leapfrog_push`` / ``solve_leapfrog_push_jacobian``, ``sample_leapfrog_jvp`` /
``sample_leapfrog_jacobian``): the conditions every case of tests/test_gpu_leapfrog_push.py meets on its references alone,
the entry points and their signatures, every refusal without a GPU, the planner at its corners, the op's fake registration,
the pack against two ``ff_mlp_wpack`` calls byte for byte, the methods' signatures and errors in their order.

The conditions (for every raw case, tests/_leapfrog_push_ref.py):
  * the fp32 floor is at most 5e-5;
  * the float64 reference misses the case's bar (FACTOR = 22 floors) by at least 100 x with two weight rows swapped in the
    first, a middle or the last hidden layer of mlp_q, likewise of mlp_p, with mlp_q and mlp_p exchanged, and, where C > 0,
    with the conditional-tangent path of either network dropped;
  * the float64 Jacobian of the reference map has determinant 1 to 1e-12 (a leapfrog of arbitrary MLPs is
    volume-preserving, not symplectic).
Of the front-end cases: the fp32 floor of the adjoint identity is at most 5e-5.

These reference-only conditions and the pinned messages of the four old methods hold without the feature; every other test
here needs it.
"""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import symplectic as Sm
from tests import _leapfrog_push_ref as L
from tests._pushforward_ref import normalised_error

ROOT = Path(__file__).resolve().parents[1]
OK, BAD, UNS = _native.FF_OK, _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED
NAMES = ["mlp_pushsel_m16_h128_d4_c4_w3", "mlp_pushsel_m16_h256_d4_c4_w2", "mlp_pushsel_m16_h256_d8_c4_w2"]


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the conditions of every case (reference only) -------------------------------------------------------------------------------
def damages_of(case):
    nh, C = len(case[2]), case[1]
    out = {}
    for n, name in ((0, "mlp_q"), (1, "mlp_p")):
        for layer in sorted({0, nh // 2, nh - 1}):
            out[f"rows 0, 1 of hidden layer {layer} of {name} swapped"] = L.Damage(swap=(n, layer, (0, 1)))
    out["mlp_q and mlp_p exchanged"] = L.Damage(exchange=True)
    if C > 0:
        out["conditional tangents of mlp_q dropped"] = L.Damage(drop_gamma=0)
        out["conditional tangents of mlp_p dropped"] = L.Damage(drop_gamma=1)
    return out


@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_floor_is_small_and_every_damage_misses_the_bar_by_100(case):
    floor, sfloor, (zo, dz) = L.raw_floor_and_reference(case)
    assert floor <= 5e-5 and sfloor <= 5e-5, (floor, sfloor)
    bar = L.FACTOR * floor
    worst = None
    for what, damage in damages_of(case).items():
        miss = normalised_error(L.raw_reference(case, torch.float64, damage)[1], dz) / bar
        worst = (miss, what) if worst is None or miss < worst[0] else worst
        assert miss >= 100.0, (what, miss)
    print(f"\n[leapfrog_push] {L.case_id(case)}: floor {floor:.2e}, smallest miss {worst[0]:.0f} x ({worst[1]})")


@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_float64_jacobian_of_the_reference_map_has_determinant_one(case):
    front, plan, rows, z, v, cond, vc = L.case_setup(case)
    ref = L.LeapfrogRef(front, torch.float64)
    J = L.jacobian_rows(ref, z, cond, rows)
    assert float((torch.linalg.det(J) - 1.0).abs().max()) <= 1e-12
    # and J times a tangent is the jvp of that tangent
    dz = L.jvp_rows(ref, z, cond, rows, v, None)[1]
    assert float((torch.einsum("bij,bkj->bki", J, v.double()) - dz).abs().max()) <= 1e-12 * max(1.0, float(dz.abs().max()))


@pytest.mark.parametrize("case", L.SAMPLE_CASES, ids=L.front_id)
def test_adjoint_identity_floor_is_small(case):
    floor = L.adjoint_floor(case)
    assert floor <= 5e-5, floor
    # in float64 the two legs agree to rounding
    front, z, v, cond, vc, w = L.front_inputs(case)
    _, dx = L.sample_jvp_ref(front, z, v, cond, vc, case[4])
    _, gz, gc = L.P.sample_vjp_ref(front, z, w, cond, case[4])
    assert L.adjoint_gap(w, dx, gz, v, gc, vc) <= 1e-13


def test_cases_cover_what_they_must():
    raw = L.RAW_CASES
    assert len(raw) == 11 and [tuple(c) for c in raw[:10]] == [tuple(c[:7]) for c in L.P.RAW_CASES[:10]]
    assert {c[5] for c in raw} >= {1, 2, 4, 7, 15} and {c[6] for c in raw} >= {1, 17}
    assert {c[4] for c in raw} >= {1, 2, 3, "hand"} and sum(len(c) > 7 for c in raw) == 1
    for c in raw:
        assert c[6] in (1, 17, 16 // (1 + c[5]) + 1)
    assert [nb for _, _, nb in L.plan_rows(L.hand_plan())] == [False, False, True, True, False]
    for steps in (1, 2, 3):          # the forward rows: 2 steps + 1, first and last on mlp_p, weights negative (t runs down)
        rows = L.plan_rows(L.case_plan((1, 0, [32], 1.0, steps, 1, 1)))
        assert len(rows) == 2 * steps + 1 and rows[0][2] and rows[-1][2] and all(float(w) < 0 for _, w, _ in rows)
    for i, case in enumerate(raw):
        assert _native.kernel_name(_native.make_push_select_plan(2 * case[0], case[1], case[2])) == L.UNIT_OF[i]
    assert set(L.UNIT_OF.values()) == set(NAMES)


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    lib = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert "#define FF_PUSH_SELECT_KERNEL_BASE 0xB0000" in header and _native.PUSH_SELECT_KERNEL_BASE == 0xB0000
    assert "int ff_pushsel_kernel_count(void);" in header and "const char* ff_pushsel_kernel_name(int index);" in header
    assert "int ff_mlp_push_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);" in header
    assert "size_t ff_mlp_push_select_wpack_floats(const ff_mlp_plan_t* plan);" in header
    assert ("int ff_mlp_push_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq, "
            "const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0, int x_col0, int c_col0, "
            "float* out);") in header
    assert ("int ff_mlp_ode_launch_push_select(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cond_tangent "
            "/* [batch, K, cond_dim] or NULL */, float* tangent_out /* [batch, K, dim] */, void* hip_stream);") in header
    assert lib.ff_pushsel_kernel_count() == 3
    assert [lib.ff_pushsel_kernel_name(i).decode() for i in range(3)] == NAMES
    assert lib.ff_pushsel_kernel_name(3) is None and lib.ff_pushsel_kernel_name(-1) is None
    # a family of its own: none of the other tables lists it, and the push table is what it was
    for count, name in ((lib.ff_kernel_count, lib.ff_kernel_name), (lib.ff_push_kernel_count, lib.ff_push_kernel_name),
                        (lib.ff_pull_kernel_count, lib.ff_pull_kernel_name), (lib.ff_pullsel_kernel_count, lib.ff_pullsel_kernel_name),
                        (lib.ff_pair_kernel_count, lib.ff_pair_kernel_name)):
        assert not any(b"pushsel" in name(i) for i in range(count()))
    assert [lib.ff_push_kernel_name(i).decode() for i in range(lib.ff_push_kernel_count())] == [n.replace("pushsel", "push") for n in NAMES]
    assert lib.ff_mlp_ode_launch_push_select.argtypes == lib.ff_mlp_ode_launch_push.argtypes
    assert "hidden widths up to 256" in _native.PUSH_SELECT_ENVELOPE and "32 dimensions" in _native.PUSH_SELECT_ENVELOPE


def _plan(dim, cond, hidden):
    p = _native.PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    return _native.lib().ff_mlp_push_select_plan(dim, cond, len(hidden), arr, ctypes.byref(p)), p


def test_planner_at_its_corners():
    lib = _native.lib()
    for dim, cond, hidden, name in ((2, 0, [1], "h128_d4_c4_w3"), (16, 16, [128] * 40, "h128_d4_c4_w3"), (16, 0, [129], "h256_d4_c4_w2"),
                                    (16, 16, [256] * 30, "h256_d4_c4_w2"), (18, 0, [128], "h256_d8_c4_w2"),
                                    (32, 16, [256] * 30, "h256_d8_c4_w2")):
        rc, p = _plan(dim, cond, hidden)
        assert rc == OK and _native.kernel_name(p) == f"mlp_pushsel_m16_{name}", (dim, cond, hidden)
        assert _native.is_push_select_plan(p) and p.kernel_id >= _native.PUSH_SELECT_KERNEL_BASE
        assert not (_native.is_pull_select_plan(p) or _native.is_pull_plan(p) or _native.is_push_plan(p) or _native.is_pair_plan(p)
                    or _native.is_select_plan(p))
        # four tiles per workgroup, as the push units: 4 x 16 // (1 + K)
        assert _native.row_width(p) == p.width and _native.samples_per_workgroup(p, _native.MODE_HUTCH) == 32
        # the shape is the push plan's of the joint state; the pack is two of its packs; the other size queries answer 0
        push = _native.make_push_plan(dim, cond, hidden)
        assert (push.tile, push.width, push.dregs, push.cregs, push.n_hidden) == (p.tile, p.width, p.dregs, p.cregs, p.n_hidden)
        assert lib.ff_mlp_push_select_wpack_floats(ctypes.byref(p)) == 2 * lib.ff_mlp_wpack_floats(ctypes.byref(push))
        for other in (lib.ff_mlp_wpack_floats, lib.ff_mlp_pair_wpack_floats, lib.ff_mlp_pull_wpack_floats,
                      lib.ff_mlp_pull_select_wpack_floats):
            assert other(ctypes.byref(p)) == 0
        assert lib.ff_mlp_push_select_wpack_floats(ctypes.byref(push)) == 0
    # the existing pull-select plans are still told apart
    ps = _native.make_pull_select_plan(16, 4, [256] * 4)
    assert _native.is_pull_select_plan(ps) and not _native.is_push_select_plan(ps)
    assert lib.ff_mlp_push_select_wpack_floats(ctypes.byref(ps)) == 0
    for args in ((3, 0, [64]), (17, 0, [64]), (0, 0, [64]), (4, -1, [64]), (4, 0, [0]), (4, 0, [])):
        assert _plan(*args)[0] == BAD, args
    for args in ((34, 0, [64]), (2, 17, [64]), (2, 0, [257])):
        assert _plan(*args)[0] == UNS, args
    arr = (ctypes.c_int * 1)(64)
    assert lib.ff_mlp_push_select_plan(4, 0, 1, arr, None) == BAD
    assert lib.ff_mlp_push_select_plan(4, 0, 1, None, ctypes.byref(_native.PlanStruct())) == BAD
    with pytest.raises(NotImplementedError, match="16 per half"):
        _native.make_push_select_plan(34, 0, [64])


def _args(buf, mode=_native.MODE_HUTCH, count=1):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of the
    empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count, a.stage_slots = 0, 1, mode, count, 1
    return a


def test_every_refusal_of_the_launch_and_the_packers_without_a_gpu():
    lib = _native.lib()
    buf = torch.zeros(64)
    ptr = buf.data_ptr()
    sel = _native.make_push_select_plan(16, 4, [256] * 4)
    plain = _native.make_push_select_plan(16, 0, [128])
    push = _native.make_push_plan(16, 4, [256] * 4)
    H, X = _native.MODE_HUTCH, _native.MODE_EXACT
    call = lambda plan, a, vc=None, out=ptr: lib.ff_mlp_ode_launch_push_select(ctypes.byref(plan), ctypes.byref(a), vc, out, None)
    ref = lambda a, vc=None, out=ptr: lib.ff_mlp_ode_launch_push(ctypes.byref(push), ctypes.byref(a), vc, out, None)
    # the modes and refusals of ff_mlp_ode_launch_push, answer for answer
    trials = []
    for count in (0, 1, 2, 7, 15, 16, -1, 40):
        trials += [(H, count, None, {}), (H, count, ptr, {}), (X, count, None, {}), (X, count, ptr, {})]
    trials += [(_native.MODE_STATE, 3, None, {}), (7, 3, None, {})]
    trials += [(X, 5, None, {"tangent_first": f}) for f in (0, 15, 16, 20, -1)]
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out"):
        trials.append((H, 3, None, {field: ptr}))
    trials.append((H, 3, None, {"probe": ptr}))              # (the state tangents: allowed)
    trials += [(H, 3, None, {field: 0}) for field in ("x_in", "x_out", "wpack", "etab", "cond")]
    trials += [(H, 3, None, {"stage_slots": 8}), (H, 3, None, {"n_aux": 1})]
    seen = set()
    for mode, count, vc, fields in trials:
        a, b = _args(buf, mode, count), _args(buf, mode, count)
        for k, val in fields.items():
            setattr(a, k, val)
            setattr(b, k, val)
        want = ref(b, vc)
        assert call(sel, a, vc) == want, (mode, count, vc, fields, want)
        seen.add(want)
    assert seen == {OK, BAD}
    assert call(sel, _args(buf, H, 3), out=None) == BAD
    assert call(plain, _args(buf, H, 3), vc=ptr) == BAD          # conditional tangents on a plan without conditional inputs
    assert lib.ff_mlp_ode_launch_push_select(ctypes.byref(sel), None, None, ptr, None) == BAD
    assert lib.ff_mlp_ode_launch_push_select(None, ctypes.byref(_args(buf, H, 3)), None, ptr, None) == BAD
    # the new launch refuses every other plan
    others = [_native.make_plan(16, 4, [256] * 4, m) for m in (_native.MODE_HUTCH, _native.MODE_STATE, _native.MODE_EXACT)]
    others += [push, _native.make_pull_plan(16, 4, [256] * 4), _native.make_pull_select_plan(16, 4, [256] * 4)]
    others += [_native.make_pair_plan(16, 4, [256] * 4, select=s) for s in (False, True)]
    for other in others:
        assert call(other, _args(buf, H, 3)) == BAD, _native.kernel_name(other)
    assert call(_native.make_plan(16, 0, [256] * 4, H, precision=_native.PREC_BF16X2), _args(buf, H, 1)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(sel)
    forged.kernel_id = _native.PUSH_SELECT_KERNEL_BASE + 3
    assert call(forged, _args(buf, H, 3)) == BAD and lib.ff_plan_kernel_name(ctypes.byref(forged)) is None
    odd = _native.PlanStruct.from_buffer_copy(sel)
    odd.dim = 15
    assert call(odd, _args(buf, H, 3)) == BAD
    # every other launch refuses the plan
    a = _args(buf, H, 3)
    assert lib.ff_mlp_ode_launch_push(ctypes.byref(sel), ctypes.byref(a), None, ptr, None) == BAD
    assert lib.ff_mlp_ode_launch_pull(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_pull_select(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_vjp(ctypes.byref(sel), ctypes.byref(a), ptr, 0, ptr, None) == BAD
    assert lib.ff_mlp_ode_launch_pull_discrete(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_logp_grad(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, None, ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_record(ctypes.byref(sel), ctypes.byref(_args(buf, _native.MODE_STATE)), ptr, None) == BAD
    assert lib.ff_mlp_ode_launch(ctypes.byref(sel), ctypes.byref(_args(buf, _native.MODE_STATE)), None) == BAD
    b = _args(buf, H, 3)
    b.dlogp_out = b.probe = ptr
    assert lib.ff_mlp_ode_launch(ctypes.byref(sel), ctypes.byref(b), None) == BAD
    assert lib.ff_mlp_ode_launch_probes(ctypes.byref(sel), ctypes.byref(b), ptr, None) == BAD
    # ... and every other packer; its own packer refuses every other plan and NULL arguments
    two = (ctypes.c_void_p * 2)(ptr, ptr)
    hw = (ctypes.c_int * 1)(128)
    assert lib.ff_mlp_wpack(ctypes.byref(plain), two, two, hw, 16, 0, 0, ptr) == BAD
    assert lib.ff_mlp_pull_wpack(ctypes.byref(plain), two, two, hw, 16, 0, 0, ptr) == BAD
    assert lib.ff_mlp_pair_wpack(ctypes.byref(plain), two, two, two, two, hw, 16, 0, 0, ptr) == BAD
    assert lib.ff_mlp_pull_select_wpack(ctypes.byref(plain), two, two, two, two, hw, 16, 0, 0, ptr) == BAD
    pack = lambda plan, *a: lib.ff_mlp_push_select_wpack(ctypes.byref(plan), *a)
    for other in (_native.make_push_plan(16, 0, [128]), _native.make_pull_select_plan(16, 0, [128]), _native.make_pair_plan(16, 0, [128]),
                  _native.make_pair_plan(16, 0, [128], select=True)):
        assert pack(other, two, two, two, two, hw, 16, 0, 0, ptr) == BAD
    for i in range(4):
        nul = [two, two, two, two]
        nul[i] = None
        assert pack(plain, *nul, hw, 16, 0, 0, ptr) == BAD
    assert pack(plain, two, two, two, two, None, 16, 0, 0, ptr) == BAD and pack(plain, two, two, two, two, hw, 16, 0, 0, None) == BAD
    assert pack(plain, two, two, two, two, hw, 16, -1, 0, ptr) == BAD and pack(plain, two, two, two, two, hw, 16, 9, 0, ptr) == BAD
    assert pack(sel, two, two, two, two, hw, 16, 0, 14, ptr) == BAD
    assert pack(plain, two, two, two, two, (ctypes.c_int * 1)(129), 16, 0, 0, ptr) == BAD
    assert lib.ff_mlp_push_select_wpack(None, two, two, two, two, hw, 16, 0, 0, ptr) == BAD


# ---- the op --------------------------------------------------------------------------------------------------------------------------
def test_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_push_select
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_push_select_plan(16, 4, [256] * 4), 1)
    with FakeTensorMode():
        z, c = torch.empty(9, 16), torch.empty(9, 4)
        y, dz, st = op(z, c, torch.empty(9, 3, 16), torch.empty(9, 3, 4), torch.empty(10), torch.empty(5, 288), None, None, None, None,
                       plan, False, 0, 3)
        assert y.shape == (9, 16) and dz.shape == (9, 3, 16) and st.shape == (1,)
        y, dz, st = op(z, c, None, None, torch.empty(10), torch.empty(5, 288), None, None, None, None, plan, True, 5, 15)
        assert dz.shape == (9, 15, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), None, torch.zeros(10), torch.zeros(5, 288), None, None, None,
           None, plan, False, 0, 3)


# ---- the pack: two ff_mlp_wpack calls on the embedded networks, byte for byte ----------------------------------------------------
@pytest.mark.parametrize("D, C, units", [(5, 3, [128, 64]), (9, 0, [128]), (4, 16, [256, 192, 256]), (1, 1, [7])])
def test_push_select_pack_is_two_forward_packs_of_the_embedded_networks(D, C, units):
    front = L.make_model(D, C, units, gain=1.5)
    net = front._net()
    plan = net.push_select_plan()
    pack = net._pack(plan)
    lib = _native.lib()
    assert pack.numel() == lib.ff_mlp_push_select_wpack_floats(ctypes.byref(plan))
    D2, half = 2 * D, pack.numel() // 2
    push = _native.make_push_plan(D2, C, units)
    assert half == lib.ff_mlp_wpack_floats(ctypes.byref(push))
    for which, seq in ((0, front.model.mlp_q_dynamics), (1, front.model.mlp_p_dynamics)):
        lin = [l for l in seq if isinstance(l, torch.nn.Linear)]
        # the network over the whole joint state [q | p | cond], as ff_mlp_pair_wpack embeds it: mlp_q reads the p half and
        # writes rows 0..D-1, mlp_p reads the q half and writes rows D..2D-1 with its output weights and bias negated
        w0 = lin[0].weight.detach()
        W1 = torch.zeros(w0.shape[0], D2 + C)
        W1[:, (D if which == 0 else 0):(D2 if which == 0 else D)] = w0[:, :D]
        W1[:, D2:] = w0[:, D:D + C]
        Wo, bo = torch.zeros(D2, lin[-1].weight.shape[1]), torch.zeros(D2)
        rows = slice(0, D) if which == 0 else slice(D, D2)
        sgn = 1.0 if which == 0 else -1.0
        Wo[rows], bo[rows] = sgn * lin[-1].weight.detach(), sgn * lin[-1].bias.detach()
        ws = [W1] + [l.weight.detach() for l in lin[1:-1]] + [Wo]
        bs = [torch.zeros(w0.shape[0])] + [l.bias.detach() for l in lin[1:-1]] + [bo]
        want = _native.pack_weights(push, ws, bs, units, 0, D2)
        got = pack[which * half:(which + 1) * half]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), ("mlp_q", "mlp_p")[which]
    # and it is what ff_mlp_pair_wpack writes for a pair plan of the same layout, where there is one
    pair = net.plan(_native.MODE_STATE, select=True)
    if (pair.tile, pair.width, pair.dregs, pair.cregs) == (plan.tile, plan.width, plan.dregs, plan.cregs):
        assert torch.equal(net._pack(pair).view(torch.int32), pack.view(torch.int32))


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def test_signatures_and_defaults():
    sig = inspect.signature(Sm.SymplecticFlowModel.sample_leapfrog_jvp)
    assert list(sig.parameters) == ["self", "z", "tangents", "conditional", "conditional_tangents", "num_steps"]
    assert all(sig.parameters[n].default is None for n in ("tangents", "conditional", "conditional_tangents"))
    assert sig.parameters["num_steps"].default == 1
    sig = inspect.signature(Sm.SymplecticFlowModel.sample_leapfrog_jacobian)
    assert list(sig.parameters) == ["self", "z", "conditional", "num_steps"]
    assert sig.parameters["conditional"].default is None and sig.parameters["num_steps"].default == 1
    sig = inspect.signature(odeint.solve_leapfrog_push)
    assert list(sig.parameters) == ["front", "z", "grid", "tangents", "cond", "cond_tangents", "unit"]
    assert all(sig.parameters[n].default is None for n in ("tangents", "cond", "cond_tangents", "unit"))
    sig = inspect.signature(odeint.solve_leapfrog_push_jacobian)
    assert list(sig.parameters) == ["front", "z", "grid", "cond"] and sig.parameters["cond"].default is None
    from flowfusion_amd.fused import FusedPair
    sig = inspect.signature(FusedPair.pushforward_select)
    assert list(sig.parameters)[:8] == ["self", "z", "etab", "tangents", "cond", "cond_tangents", "unit", "stage_slots"]
    assert sig.parameters["stage_slots"].default == 1 and sig.parameters["tangents"].default is None
    assert {"in_shift", "in_scale", "out_scale", "out_shift"} <= set(sig.parameters)
    assert "push_select" in inspect.signature(FusedPair.width).parameters


def test_fused_pair_plans_packs_and_widths():
    front = L.make_model(9, 2, [128])
    net = front._net()
    p = net.push_select_plan()
    assert _native.kernel_name(p) == "mlp_pushsel_m16_h256_d8_c4_w2" and net.push_select_plan() is p
    assert net.width(_native.MODE_STATE, push_select=True) == 256 and net.width(_native.MODE_STATE, select=True) == 128
    assert net.width(_native.MODE_STATE) == 256                                      # (two networks' worth on the pair plan)
    key_push = net._param_key("cpu", p)[0]
    key_pair = net._param_key("cpu", net.plan(_native.MODE_STATE, select=True))[0]
    key_pull = net._param_key("cpu", net.pull_select_plan())[0]
    assert key_push[-1] == "push_select" and key_pull[-1] == "pull_select" and len({key_push, key_pair, key_pull}) == 3
    table = front._leapfrog_table(torch.linspace(1.0, 0.0, 3), push_select=True)
    narrow = front._leapfrog_table(torch.linspace(1.0, 0.0, 3))
    assert table.shape == (5, 32 + 256) and narrow.shape == (5, 32 + 128)
    assert torch.equal(table[:, :32 + 128], narrow) and bool((table[:, 32 + 128:] == 0).all())
    with pytest.raises(RuntimeError, match="GPU"):
        net.pushforward_select(torch.zeros(2, 18), table, torch.zeros(2, 1, 18), cond=torch.zeros(2, 2))


def test_every_refusal_of_the_front_ends_in_order(monkeypatch):
    front = L.make_model(4, 2, [64, 64])
    z, v, c, vc = torch.zeros(3, 8), torch.zeros(3, 2, 8), torch.zeros(3, 2), torch.zeros(3, 2, 2)
    grid = torch.linspace(1.0, 0.0, 3)
    push = lambda *a, **k: odeint.solve_leapfrog_push(front, *a, **k)
    jvp = front.sample_leapfrog_jvp
    # 1. num_steps, ahead of everything else (every later refusal is armed too)
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_steps"):
            jvp(torch.zeros(3, 7), torch.zeros(3, 16, 8).double(), c, vc, num_steps=n)
        with pytest.raises(ValueError, match="num_steps"):
            front.sample_leapfrog_jacobian(torch.zeros(3, 7), c, num_steps=n)
    # 2. shapes, ahead of K, dtypes and the device
    for bad_z in (torch.zeros(8), torch.zeros(3, 7), None):
        with pytest.raises(ValueError, match="z must be"):
            push(bad_z, grid, torch.zeros(3, 16, 8).double(), c)
        with pytest.raises(ValueError, match="prior draw"):
            jvp(bad_z, torch.zeros(3, 16, 8).double(), c)
        with pytest.raises(ValueError, match="prior draw"):
            front.sample_leapfrog_jacobian(bad_z, c)
    for bad_v in (torch.zeros(3, 8), torch.zeros(3, 2, 4), torch.zeros(2, 2, 8), torch.zeros(3, 16, 7).double()):
        with pytest.raises(ValueError, match="tangents must be"):
            push(z, grid, bad_v, c)
        with pytest.raises(ValueError, match="tangents must be"):
            jvp(z, bad_v, c)
    for bad_vc in (torch.zeros(3, 2), torch.zeros(3, 2, 3), torch.zeros(2, 2, 2)):
        with pytest.raises(ValueError, match="conditional_tangents must be"):
            push(z, grid, v, c, bad_vc)
        with pytest.raises(ValueError, match="conditional_tangents must be"):
            jvp(z, v, c, bad_vc)
    with pytest.raises(ValueError, match="conditional_tangents must be"):        # (no conditional to be tangent to)
        push(z, grid, v, None, vc)
    with pytest.raises(ValueError, match="2 and 3 tangents per sample"):
        push(z, grid, v, c, torch.zeros(3, 3, 2))
    with pytest.raises(ValueError, match="conditional must be"):
        push(z, grid, v, torch.zeros(2, 2))
    with pytest.raises(ValueError, match="take no tangent tensors"):
        push(z, grid, v, c, unit=(0, 2))
    for unit in ((-1, 2), (0, 0), (9, 2)):
        with pytest.raises(ValueError, match="outside"):
            push(z, grid, None, c, unit=unit)
    # 3. no tangents at all, K = 0, K > 15: ahead of dtypes and the device
    with pytest.raises(ValueError, match="and / or conditional_tangents"):
        push(z.double(), grid, None, c)
    with pytest.raises(ValueError, match="and / or conditional_tangents"):
        jvp(z.double(), None, c)
    with pytest.raises(ValueError, match="at least one tangent"):
        push(z.double(), grid, torch.zeros(3, 0, 8), c)
    with pytest.raises(ValueError, match="at most 15"):
        push(z.double(), grid, torch.zeros(3, 16, 8), c)
    with pytest.raises(ValueError, match="at most 15"):
        jvp(z.double(), None, c, torch.zeros(3, 16, 2))
    # 4. non-fp32 tensors, ahead of the device
    for args in ((z.double(), grid, v, c, vc), (z, grid, v.double(), c, vc), (z, grid, v, c.double(), vc), (z, grid, v, c, vc.double())):
        with pytest.raises(TypeError, match="float32"):
            push(*args)
    with pytest.raises(TypeError, match="float32"):
        jvp(z, v.double(), c, vc)
    with pytest.raises(TypeError, match="float32"):
        front.sample_leapfrog_jacobian(z.double(), c)
    # 5. CPU tensors, ahead of the envelope and of the conditional against the model
    wide = L.make_model(4, 0, [300])
    for f, args in ((push, (z, grid, v, c, vc)), (jvp, (z, v, c, vc)), (jvp, (z, None, c, vc)), (front.sample_leapfrog_jacobian, (z, c)),
                    (wide.sample_leapfrog_jvp, (z, v)), (jvp, (z, v, torch.zeros(3, 5)))):
        with pytest.raises(RuntimeError, match="GPU|cuda"):
            f(*args)
    with pytest.raises(RuntimeError, match="GPU|cuda"):
        odeint.solve_leapfrog_push_jacobian(front, z, grid, c)
    # 6. and 7. with the CPU refusal out of the way
    monkeypatch.setattr(odeint, "_need_gpu", lambda x: None)
    with pytest.warns(Warning):
        with pytest.raises(NotImplementedError, match="no module-path fallback") as e:
            wide.sample_leapfrog_jvp(z, v, torch.zeros(3, 5))           # (the envelope comes before the conditional)
    assert _native.PUSH_SELECT_ENVELOPE in str(e.value) and "PUSH_SELECT_ENVELOPE" in (odeint.solve_leapfrog_push.__doc__ or "")

    class Foreign(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(8, 8)

        def forward(self, t, state, conditional):
            return self.lin(state)
    foreign = Sm.SymplecticFlowModel(Foreign(), torch.zeros(4), torch.ones(4), None, None)
    with pytest.raises(NotImplementedError, match="no module-path fallback") as e:
        foreign.sample_leapfrog_jacobian(z)
    assert _native.PUSH_SELECT_ENVELOPE in str(e.value)
    deep = L.make_model(4, 0, [256] * 19)                  # no stash, no depth ceiling: the plan holds what the pull plan refuses
    assert _native.kernel_name(deep._net().push_select_plan()) == "mlp_pushsel_m16_h256_d4_c4_w2"
    with pytest.raises(ValueError, match=r"conditional must be \[3, 2\]"):
        push(z, grid, v, torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"conditional must be \[3, 2\]"):
        jvp(z, v)
    with pytest.raises(ValueError, match="joint state has 8"):
        push(torch.zeros(3, 10), grid, torch.zeros(3, 1, 10), c)
    none = L.make_model(4, 0, [64])
    with pytest.raises(ValueError, match="no conditional inputs"):
        odeint.solve_leapfrog_push(none, z, grid, v, c)


def test_the_four_old_methods_still_raise_with_their_old_text():
    front = L.make_model(2, 0, [32])
    for name, text in (("flow_jvp", "flow_jvp / flow_jacobian of a SymplecticFlowModel: the two-network kernels carry no tangent columns"),
                       ("flow_jacobian", "flow_jvp / flow_jacobian of a SymplecticFlowModel: the two-network kernels carry no tangent columns"),
                       ("flow_vjp", "flow_vjp of a SymplecticFlowModel: the two-network kernels carry no cotangent columns"),
                       ("log_prob_grad", "log_prob_grad of a SymplecticFlowModel: the two-network kernels carry no adjoint columns")):
        with pytest.raises(NotImplementedError) as e:
            getattr(front, name)(torch.zeros(1, 2))
        assert text in str(e.value) and "on ScoreModel, ODEFlow and ConditionalODEFlow" in str(e.value)
    assert str(_err_of(front.flow_jvp)) == ("flow_jvp / flow_jacobian of a SymplecticFlowModel: the two-network kernels carry no tangent "
                                            f"columns -- {_native.PUSH_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")
    assert str(_err_of(front.flow_vjp)) == ("flow_vjp of a SymplecticFlowModel: the two-network kernels carry no cotangent columns -- "
                                            f"{_native.PULL_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")
    assert str(_err_of(front.log_prob_grad)) == ("log_prob_grad of a SymplecticFlowModel: the two-network kernels carry no adjoint "
                                                 f"columns -- {_native.PULL_ENVELOPE}, on ScoreModel, ODEFlow and ConditionalODEFlow")


def _err_of(f):
    with pytest.raises(NotImplementedError) as e:
        f()
    return e.value
