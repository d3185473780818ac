"""CPU tier of the leapfrog pull-backs (ff_mlp_pull_select_plan, ff_mlp_pull_select_wpack, ff_mlp_ode_launch_pull_select;
``FusedPair.pullback_select``, ``odeint.solve_leapfrog_pull``, ``sample_leapfrog_vjp`` / ``log_prob_leapfrog_grad``): the
conditions every case of tests/test_gpu_leapfrog_pull.py meets on its references alone, the entry points and their
signatures, every refusal without a GPU, the planner at its corners, the op's fake registration, one pull-select pack decoded
on the host against ``torch.func.vjp`` of each embedded network, the methods' signatures and errors.

The conditions (for every raw and deep case, tests/_leapfrog_pull_ref.py):
  * the fp32 floor is at most 5e-5;
  * the float64 reference misses the case's bar (FACTOR = 22 floors) by at least 100 x with two output rows swapped in the
    first, a middle or the last hidden layer of mlp_q, likewise of mlp_p, with mlp_q and mlp_p exchanged, and, where C > 0,
    with the gamma of either network dropped;
  * the float64 retraced sweep -- the kernel's algorithm -- equals autograd through the kept states to 1e-12: on shear rows
    the retracing adjoint IS the discrete adjoint.
"""
import ctypes
import inspect
from pathlib import Path

import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import symplectic as Sm
from tests import _emulator as E
from tests import _leapfrog_pull_ref as L
from tests.test_gpu_pushforward import FACTOR

ROOT = Path(__file__).resolve().parents[1]
OK, BAD, UNS = _native.FF_OK, _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED
ALL_CASES = L.RAW_CASES + L.DEEP_CASES


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the conditions of every case ------------------------------------------------------------------------------------------------
def damages_of(case):
    nh, C = len(case[2]), case[1]
    out = {}
    for n, name in ((0, "mlp_q"), (1, "mlp_p")):
        for layer in sorted({0, nh // 2, nh - 1}):
            out[f"rows 0, 1 of hidden layer {layer} of {name} swapped"] = L.Damage(swap=(n, layer, (0, 1)))
    out["mlp_q and mlp_p exchanged"] = L.Damage(exchange=True)
    if C > 0:
        out["gamma of mlp_q dropped"] = L.Damage(drop_gamma=0)
        out["gamma of mlp_p dropped"] = L.Damage(drop_gamma=1)
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=L.case_id)
def test_floor_is_small_and_every_damage_misses_the_bar_by_100(case):
    floor, (zb, gz, gc) = L.raw_floor_and_reference(case)
    assert floor <= 5e-5, floor
    bar = FACTOR * floor
    for what, damage in damages_of(case).items():
        _, dz, dc = L.raw_reference(case, torch.float64, damage)
        miss = L.normalised_pair(dz, dc, gz, gc) / bar
        assert miss >= 100.0, (what, miss)


@pytest.mark.parametrize("case", ALL_CASES, ids=L.case_id)
def test_float64_retraced_sweep_is_autograd_through_the_kept_states(case):
    front, plan, rows, z, cot, cond = L.case_setup(case)
    ref = L.LeapfrogRef(front, torch.float64)
    zb, gz, gc = ref.pull_ref(z, cond, rows, cot)
    y, alpha, gamma = ref.sweep_ref(z, cond, rows, cot)
    assert float((y - zb).abs().max()) <= 1e-12
    assert float((alpha - gz).abs().max()) <= 1e-12
    assert gc is None or float((gamma - gc).abs().max()) <= 1e-12
    # the retraced start is the true one: undoing the backward rows from it leads back to z
    assert float((ref.run(zb, ref.cast(cond), L.undo_rows(rows)) - z.double()).abs().max()) <= 1e-12


def test_cases_cover_what_they_must():
    raw = L.RAW_CASES
    assert {c[0] for c in raw} >= {1, 4, 5, 8, 9, 16} and {c[1] for c in raw} >= {0, 1, 16}
    assert {len(c[2]) for c in raw} >= {1, 2, 4, 5, 7, 8} and any(len(set(c[2])) > 1 for c in raw)
    assert {c[4] for c in raw} >= {1, 2, 3, "hand"} and {c[5] for c in raw} >= {1, 2, 4, 7, 15}
    assert {c[6] for c in raw} >= {1, 17} and any(len(c) > 7 for c in raw)
    for c in raw:
        assert c[6] in (1, 17, 16 // (1 + c[5]) + 1) and 1.0 <= c[3] <= 3.0
    hand = L.plan_rows(L.hand_plan())
    assert [nb for _, _, nb in hand] == [False, False, True, True, False]
    for steps in (1, 2, 3):
        rows = L.plan_rows(L.case_plan((1, 0, [32], 1.0, steps, 1, 1)))
        assert len(rows) == 2 * steps + 1 and rows[0][2] and rows[-1][2]
    # every unit, each at its deepest plan: one layer more is refused
    for i, case in enumerate(raw):
        assert _native.kernel_name(_native.make_pull_select_plan(2 * case[0], case[1], case[2])) == L.UNIT_OF[i]
    assert set(L.UNIT_OF.values()) == {_native.lib().ff_pullsel_kernel_name(i).decode() for i in range(3)}
    for case in L.DEEP_CASES:
        assert case[5] == 1 and 1.0 <= case[3] <= 3.0
        _native.make_pull_select_plan(2 * case[0], case[1], case[2])
        with pytest.raises(NotImplementedError):
            _native.make_pull_select_plan(2 * case[0], case[1], case[2] + case[2][:1])


# ---- the C entry points --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures():
    lib = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert "#define FF_PULL_SELECT_KERNEL_BASE 0xA0000" in header and _native.PULL_SELECT_KERNEL_BASE == 0xA0000
    assert "int ff_pullsel_kernel_count(void);" in header and "const char* ff_pullsel_kernel_name(int index);" in header
    assert "int ff_mlp_pull_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);" in header
    assert "size_t ff_mlp_pull_select_wpack_floats(const ff_mlp_plan_t* plan);" in header
    assert ("int ff_mlp_pull_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq, "
            "const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0, int x_col0, int c_col0, "
            "float* out);") in header
    assert ("int ff_mlp_ode_launch_pull_select(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cotangent_in "
            "/* [batch, K, dim] */, float* cot_x_out /* [batch, K, dim] */, float* cot_cond_out /* [batch, K, cond_dim] or NULL */, "
            "void* hip_stream);") in header
    assert lib.ff_pullsel_kernel_count() == 3
    names = [lib.ff_pullsel_kernel_name(i).decode() for i in range(3)]
    assert names == ["mlp_pullsel_m16_h128_d4_c4", "mlp_pullsel_m16_h256_d4_c4", "mlp_pullsel_m16_h256_d8_c4"]
    assert lib.ff_pullsel_kernel_name(3) is None and lib.ff_pullsel_kernel_name(-1) is None
    # a family of its own: none of the other tables lists it
    for count, name in ((lib.ff_kernel_count, lib.ff_kernel_name), (lib.ff_pull_kernel_count, lib.ff_pull_kernel_name),
                        (lib.ff_pair_kernel_count, lib.ff_pair_kernel_name)):
        assert not any(b"pullsel" in name(i) for i in range(count()))
    assert lib.ff_mlp_ode_launch_pull_select.argtypes == lib.ff_mlp_ode_launch_pull.argtypes
    assert "hidden widths up to 256" in _native.PULL_SELECT_ENVELOPE and "32 dimensions" in _native.PULL_SELECT_ENVELOPE


def _plan(dim, cond, hidden):
    p = _native.PlanStruct()
    arr = (ctypes.c_int * len(hidden))(*hidden)
    return _native.lib().ff_mlp_pull_select_plan(dim, cond, len(hidden), arr, ctypes.byref(p)), p


def test_planner_at_its_corners():
    lib = _native.lib()
    for dim, cond, hidden, name in ((2, 0, [1], "h128_d4"), (16, 16, [128] * 36, "h128_d4"), (16, 0, [129], "h256_d4"),
                                    (16, 16, [256] * 18, "h256_d4"), (18, 0, [128], "h256_d8"), (32, 16, [256] * 17, "h256_d8")):
        rc, p = _plan(dim, cond, hidden)
        assert rc == OK and _native.kernel_name(p) == f"mlp_pullsel_m16_{name}_c4", (dim, cond, hidden)
        assert _native.is_pull_select_plan(p) and p.kernel_id >= _native.PULL_SELECT_KERNEL_BASE
        assert not (_native.is_pull_plan(p) or _native.is_push_plan(p) or _native.is_pair_plan(p) or _native.is_select_plan(p))
        assert _native.row_width(p) == p.width and _native.samples_per_workgroup(p, _native.MODE_HUTCH) == 8
        # twice the pull pack of the matching pull shape; the other size queries answer 0
        pull = _native.make_pull_plan(dim, cond, hidden)
        assert (pull.tile, pull.width, pull.dregs, pull.cregs) == (p.tile, p.width, p.dregs, p.cregs)
        assert lib.ff_mlp_pull_select_wpack_floats(ctypes.byref(p)) == 2 * lib.ff_mlp_pull_wpack_floats(ctypes.byref(pull))
        for other in (lib.ff_mlp_wpack_floats, lib.ff_mlp_pair_wpack_floats, lib.ff_mlp_pull_wpack_floats):
            assert other(ctypes.byref(p)) == 0
        assert lib.ff_mlp_pull_select_wpack_floats(ctypes.byref(pull)) == 0
    for args in ((3, 0, [64]), (17, 0, [64]), (0, 0, [64]), (4, -1, [64]), (4, 0, [0]), (4, 0, [])):
        assert _plan(*args)[0] == BAD, args
    for args in ((34, 0, [64]), (2, 17, [64]), (2, 0, [257]), (16, 0, [128] * 37), (16, 0, [256] * 19), (18, 0, [256] * 18)):
        assert _plan(*args)[0] == UNS, args
    arr = (ctypes.c_int * 1)(64)
    assert lib.ff_mlp_pull_select_plan(4, 0, 1, arr, None) == BAD
    assert lib.ff_mlp_pull_select_plan(4, 0, 1, None, ctypes.byref(_native.PlanStruct())) == BAD
    with pytest.raises(NotImplementedError, match="16 per half"):
        _native.make_pull_select_plan(34, 0, [64])


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
    sel = _native.make_pull_select_plan(16, 4, [256] * 4)
    plain = _native.make_pull_select_plan(16, 0, [128])
    H = _native.MODE_HUTCH
    call = lambda plan, a, w=ptr, gx=ptr, gc=None: lib.ff_mlp_ode_launch_pull_select(ctypes.byref(plan), ctypes.byref(a), w, gx, gc, None)
    for count in (1, 2, 7, 15):
        assert call(sel, _args(buf, H, count)) == OK and call(sel, _args(buf, H, count), gc=ptr) == OK, count
        assert call(plain, _args(buf, H, count)) == OK, count
    for count in (0, -1, 16, 40):
        assert call(sel, _args(buf, H, count)) == BAD, count
    for mode in (_native.MODE_STATE, _native.MODE_EXACT, 7):
        assert call(sel, _args(buf, mode, 3)) == BAD, mode
    assert call(sel, _args(buf, H, 3), w=None) == BAD and call(sel, _args(buf, H, 3), gx=None) == BAD
    assert lib.ff_mlp_ode_launch_pull_select(ctypes.byref(sel), None, ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_pull_select(None, ctypes.byref(_args(buf, H, 3)), ptr, ptr, None, None) == BAD
    assert call(plain, _args(buf, H, 3), gc=ptr) == BAD
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out", "probe"):
        a = _args(buf, H, 3)
        setattr(a, field, ptr)
        assert call(sel, a) == BAD, field
    a = _args(buf, H, 3)
    a.n_aux = 1
    a.aux_out[0] = ptr
    assert call(sel, a) == BAD
    for field in ("x_in", "x_out", "wpack", "etab", "cond"):
        a = _args(buf, H, 3)
        setattr(a, field, 0)
        assert call(sel, a) == BAD, field
    a = _args(buf, H, 3)
    a.stage_slots = 8
    assert call(sel, a) == BAD
    # the LDS bound is the pull launch's: a forged depth whose K = 1 stash does not fit
    deep = _native.PlanStruct.from_buffer_copy(sel)
    deep.n_hidden = 20
    assert call(deep, _args(buf, H, 1)) == UNS and call(deep, _args(buf, H, 3)) == OK
    # the new launch refuses every other plan
    others = [_native.make_plan(16, 4, [256] * 4, m) for m in (_native.MODE_HUTCH, _native.MODE_STATE, _native.MODE_EXACT)]
    others += [_native.make_push_plan(16, 4, [256] * 4), _native.make_pull_plan(16, 4, [256] * 4)]
    others += [_native.make_pair_plan(16, 4, [256] * 4, select=s) for s in (False, True)]
    for other in others:
        assert call(other, _args(buf, H, 3)) == BAD, _native.kernel_name(other)
    assert call(_native.make_plan(16, 0, [256] * 4, H, precision=_native.PREC_BF16X2), _args(buf, H, 1)) == UNS
    forged = _native.PlanStruct.from_buffer_copy(sel)
    forged.kernel_id = _native.PULL_SELECT_KERNEL_BASE + 3
    assert call(forged, _args(buf, H, 3)) == BAD and _native.lib().ff_plan_kernel_name(ctypes.byref(forged)) is None
    odd = _native.PlanStruct.from_buffer_copy(sel)
    odd.dim = 15
    assert call(odd, _args(buf, H, 3)) == BAD
    # every other launch refuses the plan
    a = _args(buf, H, 3)
    assert lib.ff_mlp_ode_launch_pull(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_vjp(ctypes.byref(sel), ctypes.byref(a), ptr, 0, ptr, None) == BAD
    assert lib.ff_mlp_ode_launch_pull_discrete(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_logp_grad(ctypes.byref(sel), ctypes.byref(a), ptr, ptr, None, ptr, ptr, None, None) == BAD
    assert lib.ff_mlp_ode_launch_push(ctypes.byref(sel), ctypes.byref(a), None, ptr, None) == BAD
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
    pack = lambda plan, *a: lib.ff_mlp_pull_select_wpack(ctypes.byref(plan), *a)
    for other in (_native.make_pull_plan(16, 0, [128]), _native.make_pair_plan(16, 0, [128]), _native.make_pair_plan(16, 0, [128], select=True)):
        assert pack(other, two, two, two, two, hw, 16, 0, 0, ptr) == BAD
    for i in range(4):
        nul = [two, two, two, two]
        nul[i] = None
        assert pack(plain, *nul, hw, 16, 0, 0, ptr) == BAD
    assert pack(plain, two, two, two, two, None, 16, 0, 0, ptr) == BAD and pack(plain, two, two, two, two, hw, 16, 0, 0, None) == BAD
    assert pack(plain, two, two, two, two, hw, 16, -1, 0, ptr) == BAD and pack(plain, two, two, two, two, hw, 16, 9, 0, ptr) == BAD
    assert pack(sel, two, two, two, two, hw, 16, 0, 14, ptr) == BAD
    assert pack(plain, two, two, two, two, (ctypes.c_int * 1)(129), 16, 0, 0, ptr) == BAD
    assert lib.ff_mlp_pull_select_wpack(None, two, two, two, two, hw, 16, 0, 0, ptr) == BAD


# ---- the op --------------------------------------------------------------------------------------------------------------------------
def test_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_pull_select
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_pull_select_plan(16, 4, [256] * 4), 1)
    with FakeTensorMode():
        z, c = torch.empty(9, 16), torch.empty(9, 4)
        y, gz, gc, st = op(z, c, torch.empty(9, 3, 16), torch.empty(10), torch.empty(5, 288), None, None, None, None, plan, True)
        assert y.shape == (9, 16) and gz.shape == (9, 3, 16) and gc.shape == (9, 3, 4) and st.shape == (1,)
        y, gz, gc, st = op(z, c, torch.empty(9, 5, 16), torch.empty(10), torch.empty(5, 288), None, None, None, None, plan, False)
        assert gz.shape == (9, 5, 16) and gc.shape == (9, 5, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), torch.zeros(10), torch.zeros(5, 288), None, None, None, None,
           plan, True)


# ---- one pull-select pack, decoded on the host ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D, C, units", [(5, 3, [128, 64]), (9, 0, [128]), (4, 16, [256, 192, 256])])
def test_pull_select_pack_reproduces_the_vjp_of_each_embedded_network(D, C, units):
    """The four packs [A_q | B_q | A_p | B_p] decoded (tests/_emulator.py) and run in float64 the way the kernel runs a row:
    net A on the joint state gives the value and the slopes, net B on [alpha | 0] the transposed products.  Each half must be
    the embedded network: mlp_q reads the p half and writes rows 0..D-1, mlp_p reads the q half and writes rows D..2D-1
    negated; both read the conditional."""
    front = L.make_model(D, C, units, gain=1.5)
    net = front._net()
    plan = net.pull_select_plan()
    pack = net._pack(plan)
    lib = _native.lib()
    assert pack.numel() == lib.ff_mlp_pull_select_wpack_floats(ctypes.byref(plan))
    D2, half = 2 * D, pack.numel() // 2
    tile, dregs, cregs, H = plan.tile, plan.dregs, plan.cregs, plan.width
    NQ = 64 // tile
    pull = _native.make_pull_plan(D2, C, units)
    push = _native.make_push_plan(D2, C, units)
    nA = lib.ff_mlp_wpack_floats(ctypes.byref(push))
    wordsA = _native.plan_words(push, 0)
    wordsB = list(_native.plan_words(pull, 0))
    wordsB[0], wordsB[1], wordsB[4], wordsB[5] = NQ * (dregs + cregs), 0, dregs + cregs, 0
    cplace = {E.feat_of_reg(tile, r, q): E.feat_of_reg(tile, dregs + r, q) for r in range(cregs) for q in range(NQ)}
    ref = L.LeapfrogRef(front, torch.float64)
    g = torch.Generator().manual_seed(3)
    B = 3
    z = torch.randn(B, D2, generator=g).double()
    c = torch.randn(B, C, generator=g).double() if C else None
    alpha = torch.randn(B, D2, generator=g).double()
    t = torch.tensor(0.37)
    silu = lambda a: a * torch.sigmoid(a)
    slope = lambda a: torch.sigmoid(a) * (1 + a * (1 - torch.sigmoid(a)))
    a_, b_, c1 = front._schedule(t.reshape(1))
    Hp = net.width(_native.MODE_STATE, select=True)
    for which in (0, 1):
        part = pack[which * half:(which + 1) * half]
        W1, hid, Wo, bo, dx = E.decode_wpack(wordsA, part[:nA])
        T1, thid, To, tb, _ = E.decode_wpack(wordsB, part[nA:])
        assert tb.abs().sum() == 0 and all(bb.abs().sum() == 0 for _, bb in thid)
        c1p = torch.zeros(H, dtype=torch.float64)
        c1p[:units[0]] = c1[0, which * Hp:which * Hp + units[0]].double()
        pre = z @ W1[:, :D2].T + (c @ W1[:, dx:dx + C].T if C else 0.0) + c1p
        slopes, h = [slope(pre)], silu(pre)
        for Wl, bl in hid:
            pre = h @ Wl.T + bl
            slopes.append(slope(pre))
            h = silu(pre)
        value = (h @ Wo.T + bo)[:, :D2]
        op = torch.zeros(B, T1.shape[1], dtype=torch.float64)
        op[:, :D2] = alpha
        v = (op @ T1.T) * slopes[-1]
        for (Wl, _), s in zip(thid, reversed(slopes[:-1])):
            v = (v @ Wl.T) * s
        out = v @ To.T

        def embedded(zz, cc=None):
            q, p = zz[:, :D], zz[:, D:]
            zero = torch.zeros_like(q)
            if which == 0:
                return torch.cat([ref.net(0, p, cc, t), zero], dim=1)
            return torch.cat([zero, -ref.net(1, q, cc, t)], dim=1)
        if C:
            want, pullfn = torch.func.vjp(embedded, z, c)
            gz, gc = pullfn(alpha)
        else:
            want, pullfn = torch.func.vjp(embedded, z)
            (gz,), gc = pullfn(alpha), None
        tol = lambda ref_t: 2e-6 * max(1e-3, float(ref_t.abs().max()))       # (an fp32 time embedding in a float64 run)
        assert torch.allclose(value, want, rtol=0, atol=tol(want))
        assert torch.allclose(out[:, :D2], gz, rtol=0, atol=tol(gz))
        # the half the network does not read gets an exact zero
        dead = slice(0, D) if which == 0 else slice(D, D2)
        assert bool((out[:, dead] == 0).all()) and bool((value[:, slice(D, D2) if which == 0 else slice(0, D)] == 0).all())
        if C:
            got_c = torch.stack([out[:, cplace[j]] for j in range(C)], dim=1)
            assert torch.allclose(got_c, gc, rtol=0, atol=tol(gc))


# ---- the Python layers -----------------------------------------------------------------------------------------------------------------
def test_signatures_and_defaults():
    sig = inspect.signature(Sm.SymplecticFlowModel.sample_leapfrog_vjp)
    assert list(sig.parameters) == ["self", "z", "cotangents", "conditional", "num_steps", "return_retrace"]
    assert sig.parameters["conditional"].default is None and sig.parameters["num_steps"].default == 1
    assert sig.parameters["return_retrace"].default is False and sig.parameters["return_retrace"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(Sm.SymplecticFlowModel.log_prob_leapfrog_grad)
    assert list(sig.parameters) == ["self", "x", "conditional", "num_steps", "momentum", "return_momentum_grad", "return_retrace"]
    assert sig.parameters["num_steps"].default is None and sig.parameters["momentum"].default is None
    for name in ("momentum", "return_momentum_grad", "return_retrace"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(odeint.solve_leapfrog_pull)
    assert list(sig.parameters) == ["front", "z", "grid", "cotangents", "cond", "return_retrace"]
    assert sig.parameters["cond"].default is None and sig.parameters["return_retrace"].default is False
    from flowfusion_amd.fused import FusedPair
    sig = inspect.signature(FusedPair.pullback_select)
    assert list(sig.parameters)[:7] == ["self", "z", "etab", "cotangents", "cond", "want_cond", "stage_slots"]
    assert sig.parameters["stage_slots"].default == 1 and sig.parameters["cond"].default is None
    assert {"in_shift", "in_scale", "out_scale", "out_shift"} <= set(sig.parameters)


def test_fused_pair_plans_packs_and_widths():
    front = L.make_model(9, 2, [128])
    net = front._net()
    p = net.pull_select_plan()
    assert _native.kernel_name(p) == "mlp_pullsel_m16_h256_d8_c4" and net.pull_select_plan() is p
    assert net.width(_native.MODE_STATE, pull_select=True) == 256 and net.width(_native.MODE_STATE, select=True) == 128
    assert net.width(_native.MODE_STATE) == 256                                      # (two networks' worth on the pair plan)
    key_sel = net._param_key("cpu", p)[0]
    key_pair = net._param_key("cpu", net.plan(_native.MODE_STATE, select=True))[0]
    assert key_sel != key_pair and key_sel[-1] == "pull_select"
    table = front._leapfrog_table(torch.linspace(0.0, 1.0, 3), pull_select=True)
    narrow = front._leapfrog_table(torch.linspace(0.0, 1.0, 3))
    assert table.shape == (5, 32 + 256) and narrow.shape == (5, 32 + 128)
    assert torch.equal(table[:, :32 + 128], narrow) and bool((table[:, 32 + 128:] == 0).all())
    # the table of the flipped grid holds bitwise the same times and weights in reverse order
    from flowfusion_amd import solvers
    grid = torch.linspace(1.0, 0.0, 8)
    fwd, back = solvers.plan_leapfrog(grid), solvers.plan_leapfrog(grid.flip(0))
    assert torch.equal(fwd.t_eval, back.t_eval.flip(0)) and torch.equal(fwd.cout[:, 0], back.cout[:, 0].flip(0))
    assert torch.equal(fwd.flags, back.flags.flip(0)) and fwd.sign == -back.sign
    with pytest.raises(RuntimeError, match="GPU"):
        net.pullback_select(torch.zeros(2, 18), table, torch.zeros(2, 1, 18), cond=torch.zeros(2, 2))


def test_every_error_of_the_front_ends():
    front = L.make_model(4, 2, [64, 64])
    z, w, c = torch.zeros(3, 8), torch.zeros(3, 2, 4), torch.zeros(3, 2)
    grid = torch.linspace(1.0, 0.0, 3)
    pull = lambda *a, **k: odeint.solve_leapfrog_pull(front, *a, **k)
    # shapes
    for bad_z in (torch.zeros(8), torch.zeros(3, 7), None):
        with pytest.raises(ValueError, match="z must be"):
            pull(bad_z, grid, torch.zeros(3, 2, 8), c)
    for bad_w in (torch.zeros(3, 8), torch.zeros(3, 2, 4), torch.zeros(2, 2, 8), torch.zeros(3, 0, 8), None):
        with pytest.raises(ValueError, match="cotangents must be"):
            pull(z, grid, bad_w, c)
    with pytest.raises(ValueError, match="cotangents must be"):       # (the function form is the library's own, not public)
        pull(z, grid, lambda zo: zo[:, None, :], c)
    # K > 15
    with pytest.raises(ValueError, match="at most 15"):
        pull(z, grid, torch.zeros(3, 16, 8), c)
    # non-fp32 tensors
    with pytest.raises(TypeError, match="float32"):
        pull(z.double(), grid, torch.zeros(3, 2, 8), c)
    with pytest.raises(TypeError, match="float32"):
        pull(z, grid, torch.zeros(3, 2, 8).double(), c)
    with pytest.raises(TypeError, match="float32"):
        pull(z, grid, torch.zeros(3, 2, 8), c.double())
    # CPU tensors
    with pytest.raises(RuntimeError, match="GPU|cuda"):
        pull(z, grid, torch.zeros(3, 2, 8), c)
    # the front ends' own
    with pytest.raises(ValueError, match="num_steps"):
        front.sample_leapfrog_vjp(z, w, c, num_steps=0)
    with pytest.raises(ValueError, match="cotangents must be"):
        front.sample_leapfrog_vjp(z, torch.zeros(3, 2, 8), c)
    with pytest.raises(ValueError, match="prior draw"):
        front.sample_leapfrog_vjp(torch.zeros(3, 7), w, c)
    with pytest.raises(ValueError, match="at most 15"):
        front.sample_leapfrog_vjp(z, torch.zeros(3, 16, 4), c)
    with pytest.raises(RuntimeError, match="GPU|cuda"):
        front.sample_leapfrog_vjp(z, w, c, num_steps=2)
    x = torch.zeros(3, 4)
    for n in (None, 0, -1):
        with pytest.raises(ValueError, match="num_steps >= 1"):
            front.log_prob_leapfrog_grad(x, c, n)
    with pytest.raises(ValueError, match="momentum must be"):
        front.log_prob_leapfrog_grad(x, c, 2, momentum=torch.zeros(3, 5))
    with pytest.raises(TypeError, match="float32"):
        front.log_prob_leapfrog_grad(x, c, 2, momentum=torch.zeros(3, 4).double())
    with pytest.raises(RuntimeError, match="GPU|cuda"):
        front.log_prob_leapfrog_grad(x, c, 2, momentum=torch.zeros(3, 4))


def test_models_outside_the_envelope_are_refused_without_a_fallback(monkeypatch):
    # the checks that come before the envelope pass on a CPU model only if the CPU refusal is out of the way
    monkeypatch.setattr(odeint, "_need_gpu", lambda x: None)
    grid = torch.linspace(1.0, 0.0, 3)
    wide = L.make_model(4, 0, [300])                       # no two-network kernel holds it: the module route elsewhere
    with pytest.warns(Warning):
        with pytest.raises(NotImplementedError, match="no module-path fallback") as e:
            odeint.solve_leapfrog_pull(wide, torch.zeros(2, 8), grid, torch.zeros(2, 1, 8))
    assert _native.PULL_SELECT_ENVELOPE in str(e.value)
    deep = L.make_model(4, 0, [256] * 19)                  # the pair kernels hold it, the stash does not
    with pytest.raises(NotImplementedError, match="no module-path fallback|160 KiB") as e:
        odeint.solve_leapfrog_pull(deep, torch.zeros(2, 8), grid, torch.zeros(2, 1, 8))
    assert _native.PULL_SELECT_ENVELOPE in str(e.value)

    class Foreign(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(8, 8)

        def forward(self, t, state, conditional):
            return self.lin(state)
    foreign = Sm.SymplecticFlowModel(Foreign(), torch.zeros(4), torch.ones(4), None, None)
    with pytest.raises(NotImplementedError, match="no module-path fallback"):
        odeint.solve_leapfrog_pull(foreign, torch.zeros(2, 8), grid, torch.zeros(2, 1, 8))
    # with the model inside: the conditional's shape
    front = L.make_model(4, 2, [64, 64])
    with pytest.raises(ValueError, match=r"conditional must be \[3, 2\]"):
        odeint.solve_leapfrog_pull(front, torch.zeros(3, 8), grid, torch.zeros(3, 1, 8), torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"conditional must be \[3, 2\]"):
        odeint.solve_leapfrog_pull(front, torch.zeros(3, 8), grid, torch.zeros(3, 1, 8))
    with pytest.raises(ValueError, match="joint state has 8"):
        odeint.solve_leapfrog_pull(front, torch.zeros(3, 10), grid, torch.zeros(3, 1, 10), torch.zeros(3, 2))
    none = L.make_model(4, 0, [64])
    with pytest.raises(ValueError, match="no conditional inputs"):
        odeint.solve_leapfrog_pull(none, torch.zeros(3, 8), grid, torch.zeros(3, 1, 8), torch.zeros(3, 2))


def test_the_four_old_methods_still_raise_with_their_old_text():
    front = L.make_model(2, 0, [32])
    for name, text in (("flow_jvp", "flow_jvp / flow_jacobian of a SymplecticFlowModel: the two-network kernels carry no tangent columns"),
                       ("flow_jacobian", "flow_jvp / flow_jacobian of a SymplecticFlowModel"),
                       ("flow_vjp", "flow_vjp of a SymplecticFlowModel: the two-network kernels carry no cotangent columns"),
                       ("log_prob_grad", "log_prob_grad of a SymplecticFlowModel: the two-network kernels carry no adjoint columns")):
        with pytest.raises(NotImplementedError) as e:
            getattr(front, name)(torch.zeros(1, 2))
        assert text in str(e.value) and "on ScoreModel, ODEFlow and ConditionalODEFlow" in str(e.value)
