"""GPU tier of the leapfrog pull-backs (csrc/ff_mlp_pullsel.hpp, ff_mlp_ode_launch_pull_select, ``FusedPair.pullback_select``,
``odeint.solve_leapfrog_pull``, ``SymplecticFlowModel.sample_leapfrog_vjp`` / ``log_prob_leapfrog_grad``).

Raw launches of the three row-select pull-back units through ``FusedPair.pullback_select`` (and once more between guard words
on NaN-prefilled outputs) against float64 autograd through the kept states of the same rows (tests/_leapfrog_pull_ref.py);
the bitwise properties (the retraced state against the row-select solve of the same rows, columns, re-runs, batch slices,
zeros); the front ends against float64 autograd of the whole method and a central finite difference.

Tolerance: the derivative families' rule (tests/test_gpu_pushforward.py): per case the reference runs in float64 and in fp32;
the fp32 run's normalised error against float64 is the case's floor, and the device is held to FACTOR = 22 floors.  The CPU
conditions every case meets are in tests/test_leapfrog_pull_host.py.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from tests import _leapfrog_pull_ref as L
from tests._pushforward_ref import normalised_error
from tests.test_gpu_pushforward import FACTOR, GUARD, _guarded, _payload, fp32_floor

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


def case_table(front, plan, pull_select=True):
    """The rows of ``plan`` at the width of the pull-select plan (or of the select plan), as ``_leapfrog_table`` packs them."""
    net = front._net()
    a, b, c1 = front._schedule(plan.t_eval)
    H = net.width(_native.MODE_STATE, select=True)
    nb = (plan.flags & solvers.FLAG_NET_B) != 0
    own = torch.where(nb[:, None], c1[:, H:], c1[:, :H])
    if pull_select:
        return solvers.build_table(plan, a, b, own[:, :net.hidden[0]], net.width(_native.MODE_STATE, pull_select=True))
    return solvers.build_table(plan, a, b, own, H)


_RUNS = {}


def run_case(case, cotangents=None, rows=None, fresh=False):
    """``FusedPair.pullback_select`` on a raw case: (z_back, gz, gc, status) on the CPU.  The plain run of a case is shared."""
    key = L.case_id(case)
    plain = cotangents is None and rows is None and not fresh
    if plain and key in _RUNS:
        return _RUNS[key]
    front, plan, _, z, cot, cond = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    sl = slice(None) if rows is None else rows
    w = cot if cotangents is None else cotangents
    zb, gz, gc, status = net.pullback_select(_dev(z[sl]), case_table(front, plan).to(DEV), _dev(w[sl]),
                                             cond=None if cond is None else _dev(cond[sl]), want_cond=cond is not None,
                                             **{k: _dev(v) for k, v in L.case_maps(case).items()})
    out = (zb.cpu(), gz.cpu(), None if gc is None else gc.cpu(), int(status.item()))
    if plain:
        _RUNS[key] = out
    return out


ALL_CASES = L.RAW_CASES + L.DEEP_CASES


# ---- accuracy: every raw case within 22 floors of float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=L.case_id)
def test_raw_launch_matches_float64_autograd(case):
    floor, (zb64, gz64, gc64) = L.raw_floor_and_reference(case)
    zb, gz, gc, status = run_case(case)
    assert status == 0
    err = L.normalised_pair(gz, gc, gz64, gc64)
    # the retraced state: held to its own floor, the fp32 reference's retrace against float64
    zb32 = L.raw_reference(case, torch.float32)[0]
    sfloor, serr = fp32_floor(zb32, zb64), normalised_error(zb, zb64)
    print(f"\n[leapfrog_pull] {L.case_id(case)}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors (bar {FACTOR:.0f}); "
          f"retraced state {serr:.3e} floor {sfloor:.3e}")
    assert err <= FACTOR * floor, (err, floor)
    assert serr <= FACTOR * sfloor, (serr, sfloor)


def test_every_unit_is_reached():
    names = set()
    for i, case in enumerate(L.RAW_CASES):
        front = L.case_setup(case)[0]
        name = _native.kernel_name(front._net().pull_select_plan())
        assert name == L.UNIT_OF[i], (L.case_id(case), name)
        names.add(name)
    assert names == {_native.lib().ff_pullsel_kernel_name(i).decode() for i in range(3)}


# ---- guard words, status word: the C entry point on buffers of the test's own ---------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=L.case_id)
def test_guard_words_are_intact_and_the_c_launch_is_the_ops(case):
    front, plan, _, z, cot, cond = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    p = net.pull_select_plan()
    table = case_table(front, plan).to(DEV)
    wp = net.wpack(torch.device(DEV), _native.MODE_STATE, p)
    zd, w, c = _dev(z), _dev(cot), _dev(cond)
    keep = {k: _dev(v) for k, v in L.case_maps(case).items()}
    B, D2 = zd.shape
    K, C = w.shape[1], (0 if c is None else c.shape[1])
    xo, gx = _guarded(B * D2), _guarded(B * K * D2)
    gc = _guarded(B * K * C) if C else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab, a.status = zd.data_ptr(), xo.data_ptr() + 4 * GUARD, wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if c is None else c.data_ptr()
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    a.batch, a.n_evals, a.tangent_count, a.mode, a.stage_slots = B, table.shape[0], K, _native.MODE_HUTCH, 1
    rc = _native.lib().ff_mlp_ode_launch_pull_select(ctypes.byref(p), ctypes.byref(a), w.data_ptr(), gx.data_ptr() + 4 * GUARD,
                                                     0 if gc is None else gc.data_ptr() + 4 * GUARD,
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    zb, gz, gcc, _ = run_case(case)
    assert torch.equal(_payload(xo, (B, D2)).cpu(), zb) and torch.equal(_payload(gx, (B, K, D2)).cpu(), gz)
    assert gc is None or torch.equal(_payload(gc, (B, K, C)).cpu(), gcc)


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_retraced_state_is_bitwise_the_row_select_solve_of_the_same_rows(case):
    """The value column of the pull-back unit runs the row-select kernel's arithmetic: same packed rows, same bias-seeded MFMA
    chains, same SiLU, same stage algebra (extra registers, hidden units and stage slots add exact zeros), so the two are
    bitwise equal.  Every raw case's select plan multiplies on the 16-column tile, as every pull-back unit does.  (A network
    up to 64 wide takes the 32-column select unit, whose MFMA groups a layer's sum differently: such shapes are in the
    front-end cases, held to accuracy, and not among the raw cases.)"""
    front, plan, _, z, cot, cond = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    zb = run_case(case)[0]
    y, _, st = net.integrate_select(_dev(z), case_table(front, plan, pull_select=False).to(DEV), cond=_dev(cond),
                                    **{k: _dev(v) for k, v in L.case_maps(case).items()})
    assert int(st.item()) == 0
    assert net.plan(_native.MODE_STATE, select=True).tile == net.pull_select_plan().tile == 16
    assert torch.equal(y.cpu(), zb)


@pytest.mark.parametrize("case", [L.RAW_CASES[i] for i in (1, 2, 3, 4, 9)], ids=L.case_id)
def test_column_0_of_a_k_launch_is_the_k_1_launch(case):
    cot = L.case_setup(case)[4]
    zb, gz, gc, _ = run_case(case)
    for k in (0, cot.shape[1] - 1):
        zb1, gz1, gc1, st = run_case(case, cotangents=cot[:, k:k + 1])
        assert st == 0 and torch.equal(zb1, zb) and torch.equal(gz1[:, 0], gz[:, k])
        assert gc is None or torch.equal(gc1[:, 0], gc[:, k])


@pytest.mark.parametrize("case", [L.RAW_CASES[i] for i in (2, 5, 7, 9)], ids=L.case_id)
def test_reruns_batch_slices_and_zero_cotangents(case):
    cot = L.case_setup(case)[4]
    whole = run_case(case)
    again = run_case(case, fresh=True)
    assert all(a is None or torch.equal(a, b) for a, b in zip(whole[:3], again[:3]))
    B = cot.shape[0]
    sl = slice(1, max(2, B - 1))
    part = run_case(case, rows=sl)
    assert all(a is None or torch.equal(a, b[sl]) for a, b in zip(part[:3], whole[:3]))
    zero = run_case(case, cotangents=torch.zeros_like(cot))
    assert torch.equal(zero[0], whole[0]) and bool((zero[1] == 0).all()) and (zero[2] is None or bool((zero[2] == 0).all()))


# ---- sample_leapfrog_vjp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.SAMPLE_CASES, ids=L.front_id)
def test_sample_leapfrog_vjp(case):
    n = case[4]
    front, z, _, _, cot, cond = L.front_inputs(case)
    front = front.to(DEV)
    x, gz, gc, retrace = front.sample_leapfrog_vjp(_dev(z), _dev(cot), _dev(cond), num_steps=n, return_retrace=True)
    assert torch.equal(x, front._sample_from(_dev(z), _dev(cond), n, method="leapfrog"))
    three = front.sample_leapfrog_vjp(_dev(z), _dev(cot), _dev(cond), num_steps=n)
    assert len(three) == 3 and torch.equal(three[1], gz)
    (x64, gz64, gc64), (x32, gz32, gc32) = (L.sample_vjp_ref(front, z, cot, cond, n, dt) for dt in (torch.float64, torch.float32))
    floor = fp32_floor(gz32, gz64)
    err = normalised_error(gz, gz64)
    if gc64 is not None:
        floor, err = max(floor, fp32_floor(gc32, gc64)), max(err, normalised_error(gc, gc64))
    print(f"\n[leapfrog_pull] sample_leapfrog_vjp {L.front_id(case)}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors; "
          f"retrace {float(retrace.max()):.3e}")
    assert err <= FACTOR * floor, (err, floor)
    assert normalised_error(x, x64) <= FACTOR * fp32_floor(x32, x64)
    assert (gc is None) == (cond is None)
    assert float(retrace.max()) <= 1e-5 * float(z.abs().max())


# ---- log_prob_leapfrog_grad ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.LOGP_CASES, ids=L.front_id)
def test_log_prob_leapfrog_grad(case):
    n = case[4]
    front, _, x, p0, _, cond = L.front_inputs(case)
    front = front.to(DEV)
    xd, pd, cd = _dev(x), _dev(p0), _dev(cond)
    lp, gx, gc, gp, retrace = front.log_prob_leapfrog_grad(xd, cd, n, momentum=pd, return_momentum_grad=True, return_retrace=True)
    assert torch.equal(lp, front._log_prob_from(xd, pd, cd, method="leapfrog", num_steps=n))
    r64, r32 = (L.logp_grad_ref(front, x, p0, cond, n, dt) for dt in (torch.float64, torch.float32))
    worst = []
    for what, got, i in (("grad_x", gx, 1), ("grad_c", gc, 2), ("grad_momentum", gp, 3)):
        if r64[i] is None:
            assert got is None
            continue
        floor, err = fp32_floor(r32[i], r64[i]), normalised_error(got, r64[i])
        print(f"\n[leapfrog_pull] log_prob_leapfrog_grad {L.front_id(case)} {what}: err {err:.3e} floor {floor:.3e} = "
              f"{err / floor:.2f} floors")
        worst.append((what, err, floor))
    print(f"[leapfrog_pull] retrace {float(retrace.max()):.3e}")
    for what, err, floor in worst:
        assert err <= FACTOR * floor, (what, err, floor)
    z0 = torch.cat([(x - front.shift.cpu()) / front.scale.cpu(), p0], dim=1)
    assert float(retrace.max()) <= 1e-5 * float(z0.abs().max())
    # one independent check: a central finite difference of the float64 map along a random direction
    g = torch.Generator().manual_seed(99)
    dx = torch.randn(x.shape, generator=g)
    dc = None if cond is None else torch.randn(cond.shape, generator=g)
    fd = L.logp_central_difference(front, x, p0, cond, n, dx, dc)
    along = (gx.cpu().double() * dx).sum(1) + (0 if dc is None else (gc.cpu().double() * dc).sum(1))
    along64 = (r64[1] * dx).sum(1) + (0 if dc is None else (r64[2] * dc).sum(1))
    assert float((fd - along64).abs().max()) <= 1e-6 * float(along64.abs().max())          # the reference itself
    # (the device's error along the direction: at most its normalised error times max |grad| times the 1-norm of the direction)
    scale = float(r64[1].abs().max()) * float(dx.abs().sum(1).max())
    if dc is not None:
        scale += float(r64[2].abs().max()) * float(dc.abs().sum(1).max())
    floor = max(fp32_floor(r32[1], r64[1]), 0.0 if dc is None else fp32_floor(r32[2], r64[2]))
    assert float((fd - along).abs().max()) <= FACTOR * floor * scale + 1e-6 * float(along64.abs().max())
    # any batch slice is bitwise the same; so are the shorter returns
    part = front.log_prob_leapfrog_grad(xd[2:7], None if cd is None else cd[2:7], n, momentum=pd[2:7], return_momentum_grad=True,
                                        return_retrace=True)
    for a, b in zip(part, (lp, gx, gc, gp, retrace)):
        assert (a is None and b is None) or torch.equal(a, b[2:7])
    three = front.log_prob_leapfrog_grad(xd, cd, n, momentum=pd)
    assert len(three) == 3 and torch.equal(three[0], lp) and torch.equal(three[1], gx)


def test_row_cuts_are_bitwise(monkeypatch):
    case = L.SAMPLE_CASES[0]
    n = case[4]
    front, z, _, _, cot, cond = L.front_inputs(case)
    front = front.to(DEV)
    whole = front.sample_leapfrog_vjp(_dev(z), _dev(cot), _dev(cond), num_steps=n, return_retrace=True)
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 2 * cot.shape[1] * z.shape[1] + 1)       # two rows per piece
    cut = front.sample_leapfrog_vjp(_dev(z), _dev(cot), _dev(cond), num_steps=n, return_retrace=True)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(whole, cut))


def test_momentum_is_drawn_like_log_prob_leapfrog():
    case = L.LOGP_CASES[0]
    front, _, x, _, _, cond = L.front_inputs(case)
    front = front.to(DEV)
    torch.manual_seed(7)
    lp = front.log_prob_leapfrog_grad(_dev(x), _dev(cond), case[4])[0]
    torch.manual_seed(7)
    assert torch.equal(lp, front.log_prob_leapfrog(_dev(x), _dev(cond), case[4]))
