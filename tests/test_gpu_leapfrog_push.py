"""GPU tier of the leapfrog push-forwards (csrc/ff_mlp_pushsel.hpp, ff_mlp_ode_launch_push_select,
``FusedPair.pushforward_select``, ``odeint.solve_leapfrog_push`` / ``solve_leapfrog_push_jacobian``,
``SymplecticFlowModel.sample_leapfrog_jvp`` / ``sample_leapfrog_jacobian``).

Raw launches of the three row-select push-forward units through ``FusedPair.pushforward_select`` (and once more between guard
words on NaN-prefilled outputs) against ``torch.func.jvp`` in float64 through the same rows (tests/_leapfrog_push_ref.py); the
bitwise properties (the state against the row-select solve of the same rows, unit tangents against one-hot buffers, the half a
row leaves alone); the front ends against float64 ``torch.func.jvp`` of the whole method, and the adjoint identity against the
device's own ``sample_leapfrog_vjp``.

Tolerance: the derivative families' rule (tests/test_gpu_pushforward.py): per case the reference runs in float64 and in fp32;
the fp32 run's normalised error against float64 is the case's floor, and the device is held to FACTOR = 22 floors.  The CPU
conditions every case meets are in tests/test_leapfrog_push_host.py.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from tests import _leapfrog_push_ref as L
from tests._pushforward_ref import normalised_error
from tests.test_gpu_pushforward import GUARD, _guarded, _payload

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = L.FACTOR


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


def case_table(front, plan, push_select=True):
    """The rows of ``plan`` at the width of the push-select plan (or of the select plan), as ``_leapfrog_table`` packs them."""
    net = front._net()
    a, b, c1 = front._schedule(plan.t_eval)
    H = net.width(_native.MODE_STATE, select=True)
    nb = (plan.flags & solvers.FLAG_NET_B) != 0
    own = torch.where(nb[:, None], c1[:, H:], c1[:, :H])
    if push_select:
        return solvers.build_table(plan, a, b, own[:, :net.hidden[0]], net.width(_native.MODE_STATE, push_select=True))
    return solvers.build_table(plan, a, b, own, H)


_RUNS = {}


def run_case(case, plan=None, maps=True, **override):
    """``FusedPair.pushforward_select`` on a raw case: (z_out, dz, status) on the CPU.  The plain run of a case is shared.
    ``override``: ``tangents`` / ``cond_tangents`` / ``unit`` in place of the case's own tangents."""
    key = L.case_id(case)
    plain = plan is None and maps and not override
    if plain and key in _RUNS:
        return _RUNS[key]
    front, own_plan, _, z, v, cond, vc = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    kw = dict(tangents=_dev(v), cond_tangents=_dev(vc))
    if override:
        kw = {k: (_dev(t) if torch.is_tensor(t) else t) for k, t in override.items()}
    m = {k: _dev(t) for k, t in L.case_maps(case).items()} if maps else {}
    zo, dz, status = net.pushforward_select(_dev(z), case_table(front, own_plan if plan is None else plan).to(DEV), cond=_dev(cond),
                                            **kw, **m)
    out = (zo.cpu(), dz.cpu(), int(status.item()))
    if plain:
        _RUNS[key] = out
    return out


# ---- accuracy: every raw case within 22 floors of float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_raw_launch_matches_float64_jvp(case):
    floor, sfloor, (zo64, dz64) = L.raw_floor_and_reference(case)
    zo, dz, status = run_case(case)
    assert status == 0
    err, serr = normalised_error(dz, dz64), normalised_error(zo, zo64)
    print(f"\n[leapfrog_push] {L.case_id(case)}: dz err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors (bar {FACTOR:.0f}); "
          f"z_out {serr:.3e} floor {sfloor:.3e} = {serr / sfloor:.2f} floors")
    assert err <= FACTOR * floor, (err, floor)
    assert serr <= FACTOR * sfloor, (serr, sfloor)


def test_every_unit_is_reached():
    names = set()
    for i, case in enumerate(L.RAW_CASES):
        front = L.case_setup(case)[0]
        name = _native.kernel_name(front._net().push_select_plan())
        assert name == L.UNIT_OF[i], (L.case_id(case), name)
        names.add(name)
    assert names == {_native.lib().ff_pushsel_kernel_name(i).decode() for i in range(3)}


# ---- guard words, status word: the C entry point on buffers of the test's own ---------------------------------------------------
@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_guard_words_are_intact_and_the_c_launch_is_the_ops(case):
    front, plan, _, z, v, cond, vc = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    p = net.push_select_plan()
    table = case_table(front, plan).to(DEV)
    wp = net.wpack(torch.device(DEV), _native.MODE_STATE, p)
    zd, vd, c, vcd = _dev(z), _dev(v), _dev(cond), _dev(vc)
    keep = {k: _dev(t) for k, t in L.case_maps(case).items()}
    B, D2 = zd.shape
    K = vd.shape[1]
    xo, to = _guarded(B * D2), _guarded(B * K * D2)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab, a.status = zd.data_ptr(), xo.data_ptr() + 4 * GUARD, wp.data_ptr(), table.data_ptr(), status.data_ptr()
    a.cond = 0 if c is None else c.data_ptr()
    a.probe = vd.data_ptr()
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    a.batch, a.n_evals, a.tangent_count, a.mode, a.stage_slots = B, table.shape[0], K, _native.MODE_HUTCH, 1
    rc = _native.lib().ff_mlp_ode_launch_push_select(ctypes.byref(p), ctypes.byref(a), 0 if vcd is None else vcd.data_ptr(),
                                                     to.data_ptr() + 4 * GUARD, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    zo, dz, _ = run_case(case)
    assert torch.equal(_payload(xo, (B, D2)).cpu(), zo) and torch.equal(_payload(to, (B, K, D2)).cpu(), dz)


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.RAW_CASES, ids=L.case_id)
def test_state_is_bitwise_the_row_select_solve_of_the_same_rows(case):
    """The value column of the push-select unit runs the row-select kernel's arithmetic: same packed rows, same bias-seeded
    MFMA chains, same SiLU, same stage algebra (extra registers and hidden units add exact zeros).  Every raw case's select
    plan multiplies on the 16-column tile, as every push-select unit does."""
    front, plan, _, z, v, cond, vc = L.case_setup(case)
    front = front.to(DEV)
    net = front._net()
    zo = run_case(case)[0]
    y, _, st = net.integrate_select(_dev(z), case_table(front, plan, push_select=False).to(DEV), cond=_dev(cond),
                                    **{k: _dev(t) for k, t in L.case_maps(case).items()})
    assert int(st.item()) == 0
    assert net.plan(_native.MODE_STATE, select=True).tile == net.push_select_plan().tile == 16
    assert torch.equal(y.cpu(), zo)


@pytest.mark.parametrize("case", [L.RAW_CASES[i] for i in (1, 2, 5, 8, 10)], ids=L.case_id)
def test_unit_tangents_are_bitwise_the_one_hot_buffers(case):
    front, plan, _, z, v, cond, vc = L.case_setup(case)
    B, D2 = z.shape
    C = 0 if cond is None else cond.shape[1]
    span = D2 + C
    K = min(15, span - 1)
    first = span - K                                            # the last K of the combined space: state, then every conditional
    eye = torch.eye(span)[first:first + K][None].expand(B, K, span)
    zo_u, dz_u, st_u = run_case(case, unit=(first, K))
    zo_e, dz_e, st_e = run_case(case, tangents=eye[:, :, :D2], cond_tangents=eye[:, :, D2:] if C else None)
    assert st_u == 0 and st_e == 0
    assert torch.equal(zo_u, zo_e) and torch.equal(dz_u, dz_e) and torch.equal(zo_u, run_case(case)[0])
    # the columns are not all alike: the launch did take the unit vectors
    assert float((dz_u[:, 0] - dz_u[:, -1]).abs().max()) > 0


def _one_row(net_b):
    flags = torch.full((1,), solvers.FLAG_STEP_END | (solvers.FLAG_NET_B if net_b else 0), dtype=torch.int32)
    cout = torch.zeros(1, 8, dtype=torch.float32)
    cout[0, 0] = 0.2
    return solvers.EvalPlan(t_eval=torch.tensor([0.6]), sign=-1.0, slot=torch.zeros(1, dtype=torch.int32), flags=flags,
                            cin=torch.zeros(1, 8, dtype=torch.float32), cout=cout, n_steps=1)


@pytest.mark.parametrize("case", [L.RAW_CASES[i] for i in (2, 4, 5, 7)], ids=L.case_id)
@pytest.mark.parametrize("net_b", (False, True), ids=("mlp_q", "mlp_p"))
def test_a_single_row_leaves_the_other_half_of_every_tangent_bitwise_alone(case, net_b):
    front, _, _, z, v, cond, vc = L.case_setup(case)
    D = case[0]
    zo, dz, st = run_case(case, plan=_one_row(net_b), maps=False)
    assert st == 0
    still = slice(0, D) if net_b else slice(D, 2 * D)           # mlp_p's row moves p and leaves q; mlp_q's the other way round
    moved = slice(D, 2 * D) if net_b else slice(0, D)
    assert torch.equal(dz[:, :, still], v[:, :, still]) and torch.equal(zo[:, still], z[:, still])
    assert float((dz[:, :, moved] - v[:, :, moved]).abs().max()) > 0 and float((zo[:, moved] - z[:, moved]).abs().max()) > 0
    # and what moved is the shear's derivative
    ref = L.LeapfrogRef(front, torch.float64)
    rows = L.plan_rows(_one_row(net_b))
    zo64, dz64 = L.jvp_rows(ref, z, cond, rows, v, vc)
    ref32 = L.LeapfrogRef(front, torch.float32)
    floor = L.fp32_floor(L.jvp_rows(ref32, z, cond, rows, v, vc)[1], dz64)
    assert normalised_error(dz, dz64) <= FACTOR * floor


def test_zero_tangents_give_zero_and_either_part_alone_adds_up():
    case = L.RAW_CASES[2]
    front, plan, _, z, v, cond, vc = L.case_setup(case)
    zo, dz, _ = run_case(case)
    zero = run_case(case, tangents=torch.zeros_like(v), cond_tangents=None)
    assert torch.equal(zero[0], zo) and bool((zero[1] == 0).all())
    only_v, only_c = run_case(case, tangents=v, cond_tangents=None), run_case(case, tangents=None, cond_tangents=vc)
    assert torch.equal(only_v[0], zo) and torch.equal(only_c[0], zo)
    floor, _, (_, dz64) = L.raw_floor_and_reference(case)
    assert normalised_error(only_v[1] + only_c[1], dz64) <= FACTOR * floor          # (linear in the tangent)


# ---- the front ends -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.SAMPLE_CASES, ids=L.front_id)
def test_sample_leapfrog_jvp(case):
    n = case[4]
    front, z, v, cond, vc, w = L.front_inputs(case)
    front = front.to(DEV)
    x, dx = front.sample_leapfrog_jvp(_dev(z), _dev(v), _dev(cond), _dev(vc), num_steps=n)
    assert torch.equal(x, front._sample_from(_dev(z), _dev(cond), n, method="leapfrog"))
    (x64, dx64), (x32, dx32) = (L.sample_jvp_ref(front, z, v, cond, vc, n, dt) for dt in (torch.float64, torch.float32))
    floor, err = L.fp32_floor(dx32, dx64), normalised_error(dx, dx64)
    print(f"\n[leapfrog_push] sample_leapfrog_jvp {L.front_id(case)}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors")
    assert err <= FACTOR * floor, (err, floor)
    assert normalised_error(x, x64) <= FACTOR * L.fp32_floor(x32, x64)
    if cond is not None:                                         # the hyper-parameter sensitivity alone: no state tangents
        xc, dxc = front.sample_leapfrog_jvp(_dev(z), None, _dev(cond), _dev(vc), num_steps=n)
        r64, r32 = (L.sample_jvp_ref(front, z, None, cond, vc, n, dt)[1] for dt in (torch.float64, torch.float32))
        assert torch.equal(xc, x) and normalised_error(dxc, r64) <= FACTOR * L.fp32_floor(r32, r64)


@pytest.mark.parametrize("case", L.SAMPLE_CASES, ids=L.front_id)
def test_sample_leapfrog_jacobian(case):
    n = case[4]
    front, z, v, cond, vc, w = L.front_inputs(case)
    front = front.to(DEV)
    x, Jz, Jc = front.sample_leapfrog_jacobian(_dev(z), _dev(cond), num_steps=n)
    B, D = z.shape[0], case[0]
    assert Jz.shape == (B, D, 2 * D) and (Jc is None) == (cond is None) and (Jc is None or Jc.shape == (B, D, case[1]))
    assert torch.equal(x, front._sample_from(_dev(z), _dev(cond), n, method="leapfrog"))
    assert front.last_solver_stats["launches"] >= 1
    r64, r32 = (L.sample_jacobian_ref(front, z, cond, n, dt) for dt in (torch.float64, torch.float32))
    for what, got, i in (("J_z", Jz, 1), ("J_c", Jc, 2)):
        if r64[i] is None:
            continue
        floor, err = L.fp32_floor(r32[i], r64[i]), normalised_error(got, r64[i])
        print(f"\n[leapfrog_push] sample_leapfrog_jacobian {L.front_id(case)} {what}: err {err:.3e} floor {floor:.3e} = "
              f"{err / floor:.2f} floors")
        assert err <= FACTOR * floor, (what, err, floor)


def test_row_cuts_are_bitwise(monkeypatch):
    for case in L.SAMPLE_CASES[:2]:                             # (the first takes its state from a launch of its own)
        n = case[4]
        front, z, v, cond, vc, w = L.front_inputs(case)
        front = front.to(DEV)
        whole = front.sample_leapfrog_jvp(_dev(z), _dev(v), _dev(cond), _dev(vc), num_steps=n)
        jac = front.sample_leapfrog_jacobian(_dev(z), _dev(cond), num_steps=n)
        monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 2 * v.shape[1] * z.shape[1] + 1)       # two rows per piece
        cut = front.sample_leapfrog_jvp(_dev(z), _dev(v), _dev(cond), _dev(vc), num_steps=n)
        assert front.last_solver_stats["launches"] >= (z.shape[0] + 1) // 2
        jac_cut = front.sample_leapfrog_jacobian(_dev(z), _dev(cond), num_steps=n)
        monkeypatch.undo()
        assert all(torch.equal(a, b) for a, b in zip(whole, cut))
        assert all(a is None or torch.equal(a, b) for a, b in zip(jac, jac_cut))


@pytest.mark.parametrize("case", L.SAMPLE_CASES, ids=L.front_id)
def test_adjoint_identity_against_the_devices_own_pull_back(case):
    n = case[4]
    front, z, v, cond, vc, w = L.front_inputs(case)
    front = front.to(DEV)
    _, dx = front.sample_leapfrog_jvp(_dev(z), _dev(v), _dev(cond), _dev(vc), num_steps=n)
    _, gz, gc = front.sample_leapfrog_vjp(_dev(z), _dev(w), _dev(cond), num_steps=n)
    gap, floor = L.adjoint_gap(w, dx, gz, v, gc, vc), L.adjoint_floor(case)
    print(f"\n[leapfrog_push] adjoint identity {L.front_id(case)}: gap {gap:.3e} floor {floor:.3e} = {gap / floor:.2f} floors")
    assert gap <= FACTOR * floor, (gap, floor)
