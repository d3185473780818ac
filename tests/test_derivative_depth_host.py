"""CPU tier of tests/test_gpu_derivative_depth.py: the conditions on its cases that make a pass on the device mean something,
checked on the references alone, and the host side of the deep shapes.

For every case of the GPU file, with the GPU file's own set-up:

* the gain literal lands max |dNET/dx| (float64, the case's inputs, the middle of the span) in [0.1, 10] -- and at gain 1 the
  same model is far below the window, which is why the case carries a gain;
* the fp32 floor of what the case checks is at most 5e-5 (the discrete file's cap);
* discrimination: a float64 reference whose parameters have two output rows of ONE hidden layer's weight matrix swapped -- the
  first, a middle and the last hidden layer in turn -- misses the case's bar (22 floors) by at least 100x on cot_x (pull,
  discrete), tangent_out (push) or prod (products).  A kernel that read one stash row, one weight chunk or one slope of another
  layer in place of the right one is off by at least as much as such a swap;
* the restated LDS request is above 64 KiB where the stash holds eight samples at the ceiling and at most 160 KiB everywhere,
  and the launches' own argument check (empty batch, no GPU) accepts the ceiling depth and refuses one layer more.

And the two weight packs of the three deepest shapes, decoded and run on the host against ``torch.func.vjp`` with the gained
weights (tests/test_pullback_host.py does it for 1 and 4 hidden layers)."""
import ctypes

import pytest
import torch

from flowfusion_amd import _native
from tests import _deep_models as DM
from tests import _pushforward_ref as R
from tests import test_gpu_derivative_depth as G
from tests.test_gpu_pushforward import FACTOR, make_front
from tests.test_pullback_host import test_forward_pack_then_transposed_pack_reproduce_the_vjp_of_the_network as check_packs

CAP = 5e-5
KIB = 1024


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


def _cases(cases):
    return [pytest.param(case, id=G._id(case)) for case in cases]


def _jacobian(case, gain):
    x, _, c, _ = G.case_inputs(case)
    ref_kw = make_front(case.kind, case.D, case.C, case.widths, case.nh, gain=gain)[1]
    return DM.net_jacobian(ref_kw, x, c, DM.mid_time(case.kind))


def _damaged_layers(case):
    return sorted({0, case.nh // 2, case.nh - 1})


@pytest.mark.parametrize("case", _cases(G.CASES))
def test_every_gpu_case_sees_the_network_has_a_low_floor_and_tells_a_swapped_weight_row_pair(case):
    j = _jacobian(case, case.gain)
    fl = G.floors(case)
    main = G.MAIN[case.family]
    r64 = G.reference(case, torch.float64)
    ratios = {}
    for layer in _damaged_layers(case):
        bad = G.reference(case, torch.float64, damage=layer)
        ratios[layer] = R.normalised_error(bad[main], r64[main]) / (FACTOR * fl[main])
    print(f"\n[derivative_depth] {G._id(case)}: gain {case.gain} max|J_net| {j:.3e} lds {G.lds_bytes(case)} floors "
          + " ".join(f"{k} {v:.3e}" for k, v in fl.items())
          + " swapped rows miss the bar by " + " ".join(f"layer {l}: {r:.0f}x" for l, r in ratios.items()))
    assert DM.WINDOW[0] <= j <= DM.WINDOW[1], j
    for what in (main, "cot_cond"):
        assert what not in fl or fl[what] <= CAP, (what, fl[what])
    for layer, ratio in ratios.items():
        assert ratio >= 100.0, (layer, ratio)


def _distinct_models():
    seen, out = set(), []
    for case in G.CASES:
        key = (case.kind, case.D, case.C, case.widths, case.gain)
        if key not in seen and (case.tier != "ksweep" or case.K == 1):
            seen.add(key)
            out.append(case)
    return out


@pytest.mark.parametrize("case", _cases(_distinct_models()))
def test_the_gain_is_needed_and_the_bisection_finds_one_in_the_window(case):
    """At gain 1 the deep models are blind to the network (18 x 256: 1e-10; 36 x 128: 1e-20) and the two-layer model of the K
    sweep sits under the window too; ``critical_gain`` on the case's inputs returns a gain inside it."""
    plain = _jacobian(case, 1.0)
    assert plain < DM.WINDOW[0], plain
    if case.nh >= 17:
        assert plain < 1e-9, plain
    x, _, c, _ = G.case_inputs(case)
    found = DM.critical_gain(case.kind, case.D, case.C, case.widths, case.nh, x, c, hi=64.0 if case.nh <= 2 else 8.0,
                             target=G.target_of(case))
    again = _jacobian(case, found)
    print(f"\n[derivative_depth] {G._id(case)}: gain 1 max|J_net| {plain:.3e}; bisection {found} -> {again:.3e}; literal {case.gain}")
    assert DM.WINDOW[0] <= again <= DM.WINDOW[1], (found, again)


# ---- the LDS request and the depth the launches accept ---------------------------------------------------------------------------
def test_restated_lds_requests():
    for case in G.CASES:
        lds = G.lds_bytes(case)
        assert lds <= 160 * KIB, (case, lds)
        if G.above_64k(case):
            assert lds > 64 * KIB, (case, lds)
    # the deepest pull plans at K = 1 with all seven slots: 158 and 157 KiB
    pull = {c.unit: G.lds_bytes(c) for c in G.CEILING if c.family == "pull" and c.K == 1}
    assert pull == {"h128_d4": 161792, "h256_d4": 161792, "h256_d8": 160768}
    assert sum(G.above_64k(c) for c in G.CEILING) == 6


def _args(buf, mode, count):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch (tests/test_pullback_host.py): a refusal
    comes ahead of the empty-batch return and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count = 0, 1, mode, count
    return a


@pytest.mark.parametrize("case", _cases([c for c in G.CEILING if c.family != "push"]))
def test_the_launch_accepts_the_ceiling_depth_and_refuses_one_layer_more(case):
    """The restated formula against the library's: at the case's K and slot count the launch takes the case's depth, and with
    one hidden layer more the restated request passes 160 KiB exactly when the launch answers FF_ERR_UNSUPPORTED."""
    L, buf = _native.lib(), torch.zeros(64)
    ptr = buf.data_ptr()
    width = G.UNIT_REGS[case.unit][0]
    base = _native.make_pull_plan(case.D, case.C, [width] * min(case.nh, 17))
    assert _native.kernel_name(base) == f"mlp_pull_m16_{case.unit}_c4"
    for extra in (0, 1):
        plan = _native.PlanStruct.from_buffer_copy(base)
        plan.n_hidden = case.nh + extra
        a = _args(buf, _native.MODE_HUTCH, case.K)
        a.stage_slots = case.slots
        if case.family == "pull":
            rc = L.ff_mlp_ode_launch_pull(ctypes.byref(plan), ctypes.byref(a), ptr, ptr, None, None)
        elif case.family == "discrete":
            rc = L.ff_mlp_ode_launch_pull_discrete(ctypes.byref(plan), ctypes.byref(a), ptr, ptr, ptr, None, None)
        else:
            rc = L.ff_mlp_ode_launch_vjp(ctypes.byref(plan), ctypes.byref(a), ptr, 0, ptr, None)
        deeper = case._replace(widths=case.widths + (width,) * extra)
        fits = G.lds_bytes(deeper) <= 160 * KIB
        assert rc == (_native.FF_OK if fits else _native.FF_ERR_UNSUPPORTED), (extra, rc, G.lds_bytes(deeper))
        if extra == 0:
            assert fits
        elif case.K == 1 and case.B == 9 and case.family != "products":
            # eight samples, seven slots: the ceiling itself.  (The products launch would take 19 x 256 as the discrete one
            # does -- its slots hold dregs words -- but its cases keep to plans the planner hands out.)
            assert not fits


def test_the_discrete_h256_d8_ceiling_is_seventeen_layers():
    """K = 5 leaves two samples' stash, far inside 160 KiB at any depth the planner takes: what bounds the case is the plan --
    the pull planner refuses 18 x 256 beyond 16 dimensions and takes 17."""
    case = next(c for c in G.CEILING if c.family == "discrete" and c.unit == "h256_d8")
    assert case.nh == 17
    _native.make_pull_plan(case.D, case.C, [256] * 17)
    with pytest.raises(NotImplementedError):
        _native.make_pull_plan(case.D, case.C, [256] * 18)


# ---- the packs of the deepest shapes, decoded and run on the host -----------------------------------------------------------------
@pytest.mark.parametrize("Dn, C, hidden, gain", [(32, 0, [256] * 17, 3.018), (16, 16, [256] * 18, 3.067), (16, 0, [128] * 36, 3.067)])
def test_deep_packs_reproduce_the_vjp_of_the_gained_network(Dn, C, hidden, gain):
    check_packs(Dn, C, hidden, gain=gain)
