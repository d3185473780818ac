"""GPU tier of the derivative kernels at the edges of their envelope (csrc/ff_mlp_pull.hpp, ff_mlp_vjp.hpp, ff_mlp_dadj.hpp,
ff_mlp_ode.hpp PUSH): raw launches of the pull, discrete-adjoint, record, products and push units, through the helpers of their
own GPU files, at

* the LDS ceiling: every unit of every family that keeps a slope stash at the deepest depth its launch accepts (36 x 128,
  18 x 256, 17 x 256, and 19 x 256 for the discrete launch, on a plan forged the way tests/test_pullback_discrete_host.py
  forges it: plan 18 layers, set ``n_hidden = 19``, pack for it), where the dynamic LDS request is 145 .. 159 KiB and the
  stash offsets pass 64 KiB; the record and push launches, which keep no stash, at the same depths;
* intermediate depths 5, 7 and 8 with ragged widths, whose chunk counts leave the weight ring at different phases when it
  wraps from net B's output layer to the next row;
* every K from 1 to 15 (8, 5, 4, 3, 2, 2, 2, 1 .. 1 samples per tile; 0 .. 7 dead columns), each with a ragged second tile.

The models.  At default init a deep SiLU stack has no Jacobian to speak of (tests/_deep_models.py: max |dNET/dx| = 9.5e-11 at
18 x 256), and a derivative kernel would pass on it whatever it did with the hidden layers.  So every case multiplies the
hidden-to-hidden weights by a gain -- the literal in its row, found by ``_deep_models.critical_gain`` -- that lands
max |dNET/dx| in [0.1, 10]; tests/test_derivative_depth_host.py recomputes that on the CPU for every case, holds every fp32
floor to 5e-5, and proves that a float64 reference with two weight rows swapped in the first, a middle or the last hidden
layer misses the case's bar by at least 100x.  Nothing on the GPU bisects.

Tolerance: the push-forward tests' rule and factor (tests/test_gpu_pushforward.py).  Per case the reference runs twice on the
CPU, in fp32 and in float64; the fp32 run's error per sample, normalised by the sample's largest reference entry, is the case's
fp32 floor, as measured, and the bar is that floor times FACTOR = 22.  profiles/derivative_depth.txt lists the gains, floors
and the device's errors.

LDS.  ``lds_bytes`` restates the byte counts of csrc/ff_api.cpp (pull_lds_bytes / vjp_lds_bytes / rec_lds_bytes).  A ceiling
case with K = 1 (eight samples per tile) asserts a request above 64 KiB; the ceiling rows with K = 4, 5 and 8 keep the same
depth with 3, 2 and 1 samples' stash (56, 42 and 25 KiB: the stash stride and the base behind one or four slots are what they
move), and the record and push launches keep no stash at all (7 and 28 KiB).
"""
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from flowfusion_amd import _native, odeint, solvers
from oracle import flowfusion_oracle as fo
from tests import _deep_models as DM
from tests import _estimator_products_ref as EP
from tests import _pullback_discrete_ref as DP
from tests import _pullback_ref as P
from tests import _pushforward_ref as R
from tests.test_gpu_estimator_products import raw_vjp
from tests.test_gpu_pullback import forward_state, raw_pull
from tests.test_gpu_pullback_discrete import STATE_TOL, raw_discrete, raw_record
from tests.test_gpu_pushforward import FACTOR, fp32_floor, make_front, options_of, raw_push, span_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
KIB = 1024
UNIT_REGS = {"h128_d4": (128, 4, 4), "h256_d4": (256, 4, 4), "h256_d8": (256, 8, 4)}       # unit -> (width, dregs, cregs)
MAIN = {"pull": "cot_x", "discrete": "cot_x", "products": "prod", "push": "tangent_out"}    # what the damage must move


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


class Case(NamedTuple):
    tier: str                       # ceiling / depth / ksweep
    family: str                     # pull / discrete / products / push  (a discrete case runs the record launch first)
    unit: str
    kind: str                       # flow / vp / ve
    D: int
    C: int
    K: int
    B: int
    widths: Tuple[int, ...]
    method: str
    nsteps: int
    direction: str
    gain: float                     # the literal: _deep_models.critical_gain, checked by the host file
    flag: Optional[str] = None      # products: "rows" = per-row seeds; push: "ct" = conditional tangents given; "forged" plan

    @property
    def nh(self):
        return len(self.widths)

    @property
    def slots(self):
        """Stage slots the launch keeps in LDS: the method's stages -- and all seven at the ceiling under dopri5_fixed, whose six
        rows leave the seventh idle: the largest request a launch can make, with the stash base behind it."""
        stages = solvers.resolve_method(self.method).stages
        return solvers.MAX_SLOTS if (self.tier == "ceiling" and stages == 6) else stages


RAGGED = (255, 256, 129, 256, 255, 130, 256, 131)
# the ceiling: every unit of every stash family at its deepest accepted depth, the record and push launches beside them
CEILING = [
    Case("ceiling", "pull", "h128_d4", "flow", 16, 0, 1, 9, (128,) * 36, "dopri5_fixed", 1, "to_data", 3.054),
    Case("ceiling", "pull", "h256_d4", "flow", 16, 16, 1, 9, (256,) * 18, "dopri5_fixed", 1, "to_base", 2.993),
    Case("ceiling", "pull", "h256_d8", "flow", 32, 16, 1, 9, (256,) * 17, "dopri5_fixed", 1, "to_data", 2.969),
    Case("ceiling", "pull", "h256_d4", "flow", 5, 1, 4, 4, (256,) * 18, "euler", 2, "to_data", 3.042),
    Case("ceiling", "discrete", "h256_d4", "flow", 16, 0, 1, 9, (256,) * 19, "dopri5_fixed", 1, "to_data", 2.945, "forged"),
    Case("ceiling", "discrete", "h256_d8", "flow", 17, 1, 5, 3, (256,) * 17, "rk4", 2, "to_base", 3.142),
    Case("ceiling", "discrete", "h128_d4", "flow", 4, 0, 1, 1, (128,) * 36, "euler", 1, "to_base", 3.03),
    Case("ceiling", "products", "h256_d4", "ve", 16, 0, 1, 9, (256,) * 18, "dopri5_fixed", 1, "to_base", 3.042, "rows"),
    Case("ceiling", "products", "h256_d8", "ve", 32, 8, 8, 2, (256,) * 17, "rk4", 2, "to_base", 3.181),
    Case("ceiling", "push", "h256_d4", "flow", 16, 16, 15, 2, (256,) * 18, "rk4", 2, "to_data", 3.067, "ct"),
    Case("ceiling", "push", "h128_d4", "flow", 3, 0, 3, 5, (128,) * 36, "euler", 2, "to_base", 2.999),
]
# intermediate depths: the ring at three phases of its wrap
DEPTHS = [Case("depth", family, "h256_d4", kind, 7, 3, 2, 6, RAGGED[:nh], "rk4", 2, direction, gain)
          for family, kind, direction, gains in (("pull", "flow", "to_data", (4.176, 3.667, 3.436)),
                                                 ("discrete", "flow", "to_base", (4.176, 3.667, 3.436)))
          for nh, gain in zip((5, 7, 8), gains)]
# every K: one unit per family, B = samples per tile + 1
KSWEEP_GAIN = {"pull": 4.756, "discrete": 4.756, "products": 8.0, "push": 4.756}
KSWEEP_KIND = {"pull": ("flow", "to_base"), "discrete": ("flow", "to_data"), "products": ("ve", "to_base"), "push": ("flow", "to_data")}
KSWEEP = [Case("ksweep", family, "h256_d4", KSWEEP_KIND[family][0], 5, 1, K, 16 // (1 + K) + 1, (255, 129), "rk4", 2,
               KSWEEP_KIND[family][1], KSWEEP_GAIN[family], "ct" if family == "push" else None)
          for family in ("pull", "discrete", "products", "push") for K in range(1, 16)]
CASES = CEILING + DEPTHS + KSWEEP


def target_of(case):
    """What ``critical_gain`` aims max |dNET/dx| at for the case's literal: the low end of the window at the ceiling (the
    floor of a 17 .. 36 layer model grows with it, and a score model's drift carries the network over sigma: the products cases
    aim lower still), the middle at the intermediate depths, and 0.5 for the K sweep, whose cases with two rows see less than
    the nine rows the gain is found on."""
    if case.tier != "ceiling":
        return 1.0 if case.tier == "depth" else 0.5
    return 0.12 if case.family == "products" else 0.2


def _id(case):
    return "-".join(str(p) if not isinstance(p, tuple) else f"{len(p)}x{max(p)}" for p in case if p is not None)


# ---- the LDS request, restated ---------------------------------------------------------------------------------------------------
def lds_bytes(case, launch=None):
    """Dynamic LDS of one tile of the case's launch (``launch``: "record" for the record launch of a discrete case), the
    formulas of csrc/ff_api.cpp: stage slots of 64 lanes x 16 bytes per group of four registers -- dregs + cregs registers for a
    pull tile, dregs for a products / discrete / record tile -- then the stash, samples per tile x n_hidden x width x 4 bytes.
    A push launch is mlp_ode_kernel's: four wavefronts' worth of all seven slots, no stash."""
    width, dregs, cregs = UNIT_REGS[case.unit]
    slots = case.slots
    stash = (16 // (1 + case.K)) * case.nh * width * 4
    launch = launch or case.family
    if launch == "pull":
        return slots * ((dregs + cregs) // 4) * 64 * 16 + stash
    if launch in ("discrete", "products"):
        return slots * (dregs // 4) * 64 * 16 + stash
    if launch == "record":
        return slots * (dregs // 4) * 64 * 16
    assert launch == "push"
    return 4 * solvers.MAX_SLOTS * (dregs // 4) * 64 * 16


def above_64k(case):
    """The ceiling cases whose stash holds eight samples: the launches that ask for more than 64 KiB."""
    return case.tier == "ceiling" and case.family in ("pull", "discrete", "products") and case.K == 1


# ---- models, inputs, references ---------------------------------------------------------------------------------------------------
def build(case, damage=None):
    """(front end on the CPU, SolverMap keywords) of the case's gained model.  ``damage``: the hidden layer whose weight matrix
    gets two output rows swapped IN THE REFERENCE's parameters (the front end keeps the true model).  A "forged" case gets
    the plan the pull planner refuses: the plan of one layer fewer with ``n_hidden`` set."""
    front, ref_kw = make_front(case.kind, case.D, case.C, case.widths, case.nh, gain=case.gain)
    if damage is not None:
        ref_kw = dict(ref_kw, params=DM.swap_rows(ref_kw["params"], damage))
    if case.flag == "forged":
        plan = _native.make_pull_plan(case.D, case.C, list(case.widths[:-1]))
        plan.n_hidden = case.nh
        front._net()._plans["pull"] = plan
    return front, ref_kw


def case_inputs(case):
    """(x [B, D], w [B, K, D] -- cotangents, tangents or seeds ([n, B, K, D] with per-row seeds) --, cond [B, C] or None,
    conditional tangents [B, K, C] or None).  The cases of the K sweep cut theirs out of ONE draw of nine rows and fifteen
    columns, so row b, column 0 is the same vector at every K."""
    B, K = (9, 15) if case.tier == "ksweep" else (case.B, case.K)
    g = torch.Generator().manual_seed(41 + 1000 * B + 10 * case.D + K)
    n = case.nsteps * solvers.resolve_method(case.method).stages
    x = torch.randn(B, case.D, generator=g)
    w = torch.randn(*((n, B, K, case.D) if case.flag == "rows" else (B, K, case.D)), generator=g)
    c = torch.randn(B, case.C, generator=g) if case.C else None
    vc = torch.randn(B, K, case.C, generator=g) if (case.C and case.flag == "ct") else None
    cut = lambda t, k: None if t is None else (t[..., :case.B, :case.K, :] if k else t[:case.B]).contiguous()
    return cut(x, False), cut(w, True), cut(c, False), cut(vc, True)


def _products_grid(front, case):
    eps = float(front.sde.epsilon)
    span = torch.tensor([eps, 1.0], dtype=torch.float32)
    return solvers.plan_ode(span, case.method, {"step_size": float(span[1] - span[0]) / case.nsteps})


def per_sample(prod):
    """[n, B, K, D] -> [B, n, K, D]: the normalisation runs over everything a sample's launch wrote."""
    return prod.permute(1, 0, 2, 3)


_REFS = {}


def reference(case, dtype, damage=None):
    """name -> tensor (batch first) of the case's reference in ``dtype``, computed once and shared: the family's own reference
    (tests/_pullback_ref.py, _pullback_discrete_ref.py, _estimator_products_ref.py, _pushforward_ref.py) on the gained model."""
    key = (case, dtype, damage)
    if key in _REFS:
        return _REFS[key]
    front, ref_kw = build(case, damage)
    x, w, c, vc = case_inputs(case)
    out = {}
    if case.family == "products":
        o = fo.ScoreOracle(ref_kw["params"], R.SDES[case.kind](dtype=dtype), no_sigma=False, dtype=dtype)
        cc = None if c is None else c.to(dtype)
        xo, prod, _ = EP.table_products(lambda t, y: o.ode_drift(t, y, cc), _products_grid(front, case), x.to(dtype), w.to(dtype),
                                        case.flag == "rows")
        out = {"x_out": xo, "prod": per_sample(prod)}
    else:
        smap = R.SolverMap(direction=case.direction, method=case.method, options=options_of(front, case.direction, case.nsteps),
                           dtype=dtype, **ref_kw)
        if case.family == "pull":
            r = P.Pullback(smap)
            y, gx, gc, _ = r(x, w, c)
            out = {"x_out": y, "retraced": r.retraced, "cot_x": gx, "cot_cond": gc}
        elif case.family == "discrete":
            r = DP.DiscretePullback(smap)
            y, gx, gc = r(x, w, c)
            out = {"x_out": y, "cot_x": gx, "cot_cond": gc}
            if damage is None and dtype == torch.float64:
                out["record"] = r.stage_states(x, c)[0]
        else:
            y, d = smap.jvp(x, w, c, vc)
            out = {"x_out": y, "tangent_out": d}
    _REFS[key] = {k: v.detach() for k, v in out.items() if v is not None}
    return _REFS[key]


def floors(case):
    """name -> fp32 floor of every output the case checks at the bar."""
    r64, r32 = reference(case, torch.float64), reference(case, torch.float32)
    return {k: fp32_floor(r32[k], r64[k]) for k in r32}


# ---- the launches ----------------------------------------------------------------------------------------------------------------
def launch(case, w=None, rows=None, K=None):
    """(name -> tensor on the CPU in the USER's units, the kernels' names) of the case's raw launches.  ``w``: other cotangents /
    tangents / seeds; ``rows``: a slice of the batch; ``K``: the first K columns only."""
    front, _ = build(case)
    x, w0, c, vc = case_inputs(case)
    w = w0 if w is None else w
    if K is not None:
        w, vc = w[..., :K, :].contiguous(), (None if vc is None else vc[:, :K].contiguous())
    if rows is not None:
        x, c, vc = x[rows], (None if c is None else c[rows]), (None if vc is None else vc[rows])
        w = w[:, rows] if case.flag == "rows" else w[rows]
    if case.family == "products":
        xo, prod, name = raw_vjp(front, _products_grid(front, case), case.method, x, w, case.flag == "rows", cond=c, slots=case.slots)
        return {"x_out": xo, "prod": per_sample(prod)}, (name,)
    t_span, opts = span_of(front, case.direction), options_of(front, case.direction, case.nsteps)
    # a score model's to_data solve starts from x * sigma_max (VE): the chain rule's factor; a flow's network sees the
    # normalised conditional
    sg = float(front.sde.sigma_max) if (case.kind != "flow" and case.direction == "to_data" and hasattr(front.sde, "sigma_max")) else 1.0
    c_net, c_scale = c, None
    if case.kind == "flow" and case.C:
        c_net, c_scale = front._norm_cond(c), front.conditional_scale.detach().cpu()
    if case.family == "push":
        y, dy, name = raw_push(front, x * sg, t_span, case.method, opts, w.shape[1], tangents=w * sg, cond=c, cond_tangents=vc)
        return {"x_out": y.cpu(), "tangent_out": dy.cpu()}, (name,)
    if case.family == "pull":
        y = forward_state(front, x * sg, t_span, case.method, opts, c_net, {})
        xb, gx, gc, name = raw_pull(front, y, t_span, case.method, opts, w, cond=c_net, slots=case.slots)
        out, names = {"x_out": y.cpu(), "retraced": xb.cpu() / sg, "cot_x": gx.cpu() * sg}, (name,)
    else:
        y, rec, rec_name = raw_record(front, x * sg, t_span, case.method, opts, cond=c_net, slots=case.slots)
        gx, gc, name = raw_discrete(front, rec, t_span, case.method, opts, w, cond=c_net, slots=case.slots)
        out, names = {"x_out": y.cpu(), "record": rec.cpu(), "cot_x": gx.cpu() * sg}, (rec_name, name)
    if gc is not None:
        out["cot_cond"] = gc.cpu() if c_scale is None else gc.cpu() / c_scale
    return out, names


def unit_names(case):
    u = case.unit
    return {"pull": (f"mlp_pull_m16_{u}_c4",), "discrete": (f"mlp_rec_m16_{u}_c4", f"mlp_dadj_m16_{u}_c4"),
            "products": (f"mlp_vjp_m16_{u}_c4",), "push": (f"mlp_push_m16_{u}_c4",)}[case.family]


def check_against_float64(case, got, names):
    """Every output of the case at its bar, the record at the state tests'; the figures are printed before anything asserts."""
    # the units the case is meant for (a push unit's name goes on with its waves per SIMD)
    assert all(n == want or (case.family == "push" and n.startswith(want + "_")) for n, want in zip(names, unit_names(case))), names
    r64, fl = reference(case, torch.float64), floors(case)
    line, worst = f"\n[derivative_depth] {_id(case)} {'+'.join(names)} lds {lds_bytes(case)}:", []
    for what, floor in fl.items():
        err = R.normalised_error(got[what], r64[what])
        line += f" {what} err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors);"
        worst.append((what, err, floor))
    rec_err = None
    if "record" in got:
        rec, rec64 = got["record"].double(), r64["record"]
        rec_err = float(((rec - rec64).abs().amax(dim=(1, 2)) / rec64.abs().amax(dim=(1, 2)).clamp_min(1e-30)).max())
        line += f" record err {rec_err:.3e};"
    print(line)
    assert rec_err is None or rec_err <= STATE_TOL, rec_err
    for what, err, floor in worst:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


# ---- the ceiling and the intermediate depths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CEILING + DEPTHS, ids=_id)
def test_deep_launch_against_float64_reference(case):
    lds = lds_bytes(case)
    assert lds <= 160 * KIB and (not above_64k(case) or lds > 64 * KIB), lds
    got, names = launch(case)
    check_against_float64(case, got, names)


def test_record_launch_at_nineteen_layers_against_the_float64_stage_states():
    """The record launch keeps no stash and takes any depth: 19 x 256 on the forged plan, every stage state of dopri5's six
    rows at STATE_TOL, and its x_out at the bar."""
    case = CEILING[4]
    assert case.flag == "forged" and case.nh == 19 and lds_bytes(case, "record") == 7 * 1024
    got, names = launch(case)
    assert names[0] == f"mlp_rec_m16_{case.unit}_c4", names
    r64 = reference(case, torch.float64)
    rec, rec64 = got["record"].double(), r64["record"]
    assert rec.shape == (6, case.B, case.D)
    rec_err = float(((rec - rec64).abs().amax(dim=(1, 2)) / rec64.abs().amax(dim=(1, 2)).clamp_min(1e-30)).max())
    floor, err = floors(case)["x_out"], R.normalised_error(got["x_out"], r64["x_out"])
    print(f"\n[derivative_depth] record 19 x 256: record err {rec_err:.3e}; x_out err {err:.3e} floor {floor:.3e}")
    assert rec_err <= STATE_TOL and err <= FACTOR * floor, (rec_err, err, floor)


# ---- every K ------------------------------------------------------------------------------------------------------------------------
_K1 = {}


def _single_column_launch(family):
    """The K = 1 launch of the family's sweep (nine rows), once."""
    if family not in _K1:
        case = next(c for c in KSWEEP if c.family == family and c.K == 1)
        _K1[family] = launch(case)[0]
    return _K1[family]


@pytest.mark.parametrize("case", KSWEEP, ids=_id)
def test_every_k_against_float64_and_column_zero_is_the_single_column_launch(case):
    assert case.B == 16 // (1 + case.K) + 1 and lds_bytes(case) <= 160 * KIB         # the second tile is ragged
    got, names = launch(case)
    check_against_float64(case, got, names)
    one = _single_column_launch(case.family)
    main = MAIN[case.family]
    # rows matched: the sweep's inputs are cut out of one draw, so row b, column 0 is the K = 1 launch's row b
    assert torch.equal(got["x_out"], one["x_out"][:case.B])
    assert torch.equal(got[main][..., 0, :], one[main][:case.B][..., 0, :]), main
    if "cot_cond" in got:
        assert torch.equal(got["cot_cond"][:, 0], one["cot_cond"][:case.B, 0])
    if "record" in got:
        assert torch.equal(got["record"], one["record"][:, :case.B])


# ---- the bitwise properties, where the stash is 140+ KiB -------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CEILING if c.family in ("pull", "discrete") and c.K == 1 and c.B == 9], ids=_id)
def test_bitwise_properties_at_the_ceiling(case):
    assert lds_bytes(case) >= 140 * KIB
    got, _ = launch(case)
    again, _ = launch(case)
    assert got.keys() == again.keys() and all(torch.equal(got[k], again[k]) for k in got)          # a re-run
    rows = slice(3, 8)                                                                            # a batch slice is the whole's
    part, _ = launch(case, rows=rows)
    for k in got:
        whole = got[k][:, rows] if k == "record" else got[k][rows]
        assert torch.equal(part[k], whole), k
    _, w, _, _ = case_inputs(case)
    zero, _ = launch(case, w=torch.zeros_like(w))                                                 # zero cotangents: exact zeros
    assert bool((zero["cot_x"] == 0).all()) and ("cot_cond" not in zero or bool((zero["cot_cond"] == 0).all()))
    assert torch.equal(zero["x_out"], got["x_out"])
    # the state is the state-only solve of the same model, bit for bit: the forward solve's for the record launch, and for
    # the pull launch the retraced state against the solve over the reversed span from the same start
    front, _ = build(case)
    x, _, c, _ = case_inputs(case)
    t_span, opts = span_of(front, case.direction), options_of(front, case.direction, case.nsteps)
    c_net = front._norm_cond(c) if (case.kind == "flow" and case.C) else c
    dev = lambda t: None if t is None else t.to(DEV, torch.float32).contiguous()
    solo = forward_state(front, x, t_span, case.method, opts, c_net, {})
    assert torch.equal(got["x_out"], solo.cpu())
    if case.family == "pull":
        back, _ = odeint.solve(front.to(DEV), solo, torch.flip(t_span, dims=(0,)), case.method, opts, _native.MODE_STATE, 0.0, 0.0,
                               cond=dev(c_net))
        same = torch.equal(got["retraced"], back.cpu())
        print(f"\n[derivative_depth] {_id(case)}: retraced state against the reversed state-only solve: bitwise {same}, "
              f"max diff {float((got['retraced'] - back.cpu()).abs().max()):.3e}")
        assert same
