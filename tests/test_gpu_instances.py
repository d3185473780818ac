"""GPU tier: every compiled kernel instance, in every launch kind it serves and every mode it carries, against the float64
oracle -- driven by the instance table of tests/_instances.py (whose planner and registry side tests/test_instance_table.py
checks on the CPU).

For each table row (a network at the top or the bottom corner of its instance), through the product classes:

* launch kinds, each asserted with ff_mlp_launch_kind before it runs: the one-wavefront kernel (FF_COOP=0), its cooperative
  twin (FF_COOP=1) where one exists, and the one-wavefront kernel with the leftover tiles on the twin (a batch of one round
  of the chip plus a few tiles); batches of 1 row, a partly filled last tile, and 1 or 3 tiles past a multiple of four (the
  one-wavefront kernel's last workgroup partly filled);
* modes: fixed-grid RK4 state solve and Euler-Maruyama with supplied noise on state-only instances (steps no longer than
  the explicit methods' stability limit at the VP schedule's beta_max = 20 allows: beyond it the fp32 rounding of the
  oracle's own arithmetic is amplified past the bars); Hutchinson and
  exact-trace forward solves (the divergence integral of solve_odes_forward: no prior term to cancel against) and the
  Jacobian output (host_stepper.RowStepper, against float64 autograd of the oracle's drift) on divergence-capable ones;
* the reference is oracle.ScoreOracle in float64, on a seeded set of at most 32 rows of each batch (first tile, workgroup
  boundaries, the last full round, the tail, the last row): fixed-grid rows are independent of each other.

Bars: STATE_TOL / LOGP_TOL (2e-5) of test_gpu_parity, 5e-5 on Jacobians, the split family's bars of
test_split_random_shapes_against_oracle (two-part log-densities at twice LOGP_TOL).  A negative control per kernel family
perturbs the oracle's last-layer weights of the highest state dimension by 1e-3 relative on a top-corner row: the same
comparison must then fail, which shows it reads the edge registers.  The last test asserts that the (instance, launch
kind, mode) triples that passed are exactly the ones the table says exist (it needs the whole file to have run)."""
import re

import pytest
import torch

from tests._instances import (ONE_WAVE, ROWS, TAIL, TWIN, act_module, chip_tiles, expected_coverage, launch_kinds,
                              registry, solve_modes)
from tests._util import max_rel
from tests.test_gpu_parity import DEV, LOGP_TOL, STATE_TOL

pytestmark = pytest.mark.gpu

JAC_TOL = 5e-5                       # test_jacobian_output_against_autograd
SDES = ("VPSDE", "VESDE", "SUBVPSDE")
PASSED = set()                       # (kernel, launch kind, mode) triples that met their bar
CONTROLS = {}                        # kernel family -> (perturbed error, row) of the negative control
REGISTRY = registry()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _family(name):
    m = re.match(r"mlp_ode_(m\d+_h\d+|split\d?_h\d+(?:_d2)?)", name)
    return m.group(1)


def _oracle(params, sde_name, no_sigma, act):
    from oracle import flowfusion_oracle as O
    sde = {"VPSDE": O.VP, "VESDE": O.VE, "SUBVPSDE": O.SubVP}[sde_name](dtype=torch.float64)
    return O.ScoreOracle(params, sde, no_sigma=no_sigma, dtype=torch.float64, activation=act)


def _model(row, seed):
    from flowfusion_amd import diffusion as Dm
    from oracle import flowfusion_oracle as O
    torch.manual_seed(seed)
    sde_name, no_sigma = SDES[seed % 3], seed % 2 == 0
    act = act_module(row.act)
    sm = Dm.ScoreModel(Dm.MLP(row.D, row.C, 8, list(row.units), activation=act), getattr(Dm, sde_name)(),
                       no_sigma=no_sigma, precision=row.prec).eval()
    params = O.mlp_params_from_state_dict({k: v.detach().clone() for k, v in sm.state_dict().items()})
    return sm.to(DEV), params, (sde_name, no_sigma, act)


def _sample_rows(B, spt, chip, seed):
    """At most 32 rows of a batch of B: the first tile, the boundaries of the first workgroups, the last full round of the
    chip and the first row past it, the last rows, and seeded others."""
    want = {0, 1, spt - 1, spt, 4 * spt - 1, 4 * spt, chip * spt - 1, chip * spt, chip * spt + 1, B - 2, B - 1}
    rows = sorted(i for i in want if 0 <= i < B)
    g = torch.Generator().manual_seed(seed)
    extra = torch.randperm(B, generator=g).tolist()
    for i in extra:
        if len(rows) >= 32:
            break
        if i not in rows:
            rows.append(i)
    return torch.tensor(sorted(rows))


def _batch(tiles, spt):
    return tiles * spt - 1 if spt > 1 else tiles             # (a partly filled last tile where a tile holds several rows)


def _batches(kind, corner, spt, chip):
    if kind == ONE_WAVE:                                      # 5 / 7 tiles: one / three tiles past a multiple of four
        return [1, _batch(5, spt)] if corner == "top" else [_batch(7, spt)]
    if kind == TWIN:
        return [1] if corner == "top" else [_batch(3, spt)]
    return [_batch(chip + 3, spt)]                            # a round of the chip and three tiles


def _pin(monkeypatch, kind):
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    if kind == TAIL:
        monkeypatch.delenv("FF_COOP", raising=False)
    else:
        monkeypatch.setenv("FF_COOP", "1" if kind == TWIN else "0")


def _check_kind(plan, B, mode, kind, counts=(0,), jac=False):
    """ff_mlp_launch_kind of every launch a solve makes (the tail split: the first, widest exact-trace pass)."""
    from flowfusion_amd import _native as N
    code = {ONE_WAVE: N.LAUNCH_ONE_WAVE, TWIN: N.LAUNCH_TWIN, TAIL: N.LAUNCH_ONE_WAVE_AND_TWIN}[kind]
    for c in (counts[:1] if kind == TAIL else counts):
        got = N.launch_kind(plan, B, mode, c, jac)
        assert got == code, (N.kernel_name(plan), B, mode, c, got, kind)


def _spt(plan, mode, count=0):
    """Rows per tile (f32) or per workgroup (split) of a launch."""
    from flowfusion_amd import _native as N
    if plan.precision != N.PREC_F32:
        return N.samples_per_workgroup(plan, mode)
    return plan.tile // (1 + (count if mode == N.MODE_EXACT else (1 if mode == N.MODE_HUTCH else 0)))


def _state(sm, x, cd, opts):
    return sm.sample_ode_from_base(x, conditional=cd, method="rk4", options=opts)[0]


def _run_row(row, seed, monkeypatch):
    from flowfusion_amd import _native as N, host_stepper
    from flowfusion_amd.fused import exact_trace_passes
    entry = REGISTRY[row.kernel]
    sm, params, (sde_name, no_sigma, act) = _model(row, seed)
    so = _oracle(params, sde_name, no_sigma, act)
    net = sm._net()
    eps = float(sm.sde.epsilon)
    D, C = row.D, row.C
    chip = chip_tiles(entry)
    bf16x2 = row.prec == "bf16x2"
    logp_tol = LOGP_TOL * (2 if bf16x2 else 1)
    g = torch.Generator().manual_seed(seed)
    for kind in launch_kinds(entry):
        for mode_name in solve_modes(entry, kind):
            mode = {"rk4": N.MODE_STATE, "em": N.MODE_STATE, "hutch": N.MODE_HUTCH, "exact": N.MODE_EXACT,
                    "jac": N.MODE_EXACT}[mode_name]
            plan = net.plan(mode)
            assert N.kernel_name(plan) == row.kernel, (row, mode_name)
            counts = tuple(c for _, c in exact_trace_passes(D, plan.tile)) if mode == N.MODE_EXACT else (0,)
            spt = _spt(plan, mode, counts[0])
            for B in _batches(kind, row.corner, spt, chip):
                tag = (row, kind, mode_name, B, sde_name, no_sigma)
                _pin(monkeypatch, kind)
                _check_kind(plan, B, mode, kind, counts, jac=mode_name == "jac")
                idx = _sample_rows(B, spt, chip, seed + B)
                x = torch.randn(B, D, generator=g)
                cond = torch.randn(B, C, generator=g) if C else None
                cd = None if cond is None else cond.to(DEV)
                c64 = None if cond is None else cond[idx].double()
                if mode_name == "rk4":
                    opts = {"step_size": (1.0 - eps) / 4}
                    got = _state(sm, x.to(DEV), cd, opts).cpu()[idx]
                    ref = so.sample_ode_from_base(x[idx].double(), c64, "rk4", opts)
                    err = max_rel(got, ref, floor=ref.abs().max().item())
                    assert err < STATE_TOL, tag + (err,)
                elif mode_name == "em":
                    steps = 6
                    scale = float(sm.sde.sigma_max) if hasattr(sm.sde, "sigma_max") else 1.0
                    prior = torch.randn(B, D, generator=g) * scale
                    noise = torch.randn(steps, B, D, generator=g)
                    it = iter(noise.to(DEV))
                    got = sm._sample_sde_from(prior.to(DEV), lambda like: next(it), cd, steps=steps).cpu()[idx]
                    ref = so.sample_sde(prior[idx].double(), [n[idx].double() for n in noise], c64, steps=steps)
                    err = max_rel(got, ref, floor=ref.abs().max().item())
                    assert err < STATE_TOL, tag + (err,)
                elif mode_name in ("hutch", "exact"):
                    opts = {"step_size": (1.0 - eps) / 4}
                    tab = sm._ode_table(torch.tensor([eps, 1.0]), "midpoint", opts, mode)
                    x0 = x * 0.5
                    e = torch.sign(torch.randn(B, D, generator=g)) if mode_name == "hutch" else None
                    xT, dl, status = net.integrate(x0.to(DEV), tab, mode, cond=cd, probe=None if e is None else e.to(DEV))
                    rx, rdl = so.solve_odes_forward(x0[idx].double(), c64, "midpoint", opts, mode_name,
                                                    None if e is None else e[idx].double())
                    # (the forward VP / sub-VP solve contracts the state by up to e^-5: its error is measured against the
                    # scale of the trajectory, max |x0|, |xT| -- against |xT| alone the fp32 oracle misses the bar itself)
                    err_x = max_rel(xT.cpu()[idx], rx, floor=max(rx.abs().max().item(), x0[idx].abs().max().item()))
                    err_l = max_rel(dl.cpu().view(-1)[idx], rdl.view(-1), floor=1.0)
                    assert err_x < STATE_TOL and err_l < logp_tol, tag + (err_x, err_l)
                else:                                          # jac: A[b] = J[b]^T of the right-hand side at t = 0.37
                    t = torch.tensor([0.37])
                    a, b, c1, _ = sm._schedule(t, "ode")
                    got = {}
                    xd = x.to(DEV)
                    st = host_stepper.RowStepper(net, xd.device, cd, lambda A: got.setdefault("A", A).new_zeros(B))
                    rhs, _ = st.rhs_div(xd, float(a[0]), float(b[0]), c1[0])
                    t64 = t.double()[0]
                    xs = x[idx].double()
                    f = lambda v: so.ode_drift(t64, v, c64)
                    with torch.enable_grad():
                        J = torch.autograd.functional.jacobian(lambda v: f(v).sum(0), xs, vectorize=True)   # [i, b, j]
                    want = J.permute(1, 2, 0)
                    r64 = f(xs)
                    err_r = max_rel(rhs.cpu()[idx], r64, floor=r64.abs().max().item())
                    err_j = max_rel(got["A"].cpu()[idx], want, floor=want.abs().max().item())
                    assert err_r < STATE_TOL and err_j < JAC_TOL, tag + (err_r, err_j)
                monkeypatch.delenv("FF_COOP", raising=False)
            PASSED.add((row.kernel, kind, mode_name))


@pytest.mark.parametrize("kernel", list(REGISTRY))
def test_instance_against_oracle(kernel, monkeypatch):
    rows = [(i, r) for i, r in enumerate(ROWS) if r.kernel == kernel]
    assert rows, f"no table row for {kernel}"
    for i, r in rows:
        _run_row(r, 7000 + i, monkeypatch)


def _control_model(row, seed):
    """A VP model without sigma normalisation whose last layer is scaled up (by 20 behind the five hidden layers of the f32
    top corners, by 2 behind the split family's one to four): the network's output is then of the order of the state, so
    that an error in one of its output rows shows in the solved state."""
    from flowfusion_amd import diffusion as Dm
    from oracle import flowfusion_oracle as O
    torch.manual_seed(seed)
    act = act_module(row.act)
    sm = Dm.ScoreModel(Dm.MLP(row.D, row.C, 8, list(row.units), activation=act), Dm.VPSDE(), no_sigma=True,
                       precision=row.prec).eval()
    with torch.no_grad():
        k = 20.0 if len(row.units) == 5 else 2.0
        sm.model.NN[-1].weight.mul_(k)
        sm.model.NN[-1].bias.mul_(k)
    params = O.mlp_params_from_state_dict({k: v.detach().clone() for k, v in sm.state_dict().items()})
    return sm.to(DEV), params, act


FAMILIES = {}
for _name in REGISTRY:
    FAMILIES.setdefault(_family(_name), _name)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_negative_control_sees_the_edge_register(family, monkeypatch):
    """Per kernel family, on the top corner (the highest state dimension in the last state register) of its first
    instance: the RK4 state solve meets STATE_TOL against the float64 oracle, and misses it when the oracle's last-layer
    weights of dimension D - 1 are off by 1e-3 relative."""
    from flowfusion_amd import _native as N
    name = FAMILIES[family]
    entry = REGISTRY[name]
    row = next(r for r in ROWS if r.kernel == name and r.corner == "top")
    assert row.mode == "state", row
    sm, params, act = _control_model(row, 9100 + list(FAMILIES).index(family))
    plan = sm._net().plan(N.MODE_STATE)
    assert N.kernel_name(plan) == name
    kind = ONE_WAVE if ONE_WAVE in launch_kinds(entry) else TWIN
    spt = _spt(plan, N.MODE_STATE)
    B = _batch(5, spt)
    _pin(monkeypatch, kind)
    _check_kind(plan, B, N.MODE_STATE, kind)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, row.D, generator=g)
    cond = torch.randn(B, row.C, generator=g) if row.C else None
    idx = _sample_rows(B, spt, chip_tiles(entry), 17)
    c64 = None if cond is None else cond[idx].double()
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / 16}
    got = _state(sm, x.to(DEV), None if cond is None else cond.to(DEV), opts).cpu()[idx]
    ref = _oracle(params, "VPSDE", True, act).sample_ode_from_base(x[idx].double(), c64, "rk4", opts)
    err = max_rel(got, ref, floor=ref.abs().max().item())
    assert err < STATE_TOL, (row, err)
    bad = params.to(torch.float64)
    bad.weights[-1][row.D - 1] *= 1.0 + 1e-3
    rb = _oracle(bad, "VPSDE", True, act).sample_ode_from_base(x[idx].double(), c64, "rk4", opts)
    perr = max_rel(got, rb, floor=rb.abs().max().item())
    assert perr > STATE_TOL, (row, "the perturbed oracle passed", perr)
    CONTROLS[family] = (perr, name)


def test_every_instance_kind_and_mode_passed():
    want = expected_coverage()
    by_kernel = {}
    for k, kind, mode in sorted(PASSED):
        by_kernel.setdefault(k, {}).setdefault(kind, []).append(mode)
    print("\n[instances] passed against the float64 oracle:")
    for k, kinds in by_kernel.items():
        print(f"  {k}: " + "; ".join(f"{kind}: {', '.join(m)}" for kind, m in kinds.items()))
    print("[instances] negative controls (perturbed error, instance): " +
          ", ".join(f"{fam} {e:.1e} ({k})" for fam, (e, k) in sorted(CONTROLS.items())))
    assert PASSED == want, (sorted(want - PASSED), sorted(PASSED - want))
    assert set(CONTROLS) == set(FAMILIES), sorted(CONTROLS)
