"""GPU tier: every two-network kernel -- the mlp_pair_* instances, their row-select mlp_pairsel_* variants and the cooperative
twins of both -- in every launch kind it serves, at the corners of its envelope, against float64.  Driven by the table of
tests/_pair_instances.py, whose planner, registry and packed-weight side tests/test_pair_instance_table.py checks on the CPU.

For each table row (top, bottom and split corner of an instance) and each variant, through the product's own entry points:

* launch kinds, each asserted with ff_mlp_launch_kind before it runs: the one-wavefront kernel (FF_COOP=0), the cooperative
  twin (FF_COOP=1) and whole rounds of the chip on the one-wavefront kernel with the leftover tiles on the twin; batches of
  1 row, a partly filled last tile one or three tiles past a multiple of the four-tile workgroup, three tiles on the twin,
  a round of the chip and three tiles for the tail split;
* pair modes: ``euler`` (_integrate on linspace(1, 0, 4)); ``rk4`` (odeint.solve over [0, 1] at step 0.25 as _log_prob_from
  calls it -- four stage slots per step -- and _log_prob_from's log-density of the same solve, for ``method="rk4"``, which
  is torchdiffeq's rk4, Kutta's 3/8 rule, and for ``method="rk4_classic"``, the classical weights, each against that rule
  written here in float64); ``attempt`` (a raw ff_mlp_ode_launch with k1_in, five attempt-style rows and aux_out[0], on the
  one-wavefront kernel and the twin, top and split rows: against the float64 emulation of the pair loop on the packed
  weights, itself held against the same stages written on SymplecticRef.forward);
* select modes: ``leapfrog`` (_integrate on the same grid, 7 rows) and ``leapfrog_logp`` (_log_prob_from on the flipped grid);
* the reference is tests/_symplectic_ref.SymplecticRef in float64 on at most 32 rows of each batch (first tile, workgroup
  boundaries, the last row of the whole rounds and the first past it, the last two rows, seeded others).

Always the whole state [B, 2D], relative to max |reference|, under STATE_TOL (2e-5) of tests/test_gpu_symplectic.py;
log-densities under its _logp_err bar of 2e-5.  The inputs are the gained weights of tests/_pair_instances.py: on them the
fp32 arithmetic alone stays under an eighth of the bar and a 1e-3 error in an edge weight moves the result by three times
the bar or more (asserted on the CPU).  A negative control per kernel and variant compares the top row's GPU output with
the float64 solve of each of the four perturbed weight sets: every one must MISS the bar.  The last test asserts that the
(kernel, variant, launch kind, mode) cells that passed are exactly the ones the table says exist (it needs the whole file to
have run)."""
import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd.fused import MODE_STATE
from tests import _pair_instances as T
from tests._pair_instances import ONE_WAVE, PAIR, ROWS, SELECT, TAIL, TWIN
from tests._symplectic_ref import SymplecticRef
from tests.test_gpu_symplectic import STATE_TOL, _logp_err
from tests.test_gpu_symplectic_twin import attempt_table, raw_launch
from tests.test_symplectic_host import _emulate_pair
from tests.test_symplectic_leapfrog_host import leapfrog_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGP_TOL = 2e-5                      # tests/test_gpu_symplectic.py: log_prob against its anchors
HOST_TOL = 1e-5                      # tests/test_symplectic_host.py: the emulated pack against the restatement
REGISTRY = T.registry()
PASSED = set()                       # (kernel, variant, launch kind, mode) cells that met their bar
CONTROL_ERRS = {}                    # (kernel, variant) -> {control: perturbed error}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _case(row):
    """(model on the GPU, state_dict, float64 restatement), built once per row."""
    if row not in _cache:
        fm = T.gained_model(row)
        sd = {k: v.detach().clone() for k, v in fm.state_dict().items()}
        _cache[row] = (fm.to(DEV), sd, SymplecticRef(sd))
    return _cache[row]


def _pin(monkeypatch, kind):
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    if kind == TAIL:
        monkeypatch.delenv("FF_COOP", raising=False)
    else:
        monkeypatch.setenv("FF_COOP", "1" if kind == TWIN else "0")


def _check_kind(plan, B, kind):
    code = {ONE_WAVE: _native.LAUNCH_ONE_WAVE, TWIN: _native.LAUNCH_TWIN, TAIL: _native.LAUNCH_ONE_WAVE_AND_TWIN}[kind]
    got = _native.launch_kind(plan, B, MODE_STATE)
    assert got == code, (_native.kernel_name(plan), B, got, kind)


def _dev(t):
    return None if t is None else t.to(DEV)


def _report(name, variant, kind, mode, B, err):
    print(f"[pair-instances] {name} {variant} {kind} {mode} {B} {err:.2e}")


def _attempt_stages(ref, z, k1, c64):
    """tests/test_gpu_symplectic_twin.attempt_table's five rows on the restatement's dynamics: stage slot 0 is k1; row i
    fills slot i + 1 from y + 0.1 k[0] + 0.05 k[i] at t_i of linspace(0.2, 0.8, 5); the last row ends the step,
    x += 0.2 sum_s k[s]; aux_0 = x + 0.2 sum_s k[s]."""
    c = lambda v: float(torch.tensor(v, dtype=torch.float32))
    ks = [k1.double()]
    z = z.double()
    for i, t in enumerate(torch.linspace(0.2, 0.8, 5)):
        y = z + c(0.1) * ks[0] + (c(0.05) * ks[i] if i else 0.0)
        ks.append(ref.forward(float(t), y, c64))
    x = z + c(0.2) * sum(ks)
    return x, x + c(0.2) * sum(ks)


def _run_row(row, variant, monkeypatch):
    e = REGISTRY[row.kernel]
    fm, sd, ref = _case(row)
    net = fm._net()
    select = variant == SELECT
    plan = net.plan(MODE_STATE, select=select)
    name = T.variant_name(row.kernel, variant)
    assert _native.kernel_name(plan) == name, (row, variant)
    tile, chip = e.tile, T.chip_tiles(e)
    grid = T.grid()
    span = torch.tensor([0.0, 1.0])
    rk_opts = {"step_size": T.RK4_STEP}
    for kind in T.launch_kinds(e):
        done = set()
        for B in T.batches(kind, row.corner, tile, chip):
            z, x, p0, k1, cond = T.draw(row, B)
            idx = T.sample_rows(B, tile, chip, T.SEED + B)
            zd, xd, pd, cd = z.to(DEV), x.to(DEV), p0.to(DEV), _dev(cond)
            cn = fm._norm_cond(cd)
            c64 = ref.norm_cond(None if cond is None else cond[idx])
            z0_64 = torch.cat([(x[idx].double() - ref.shift) / ref.scale, p0[idx].double()], dim=1)
            for mode in T.solve_modes(variant, kind):
                if mode == "attempt" and row.corner == "bottom":
                    continue
                tag = (row, variant, kind, mode, B)
                _pin(monkeypatch, kind)
                _check_kind(plan, B, kind)
                if mode == "euler":
                    got = fm._integrate(zd, grid, cn, "euler")
                    err = T.rel_to_max(got.cpu()[idx], T.euler(ref.forward, z[idx].double(), grid, c64))
                    _report(name, variant, kind, mode, B, err)
                    assert err < STATE_TOL, tag + (err,)
                elif mode == "rk4":
                    z0 = torch.cat([(xd - fm.shift) / fm.scale, pd], dim=-1)
                    for method, rule in (("rk4", T.rk4_38), ("rk4_classic", T.rk4_classic)):
                        got, _ = odeint.solve(fm, z0, span, method, rk_opts, MODE_STATE, None, None, cond=cn)
                        want = rule(ref.forward, z0_64, T.rk4_nodes(), c64)
                        err = T.rel_to_max(got.cpu()[idx], want)
                        lp = fm._log_prob_from(xd, pd, cd, method=method, options=rk_opts)
                        err_l = _logp_err(lp.cpu()[idx], T.log_density(want, p0[idx], ref.scale))
                        _report(name, variant, kind, method, B, err)
                        _report(name, variant, kind, method + "/logp", B, err_l)
                        assert err < STATE_TOL and err_l < LOGP_TOL, tag + (method, err, err_l)
                elif mode == "attempt":
                    tab = attempt_table(fm, 5)
                    out, aux = raw_launch(_native.lib(), plan, net.wpack(DEV, MODE_STATE), zd, tab, 5, cond=cn, k1=k1.to(DEV),
                                          n_aux=1, FF_COOP=1 if kind == TWIN else 0)
                    cn_i = None if cn is None else cn.cpu()[idx]
                    want = _emulate_pair(plan, net.wpack("cpu", MODE_STATE), tab.cpu(), z[idx], cn_i, k1=k1[idx], n_aux=1)
                    direct = _attempt_stages(ref, z[idx], k1[idx], c64)
                    for w, d in zip(want, direct):
                        assert T.rel_to_max(w, d) < HOST_TOL, tag + ("emulation against the restatement", T.rel_to_max(w, d))
                    err, err_a = T.rel_to_max(out.cpu()[idx], want[0]), T.rel_to_max(aux.cpu()[idx], want[1])
                    _report(name, variant, kind, mode, B, err)
                    _report(name, variant, kind, mode + "/aux", B, err_a)
                    assert err < STATE_TOL and err_a < STATE_TOL, tag + (err, err_a)
                elif mode == "leapfrog":
                    got = fm._integrate(zd, grid, cn, "leapfrog")
                    err = T.rel_to_max(got.cpu()[idx], leapfrog_f64(ref, z[idx], grid, c64))
                    _report(name, variant, kind, mode, B, err)
                    assert err < STATE_TOL, tag + (err,)
                else:
                    assert mode == "leapfrog_logp"
                    lp = fm._log_prob_from(xd, pd, cd, method="leapfrog", num_steps=T.STEPS)
                    want = T.log_density(leapfrog_f64(ref, z0_64, grid.flip(0), c64), p0[idx], ref.scale)
                    err = _logp_err(lp.cpu()[idx], want)
                    _report(name, variant, kind, mode, B, err)
                    assert err < LOGP_TOL, tag + (err,)
                done.add(mode)
        PASSED.update((name, variant, kind, mode) for mode in done)


CASES = [(r, v) for r in ROWS for v in T.variants(REGISTRY[r.kernel])]


@pytest.mark.parametrize("row,variant", CASES, ids=[f"{r.kernel}-{r.corner}-{v}" for r, v in CASES])
def test_pair_instance_against_float64(row, variant, monkeypatch):
    print()
    _run_row(row, variant, monkeypatch)


CONTROL_CASES = [(k, v) for k, e in REGISTRY.items() for v in T.variants(e)]


@pytest.mark.parametrize("kernel,variant", CONTROL_CASES, ids=[f"{k}-{v}" for k, v in CONTROL_CASES])
def test_negative_control_sees_the_edge_weights(kernel, variant, monkeypatch):
    """Per kernel and variant, on its top row (every state and conditional register live) in the one-wavefront kind: the
    Euler / leapfrog state meets STATE_TOL against the float64 solve, and MISSES it against the float64 solve of each
    perturbed weight set: the last output row of mlp_q, of mlp_p, the last conditional column and the last state column of
    both first layers, each off by 1e-3 relative."""
    e = REGISTRY[kernel]
    row = next(r for r in ROWS if r.kernel == kernel and r.corner == "top")
    fm, sd, ref = _case(row)
    plan = fm._net().plan(MODE_STATE, select=variant == SELECT)
    name = T.variant_name(kernel, variant)
    assert _native.kernel_name(plan) == name
    B = T.control_batch(e.tile)
    _pin(monkeypatch, ONE_WAVE)
    _check_kind(plan, B, ONE_WAVE)
    z, _, _, _, cond = T.draw(row, B)
    idx = T.sample_rows(B, e.tile, T.chip_tiles(e), T.SEED + B)
    grid = T.grid()
    method = "leapfrog" if variant == SELECT else "euler"
    got = fm._integrate(z.to(DEV), grid, fm._norm_cond(_dev(cond)), method).cpu()[idx]

    def solve(r):
        c64 = r.norm_cond(cond[idx])
        return leapfrog_f64(r, z[idx], grid, c64) if variant == SELECT else T.euler(r.forward, z[idx].double(), grid, c64)
    err = T.rel_to_max(got, solve(ref))
    assert err < STATE_TOL, (row, variant, err)
    errs = {k: T.rel_to_max(got, solve(SymplecticRef(bad))) for k, bad in T.controls(sd, row.D, row.C).items()}
    print(f"\n[pair-instances] control {name} {variant} {method} {B}: true weights {err:.2e}; "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(errs) == set(T.CONTROLS)
    for k, v in errs.items():
        assert v > STATE_TOL, (row, variant, k, "the perturbed reference passed", v)
    CONTROL_ERRS[(name, variant)] = errs


def test_every_pair_kernel_kind_and_mode_passed():
    want = T.expected_coverage()
    print("\n[pair-instances] passed against float64:")
    for kind in (ONE_WAVE, TWIN, TAIL):
        for v in (PAIR, SELECT):
            names = sorted({c[0] for c in PASSED if c[1] == v and c[2] == kind})
            for n in names:
                print(f"  {kind} {n}: " + ", ".join(sorted(c[3] for c in PASSED if c[:3] == (n, v, kind))))
    print("[pair-instances] negative controls, smallest perturbed error: "
          + ", ".join(f"{n} {min(errs.values()):.1e}" for (n, v), errs in sorted(CONTROL_ERRS.items())))
    assert PASSED == want, (sorted(want - PASSED), sorted(PASSED - want))
    launchers = lambda v, kind: len({c[0] for c in PASSED if c[1] == v and c[2] == kind})
    assert [(launchers(PAIR, k), launchers(SELECT, k)) for k in (ONE_WAVE, TWIN, TAIL)] == [(3, 3), (2, 2), (2, 2)]
    assert set(CONTROL_ERRS) == {(T.variant_name(k, v), v) for k, v in CONTROL_CASES}, sorted(CONTROL_ERRS)
