"""CPU tier: the instance table of the two-network kernels (tests/_pair_instances.py) against the pair planner, the pair
registry and the packed weights.  The planner and the packer are host code of the built library, so this runs without a GPU;
tests/test_gpu_pair_instances.py then runs every row on the GPU.

* the table and the library agree in both directions (ff_pair_kernel_count / ff_pair_kernel_name, build.PAIR_INSTANCES), and
  every instance has its three corners: the missing ones are named;
* every row plans to its instance, and to the matching mlp_pairsel_* with select=True;
* a top corner is the instance's limit (the plan's state and conditional registers hold exactly 2D = 32 and C = 16 features;
  D + 1, C + 1 plan to nothing, width + 1 to another instance or to nothing); a bottom corner is the smallest shape on the
  instance (width - 1 plans to the narrower one);
* each instance's launch kinds, pair and select, asked of ff_mlp_launch_kind, are the ones the GPU test runs;
* the pack at every row: the float64 emulations of the pair loop and of the row-select loop on the product's packed
  weights and tables against float64 Euler and leapfrog loops written on SymplecticRef.forward, with the gained weights;
* what makes the GPU tier's bars meaningful, on the reference alone: the fp32 torch evaluation of the same solves lies
  within an eighth of the bar of float64, and each of the four 1e-3 weight perturbations moves the float64 result by at
  least three times the bar."""
import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.fused import MODE_STATE
from tests import _pair_instances as T
from tests._pair_instances import CORNERS, ONE_WAVE, PAIR, ROWS, SELECT, TAIL, TWIN
from tests._symplectic_ref import SymplecticRef
from tests.test_symplectic_host import _emulate_pair
from tests.test_symplectic_leapfrog_host import emulate_select, leapfrog_f64

STATE_TOL = 2e-5        # the GPU tier's bar (tests/test_gpu_symplectic.py), relative to max |reference state|
LOGP_TOL = 2e-5         # and its bar on log-densities, relative with a floor of 1
HOST_TOL = 1e-5         # tests/test_symplectic_host.py: the emulated pack against the restatement
ROW_IDS = [f"{r.kernel}-{r.corner}" for r in ROWS]
_cache = {}


def case(row):
    """(model, state_dict, float64 restatement, inputs of the control batch, its sampled rows), built once per row."""
    if row not in _cache:
        fm = T.gained_model(row, T.SEED)
        sd = {k: v.detach().clone() for k, v in fm.state_dict().items()}
        e = T.registry()[row.kernel]
        B = T.control_batch(e.tile)
        _cache[row] = (fm, sd, SymplecticRef(sd), T.draw(row, B, T.SEED), T.sample_rows(B, e.tile, T.chip_tiles(e), T.SEED + B))
    return _cache[row]


def _library_names(lib):
    return [lib.ff_pair_kernel_name(i).decode() for i in range(lib.ff_pair_kernel_count())]


def test_table_and_library_agree(built_library):
    names = _library_names(built_library)
    reg = T.registry()
    missing = [n for n in list(reg) + names if not any(r.kernel == n for r in ROWS)]
    assert not missing, f"pair instances without a row in tests/_pair_instances.py: {sorted(set(missing))}"
    assert sorted(names) == sorted(reg)
    short = [(n, sorted(set(CORNERS) - {r.corner for r in ROWS if r.kernel == n})) for n in reg
             if sorted(r.corner for r in ROWS if r.kernel == n) != sorted(CORNERS)]
    assert not short, f"pair instances without exactly one top, bottom and split row: {short}"
    unknown = sorted({r.kernel for r in ROWS} - set(reg))
    assert not unknown, f"rows naming no pair instance: {unknown}"
    from flowfusion_amd import build as B
    assert all(i in B.PAIR_INSTANCES for i in B.PAIR_SELECT_INSTANCES)
    assert all(e.select for e in reg.values()), "a pair instance without a row-select variant: the GPU tier's coverage shrinks"


def test_every_row_plans_to_its_instance_and_its_select_variant(built_library):
    wrong = []
    for r in ROWS:
        for v in T.variants(T.registry()[r.kernel]):
            got, plan = T.plan_row(r, select=v == SELECT)
            if got != T.variant_name(r.kernel, v) or _native.is_select_plan(plan) != (v == SELECT):
                wrong.append((r, v, got))
    assert not wrong, "\n".join(map(str, wrong))


def _widen(units, by):
    w = max(units)
    return tuple(u + by if u == w else u for u in units)


def test_top_corners_are_the_instance_limits(built_library):
    bad = []
    for r in (r for r in ROWS if r.corner == "top"):
        for select in (False, True):
            name, p = T.plan_row(r, select)
            per_reg = 64 // p.tile
            if (p.dregs * per_reg, p.cregs * per_reg, p.width) != (32, 16, max(r.units)) or (2 * r.D, r.C) != (32, 16):
                bad.append((r, select, "limits", (p.dregs * per_reg, p.cregs * per_reg, p.width)))
            for what, kw in (("D + 1", dict(D=r.D + 1)), ("C + 1", dict(C=r.C + 1))):
                if T.plan_row(r, select, **kw)[0] is not None:
                    bad.append((r, select, what, T.plan_row(r, select, **kw)[0]))
            if T.plan_row(r, select, units=_widen(r.units, 1))[0] == name:
                bad.append((r, select, "width + 1", name))
    assert not bad, "\n".join(map(str, bad))


def test_bottom_corners_are_the_smallest_shapes_on_the_instance(built_library):
    widths = sorted(e.width for e in T.registry().values())
    bad = []
    for r in (r for r in ROWS if r.corner == "bottom"):
        if (r.D, r.C, len(r.units)) != (1, 0, 1):
            bad.append((r, "not the smallest state, conditional width and depth"))
        w = T.registry()[r.kernel].width
        below = [x for x in widths if x < w]
        if not below:
            if r.units != (1,):
                bad.append((r, "the narrowest instance starts at width 1"))
            continue
        for select in (False, True):
            narrower = next(n for n, e in T.registry().items() if e.width == below[-1])
            got = T.plan_row(r, select, units=(r.units[0] - 1,))[0]
            if got != T.variant_name(narrower, SELECT if select else PAIR):
                bad.append((r, select, "width - 1", got))
    assert not bad, "\n".join(map(str, bad))


def test_launch_kinds_per_instance_and_variant(built_library, monkeypatch):
    names = {_native.LAUNCH_ONE_WAVE: ONE_WAVE, _native.LAUNCH_TWIN: TWIN, _native.LAUNCH_ONE_WAVE_AND_TWIN: TAIL}
    bad = []
    for name, e in T.registry().items():
        r = next(r for r in ROWS if r.kernel == name and r.corner == "top")
        for v in T.variants(e):
            _, p = T.plan_row(r, select=v == SELECT)
            tile = int(p.tile)
            assert tile == e.tile and _native.samples_per_workgroup(p, MODE_STATE) == 4 * tile
            monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
            seen = []
            for pin in ("0", "1"):
                monkeypatch.setenv("FF_COOP", pin)
                seen.append(names[_native.launch_kind(p, 7 * tile - 1, MODE_STATE)])
            monkeypatch.delenv("FF_COOP")
            seen.append(names[_native.launch_kind(p, (T.chip_tiles(e) + 3) * tile - 1, MODE_STATE)])
            want = T.launch_kinds(e) if e.coop else [ONE_WAVE] * 3
            if seen != want:
                bad.append((name, v, seen, want))
    cov = T.expected_coverage()
    count = lambda v, k: len({c[0] for c in cov if c[1] == v and c[2] == k})
    print(f"\n[pair-instances] {len(T.registry())} pair instances, {len(ROWS)} table rows; launchers the GPU tier runs: "
          + ", ".join(f"{count(PAIR, k)} + {count(SELECT, k)} {k}" for k in (ONE_WAVE, TWIN, TAIL)) + f"; {len(cov)} cells")
    assert not bad, "\n".join(map(str, bad))
    assert [count(PAIR, k) + count(SELECT, k) for k in (ONE_WAVE, TWIN, TAIL)] == [6, 4, 4]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_pack_at_every_row(built_library, row):
    """_emulate_pair on the product's Euler table and emulate_select on its leapfrog table, both on the product's packed
    weights, against float64 loops on SymplecticRef.forward: gained weights, STEPS steps, the whole state."""
    fm, sd, ref, (z, _, _, _, cond), idx = case(row)
    z = z[idx]
    cond = None if cond is None else cond[idx]
    net = fm._net()
    wpack = net.wpack("cpu", MODE_STATE)
    cond_n = fm._norm_cond(cond)
    c64 = ref.norm_cond(cond)
    grid = T.grid()
    got = _emulate_pair(net.plan(MODE_STATE), wpack, fm._ode_table(grid, "euler", None, MODE_STATE), z, cond_n)
    err_e = T.rel_to_max(got, T.euler(ref.forward, z.double(), grid, c64))
    got = emulate_select(net.plan(MODE_STATE, select=True), wpack, fm._leapfrog_table(grid), z, cond_n)
    err_l = T.rel_to_max(got, leapfrog_f64(ref, z, grid, c64))
    print(f"\n[pair-instances] pack {row.kernel} {row.corner}: euler {err_e:.2e}, leapfrog {err_l:.2e}")
    assert err_e < HOST_TOL and err_l < HOST_TOL, (row, err_e, err_l)


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_the_bars_can_tell_on_these_inputs(row):
    """Per row, at the table's seed, on the reference alone: (a) the fp32 torch evaluation of the Euler, leapfrog and RK4
    solves and of the leapfrog log-density is within bar / 8 of float64; (b) every control moves the float64 Euler and
    leapfrog states by at least 3 x bar, on the sampled rows of the batch the GPU tier's negative controls run.  A row or
    seed that misses either needs another seed, not other factors."""
    fm, sd, ref, (z, x, p0, _, cond), idx = case(row)
    c64 = ref.norm_cond(cond)
    c32 = fm._norm_cond(cond)
    f32 = T.fp32_forward(fm)
    grid = T.grid()
    back = grid.flip(0)
    z0 = torch.cat([(x - fm.shift) / fm.scale, p0], dim=1)
    z0_64 = torch.cat([(x.double() - ref.shift) / ref.scale, p0.double()], dim=1)
    lp64 = T.log_density(leapfrog_f64(ref, z0_64, back, c64), p0, ref.scale)
    lp32 = T.log_density(T.leapfrog(f32, z0, back, c32), p0, fm.scale)
    floors = {"euler": T.rel_to_max(T.euler(f32, z, grid, c32), T.euler(ref.forward, z.double(), grid, c64)),
              "leapfrog": T.rel_to_max(T.leapfrog(f32, z, grid, c32), leapfrog_f64(ref, z, grid, c64)),
              "rk4": T.rel_to_max(T.rk4_38(f32, z0, T.rk4_nodes(), c32), T.rk4_38(ref.forward, z0_64, T.rk4_nodes(), c64)),
              "rk4_classic": T.rel_to_max(T.rk4_classic(f32, z0, T.rk4_nodes(), c32),
                                          T.rk4_classic(ref.forward, z0_64, T.rk4_nodes(), c64)),
              "leapfrog_logp": float(((lp32 - lp64).abs() / lp64.abs().clamp_min(1.0)).max())}
    zi = z[idx].double()
    ci = None if c64 is None else c64[idx]
    base = {"euler": T.euler(ref.forward, zi, grid, ci), "leapfrog": leapfrog_f64(ref, zi, grid, ci)}
    field = float(ref.forward(1.0, zi, ci).abs().max())
    moves = {}
    for name, bad_sd in T.controls(sd, row.D, row.C).items():
        bad = SymplecticRef(bad_sd)
        moves[name] = (T.rel_to_max(base["euler"], T.euler(bad.forward, zi, grid, ci)),
                       T.rel_to_max(base["leapfrog"], leapfrog_f64(bad, zi, grid, ci)))
    print(f"\n[pair-instances] floors {row.kernel} {row.corner} seed {T.SEED}: max |v| {field:.1f}, max |z| {float(zi.abs().max()):.1f}; fp32 - f64 "
          + ", ".join(f"{k} {v:.1e}" for k, v in floors.items()) + "; controls (euler, leapfrog) "
          + ", ".join(f"{k} {a:.1e} {b:.1e}" for k, (a, b) in moves.items()))
    assert set(moves) == set(T.CONTROLS) - ({"cond_col"} if row.C == 0 else set())
    for k, v in floors.items():
        assert v < (LOGP_TOL if k.endswith("logp") else STATE_TOL) / 8, (row, k, v)
    for k, (a, b) in moves.items():
        assert a >= 3 * STATE_TOL and b >= 3 * STATE_TOL, (row, k, a, b)
