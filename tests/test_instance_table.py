"""CPU tier: the instance table (tests/_instances.py) against the planner and the kernel registry.  The planner is host code
of the built library, so this runs without a GPU; tests/test_gpu_instances.py then runs every row on the GPU.

* every row plans to the instance it names, in every mode the row stands for;
* the rows cover every registry entry, each with a top and a bottom corner (the missing ones are named);
* a top corner is the instance's real limit: the plan's registers hold exactly D / C and the widest layer is the plan's
  width, and one step past it (D + 1, C + 1, width + 1) plans to another instance or to none;
* a bottom corner is the smallest shape on the instance: one step below it (D - 1, C - 1, width - 1) plans elsewhere;
* each instance's launch kinds (ff_mlp_launch_kind under FF_COOP=0 / 1 and at a batch just past one round of the chip)
  are the ones build.py declares and the GPU test runs."""
import re

from tests._instances import (ACT_CODES, ONE_WAVE, ROWS, TAIL, TWIN, chip_tiles, launch_kinds, plan_modes, plan_row,
                              registry)


def _library_names(lib):
    return [lib.ff_kernel_name(i).decode() for i in range(lib.ff_kernel_count())]


def test_registry_matches_the_build_declaration(built_library):
    assert sorted(_library_names(built_library)) == sorted(registry())


def test_every_row_plans_to_its_instance(built_library):
    wrong = []
    for r in ROWS:
        for mode in plan_modes(r):
            got = plan_row(r, mode)
            if got != r.kernel:
                wrong.append((r, mode, got))
    assert not wrong, "\n".join(map(str, wrong))


def test_rows_cover_every_registry_entry(built_library):
    names = _library_names(built_library)
    missing = [n for n in names if not any(r.kernel == n for r in ROWS)]
    assert not missing, f"registry entries without a row in tests/_instances.py: {missing}"
    one_sided = [n for n in names if {r.corner for r in ROWS if r.kernel == n} != {"top", "bottom"}]
    assert not one_sided, f"registry entries without both a top and a bottom corner: {one_sided}"
    unknown = sorted({r.kernel for r in ROWS} - set(names))
    assert not unknown, f"rows naming no registry entry: {unknown}"
    # run-time-activation instances (_a9): a row per non-SiLU activation; compiled-in ones (_a<k>): that activation
    non_silu = set(ACT_CODES) - {"silu"}
    acts = {n: ({a for a, c in ACT_CODES.items() if c == int(n.rsplit("_a", 1)[1])} if re.search(r"_a\d$", n) else {"silu"})
            for n in names}
    acts.update({n: non_silu for n in names if n.endswith("_a9")})
    short = [(n, sorted(a - {r.act for r in ROWS if r.kernel == n})) for n, a in acts.items()
             if not a <= {r.act for r in ROWS if r.kernel == n}]
    assert not short, f"registry entries missing a row for an activation they serve: {short}"


def _limits(r, mode):
    """(largest D, largest C, width) the plan of a row holds (ff_mlp_plan_t: registers per lane, tile, on-chip width)."""
    from flowfusion_amd import _native as N
    from flowfusion_amd.fused import activation_spec
    from tests._instances import act_module
    p = N.make_plan(r.D, r.C, list(r.units), mode, activation_spec(act_module(r.act)), N.PRECISIONS[r.prec])
    if r.prec == "f32":
        per_reg = 64 // p.tile
        return p.dregs * per_reg, p.cregs * per_reg, p.width
    return 2 * p.dregs, (16 if p.cregs else 0), p.width          # split: 8 registers per 16-dimension state tile


def _widen(units, by):
    w = max(units)
    return tuple(u + by if u == w else u for u in units)


def test_top_corners_are_the_instance_limits(built_library):
    bad = []
    for r in (r for r in ROWS if r.corner == "top"):
        mode = plan_modes(r)[0]
        d_max, c_max, width = _limits(r, mode)
        # (a conditional-free instance of the f32 family has no conditional registers: its top corner has C = 0)
        if (r.D, r.C, max(r.units)) != (d_max, c_max, width):
            bad.append((r, "limits", (d_max, c_max, width)))
        for what, kw in (("D + 1", dict(D=r.D + 1)), ("C + 1", dict(C=r.C + 1)), ("width + 1", dict(units=_widen(r.units, 1)))):
            nxt = plan_row(r, mode, **kw)
            if nxt == r.kernel:
                bad.append((r, what, nxt))
    assert not bad, "\n".join(map(str, bad))


def test_bottom_corners_are_the_smallest_shapes_on_the_instance(built_library):
    bad = []
    for r in (r for r in ROWS if r.corner == "bottom"):
        mode = plan_modes(r)[0]
        steps = []
        if r.D > 1:
            steps.append(("D - 1", dict(D=r.D - 1)))
        if r.C > 0:
            steps.append(("C - 1", dict(C=r.C - 1)))
        if max(r.units) > 1:
            steps.append(("width - 1", dict(units=tuple(min(u, max(r.units) - 1) for u in r.units))))
        for what, kw in steps:
            nxt = plan_row(r, mode, **kw)
            if nxt == r.kernel:
                bad.append((r, what, nxt))
    assert not bad, "\n".join(map(str, bad))


def test_launch_kinds_per_instance(built_library, monkeypatch):
    from flowfusion_amd import _native as N
    from flowfusion_amd.fused import activation_spec
    from tests._instances import act_module
    names = {N.LAUNCH_ONE_WAVE: ONE_WAVE, N.LAUNCH_TWIN: TWIN, N.LAUNCH_ONE_WAVE_AND_TWIN: TAIL}
    reg = registry()
    bad = []
    for name, entry in reg.items():
        r = next(r for r in ROWS if r.kernel == name and r.corner == "top")
        mode = plan_modes(r)[0]
        p = N.make_plan(r.D, r.C, list(r.units), mode, activation_spec(act_module(r.act)), N.PRECISIONS[r.prec])
        spt = N.samples_per_workgroup(p, mode) // (1 if name.endswith("_wide") or r.prec != "f32" else 4)
        seen = set()
        monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
        for pin in ("0", "1"):
            monkeypatch.setenv("FF_COOP", pin)
            seen.add(names[N.launch_kind(p, 7 * spt - 1, mode)])
        monkeypatch.delenv("FF_COOP")
        seen.add(names[N.launch_kind(p, (chip_tiles(entry) + 3) * spt - 1, mode)])
        if seen != set(launch_kinds(entry)):
            bad.append((name, sorted(seen), launch_kinds(entry)))
    n_one = sum(1 for e in reg.values() if e[0] == "f32")
    n_twin = sum(1 for e in reg.values() if e[0] != "split" and e[2])
    n_one_twin = sum(1 for e in reg.values() if e[0] == "f32" and e[2])
    n_split = sum(1 for e in reg.values() if e[0] == "split")
    print(f"\n[instances] {len(reg)} registry entries: {n_one} f32 one-wavefront kernels ({n_one_twin} with a cooperative twin), "
          f"{n_twin - n_one_twin} wide catch-alls (twin only), {n_twin} cooperative kernels in all, {n_split} split-precision "
          f"kernels; {len(ROWS)} table rows")
    assert not bad, "\n".join(map(str, bad))
