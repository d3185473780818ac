"""What the four custom ops hand to ff_mlp_ode_launch, recorded on the GPU and compared with a committed record.

tests/test_launch_records.py pins what the C ABI enqueues for a given ff_ode_args; this file pins the layer above it: which
ff_ode_args `torch.ops.flowfusion_amd.mlp_ode / mlp_ode_step / mlp_rhs_jac / mlp_ode_jacobians` fill for their arguments.
The bound `ff_mlp_ode_launch` of the loaded library is replaced by a Python recorder that reads the plan and the arguments
behind the two `byref`s, notes them and forwards to the real function: every recorded call is a real, valid launch.  A line
holds the integer fields verbatim and every pointer as `0`, the name of the input tensor it is, `out:<i>` (`out:<i>+<bytes>`
for the auxiliary outputs inside a returned tensor) or `scratch`; then the shapes, dtypes and devices of what the op
returned.  Faulty arguments (one fault per call) raise in Python before any launch: their record is the exception.

tests/op_records/expected.txt is the record of the commit BEFORE the four ops were folded onto one argument fill, never of
the code under test: its Python package, this tree's built library.  A change that means to alter what an op passes
regenerates it from a tree it trusts, in a fresh process:
    python tests/test_gpu_op_records.py --write <checkout of that commit> [<file>, default tests/op_records/expected.txt]
"""
import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
EXPECTED = ROOT / "tests" / "op_records" / "expected.txt"

_POINTERS = ("x_in", "x_out", "cond", "probe", "dlogp_out", "noise", "wpack", "etab", "in_shift", "in_scale", "out_scale",
             "out_shift", "status", "k1_in", "kl1_in", "dlogp_in", "jac_out", "gate")
_INTS = ("batch", "noise_stride", "n_evals", "mode", "tangent_first", "tangent_count", "n_aux", "rng_noise_base", "rng_seed",
         "rng_sample_offset", "jac_all", "stage_slots")
_PLAN = ("dim", "cond_dim", "n_hidden", "width", "dregs", "cregs", "kernel_id", "tile", "activation", "precision")


class _Recorder:
    """Stands where `lib().ff_mlp_ode_launch` stood: notes the plan and the arguments, then launches."""

    def __init__(self, real):
        self.real = real
        self.calls = []

    def __call__(self, plan_ref, args_ref, stream):
        p, a = plan_ref._obj, args_ref._obj
        call = {"plan": [int(getattr(p, f)) for f in _PLAN] + [float(v) for v in p.act_param],
                "ints": [int(getattr(a, f)) for f in _INTS],
                "ptrs": [int(getattr(a, f) or 0) for f in _POINTERS],
                "aux": [int(v or 0) for v in a.aux_out], "aux_lp": [int(v or 0) for v in a.aux_lp_out],
                "stream": (stream.value or 0) == torch.cuda.current_stream().cuda_stream}
        self.calls.append(call)
        return self.real(plan_ref, args_ref, stream)


def _name(ptr, inputs, outs):
    if ptr == 0:
        return "0"
    for name, t in inputs.items():
        if torch.is_tensor(t) and t.numel() and t.data_ptr() == ptr:
            return name
    for i, t in enumerate(outs):
        off = ptr - t.data_ptr() if t.numel() else -1
        if 0 <= off < t.numel() * t.element_size():
            return f"out:{i}" + (f"+{off}" if off else "")
    return "scratch"


def _line(call, inputs, outs):
    words = ["plan=" + ",".join(str(v) for v in call["plan"])]
    words += [f"{f}={v}" for f, v in zip(_INTS, call["ints"])]
    words += [f"{f}={_name(v, inputs, outs)}" for f, v in zip(_POINTERS, call["ptrs"])]
    words += [f"{f}=[" + ",".join(_name(v, inputs, outs) for v in call[f]) + "]" for f in ("aux", "aux_lp")]
    return " ".join(words + [f"stream_is_current={call['stream']}"])


def record() -> str:
    """The sweep (module docstring) through torch.ops.flowfusion_amd.* on the current GPU; returns the record's text."""
    from flowfusion_amd import _native as N
    from flowfusion_amd import solvers

    dev = torch.device("cuda", torch.cuda.current_device())
    ops = torch.ops.flowfusion_amd
    gen = torch.Generator().manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, generator=gen) * 0.3
    lines = []
    L = N.lib()
    rec = _Recorder(L.ff_mlp_ode_launch)

    def run(label, op, inputs):
        """One call of ``op(*inputs.values())``: a line per launch it made and one for what it returned or raised."""
        del rec.calls[:]
        try:
            out = op(*inputs.values())
        except Exception as e:                                  # the record of a faulty argument
            assert not rec.calls, "a faulty argument must raise before any launch"
            lines.append(f"{label} raises {type(e).__name__}: {e}")
            return
        torch.cuda.synchronize()
        outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        for call in rec.calls:
            lines.append(f"{label} launch " + _line(call, inputs, outs))
        lines.append(f"{label} returns " + "; ".join(f"{tuple(t.shape)} {t.dtype} {t.device}" for t in outs))

    # ---- networks, weights, tables ----------------------------------------------------------------------------------
    def single(D, C, hidden, mode):
        plan = N.make_plan(D, C, hidden, mode)
        sizes = [1 + D + C] + hidden + [D]                       # first layer: [time | x | cond]
        Ws = [rand(o, i) for i, o in zip(sizes[:-1], sizes[1:])]
        bs = [rand(o) for o in sizes[1:]]
        return plan, N.pack_weights(plan, Ws, bs, hidden, 1, 1 + D).to(dev)

    def pair(state, C, hidden, select):
        plan = N.make_pair_plan(state, C, hidden, select=select)
        sizes = [state // 2 + C + 2] + hidden + [state // 2]     # first layers: [half of the state | cond | time features]
        nets = [[torch.nn.Linear(i, o) for i, o in zip(sizes[:-1], sizes[1:])] for _ in range(2)]
        for net in nets:
            for l in net:
                l.weight.data, l.bias.data = rand(*l.weight.shape), rand(*l.bias.shape)
        return plan, N.pack_pair_weights(plan, nets[0], nets[1], hidden, 0, state // 2).to(dev)

    def table(plan, ev, real_width, noise=False):
        n = ev.t_eval.numel()
        if noise:
            ev.flags |= solvers.FLAG_NOISE
        return solvers.build_table(ev, torch.zeros(n), torch.ones(n), rand(n, real_width), N.row_width(plan),
                                   gn=torch.full((n,), 0.1) if noise else None,
                                   noise_idx=torch.arange(n) if noise else None).to(dev)

    def grid(method, rows):
        steps = rows // solvers.FIXED_METHODS[method].stages
        ev = solvers.plan_ode(torch.tensor([0.0, 1.0]), method, {"step_size": 1.0 / steps})
        assert ev.t_eval.numel() == rows
        return ev

    def attempt_table(plan, real_width, n_rows=2):
        """``n_rows`` evaluation rows into slots 1.., then the two auxiliary rows: aux_0 = y + slot 0, aux_1 = slot 1,
        aux_2 = y + slot 2 / 2, aux_3 = slot 1 - slot 2 (rows as `FusedNet.make_step` lays them out)."""
        ev = grid("euler", n_rows)
        ev.flags[:] = 0
        ev.slot[:] = torch.arange(1, n_rows + 1, dtype=torch.int32)
        rows = torch.cat([table(plan, ev, real_width).cpu(), torch.zeros(2, 32 + N.row_width(plan))])
        rows[n_rows, 8], rows[n_rows, 16 + 1] = 1.0, 1.0
        rows[n_rows + 1, 8 + 2], rows[n_rows + 1, 16 + 1], rows[n_rows + 1, 16 + 2] = 0.5, 1.0, -1.0
        rows.view(torch.int32)[n_rows, 3] = 0b0101
        return rows.to(dev)

    D, C, hidden = 3, 2, [32, 32]
    modes = {"state": N.MODE_STATE, "hutch": N.MODE_HUTCH, "exact": N.MODE_EXACT}
    nets = {m: single(D, C, hidden, code) for m, code in modes.items()}
    plan_nc, wpack_nc = single(D, 0, hidden, N.MODE_STATE)       # the same network without conditional inputs
    on = lambda *shape: rand(*shape).to(dev)
    L.ff_mlp_ode_launch = rec
    try:
        # ---- mlp_ode ------------------------------------------------------------------------------------------------
        def ode_inputs(m, B, plan=None, wpack=None, etab=None, words=None, **over):
            p, w = nets[m] if plan is None else (plan, wpack)
            inputs = {"x": on(B, p.dim), "cond": on(B, p.cond_dim) if p.cond_dim else None,
                      "probe": on(B, p.dim) if m == "hutch" else None, "noise": None, "wpack": w,
                      "etab": table(p, grid("euler", 2), 32) if etab is None else etab,
                      "in_shift": None, "in_scale": None, "out_scale": None, "out_shift": None,
                      "plan": N.plan_words(p) if words is None else words, "mode": modes.get(m, N.MODE_STATE),
                      "tangent_first": 0, "tangent_count": 0, "rng_seed": 0, "rng_sample_offset": 0, "rng_noise_base": 0}
            assert set(over) <= set(inputs)
            inputs.update(over)
            return inputs

        for m in modes:
            for B in (0, 5):
                run(f"mlp_ode {m} B={B}", ops.mlp_ode, ode_inputs(m, B))
        run("mlp_ode exact tangents 1..2", ops.mlp_ode, ode_inputs("exact", 5, tangent_first=1, tangent_count=2))
        run("mlp_ode state three rows", ops.mlp_ode, ode_inputs("state", 5, etab=table(nets["state"][0], grid("euler", 3), 32)))
        run("mlp_ode state no cond", ops.mlp_ode, ode_inputs("nc", 5, plan_nc, wpack_nc))
        run("mlp_ode state with probe", ops.mlp_ode, ode_inputs("state", 5, probe=on(5, D)))
        for name in ("in_shift", "in_scale", "out_scale", "out_shift"):
            run(f"mlp_ode state {name}", ops.mlp_ode, ode_inputs("state", 5, **{name: on(D).abs() + 0.5}))
        run("mlp_ode hutch every affine map", ops.mlp_ode, ode_inputs(
            "hutch", 5, **{k: on(D).abs() + 0.5 for k in ("in_shift", "in_scale", "out_scale", "out_shift")}))
        noisy = table(nets["state"][0], grid("euler", 2), 32, noise=True)
        run("mlp_ode state noise buffer", ops.mlp_ode, ode_inputs("state", 5, etab=noisy, noise=on(2, 5, D)))
        run("mlp_ode state noise in kernel", ops.mlp_ode, ode_inputs(
            "state", 5, etab=noisy, rng_seed=(1 << 62) + 12345, rng_sample_offset=(1 << 33) + 7, rng_noise_base=3))
        run("mlp_ode state negative seed", ops.mlp_ode, ode_inputs("state", 5, etab=noisy, rng_seed=-2))
        p_state = nets["state"][0]
        run("mlp_ode state plan without the slots word", ops.mlp_ode, ode_inputs("state", 5, words=N.plan_words(p_state)[:-1]))
        run("mlp_ode state plan with slots=1", ops.mlp_ode, ode_inputs("state", 5, words=N.plan_words(p_state, 1)))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run("mlp_ode state on a side stream", ops.mlp_ode, ode_inputs("state", 5))
        torch.cuda.current_stream().wait_stream(side)
        # the two-network plans: state 4, one conditional input, one hidden layer of 64
        pairs = {"pair": pair(4, 1, [64], False), "select": pair(4, 1, [64], True)}
        for B in (0, 5):
            run(f"mlp_ode pair B={B}", ops.mlp_ode, ode_inputs("pair", B, *pairs["pair"],
                                                                 etab=table(pairs["pair"][0], grid("midpoint", 2), 128)))
            leap = table(pairs["select"][0], solvers.plan_leapfrog(torch.tensor([0.0, 1.0])), 64)      # kick, drift, kick
            run(f"mlp_ode select B={B}", ops.mlp_ode, ode_inputs("select", B, *pairs["select"], etab=leap,
                                                                   words=N.plan_words(pairs["select"][0], 1)))

        # ---- mlp_ode_step -------------------------------------------------------------------------------------------
        def step_inputs(m, B, n_aux, plan=None, wpack=None, real_width=32, k1=True, kl1=False, dlogp0=False, words=None,
                        **over):
            p, w = nets[m] if plan is None else (plan, wpack)
            inputs = {"x": on(B, p.dim), "cond": on(B, p.cond_dim), "probe": on(B, p.dim) if m == "hutch" else None,
                      "k1": on(B, p.dim) if k1 else None, "kl1": on(B) if kl1 else None, "dlogp0": on(B) if dlogp0 else None,
                      "wpack": w, "etab": attempt_table(p, real_width), "plan": N.plan_words(p, 3) if words is None else words,
                      "mode": modes.get(m, N.MODE_STATE), "n_aux": n_aux, "tangent_first": 0, "tangent_count": 0}
            assert set(over) <= set(inputs)
            inputs.update(over)
            return inputs

        for m in modes:
            run(f"mlp_ode_step {m} B=0", ops.mlp_ode_step, step_inputs(m, 0, 4))
            for n_aux in (1, 2, 3, 4):
                run(f"mlp_ode_step {m} n_aux={n_aux}", ops.mlp_ode_step,
                    step_inputs(m, 5, n_aux, kl1=m != "state", dlogp0=m != "state"))
            run(f"mlp_ode_step {m} no k1", ops.mlp_ode_step, step_inputs(m, 5, 2, k1=False))
        for m in ("hutch", "exact"):
            run(f"mlp_ode_step {m} kl1 only", ops.mlp_ode_step, step_inputs(m, 5, 2, kl1=True))
            run(f"mlp_ode_step {m} dlogp0 only", ops.mlp_ode_step, step_inputs(m, 5, 2, dlogp0=True))
        run("mlp_ode_step exact tangents 1..2", ops.mlp_ode_step, step_inputs("exact", 5, 4, tangent_first=1, tangent_count=2))
        run("mlp_ode_step state plan without the slots word", ops.mlp_ode_step,
            step_inputs("state", 5, 4, words=N.plan_words(p_state)[:-1]))
        for n_aux in (1, 4):
            run(f"mlp_ode_step pair n_aux={n_aux}", ops.mlp_ode_step,
                step_inputs("pair", 5, n_aux, *pairs["pair"], real_width=128))
        run("mlp_ode_step pair B=0", ops.mlp_ode_step, step_inputs("pair", 0, 4, *pairs["pair"], real_width=128))

        # ---- the two Jacobian ops (fp32 single-network exact-mode plans) -------------------------------------------------
        p_exact, w_exact = nets["exact"]

        def rhs_jac_inputs(B, first, count, **over):
            etab = attempt_table(p_exact, 32, n_rows=1)
            etab[1:] = 0
            etab[1, 8] = 1.0                                     # auxiliary output 0 = stage slot 0 (`RowStepper.rhs_div`)
            etab.view(torch.int32)[0, 4] = 0
            inputs = {"x": on(B, D), "cond": on(B, C), "wpack": w_exact, "etab": etab, "plan": N.plan_words(p_exact),
                      "tangent_first": first, "tangent_count": count, "jac": torch.zeros(B, D, D, device=dev)}
            assert set(over) <= set(inputs)
            inputs.update(over)
            return inputs

        def jacobians_inputs(B, first, count, method="midpoint", rows=2, **over):
            inputs = {"x": on(B, D), "cond": on(B, C), "wpack": w_exact, "etab": table(p_exact, grid(method, rows), 32),
                      "plan": N.plan_words(p_exact), "tangent_first": first, "tangent_count": count,
                      "jac": torch.zeros(rows, B, D, D, device=dev)}
            assert set(over) <= set(inputs)
            inputs.update(over)
            return inputs

        for B, first, count in ((0, 0, 3), (5, 0, 3), (5, 0, 0), (5, 1, 2), (5, 2, 1)):
            run(f"mlp_rhs_jac B={B} tangents {first}+{count}", ops.mlp_rhs_jac, rhs_jac_inputs(B, first, count))
            run(f"mlp_ode_jacobians B={B} tangents {first}+{count}", ops.mlp_ode_jacobians, jacobians_inputs(B, first, count))
        run("mlp_ode_jacobians three rows", ops.mlp_ode_jacobians, jacobians_inputs(5, 0, 3, "euler", 3))

        # ---- one faulty argument at a time: raised in Python, nothing launched ------------------------------------------
        def strided(t):
            if t.dim() == 1:
                return torch.zeros(2 * t.numel(), device=t.device)[::2]
            return t.transpose(-1, -2).contiguous().transpose(-1, -2)

        def faults(op_name, op, inputs, shapes):
            """``inputs``: a valid call with every tensor present; ``shapes``: {label: replacement arguments}."""
            for name, t in inputs.items():
                if not torch.is_tensor(t):
                    continue
                for what, bad in (("on the CPU", t.cpu()), ("float64", t.double()), ("not contiguous", strided(t))):
                    if what == "not contiguous" and bad.is_contiguous():        # ([B, 1]: every stride order is contiguous)
                        continue
                    assert bad.shape == t.shape
                    run(f"{op_name} fault {name} {what}", op, {**inputs, name: bad})
            for label, over in shapes.items():
                assert set(over) <= set(inputs)
                run(f"{op_name} fault {label}", op, {**inputs, **over})

        wide = lambda etab: torch.cat([etab, torch.zeros(etab.shape[0], 1, device=dev)], dim=1).contiguous()
        full = ode_inputs("hutch", 5, etab=noisy, noise=on(2, 5, D),
                          **{k: on(D).abs() + 0.5 for k in ("in_shift", "in_scale", "out_scale", "out_shift")})
        faults("mlp_ode", ops.mlp_ode, full, {
            "x of 4 columns": {"x": on(5, 4)}, "cond of 3 columns": {"cond": on(5, 3)}, "cond of 4 rows": {"cond": on(4, C)},
            "probe of 4 columns": {"probe": on(5, 4)}, "probe of 4 rows": {"probe": on(4, D)},
            "table one word too wide": {"etab": wide(full["etab"])}})
        pair_ode = ode_inputs("pair", 5, *pairs["pair"], etab=table(pairs["pair"][0], grid("midpoint", 2), 128))
        faults("mlp_ode pair", ops.mlp_ode, pair_ode, {
            "table of a single network's width": {"etab": pair_ode["etab"][:, :32 + 64].contiguous()}})
        full = step_inputs("hutch", 5, 4, kl1=True, dlogp0=True)
        faults("mlp_ode_step", ops.mlp_ode_step, full, {
            "table one word too wide": {"etab": wide(full["etab"])}, "table of one row": {"etab": full["etab"][:1].contiguous()}})
        full = rhs_jac_inputs(5, 0, 3)
        faults("mlp_rhs_jac", ops.mlp_rhs_jac, full, {
            "jac [B, D, D + 1]": {"jac": torch.zeros(5, D, D + 1, device=dev)},
            "jac [B + 1, D, D]": {"jac": torch.zeros(6, D, D, device=dev)},
            "table of four rows": {"etab": torch.cat([full["etab"], full["etab"][:1]]).contiguous()},
            "table one word too wide": {"etab": wide(full["etab"])}})
        full = jacobians_inputs(5, 0, 3)
        faults("mlp_ode_jacobians", ops.mlp_ode_jacobians, full, {
            "jac of three rows": {"jac": torch.zeros(3, 5, D, D, device=dev)},
            "jac [n, B, D, D + 1]": {"jac": torch.zeros(2, 5, D, D + 1, device=dev)},
            "table one word too wide": {"etab": wide(full["etab"])}})
    finally:
        L.ff_mlp_ode_launch = rec.real
    return "\n".join(lines) + "\n"


@pytest.mark.gpu
def test_ops_fill_the_recorded_arguments(built_library):
    got, want = record().splitlines(), EXPECTED.read_text().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            diff = [f"{a} (recorded: {b})" for a, b in zip(g.split(" "), w.split(" ")) if a != b]
            assert g == w, f"line {i + 1} of the record, {w.split(' launch ')[0]!r}: {diff[:8]}"
    assert len(got) == len(want)


if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "--write", __doc__
    tree = Path(sys.argv[2]).resolve()
    os.environ["FLOWFUSION_AMD_LIB"] = str(ROOT / "flowfusion_amd" / "lib" / "libflowfusion_amd.so")
    sys.path.insert(0, str(tree))                  # that tree's Python package on this tree's built library
    import flowfusion_amd
    assert Path(flowfusion_amd.__file__).resolve().parents[1] == tree
    out = Path(sys.argv[3]) if len(sys.argv) == 4 else EXPECTED
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(record())
