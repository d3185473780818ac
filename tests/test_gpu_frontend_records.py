"""What the Python front ends hand to the kernel, recorded on the GPU and compared with a committed record.

tests/test_gpu_op_records.py pins which ff_ode_args the custom ops fill for their arguments; this file pins the layer above
them: which `FusedNet.integrate` calls the public methods of diffusion.py, flow.py and distributed.py make (through
odeint.py).  `FusedNet.integrate` is wrapped by a recorder that notes the call and passes it through: every recorded call is
a real launch.  A line holds `mode`, `stage_slots`, `per_probe`, the plan's kernel, the shapes of `x`, `cond` and `probe`
(`None` where absent), and the SHA-256 of the bytes of the evaluation table, the probe, the conditional and the four affine
vectors; after the public call one line holds the shapes and dtypes of what it returned and of `model.e` /
`model.dlogp_probes` (removed before every call, so the line shows what that call set).  A refusal is recorded as the
exception's type and text and must come before any `integrate` call.  No kernel output is hashed: the record does not
depend on the kernels' rounding.  (The evaluation tables are computed by torch on the host.  The flows' tables
hashed alike on every host tried; the score models' -- exp, sin, cos and a sum over the time features -- differed in the last
bits between a host with another CPU and the GPU machines, so the record belongs to the class of machine the GPU tier runs on.)

The sweep: state dimension 3, conditional width 2, hidden [32, 32], batch 5, rk4 with two steps, on seeded models -- a VP
`ScoreModel` (Hutchinson and exact), the two population wrappers, an `ODEFlow` and a `ConditionalODEFlow` with
non-trivial shift and scale; Hutchinson solves with K in {1, 3} from torch's generator and the counter-based stream, with the
standard error and with the rows cut (`odeint.PROBE_BUFFER_FLOATS = 2 K D + 1`: pieces of 2, 2 and 1 rows).

tests/op_records/frontend_expected.txt is the record of the commit BEFORE the front ends were folded onto one Hutchinson
path, never of the code under test: its Python package, this tree's built library, in a fresh process:
    python tests/test_gpu_frontend_records.py --write <tree with that commit's flowfusion_amd/> [<file>]
`--compare <tree>` runs the sweep in two fresh child processes (that tree's package, then this one's; each under its own
time limit, the second only if the first succeeded) and compares every returned tensor, `model.e` and
`model.dlogp_probes` byte for byte; it prints the count compared and exits non-zero on any difference.
"""
import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
EXPECTED = ROOT / "tests" / "op_records" / "frontend_expected.txt"

D, C, HIDDEN, B = 3, 2, [32, 32], 5


def _sha(t):
    if t is None:
        return "None"
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def _shape(t):
    return "None" if t is None else str(tuple(t.shape)).replace(" ", "")


def _describe(obj):
    """Shapes and dtypes of a returned value: tensors inside tuples / lists, anything else by its repr."""
    if torch.is_tensor(obj):
        return f"{_shape(obj)}:{obj.dtype}"
    if isinstance(obj, (tuple, list)):
        inner = ",".join(_describe(o) for o in obj)
        return f"({inner})" if isinstance(obj, tuple) else f"[{inner}]"
    return repr(obj)


def _tensors(obj):
    if torch.is_tensor(obj):
        return [obj.detach().cpu()]
    if isinstance(obj, (tuple, list)):
        return [t for o in obj for t in _tensors(o)]
    return []


def sweep():
    """The sweep (module docstring) on the current GPU; returns (the record's text, {label: tensors returned and kept})."""
    from flowfusion_amd import _native, distributed, odeint
    from flowfusion_amd.diffusion import MLP, VPSDE, PopulationModelDiffusion, PopulationModelDiffusionConditional, ScoreModel
    from flowfusion_amd.flow import ConditionalODEFlow, ODEFlow
    from flowfusion_amd.fused import FusedNet, MODE_STATE

    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, generator=gen) * 0.3
    lines, kept, calls = [], {}, []
    real = FusedNet.integrate

    def recording(net, x, etab, mode=MODE_STATE, cond=None, probe=None, noise=None, in_shift=None, in_scale=None,
                  out_scale=None, out_shift=None, rng=None, stage_slots=0, plan=None, per_probe=False):
        kernel = _native.kernel_name(net.plan(mode) if plan is None else plan)
        words = [f"mode={mode}", f"stage_slots={stage_slots}", f"per_probe={per_probe}", f"kernel={kernel}",
                 f"x={_shape(x)}", f"cond={_shape(cond)}", f"probe={_shape(probe)}", f"noise={_shape(noise)}", f"rng={rng}"]
        words += [f"{name}#{_sha(t)}" for name, t in (("etab", etab), ("probe", probe), ("cond", cond), ("in_shift", in_shift),
                                                       ("in_scale", in_scale), ("out_scale", out_scale), ("out_shift", out_shift))]
        calls.append(" ".join(words))
        return real(net, x, etab, mode, cond=cond, probe=probe, noise=noise, in_shift=in_shift, in_scale=in_scale,
                    out_scale=out_scale, out_shift=out_shift, rng=rng, stage_slots=stage_slots, plan=plan, per_probe=per_probe)

    def run(label, model, fn, seed=None):
        """One public call: a line per ``integrate`` call it made, then one for what it returned (or raised) and kept."""
        del calls[:]
        for name in ("e", "dlogp_probes"):
            model.__dict__.pop(name, None)
        if seed is not None:
            torch.manual_seed(seed)
        try:
            out = fn()
        except Exception as e:                                  # the record of a refusal
            assert not calls, f"{label}: a refusal must come before any launch"
            lines.append(f"{label} raises {type(e).__name__}: {e}")
            return
        torch.cuda.synchronize()
        lines.extend(f"{label} integrate {c}" for c in calls)
        e, d = getattr(model, "e", None), getattr(model, "dlogp_probes", None)
        lines.append(f"{label} returns {_describe(out)} e={_describe(e)} dlogp_probes={_describe(d)}")
        kept[label] = _tensors(out) + _tensors(e) + _tensors(d)

    def seeded(module):
        for p in module.parameters():
            p.data = rand(*p.shape)
        return module.to(dev).eval()

    # ---- models and inputs ------------------------------------------------------------------------------------------
    on = lambda *shape: rand(*shape).to(dev)
    stats = lambda n: (rand(n), rand(n).abs() + 0.5)             # (shift, scale) of n columns
    mlp_c, mlp_u = seeded(MLP(D, C, 8, HIDDEN)), seeded(MLP(D, 0, 8, HIDDEN))
    sm_h = ScoreModel(mlp_c, VPSDE(), hutchinson=True).to(dev)
    sm_x = ScoreModel(mlp_c, VPSDE()).to(dev)
    opts = {"step_size": (1.0 - 1e-3) / 2}
    rk4 = dict(method="rk4", options=opts)
    pm_u = PopulationModelDiffusion(mlp_u, VPSDE(), *stats(D), **rk4).to(dev)
    pm_c = PopulationModelDiffusionConditional(mlp_c, VPSDE(), *stats(D), *stats(C), **rk4).to(dev)
    pm_64 = PopulationModelDiffusion(mlp_u, VPSDE(), *(s.double() for s in stats(D)), **rk4).to(dev)
    flow_u = seeded(ODEFlow(D, HIDDEN, torch.nn.SiLU, *stats(D)))
    flow_c = seeded(ConditionalODEFlow(D, C, HIDDEN, torch.nn.SiLU, *stats(D), *stats(C)))
    frk4 = dict(method="rk4", options={"step_size": 0.5})
    x, z, c = on(B, D), on(B, D), on(B, C)
    probes = {"torch": (dict(), 0), "philox": (dict(probe="philox", seed=7, sample_offset=2 ** 33 + 1), None)}
    flows = (("flow", flow_u, ()), ("cflow", flow_c, (c,)))

    def cut(K, fn):
        """``fn()`` with the rows of a K-probe solve cut into pieces of 2, 2 and 1."""
        def call():
            whole = odeint.PROBE_BUFFER_FLOATS
            odeint.PROBE_BUFFER_FLOATS = 2 * K * D + 1
            try:
                return fn()
            finally:
                odeint.PROBE_BUFFER_FLOATS = whole
        return call

    FusedNet.integrate = recording
    try:
        # ---- score model, Hutchinson ------------------------------------------------------------------------------------
        for pname, (pkw, seed) in probes.items():
            for K in (1, 3):
                kw = dict(conditional=c, num_probes=K, **rk4, **pkw)
                run(f"score log_prob K={K} {pname}", sm_h, lambda: sm_h.log_prob(x, **kw), seed)
                run(f"score solve_odes_forward K={K} {pname}", sm_h, lambda: sm_h.solve_odes_forward(x, **kw), seed)
            kw = dict(conditional=c, num_probes=3, **rk4, **pkw)
            run(f"score log_prob K=3 stderr {pname}", sm_h, lambda: sm_h.log_prob(x, return_stderr=True, **kw), seed)
            run(f"score solve_odes_forward K=3 stderr {pname}", sm_h,
                lambda: sm_h.solve_odes_forward(x, return_stderr=True, **kw), seed)
            for se in (False, True):
                run(f"score log_prob K=3 cut stderr={se} {pname}", sm_h,
                    cut(3, lambda: sm_h.log_prob(x, return_stderr=se, **kw)), seed)
        # ---- score model, exact trace; sampling -----------------------------------------------------------------------------
        run("score log_prob exact", sm_x, lambda: sm_x.log_prob(x, conditional=c, **rk4))
        run("score sample_ode_from_base", sm_x, lambda: sm_x.sample_ode_from_base(z, conditional=c, **rk4))
        run("population forward", pm_u.score_model, lambda: pm_u(z))
        run("population conditional forward", pm_c.score_model, lambda: pm_c(z, c))
        run("population forward float64 statistics", pm_64.score_model, lambda: pm_64(z))
        # ---- the flows ------------------------------------------------------------------------------------------------------
        for name, flow, cargs in flows:
            run(f"{name} sample", flow, lambda: flow.sample(z, *cargs, **frk4))
            run(f"{name} log_prob exact", flow, lambda: flow.log_prob(x, *cargs, **frk4))
            for pname, (pkw, seed) in probes.items():
                for K in (1, 3):
                    kw = dict(hutchinson=True, num_probes=K, **frk4, **pkw)
                    run(f"{name} log_prob K={K} {pname}", flow, lambda: flow.log_prob(x, *cargs, **kw), seed)
                    run(f"{name} solve_ode_forward K={K} {pname}", flow, lambda: flow.solve_ode_forward(x, *cargs, **kw), seed)
                kw = dict(hutchinson=True, num_probes=3, **frk4, **pkw)
                run(f"{name} log_prob K=3 stderr {pname}", flow, lambda: flow.log_prob(x, *cargs, return_stderr=True, **kw), seed)
                for se in (False, True):
                    run(f"{name} log_prob K=3 cut stderr={se} {pname}", flow,
                        cut(3, lambda: flow.log_prob(x, *cargs, return_stderr=se, **kw)), seed)
        # ---- sharded entry points without a process group (one rank owns every row) -------------------------------------------
        for gather in (True, False):
            for se in (False, True):
                kw = dict(seed=7, gather=gather, return_stderr=se, num_probes=3)
                run(f"log_prob_sharded gather={gather} stderr={se}", sm_h,
                    lambda: distributed.log_prob_sharded(sm_h, x, c, **kw, **rk4))
                for name, flow, cargs in flows:
                    run(f"flow_log_prob_sharded {name} gather={gather} stderr={se}", flow,
                        lambda: distributed.flow_log_prob_sharded(flow, x, *cargs, hutchinson=True, **kw, **frk4))
        run("log_prob_sharded exact", sm_x, lambda: distributed.log_prob_sharded(sm_x, x, c, seed=7, **rk4))
        run("sample_ode_sharded", sm_x, lambda: distributed.sample_ode_sharded(sm_x, B, D, seed=7, conditional=c, **rk4))
        for name, flow, cargs in flows:
            run(f"flow_sample_sharded {name}", flow, lambda: distributed.flow_sample_sharded(flow, B, 7, *cargs, **frk4))
        # ---- refusals: raised before anything is launched ---------------------------------------------------------------------
        run("score refuses stderr with K=1", sm_h, lambda: sm_h.log_prob(x, conditional=c, return_stderr=True, **rk4))
        run("score refuses stderr with dopri5", sm_h, lambda: sm_h.log_prob(x, conditional=c, num_probes=3, return_stderr=True))
        run("score refuses num_probes=2 on an exact model", sm_x, lambda: sm_x.log_prob(x, conditional=c, num_probes=2, **rk4))
        run("score refuses seed= with probe='torch'", sm_h, lambda: sm_h.log_prob(x, conditional=c, seed=7, **rk4))
        run("cflow refuses stderr with K=1", flow_c, lambda: flow_c.log_prob(x, c, hutchinson=True, return_stderr=True, **frk4))
        run("cflow refuses stderr with dopri5", flow_c,
            lambda: flow_c.log_prob(x, c, hutchinson=True, num_probes=3, return_stderr=True))
        run("cflow refuses num_probes=2 on the exact trace", flow_c, lambda: flow_c.log_prob(x, c, num_probes=2, **frk4))
        run("cflow refuses seed= with probe='torch'", flow_c, lambda: flow_c.log_prob(x, c, hutchinson=True, seed=7, **frk4))
    finally:
        FusedNet.integrate = real
    return "\n".join(lines) + "\n", kept


@pytest.mark.gpu
def test_front_ends_hand_the_recorded_calls_to_the_kernel(built_library):
    got, want = sweep()[0].splitlines(), EXPECTED.read_text().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            diff = [f"{a} (recorded: {b})" for a, b in zip(g.split(" "), w.split(" ")) if a != b]
            assert g == w, f"line {i + 1} of the record, {w.split(' integrate ')[0]!r}: {diff[:8]}"
    assert len(got) == len(want)


def _use_tree(tree):
    """That tree's Python package on this tree's built library (before the first import of the package)."""
    os.environ["FLOWFUSION_AMD_LIB"] = str(ROOT / "flowfusion_amd" / "lib" / "libflowfusion_amd.so")
    sys.path.insert(0, str(tree))
    import flowfusion_amd
    assert Path(flowfusion_amd.__file__).resolve().parents[1] == tree


def _compare(tree, limit=300):
    with tempfile.TemporaryDirectory() as tmp:
        dumps = [Path(tmp) / "theirs.pt", Path(tmp) / "ours.pt"]
        for t, dump in zip((tree, ROOT), dumps):
            done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--dump", str(t), str(dump)])
            if done.returncode != 0:                # nothing more is started after a failure
                sys.exit(f"the sweep on {t} ended with status {done.returncode}")
        theirs, ours = (torch.load(d) for d in dumps)
    assert list(theirs) == list(ours), "the two sweeps made different calls"
    n = bad = 0
    for label in theirs:
        assert len(theirs[label]) == len(ours[label]), label
        for a, b in zip(theirs[label], ours[label]):
            n += 1
            if a.dtype != b.dtype or a.shape != b.shape or a.numpy().tobytes() != b.numpy().tobytes():
                bad += 1
                print(f"DIFFERENT: {label} {tuple(a.shape)} {a.dtype}")
    print(f"compared {n} tensors of {len(theirs)} calls byte for byte: {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] in ("--write", "--dump", "--compare"), __doc__
    tree = Path(sys.argv[2]).resolve()
    if sys.argv[1] == "--compare":
        _compare(tree)
    _use_tree(tree)
    text, kept = sweep()
    if sys.argv[1] == "--dump":
        torch.save(kept, sys.argv[3])
    else:
        out = Path(sys.argv[3]) if len(sys.argv) == 4 else EXPECTED
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(text)
