"""Hutch++ / XTrace log-densities by the two routes, products="jacobian" against products="vjp": the timing table of
profiles/estimator_products.txt.

    python scratch/estimator_products_bench.py [--parent DIR] [--rows 65536] [--steps 100] [--repeats 5]

Workloads: rk4 with ``--steps`` steps over ``--rows`` rows, VP score models of 16 dimensions and of 32 dimensions, 4 x 256.
Per estimator (Hutch++ r = m = 1 and r = m = 4, XTrace m = 2): both routes as whole ``log_prob`` calls, then the pieces of the
products route on one chunk -- sweep 1, ff_trace_basis, sweep 2, ff_trace_combine.  For scale: the exact-trace and the
Hutchinson ``log_prob`` of the same model.  ``--parent DIR``: a checkout of the parent commit with its library built; its
``log_prob`` (the recorded-Jacobian route, the only one it has) is timed in a child process in the same run, and every ratio
is taken against it.  Times: median of ``--repeats`` after two warm-up calls, device-synchronised wall clock.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
ESTIMATORS = [("hutchpp r=m=1", dict(hutchpp=True, hpp_rank=1, hpp_vecs=1)), ("hutchpp r=m=4", dict(hutchpp=True, hpp_rank=4, hpp_vecs=4)),
              ("xtrace m=2", dict(xtrace=True, xt_vecs=2))]


def timed(fn, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def model(Dm, D, **kw):
    torch.manual_seed(1)
    m = Dm.MLP(n_dimensions=D, n_conditionals=0, embedding_dimensions=8, units=[256] * 4)
    return Dm.ScoreModel(m, Dm.VPSDE(), **kw).to("cuda").eval()


def whole_calls(D, rows, steps, repeats, routes):
    """{label: (median, min, max) ms} of log_prob on this interpreter's flowfusion_amd."""
    from flowfusion_amd import diffusion as Dm
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(2)).to("cuda")
    kw = dict(method="rk4", options={"step_size": (1.0 - 1e-5) / steps})
    out = {}
    for label, mk in ESTIMATORS:
        sm = model(Dm, D, **mk)
        for route in routes:
            extra = {} if route is None else {"products": route}
            out[f"{label} {route or 'parent'}"] = timed(lambda: sm.log_prob(x, **kw, **extra), repeats)
    if None not in routes:
        out["exact trace"] = timed(lambda sm=model(Dm, D): sm.log_prob(x, **kw), repeats)
        out["hutchinson"] = timed(lambda sm=model(Dm, D, hutchinson=True): sm.log_prob(x, **kw), repeats)
    return out


def pieces(D, rows, steps, repeats):
    """The four launches of the products route on one chunk of ``rows`` samples (cut to fit 8 GiB of seeds and products)."""
    from flowfusion_amd import _native, solvers
    from flowfusion_amd import diffusion as Dm
    out = {}
    for label, mk in ESTIMATORS:
        sm = model(Dm, D, **mk)
        net = sm._net()
        span = torch.tensor([float(sm.sde.epsilon), 1.0])
        opts = {"step_size": (1.0 - 1e-5) / steps}
        grid = solvers.plan_ode(span, "rk4", opts)
        table = solvers.build_table(grid, *sm._host_schedule()(grid.t_eval), int(net.pull_plan().width)).to("cuda")
        n = table.shape[0]
        (r, m), mx = sm._probe_counts(D)
        kind, K1, K2 = ("hutchpp", r, r + m) if sm.hutchpp else ("xtrace", mx, mx)
        b = min(rows, (8 << 30) // (n * (K1 + 2 * K2) * D * 4))
        g = torch.Generator().manual_seed(3)
        x = torch.randn(b, D, generator=g).to("cuda")
        sign = lambda k: (torch.randint(0, 2, (k, b, D), generator=g).float() * 2 - 1).to("cuda")
        probes = (sign(r), sign(m)) if sm.hutchpp else (sign(mx),)
        seeds1 = probes[0].permute(1, 0, 2).contiguous()
        sweep = lambda s, per_row: net.vjp_products(x, table, s, per_row=per_row, stage_slots=4)
        _, Y, _ = sweep(seeds1, False)
        basis, rfac = _native.trace_basis(Y, kind, probes)
        _, Z, _ = sweep(basis, True)
        scale = rows / b
        for what, fn in (("sweep 1", lambda: sweep(seeds1, False)), ("basis", lambda: _native.trace_basis(Y, kind, probes)),
                         ("sweep 2", lambda: sweep(basis, True)), ("combine", lambda: _native.trace_combine(basis, rfac, Z, kind, probes))):
            med, lo, hi = timed(fn, repeats)
            out[f"{label} {what}"] = (med * scale, lo * scale, hi * scale, b)
        del Y, Z, basis, rfac
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dims", default="16,32")
    ap.add_argument("--child", default=None, help="(internal) time the parent's calls at this dimension, print JSON")
    a = ap.parse_args()
    if a.child is None:
        sys.path.insert(0, str(ROOT))               # (the child imports the parent's package through PYTHONPATH)
    if a.child is not None:
        print("JSON " + json.dumps(whole_calls(int(a.child), a.rows, a.steps, a.repeats, [None])))
        return
    print(f"# rk4, {a.steps} steps, {a.rows} rows, VP, 4 x 256; median [min, max] ms of {a.repeats} after 2 warm-ups; device: "
          f"{torch.cuda.get_device_name(0)}")
    for D in (int(d) for d in a.dims.split(",")):
        print(f"\n## {D} dimensions")
        parent = {}
        if a.parent:
            env = dict(os.environ, PYTHONPATH=str(Path(a.parent).resolve()))
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(D), "--rows", str(a.rows), "--steps",
                                str(a.steps), "--repeats", str(a.repeats)], env=env, cwd=a.parent, capture_output=True, text=True,
                               timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            parent = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("JSON "))[5:])
        own = whole_calls(D, a.rows, a.steps, a.repeats, ["jacobian", "vjp"])
        for label, _ in ESTIMATORS:
            base = parent.get(f"{label} parent")
            if base:
                print(f"{label:16s} parent commit       {base[0]:9.1f} [{base[1]:.1f}, {base[2]:.1f}]")
            for route in ("jacobian", "vjp"):
                med, lo, hi = own[f"{label} {route}"]
                ratio = f"   {med / base[0]:.2f}x the parent's call" if base else ""
                print(f"{label:16s} products={route:9s} {med:9.1f} [{lo:.1f}, {hi:.1f}]{ratio}")
        for what in ("exact trace", "hutchinson"):
            med, lo, hi = own[what]
            print(f"{what:36s} {med:9.1f} [{lo:.1f}, {hi:.1f}]")
        print(f"# the products route's launches, one chunk scaled to {a.rows} rows")
        for key, (med, lo, hi, b) in pieces(D, a.rows, a.steps, a.repeats).items():
            print(f"{key:36s} {med:9.1f} [{lo:.1f}, {hi:.1f}]   (chunk of {b} rows)")


if __name__ == "__main__":
    main()
