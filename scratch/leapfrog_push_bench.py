"""The timings of profiles/leapfrog_push.txt: the leapfrog push-forwards on an MI355X.  Needs the GPU and the built library.

    python scratch/leapfrog_push_bench.py [--rows 65536] [--steps 100]

Model A: D = 16 (joint 32), C = 0, 3 x 256, ``num_steps`` leapfrog steps (2 steps + 1 rows).
  1. the push-select launch (``FusedPair.pushforward_select``) at K = 1 / 3 / 7 / 15 against the ``integrate_select`` launch of
     the same rows, the two alternated window by window;
  2. the whole Jacobian by ``sample_leapfrog_jacobian`` against D cotangents through ``sample_leapfrog_vjp``, alternated; the
     same on model C (D = 16, C = 4: the hyper-parameter columns ride along);
  3. ``torch.func.jvp`` on the device at 2^12 rows, K = 1: time and agreement.
Times: device events around ``reps`` calls after a warm-up, the median of ``trials`` such windows; (min, max) is the spread.
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from flowfusion_amd import _native, solvers                      # noqa: E402
from flowfusion_amd import symplectic as Sm                     # noqa: E402

DEV = "cuda"


def alternated(fns, reps, trials=5):
    """[(median, min, max)] of the mean milliseconds of ``reps`` calls of each function: in every one of the ``trials`` rounds
    each function gets one window, in turn, so that a drift of the machine falls on all of them alike."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(trials):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[i].append(a.elapsed_time(b) / reps)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def fmt(t):
    return f"{t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})"


def symplectic(D, C, units, seed=5):
    torch.manual_seed(seed)
    mlp = Sm.SymplecticMLP(D, C, 4, units)
    cs = (torch.zeros(C), torch.ones(C)) if C else (None, None)
    return Sm.SymplecticFlowModel(mlp, torch.zeros(D), torch.ones(D), *cs).eval().to(DEV)


def torch_jvp(front, z, v, n):
    """``_sample_from(.., method="leapfrog")`` and one tangent by torch.func.jvp on the device: the rows of plan_leapfrog, fp32."""
    m = front.model
    rows = solvers.plan_leapfrog(torch.linspace(1.0, 0.0, n + 1))
    w = (rows.sign * rows.cout[:, 0]).tolist()
    nb = ((rows.flags & solvers.FLAG_NET_B) != 0).tolist()
    ts = rows.t_eval.to(DEV)
    D = z.shape[1] // 2

    def f(zz):
        q, p = zz[:, :D], zz[:, D:]
        for i in range(len(w)):
            arg = ts[i].expand(zz.shape[0])[:, None] * m.W[None, :] * 2 * math.pi
            emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
            if nb[i]:
                p = p - w[i] * m.mlp_p_dynamics(torch.cat([q, emb], dim=1))
            else:
                q = q + w[i] * m.mlp_q_dynamics(torch.cat([p, emb], dim=1))
        return q
    with torch.no_grad():
        return torch.func.jvp(f, (z,), (v,))


def jacobian_routes(front, z, cond, n, reps, label):
    D = z.shape[1] // 2
    eye = torch.eye(D, device=DEV)[None].expand(z.shape[0], D, D)

    def by_vjp():
        outs = [front.sample_leapfrog_vjp(z, eye[:, k0:k0 + 15].contiguous(), cond, num_steps=n) for k0 in range(0, D, 15)]
        return torch.cat([o[1] for o in outs], dim=1), (None if cond is None else torch.cat([o[2] for o in outs], dim=1))
    fwd, rev = alternated([lambda: front.sample_leapfrog_jacobian(z, cond, num_steps=n), by_vjp], reps, trials=3)
    _, Jz, Jc = front.sample_leapfrog_jacobian(z, cond, num_steps=n)
    Gz, Gc = by_vjp()
    rel = lambda a, b: float(((a - b).abs().amax(dim=(1, 2)) / b.abs().amax(dim=(1, 2))).max())
    C = 0 if cond is None else cond.shape[1]
    print(f"\n# the whole Jacobian dx/d(z, c), {label}: {2 * D + C} unit tangents in {-(-(2 * D + C) // 15)} push launches against "
          f"{D} cotangents in {-(-D // 15)} x (forward + pull) launches")
    print(f"sample_leapfrog_jacobian             {fmt(fwd)}")
    print(f"D cotangents, sample_leapfrog_vjp    {fmt(rev)}    vjp route / jacobian route {rev[0] / fwd[0]:.2f}")
    print(f"agreement of the two: J_z {rel(Jz, Gz):.3e}" + ("" if Jc is None else f", J_c {rel(Jc, Gc):.3e}") +
          " (max over rows of max |diff| / max |J|)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B, n = a.rows, a.steps
    print(f"# device: {torch.cuda.get_device_name(0)}; rows {B}, num_steps {n} ({2 * n + 1} table rows)")
    g = torch.Generator().manual_seed(0)

    # ---- 1. the launch ------------------------------------------------------------------------------------------------------------
    A = symplectic(16, 0, [256] * 3)
    net = A._net()
    plan = net.push_select_plan()
    z = torch.randn(B, 32, generator=g).to(DEV)
    grid = torch.linspace(1.0, 0.0, n + 1)
    sel_table = A._leapfrog_table(grid).to(DEV)
    table = A._leapfrog_table(grid, push_select=True).to(DEV)
    print(f"\n# model A: D = 16 (joint 32), C = 0, 3 x 256; units {_native.kernel_name(net.plan(_native.MODE_STATE, select=True))} "
          f"(integrate_select), {_native.kernel_name(plan)} (push-select)")
    base = None
    for K in (1, 3, 7, 15):
        v = torch.randn(B, K, 32, generator=g).to(DEV)
        sel, push = alternated([lambda: net.integrate_select(z, sel_table), lambda: net.pushforward_select(z, table, v)], a.reps)
        base = push[0] if base is None else base
        print(f"K = {K:2d}: integrate_select {fmt(sel)}   push-select {fmt(push)}   x integrate_select {push[0] / sel[0]:.2f}, "
              f"x K = 1 {push[0] / base:.2f}; {16 // (1 + K)} samples per tile")
        del v

    # ---- 2. the Jacobian routes ---------------------------------------------------------------------------------------------------
    jacobian_routes(A, z, None, n, 1, "model A")
    Cm = symplectic(16, 4, [256] * 3)
    cond = torch.randn(B, 4, generator=g).to(DEV)
    jacobian_routes(Cm, z, cond, n, 1, "model C (D = 16, C = 4, 3 x 256)")
    del Cm, cond

    # ---- 3. torch.func.jvp on the device, 2^12 rows -------------------------------------------------------------------------------
    Bs = min(B, 1 << 12)
    zs = z[:Bs].contiguous()
    vs = torch.randn(Bs, 1, 32, generator=g).to(DEV)
    tt, tk = alternated([lambda: torch_jvp(A, zs, vs[:, 0], n), lambda: A.sample_leapfrog_jvp(zs, vs, num_steps=n)], 1, trials=3)
    x_t, dx_t = torch_jvp(A, zs, vs[:, 0], n)
    x_k, dx_k = A.sample_leapfrog_jvp(zs, vs, num_steps=n)
    rel = lambda got, ref: float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    print(f"\n# torch.func.jvp on the device, model A, {Bs} rows, K = 1 (fp32)")
    print(f"torch.func.jvp                       {fmt(tt)}")
    print(f"sample_leapfrog_jvp                  {fmt(tk)}    torch / kernel {tt[0] / tk[0]:.1f}")
    print(f"agreement: dx max over rows of max |diff| / max |dx| = {rel(dx_k[:, 0], dx_t):.3e}; x {rel(x_k, x_t):.3e}")


if __name__ == "__main__":
    main()
