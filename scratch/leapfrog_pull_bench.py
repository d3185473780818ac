"""The timings of profiles/leapfrog_pull.txt: the leapfrog pull-backs on an MI355X.  Needs the GPU and the built library.

    python scratch/leapfrog_pull_bench.py [--rows 65536] [--steps 100]

Model A: D = 16 (joint 32), C = 0, 3 x 256, ``num_steps`` leapfrog steps (2 steps + 1 rows).
  * whole ``log_prob_leapfrog_grad`` against ``log_prob_leapfrog`` on the same momenta;
  * the backward launch alone (``FusedPair.pullback_select``) at K = 1 / 3 / 7 / 15, beside the forward launch;
  * torch autograd on the device at 2^12 rows: time and agreement.
Model B: D = 8 (joint 16), C = 0, 3 x 256, the same rows: the one pull-select launch against the record plus discrete-adjoint
  pair of the single-network family on a conventional 16-d network of the same widths and as many rows (Euler).
Times: device events around ``reps`` calls after a warm-up, the median of ``trials`` such windows.
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from flowfusion_amd import _native, odeint, solvers            # noqa: E402
from flowfusion_amd import flow as Fm                           # noqa: E402
from flowfusion_amd import symplectic as Sm                     # noqa: E402

DEV = "cuda"


def timed(fn, reps, trials=5):
    """Median over ``trials`` windows of the mean milliseconds of ``reps`` calls; the spread (min, max) beside it."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})"


def symplectic(D, units, seed=5):
    torch.manual_seed(seed)
    mlp = Sm.SymplecticMLP(D, 0, 4, units)
    return Sm.SymplecticFlowModel(mlp, torch.zeros(D), torch.ones(D), None, None).eval().to(DEV)


def lds_bytes(plan, K, slots=1):
    return slots * (plan.dregs + plan.cregs) * 256 + (plan.tile // (1 + K)) * plan.n_hidden * plan.width * 4


def torch_autograd(front, x, p0, n):
    """log_prob_leapfrog and its gradient by torch on the device: the rows of plan_leapfrog, states kept, fp32."""
    m = front.model
    rows = solvers.plan_leapfrog(torch.linspace(1.0, 0.0, n + 1).flip(0))
    w = (rows.sign * rows.cout[:, 0]).tolist()
    nb = ((rows.flags & solvers.FLAG_NET_B) != 0).tolist()
    x = x.clone().requires_grad_(True)
    D = x.shape[1]
    q, p = x, p0
    for i in range(len(w)):
        t = rows.t_eval[i].to(DEV).expand(x.shape[0])
        arg = t[:, None] * m.W[None, :] * 2 * math.pi
        emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
        if nb[i]:
            p = p - w[i] * m.mlp_p_dynamics(torch.cat([q, emb], dim=1))
        else:
            q = q + w[i] * m.mlp_q_dynamics(torch.cat([p, emb], dim=1))
    z1 = torch.cat([q, p], dim=1)
    lp = (-0.5 * z1 ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1) - (-0.5 * p0 ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
    g, = torch.autograd.grad(lp.sum(), x)
    return lp.detach(), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B, n = a.rows, a.steps
    print(f"# device: {torch.cuda.get_device_name(0)}; rows {B}, num_steps {n} ({2 * n + 1} table rows)")
    g = torch.Generator().manual_seed(0)

    # ---- model A ----------------------------------------------------------------------------------------------------------------
    A = symplectic(16, [256] * 3)
    net = A._net()
    plan = net.pull_select_plan()
    x = torch.randn(B, 16, generator=g).to(DEV)
    p0 = torch.randn(B, 16, generator=g).to(DEV)
    print(f"\n# model A: D = 16 (joint 32), C = 0, 3 x 256; units {_native.kernel_name(net.plan(_native.MODE_STATE, select=True))} "
          f"(forward), {_native.kernel_name(plan)} (backward)")
    fwd = timed(lambda: A._log_prob_from(x, p0, None, method="leapfrog", num_steps=n), a.reps)
    grad = timed(lambda: A.log_prob_leapfrog_grad(x, None, n, momentum=p0), a.reps)
    print(f"log_prob_leapfrog (same momenta)     {fmt(fwd)}")
    print(f"log_prob_leapfrog_grad               {fmt(grad)}    ratio {grad[0] / fwd[0]:.2f}")
    print(f"LDS per tile of the backward launch at K = 1, one stage slot: {lds_bytes(plan, 1)} bytes "
          f"({160 * 1024 // lds_bytes(plan, 1)} tiles fit 160 KiB; the registers allow 1 wavefront per SIMD, 4 per compute unit)")
    grid = torch.linspace(1.0, 0.0, n + 1).flip(0)
    z0 = torch.cat([x, p0], dim=1)
    z1 = odeint.solve_leapfrog(A, z0, grid)
    only_fwd = timed(lambda: odeint.solve_leapfrog(A, z0, grid), a.reps)
    print(f"forward launch alone                 {fmt(only_fwd)}")
    table = A._leapfrog_table(grid.flip(0), pull_select=True).to(DEV)
    for K in (1, 3, 7, 15):
        cot = torch.randn(B, K, 32, generator=g).to(DEV)
        t = timed(lambda: net.pullback_select(z1, table, cot), a.reps)
        print(f"backward launch alone, K = {K:2d}        {fmt(t)}    x forward launch {t[0] / only_fwd[0]:.2f}; "
              f"LDS per tile {lds_bytes(plan, K)} bytes, {16 // (1 + K)} samples per tile")
        del cot

    # ---- torch autograd on the device, 2^12 rows ---------------------------------------------------------------------------------
    Bs = min(B, 1 << 12)
    xs, ps = x[:Bs].contiguous(), p0[:Bs].contiguous()
    ta = timed(lambda: torch_autograd(A, xs, ps, n), 1, trials=3)
    tk = timed(lambda: A.log_prob_leapfrog_grad(xs, None, n, momentum=ps), a.reps)
    lp_t, g_t = torch_autograd(A, xs, ps, n)
    lp_k, g_k, _ = A.log_prob_leapfrog_grad(xs, None, n, momentum=ps)
    rel = lambda got, ref: float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    print(f"\n# torch autograd on the device, model A, {Bs} rows (fp32, states kept)")
    print(f"torch forward + backward             {fmt(ta)}")
    print(f"log_prob_leapfrog_grad               {fmt(tk)}    torch / kernel {ta[0] / tk[0]:.1f}")
    print(f"agreement: grad_x max over rows of max |diff| / max |grad| = {rel(g_k, g_t):.3e}; "
          f"log_p max |diff| = {float((lp_k - lp_t).abs().max()):.3e} (|log_p| up to {float(lp_t.abs().max()):.1f})")
    del A, net, x, p0, z0, z1, table

    # ---- model B -------------------------------------------------------------------------------------------------------------------
    Bm = symplectic(8, [256] * 3)
    netb = Bm._net()
    planb = netb.pull_select_plan()
    zb0 = torch.randn(B, 16, generator=g).to(DEV)
    zb1 = odeint.solve_leapfrog(Bm, zb0, grid)
    tableb = Bm._leapfrog_table(grid.flip(0), pull_select=True).to(DEV)
    cotb = torch.randn(B, 1, 16, generator=g).to(DEV)
    tsel = timed(lambda: netb.pullback_select(zb1, tableb, cotb), a.reps)
    tfw = timed(lambda: odeint.solve_leapfrog(Bm, zb0, grid), a.reps)
    torch.manual_seed(5)
    flow = Fm.ODEFlow(16, [256] * 3).eval().to(DEV)
    fnet = flow._net()
    E = 2 * n + 1
    span = torch.tensor([0.0, 1.0])
    opts = {"step_size": 1.0 / E}
    tab = solvers.plan_ode(span, "euler", opts)
    ftable = solvers.build_table(tab, *flow._host_schedule()(tab.t_eval), int(fnet.pull_plan().width)).to(DEV)
    assert ftable.shape[0] == E
    def pair():
        _, rec, _ = fnet.record(zb0, ftable, stage_slots=1)
        return fnet.pullback_discrete(rec, ftable, cotb, stage_slots=1)
    trec = timed(lambda: fnet.record(zb0, ftable, stage_slots=1), a.reps)
    tpair = timed(pair, a.reps)
    print(f"\n# model B: D = 8 (joint 16), C = 0, 3 x 256, {E} rows, K = 1; units {_native.kernel_name(planb)} against "
          f"mlp_rec / mlp_dadj of {_native.kernel_name(fnet.pull_plan())}")
    print(f"symplectic forward launch            {fmt(tfw)}")
    print(f"ONE pull-select launch               {fmt(tsel)}    (no record)")
    print(f"single-network record launch         {fmt(trec)}    record {E * B * 16 * 4 / 2 ** 30:.2f} GiB")
    print(f"record + discrete adjoint            {fmt(tpair)}    pair / pull-select {tpair[0] / tsel[0]:.2f}")
    print("(the pull-select launch runs two networks per row -- forward and transposed -- of ONE of mlp_q / mlp_p; the record launch "
          "runs one forward network per row and the discrete adjoint one forward and one transposed: 3 network passes against 2)")


if __name__ == "__main__":
    main()
