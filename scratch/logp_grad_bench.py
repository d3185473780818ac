"""Cost of the log-density gradient: python scratch/logp_grad_bench.py [rows of the autograd contender]

The 2^16 x 16-d 4 x 256 VP score model with a Hutchinson probe, 100-step rk4 (scratch/pullback_discrete_bench.py's model and
grid), one probe per sample.

``log_prob_grad`` -- per piece of rows the value solve, one record launch (mlp_rec_m16_h256_d4_c4) and one gradient launch
(mlp_lgrad_m16_h256_d4_c4) -- against the Hutchinson ``log_prob`` alone and against ``flow_vjp(adjoint="discrete")`` at K = 1, in
the same run.  HIP events, the contenders alternating in one process, a warm-up turn, median [min, max] of 9.  The three launches
are also timed alone (through ``log_prob``, FusedNet.record and FusedNet.logp_grad on the first piece of rows the front end cuts).
At 2^12 rows the same gradient by torch autograd on the device (double backward through ``ScoreModel.forward`` over the same
3/8-rule steps) is timed against ``log_prob_grad`` on those rows, and the largest difference between the two is printed."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd import odeint, solvers                            # noqa: E402

B, DIM, STEPS = 1 << 16, 16, 100


def timed(fns, turns=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for r in range(turns):                        # the first turn warms up
        for k, fn in fns.items():
            torch.cuda.synchronize()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(s.elapsed_time(e))
    return times


def autograd_gradient(sm, x, e, eps, steps):
    """(log_p [B], grad_x [B, D]) by torch autograd: the 3/8-rule steps of method="rk4" on ``ScoreModel.forward`` (its Hutchinson
    divergence is a ``create_graph`` vjp), then one backward through all of it."""
    sm.prob, sm.e, sm.conditional = True, e, None
    with torch.enable_grad():
        x0 = x.clone().requires_grad_(True)
        y, lp = x0, torch.zeros(x.shape[0], device=x.device)
        h = (1.0 - eps) / steps
        f = lambda t, v: sm.forward(torch.tensor(t, device=x.device), (v, None))
        for i in range(steps):
            t = eps + i * h
            k1, d1 = f(t, y)
            k2, d2 = f(t + h / 3, y + h * k1 / 3)
            k3, d3 = f(t + 2 * h / 3, y + h * (k2 - k1 / 3))
            k4, d4 = f(t + h, y + h * (k1 - k2 + k3))
            y = y + h * (k1 + 3 * (k2 + k3) + k4) / 8
            lp = lp + h * (d1 + 3 * (d2 + d3) + d4).view(-1) / 8
        logp = lp + sm.sde.prior(y.shape).log_prob(y).sum(dim=1)
        (g,) = torch.autograd.grad(logp.sum(), x0)
    return logp.detach(), g


def main(small):
    torch.manual_seed(0)
    sm = D.ScoreModel(D.MLP(DIM, 0, 8, [256] * 4), D.VPSDE(), no_sigma=True, hutchinson=True).eval().to("cuda")
    eps = float(sm.sde.epsilon)
    opts = {"step_size": (1.0 - eps) / STEPS}
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    kw = dict(method="rk4", options=opts, probe="philox", seed=7)
    sm.log_prob_grad(x[:64], **kw)                                        # (builds and caches packs and tables)
    sm.flow_vjp(x[:64], torch.ones(64, 1, DIM, device="cuda"), direction="to_base", method="rk4", options=opts, adjoint="discrete")
    net = sm._net()
    plan = net.pull_plan()
    tab = solvers.plan_ode(torch.tensor([eps, 1.0]), "rk4", opts)
    table = solvers.build_table(tab, *sm._host_schedule()(tab.t_eval), int(plan.width)).to("cuda")
    E = int(table.shape[0])
    rows = min(B, odeint.discrete_piece_rows(B, 1, E, DIM))                 # the front end's first piece
    print(f"# B = {B}, {DIM}-d, 4 x 256, VP, {STEPS}-step rk4 = {E} rows; one probe; record {E * B * DIM * 4 / 1e9:.2f} GB each way per "
          f"call, {-(-B // rows)} pieces of {rows} rows")
    xp = x[:rows].contiguous()
    w = torch.randn(B, 1, DIM, device="cuda")
    ep = torch.sign(torch.randn(rows, DIM, device="cuda"))
    _, rec, _ = net.record(xp, table, stage_slots=4)
    cot = torch.randn(rows, DIM, device="cuda")
    outs = {}
    times = timed({"log_prob": lambda: sm.log_prob(x, **kw),
                   "discrete": lambda: sm.flow_vjp(x, w, direction="to_base", method="rk4", options=opts, adjoint="discrete"),
                   "log_prob_grad": lambda: outs.__setitem__("grad", sm.log_prob_grad(x, **kw)),
                   "value": lambda: sm.log_prob(xp, **kw),
                   "record": lambda: net.record(xp, table, stage_slots=4),
                   "gradient": lambda: net.logp_grad(rec, table, ep, cot, None, stage_slots=4),
                   "backward": lambda: net.pullback_discrete(rec, table, cot[:, None].contiguous(), stage_slots=4)})
    med = {k: statistics.median(v) for k, v in times.items()}
    rng = {k: f"[{min(v):.1f}, {max(v):.1f}]" for k, v in times.items()}
    print(f"log_prob (Hutchinson) {med['log_prob']:8.1f} ms {rng['log_prob']}   flow_vjp discrete K = 1 {med['discrete']:8.1f} ms "
          f"{rng['discrete']}   log_prob_grad {med['log_prob_grad']:8.1f} ms {rng['log_prob_grad']}  "
          f"({med['log_prob_grad'] / med['log_prob']:.2f} x log_prob, {med['log_prob_grad'] / med['discrete']:.2f} x the discrete flow_vjp)")
    print(f"per piece of {rows} rows: value solve {med['value']:7.1f} ms {rng['value']}, record launch {med['record']:7.1f} ms "
          f"{rng['record']}, gradient launch {med['gradient']:8.1f} ms {rng['gradient']} ({med['gradient'] / med['value']:.2f} x the "
          f"Hutchinson solve, {med['gradient'] / med['backward']:.2f} x the discrete-adjoint launch {med['backward']:.1f} ms {rng['backward']})")
    del rec
    # the same gradient by torch autograd, at `small` rows
    xs = x[:small].contiguous()
    lp, gx, _ = sm.log_prob_grad(xs, **kw)
    e = sm.e.clone()
    alp, ag = autograd_gradient(sm, xs, e, eps, STEPS)
    scale = float(ag.abs().max())
    t2 = timed({"autograd": lambda: autograd_gradient(sm, xs, e, eps, STEPS), "log_prob_grad": lambda: sm.log_prob_grad(xs, **kw)}, turns=4)
    m2 = {k: statistics.median(v) for k, v in t2.items()}
    print(f"{small} rows: torch autograd (double backward) {m2['autograd']:8.1f} ms [{min(t2['autograd']):.1f}, {max(t2['autograd']):.1f}]   "
          f"log_prob_grad {m2['log_prob_grad']:7.1f} ms [{min(t2['log_prob_grad']):.1f}, {max(t2['log_prob_grad']):.1f}]  "
          f"({m2['autograd'] / m2['log_prob_grad']:.1f} x faster);  largest |grad_x - autograd| {float((gx - ag).abs().max()) / scale:.2e} of "
          f"max |grad|, |log_p - autograd| {float((lp[:, 0] - alp).abs().max()):.2e}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 12)
