"""The timings of profiles/marginal_grad.txt: ``SymplecticFlowModel.log_prob_marginal_grad`` on an MI355X.  Needs the GPU and the
built library.

    python scratch/marginal_grad_bench.py [--points 4096] [--momenta 16] [--steps 100]

Model: D = 16 (joint 32), C = 0, 3 x 256, ``num_steps`` leapfrog steps; ``points`` x ``momenta`` rows.
  1. the whole call at ``min_weight`` = 0 against the route a user composes by hand (regenerate the momenta, run
     ``log_prob_leapfrog_grad`` on all B K rows, a float64 softmax and a contraction in torch), alternated in one run;
  2. the whole call at two ``min_weight`` values (the 50 % and 90 % quantiles of the normalised weights): the kept fraction,
     the time, and the gradient's distance from the ``min_weight`` = 0 result beside the stated bound K m max |grad lw|;
  3. the two kernels against the float64 torch composition they replace, on the rows of 1.
Times: device events around ``reps`` calls after a warm-up, the median of ``trials`` such windows.
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from flowfusion_amd import _native, odeint                      # noqa: E402
from flowfusion_amd import symplectic as Sm                     # noqa: E402

DEV = "cuda"
SEED = 11


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def timed(fn, reps, trials=5):
    """Median over ``trials`` windows of the mean milliseconds of ``reps`` calls; the spread (min, max) beside it."""
    fn()
    torch.cuda.synchronize()
    out = [window(fn, reps) for _ in range(trials)]
    return statistics.median(out), min(out), max(out)


def alternated(fa, fb, reps, trials=5):
    """The same for two routes whose windows alternate: a, b, a, b, .."""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(trials):
        ta.append(window(fa, reps))
        tb.append(window(fb, reps))
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def fmt(t):
    return f"{t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})"


def by_hand(front, x, K, n, seed):
    """What a user writes without the method: the stream's momenta regenerated, ``log_prob_leapfrog_grad`` on every row, a
    float64 softmax over each point's K values and a weighted sum."""
    B, D = x.shape
    z0, _ = _native.marginal_expand(x, K, seed, 0, front.shift, front.scale)
    p0 = z0[:, D:].contiguous()
    xr = x.repeat_interleave(K, dim=0)
    lp, gx, _ = front.log_prob_leapfrog_grad(xr, None, n, momentum=p0)
    lw = lp.double().view(B, K)
    wn = torch.softmax(lw, dim=1)
    log_p = (torch.logsumexp(lw, dim=1) - math.log(K)).float()
    return log_p, (wn[..., None] * gx.double().view(B, K, D)).sum(1).float()


def torch_weigh(z1, p0, K, log_det, m):
    """ff_marginal_weigh in float64 torch ops."""
    D = p0.shape[1]
    lw = -0.5 * ((z1.double() ** 2).sum(1) - (p0.double() ** 2).sum(1)) - D * 0.5 * math.log(2 * math.pi)
    rows = lw.view(-1, K)
    wn = torch.softmax(rows, dim=1)
    out = (torch.logsumexp(rows, dim=1) - math.log(K) - log_det).float()
    ess = (1.0 / (wn ** 2).sum(1)).float()
    return out, ess, lw, ((wn > 0) & (wn >= m)).view(-1).to(torch.int32)


def torch_grad_reduce(lw, gz, K, scale):
    """ff_marginal_grad_reduce (every row kept, no conditional) in float64 torch ops."""
    D = gz.shape[1] // 2
    wn = torch.softmax(lw.view(-1, K), dim=1)
    return ((wn[..., None] * gz[:, :D].double().view(-1, K, D)).sum(1) / scale.double()).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 12)
    ap.add_argument("--momenta", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B, K, n, D = a.points, a.momenta, a.steps, 16
    print(f"# device: {torch.cuda.get_device_name(0)}; {B} points x K = {K} momenta = {B * K} rows, D = {D}, 3 x 256, "
          f"num_steps {n} ({2 * n + 1} table rows)")
    torch.manual_seed(5)
    front = Sm.SymplecticFlowModel(Sm.SymplecticMLP(D, 0, 4, [256] * 3), torch.zeros(D), torch.ones(D), None, None).eval().to(DEV)
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(0)).to(DEV)
    call = lambda m=0.0: front.log_prob_marginal_grad(x, None, K, num_steps=n, seed=SEED, min_weight=m)

    # ---- 1. the whole call against the hand-written route ----------------------------------------------------------------------
    t_new, t_hand = alternated(call, lambda: by_hand(front, x, K, n, SEED), a.reps)
    lp, gx, _ = call()
    stats = dict(front.last_marginal_grad_stats)
    lp_h, gx_h = by_hand(front, x, K, n, SEED)
    rel = lambda got, ref: float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    print("\n# 1. the whole call, min_weight = 0, alternated with the hand-written route (windows a, b, a, b, ..)")
    print(f"log_prob_marginal_grad               {fmt(t_new)}    {stats}")
    print(f"by hand (log_prob_leapfrog_grad on all rows + torch)   {fmt(t_hand)}    by hand / method {t_hand[0] / t_new[0]:.2f}")
    print(f"agreement: grad_x max over points of max |diff| / max |grad| = {rel(gx, gx_h):.3e}; log_p max |diff| = "
          f"{float((lp - lp_h).abs().max()):.3e} (|log_p| up to {float(lp.abs().max()):.1f})")
    t_val = timed(lambda: front.log_prob_marginal(x, None, K, method="leapfrog", num_steps=n, seed=SEED), a.reps)
    print(f"log_prob_marginal (the value alone)  {fmt(t_val)}    gradient call / value call {t_new[0] / t_val[0]:.2f}")

    # ---- 2. min_weight -----------------------------------------------------------------------------------------------------------
    print("\n# 2. the whole call at min_weight > 0: rows kept, time, and the truncation beside its bound K m max |grad lw|")
    z0, _ = _native.marginal_expand(x, K, SEED, 0, front.shift, front.scale)
    _, g_rows, _ = front.log_prob_leapfrog_grad(x.repeat_interleave(K, dim=0), None, n, momentum=z0[:, D:].contiguous())
    gmax = float(g_rows.abs().max())
    _, lw0, _ = _native.marginal_weigh(odeint.solve_leapfrog(front, z0, torch.linspace(1.0, 0.0, n + 1).flip(0)), K, SEED, 0, 0.0, 0.0)
    wn = torch.softmax(lw0.view(B, K), dim=1).view(-1)
    print(f"normalised weights: min {float(wn.min()):.3e}, median {float(wn.median()):.3e}, max {float(wn.max()):.3e} (uniform: "
          f"{1.0 / K:.4f}); min_weight at their 50 % and 90 % quantiles")
    for q in (0.5, 0.9):
        m = float(torch.quantile(wn, q))
        t = timed(lambda: call(m), a.reps)
        _, gm, _ = call(m)
        s = front.last_marginal_grad_stats
        moved = float((gm - gx).abs().max())
        print(f"min_weight = {m:.4e}: kept {s['rows_kept']} of {s['rows']} rows ({s['rows_kept'] / s['rows']:.3f})  {fmt(t)}    "
              f"x the min_weight = 0 call {t[0] / t_new[0]:.2f};  max |grad_x - grad_x(0)| = {moved:.3e}, bound {K * m * gmax:.3e} "
              f"(max |grad lw| = {gmax:.3f})")

    # ---- 3. the two kernels against the float64 torch composition ------------------------------------------------------------------
    grid = torch.linspace(1.0, 0.0, n + 1).flip(0)
    z1 = odeint.solve_leapfrog(front, z0, grid)
    p0 = z0[:, D:].contiguous()
    out, lw, keep = _native.marginal_weigh(z1, K, SEED, 0, 0.0, 0.0)
    _, gz, _ = odeint._leapfrog_pull_from(front, z1, grid, (-z1)[:, None, :], None)
    gz = gz[:, 0]
    rows = torch.arange(B * K, dtype=torch.int32, device=DEV)
    scale = front.scale
    tw = timed(lambda: _native.marginal_weigh(z1, K, SEED, 0, 0.0, 0.0), 20)
    tr = timed(lambda: _native.marginal_reduce(z1, K, SEED, 0, 0.0), 20)
    tg = timed(lambda: _native.marginal_grad_reduce(lw, rows, gz, None, K, scale), 20)
    tw_t = timed(lambda: torch_weigh(z1, p0, K, 0.0, 0.0), 20)
    tg_t = timed(lambda: torch_grad_reduce(lw, gz, K, scale), 20)
    ow, _, lw_t, keep_t = torch_weigh(z1, p0, K, 0.0, 0.0)
    print(f"\n# 3. the kernels on the {B * K} rows of 1. against float64 torch ops (the momenta already in memory for torch)")
    print(f"ff_marginal_reduce                   {fmt(tr)}")
    print(f"ff_marginal_weigh                    {fmt(tw)}    torch / kernel {tw_t[0] / tw[0]:.1f}")
    print(f"  torch: squares, sums, softmax, logsumexp, keep   {fmt(tw_t)}")
    print(f"ff_marginal_grad_reduce              {fmt(tg)}    torch / kernel {tg_t[0] / tg[0]:.1f}")
    print(f"  torch: softmax, slice, weighted sum, division    {fmt(tg_t)}")
    print(f"agreement: log_p max |diff| {float((out - ow).abs().max()):.3e}; lw max |diff| {float((lw - lw_t).abs().max()):.3e}; keep "
          f"differs on {int((keep != keep_t).sum())} rows; grad_x max |diff| "
          f"{float((_native.marginal_grad_reduce(lw, rows, gz, None, K, scale)[0] - torch_grad_reduce(lw, gz, K, scale)).abs().max()):.3e}")
    tf = timed(lambda: odeint.solve_leapfrog(front, z0, grid), a.reps)
    tb = timed(lambda: odeint._leapfrog_pull_from(front, z1, grid, (-z1)[:, None, :], None), a.reps)
    print(f"forward launch alone                 {fmt(tf)}")
    print(f"backward launch alone                {fmt(tb)}    x forward launch {tb[0] / tf[0]:.2f}")


if __name__ == "__main__":
    main()
