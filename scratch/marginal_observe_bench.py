"""The timings of profiles/marginal_observe.txt: ``SymplecticFlowModel.log_prob_marginal_noisy`` / ``log_prob_marginal_noisy_grad``
on an MI355X.  Needs the GPU and the built library.

    python scratch/marginal_observe_bench.py [--points 4096] [--draws 16] [--steps 100]

Model: D = 16 (joint 32), C = 0, 3 x 256, ``num_steps`` leapfrog steps; ``points`` x ``draws`` rows; sigma = 0.2 (0.5 + u) per
object and dimension.
  1. the whole gradient call (with and without grad_noise_std) against ``log_prob_marginal_grad`` on the same rows, and the whole
     value call against ``log_prob_marginal``, the sides alternated in one run;
  2. the gradient call at two ``min_weight`` values (the 50 % and 90 % quantiles of the normalised weights): rows kept and time;
  3. each new kernel against the torch composition it replaces, on the rows of 1.
Times: device events around ``reps`` calls after a warm-up, the median of ``trials`` such windows.
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from flowfusion_amd import _native, odeint                      # noqa: E402
from flowfusion_amd import symplectic as Sm                     # noqa: E402
from scratch.marginal_grad_bench import alternated, fmt, timed  # noqa: E402

DEV = "cuda"
SEED = 11


def torch_expand(x, std, K, seed, shift, scale):
    """ff_marginal_observe_expand in torch ops: 2 K ff_normal_fill launches, stacks, repeat_interleave, the arithmetic, cat."""
    B, D = x.shape
    fill = lambda base: torch.stack([_native.normal_fill(B, D, seed, 0, x.device, noise_index=base + k) for k in range(K)], dim=1)
    z, p = fill(_native.OBS_NOISE_BASE), fill(_native.MOMENTUM_NOISE_BASE)
    y = x[:, None, :] - std[:, None, :] * z
    return torch.cat([(y - shift) / scale, p], dim=-1).view(B * K, 2 * D)


def torch_grad_reduce(lw, gz, z, K, scale):
    """ff_marginal_observe_grad_reduce (every row kept, no conditional) in float64 torch ops, the noise already in memory."""
    D = gz.shape[1] // 2
    wn = torch.softmax(lw.view(-1, K), dim=1)[..., None]
    g = gz[:, :D].double().view(-1, K, D)
    return ((wn * g).sum(1) / scale.double()).float(), (-(wn * z.double() * g).sum(1) / scale.double()).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 12)
    ap.add_argument("--draws", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B, K, n, D = a.points, a.draws, a.steps, 16
    print(f"# device: {torch.cuda.get_device_name(0)}; {B} points x K = {K} draws = {B * K} rows, D = {D}, 3 x 256, "
          f"num_steps {n} ({2 * n + 1} table rows)")
    torch.manual_seed(5)
    front = Sm.SymplecticFlowModel(Sm.SymplecticMLP(D, 0, 4, [256] * 3), torch.zeros(D), torch.ones(D), None, None).eval().to(DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, D, generator=g).to(DEV)
    std = (0.2 * (0.5 + torch.rand(B, D, generator=g))).to(DEV)
    noisy = lambda m=0.0, s=True: front.log_prob_marginal_noisy_grad(x, std, None, K, num_steps=n, seed=SEED, min_weight=m,
                                                                     return_noise_grad=s)
    plain = lambda: front.log_prob_marginal_grad(x, None, K, num_steps=n, seed=SEED)

    print("\n# 1. whole calls, the sides alternated (windows a, b, a, b, ..)")
    t_new, t_old = alternated(noisy, plain, a.reps)
    print(f"log_prob_marginal_noisy_grad (+ grad_noise_std)   {fmt(t_new)}    {front.last_marginal_noisy_grad_stats}")
    print(f"log_prob_marginal_grad, the same rows             {fmt(t_old)}    noisy / plain {t_new[0] / t_old[0]:.4f}")
    t_new2, t_old2 = alternated(lambda: noisy(0.0, False), plain, a.reps)
    print(f"log_prob_marginal_noisy_grad (no grad_noise_std)  {fmt(t_new2)}")
    print(f"log_prob_marginal_grad, the same rows             {fmt(t_old2)}    noisy / plain {t_new2[0] / t_old2[0]:.4f}")
    vkw = dict(method="leapfrog", num_steps=n, seed=SEED)
    t_v, t_vo = alternated(lambda: front.log_prob_marginal_noisy(x, std, None, K, **vkw),
                           lambda: front.log_prob_marginal(x, None, K, **vkw), a.reps)
    print(f"log_prob_marginal_noisy                           {fmt(t_v)}")
    print(f"log_prob_marginal, the same rows                  {fmt(t_vo)}    noisy / plain {t_v[0] / t_vo[0]:.4f}")

    print("\n# 2. the gradient call at min_weight > 0: rows kept and time")
    z0, _ = _native.marginal_observe_expand(x, std, K, SEED, 0, front.shift, front.scale)
    grid = torch.linspace(1.0, 0.0, n + 1).flip(0)
    z1 = odeint.solve_leapfrog(front, z0, grid)
    _, lw, _ = _native.marginal_weigh(z1, K, SEED, 0, 0.0, 0.0)
    wn = torch.softmax(lw.view(B, K), dim=1).view(-1)
    print(f"normalised weights: min {float(wn.min()):.3e}, median {float(wn.median()):.3e}, max {float(wn.max()):.3e} (uniform: "
          f"{1.0 / K:.4f}); min_weight at their 50 % and 90 % quantiles")
    for q in (0.5, 0.9):
        m = float(torch.quantile(wn, q))
        t = timed(lambda: noisy(m), a.reps)
        s = front.last_marginal_noisy_grad_stats
        print(f"min_weight = {m:.4e}: kept {s['rows_kept']} of {s['rows']} rows ({s['rows_kept'] / s['rows']:.3f})  {fmt(t)}    "
              f"x the min_weight = 0 call {t[0] / t_new[0]:.2f}")

    print(f"\n# 3. the kernels on the {B * K} rows of 1. against the torch composition they replace")
    _, gz, _ = odeint._leapfrog_pull_from(front, z1, grid, (-z1)[:, None, :], None)
    gz = gz[:, 0]
    rows = torch.arange(B * K, dtype=torch.int32, device=DEV)
    scale, shift = front.scale, front.shift
    z = torch.stack([_native.normal_fill(B, D, SEED, 0, DEV, noise_index=_native.OBS_NOISE_BASE + k) for k in range(K)], dim=1)
    te = timed(lambda: _native.marginal_observe_expand(x, std, K, SEED, 0, shift, scale), 20)
    te_p = timed(lambda: _native.marginal_expand(x, K, SEED, 0, shift, scale), 20)
    te_t = timed(lambda: torch_expand(x, std, K, SEED, shift, scale), 20)
    tg = timed(lambda: _native.marginal_observe_grad_reduce(lw, rows, gz, None, std, K, SEED, 0, scale), 20)
    tg_p = timed(lambda: _native.marginal_grad_reduce(lw, rows, gz, None, K, scale), 20)
    tg_t = timed(lambda: torch_grad_reduce(lw, gz, z, K, scale), 20)
    print(f"ff_marginal_observe_expand            {fmt(te)}    torch / kernel {te_t[0] / te[0]:.1f}")
    print(f"  ff_marginal_expand (its parent)     {fmt(te_p)}")
    print(f"  torch: 2 K fills, stack, arithmetic, cat   {fmt(te_t)}")
    print(f"ff_marginal_observe_grad_reduce       {fmt(tg)}    torch / kernel {tg_t[0] / tg[0]:.1f}")
    print(f"  ff_marginal_grad_reduce (its parent) {fmt(tg_p)}")
    print(f"  torch: softmax, slice, two weighted sums, divisions (z in memory)   {fmt(tg_t)}")
    ze = torch_expand(x, std, K, SEED, shift, scale)
    gx, _, gs = _native.marginal_observe_grad_reduce(lw, rows, gz, None, std, K, SEED, 0, scale)
    gx_t, gs_t = torch_grad_reduce(lw, gz, z, K, scale)
    print(f"agreement: z0 differs from the torch composition on {int((ze != z0).sum())} of {z0.numel()} entries; grad_x max |diff| "
          f"{float((gx - gx_t).abs().max()):.3e}; grad_noise_std max |diff| {float((gs - gs_t).abs().max()):.3e} "
          f"(|grad_noise_std| up to {float(gs.abs().max()):.2f})")


if __name__ == "__main__":
    main()
