"""Cost of the gradient of the noisy-observation log-density: python scratch/observe_grad_bench.py

2^12 observations x K = 16 noise draws of the 16-d 4 x 256 VP score model with a Hutchinson probe, 100-step rk4
(scratch/logp_grad_bench.py's model and grid), per-object error bars.  The hidden-to-hidden weights carry a gain of 4
(tests/_deep_models.py): at torch's default initialisation the network's Jacobian vanishes, every row of a point has the same
log-density and all K weights are 1 / K -- with the gain the weights spread as a trained model's do (on this model mostly by the
noise of the one-probe divergence estimate: the error bars hardly matter).  HIP events, the contenders alternating in one process, a
warm-up turn, median [min, max] of 9.

* ff_observe_keep + ff_observe_grad_reduce against the torch composition they replace on the same log-densities and gradient
  rows: ``softmax(lp.double())``, K ff_normal_fill launches for z, two weighted sums over [B, K, D] temporaries.
* ``log_prob_noisy_grad`` at ``min_weight`` = 0 against the parent commit's ingredients in the same run: ``log_prob_noisy`` plus
  ``log_prob_grad`` on the B K expanded rows (what a user composed by hand, without the reduction).
* ``log_prob_noisy_grad`` at ``min_weight`` = 1e-4 and 1e-2: rows kept, and the deviation from the ``min_weight`` = 0 gradient
  next to its bound K m max |grad lp|."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import _native                                    # noqa: E402
from flowfusion_amd import diffusion as D                             # noqa: E402
from tests._deep_models import apply_gain                             # noqa: E402

B, K, DIM, STEPS, SEED, GAIN = 1 << 12, 16, 16, 100, 7, 4.0


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


def show(t):
    return f"{statistics.median(t):8.2f} ms [{min(t):.2f}, {max(t):.2f}]"


def main():
    torch.manual_seed(0)
    mlp = D.MLP(DIM, 0, 8, [256] * 4)
    apply_gain(list(mlp.NN), GAIN)
    sm = D.ScoreModel(mlp, D.VPSDE(), no_sigma=True, hutchinson=True).eval().to("cuda")
    eps = float(sm.sde.epsilon)
    opts = {"step_size": (1.0 - eps) / STEPS}
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    std = (0.2 + 0.6 * torch.rand(B, DIM)).to("cuda")
    kw = dict(method="rk4", options=opts, seed=SEED)
    sm.log_prob_noisy_grad(x[:64], std[:64], None, K, **kw)               # (builds and caches packs and tables)
    print(f"# {B} observations x K = {K} draws = {B * K} rows, {DIM}-d, 4 x 256, VP (gain {GAIN:g}), Hutchinson, {STEPS}-step rk4")

    # the rows a hand-written composition works on: the parent's ingredients
    y, _ = _native.observe_expand(x, std, K, SEED, 0)
    rows_kw = dict(method="rk4", options=opts, probe="philox", seed=SEED, sample_offset=0)
    lp, g, _ = sm.log_prob_grad(y, **rows_kw)
    lp = lp.view(-1).contiguous()
    every = torch.arange(B * K, dtype=torch.int32, device="cuda")

    def compaction(keep):
        return torch.where(keep > 0, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)

    def kernels():
        _native.observe_keep(lp, K, 0.0)
        return _native.observe_grad_reduce(lp, every, g, None, std, K, SEED, 0)

    def kernels_and_compaction():
        keep = _native.observe_keep(lp, K, 0.0)
        rows = torch.nonzero(keep).view(-1)
        return _native.observe_grad_reduce(lp, compaction(keep), g.index_select(0, rows), None, std, K, SEED, 0)

    def composition():
        w = torch.softmax(lp.double().view(B, K), dim=1)[..., None]
        z = torch.stack([_native.normal_fill(B, DIM, SEED, 0, "cuda", noise_index=_native.OBS_NOISE_BASE + k) for k in range(K)], 1)
        gr = g.view(B, K, DIM)
        return (w * gr).sum(1).float(), None, (-(w * z * gr).sum(1)).float()

    a, b = kernels(), composition()
    print(f"kernels against the composition: max |grad_x| gap {float((a[0] - b[0]).abs().max()):.2e}, "
          f"max |grad_noise_std| gap {float((a[2] - b[2]).abs().max()):.2e}")
    t = timed({"kernels": kernels, "with compaction": kernels_and_compaction, "composition": composition})
    print(f"ff_observe_keep + ff_observe_grad_reduce {show(t['kernels'])}   with the torch compaction and gather "
          f"{show(t['with compaction'])}   torch composition {show(t['composition'])}  "
          f"({statistics.median(t['composition']) / statistics.median(t['kernels']):.1f} x the kernels)")

    outs = {}
    call = lambda m: sm.log_prob_noisy_grad(x, std, None, K, min_weight=m, return_ess=True, return_noise_grad=True, **kw)
    fns = {"noisy": lambda: sm.log_prob_noisy(x, std, None, K, **kw),
           "grad rows": lambda: sm.log_prob_grad(y, **rows_kw),
           "m=0": lambda: outs.__setitem__(0.0, (call(0.0), dict(sm.last_noisy_grad_stats))),
           "m=1e-4": lambda: outs.__setitem__(1e-4, (call(1e-4), dict(sm.last_noisy_grad_stats))),
           "m=1e-2": lambda: outs.__setitem__(1e-2, (call(1e-2), dict(sm.last_noisy_grad_stats)))}
    t = timed(fns)
    med = {k: statistics.median(v) for k, v in t.items()}
    ess = outs[0.0][0][3]
    (_, gx0, _, _, gs0), _ = outs[0.0]
    print(f"effective sample size of the {K} weights: median {float(ess.median()):.2f}, mean {float(ess.mean()):.2f}; points without a "
          f"gradient (a non-finite row): {int(torch.isnan(gx0[:, 0]).sum())}")
    print(f"log_prob_noisy {show(t['noisy'])}   log_prob_grad on the {B * K} expanded rows {show(t['grad rows'])}   "
          f"sum {med['noisy'] + med['grad rows']:.2f} ms")
    print(f"log_prob_noisy_grad, min_weight = 0 {show(t['m=0'])}  ({med['m=0'] / (med['noisy'] + med['grad rows']):.3f} x the parent's "
          f"ingredients, which solve for the value twice; {med['m=0'] / med['grad rows']:.3f} x log_prob_grad on the rows = one "
          f"value solve plus the record and gradient launches)")
    gmax = float(g.abs().max())
    for m, name in ((1e-4, "m=1e-4"), (1e-2, "m=1e-2")):
        (_, gx, _, _, gs), stats = outs[m]
        print(f"log_prob_noisy_grad, min_weight = {m:g} {show(t[name])}  ({med[name] / med['m=0']:.3f} x min_weight = 0); rows kept "
              f"{stats['rows_kept']} of {stats['rows']} ({stats['rows_kept'] / stats['rows']:.3f}); max |grad_x - grad_x at 0| "
              f"{float(torch.nan_to_num(gx - gx0).abs().max()):.3e}, bound K m max |grad lp| = {K * m * gmax:.3e}")


if __name__ == "__main__":
    main()
