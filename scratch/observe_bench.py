"""The two ends of log_prob_noisy (ff_observe_expand / ff_logmeanexp) against the torch-op composition each replaces and
against HBM, and the whole call against log_prob on the same rows expanded beforehand.  One MI355X; HIP events around 20
calls; contenders alternating in one process; median [min, max] of 9.  Also the float64 statement of the closed-form test
(tests/test_observe_host.py), which needs no GPU.  Output: profiles/observe.txt.

    python scratch/observe_bench.py [out_file]
"""
import math
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from flowfusion_amd import _native                                             # noqa: E402
from flowfusion_amd.diffusion import MLP, VPSDE, ScoreModel                    # noqa: E402

DEV = "cuda"
HBM = 8.0e12
BASE = _native.OBS_NOISE_BASE
INNER = 20
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps=9, warm=2, inner=INNER):
    """Median [min, max] in ms per call of each callable: ``inner`` calls between two events, alternating the callables
    inside every repetition."""
    for _ in range(warm):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / inner)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def fmt(t):
    return f"{t[0]:9.4f} ms [{t[1]:.4f}, {t[2]:.4f}]"


def torch_expand(x, std, K, seed):
    """What the parent commit can do: K ff_normal_fill launches, a multiply, a subtract over [B, K, D]."""
    B, D = x.shape
    z = torch.empty(B, K, D, device=x.device)
    for k in range(K):
        z[:, k] = _native.normal_fill(B, D, seed, 0, x.device, noise_index=BASE + k)
    return (x.view(B, 1, D) - std.view(B, 1, D) * z).view(B * K, D)


def torch_logmeanexp(lp, K):
    """The other end in torch ops (fp32, as a user would write it around log_prob)."""
    return torch.logsumexp(lp.view(-1, K), dim=1) - math.log(K)


def closed_form_reference():
    from tests.test_observe_host import closed_form_inputs, exact_observed
    B, D, seed, shift, scale, sigma, x = closed_form_inputs()
    exact = exact_observed(x, shift, scale, sigma)
    sc = scale.astype(np.float64)
    out = {}
    for K in (4, 64):
        y = _native.observe_expand(torch.from_numpy(x), torch.from_numpy(sigma), K, seed, 0)[0].numpy().astype(np.float64)
        lp = (-0.5 * ((y - shift) / sc) ** 2 - 0.5 * math.log(2 * math.pi)).sum(1) - np.log(sc).sum()
        ess = torch.empty(B)
        got = _native.logmeanexp(torch.from_numpy(lp.astype(np.float32)), K, None, ess).numpy().astype(np.float64)
        out[K] = (float(np.sqrt(np.mean((got - exact) ** 2))), float(ess.mean()))
    say("# closed form N(shift, scale^2 + sigma^2), 256 points, D = 3, sigma = 0.2 .. 0.6 scale, seed 8 -- the estimator on the CPU "
        "(host twins, per-row log-density in float64):")
    say(f"[closed form, CPU float64] rms error K=4 {out[4][0]:.4f} nats, K=64 {out[64][0]:.4f} nats, ratio {out[64][0] / out[4][0]:.3f} "
        f"(bar 0.35, theory 0.25); mean ess at K=64 {out[64][1]:.2f}")


def main():
    out_file = sys.argv[1] if len(sys.argv) > 1 else "profiles/observe.txt"
    say(f"# python scratch/observe_bench.py  (one MI355X; HIP events around {INNER} calls; contenders alternating in one process; "
        "median [min, max] of 9, per call)")
    closed_form_reference()
    assert torch.cuda.is_available(), "the timings need the GPU"
    torch.manual_seed(0)
    D, K, B, steps, seed = 16, 16, 1 << 16, 100, 11
    rows = B * K
    say(f"# B = 2^16 observations, K = {K} draws (2^20 rows), D = {D}, noise_std [B, D]")
    x, std = torch.randn(B, D, device=DEV), torch.rand(B, D, device=DEV) * 0.5

    y, _ = _native.observe_expand(x, std, K, seed, 0)
    assert torch.equal(y, torch_expand(x, std, K, seed)), "the kernel and the torch composition write different rows"
    lp = torch.randn(rows, device=DEV) * 3 - 20
    a, b = _native.logmeanexp(lp, K), torch_logmeanexp(lp, K)
    say(f"# ff_logmeanexp against the fp32 torch composition: max |diff| {float((a - b).abs().max()):.3e} nats")

    t_exp, t_texp = timed([lambda: _native.observe_expand(x, std, K, seed, 0), lambda: torch_expand(x, std, K, seed)])
    t_red, t_tred = timed([lambda: _native.logmeanexp(lp, K), lambda: torch_logmeanexp(lp, K)])
    exp_bytes = 4 * (2 * B * D + rows * D)
    red_bytes = 4 * (rows + B)
    say(f"[expand] ff_observe_expand {fmt(t_exp)}   torch ops (K normal_fill, multiply, subtract) {fmt(t_texp)}   "
        f"ratio torch / kernel {t_texp[0] / t_exp[0]:.2f}")
    say(f"[expand] algorithmic bytes {exp_bytes / 1e6:.1f} MB (read x and noise_std, write y): "
        f"{exp_bytes / (t_exp[0] * 1e-3) / 1e12:.2f} TB/s = {exp_bytes / (t_exp[0] * 1e-3) / HBM:.2f} of 8 TB/s")
    say(f"[reduce] ff_logmeanexp     {fmt(t_red)}   torch ops (logsumexp, - log K; fp32) {fmt(t_tred)}   "
        f"ratio torch / kernel {t_tred[0] / t_red[0]:.2f}")
    say(f"[reduce] algorithmic bytes {red_bytes / 1e6:.2f} MB (read lp, write out): "
        f"{red_bytes / (t_red[0] * 1e-3) / 1e12:.3f} TB/s = {red_bytes / (t_red[0] * 1e-3) / HBM:.3f} of 8 TB/s")
    del y, lp

    # the whole call on the headline score model (16-dim VP-SDE, 4 x 256, Hutchinson divergence, 100-step RK4)
    sm = ScoreModel(MLP(D, 0, 8, [256] * 4), VPSDE(), no_sigma=True, hutchinson=True).eval().to(DEV)
    solver = dict(method="rk4", options={"step_size": (1.0 - 1e-3) / steps})
    y, _ = _native.observe_expand(x, std, K, seed, 0)
    noisy = lambda: sm.log_prob_noisy(x, std, num_draws=K, seed=seed, **solver)
    plain = lambda: sm.log_prob(y, probe="philox", seed=seed, sample_offset=0, **solver)
    assert torch.equal(noisy(), _native.logmeanexp(plain(), K).view(-1, 1))
    t_noisy, t_plain = timed([noisy, plain], reps=3, warm=1, inner=1)
    say(f"[whole]  log_prob_noisy(B = 2^16, K = {K}, rk4 {steps} steps, Hutchinson) {fmt(t_noisy)}   log_prob on the 2^20 rows "
        f"expanded beforehand {fmt(t_plain)}   ratio {t_noisy[0] / t_plain[0]:.4f} (median of 3)")
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
