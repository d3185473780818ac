"""ff_weighted_resample against the torch-op composition it replaces and against HBM, and the whole posterior_noisy call
against log_prob_noisy on the same observations.  One MI355X; HIP events around 20 calls; contenders alternating in one
process; median [min, max] of 9 (the method of scratch/observe_bench.py).  Output: profiles/observe_posterior.txt.

    python scratch/observe_posterior_bench.py [out_file]
"""
import ctypes
import sys

import torch

sys.path.insert(0, ".")
from flowfusion_amd import _native                                             # noqa: E402
from flowfusion_amd.diffusion import MLP, VPSDE, ScoreModel                    # noqa: E402
from scratch.observe_bench import DEV, HBM, INNER, fmt, lines, say, timed      # noqa: E402


def torch_posterior(y, lp, K, M):
    """What a user composes today from the particles: a float64 softmax, a cumsum, a searchsorted on torch's generator, a
    gather, and the weighted mean and variance."""
    B, D = y.shape[0] // K, y.shape[1]
    w = torch.softmax(lp.double().view(B, K), dim=1)
    cum = torch.cumsum(w, dim=1)
    u = torch.rand(B, M, device=y.device, dtype=torch.float64) * cum[:, -1:]
    index = torch.searchsorted(cum, u, right=True).clamp_(max=K - 1)
    yk = y.view(B, K, D)
    samples = torch.gather(yk, 1, index[:, :, None].expand(B, M, D))
    mean = (w[:, :, None] * yk).sum(1)
    var = (w[:, :, None] * (yk - mean[:, None, :]) ** 2).sum(1)
    return samples, index.int(), mean.float(), var.float()


def main():
    out_file = sys.argv[1] if len(sys.argv) > 1 else "profiles/observe_posterior.txt"
    say(f"# python scratch/observe_posterior_bench.py  (one MI355X; HIP events around {INNER} calls; contenders alternating in one "
        "process; median [min, max] of 9, per call)")
    assert torch.cuda.is_available(), "the timings need the GPU"
    torch.manual_seed(0)
    D, K, B, steps, seed = 16, 16, 1 << 16, 100, 11
    rows = B * K
    say(f"# B = 2^16 observations, K = {K} particles each (2^20 rows), D = {D}")
    x, std = torch.randn(B, D, device=DEV), torch.rand(B, D, device=DEV) * 0.5
    y, _ = _native.observe_expand(x, std, K, seed, 0)
    lp = torch.randn(rows, device=DEV) * 3 - 20
    for M in (1, 8):
        got, ref = _native.weighted_resample(y, lp, K, M, seed), torch_posterior(y, lp, K, M)
        say(f"# M = {M}: kernel against the torch composition: max |mean diff| {float((got[2] - ref[2]).abs().max()):.3e}, "
            f"max |var diff| {float((got[3] - ref[3]).abs().max()):.3e} (other uniforms: the indices are not comparable)")
        t_k, t_t = timed([lambda: _native.weighted_resample(y, lp, K, M, seed), lambda: torch_posterior(y, lp, K, M)])
        # the C entry point on outputs allocated once: the kernel without the binding's four allocations per call
        L, (s, i, mu, v) = _native.lib(), got
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        raw = lambda: L.ff_weighted_resample(y.data_ptr(), lp.data_ptr(), B, D, K, M, seed, 0, s.data_ptr(), i.data_ptr(),
                                             mu.data_ptr(), v.data_ptr(), stream)
        (t_raw,) = timed([raw])
        assert all(torch.equal(a, b) for a, b in zip(got, _native.weighted_resample(y, lp, K, M, seed)))
        say(f"[resample M={M}] the C entry point on preallocated outputs {fmt(t_raw)}")
        t_best = min(t_k, t_raw)
        nbytes = 4 * (rows + rows * D + B * M * D + B * M + 2 * B * D)
        say(f"[resample M={M}] ff_weighted_resample {fmt(t_k)}   torch ops (float64 softmax, cumsum, searchsorted, gather, moments) "
            f"{fmt(t_t)}   ratio torch / kernel {t_t[0] / t_k[0]:.2f}")
        say(f"[resample M={M}] algorithmic bytes {nbytes / 1e6:.1f} MB (read lp and y once, write samples, index, mean, var), at the "
            f"faster of the two timings of the kernel: "
            f"{nbytes / (t_best[0] * 1e-3) / 1e12:.2f} TB/s = {nbytes / (t_best[0] * 1e-3) / HBM:.2f} of 8 TB/s")
    del y, lp

    # the whole call on the headline score model (16-dim VP-SDE, 4 x 256, Hutchinson divergence, 100-step RK4)
    sm = ScoreModel(MLP(D, 0, 8, [256] * 4), VPSDE(), no_sigma=True, hutchinson=True).eval().to(DEV)
    solver = dict(method="rk4", options={"step_size": (1.0 - 1e-3) / steps})
    post = lambda: sm.posterior_noisy(x, std, num_draws=K, num_samples=8, seed=seed, **solver)
    noisy = lambda: sm.log_prob_noisy(x, std, num_draws=K, seed=seed, return_ess=True, **solver)
    a, b = post(), noisy()
    assert torch.equal(a.log_prob, b[0]) and torch.equal(a.ess, b[1])
    t_post, t_noisy = timed([post, noisy], reps=3, warm=1, inner=1)
    say(f"[whole]  posterior_noisy(B = 2^16, K = {K}, M = 8, rk4 {steps} steps, Hutchinson) {fmt(t_post)}   log_prob_noisy(return_ess) "
        f"{fmt(t_noisy)}   ratio {t_post[0] / t_noisy[0]:.4f} (median of 3)")
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
