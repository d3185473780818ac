"""The two ends of log_prob_marginal (ff_marginal_expand / ff_marginal_reduce) against the torch-op composition of the same
ends, against the 100-step leapfrog solve between them, and against HBM; peak device memory with and without chunking.
One MI355X; HIP events; contenders alternating in one process; median [min, max] of 9.  Output: profiles/marginal.txt.

    python scratch/marginal_bench.py [out_file]
"""
import math
import statistics
import sys

import torch

sys.path.insert(0, ".")
from flowfusion_amd import _native                                             # noqa: E402
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP       # noqa: E402

DEV = "cuda"
HBM = 8.0e12
BASE = _native.MOMENTUM_NOISE_BASE
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps=9, warm=2):
    """Median [min, max] in ms of each callable, alternating them inside every repetition."""
    for _ in range(warm):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def torch_expand(x, shift, scale, K, seed):
    """What the parent commit can do: K ff_normal_fill launches, repeat_interleave, cat."""
    B, D = x.shape
    q0 = ((x - shift) / scale).repeat_interleave(K, dim=0)
    p0 = torch.empty(B, K, D, device=x.device)
    for k in range(K):
        p0[:, k] = _native.normal_fill(B, D, seed, 0, x.device, noise_index=BASE + k)
    p0 = p0.view(B * K, D)
    return torch.cat([q0, p0], dim=-1), p0


def torch_reduce(z1, p0, K, log_det):
    """The other end in torch ops, p0 kept from the expand: two Normal.log_prob, sums, logsumexp (fp32, as log_prob)."""
    normal = torch.distributions.Normal(0, 1)
    lw = (normal.log_prob(z1).sum(dim=-1) - normal.log_prob(p0).sum(dim=-1)).view(-1, K)
    return torch.logsumexp(lw, dim=1) - math.log(K) - log_det


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out_file = sys.argv[1] if len(sys.argv) > 1 else "profiles/marginal.txt"
    torch.manual_seed(0)
    D, K, B, steps, seed = 16, 16, 1 << 16, 100, 11
    fm = SymplecticFlowModel(SymplecticMLP(D, 0, 16, [256] * 3), torch.randn(D) * 0.3, torch.rand(D) + 0.5, None, None).to(DEV)
    x = torch.randn(B, D, device=DEV)
    log_det = float(torch.log(fm.scale.double()).sum())
    say("# python scratch/marginal_bench.py  (one MI355X; HIP events; contenders alternating in one process; median [min, max] of 9)")
    say(f"# B = 2^16 data points, K = {K} momenta (2^20 rows), D = {D}, C = 0, E = 16, three hidden layers of 256")

    z0, _ = _native.marginal_expand(x, K, seed, 0, fm.shift, fm.scale)
    zt, p0 = torch_expand(x, fm.shift, fm.scale, K, seed)
    assert torch.equal(z0, zt), "the kernel and the torch composition write different starting states"
    grid = torch.linspace(1.0, 0.0, steps + 1).flip(0)
    z1 = fm._integrate(z0, grid, None, "leapfrog")
    lp = _native.marginal_reduce(z1, K, seed, 0, log_det)
    lt = torch_reduce(z1, p0, K, log_det)
    say(f"# reduce kernel against the fp32 torch composition: max |diff| {float((lp - lt).abs().max()):.3e} nats")

    t_exp, t_texp = timed([lambda: _native.marginal_expand(x, K, seed, 0, fm.shift, fm.scale),
                           lambda: torch_expand(x, fm.shift, fm.scale, K, seed)])
    t_red, t_tred = timed([lambda: _native.marginal_reduce(z1, K, seed, 0, log_det), lambda: torch_reduce(z1, p0, K, log_det)])
    (t_solve,) = timed([lambda: fm._integrate(z0, grid, None, "leapfrog")], warm=1)
    rows = B * K
    exp_bytes = 4 * (B * D + rows * 2 * D)
    red_bytes = 4 * (rows * 2 * D + B)
    say(f"[expand] ff_marginal_expand {fmt(t_exp)}   torch ops (K normal_fill, repeat_interleave, cat) {fmt(t_texp)}   "
        f"ratio torch / kernel {t_texp[0] / t_exp[0]:.2f}")
    say(f"[expand] algorithmic bytes {exp_bytes / 1e6:.1f} MB (read x, write z0): {exp_bytes / (t_exp[0] * 1e-3) / 1e12:.2f} TB/s = "
        f"{exp_bytes / (t_exp[0] * 1e-3) / HBM:.2f} of 8 TB/s")
    say(f"[reduce] ff_marginal_reduce {fmt(t_red)}   torch ops (2 Normal.log_prob, sums, logsumexp; p0 kept) {fmt(t_tred)}   "
        f"ratio torch / kernel {t_tred[0] / t_red[0]:.2f}")
    say(f"[reduce] algorithmic bytes {red_bytes / 1e6:.1f} MB (read z1, write log p): {red_bytes / (t_red[0] * 1e-3) / 1e12:.2f} TB/s = "
        f"{red_bytes / (t_red[0] * 1e-3) / HBM:.2f} of 8 TB/s")
    say(f"[solve]  leapfrog, {steps} steps, 2^20 rows {fmt(t_solve)}   both kernels / solve {(t_exp[0] + t_red[0]) / t_solve[0]:.5f}   "
        f"both torch ends / solve {(t_texp[0] + t_tred[0]) / t_solve[0]:.5f}")
    t_all = timed([lambda: fm.log_prob_marginal(x, num_momenta=K, seed=seed, method="leapfrog", num_steps=steps)], reps=3, warm=1)[0]
    say(f"[whole]  log_prob_marginal(K = {K}, leapfrog {steps}) {fmt(t_all)} (median of 3)")
    del z0, zt, p0, z1, lp, lt

    # peak device memory, B = 2^20 points x K = 16 (2^24 rows), one leapfrog step (the memory does not depend on the steps)
    Bm = 1 << 20
    xm = torch.randn(Bm, D, device=DEV)
    res = {}
    for name, chunk in (("default chunks (2^22 rows)", None), ("one chunk (2^24 rows)", Bm)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res[name] = fm.log_prob_marginal(xm, num_momenta=K, seed=seed, method="leapfrog", num_steps=1, chunk_points=chunk)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        say(f"[memory] B = 2^20, K = {K}, {name}: peak {peak / 2 ** 20:.0f} MiB above the inputs")
    a, b = res.values()
    say(f"[memory] the two results are bitwise equal: {torch.equal(a, b)}")
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
