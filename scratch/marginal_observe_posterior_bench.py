"""The timings of profiles/marginal_observe_posterior.txt: ``SymplecticFlowModel.posterior_marginal_noisy`` and
ff_marginal_observe_resample on an MI355X.  Needs the GPU, the built library and a built checkout of the PARENT commit.

    python scratch/marginal_observe_posterior_bench.py --parent PATH [--points 4096] [--draws 16] [--steps 100] [--rounds 3]

Model: D = 16 (joint 32), C = 0, 3 x 256, ``num_steps`` leapfrog steps; ``points`` x ``draws`` rows; sigma = 0.2 (0.5 + u) per
object and dimension.
  1. the whole call, against the parent commit's own code: a fresh child process per side and round, the sides alternated
     (parent, this, parent, this, ..).  The parent side times ``log_prob_marginal_noisy(return_ess=True)``; this side times the
     same call and ``posterior_marginal_noisy`` at M = 1 and M = 8.
  2. the new kernel on the rows of 1. against (a) the torch composition it replaces -- regenerate the noise, form y, a float64
     softmax, multinomial, gather, moments -- and (b) ff_weighted_resample fed a materialised particle buffer and fp32 weights.
Times: device events around ``reps`` calls after a warm-up, the median of ``trials`` such windows.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
SEED = 11


def child(a):
    """One side, one round, in this process: prints a JSON line of {name: [median, min, max] ms}."""
    sys.path.insert(0, str(Path(a.tree).resolve()))
    import torch
    from flowfusion_amd import symplectic as Sm
    B, K, n, D = a.points, a.draws, a.steps, 16

    def window(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    def timed(fn, reps=a.reps, trials=5):
        fn()
        torch.cuda.synchronize()
        out = [window(fn, reps) for _ in range(trials)]
        return [statistics.median(out), min(out), max(out)]

    torch.manual_seed(5)
    front = Sm.SymplecticFlowModel(Sm.SymplecticMLP(D, 0, 4, [256] * 3), torch.zeros(D), torch.ones(D), None, None).eval().to("cuda")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, D, generator=g).to("cuda")
    std = (0.2 * (0.5 + torch.rand(B, D, generator=g))).to("cuda")
    kw = dict(method="leapfrog", num_steps=n, seed=SEED)
    res = {"value": timed(lambda: front.log_prob_marginal_noisy(x, std, None, K, return_ess=True, **kw))}
    if a.child == "this":
        for M in (1, 8):
            res[f"posterior M={M}"] = timed(lambda: front.posterior_marginal_noisy(x, std, None, K, M, **kw))
    if a.child == "this" and a.kernels:
        res.update(kernels(front, x, std, K, n, timed))
    print("RESULT " + json.dumps(res), flush=True)


def kernels(front, x, std, K, n, timed):
    import torch
    from flowfusion_amd import _native, odeint
    B, D = x.shape
    M = 8
    z0, _ = _native.marginal_observe_expand(x, std, K, SEED, 0, front.shift, front.scale)
    z1 = odeint.solve_leapfrog(front, z0, torch.linspace(1.0, 0.0, n + 1).flip(0))
    _, lw, _ = _native.marginal_weigh(z1, K, SEED, 0, 0.0, 0.0)
    lp = lw.float()
    y, _ = _native.observe_expand(x, std, K, SEED, 0)

    def torch_posterior():
        """regenerate the noise, form y, float64 softmax, multinomial (torch's generator), gather, moments"""
        z = torch.stack([_native.normal_fill(B, D, SEED, 0, x.device, noise_index=_native.OBS_NOISE_BASE + k) for k in range(K)], dim=1)
        yk = x[:, None, :] - std[:, None, :] * z
        wn = torch.softmax(lw.view(B, K), dim=1)
        idx = torch.multinomial(wn, M, replacement=True)
        samples = torch.gather(yk, 1, idx[..., None].expand(B, M, D))
        mean = (wn[..., None] * yk.double()).sum(1)
        var = (wn[..., None] * (yk.double() - mean[:, None, :]) ** 2).sum(1)
        return samples, idx, mean.float(), var.float()

    def buffered():
        yb, _ = _native.observe_expand(x, std, K, SEED, 0)
        return _native.weighted_resample(yb, lw.float(), K, M, SEED, 0)

    out = {}
    for m in (1, 8, 0):
        out[f"ff_marginal_observe_resample M={m}"] = timed(lambda: _native.marginal_observe_resample(x, std, lw, K, m, SEED, 0), 20)
    out["torch composition M=8"] = timed(torch_posterior, 20)
    out["ff_observe_expand + fp32 cast + ff_weighted_resample M=8"] = timed(buffered, 20)
    out["ff_weighted_resample alone (buffer and fp32 weights in memory) M=8"] = timed(
        lambda: _native.weighted_resample(y, lp, K, M, SEED, 0), 20)
    new, old = _native.marginal_observe_resample(x, std, lw, K, M, SEED, 0), _native.weighted_resample(y, lp, K, M, SEED, 0)
    wn = torch.softmax(lw.view(B, K), dim=1)
    out["index differs from the fp32-weight route on (of B M)"] = [float((new[1] != old[1]).sum()), float(B * M), 0.0]
    out["mean max |diff| from the fp32-weight route, ess mean"] = [float((new[2] - old[2]).abs().max()),
                                                                   float((1.0 / (wn ** 2).sum(1)).mean()), 0.0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--points", type=int, default=1 << 12)
    ap.add_argument("--draws", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", choices=("parent", "this"))
    ap.add_argument("--tree", default=str(HERE))
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    print(f"# {a.points} points x K = {a.draws} draws = {a.points * a.draws} rows, D = 16, 3 x 256, num_steps {a.steps}; "
          f"{a.rounds} rounds, a fresh process per side and round, order parent, this, parent, this, ..")
    for r in range(a.rounds):
        for side, tree in (("parent", a.parent), ("this", str(HERE))):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", side, "--tree", tree, "--points", str(a.points),
                   "--draws", str(a.draws), "--steps", str(a.steps), "--reps", str(a.reps)]
            if side == "this" and r == a.rounds - 1:
                cmd.append("--kernels")
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=tree))
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                return p.returncode
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for name, t in res.items():
                print(f"round {r} {side:6s} {name:70s} {t[0]:10.4f} ms  (min {t[1]:.4f}, max {t[2]:.4f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
