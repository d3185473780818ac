"""Hutchinson log-density with K probes per sample in one launch (num_probes=K) against the exact trace and against K
separate single-probe solves; ff_probe_fill against the torch composition of K ff_normal_fill launches, and against HBM.
One MI355X; HIP events; contenders alternating in one process; median [min, max] of 5.  Output: profiles/hutch_multi.txt.

    python scratch/hutch_multi_bench.py [out_file]
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from flowfusion_amd import _native                                             # noqa: E402
from flowfusion_amd.diffusion import MLP, VPSDE, ScoreModel                    # noqa: E402
from flowfusion_amd.flow import ODEFlow                                        # noqa: E402
from flowfusion_amd.fused import MODE_EXACT, MODE_HUTCH, exact_trace_passes    # noqa: E402

DEV = "cuda"
HBM = 8.0e12
KS = (1, 3, 7, 15)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fns, reps=5, warm=1):
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
    return f"{t[0]:9.2f} ms [{t[1]:.2f}, {t[2]:.2f}]"


def report(tag, exact, multi, separate, tile, passes):
    say(f"[{tag}] exact trace ({passes} pass{'es' if passes > 1 else ''})          {fmt(exact)}")
    one = multi[1][0]
    for K in KS:
        occupancy = (tile // 2) / (tile // (1 + K))          # tiles per sample against K = 1
        say(f"[{tag}] num_probes={K:2d} (one launch)        {fmt(multi[K])}   = {multi[K][0] / one:5.2f} x K=1 (tile occupancy predicts "
            f"{occupancy:.1f}), {multi[K][0] / exact[0]:5.2f} x exact;   {K} separate K=1 solves {fmt(separate[K])}   "
            f"separate / one launch {separate[K][0] / multi[K][0]:.2f}")


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out_file = sys.argv[1] if len(sys.argv) > 1 else "profiles/hutch_multi.txt"
    say("# python scratch/hutch_multi_bench.py  (one MI355X; HIP events; contenders alternating in one process; median [min, max] of 5)")
    say("# whole front-end calls with probe='philox' (the probe fill is inside the timing); 100-step rk4")
    torch.manual_seed(0)

    # the headline workload: 2^16 x 16-d, 4 x 256
    B, D = 1 << 16, 16
    sm = ScoreModel(MLP(D, 0, 8, [256] * 4), VPSDE(), no_sigma=True, hutchinson=True).eval().to(DEV)
    x = torch.randn(B, D, device=DEV) * 0.8
    kw = dict(method="rk4", options={"step_size": (1.0 - float(sm.sde.epsilon)) / 100})
    tile = int(sm._net().plan(MODE_HUTCH).tile)

    def exact():
        sm.hutch = False
        sm.log_prob(x, **kw)
        sm.hutch = True

    def multi(K):
        return lambda: sm.log_prob(x, probe="philox", seed=5, num_probes=K, **kw)

    def separate(K):
        def run():
            for k in range(K):
                sm.log_prob(x, probe="philox", seed=100 + k, **kw)
        return run
    fns = [exact] + [multi(K) for K in KS] + [separate(K) for K in KS]
    t = timed(fns)
    say(f"# score model, B = 2^16, D = 16, 4 x 256 ({_native.kernel_name(sm._net().plan(MODE_HUTCH))}, tile {tile})")
    report("c2 16d", t[0], dict(zip(KS, t[1:5])), dict(zip(KS, t[5:9])), tile, len(exact_trace_passes(D, tile)))
    del sm, x

    # config 4's flow: 2^14 x 64-d, 5 x 512
    B, D = 1 << 14, 64
    f = ODEFlow(D, [512] * 5).eval().to(DEV)
    x = torch.randn(B, D, device=DEV)
    kw = dict(method="rk4", options={"step_size": 0.01})
    tile = int(f._net().plan(MODE_HUTCH).tile)
    fns = ([lambda: f.log_prob(x, **kw)] +
           [(lambda K: lambda: f.log_prob(x, hutchinson=True, probe="philox", seed=5, num_probes=K, **kw))(K) for K in KS] +
           [(lambda K: lambda: [f.log_prob(x, hutchinson=True, probe="philox", seed=100 + k, **kw) for k in range(K)])(K) for K in KS])
    t = timed(fns, reps=3)
    say(f"# flow, B = 2^14, D = 64, 5 x 512 ({_native.kernel_name(f._net().plan(MODE_HUTCH))}, tile {tile}; median of 3)")
    report("c4 64d", t[0], dict(zip(KS, t[1:5])), dict(zip(KS, t[5:9])), tile, len(exact_trace_passes(D, int(f._net().plan(MODE_EXACT).tile))))
    del f, x

    # the probe fill against the torch composition
    B, D = 1 << 16, 16
    for K in (3, 15):
        scale = K ** -0.5
        idx = [_native.PROBE_NOISE_INDEX] + [_native.HUTCH_PROBE_NOISE_BASE + k for k in range(1, K)]

        def composed():
            zs = torch.stack([_native.normal_fill(B, D, 5, 0, DEV, noise_index=i) for i in idx], dim=1)
            return torch.where(zs >= 0, 1.0, -1.0) * scale
        assert torch.equal(_native.probe_fill(B, K, D, 5, 0, DEV, scale=scale), composed())
        t_fill, t_comp = timed([lambda: _native.probe_fill(B, K, D, 5, 0, DEV, scale=scale), composed], reps=9, warm=2)
        nbytes = 4 * B * K * D
        say(f"[fill K={K:2d}] ff_probe_fill {fmt(t_fill)}   torch ops (K normal_fill, stack, where, mul) {fmt(t_comp)}   ratio "
            f"{t_comp[0] / t_fill[0]:.1f};  {nbytes / 1e6:.1f} MB written: {nbytes / (t_fill[0] * 1e-3) / 1e12:.2f} TB/s = "
            f"{nbytes / (t_fill[0] * 1e-3) / HBM:.2f} of 8 TB/s")
    with open(out_file, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
