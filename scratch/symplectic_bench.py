"""Symplectic flow timing (not a test): sample at 2^20 samples with num_steps 1 and 100 and the default log_prob at 2^18
for a D=16, C=0, E=16, [256]*3 model, on the two-network kernel and on the generic route (torch evaluates the two
networks, the library steps), HIP events after a warm-up.  FLOP/s count the reference's MACs (layer-1 inputs D + C + E,
not the zero blocks of the pack); the share of the fp32 MFMA peak (157.3 TFLOP/s) is end-to-end.

Then the small-batch lines (``python scratch/symplectic_bench.py small`` prints only these): cooperative twin against
one-wavefront kernel (FF_COOP=1 / 0, alternating in this process, median and range of the repeats) for [256]*3 and
[128]*3 models -- sample with num_steps 1 and 100 from 256 samples to one round plus a tail, the default log_prob at
2,048 and 50,000 points -- beside what the launcher picks on its own (ff_mlp_launch_kind)."""
import copy
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from flowfusion_amd import _native  # noqa: E402
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP  # noqa: E402

PEAK = 157.3e12
D, C, E, UNITS = 16, 0, 16, [256] * 3
MACS = 2 * ((D + C + E) * UNITS[0] + sum(a * b for a, b in zip(UNITS[:-1], UNITS[1:])) + UNITS[-1] * D)


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / 1e3)
    return best


def main():
    torch.manual_seed(0)
    fm = SymplecticFlowModel(SymplecticMLP(D, C, E, UNITS), torch.randn(D), torch.rand(D) + 0.5, None, None).cuda()
    gm = copy.deepcopy(fm)
    object.__setattr__(gm, "_fusable", lambda: False)          # the generic route on the same model
    print(f"MACs per sample-evaluation (both networks): {MACS}; pair kernel: {_native.kernel_name(fm._net().plan(0))}")
    prior = torch.randn(1 << 20, 2 * D, device="cuda")
    x = torch.randn(1 << 18, D, device="cuda")
    p0 = torch.randn_like(x)
    for route, m in (("pair", fm), ("generic", gm)):
        for n in (1, 100):
            t = timed(lambda: m._sample_from(prior, None, n))
            flop = 2.0 * MACS * n * prior.shape[0]
            print(f"{route:8s} sample 2^20 num_steps={n:3d}: {t * 1e3:9.2f} ms  {prior.shape[0] * n / t:.3e} sample-evals/s  "
                  f"{flop / t / 1e12:6.1f} TFLOP/s = {flop / t / PEAK:.3f} of peak")
        t = timed(lambda: m._log_prob_from(x, p0))
        st = m.last_solver_stats
        evals = 6 * st["attempts"] + 2
        flop = 2.0 * MACS * evals * x.shape[0]
        print(f"{route:8s} log_prob 2^18 (dopri5, 1e-5): {t * 1e3:9.2f} ms  {st}  ~{evals} evals  "
              f"{flop / t / 1e12:6.1f} TFLOP/s = {flop / t / PEAK:.3f} of peak")


KINDS = {_native.LAUNCH_ONE_WAVE: "one-wave", _native.LAUNCH_TWIN: "twin", _native.LAUNCH_ONE_WAVE_AND_TWIN: "one-wave+twin"}


def alternating(fn, pins, reps=9):
    """ms of fn() under each environment of `pins` (name -> {var: value}), the environments taking turns rep by rep."""
    times = {k: [] for k in pins}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for name, env in pins.items():
            os.environ.update(env)
            try:
                torch.cuda.synchronize()
                s.record()
                fn()
                e.record()
                torch.cuda.synchronize()
            finally:
                for k in env:
                    del os.environ[k]
            if r:                                             # (the first turn is the warm-up)
                times[name].append(s.elapsed_time(e))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def small_batches():
    fmt = lambda t: f"{t[0]:8.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"
    for width, chip in ((256, 2048), (128, 3072)):
        torch.manual_seed(0)
        fm = SymplecticFlowModel(SymplecticMLP(D, C, E, [width] * 3), torch.randn(D), torch.rand(D) + 0.5, None, None).cuda()
        plan = fm._net().plan(0)
        tail = chip * 16 + (300 if width == 256 else 120)
        print(f"\n[{width}] {_native.kernel_name(plan)}; chip = {chip} tiles of 16 samples")
        for n in (1, 100):
            # (100 steps: every 128 or 256 tiles up to a chip's worth -- the curve the launcher's rule is checked against)
            sizes = (256, 2048, 8192, 16384) if n == 1 else \
                (256, 2048, 4096, 6144, 8192, 10240, 12288, 14336, 16384) + tuple(range(20480, chip * 16 + 1, 4096))
            for B in sizes + (tail,):
                prior = torch.randn(B, 2 * D, device="cuda")
                pick = KINDS[_native.launch_kind(plan, B, 0)]
                if B == tail:
                    r = alternating(lambda: fm._sample_from(prior, None, n), {"whole": {"FF_TAIL_SPLIT": "0"}, "split": {"FF_TAIL_SPLIT": "1"}})
                    print(f"[{width}] sample B={B:6d} num_steps={n:3d}: one-wave {fmt(r['whole'])}  rounds + twin tail {fmt(r['split'])}  "
                          f"ratio {r['whole'][0] / r['split'][0]:.2f}  default: {pick}")
                else:
                    r = alternating(lambda: fm._sample_from(prior, None, n), {"one": {"FF_COOP": "0"}, "twin": {"FF_COOP": "1"}})
                    print(f"[{width}] sample B={B:6d} num_steps={n:3d}: one-wave {fmt(r['one'])}  twin {fmt(r['twin'])}  "
                          f"ratio {r['one'][0] / r['twin'][0]:.2f}  default: {pick}")
        for B in (2048, 50000):
            x = torch.randn(B, D, device="cuda")
            p0 = torch.randn_like(x)
            stats = {}

            def run():
                fm._log_prob_from(x, p0)
                stats[os.environ.get("FF_COOP", "rule")] = (fm.last_solver_stats["attempts"], fm.last_solver_stats["accepted"])
            r = alternating(run, {"one": {"FF_COOP": "0", "FF_TAIL_SPLIT": "0"}, "twin": {"FF_COOP": "1"}, "rule": {"FF_TAIL_SPLIT": "1"}})
            print(f"[{width}] log_prob B={B:6d} (dopri5, 1e-5): one-wave {fmt(r['one'])}  twin {fmt(r['twin'])}  "
                  f"launcher's choice ({KINDS[_native.launch_kind(plan, B, 0)]}) {fmt(r['rule'])}  "
                  f"ratio one-wave / choice {r['one'][0] / r['rule'][0]:.2f}  attempts/accepted {stats}")


if __name__ == "__main__":
    if "small" not in sys.argv[1:]:
        main()
    small_batches()
