"""Row-select kernel timing (not a test): leapfrog on the select kernel against Euler / dopri5 on the pair kernel.

HIP events, the contenders taking turns in one process, median and range of 9 repeats after a warm-up turn.

1. Throughput: D = 16, [256]*3, 2^20 rows, 100 steps -- leapfrog (201 single-network rows) against Euler (100 two-network
   rows; the pair kernel's ISA is the parent commit's, instruction for instruction).  Work ratio 201 / 200.  The share of
   the fp32 MFMA peak (157.3 TFLOP/s) counts the EXECUTED multiply-adds: the zero-padded on-chip shapes.
2. Twin crossover: leapfrog, 100 steps, 256 .. 16,384 rows and one round + a tail, widths 256 and 128: cooperative twin
   against one-wavefront kernel (FF_COOP=1 / 0), and what the launcher's rule picks (ff_mlp_launch_kind).
3. log_prob latency: 2,048 and 50,000 points, widths 256 and 128: method="leapfrog", num_steps=100 against the default
   dopri5, with the solver's own counts."""
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from flowfusion_amd import _native  # noqa: E402
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP  # noqa: E402

PEAK = 157.3e12
D, C, E = 16, 0, 16
KINDS = {_native.LAUNCH_ONE_WAVE: "one-wave", _native.LAUNCH_TWIN: "twin", _native.LAUNCH_ONE_WAVE_AND_TWIN: "one-wave+twin"}
fmt = lambda t: f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def alternating(jobs, reps=9):
    """ms of every job of `jobs` (name -> (fn, environment)), the jobs taking turns rep by rep; the first turn warms up."""
    times = {k: [] for k in jobs}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        for name, (fn, env) in jobs.items():
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
            if r:
                times[name].append(s.elapsed_time(e))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def model(width):
    torch.manual_seed(0)
    return SymplecticFlowModel(SymplecticMLP(D, C, E, [width] * 3), torch.randn(D), torch.rand(D) + 0.5, None, None).cuda()


def executed_macs(plan):
    """Multiply-adds of ONE network per sample as the kernel runs it: layer 1 over the state and conditional registers'
    columns, the hidden layers at the on-chip width, the output layer's blocks of 32 rows."""
    per_reg = 64 // plan.tile
    k1 = (plan.dregs + plan.cregs) * per_reg
    out_rows = -(-(plan.dregs * per_reg) // 32) * 32
    return k1 * plan.width + (plan.n_hidden - 1) * plan.width ** 2 + plan.width * out_rows


def throughput():
    fm = model(256)
    sel, pair = fm._net().plan(0, select=True), fm._net().plan(0)
    B, n = 1 << 20, 100
    grid = torch.linspace(1.0, 0.0, n + 1)
    z = torch.randn(B, 2 * D, device="cuda")
    print(f"[throughput] {_native.kernel_name(sel)} against {_native.kernel_name(pair)}; B = 2^20, {n} steps")
    r = alternating({"leapfrog": (lambda: fm._integrate(z, grid, None, "leapfrog"), {}),
                     "euler": (lambda: fm._integrate(z, grid, None, "euler"), {})})
    macs = executed_macs(sel)
    for name, rows_nets in (("leapfrog", 2 * n + 1), ("euler", 2 * n)):
        flop = 2.0 * macs * rows_nets * B
        t = r[name][0] / 1e3
        print(f"[throughput] {name:8s} {fmt(r[name])}  {rows_nets} network evaluations per row of the batch  "
              f"{flop / t / 1e12:6.1f} TFLOP/s executed = {flop / t / PEAK:.3f} of the fp32 MFMA peak")
    print(f"[throughput] leapfrog / euler = {r['leapfrog'][0] / r['euler'][0]:.4f} (work ratio 201 / 200 = {201 / 200:.4f})")


def crossover():
    for width, chip in ((256, 2048), (128, 3072)):
        fm = model(width)
        plan = fm._net().plan(0, select=True)
        grid = torch.linspace(1.0, 0.0, 101)
        tail = chip * 16 + (300 if width == 256 else 120)
        print(f"\n[{width}] {_native.kernel_name(plan)}; chip = {chip} tiles of 16 rows; leapfrog, 100 steps")
        for B in (256, 2048, 4096, 6144, 8192, 10240, 12288, 14336, 16384, tail):
            z = torch.randn(B, 2 * D, device="cuda")
            pick = KINDS[_native.launch_kind(plan, B, 0)]
            run = lambda: fm._integrate(z, grid, None, "leapfrog")
            if B == tail:
                r = alternating({"whole": (run, {"FF_TAIL_SPLIT": "0"}), "split": (run, {"FF_TAIL_SPLIT": "1"})})
                print(f"[{width}] B={B:6d}: one-wave {fmt(r['whole'])}  rounds + twin tail {fmt(r['split'])}  "
                      f"ratio {r['whole'][0] / r['split'][0]:.2f}  default: {pick}")
            else:
                r = alternating({"one": (run, {"FF_COOP": "0"}), "twin": (run, {"FF_COOP": "1"})})
                print(f"[{width}] B={B:6d}: one-wave {fmt(r['one'])}  twin {fmt(r['twin'])}  "
                      f"ratio {r['one'][0] / r['twin'][0]:.2f}  default: {pick}")


def log_prob_latency():
    for width in (256, 128):
        fm = model(width)
        for B in (2048, 50000):
            x = torch.randn(B, D, device="cuda")
            p0 = torch.randn_like(x)
            stats = {}

            def lf():
                fm._log_prob_from(x, p0, method="leapfrog", num_steps=100)
                stats["leapfrog"] = dict(fm.last_solver_stats)

            def dp():
                fm._log_prob_from(x, p0)
                stats["dopri5"] = dict(fm.last_solver_stats)
            r = alternating({"leapfrog": (lf, {}), "dopri5": (dp, {})})
            print(f"[{width}] log_prob B={B:6d}: leapfrog(100) {fmt(r['leapfrog'])}  dopri5(1e-5) {fmt(r['dopri5'])}  "
                  f"ratio dopri5 / leapfrog {r['dopri5'][0] / r['leapfrog'][0]:.2f}\n        leapfrog {stats['leapfrog']}\n        dopri5   {stats['dopri5']}")


if __name__ == "__main__":
    throughput()
    crossover()
    print()
    log_prob_latency()
