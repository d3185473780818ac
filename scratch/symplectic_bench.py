"""Symplectic flow timing (not a test): sample at 2^20 samples with num_steps 1 and 100 and the default log_prob at 2^18
for a D=16, C=0, E=16, [256]*3 model, on the two-network kernel and on the generic route (torch evaluates the two
networks, the library steps), HIP events after a warm-up.  FLOP/s count the reference's MACs (layer-1 inputs D + C + E,
not the zero blocks of the pack); the share of the fp32 MFMA peak (157.3 TFLOP/s) is end-to-end."""
import copy
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


if __name__ == "__main__":
    main()
