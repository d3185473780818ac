"""Cost of the flow-map pull-backs: python scratch/pullback_bench.py [one K STEPS]

The 2^16 x 16-d 4 x 256 VP score model, 100-step rk4, direction to_base (the parent's push-forward benchmark's model).

1. ``flow_vjp`` at K = 1 / 3 / 7 / 15 cotangents per sample -- the state-only forward solve plus ONE pull launch
   (mlp_pull_m16_h256_d4_c4) -- against the parent's only route to ``w^T d x_out / d x``: ``flow_jacobian`` (two push launches,
   15 + 1 unit tangents) plus the contraction with ``w``.  HIP events, the contenders alternating in one process, a warm-up
   turn, median [min, max] of 9.  The pull launch alone is timed too (raw, through FusedNet.pullback), and its share of the
   MFMA pipe worked out from the MFMA count: per evaluation row net A and net B issue 3264 + 3264 MFMAs of 32 cycles each on
   one SIMD; the chip has 1024 SIMDs at CLOCK_GHZ.  Wavefronts per CU: what the tile's LDS leaves of the CU's 160 KiB, and at
   most one per SIMD (the 256-wide unit takes 364 of a SIMD's 512 registers).
2. The two routes differ by the discretisation error, not by rounding: the largest difference is printed with the retrace.

``one K STEPS``: a single pull launch of K cotangents over STEPS rk4 steps and nothing else, for a counter run
(rocprofv3 --pmc ... -- python scratch/pullback_bench.py one 1 10)."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import _native                                    # noqa: E402
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd import solvers                                    # noqa: E402

B, DIM, STEPS = 1 << 16, 16, 100
CLOCK_GHZ, SIMDS, MFMA_CYCLES = 2.4, 1024, 32
MFMAS_PER_ROW = 2 * 3264               # layer 1: 2 groups x 8 blocks x 4 x 2 = 128; hidden 3 x 16 x 8 x 8 = 3072; output 16 x 4 = 64


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


def setup(steps):
    torch.manual_seed(0)
    sm = D.ScoreModel(D.MLP(DIM, 0, 8, [256] * 4), D.VPSDE(), no_sigma=True).eval().to("cuda")
    eps = float(sm.sde.epsilon)
    opts = {"step_size": (1.0 - eps) / steps}
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    return sm, opts, x


def pull_alone(sm, opts, y, w):
    """The pull launch of flow_vjp(direction="to_base") by itself: (callable, rows of its table)."""
    net = sm._net()
    plan = net.pull_plan()
    eps = float(sm.sde.epsilon)
    tab = solvers.plan_ode(torch.tensor([1.0, eps]), "rk4", opts)
    table = solvers.build_table(tab, *sm._host_schedule()(tab.t_eval), int(plan.width)).to("cuda")
    return (lambda: net.pullback(y, table, w, stage_slots=4)), table.shape[0], _native.kernel_name(plan)


def main():
    sm, opts, x = setup(STEPS)
    kw = dict(direction="to_base", method="rk4", options=opts)
    y = sm.flow_vjp(x[:64], torch.ones(64, 1, DIM, device="cuda"), **kw)[0]          # (builds and caches packs and tables)
    print(f"# B = {B}, {DIM}-d, 4 x 256, VP, {STEPS}-step rk4 = {4 * STEPS} rows; clock taken as {CLOCK_GHZ} GHz")
    outs = {}

    def jac_route(w):
        yj, J, _ = sm.flow_jacobian(x, **kw)
        outs["jac"] = torch.einsum("bki,bij->bkj", w, J)

    for K in (1, 3, 7, 15):
        w = torch.randn(B, K, DIM, device="cuda")
        yT = sm.flow_vjp(x, w, **kw)[0]
        alone, rows, name = pull_alone(sm, opts, yT, w)

        def vjp_route():
            outs["vjp"] = sm.flow_vjp(x, w, return_retrace=True, **kw)

        times = timed({"jacobian": lambda: jac_route(w), "flow_vjp": vjp_route, "pull": alone})
        med = {k: statistics.median(v) for k, v in times.items()}
        rng = {k: f"[{min(v):.1f}, {max(v):.1f}]" for k, v in times.items()}
        tiles = -(-B // (16 // (1 + K)))
        share = tiles * rows * MFMAS_PER_ROW * MFMA_CYCLES / (med["pull"] * 1e-3 * CLOCK_GHZ * 1e9 * SIMDS)
        lds = 4 * 8 * 256 + (16 // (1 + K)) * 4 * 256 * 4          # rk4's four stage slots of 8 words, then the stash
        gx, retrace = outs["vjp"][1], outs["vjp"][3]
        gap = float((gx - outs["jac"]).abs().max() / outs["jac"].abs().max())
        print(f"K = {K:2d}  jacobian + contraction {med['jacobian']:9.1f} ms {rng['jacobian']}   flow_vjp {med['flow_vjp']:9.1f} ms "
              f"{rng['flow_vjp']}  ({med['jacobian'] / med['flow_vjp']:.2f} x)   pull launch alone ({name}) {med['pull']:9.1f} ms "
              f"{rng['pull']}: {tiles} tiles, LDS {lds / 1024:.0f} KiB per tile = {min(160 * 1024 // lds, 4)} wavefronts per CU, MFMA-pipe "
              f"share {100 * share:.1f} %;  routes differ by {gap:.2e} of max |w^T J|, retrace max {float(retrace.max()):.2e}")


def one(K, steps):
    sm, opts, x = setup(steps)
    w = torch.randn(B, K, DIM, device="cuda")
    y = sm.flow_vjp(x, w, direction="to_base", method="rk4", options=opts)[0]
    alone, rows, name = pull_alone(sm, opts, y, w)
    alone()
    torch.cuda.synchronize()
    print(f"one pull launch: {name}, K = {K}, {rows} rows, {-(-B // (16 // (1 + K)))} tiles")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "one":
        one(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
