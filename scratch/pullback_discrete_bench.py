"""Cost of the exact discrete adjoint: python scratch/pullback_discrete_bench.py [Ks]

The 2^16 x 16-d 4 x 256 VP score model, 100-step rk4, direction to_base (scratch/pullback_bench.py's model and grid).

``flow_vjp(adjoint="discrete")`` at K = 1 / 3 / 7 / 15 cotangents per sample -- per piece of rows one record launch
(mlp_rec_m16_h256_d4_c4) and one discrete-adjoint launch (mlp_dadj_m16_h256_d4_c4) over the same forward table -- against the
continuous ``flow_vjp`` (the default route: the state-only solve plus one pull launch) and against ``flow_jacobian`` plus the
contraction with ``w``, in the same run.  HIP events, the contenders alternating in one process, a warm-up turn, median
[min, max] of 9.  The two launches of the discrete route are also timed alone (raw, through FusedNet.record /
FusedNet.pullback_discrete, on the first piece of rows the front end cuts), and the record's traffic is printed: n_evals x B x D
floats written by the first and read by the second.  The largest differences between the three results are printed too: the
discrete route against ``w^T J`` is rounding, the continuous one the discretisation error."""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd import odeint, solvers                            # noqa: E402

B, DIM, STEPS = 1 << 16, 16, 100


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


def main(Ks):
    torch.manual_seed(0)
    sm = D.ScoreModel(D.MLP(DIM, 0, 8, [256] * 4), D.VPSDE(), no_sigma=True).eval().to("cuda")
    eps = float(sm.sde.epsilon)
    opts = {"step_size": (1.0 - eps) / STEPS}
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    kw = dict(direction="to_base", method="rk4", options=opts)
    for adjoint in ("continuous", "discrete"):                            # (builds and caches packs and tables)
        sm.flow_vjp(x[:64], torch.ones(64, 1, DIM, device="cuda"), adjoint=adjoint, **kw)
    net = sm._net()
    plan = net.pull_plan()
    tab = solvers.plan_ode(torch.tensor([eps, 1.0]), "rk4", opts)
    table = solvers.build_table(tab, *sm._host_schedule()(tab.t_eval), int(plan.width)).to("cuda")
    E = int(table.shape[0])
    print(f"# B = {B}, {DIM}-d, 4 x 256, VP, {STEPS}-step rk4 = {E} rows; record {E * B * DIM * 4 / 1e9:.2f} GB each way per call")
    solo = sm.flow_vjp(x, torch.ones(B, 1, DIM, device="cuda"), **kw)[0]
    outs = {}
    for K in Ks:
        w = torch.randn(B, K, DIM, device="cuda")
        rows = min(B, odeint.discrete_piece_rows(B, K, E, DIM))                            # the front end's first piece
        xp, wp = x[:rows].contiguous(), w[:rows].contiguous()
        _, rec, _ = net.record(xp, table, stage_slots=4)

        def jac_route():
            _, J, _ = sm.flow_jacobian(x, **kw)
            outs["jac"] = torch.einsum("bki,bij->bkj", w, J)

        def cont_route():
            outs["cont"] = sm.flow_vjp(x, w, **kw)

        def disc_route():
            outs["disc"] = sm.flow_vjp(x, w, adjoint="discrete", **kw)

        times = timed({"jacobian": jac_route, "continuous": cont_route, "discrete": disc_route,
                       "record": lambda: net.record(xp, table, stage_slots=4),
                       "backward": lambda: net.pullback_discrete(rec, table, wp, stage_slots=4)})
        med = {k: statistics.median(v) for k, v in times.items()}
        rng = {k: f"[{min(v):.1f}, {max(v):.1f}]" for k, v in times.items()}
        scale = float(outs["jac"].abs().max())
        gap_d = float((outs["disc"][1] - outs["jac"]).abs().max()) / scale
        gap_c = float((outs["cont"][1] - outs["jac"]).abs().max()) / scale
        pieces = -(-B // rows)
        print(f"K = {K:2d}  jacobian + contraction {med['jacobian']:8.1f} ms {rng['jacobian']}   continuous flow_vjp "
              f"{med['continuous']:8.1f} ms {rng['continuous']}   discrete flow_vjp {med['discrete']:8.1f} ms {rng['discrete']}  "
              f"({med['discrete'] / med['continuous']:.2f} x the continuous route, {med['jacobian'] / med['discrete']:.2f} x faster than "
              f"the jacobian route)   per piece of {rows} rows ({pieces} pieces): record launch {med['record']:7.1f} ms {rng['record']}, "
              f"backward launch {med['backward']:8.1f} ms {rng['backward']};  against w^T J: discrete {gap_d:.2e}, continuous "
              f"{gap_c:.2e} of max |w^T J|;  x_out bitwise the state-only solve: {torch.equal(outs['disc'][0], solo)}")
        del rec


if __name__ == "__main__":
    main([int(k) for k in sys.argv[1:]] or [1, 3, 7, 15])
