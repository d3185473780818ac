"""Cost of the flow-map sensitivities: python scratch/pushforward_bench.py PARENT_LIB

PARENT_LIB = libflowfusion_amd.so built from the parent commit.  The 2^16 x 16-d 4 x 256 VP score model, 100-step rk4.

1. A K-tangent push-forward launch (ff_mlp_ode_launch_push, mlp_push_m16_h256_d4_c4_w2) against the parent's num_probes = K
   Hutchinson launch (ff_mlp_ode_launch, FF_MODE_HUTCH, tangent_count = K) on the same rows and grid, K = 1 / 7 / 15: one
   launch through the C ABI per timing, HIP events, the two contenders alternating in one process, a warm-up turn, median
   [min, max] of 9.  Also checks that both return the same state bit for bit.
2. flow_jacobian (two launches: 15 + 1 unit tangents) against forward-mode torch on the device: the same rk4 steps written
   in torch over ScoreModel.ode_drift, differentiated by vmap(jvp) over the 16 unit directions -- what torch.func.jacfwd
   composes -- at 2^12 rows (torch holds 16 x the batch in every activation)."""
import ctypes
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import _native                                    # noqa: E402
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd import solvers                                    # noqa: E402
from flowfusion_amd.fused import MODE_HUTCH                           # noqa: E402

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


def main(parent_path):
    parent = ctypes.CDLL(str(Path(parent_path).resolve()))
    parent.ff_mlp_ode_launch.restype = ctypes.c_int
    parent.ff_mlp_ode_launch.argtypes = [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs), ctypes.c_void_p]
    this = _native.lib()
    torch.manual_seed(0)
    sm = D.ScoreModel(D.MLP(DIM, 0, 8, [256] * 4), D.VPSDE(), no_sigma=True, hutchinson=True).eval().to("cuda")
    net = sm._net()
    hutch, push = net.plan(MODE_HUTCH), net.push_plan()
    eps = float(sm.sde.epsilon)
    t_span, opts = torch.tensor([eps, 1.0]), {"step_size": (1.0 - eps) / STEPS}
    tab = sm._ode_table(t_span, "rk4", opts, MODE_HUTCH).to("cuda").contiguous()
    assert hutch.width == push.width                       # one table serves both
    dev = torch.device("cuda", torch.cuda.current_device())
    wh, wp = net.wpack(dev, MODE_HUTCH), net.wpack(dev, MODE_HUTCH, push)
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    print(f"# parent: {_native.kernel_name(hutch)}; this: {_native.kernel_name(push)}; B = {B}, rows = {tab.shape[0]}")
    for K in (1, 7, 15):
        probes = _native.probe_fill(B, K, DIM, 5, 0, x.device, scale=K ** -0.5)
        outs = {}

        def launch(name):
            x_out = torch.empty_like(x)
            a = _native.OdeArgs()
            a.x_in, a.x_out, a.probe = x.data_ptr(), x_out.data_ptr(), probes.data_ptr()
            a.etab = tab.data_ptr()
            a.batch, a.n_evals, a.mode, a.tangent_count, a.stage_slots = B, tab.shape[0], MODE_HUTCH, K, 4
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if name == "parent":
                dl = torch.zeros(B, device="cuda")
                a.wpack, a.dlogp_out = wh.data_ptr(), dl.data_ptr()
                rc = parent.ff_mlp_ode_launch(ctypes.byref(hutch), ctypes.byref(a), stream)
                outs[name] = (x_out, dl)
            else:
                t_out = torch.empty(B, K, DIM, device="cuda")
                a.wpack = wp.data_ptr()
                rc = this.ff_mlp_ode_launch_push(ctypes.byref(push), ctypes.byref(a), None, t_out.data_ptr(), stream)
                outs[name] = (x_out, t_out)
            assert rc == 0, (name, rc)

        times = timed({"parent": lambda: launch("parent"), "push": lambda: launch("push")})
        assert torch.equal(outs["parent"][0], outs["push"][0])
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(times["parent"]) - min(times["parent"])
        print(f"K = {K:2d}  parent hutch {med['parent']:9.3f} ms [{min(times['parent']):.3f}, {max(times['parent']):.3f}]   "
              f"push {med['push']:9.3f} ms [{min(times['push']):.3f}, {max(times['push']):.3f}]   "
              f"{100 * (med['push'] - med['parent']) / med['parent']:+.3f} % of the parent's median; parent's own spread "
              f"{spread:.3f} ms ({100 * spread / med['parent']:.3f} %); states bitwise equal")
    # ---- the whole Jacobian against forward-mode torch ----
    Bj = 1 << 12
    xj = x[:Bj].contiguous()
    grid = solvers.fixed_grid(t_span, opts["step_size"]).to("cuda")

    def torch_map(y):
        for t0, t1 in zip(grid[:-1], grid[1:]):
            dt = t1 - t0
            f = lambda t, s: sm.ode_drift(t, s)
            k1 = f(t0, y)
            k2 = f(t0 + dt / 3, y + dt * k1 / 3)
            k3 = f(t0 + dt * 2 / 3, y + dt * (k2 - k1 / 3))
            k4 = f(t1, y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        return y

    basis = torch.eye(DIM, device="cuda")[:, None, :].expand(DIM, Bj, DIM).contiguous()
    outs = {}

    def torch_jac():
        with torch.no_grad():
            cols = torch.func.vmap(lambda v: torch.func.jvp(torch_map, (xj,), (v,))[1])(basis)      # [D, B, D]
        outs["torch"] = cols.permute(1, 2, 0)

    def ours():
        outs["ours"] = sm.flow_jacobian(xj, direction="to_base", method="rk4", options=opts)[1]

    times = timed({"torch": torch_jac, "ours": ours}, turns=4)
    med = {k: statistics.median(v) for k, v in times.items()}
    err = float((outs["ours"] - outs["torch"]).abs().max() / outs["torch"].abs().max())
    print(f"flow_jacobian, B = {Bj}: forward-mode torch {med['torch']:9.3f} ms, flow_jacobian {med['ours']:9.3f} ms "
          f"({med['torch'] / med['ours']:.1f} x); max |difference| / max |J| {err:.2e}")


if __name__ == "__main__":
    main(sys.argv[1])
