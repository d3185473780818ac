"""The five 32-column units whose register allocation moved with the longer argument block (profiles/pushforward_resources.txt),
timed against the parent's:  python scratch/pushforward_units_bench.py PARENT_LIB

PARENT_LIB = libflowfusion_amd.so built from the parent commit.  One ff_mlp_ode_launch per timing on the same plan, weights,
table and rows through either library; VP score models, 2^18 rows, 50-step rk4; HIP events, the two libraries alternating
in one process, a warm-up turn, median [min, max] of 9.  Also checks that both return the same bits."""
import ctypes
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import _native                                    # noqa: E402
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd.fused import MODE_HUTCH, MODE_STATE               # noqa: E402

B, STEPS = 1 << 18, 50
# (kernel expected, dim, cond_dim, units, mode)
UNITS = [
    ("mlp_ode_m32_h128_d16_c0_t0", 32, 0, [128] * 3, MODE_STATE),
    ("mlp_ode_m32_h128_d16_c0_t1", 32, 0, [128] * 3, MODE_HUTCH),
    ("mlp_ode_m32_h64_d16_c0_t0", 32, 0, [64, 64], MODE_STATE),
    ("mlp_ode_m32_h64_d8_c8_t0", 16, 8, [64, 64], MODE_STATE),
    ("mlp_ode_m32_h64_d8_c8_t1", 16, 8, [64, 64], MODE_HUTCH),
]


def main(parent_path):
    libs = {"parent": ctypes.CDLL(str(Path(parent_path).resolve())), "this": _native.lib()}
    for lib in libs.values():
        lib.ff_mlp_ode_launch.restype = ctypes.c_int
        lib.ff_mlp_ode_launch.argtypes = [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs), ctypes.c_void_p]
    dev = torch.device("cuda", torch.cuda.current_device())
    for want, dim, cdim, units, mode in UNITS:
        torch.manual_seed(0)
        sm = D.ScoreModel(D.MLP(dim, cdim, 8, units), D.VPSDE(), no_sigma=True, hutchinson=mode == MODE_HUTCH).eval().to("cuda")
        net = sm._net()
        plan = net.plan(mode)
        assert _native.kernel_name(plan) == want, (_native.kernel_name(plan), want)
        eps = float(sm.sde.epsilon)
        tab = sm._ode_table(torch.tensor([eps, 1.0]), "rk4", {"step_size": (1.0 - eps) / STEPS}, mode).to("cuda").contiguous()
        wpack = net.wpack(dev, mode)
        x = (torch.randn(B, dim) * 0.8 + 0.3).to("cuda")
        cond = torch.randn(B, cdim).to("cuda") if cdim else None
        probe = torch.sign(torch.randn(B, dim)).to("cuda") if mode == MODE_HUTCH else None
        outs, times = {}, {k: [] for k in libs}
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(10):                       # the first turn warms up
            for k, lib in libs.items():
                x_out, dl = torch.empty_like(x), torch.zeros(B, device="cuda")
                a = _native.OdeArgs()
                a.x_in, a.x_out, a.wpack, a.etab = x.data_ptr(), x_out.data_ptr(), wpack.data_ptr(), tab.data_ptr()
                a.cond = 0 if cond is None else cond.data_ptr()
                if mode == MODE_HUTCH:
                    a.probe, a.dlogp_out = probe.data_ptr(), dl.data_ptr()
                a.batch, a.n_evals, a.mode, a.stage_slots = B, tab.shape[0], mode, 4
                torch.cuda.synchronize()
                s.record()
                rc = lib.ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                e.record()
                torch.cuda.synchronize()
                assert rc == 0, (k, rc)
                outs[k] = (x_out, dl)
                if r:
                    times[k].append(s.elapsed_time(e))
        assert torch.equal(outs["parent"][0], outs["this"][0]) and torch.equal(outs["parent"][1], outs["this"][1]), want
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(times["parent"]) - min(times["parent"])
        print(f"{want:30s} parent {med['parent']:8.3f} ms [{min(times['parent']):.3f}, {max(times['parent']):.3f}]   "
              f"this {med['this']:8.3f} ms [{min(times['this']):.3f}, {max(times['this']):.3f}]   "
              f"{100 * (med['this'] - med['parent']) / med['parent']:+.3f} %; parent's own spread {100 * spread / med['parent']:.3f} %; "
              f"same bits", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
