"""Cost of the per-probe Hutchinson output (ff_mlp_ode_launch_probes): python scratch/hutch_probe_out_bench.py PARENT_LIB

PARENT_LIB = libflowfusion_amd.so built from the parent commit.  The 2^16 x 16-d 4 x 256 score model, 100-step rk4, K = 7
(mlp_ode_m16_h256_d4_c0_t1_w2, two samples per tile), one launch through the C ABI per timing; HIP events, the three
contenders alternating in one process, a warm-up turn, median [min, max] of 9:
    parent          ff_mlp_ode_launch of the parent commit's library
    this, NULL      ff_mlp_ode_launch_probes of this library with dlogp_probe_out = NULL
    this, set       the same with the [B, K] output
Also checks that the three launches return the same state and dlogp bit for bit."""
import ctypes
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from flowfusion_amd import _native                                    # noqa: E402
from flowfusion_amd import diffusion as D                             # noqa: E402
from flowfusion_amd.fused import MODE_HUTCH                           # noqa: E402

B, DIM, K, STEPS = 1 << 16, 16, 7, 100


def main(parent_path):
    parent = ctypes.CDLL(str(Path(parent_path).resolve()))
    parent.ff_mlp_ode_launch.restype = ctypes.c_int
    parent.ff_mlp_ode_launch.argtypes = [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs), ctypes.c_void_p]
    this = _native.lib()
    torch.manual_seed(0)
    sm = D.ScoreModel(D.MLP(DIM, 0, 8, [256] * 4), D.VPSDE(), no_sigma=True, hutchinson=True).eval().to("cuda")
    net = sm._net()
    plan = net.plan(MODE_HUTCH)
    eps = float(sm.sde.epsilon)
    tab = sm._ode_table(torch.tensor([eps, 1.0]), "rk4", {"step_size": (1.0 - eps) / STEPS}, MODE_HUTCH).to("cuda").contiguous()
    wpack = net.wpack(torch.device("cuda", torch.cuda.current_device()), MODE_HUTCH)
    x = (torch.randn(B, DIM) * 0.8 + 0.3).to("cuda")
    probes = _native.probe_fill(B, K, DIM, 5, 0, x.device, scale=K ** -0.5)
    print(f"# {_native.kernel_name(plan)}, B = {B}, K = {K}, rows = {tab.shape[0]}, "
          f"launch kind {_native.launch_kind(plan, B, MODE_HUTCH, K)} (0 = one-wavefront kernel)")
    outs = {}

    def launch(name):
        x_out, dl = torch.empty_like(x), torch.zeros(B, device="cuda")
        d = torch.zeros(B, K, device="cuda") if name == "this, set" else None
        a = _native.OdeArgs()
        a.x_in, a.x_out, a.probe, a.dlogp_out = x.data_ptr(), x_out.data_ptr(), probes.data_ptr(), dl.data_ptr()
        a.wpack, a.etab = wpack.data_ptr(), tab.data_ptr()
        a.batch, a.n_evals, a.mode, a.tangent_count, a.stage_slots = B, tab.shape[0], MODE_HUTCH, K, 4
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if name == "parent":
            rc = parent.ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), stream)
        else:
            rc = this.ff_mlp_ode_launch_probes(ctypes.byref(plan), ctypes.byref(a), None if d is None else d.data_ptr(), stream)
        assert rc == 0, (name, rc)
        outs[name] = (x_out, dl, d)

    names = ("parent", "this, NULL", "this, set")
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in names}
    for r in range(10):                           # the first turn warms up
        for k in names:
            torch.cuda.synchronize()
            s.record()
            launch(k)
            e.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(s.elapsed_time(e))
    for k in names[1:]:
        assert torch.equal(outs[k][0], outs["parent"][0]) and torch.equal(outs[k][1], outs["parent"][1]), k
    d = outs["this, set"][2]
    print(f"# state and dlogp of the three launches: bitwise equal; |row sums of the output - dlogp| max "
          f"{float((d.double().sum(1) - outs['parent'][1].double()).abs().max()):.3g} (|dlogp| max {float(outs['parent'][1].abs().max()):.3g})")
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in names:
        print(f"{k:12s} {med[k]:9.3f} ms [{min(times[k]):.3f}, {max(times[k]):.3f}]   {100 * (med[k] - med['parent']) / med['parent']:+.3f} % of the parent's median")
    spread = max(times["parent"]) - min(times["parent"])
    print(f"parent's own spread over its 9 repeats: {spread:.3f} ms ({100 * spread / med['parent']:.3f} %)")
    for k in names[1:]:
        inside = min(times["parent"]) <= med[k] <= max(times["parent"])
        print(f"{k}: median {'inside' if inside else 'OUTSIDE'} the parent's [min, max]")


if __name__ == "__main__":
    main(sys.argv[1])
