"""Solver-frame refactor check (not a test): the product library against a library built from the PARENT commit.

    python scratch/frame_compare.py PARENT_LIB [bits] [time]

`bits`: the same seeded raw ff_mlp_ode_launch through both libraries, one instance of every kernel family of
ff_mlp_ode.hpp / ff_mlp_pair.hpp; x_out, dlogp_out, every aux_out / aux_lp_out and the status word compared as raw bytes.
Every launch: a last tile that is partly empty, dim below the register capacity, conditional inputs, input and output
affine maps, a table of six rows with two STEP_ENDs, two noise rows, a row naming slot 7 (so the bad-slot bit is set).
A launch takes its noise either from the caller's buffer or from the in-kernel generator (ff_ode_args.noise NULL or not),
so every state-only case runs once each way; the tangent kernels draw nothing in the kernel and run from the buffer only.
Each case runs with two and with three hidden layers (the twin's exchange buffer alternates both ways), plain and -- where
the launcher accepts them -- as an adaptive attempt (k1_in, kl1_in, dlogp_in, n_aux = 4).

`time`: both libraries and a byte copy of the parent library under a second file name (the noise floor) take turns in
one process through ff_mlp_ode_launch: HIP events, a warm-up turn, median of 9.  A case passes if
|this - parent| <= |parent copy - parent|, the gap that two loads of the SAME code show.

`probe`: the first case of `bits` with the features of the launch taken away one at a time, this library and the parent's
byte copy against the parent: where a mismatch comes from, and whether two loads of the same code agree at all."""
import ctypes
import os
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from flowfusion_amd import _native  # noqa: E402

DEV = "cuda"
HDR = 32
f32 = lambda t: t.to(DEV, torch.float32).contiguous()


class Net:
    """A seeded network of one kernel family: its plan in every library, packed weights, raw launches."""

    def __init__(self, name, dim, cond, hidden, mode=0, pair=False, select=False, coop=None, seed=0):
        self.name, self.dim, self.cond, self.hidden, self.mode = name, dim, cond, list(hidden), mode
        self.pair, self.select, self.coop = pair, select, coop
        g = torch.Generator().manual_seed(seed)
        self.g = g
        lin = lambda o, i: (torch.randn(o, i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1)
        widths = self.hidden
        state = dim // 2 if pair else dim             # a pair's networks read one half of the state each

        def layers():
            ins = [state + cond] + widths
            outs = widths + [state]
            return [lin(o, i) for o, i in zip(outs, ins)]
        if pair:
            q, p = layers(), layers()
            self.plan = _native.make_pair_plan(dim, cond, widths, select=select)
            mk = lambda ls: [torch.nn.Linear(w.shape[1], w.shape[0]) for w, _ in ls]
            ql, pl = mk(q), mk(p)
            for mods, ls in ((ql, q), (pl, p)):
                for m, (w, b) in zip(mods, ls):
                    m.weight.data.copy_(w)
                    m.bias.data.copy_(b)
            self.wpack = f32(_native.pack_pair_weights(self.plan, ql, pl, widths, 0, state))
        else:
            ls = layers()
            self.plan = _native.make_plan(dim, cond, widths, mode)
            self.wpack = f32(_native.pack_weights(self.plan, [w for w, _ in ls], [b for _, b in ls], widths, 0, dim))
        self.kernel = _native.kernel_name(self.plan)
        self.row_width = _native.row_width(self.plan)

    def plan_of(self, L):
        """The plan library `L` makes for this network: kernel ids are per library, the layout must be the product's."""
        p = _native.PlanStruct()
        arr = (ctypes.c_int * len(self.hidden))(*self.hidden)
        if self.pair:
            rc = (L.ff_mlp_pair_select_plan if self.select else L.ff_mlp_pair_plan)(self.dim, self.cond, len(arr), arr, ctypes.byref(p))
        else:
            prm = (ctypes.c_float * 2)(0.0, 0.0)
            rc = L.ff_mlp_plan_prec(self.dim, self.cond, len(arr), arr, self.mode, _native.ACT_SILU, prm, _native.PREC_F32, ctypes.byref(p))
        assert rc == 0, rc
        assert bytes(p) == bytes(self.plan), "the libraries plan this network differently"
        return p

    def table(self, rows):
        """`rows`: list of dicts (a, b, gn, flags, slot, noise_idx, cin, cout) -> device table with random c1 per row."""
        t = torch.zeros(len(rows), HDR + self.row_width)
        ints = t.view(torch.int32)
        for i, r in enumerate(rows):
            t[i, 0], t[i, 1], t[i, 2] = r.get("a", 0.0), r.get("b", 1.0), r.get("gn", 0.0)
            ints[i, 3], ints[i, 4], ints[i, 5] = r.get("flags", 0), r.get("slot", 0), r.get("noise_idx", 0)
            for s, v in enumerate(r.get("cin", ())):
                t[i, 8 + s] = v
            for s, v in enumerate(r.get("cout", ())):
                t[i, 16 + s] = v
        t[:, HDR:] = torch.randn(len(rows), self.row_width, generator=self.g) * 0.5
        return f32(t)

    def launch(self, L, x, table, n_evals, cond=None, probe=None, noise=None, rng=None, affine=None, attempt=None, status=True):
        """One raw launch through `L`; returns the output tensors (sentinel-filled where the kernel writes nothing)."""
        B, D = x.shape
        out = {"x_out": torch.full_like(x, -123.0), "status": torch.zeros(1, dtype=torch.int32, device=DEV)}
        a = _native.OdeArgs()
        a.x_in, a.x_out, a.wpack, a.etab = x.data_ptr(), out["x_out"].data_ptr(), self.wpack.data_ptr(), table.data_ptr()
        a.batch, a.n_evals, a.mode, a.stage_slots = B, n_evals, self.mode, 0
        if status:
            a.status = out["status"].data_ptr()
        if cond is not None:
            a.cond = cond.data_ptr()
        if self.mode:
            out["dlogp_out"] = torch.full((B,), -55.0, device=DEV)
            a.dlogp_out, a.probe = out["dlogp_out"].data_ptr(), probe.data_ptr()
        if noise is not None:
            a.noise, a.noise_stride = noise.data_ptr(), noise.shape[1] * noise.shape[2]
        if rng is not None:
            a.rng_seed, a.rng_sample_offset, a.rng_noise_base = rng
        if affine is not None:
            a.in_shift, a.in_scale, a.out_scale, a.out_shift = (0 if t is None else t.data_ptr() for t in affine)
        if attempt is not None:
            a.k1_in, a.n_aux = attempt["k1"].data_ptr(), 4
            out["aux_out"] = torch.full((4, B, D), -321.0, device=DEV)
            for j in range(4):
                a.aux_out[j] = out["aux_out"][j].data_ptr()
            if self.mode:
                a.kl1_in, a.dlogp_in = attempt["kl1"].data_ptr(), attempt["lp0"].data_ptr()
                out["aux_lp_out"] = torch.full((4, B), -77.0, device=DEV)
                for j in range(4):
                    a.aux_lp_out[j] = out["aux_lp_out"][j].data_ptr()
        old = os.environ.pop("FF_COOP", None)
        if self.coop is not None:
            os.environ["FF_COOP"] = "1" if self.coop else "0"
        try:
            rc = L.ff_mlp_ode_launch(ctypes.byref(self.plan_of(L)), ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        finally:
            os.environ.pop("FF_COOP", None)
            if old is not None:
                os.environ["FF_COOP"] = old
        return rc, out


def bit_rows(net, attempt):
    """Six rows: stage inputs from the slots filled so far, STEP_END on rows 2 and 5, noise on rows 1 and 4, row 3 names
    slot 7; a row of a select plan runs net B on rows 1, 2 and 4.  An attempt's rows leave slot 0 to k1_in.  Then the two
    coefficient rows of the auxiliary outputs (use_y of outputs 0 and 2)."""
    g, rows, base = net.g, [], (1 if attempt else 0)
    for i in range(6):
        r = {"a": float(torch.randn((), generator=g)) * 0.1, "b": 1.0, "slot": 7 if i == 3 else base + i,
             "cin": [float(v) for v in torch.randn(base + i, generator=g) * 0.1], "flags": 0}
        if i in (2, 5):
            r["flags"] |= 1
            r["cout"] = [float(v) for v in torch.randn(base + i + 1, generator=g) * 0.2]
        if i in (1, 4):
            r["flags"] |= 2
            r["noise_idx"], r["gn"] = (1 if i == 1 else 0), 0.3
        if net.select and i in (1, 2, 4):
            r["flags"] |= 4
        rows.append(r)
    for j in range(2):
        rows.append({"flags": 0b0101 if j == 0 else 0, "cin": [float(v) for v in torch.randn(7, generator=g) * 0.2],
                     "cout": [float(v) for v in torch.randn(7, generator=g) * 0.2]})
    return rows


def bit_cases():
    for nh in (2, 3):
        yield Net("256 state-only", 13, 3, [256] * nh, coop=False)
        yield Net("256 tangents (Hutchinson)", 13, 3, [256] * nh, mode=1, coop=False)
        yield Net("128 three-wavefront", 13, 3, [128] * nh, coop=False)
        yield Net("128 three-wavefront, tangents", 13, 3, [128] * nh, mode=1, coop=False)
        yield Net("64 32-column", 5, 3, [64] * nh, coop=False)
        yield Net("512", 40, 3, [512] * nh, coop=False)
        yield Net("256 cooperative twin", 13, 3, [256] * nh, coop=True)
        yield Net("256 cooperative twin, tangents", 13, 3, [256] * nh, mode=1, coop=True)
        yield Net("wide catch-all", 70, 20, [1024] * nh)
        yield Net("wide catch-all, tangents", 70, 20, [1024] * nh, mode=1)
        yield Net("pair 256", 26, 3, [256] * nh, pair=True, coop=False)
        yield Net("pair 128", 26, 3, [128] * nh, pair=True, coop=False)
        yield Net("pair 64", 26, 3, [64] * nh, pair=True, coop=False)
        yield Net("pair 256 twin", 26, 3, [256] * nh, pair=True, coop=True)
        yield Net("pair 128 twin", 26, 3, [128] * nh, pair=True, coop=True)
        yield Net("select 128", 26, 3, [128] * nh, pair=True, select=True, coop=False)
        yield Net("select 128 twin", 26, 3, [128] * nh, pair=True, select=True, coop=True)
        yield Net("select 256", 26, 3, [256] * nh, pair=True, select=True, coop=False)


def bits(libs):
    this, parent = libs["this"], libs["parent"]
    bad = 0
    for net in bit_cases():
        g = net.g
        B, D = 77, net.dim                      # 77 rows: the last tile of 16 or 32 columns (8 samples with a tangent column) is partly empty
        rnd = lambda *s: f32(torch.randn(*s, generator=g))
        x, cond, probe = rnd(B, D), rnd(B, net.cond), f32(torch.sign(torch.randn(B, D, generator=g)))
        noise = rnd(2, B, D)
        affine = tuple(f32(t) for t in (torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) + 0.5,
                                        torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1))
        att = {"k1": rnd(B, D), "kl1": rnd(B), "lp0": rnd(B)}
        for attempt in (None, att):
            tab = net.table(bit_rows(net, attempt is not None))
            for src in ("buffer", "in-kernel") if net.mode == 0 else ("buffer",):
                kw = dict(noise=noise) if src == "buffer" else dict(rng=(1234, 1000, 3))
                res = [net.launch(L, x, tab, 6, cond=cond, probe=probe, affine=affine, attempt=attempt, **kw) for L in (parent, this)]
                torch.cuda.synchronize()
                tag = f"{net.kernel:34s} {net.name:32s} hidden={len(net.hidden)} {'attempt(k1_in, n_aux=4)' if attempt else 'plain':24s} noise={src:9s}"
                (rp, op), (rt, ot) = res
                if rp != 0 or rt != 0:
                    ok = rp == rt
                    print(f"{tag} refused by the launcher: parent rc={rp}, this rc={rt} -> {'same' if ok else 'DIFFERENT'}")
                else:
                    diff = [f"{k} (max |difference| {float((op[k].double() - ot[k].double()).abs().nan_to_num(nan=9e9).max()):.3g})"
                            for k in op if not torch.equal(op[k].view(torch.int32), ot[k].view(torch.int32))]
                    ok = not diff
                    fin = bool(torch.isfinite(op["x_out"]).all())
                    print(f"{tag} status={int(op['status'])} finite={fin} outputs={'+'.join(op)}: "
                          f"{'bitwise equal' if ok else 'MISMATCH in ' + ','.join(diff)}")
                bad += not ok
    print(f"\nbits: {bad} case(s) differ from the parent")
    return bad


def rk4_table(net, steps, h):
    rows = []
    for _ in range(steps):
        rows += [{"slot": 0}, {"slot": 1, "cin": [h / 2]}, {"slot": 2, "cin": [0, h / 2]},
                 {"slot": 3, "cin": [0, 0, h], "flags": 1, "cout": [h / 6, h / 3, h / 3, h / 6]}]
    if net.select:
        for i, r in enumerate(rows):
            r["flags"] = r.get("flags", 0) | (4 if i % 2 else 0)
    return net.table(rows)


def timing(libs):
    cases = [(Net("headline 4x256 state-only", 16, 0, [256] * 4, coop=False), 1 << 20, 100),
             (Net("headline's tangent twin (Hutchinson)", 16, 0, [256] * 4, mode=1, coop=False), 1 << 18, 100),
             (Net("128-wide 3x128", 16, 4, [128] * 3, coop=False), 1 << 20, 100),
             (Net("512-wide 5x512", 64, 4, [512] * 5, coop=False), 1 << 17, 50),
             (Net("pair 256", 16, 0, [256] * 3, pair=True, coop=False), 1 << 19, 50),
             (Net("pair 128", 16, 0, [128] * 3, pair=True, coop=False), 1 << 20, 50),
             (Net("select 256", 16, 0, [256] * 3, pair=True, select=True, coop=False), 1 << 19, 100),
             (Net("pair 256 twin, small batch", 16, 0, [256] * 3, pair=True, coop=True), 2048, 500)]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bad = 0
    for net, B, steps in cases:
        g = net.g
        x = f32(torch.randn(B, net.dim, generator=g))
        cond = f32(torch.randn(B, net.cond, generator=g)) if net.cond else None
        probe = f32(torch.sign(torch.randn(B, net.dim, generator=g))) if net.mode else None
        tab = rk4_table(net, steps, 1.0 / steps)
        times = {k: [] for k in libs}
        for r in range(10):                       # the first turn warms up
            for k, L in libs.items():
                torch.cuda.synchronize()
                s.record()
                rc, _ = net.launch(L, x, tab, tab.shape[0], cond=cond, probe=probe, status=False)
                e.record()
                torch.cuda.synchronize()
                assert rc == 0, rc
                if r:
                    times[k].append(s.elapsed_time(e))
        med = {k: statistics.median(v) for k, v in times.items()}
        floor, gap = abs(med["parent copy"] - med["parent"]), abs(med["this"] - med["parent"])
        ok = gap <= floor
        bad += not ok
        print(f"{net.kernel:34s} {net.name:38s} B={B:8d} rows={tab.shape[0]:5d}  " +
              "  ".join(f"{k} {med[k]:9.3f} ms [{min(times[k]):.3f}, {max(times[k]):.3f}]" for k in libs) +
              f"  |this - parent| = {gap:.3f} ms ({100 * gap / med['parent']:.3f} %), |copy - parent| = {floor:.3f} ms "
              f"({100 * floor / med['parent']:.3f} %): {'within' if ok else 'OUTSIDE'} the parent-against-parent gap", flush=True)
    print(f"\ntime: {bad} case(s) outside their parent-against-parent gap")
    return bad


def probe(libs):
    """Where a mismatch comes from: the first case with features of the launch taken away one at a time, and the parent
    library against its own byte copy."""
    net = Net("256 state-only", 13, 3, [256, 256], coop=False)
    g = net.g
    B, D = 77, net.dim
    rnd = lambda *s: f32(torch.randn(*s, generator=g))
    x, cond, noise = rnd(B, D), rnd(B, net.cond), rnd(2, B, D)
    affine = tuple(f32(t) for t in (torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) + 0.5,
                                    torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1))
    base = bit_rows(net, False)
    import copy

    def variant(name, rows, n, **kw):
        tab = net.table(rows)
        outs = {k: net.launch(L, x, tab, n, cond=cond, **kw)[1]["x_out"] for k, L in libs.items()}
        torch.cuda.synchronize()
        d = lambda a, b: float((outs[a].double() - outs[b].double()).abs().max())
        print(f"probe {name:44s} |this - parent| = {d('this', 'parent'):.3g}   |parent copy - parent| = {d('parent copy', 'parent'):.3g}")
    variant("full", copy.deepcopy(base), 6, noise=noise, affine=affine)
    variant("no affine maps", copy.deepcopy(base), 6, noise=noise)
    variant("output affine map only", copy.deepcopy(base), 6, noise=noise, affine=(None, None) + affine[2:])
    rows = copy.deepcopy(base)
    for r in rows[:6]:
        r["flags"] &= ~2
    variant("no noise rows, no affine", rows, 6)
    for r in rows[:6]:
        r["flags"] = 0
    variant("no noise, no STEP_END, no affine", rows, 6)
    variant("one row, nothing else", rows[:1] + rows[6:], 1)
    rows1 = copy.deepcopy(rows[:1] + rows[6:])
    rows1[0]["flags"] = 1
    rows1[0]["cout"] = [1.0]
    rows1[0]["a"] = 0.0
    variant("one Euler step, a = 0", rows1, 1)


if __name__ == "__main__":
    parent_path = Path(sys.argv[1]).resolve()
    what = sys.argv[2:] or ["bits", "time"]
    libs = {"parent": _native.load_library(parent_path), "this": _native.lib()}
    bad = 0
    if "bits" in what:
        bad += bits(libs)
    if "time" in what or "probe" in what:
        copy = Path(tempfile.mkdtemp()) / "libflowfusion_amd_parent_copy.so"
        shutil.copyfile(parent_path, copy)
        libs = {"parent": libs["parent"], "parent copy": _native.load_library(copy), "this": libs["this"]}
        if "probe" in what:
            probe(libs)
        if "time" in what:
            bad += timing(libs)
    sys.exit(1 if bad else 0)
