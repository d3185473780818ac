"""Hutch++ / XTrace from J^T v products (``products="vjp"``): CPU tier.

The streaming steps' host twins (ff_trace_basis_host / ff_trace_combine_host, csrc/ff_trace_prod.h) against the recorded-
Jacobian estimator they restate (ff_trace_estimate_host) -- for EQUALITY OF BITS on matrices whose products are exact -- and
against the reference's fixtures with torch.autograd products; ``RowStepper.run_table_products`` with an injected launcher;
every refusal of the front ends and of ff_mlp_ode_launch_vjp; the C ABI of the new struct."""
import ctypes
import inspect
import os
import subprocess
from pathlib import Path

import pytest
import torch
from torch import nn

from flowfusion_amd import _native, host_stepper, odeint, solvers, trace_estimators as TE
from flowfusion_amd import diffusion as D
from tests import _estimator_products_ref as EP
from tests._util import golden_names, load_golden, score_model
from tests.test_trace_estimators import _close, well_posed

ROOT = Path(__file__).resolve().parents[1]
CASES = golden_names("trace_")
OK, BAD, UNS = _native.FF_OK, _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED


@pytest.fixture(autouse=True)
def _lib(built_library):
    return built_library


# ---- the same arithmetic as the Jacobian estimator, bit for bit -----------------------------------------------------------------
def _one_per_row(n, B, Dn, g):
    """A[e, b] = a permutation times a diagonal of non-zero fp32 values: (perm [n, B, D], vals [n, B, D], A [n, B, D, D]).
    Every row of a product A v then has ONE term, so the product formed elementwise in fp32 is what trace::matvec sums."""
    perm = torch.stack([torch.stack([torch.randperm(Dn, generator=g) for _ in range(B)]) for _ in range(n)])
    vals = (0.25 + torch.rand(n, B, Dn, generator=g)) * torch.sign(torch.randn(n, B, Dn, generator=g))
    A = torch.zeros(n, B, Dn, Dn)
    A.scatter_(3, perm.unsqueeze(-1), vals.unsqueeze(-1))
    return perm, vals, A


def _exact_products(perm, vals, V):
    """A V for V [n, B, K, D]: one fp32 product per entry, added to the +0 a sum starts from."""
    K = V.shape[2]
    idx = perm.unsqueeze(2).expand(-1, -1, K, -1)
    return vals.unsqueeze(2) * torch.gather(V, 3, idx) + 0.0


@pytest.mark.parametrize("Dn, r, m, kinds", [(1, 1, 2, ("hutchpp", "xtrace")), (5, 2, 3, ("hutchpp", "xtrace")),
                                            (16, 1, 1, ("hutchpp", "xtrace")), (16, 4, 4, ("hutchpp", "xtrace")),
                                            (32, 3, 2, ("hutchpp", "xtrace")), (16, 15, 0, ("xtrace",))])
def test_basis_and_combine_restate_the_jacobian_estimator_bit_for_bit(Dn, r, m, kinds):
    n, B = 3, 9
    g = torch.Generator().manual_seed(100 * Dn + 10 * r + m)
    perm, vals, A = _one_per_row(n, B, Dn, g)
    S = torch.sign(torch.randn(r, B, Dn, generator=g))
    G = torch.sign(torch.randn(max(m, 1), B, Dn, generator=g))
    for kind in kinds:
        probes = (S, G) if kind == "hutchpp" else (S,)
        want = _native.trace_estimate(A, kind, probes, host=True)
        P = S.permute(1, 0, 2).unsqueeze(0).expand(n, B, r, Dn).contiguous()
        Y = _exact_products(perm, vals, P)
        assert torch.equal(Y, torch.einsum("ebik,ebck->ebci", A, P))             # (the premise: the products are exact)
        basis, rfac = _native.trace_basis(Y, kind, probes, host=True)
        K2 = r + m if kind == "hutchpp" else r
        assert basis.shape == (n, B, K2, Dn) and ((rfac is None) if kind == "hutchpp" else rfac.shape == (n, B, r, r))
        got = _native.trace_combine(basis, rfac, _exact_products(perm, vals, basis), kind, probes, host=True)
        assert got.shape == want.shape == (n, B)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, (got - want).abs().max())


# ---- against the reference fixtures ------------------------------------------------------------------------------------------------
def _autograd_products(sm, t, x, cond, V):
    """[B, K, D]: (d ode_drift(t, x[b]) / d x)^T V[b, k] by reverse mode, as the reference forms them."""
    y = x.clone().requires_grad_(True)
    f = sm.ode_drift(t, y, conditional=cond)
    return torch.stack([torch.autograd.grad(f, y, grad_outputs=V[:, k].contiguous(), retain_graph=True)[0]
                        for k in range(V.shape[1])], dim=1)


@pytest.mark.parametrize("name", ["trace_vp_nosigma_16d", "trace_vp_sigma_cond", "trace_ve_nosigma_cond32"])
def test_autograd_products_through_basis_and_combine_match_reference_fixtures(name):
    assert name in CASES
    meta, a = load_golden(name)
    sm = score_model(meta, a)
    x, cond = a["x"], a.get("cond")
    ok_s, ok_o = well_posed(a["S"]), well_posed(a["O"])
    assert int(ok_s.sum()) >= 8 and int(ok_o.sum()) >= 8 and x.shape[0] == 10
    ts = [a[f"t{i}"] for i in range(3)]
    for kind, probes, ok, key in (("hutchpp", (a["S"], a["G"]), ok_s, "div_hpp_"), ("xtrace", (a["O"],), ok_o, "div_xt_")):
        P = probes[0].permute(1, 0, 2).contiguous()
        Y = torch.stack([_autograd_products(sm, t, x, cond, P) for t in ts])
        basis, rfac = _native.trace_basis(Y, kind, probes, host=True)
        Z = torch.stack([_autograd_products(sm, t, x, cond, basis[i]) for i, t in enumerate(ts)])
        div = _native.trace_combine(basis, rfac, Z, kind, probes, host=True)
        for i in range(3):
            _close(div[i], a[f"{key}{i}"], ok)


# ---- run_table_products on the CPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_run_table_products_reproduces_reference_log_density(name):
    """The four steps per chunk with an injected launcher (torch VJP products at the stage states of the same table) give
    the fixtures' log-densities at the bar of test_row_stepper_reproduces_reference_log_density; a chunk budget of one row
    per chunk gives the same bits."""
    meta, a = load_golden(name)
    sm = score_model(meta, a)
    x, cond = a["x"], a.get("cond")
    eps = float(sm.sde.epsilon)
    span, opts = torch.tensor([eps, 1.0]), {"step_size": meta["step_size"]}
    plan = solvers.plan_ode(span, "rk4", opts)
    table = solvers.build_table(plan, *sm._host_schedule()(plan.t_eval), int(sm._net().pull_plan().width))
    calls = []

    def launcher(xc, cc, tab, seeds, per_row):
        assert tab.shape == table.shape and seeds.dim() == (4 if per_row else 3)
        calls.append((xc.shape[0], bool(per_row), seeds.shape[-2]))
        # one sample at a time: torch's CPU matmuls round differently at different batch sizes, the kernel's columns do not
        outs = []
        for b in range(xc.shape[0]):
            cb = None if cc is None else cc[b:b + 1]
            sb = seeds[:, b:b + 1] if per_row else seeds[b:b + 1]
            outs.append(EP.table_products(lambda t, y: sm.ode_drift(t, y, conditional=cb), plan, xc[b:b + 1], sb, per_row)[:2])
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs], dim=1)

    st = host_stepper.RowStepper(sm._net(), "cpu", cond, None, launcher=lambda *a_: None)
    for kind, probes, want in (("hutchpp", (a["S"], a["G"]), a["lp_hpp_rk4"]), ("xtrace", (a["O"],), a["lp_xt_rk4"])):
        ok = well_posed(probes[0])
        del calls[:]
        xT, dlp = st.run_table_products(x, table, kind, probes, cond=cond, launcher=launcher)
        r = probes[0].shape[0]
        K2 = r + a["G"].shape[0] if kind == "hutchpp" else r
        assert calls == [(x.shape[0], False, r), (x.shape[0], True, K2)]
        lp = dlp.view(-1, 1) + sm.sde.prior(xT.shape).log_prob(xT).sum(1, keepdim=True)
        _close(lp, want, ok, 3e-5)
        # one row per chunk: the budget rule n * rows * (K1 + 2 K2) * D * 4, bitwise the same
        del calls[:]
        one = table.shape[0] * (r + 2 * K2) * x.shape[1] * 4
        xT1, dlp1 = st.run_table_products(x, table, kind, probes, cond=cond, max_bytes=one, launcher=launcher)
        assert len(calls) == 2 * x.shape[0] and all(c[0] == 1 for c in calls)
        # (bits, not values: an ill-posed XTrace row -- a singular R -- is NaN on both sides)
        assert torch.equal(xT1, xT) and torch.equal(dlp1.view(torch.int32), dlp.view(torch.int32))
        del calls[:]
        st.run_table_products(x, table, kind, probes, cond=cond, max_bytes=3 * one + one // 2, launcher=launcher)
        assert [c[0] for c in calls[::2]] == [3, 3, 3, 1]


def test_row_weights_are_what_run_table_recorded_computed():
    """The helper factored out of run_table_recorded: every stage row of a step weighs dt * b_j, the step-end row's cout word
    of the slot the stage sits in, in fp32 (torchdiffeq's rk4 is the 3/8 rule); a slot written twice belongs to its last row."""
    plan = solvers.plan_ode(torch.tensor([0.0, 1.0]), "rk4", {"step_size": 0.5})
    table = solvers.build_table(plan, torch.zeros(8), torch.zeros(8), torch.zeros(8, 4), 32)
    w = host_stepper.row_weights(table)
    assert w.dtype == torch.float32 and torch.equal(w, plan.cout.reshape(2, 4, 8)[:, 3, :4].reshape(-1))
    assert torch.equal(w, torch.tensor([1 / 8, 3 / 8, 3 / 8, 1 / 8] * 2) * 0.5)
    assert "row_weights(table)" in inspect.getsource(host_stepper.RowStepper.run_table_recorded)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _model(D_=4, C=0, units=(64, 64), act=None, **kw):
    torch.manual_seed(3)
    mk = {} if act is None else {"activation": act}
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=C, embedding_dimensions=8, units=list(units), **mk), D.VPSDE(),
                        **kw).eval()


class _Foreign(nn.Module):
    n_dimensions = 4

    def forward(self, t, x, conditional=None):
        return -x


@pytest.fixture
def no_device(monkeypatch):
    """Nothing of the solve may be reached: not the probe draw, not the stepper, not a launch."""
    def boom(*a, **k):
        raise AssertionError("the refusal came too late")
    for mod, name in ((TE, "draw_probes"), (TE, "draw_probes_philox"), (odeint, "RowStepper"), (odeint, "_estimator_budget"),
                      (_native, "trace_basis"), (_native, "trace_estimate")):
        monkeypatch.setattr(mod, name, boom)


def test_products_keyword_is_keyword_only_and_defaults_to_the_jacobian_route():
    for fn in (D.ScoreModel.solve_odes_forward, D.ScoreModel.log_prob):
        prm = inspect.signature(fn).parameters["products"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == "jacobian", fn
    assert inspect.signature(odeint.solve).parameters["products"].default == "jacobian"
    for cls in (D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional):
        assert "products" not in inspect.signature(cls.log_prob).parameters          # hard-wired to adaptive dopri5
    doc = " ".join(D.ScoreModel.solve_odes_forward.__doc__.split())
    for piece in ("small D", "agree to rounding, not bitwise", "adaptive solves, the reference's defaults, still take the Jacobian route"):
        assert piece in doc, piece


def test_front_end_refusals_come_before_the_device(no_device):
    x = torch.randn(6, 4)
    fixed = dict(method="rk4", options={"step_size": 0.25}, products="vjp")
    for kw in (dict(hutchpp=True, hpp_rank=2, hpp_vecs=2), dict(xtrace=True, xt_vecs=3)):
        sm = _model(**kw)
        # default arguments: adaptive dopri5
        with pytest.raises(ValueError) as info:
            sm.log_prob(x, products="vjp")
        for piece in ("adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}', 'products="jacobian"'):
            assert piece in str(info.value), (piece, str(info.value))
        for method in solvers.ALL_ADAPTIVE:
            with pytest.raises(ValueError, match="adaptive"):
                sm.solve_odes_forward(x, method=method, products="vjp")
        with pytest.raises(ValueError, match="grid_constructor"):
            sm.log_prob(x, method="rk4", options={"grid_constructor": lambda f, y, t: t}, products="vjp")
        with pytest.raises(ValueError, match="perturb"):
            sm.log_prob(x, method="rk4", options={"step_size": 0.5, "perturb": True}, products="vjp")
        with pytest.raises(ValueError, match="expected 'jacobian'"):
            sm.log_prob(x, method="rk4", options={"step_size": 0.5}, products="adjoint")
    # a model that is not an estimator model
    for kw in (dict(), dict(hutchinson=True)):
        with pytest.raises(ValueError, match="hutchpp=True or xtrace=True"):
            _model(**kw).log_prob(x, **fixed)
    # more seed columns than a tile holds beside the value column
    x16 = torch.randn(6, 16)
    with pytest.raises(ValueError, match=r"hpp_rank \+ hpp_vecs = 8 \+ 8 > 15") as info:
        _model(D_=16, hutchpp=True, hpp_rank=8, hpp_vecs=8).log_prob(x16, **fixed)
    assert 'products="jacobian"' in str(info.value)
    with pytest.raises(ValueError, match="xt_vecs = 16 > 15") as info:
        _model(D_=16, xtrace=True, xt_vecs=16).log_prob(x16, **fixed)
    assert 'products="jacobian"' in str(info.value)
    for prec in ("bf16x3", "bf16x2"):
        with pytest.raises(ValueError, match="precision='f32'"):
            _model(hutchpp=True, precision=prec).log_prob(x, **fixed)
    # outside the pull units; a model= module
    outside = [_model(units=(512, 512), hutchpp=True), _model(act=nn.Tanh(), xtrace=True), _model(D_=40, hutchpp=True),
               _model(units=(256,) * 19, xtrace=True)]
    for sm in outside:
        with pytest.raises(NotImplementedError) as info:
            sm.log_prob(torch.randn(6, sm.model.n_dimensions), **fixed)
        assert _native.PULL_ENVELOPE in str(info.value)
    with pytest.raises(NotImplementedError) as info:
        D.ScoreModel(_Foreign(), D.VPSDE(), hutchpp=True).log_prob(x, **fixed)
    assert _native.PULL_ENVELOPE in str(info.value) and "no module-path fallback" in str(info.value)


def test_what_passes_the_checks_stops_at_the_device():
    sm = _model(hutchpp=True, hpp_rank=2, hpp_vecs=2)
    with pytest.raises(RuntimeError, match="GPU|cuda"):
        sm.log_prob(torch.randn(6, 4), method="rk4", options={"step_size": 0.25}, products="vjp")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported():
    L = _native.lib()
    for name in ("ff_mlp_ode_launch_vjp", "ff_vjp_kernel_count", "ff_vjp_kernel_name", "ff_trace_basis", "ff_trace_combine",
                 "ff_trace_basis_host", "ff_trace_combine_host", "ff_trace_prod_workspace_floats"):
        assert hasattr(L, name), name
    assert L.ff_vjp_kernel_count() == L.ff_pull_kernel_count() == 3
    names = [L.ff_vjp_kernel_name(i).decode() for i in range(3)]
    assert names == ["mlp_vjp_m16_h128_d4_c4", "mlp_vjp_m16_h256_d4_c4", "mlp_vjp_m16_h256_d8_c4"]
    assert names == [L.ff_pull_kernel_name(i).decode().replace("pull", "vjp") for i in range(3)]      # siblings, index by index
    assert L.ff_vjp_kernel_name(3) is None and L.ff_vjp_kernel_name(-1) is None
    assert _native.VJP_KERNEL_BASE == 0x60000 > _native.PULL_KERNEL_BASE
    header = (ROOT / "include" / "flowfusion_amd.h").read_text()
    assert "#define FF_VJP_KERNEL_BASE 0x60000" in header
    assert int(L.ff_trace_prod_workspace_floats(_native.TRACE_HUTCHPP, 16, 4, 10)) == 10 * (16 * 4 + 2 * 4)
    assert int(L.ff_trace_prod_workspace_floats(_native.TRACE_XTRACE, 16, 4, 10)) == 10 * (16 * 4 + 4 + 5 * 16)


def test_struct_layout_matches_the_header(tmp_path):
    """tests/abi/trace_prod_probe.c, compiled as C11 against the public header and linked with the library: sizeof and
    offsetof of every ff_trace_prod_args field equal the ctypes mirror's, and the host twins run from C."""
    lib = _native.library_path()
    exe = tmp_path / "trace_prod_probe"
    cmd = ["gcc", "-x", "c", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "abi" / "trace_prod_probe.c"), "-x", "none", str(lib), f"-Wl,-rpath,{lib.parent}",
           "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, LD_LIBRARY_PATH=f"{lib.parent}:/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    offsets, other = {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "offsetof":
            offsets[w[1]] = int(w[2])
        else:
            other[w[0]] = w[1:]
    st = _native.TraceProdArgs
    assert int(other["sizeof"][0]) == ctypes.sizeof(st)
    names = [n for n, *_ in st._fields_]
    assert set(names) == set(offsets), set(names) ^ set(offsets)
    for n in names:
        assert getattr(st, n).offset == offsets[n], n
    # tr [[1, 2], [3, 4]] = 5 with r = D = 2: Hutch++ is the trace; NULL arguments are refused
    assert other["basis"][0] == "0" and other["combine"][0] == "0" and abs(float(other["combine"][1]) - 5.0) < 1e-5
    assert other["nullbasis"][0] == "-1" and other["nullcombine"][0] == "-1" and other["nullvjp"][0] == "-1"


def _args(buf, mode=_native.MODE_HUTCH, count=1):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of the
    empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.cond = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count = 0, 1, mode, count
    return a


def test_every_refusal_of_the_products_launch_without_a_gpu():
    L = _native.lib()
    buf = torch.zeros(64)
    ptr = buf.data_ptr()
    pull = _native.make_pull_plan(16, 4, [256] * 4)
    plain = _native.make_pull_plan(16, 0, [128])
    H = _native.MODE_HUTCH
    call = lambda plan, a, seeds=ptr, stride=0, prod=ptr: L.ff_mlp_ode_launch_vjp(ctypes.byref(plan), ctypes.byref(a), seeds, stride,
                                                                                 prod, None)
    for count in (1, 2, 4, 15):
        assert call(pull, _args(buf, H, count)) == OK and call(plain, _args(buf, H, count)) == OK, count
    # K < 1 or K > tile - 1; a mode other than FF_MODE_HUTCH
    for count in (0, -1, 16, 40):
        assert call(pull, _args(buf, H, count)) == BAD, count
    for mode in (_native.MODE_STATE, _native.MODE_EXACT, 7):
        assert call(pull, _args(buf, mode, 3)) == BAD, mode
    # NULL seed_in / prod_out; no arguments
    assert call(pull, _args(buf, H, 3), seeds=None) == BAD and call(pull, _args(buf, H, 3), prod=None) == BAD
    assert L.ff_mlp_ode_launch_vjp(ctypes.byref(pull), None, ptr, 0, ptr, None) == BAD
    # seed_row_stride: 0 or batch * K * dim, nothing else
    for stride in (16, 3 * 16, -1):
        assert call(pull, _args(buf, H, 3), stride=stride) == BAD, stride      # (an empty batch: only 0 = batch * K * dim)
    # ... with a batch: on a forged plan whose stash does not fit at K = 1, a stride that passes reaches that refusal
    # (FF_ERR_UNSUPPORTED, which comes behind it), so nothing is launched either way.  (A products tile keeps dregs words per
    # stage slot where a pull tile keeps dregs + cregs: 19 layers fit it, 20 do not.)
    deep = _native.PlanStruct.from_buffer_copy(pull)
    deep.n_hidden = 20
    for stride, rc in ((0, UNS), (5 * 1 * 16, UNS), (16, BAD), (5 * 16 + 1, BAD), (5 * 16 - 1, BAD), (-1, BAD), (5 * 2 * 16, BAD)):
        a = _args(buf, H, 1)
        a.batch = 5
        assert call(deep, a, stride=stride) == rc, stride
    # the divergence side, attempt launches, the Jacobian output, noise, probes
    for field in ("noise", "k1_in", "kl1_in", "dlogp_in", "jac_out", "dlogp_out", "probe"):
        a = _args(buf, H, 3)
        setattr(a, field, ptr)
        assert call(pull, a) == BAD, field
    a = _args(buf, H, 3)
    a.n_aux = 1
    a.aux_out[0] = ptr
    assert call(pull, a) == BAD
    for field in ("x_in", "x_out", "wpack", "etab", "cond"):
        a = _args(buf, H, 3)
        setattr(a, field, 0)
        assert call(pull, a) == BAD, field
    # a depth whose stash does not fit at this K: a plan the planner would have refused, forged
    deep = _native.PlanStruct.from_buffer_copy(pull)
    deep.n_hidden = 20
    assert call(deep, _args(buf, H, 1)) == UNS
    assert call(deep, _args(buf, H, 3)) == OK
    # a plan that is not a pull plan; a split-precision plan; forged indices
    for mode in (_native.MODE_HUTCH, _native.MODE_STATE, _native.MODE_EXACT):
        assert call(_native.make_plan(16, 4, [256] * 4, mode), _args(buf, H, 3)) == BAD
    assert call(_native.make_push_plan(16, 4, [256] * 4), _args(buf, H, 3)) == BAD
    split = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH, precision=_native.PREC_BF16X2)
    assert call(split, _args(buf, H, 1)) == UNS
    for kid in (_native.PULL_KERNEL_BASE + 3, _native.VJP_KERNEL_BASE, _native.VJP_KERNEL_BASE + 1):
        forged = _native.PlanStruct.from_buffer_copy(pull)
        forged.kernel_id = kid
        assert call(forged, _args(buf, H, 3)) == BAD
    # the other entry points keep refusing a pull plan
    a = _args(buf, H, 3)
    a.dlogp_out = a.probe = ptr
    assert L.ff_mlp_ode_launch(ctypes.byref(pull), ctypes.byref(a), None) == BAD
    assert L.ff_mlp_ode_launch_probes(ctypes.byref(pull), ctypes.byref(a), ptr, None) == BAD
    assert L.ff_mlp_ode_launch_push(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), None, ptr, None) == BAD
    assert L.ff_mlp_ode_launch_pull(ctypes.byref(pull), ctypes.byref(_args(buf, H, 3)), ptr, ptr, None, None) == OK


def test_streaming_launches_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    buf = torch.zeros(256)

    def args(**kw):
        a = _native.TraceProdArgs()
        a.kind, a.dim, a.n_rows, a.r, a.m, a.batch = _native.TRACE_HUTCHPP, 4, 1, 2, 1, 1
        for f in ("probes0", "probes1", "y", "basis", "rfac", "prod", "out", "workspace"):
            setattr(a, f, buf.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    both = (L.ff_trace_basis_host, L.ff_trace_combine_host)
    assert all(fn(ctypes.byref(args())) == OK for fn in both)
    for kw in (dict(kind=0), dict(kind=3), dict(dim=0), dict(r=0), dict(r=5), dict(m=0), dict(probes1=0), dict(probes0=0),
               dict(basis=0), dict(workspace=0), dict(kind=_native.TRACE_XTRACE, rfac=0), dict(n_rows=-1), dict(batch=-1)):
        assert all(fn(ctypes.byref(args(**kw))) == BAD for fn in both), kw
    assert L.ff_trace_basis_host(ctypes.byref(args(y=0))) == BAD and L.ff_trace_combine_host(ctypes.byref(args(y=0))) == OK
    for kw in (dict(prod=0), dict(out=0)):
        assert L.ff_trace_combine_host(ctypes.byref(args(**kw))) == BAD and L.ff_trace_basis_host(ctypes.byref(args(**kw))) == OK
    assert L.ff_trace_basis_host(None) == BAD and L.ff_trace_combine(None, None) == BAD and L.ff_trace_basis(None, None) == BAD
    # Python's wrappers: shapes that do not match, device memory only
    S, G = torch.ones(2, 3, 4), torch.ones(1, 3, 4)
    with pytest.raises(RuntimeError, match="do not match"):
        _native.trace_basis(torch.zeros(1, 3, 3, 4), "hutchpp", (S, G), host=True)
    with pytest.raises(RuntimeError, match="device memory"):
        _native.trace_basis(torch.zeros(1, 3, 2, 4), "hutchpp", (S, G))


def test_eighth_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_vjp_products
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_pull_plan(16, 4, [256] * 4), 4)
    with FakeTensorMode():
        x, c = torch.empty(9, 16), torch.empty(9, 4)
        y, prod, st = op(x, c, torch.empty(9, 3, 16), torch.empty(10), torch.empty(12, 32 + 256), None, None, None, None, plan)
        assert y.shape == (9, 16) and prod.shape == (12, 9, 3, 16) and st.shape == (1,)
        y, prod, st = op(x, c, torch.empty(12, 9, 5, 16), torch.empty(10), torch.empty(12, 288), None, None, None, None, plan)
        assert prod.shape == (12, 9, 5, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), torch.zeros(2, 4), torch.zeros(2, 3, 16), torch.zeros(10), torch.zeros(12, 288), None, None, None, None,
           plan)
