"""GPU tier of the per-probe Hutchinson output (`-m gpu`): ff_mlp_ode_launch_probes stores every tangent column's own
integrated divergence, [batch, K], beside the sum the launch has always returned.

* ops level: the networks, grid and batches of tests/test_gpu_hutchinson_multi.py with Gaussian probes, both launch kinds
  -- state and dlogp bitwise those of the op without the output, the output bitwise equal between the launch kinds, equal to
  dlogp at K = 1, its row sums on dlogp, and every (row, probe) entry against the float64 oracle at LOGP_TOL;
* C level: the entry point called directly, its output between guard words;
* the tail launch (FF_LAUNCH_ONE_WAVE_AND_TWIN): the pointer moves by row0 * K;
* every f32 instance that serves FF_MODE_HUTCH, at both corners, K = 2 and K = tile - 1, a batch of 2 spt + 1 rows on the
  one-wavefront kernel and on the twin -- and, where an instance has both, the two-launch kind at K = 2 on a batch of one
  round of the chip and three tiles (rows at the start, around the first row of the second launch and at the end);
* the front ends: ``return_stderr=True`` on ScoreModel.log_prob and ODEFlow.log_prob.
"""
import ctypes

import pytest
import torch

from flowfusion_amd import _native, odeint, trace_estimators
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd.fused import MODE_HUTCH
from tests._instances import ONE_WAVE, ROWS, TAIL, TWIN, act_module, chip_tiles, launch_kinds, registry
from tests.test_gpu_hutchinson_multi import CASES, NETS, WrappedMLP, _grid, _net
from tests.test_gpu_parity import DEV, LOGP_TOL, _logp_err, _seeded_score_model

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e33
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _oracle_per_probe(so64, x, cond, probes, opts, method="rk4"):
    """The float64 oracle's divergence of every (row, probe) pair [B, K]: ONE single-probe solve over the B K pairs (rows
    are independent) -- the solve of test_gpu_hutchinson_multi._oracle_sum, before its sum."""
    B, K, Dn = probes.shape
    xs = x.double()[:, None, :].expand(B, K, Dn).reshape(B * K, Dn)
    cs = None if cond is None else cond.double()[:, None, :].expand(B, K, cond.shape[1]).reshape(B * K, -1)
    _, dl = so64.solve_odes_forward(xs, cs, method, opts, "hutch", probes.double().reshape(B * K, Dn))
    return dl.reshape(B, K)


def _pin(monkeypatch, pin):
    if pin is None:
        monkeypatch.delenv("FF_COOP", raising=False)
    else:
        monkeypatch.setenv("FF_COOP", pin)


# ---- ops level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", CASES)
def test_per_probe_output_against_the_oracle(name, K, monkeypatch):
    sm, so64, tile = _net(name)
    Dn, C = NETS[name][0], NETS[name][1]
    opts, tab = _grid(sm)
    net = sm._net()
    spt = tile // (1 + K)
    g = torch.Generator().manual_seed(2000 + K)
    for B in (spt - 1, spt + 1, 4 * spt + 1):
        x = torch.randn(B, Dn, generator=g) * 0.8 + 0.3
        cond = torch.randn(B, C, generator=g) if C else None
        probes = torch.randn(B, K, Dn, generator=g)
        xd, cd, pd = x.to(DEV), None if cond is None else cond.to(DEV), probes.to(DEV)
        results = {}
        for pin in (None, "0"):            # the launcher's choice (the twin at these sizes), and the one-wavefront kernel
            _pin(monkeypatch, pin)
            xT0, dl0, _ = net.integrate(xd, tab, MODE_HUTCH, cond=cd, probe=pd, stage_slots=4)
            xT, dl, d, status = net.integrate(xd, tab, MODE_HUTCH, cond=cd, probe=pd, stage_slots=4, per_probe=True)
            assert xT.shape == (B, Dn) and dl.shape == (B,) and d.shape == (B, K) and d.dtype == torch.float32
            assert torch.equal(xT, xT0) and torch.equal(dl, dl0), (name, K, B, pin, "the launch changed with the output")
            if K == 1:
                assert torch.equal(d[:, 0], dl), (name, B, pin)
                d1 = net.integrate(xd, tab, MODE_HUTCH, cond=cd, probe=pd[:, 0].contiguous(), stage_slots=4, per_probe=True)[2]
                assert torch.equal(d1, d), (name, B, pin, "[B, D] probe, tangent_count 0")
            results[pin] = d
        monkeypatch.delenv("FF_COOP", raising=False)
        assert torch.equal(results[None], results["0"]), (name, K, B)
        if B == 0:
            continue
        assert int(status.item()) == 0
        d = results[None]
        err_sum = _logp_err(d.double().sum(dim=1).float(), dl.cpu())
        want = _oracle_per_probe(so64, x, cond, probes, opts)
        err = _logp_err(d, want.float())
        print(f"{name} K={K} B={B}: per-probe err {err:.3g}, row sums against dlogp {err_sum:.3g}")
        assert err_sum < LOGP_TOL, (name, K, B, err_sum)
        assert err < LOGP_TOL, (name, K, B, err)


def test_empty_batch_returns_empty_tensors():
    sm, _, _ = _net("16d_4x256")
    _, tab = _grid(sm)
    xT, dl, d, status = sm._net().integrate(torch.zeros(0, 16, device=DEV), tab, MODE_HUTCH,
                                            probe=torch.zeros(0, 3, 16, device=DEV), stage_slots=4, per_probe=True)
    assert xT.shape == (0, 16) and dl.shape == (0,) and d.shape == (0, 3) and int(status.item()) == 0


def test_fifth_op_passes_opcheck():
    """Schema and fake-tensor registration of flowfusion_amd::mlp_ode_probes as torch.library.opcheck sees them."""
    sm, _, _ = _net("8d_c3_2x256")
    _, tab = _grid(sm)
    net = sm._net()
    x, cond = torch.randn(11, 8, device=DEV), torch.randn(11, 3, device=DEV)
    tests = ("test_schema", "test_faketensor")
    for probe, count in ((torch.randn(11, 3, 8, device=DEV), 3), (torch.randn(11, 8, device=DEV), 0)):
        args = (x, cond, probe, net.wpack(x.device, MODE_HUTCH), tab.to(DEV), None, None, None, None,
                _native.plan_words(net.plan(MODE_HUTCH), 4), count)
        torch.library.opcheck(torch.ops.flowfusion_amd.mlp_ode_probes.default, args, test_utils=tests)


# ---- C level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])          # 16 columns: five samples and a dead column; four samples, no dead column
def test_entry_point_writes_nothing_outside_its_output(K, monkeypatch):
    sm, _, tile = _net("16d_4x256")
    _, tab = _grid(sm)
    net = sm._net()
    plan = net.plan(MODE_HUTCH)
    spt = tile // (1 + K)
    B = 2 * spt + 3                              # not a multiple of spt: the last tile holds three rows
    g = torch.Generator().manual_seed(77 + K)
    x = (torch.randn(B, 16, generator=g) * 0.8 + 0.3).to(DEV)
    probes = torch.randn(B, K, 16, generator=g).to(DEV)
    wpack, etab = net.wpack(x.device, MODE_HUTCH), tab.to(DEV).contiguous()
    L = _native.lib()
    for pin in (None, "0"):
        _pin(monkeypatch, pin)
        _, dl_op, d_op, _ = net.integrate(x, tab, MODE_HUTCH, probe=probes, stage_slots=4, per_probe=True)
        for misalign in (0, 1):
            n = B * K
            arena = torch.full((GUARD + n + GUARD + 1,), SENTINEL, device=DEV)
            lo = GUARD + misalign
            x_out, dl, status = torch.empty_like(x), torch.zeros(B, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            a = _native.OdeArgs()
            a.x_in, a.x_out, a.probe, a.dlogp_out = x.data_ptr(), x_out.data_ptr(), probes.data_ptr(), dl.data_ptr()
            a.wpack, a.etab, a.status = wpack.data_ptr(), etab.data_ptr(), status.data_ptr()
            a.batch, a.n_evals, a.mode, a.tangent_count, a.stage_slots = B, etab.shape[0], MODE_HUTCH, K, 4
            rc = L.ff_mlp_ode_launch_probes(ctypes.byref(plan), ctypes.byref(a), arena[lo:].data_ptr(),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == _native.FF_OK
            torch.cuda.synchronize()
            assert bool((arena[:lo] == SENTINEL).all()) and bool((arena[lo + n:] == SENTINEL).all()), (K, pin, misalign)
            assert torch.equal(arena[lo:lo + n].view(B, K), d_op) and torch.equal(dl, dl_op), (K, pin, misalign)
            assert not bool((arena[lo:lo + n] == SENTINEL).any()) and int(status.item()) == 0
    monkeypatch.delenv("FF_COOP", raising=False)


# ---- the tail launch ---------------------------------------------------------------------------------------------------------
def test_tail_launch_moves_the_output_by_k_floats_per_row(monkeypatch):
    monkeypatch.delenv("FF_COOP", raising=False)
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    name, K = "16d_4x256", 3
    sm, so64, tile = _net(name)
    opts, tab = _grid(sm)
    net, plan = sm._net(), sm._net().plan(MODE_HUTCH)
    spt = tile // (1 + K)
    B = (2048 + 100) * spt + 1                       # two wavefronts per SIMD: 2048 tiles a round, 101 left over
    assert _native.launch_kind(plan, B, MODE_HUTCH, K) == _native.LAUNCH_ONE_WAVE_AND_TWIN
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 16, generator=g) * 0.8 + 0.3
    probes = torch.randn(B, K, 16, generator=g)
    xT0, dl0, _ = net.integrate(x.to(DEV), tab, MODE_HUTCH, probe=probes.to(DEV), stage_slots=4)
    xT, dl, d, status = net.integrate(x.to(DEV), tab, MODE_HUTCH, probe=probes.to(DEV), stage_slots=4, per_probe=True)
    assert int(status.item()) == 0 and torch.equal(xT, xT0) and torch.equal(dl, dl0) and d.shape == (B, K)
    row0 = 2048 * spt
    rows = torch.cat([torch.arange(0, 5), torch.arange(row0 - 3, row0 + 6), torch.arange(B - 6, B)])
    want = _oracle_per_probe(so64, x[rows], None, probes[rows], opts)
    err = _logp_err(d[rows.to(DEV)], want.float())
    print(f"tail rows: per-probe err {err:.3g}")
    assert err < LOGP_TOL
    # the same rows as a batch of their own (the twin): bitwise
    d_small = net.integrate(x[rows].to(DEV), tab, MODE_HUTCH, probe=probes[rows].to(DEV), stage_slots=4, per_probe=True)[2]
    assert torch.equal(d_small, d[rows.to(DEV)])


# ---- every instance ------------------------------------------------------------------------------------------------------------
REGISTRY = registry()
SDES = ("VPSDE", "VESDE", "SUBVPSDE")
HUTCH_KERNELS = [name for name, e in REGISTRY.items() if e[0] in ("f32", "wide") and e[3]]


def _row_model(row, seed):
    from oracle import flowfusion_oracle as O
    torch.manual_seed(seed)
    sde_name, no_sigma = SDES[seed % 3], seed % 2 == 0
    act = act_module(row.act)
    sm = D.ScoreModel(D.MLP(row.D, row.C, 8, list(row.units), activation=act), getattr(D, sde_name)(), no_sigma=no_sigma).eval()
    params = O.mlp_params_from_state_dict({k: v.detach().clone() for k, v in sm.state_dict().items()})
    sde = {"VPSDE": O.VP, "VESDE": O.VE, "SUBVPSDE": O.SubVP}[sde_name](dtype=torch.float64)
    return sm.to(DEV), O.ScoreOracle(params, sde, no_sigma=no_sigma, dtype=torch.float64, activation=act)


@pytest.mark.parametrize("kernel", HUTCH_KERNELS)
def test_every_hutchinson_instance_per_probe_against_the_oracle(kernel, monkeypatch):
    rows = [(i, r) for i, r in enumerate(ROWS) if r.kernel == kernel]
    assert rows and all(r.prec == "f32" and r.mode == "tangent" for _, r in rows), kernel
    kinds = [k for k in launch_kinds(REGISTRY[kernel]) if k in (ONE_WAVE, TWIN)]
    assert kinds
    for i, row in rows:
        seed = 9000 + i
        sm, so = _row_model(row, seed)
        net = sm._net()
        plan = net.plan(MODE_HUTCH)
        assert _native.kernel_name(plan) == row.kernel, row
        tile = int(plan.tile)
        eps = float(sm.sde.epsilon)
        opts = {"step_size": (1.0 - eps) / 4}
        tab = sm._ode_table(torch.tensor([eps, 1.0]), "midpoint", opts, MODE_HUTCH)
        g = torch.Generator().manual_seed(seed)
        for K in (2, tile - 1):
            spt = tile // (1 + K)
            B = 2 * spt + 1
            x0 = torch.randn(B, row.D, generator=g) * 0.5
            cond = torch.randn(B, row.C, generator=g) if row.C else None
            probes = torch.randn(B, K, row.D, generator=g)
            want = _oracle_per_probe(so, x0, cond, probes, opts, "midpoint").float()
            for kind in kinds:
                monkeypatch.setenv("FF_COOP", "1" if kind == TWIN else "0")
                code = _native.LAUNCH_TWIN if kind == TWIN else _native.LAUNCH_ONE_WAVE
                assert _native.launch_kind(plan, B, MODE_HUTCH, K) == code, (row, K, kind)
                _, dl, d, status = net.integrate(x0.to(DEV), tab, MODE_HUTCH, cond=None if cond is None else cond.to(DEV),
                                                 probe=probes.to(DEV), per_probe=True)
                err = _logp_err(d, want)
                print(f"{row.kernel} {row.corner} {row.act} K={K} {kind}: per-probe err {err:.3g}")
                assert int(status.item()) == 0 and d.shape == (B, K)
                assert err < LOGP_TOL, (row, K, kind, err)
            monkeypatch.delenv("FF_COOP", raising=False)
        if TAIL in launch_kinds(REGISTRY[kernel]):
            # full rounds on the one-wavefront kernel, the leftover tiles on the twin: the output moves on by row0 * K floats
            monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
            K = 2
            spt, chip = tile // (1 + K), chip_tiles(REGISTRY[kernel])
            B, row0 = (chip + 3) * spt - 1, chip * spt
            assert _native.launch_kind(plan, B, MODE_HUTCH, K) == _native.LAUNCH_ONE_WAVE_AND_TWIN, (row, B)
            x0 = torch.randn(B, row.D, generator=g) * 0.5
            cond = torch.randn(B, row.C, generator=g) if row.C else None
            probes = torch.randn(B, K, row.D, generator=g)
            idx = torch.cat([torch.arange(0, 3), torch.arange(row0 - 3, row0 + 4), torch.arange(B - 3, B)])
            want = _oracle_per_probe(so, x0[idx], None if cond is None else cond[idx], probes[idx], opts, "midpoint").float()
            _, dl, d, status = net.integrate(x0.to(DEV), tab, MODE_HUTCH, cond=None if cond is None else cond.to(DEV),
                                             probe=probes.to(DEV), per_probe=True)
            err = _logp_err(d[idx.to(DEV)], want)
            print(f"{row.kernel} {row.corner} {row.act} K={K} {TAIL}: per-probe err {err:.3g}")
            assert int(status.item()) == 0 and d.shape == (B, K)
            assert err < LOGP_TOL, (row, K, TAIL, err)


# ---- front ends ----------------------------------------------------------------------------------------------------------------
def _flow_single_probe(flow, x, e_k, opts):
    xn = (x - flow.target_shift) / flow.target_scale
    t_span = torch.tensor([0.0, 1.0], dtype=torch.float32)
    return odeint.solve(flow, xn, t_span, "rk4", opts, MODE_HUTCH, 1e-5, 1e-5, probe=e_k.contiguous())[1]


def test_score_model_log_prob_returns_the_standard_error(monkeypatch):
    B, K, Dn = 37, 7, 16
    sm, _, _ = _seeded_score_model(Dn, 0, [256] * 4, "VPSDE", True, 12)
    sm.hutch = True
    torch.manual_seed(4321)
    x = (torch.randn(B, Dn) * 0.8 + 0.3).to(DEV)
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / 4}
    kw = dict(method="rk4", options=opts, probe="philox", seed=31, num_probes=K)
    plain = sm.log_prob(x, **kw)
    lp, se = sm.log_prob(x, return_stderr=True, **kw)
    d, e = sm.dlogp_probes.clone(), sm.e.clone()
    assert torch.equal(lp, plain) and lp.shape == (B, 1) and se.shape == (B, 1) and se.dtype == torch.float32
    assert d.shape == (B, K) and e.shape == (B, K, Dn) and torch.equal(e, _native.probe_fill(B, K, Dn, 31, 0, DEV))
    assert torch.equal(se, trace_estimators.hutchinson_stderr(d).view(-1, 1)) and bool((se > 0).all())
    # solve_odes_forward: (xT, delta_logp, stderr); delta_logp is the mean of the columns up to the order of the additions
    xT, dlp, se2 = sm.solve_odes_forward(x, return_stderr=True, **kw)
    assert torch.equal(se2, se) and torch.equal(sm.dlogp_probes, d)
    assert _logp_err(d.double().mean(dim=1).float().view(-1, 1), dlp.cpu()) < LOGP_TOL
    # column k is the single-probe solve with probe k of model.e
    t_span = torch.tensor([float(sm.sde.epsilon), 1.0], dtype=torch.float32)
    worst = 0.0
    for k in range(K):
        single = odeint.solve(sm, x, t_span, "rk4", opts, MODE_HUTCH, 1e-5, 1e-5, probe=e[:, k].contiguous())[1]
        worst = max(worst, _logp_err(d[:, k], single.cpu()))
    print(f"ScoreModel: dlogp_probes against K single-probe solves {worst:.3g}")
    assert worst < LOGP_TOL
    # a forced row cut: bitwise
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 7 * K * Dn + 1)       # seven rows per launch
    lp_c, se_c = sm.log_prob(x, return_stderr=True, **kw)
    assert torch.equal(lp_c, lp) and torch.equal(se_c, se) and torch.equal(sm.dlogp_probes, d) and torch.equal(sm.e, e)
    monkeypatch.undo()
    # a row slice with its offset, and the sharded entry point in a one-rank group
    lo, hi = 9, 30
    lp_s, se_s = sm.log_prob(x[lo:hi].contiguous(), sample_offset=lo, return_stderr=True, **kw)
    assert torch.equal(lp_s, lp[lo:hi]) and torch.equal(se_s, se[lo:hi])
    from flowfusion_amd.distributed import log_prob_sharded
    lp_d, se_d = log_prob_sharded(sm, x, seed=31, method="rk4", options=opts, num_probes=K, return_stderr=True)
    assert torch.equal(lp_d, lp) and torch.equal(se_d, se)
    # the generic route: the same network behind a module the envelope does not know
    gm = D.ScoreModel(WrappedMLP(sm.model), sm.sde, no_sigma=True, hutchinson=True).eval()
    assert not gm._fusable()
    torch.manual_seed(99)
    lp_f, se_f = sm.log_prob(x, method="rk4", options=opts, num_probes=K, return_stderr=True)       # torch's probes
    torch.manual_seed(99)
    lp_g, se_g = gm.log_prob(x, method="rk4", options=opts, num_probes=K, return_stderr=True)
    assert torch.equal(gm.e, sm.e) and gm.e.shape == (B, K, Dn) and gm.dlogp_probes.shape == (B, K)
    assert se_g.shape == (B, 1) and torch.equal(se_g, trace_estimators.hutchinson_stderr(gm.dlogp_probes).view(-1, 1))
    errs = (_logp_err(lp_g, lp_f.cpu()), _logp_err(gm.dlogp_probes, sm.dlogp_probes.cpu()), _logp_err(se_g, se_f.cpu()))
    print(f"ScoreModel generic route against fused: log_p {errs[0]:.3g}, per probe {errs[1]:.3g}, stderr {errs[2]:.3g}")
    assert max(errs) < LOGP_TOL               # the same quantities on both routes: estimate, per-probe values, standard error


def test_flow_log_prob_returns_the_standard_error(monkeypatch):
    B, K, Dn = 37, 7, 6
    torch.manual_seed(9)
    f = F.ODEFlow(Dn, [128, 128], target_shift=torch.randn(Dn), target_scale=torch.rand(Dn) + 0.5).eval().to(DEV)
    x = torch.randn(B, Dn, device=DEV)
    opts = {"step_size": 0.25}
    kw = dict(method="rk4", options=opts, hutchinson=True, probe="philox", seed=8, num_probes=K)
    plain = f.log_prob(x, **kw)
    lp, se = f.log_prob(x, return_stderr=True, **kw)
    d, e = f.dlogp_probes.clone(), f.e.clone()
    assert torch.equal(lp, plain) and lp.shape == (B,) and se.shape == (B,) and d.shape == (B, K)
    assert torch.equal(e, _native.probe_fill(B, K, Dn, 8, 0, DEV))
    assert torch.equal(se, trace_estimators.hutchinson_stderr(d)) and bool((se > 0).all())
    worst = max(_logp_err(d[:, k], _flow_single_probe(f, x, e[:, k], opts).cpu()) for k in range(K))
    print(f"ODEFlow: dlogp_probes against K single-probe solves {worst:.3g}")
    assert worst < LOGP_TOL
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 7 * K * Dn + 1)
    lp_c, se_c = f.log_prob(x, return_stderr=True, **kw)
    assert torch.equal(lp_c, lp) and torch.equal(se_c, se) and torch.equal(f.dlogp_probes, d) and torch.equal(f.e, e)
    monkeypatch.undo()
    from flowfusion_amd.distributed import flow_log_prob_sharded
    lp_d, se_d = flow_log_prob_sharded(f, x, seed=8, method="rk4", options=opts, hutchinson=True, num_probes=K, return_stderr=True)
    assert torch.equal(lp_d, lp) and torch.equal(se_d, se)
    # the generic route (torch evaluates the velocity network, K single-probe passes): the same flow, told it is not fusable
    torch.manual_seed(5)
    lp_f, se_f = f.log_prob(x, method="rk4", options=opts, hutchinson=True, num_probes=K, return_stderr=True)
    d_f, e_f = f.dlogp_probes.clone(), f.e.clone()
    monkeypatch.setattr(F.ODEFlow, "_fusable", lambda self: False)
    torch.manual_seed(5)
    lp_g, se_g = f.log_prob(x, method="rk4", options=opts, hutchinson=True, num_probes=K, return_stderr=True)
    assert torch.equal(f.e, e_f) and f.dlogp_probes.shape == (B, K)
    assert se_g.shape == (B,) and torch.equal(se_g, trace_estimators.hutchinson_stderr(f.dlogp_probes))
    errs = (_logp_err(lp_g, lp_f.cpu()), _logp_err(f.dlogp_probes, d_f.cpu()), _logp_err(se_g, se_f.cpu()))
    print(f"ODEFlow generic route against fused: log_p {errs[0]:.3g}, per probe {errs[1]:.3g}, stderr {errs[2]:.3g}")
    assert max(errs) < LOGP_TOL               # the same quantities on both routes: estimate, per-probe values, standard error
