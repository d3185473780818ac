"""GPU tier of the K-probe Hutchinson log-density (`-m gpu`): K independent probes per sample in the tangent columns of ONE
launch (ff_ode_args.tangent_count = K in FF_MODE_HUTCH, probe [B, K, D]).

* ops level, fixed grid: Gaussian probes (a wrong stride cannot hide behind +-1), four networks on four kernels, every K a
  tile holds, batches around the samples-per-tile boundary, both launch kinds -- the state bitwise that of the K = 1
  launch, the divergence against the float64 oracle's sum over the K single-probe solves at the bar of
  tests/test_gpu_parity.py;
* ff_probe_fill bitwise against the K ff_normal_fill sign compositions, between guard words;
* the adaptive routes (device controller, host controller);
* the front ends: ScoreModel, the population wrapper, the flows, the sharded entry point, the generic route.
"""
import math

import pytest
import torch
from torch import nn

from flowfusion_amd import _native, odeint
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from flowfusion_amd.fused import MODE_HUTCH
from tests._util import flow_oracle
from tests.test_gpu_parity import ADAPT_TOL, DEV, LOGP_TOL, _logp_err, _seeded_score_model

pytestmark = pytest.mark.gpu
SENTINEL = -7.5e33
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


# ---- ops level, fixed grid ---------------------------------------------------------------------------------------------------
NETS = {
    # name: (D, C, units, sde, no_sigma)
    "16d_4x256": (16, 0, [256] * 4, "VPSDE", True),
    "2d_3x128": (2, 0, [128] * 3, "VESDE", False),
    "4d_64_64_tile32": (4, 0, [64, 64], "VPSDE", False),
    "8d_c3_2x256": (8, 3, [256, 256], "SUBVPSDE", False),
}
_models = {}


def _net(name):
    """(product model on the GPU, float64 oracle, tile of its Hutchinson plan), built once per network."""
    if name not in _models:
        Dn, C, units, sde_name, no_sigma = NETS[name]
        sm, _, so64 = _seeded_score_model(Dn, C, units, sde_name, no_sigma, 77)
        sm.hutch = True
        _models[name] = (sm, so64, int(sm._net().plan(MODE_HUTCH).tile))
    return _models[name]


def _grid(sm, steps=3):
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / steps}
    t_span = torch.tensor([float(sm.sde.epsilon), 1.0], dtype=torch.float32)
    return opts, sm._ode_table(t_span, "rk4", opts, MODE_HUTCH)


def _oracle_sum(so64, x, cond, probes, opts):
    """sum_k solve_odes_forward(.., "hutch", p_k) of the float64 oracle, as ONE solve over the B K (row, probe) pairs
    (rows are independent); returns (xT [B, D], sum of the K divergences [B])."""
    B, K, Dn = probes.shape
    xs = x.double()[:, None, :].expand(B, K, Dn).reshape(B * K, Dn)
    cs = None if cond is None else cond.double()[:, None, :].expand(B, K, cond.shape[1]).reshape(B * K, -1)
    xT, dl = so64.solve_odes_forward(xs, cs, "rk4", opts, "hutch", probes.double().reshape(B * K, Dn))
    return xT.reshape(B, K, Dn)[:, 0], dl.reshape(B, K).sum(dim=1)


CASES = [(n, K) for n in NETS for K in (1, 2, 3, 7, 15)] + [("4d_64_64_tile32", 31)]


@pytest.mark.parametrize("name,K", CASES)
def test_k_probes_in_one_launch_against_the_oracle(name, K, monkeypatch):
    sm, so64, tile = _net(name)
    Dn, C = NETS[name][0], NETS[name][1]
    opts, tab = _grid(sm)
    net = sm._net()
    spt = tile // (1 + K)
    g = torch.Generator().manual_seed(1000 + K)
    for B in (spt - 1, spt + 1, 4 * spt + 1):
        x = torch.randn(B, Dn, generator=g) * 0.8 + 0.3
        cond = torch.randn(B, C, generator=g) if C else None
        probes = torch.randn(B, K, Dn, generator=g)
        xd, cd, pd = x.to(DEV), None if cond is None else cond.to(DEV), probes.to(DEV)
        results = {}
        for pin in (None, "0"):            # the launcher's choice (the twin at these sizes), and the one-wavefront kernel
            if pin is None:
                monkeypatch.delenv("FF_COOP", raising=False)
            else:
                monkeypatch.setenv("FF_COOP", pin)
            xT, dl, status = net.integrate(xd, tab, MODE_HUTCH, cond=cd, probe=pd, stage_slots=4)
            x1, dl1, _ = net.integrate(xd, tab, MODE_HUTCH, cond=cd, probe=pd[:, 0].contiguous(), stage_slots=4)
            assert xT.shape == (B, Dn) and dl.shape == (B,)
            assert torch.equal(xT, x1), (name, K, B, pin, "the state depends on the probes")
            if K == 1:      # [B, 1, D] with tangent_count = 1 is the op without it
                assert torch.equal(dl, dl1), (name, B, pin)
            results[pin] = (xT, dl)
        monkeypatch.delenv("FF_COOP", raising=False)
        assert torch.equal(results[None][0], results["0"][0]) and torch.equal(results[None][1], results["0"][1]), (name, K, B)
        if B == 0:
            continue
        assert int(status.item()) == 0
        xT64, want = _oracle_sum(so64, x, cond, probes, opts)
        err = _logp_err(results[None][1], want.float())
        print(f"{name} K={K} B={B}: dlogp err {err:.3g}")
        assert err < LOGP_TOL, (name, K, B, err)


def test_tail_launch_moves_the_probes_by_k_rows_per_sample(monkeypatch):
    """A batch whose last round of tiles goes to the twin as a second launch (FF_LAUNCH_ONE_WAVE_AND_TWIN): the rows of the
    tail -- their probes start row0 K D floats into the buffer -- and rows of the main launch, against the oracle."""
    monkeypatch.delenv("FF_COOP", raising=False)
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    name, K = "16d_4x256", 3
    sm, so64, tile = _net(name)
    opts, tab = _grid(sm)
    net, plan = sm._net(), sm._net().plan(MODE_HUTCH)
    spt = tile // (1 + K)
    B = (2048 + 100) * spt + 1                       # two wavefronts per SIMD: 2048 tiles a round, 101 left over
    assert _native.launch_kind(plan, B, MODE_HUTCH, K) == _native.LAUNCH_ONE_WAVE_AND_TWIN
    assert _native.launch_kind(plan, 40 * spt, MODE_HUTCH, K) == _native.LAUNCH_TWIN
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 16, generator=g) * 0.8 + 0.3
    probes = torch.randn(B, K, 16, generator=g)
    xT, dl, status = net.integrate(x.to(DEV), tab, MODE_HUTCH, probe=probes.to(DEV), stage_slots=4)
    assert int(status.item()) == 0
    row0 = 2048 * spt
    rows = torch.cat([torch.arange(0, 5), torch.arange(row0 - 3, row0 + 6), torch.arange(B - 6, B)])
    _, want = _oracle_sum(so64, x[rows], None, probes[rows], opts)
    err = _logp_err(dl[rows.to(DEV)], want.float())
    print(f"tail rows: dlogp err {err:.3g}")
    assert err < LOGP_TOL
    # the same rows as a batch of their own (the twin): bitwise
    _, dl_small, _ = net.integrate(x[rows].to(DEV), tab, MODE_HUTCH, probe=probes[rows].to(DEV), stage_slots=4)
    assert torch.equal(dl_small, dl[rows.to(DEV)])


def test_op_refuses_a_probe_that_does_not_match_the_count():
    sm, _, _ = _net("16d_4x256")
    _, tab = _grid(sm)
    net = sm._net()
    x = torch.randn(5, 16, device=DEV)
    args = (x, None, None, None, net.wpack(x.device, MODE_HUTCH), tab.to(DEV), None, None, None, None,
            _native.plan_words(net.plan(MODE_HUTCH), 4), MODE_HUTCH)
    op = torch.ops.flowfusion_amd.mlp_ode
    for probe, count in ((torch.randn(5, 3, 16), 0), (torch.randn(5, 16), 3), (torch.randn(5, 3, 16), 2)):
        with pytest.raises(RuntimeError, match="probe has shape"):
            op(args[0], args[1], probe.to(DEV), *args[3:], 0, count)
    with pytest.raises(RuntimeError, match="FF_ERR_BADARG"):          # 1 + K > tile
        op(args[0], args[1], torch.randn(5, 16, 16, device=DEV), *args[3:], 0, 16)


# ---- ff_probe_fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D_", [1, 5, 16])
def test_probe_fill_is_the_k_normal_fill_sign_compositions(D_):
    seed, offset = 991 + D_, 2 ** 33 + 5
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for K in (1, 2, 15):
        scale = float(torch.tensor(K ** -0.5, dtype=torch.float32))
        idx = [_native.PROBE_NOISE_INDEX] + [_native.HUTCH_PROBE_NOISE_BASE + k for k in range(1, K)]
        for B in (0, 1, 256 // ((D_ + 3) // 4) // K + 1, 1031):              # empty, one row, one item past a block, many blocks
            for misalign in (0, 1):
                n = B * K * D_
                arena = torch.full((GUARD + n + GUARD + 1,), SENTINEL, device=DEV)
                lo = GUARD + misalign
                view = arena[lo:lo + n]
                rc = _native.lib().ff_probe_fill(view.data_ptr() if n else arena.data_ptr(), B, K, D_, seed, offset, scale, stream())
                assert rc == _native.FF_OK
                torch.cuda.synchronize()
                assert bool((arena[:lo] == SENTINEL).all()) and bool((arena[lo + n:] == SENTINEL).all()), (B, K, D_, misalign)
                if B == 0:
                    continue
                zs = torch.stack([_native.normal_fill(B, D_, seed, offset, DEV, noise_index=i) for i in idx], dim=1)
                want = torch.where(zs >= 0, 1.0, -1.0).to(torch.float32) * scale
                assert torch.equal(view.view(B, K, D_), want), (B, K, D_, misalign)
    got = _native.probe_fill(37, 3, D_, seed, 11, DEV)
    assert torch.equal(got[:, 0], torch.where(_native.normal_fill(37, D_, seed, 11, DEV, noise_index=_native.PROBE_NOISE_INDEX) >= 0, 1.0, -1.0))
    assert torch.equal(_native.probe_fill(20, 3, D_, seed, 11 + 9, DEV), got[9:29])


# ---- adaptive routes -----------------------------------------------------------------------------------------------------------
ADAPTIVE = {"cond_5d_c3_ragged": (5, 3, [64, 100], "SUBVPSDE", False, 33), "c2_16d_4x256": (16, 0, [256] * 4, "VPSDE", True, 48)}


def _both(monkeypatch, fn):
    monkeypatch.delenv("FF_HOST_CONTROLLER", raising=False)
    dev = fn()
    monkeypatch.setenv("FF_HOST_CONTROLLER", "1")
    host = fn()
    monkeypatch.delenv("FF_HOST_CONTROLLER", raising=False)
    return dev, host


@pytest.mark.parametrize("name", list(ADAPTIVE))
def test_adaptive_solves_carry_k_probes(name, monkeypatch):
    Dn, C, units, sde_name, no_sigma, B = ADAPTIVE[name]
    sm, so32, _ = _seeded_score_model(Dn, C, units, sde_name, no_sigma, 901)
    sm.hutch = True
    torch.manual_seed(17)
    x0 = torch.randn(B, Dn) * 0.5
    cond = torch.randn(B, C) if C else None
    cd = None if cond is None else cond.to(DEV)
    e = torch.sign(torch.randn(B, Dn))
    opts = {"min_step": 1e-6}
    # four copies of e / 2 are the single-probe problem: 4 (e/2)^T J (e/2) = e^T J e, up to the order of a few fp32 additions
    monkeypatch.delenv("FF_HOST_CONTROLLER", raising=False)
    four = (e / 2)[:, None, :].expand(B, 4, Dn).contiguous().to(DEV)
    t_span = torch.tensor([float(sm.sde.epsilon), 1.0], dtype=torch.float32)
    sm.prob, sm.conditional = True, cd
    xT, dl = odeint.solve(sm, x0.to(DEV), t_span, "dopri5", opts, MODE_HUTCH, 1e-4, 1e-4, cond=cd, probe=four)
    assert "chunks" in sm.last_solver_stats and sm.last_solver_stats["accepted"] >= 3          # the device controller
    lp = dl.view(-1, 1) + sm.sde.prior(xT.shape).log_prob(xT).sum(1, keepdim=True)
    ref = so32.log_prob(x0, cond, "dopri5", opts, "hutch", e)
    err = _logp_err(lp, ref)
    print(f"{name}: four copies of e/2 against the single-probe oracle: {err:.3g}")
    assert err < ADAPT_TOL

    # three independent probes under both controllers
    def logp():
        torch.manual_seed(5)
        lp = sm.log_prob(x0.to(DEV), conditional=cd, num_probes=3)
        return lp, dict(sm.last_solver_stats), sm.e.clone()
    (ld, sd, ed), (lh, sh, eh) = _both(monkeypatch, logp)
    assert "chunks" in sd and "chunks" not in sh
    assert (sd["attempts"], sd["accepted"]) == (sh["attempts"], sh["accepted"]), (sd, sh)
    assert ed.shape == (B, 3, Dn) and torch.equal(ed, eh)
    err = _logp_err(ld, lh.cpu())
    print(f"{name}: K=3 device against host controller: {err:.3g}, {sd}")
    assert err < 1e-5


# ---- front ends ------------------------------------------------------------------------------------------------------------------
def test_score_model_log_prob_with_num_probes(monkeypatch):
    sm, _, so64 = _seeded_score_model(16, 0, [256] * 4, "VPSDE", True, 12)
    sm.hutch = True
    B, K = 41, 3
    torch.manual_seed(4321)
    x0 = torch.randn(B, 16) * 0.8 + 0.3
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / 4}
    kw = dict(method="rk4", options=opts)
    torch.manual_seed(99)
    lp = sm.log_prob(x0.to(DEV), num_probes=K, **kw)
    e = sm.e.cpu()
    torch.manual_seed(99)
    assert e.shape == (B, K, 16) and torch.equal(e, torch.sign(torch.randn(B, K, 16)))
    want = torch.stack([so64.log_prob(x0.double(), None, "rk4", opts, "hutch", e[:, k].double()) for k in range(K)]).mean(dim=0)
    err = _logp_err(lp, want.float())
    print(f"ScoreModel.log_prob(num_probes=3): {err:.3g}")
    assert lp.shape == (B, 1) and err < LOGP_TOL
    # num_probes=1 is the call without the keyword
    torch.manual_seed(7)
    a = sm.log_prob(x0.to(DEV), **kw)
    ea = sm.e.clone()
    torch.manual_seed(7)
    b = sm.log_prob(x0.to(DEV), num_probes=1, **kw)
    assert torch.equal(a, b) and torch.equal(ea, sm.e) and sm.e.shape == (B, 16)
    # philox: a slice with sample_offset, a forced row cut, the sharded entry point in a one-rank group -- all bitwise
    pk = dict(probe="philox", seed=31, num_probes=K, **kw)
    xd = x0.to(DEV)
    whole = sm.log_prob(xd, **pk)
    e_whole = sm.e.clone()
    assert torch.equal(e_whole, _native.probe_fill(B, K, 16, 31, 0, DEV))
    assert torch.equal(e_whole[:, 0], torch.where(_native.normal_fill(B, 16, 31, 0, DEV, noise_index=_native.PROBE_NOISE_INDEX) >= 0, 1.0, -1.0))
    lo, hi = 9, 30
    assert torch.equal(sm.log_prob(xd[lo:hi].contiguous(), sample_offset=lo, **pk), whole[lo:hi])
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 7 * K * 16 + 1)      # seven rows per launch (strictly fewer floats)
    cut = sm.log_prob(xd, **pk)
    assert torch.equal(cut, whole) and torch.equal(sm.e, e_whole)
    torch.manual_seed(99)
    assert torch.equal(sm.log_prob(xd, num_probes=K, **kw), lp) and torch.equal(sm.e.cpu(), e)      # torch probes, cut
    monkeypatch.undo()
    from flowfusion_amd.distributed import log_prob_sharded
    assert torch.equal(log_prob_sharded(sm, xd, seed=31, num_probes=K, **kw), whole)
    assert not torch.equal(sm.log_prob(xd, **{**pk, "seed": 32}), whole)


class WrappedMLP(nn.Module):
    """An MLP behind a module that does not look like one (no NN / W / pi attributes): takes the generic route."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, t, x, conditional=None):
        return self.inner(t, x, conditional=conditional)


def _flow_oracle_log_prob(flow, args, probes, opts):
    """log_prob of tests/_util.flow_oracle's float64 flow with the Hutchinson divergence averaged over ``probes`` [B, K, D]:
    the oracle's own dynamics and rk4 stepper, the divergence by one autograd product per probe (the oracle has the exact
    trace only: flow.py has no Hutchinson mode to restate)."""
    from oracle import flowfusion_oracle as O
    fo = flow_oracle({k: v.detach().cpu().clone() for k, v in flow.state_dict().items()}, torch.float64)
    x = (args[0].double() - fo.p.target_shift) / fo.p.target_scale
    cond = args[1].double() if len(args) > 1 else None
    P = probes.double()

    def func(t, y):
        with torch.enable_grad():
            z = y[0].detach().requires_grad_(True)
            v = fo.dynamics(t, z, cond)
            div = sum((torch.autograd.grad(v, z, P[:, k], retain_graph=True)[0] * P[:, k]).sum(dim=1) for k in range(P.shape[1]))
        return v.detach(), (div / P.shape[1]).detach().view(-1, 1)
    times = torch.tensor([0.0, 1.0], dtype=torch.float32).double()
    xT, logj = O.odeint(func, (x, torch.zeros(x.shape[0], 1, dtype=torch.float64)), times, "rk4", opts, 1e-5, 1e-5)
    return torch.sum(-0.5 * xT ** 2 - 0.5 * torch.log(fo.twopi), dim=1) + logj.squeeze(1) - torch.sum(torch.log(fo.p.target_scale))


def test_one_row_each_for_the_other_front_ends():
    K = 3
    # the generic route: the same network behind a module the envelope does not know, against the fused value
    sm, _, _ = _seeded_score_model(5, 3, [64, 100], "VESDE", False, 23)
    gm = D.ScoreModel(WrappedMLP(sm.model), sm.sde, no_sigma=False, hutchinson=True).eval()
    sm.hutch = True
    assert not gm._fusable() and sm._fusable()
    torch.manual_seed(2)
    x0, c = torch.randn(40, 5, device=DEV) * 0.5, torch.randn(40, 3, device=DEV)
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / 4}
    torch.manual_seed(9)
    la = sm.log_prob(x0, conditional=c, method="midpoint", options=opts, num_probes=K)
    torch.manual_seed(9)
    lb = gm.log_prob(x0, conditional=c, method="midpoint", options=opts, num_probes=K)
    assert lb.shape == (40, 1) and gm.e.shape == (40, K, 5) and torch.equal(gm.e, sm.e)
    assert _logp_err(lb, la.cpu()) < LOGP_TOL
    # a population wrapper: the affine map in the kernel's prologue, dopri5 as the reference fixes it there
    torch.manual_seed(3)
    shift, scale = torch.randn(5), torch.rand(5) + 0.5
    sm0, _, _ = _seeded_score_model(5, 0, [64, 100], "VESDE", False, 24)
    pm = D.PopulationModelDiffusion(model=sm0.model, sde=sm0.sde, shift=shift, scale=scale, hutchinson=True).to(DEV).eval()
    xp = (torch.randn(33, 5) * 0.5 * scale + shift).to(DEV)
    torch.manual_seed(6)
    lp = pm.log_prob(xp, atol=1e-4, rtol=1e-4, num_probes=K)
    e = pm.score_model.e
    assert lp.shape == (33, 1) and e.shape == (33, K, 5)
    sm0.hutch = True
    torch.manual_seed(6)
    want = sm0.log_prob((xp - shift.to(DEV)) / scale.to(DEV), atol=1e-4, rtol=1e-4, method="dopri5", options=None, num_probes=K)
    assert torch.equal(sm0.e, e) and _logp_err(lp, want.cpu()) < ADAPT_TOL
    # the flows: the mean of the K single-probe calls' divergences (same probes through probe="philox": probe 0 is the
    # single-probe stream's; the K-probe value against the three K = 1 launches with the probes of the fill)
    torch.manual_seed(9)
    f = F.ODEFlow(6, [128, 128], target_shift=torch.randn(6), target_scale=torch.rand(6) + 0.5).eval().to(DEV)
    g = F.ConditionalODEFlow(5, 3, [64, 100]).eval().to(DEV)
    fo = {"step_size": 0.25}
    for flow, args in ((f, (torch.randn(29, 6, device=DEV),)), (g, (torch.randn(29, 5, device=DEV), torch.randn(29, 3, device=DEV)))):
        kw = dict(method="rk4", options=fo, hutchinson=True, probe="philox", seed=8)
        lpk = flow.log_prob(*args, num_probes=K, **kw)
        assert lpk.shape == (29,) and torch.equal(lpk, flow.log_prob(*args, num_probes=K, **kw))
        assert torch.equal(flow.log_prob(*[a[5:20].contiguous() for a in args], num_probes=K, sample_offset=5, **kw), lpk[5:20])
        assert torch.equal(flow.log_prob(*args, num_probes=1, **kw), flow.log_prob(*args, **kw))
        # against the single-probe op, probe by probe
        Dn = flow.target_dimension
        x = (args[0] - flow.target_shift) / flow.target_scale
        cond = flow._norm_cond(args[1]) if len(args) > 1 else None
        probes = _native.probe_fill(29, K, Dn, 8, 0, DEV)
        t_span = torch.tensor([0.0, 1.0], dtype=torch.float32)
        singles = [odeint.solve(flow, x, t_span, "rk4", fo, MODE_HUTCH, 1e-5, 1e-5, cond=cond, probe=probes[:, k].contiguous())
                   for k in range(K)]
        xT = singles[0][0]
        logj = torch.stack([s[1] for s in singles]).mean(dim=0)
        want = torch.sum(-0.5 * xT ** 2 - 0.5 * math.log(2 * math.pi), dim=1) + logj - torch.sum(torch.log(flow.target_scale))
        assert _logp_err(lpk, want.cpu()) < LOGP_TOL
        # and against the float64 oracle of the flow (its velocity network and stepper; the mean of the K probes' p^T J p by
        # autograd), which shares no code with the library
        want64 = _flow_oracle_log_prob(flow, [a.cpu() for a in args], probes.cpu(), fo)
        err = _logp_err(lpk, want64.float())
        print(f"{type(flow).__name__}.log_prob(num_probes={K}) against the float64 oracle: {err:.3g}")
        assert err < LOGP_TOL
