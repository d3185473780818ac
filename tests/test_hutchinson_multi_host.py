"""CPU tier of the K-probe Hutchinson log-density: the probes' host twin (ff_probe_fill_host, csrc/ff_probe.hip) against
tests/_philox.py, the argument rules of the C entry points and of ``num_probes``, the launcher's rule for K probes as
ff_mlp_launch_kind states it, and -- from the host twin's probes and the float64 oracle -- what the feature is for: the
variance of the estimate falls as 1 / K and its mean stays on the exact trace.  That last test is also the one that
catches two probe indices colliding (two probes of a sample equal: the variance would not fall)."""
import ctypes
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from tests._philox import normals
from tests._util import score_oracle

ROOT = Path(__file__).resolve().parent.parent
KS = [1, 2, 15]
DS = [1, 5, 16]
UNAMBIGUOUS = 1e-6          # |z| below this: libm and the device may disagree on a sign (they agree to 2e-6 on z)


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


def probe_indices(K):
    return [_native.PROBE_NOISE_INDEX] + [_native.HUTCH_PROBE_NOISE_BASE + k for k in range(1, K)]


def host_fill(B, K, D, seed, offset, scale=1.0):
    out = _native.probe_fill(B, K, D, seed, offset, "cpu", scale=scale)
    assert out.shape == (B, K, D) and out.dtype == torch.float32
    return out.numpy()


# ---- the probes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2 ** 33 + 7])
@pytest.mark.parametrize("D_", DS)
@pytest.mark.parametrize("K", KS)
def test_host_probes_are_the_signs_of_the_streams_normals(K, D_, offset):
    B, seed = 9, 4242 + 17 * K + D_
    z = normals(seed, offset, B, D_, probe_indices(K))                    # [K, B, D]
    assert np.abs(z).min() >= UNAMBIGUOUS, "choose another seed: a normal this close to zero has no certain sign"
    for scale in (1.0, float(np.float32(K ** -0.5))):
        got = host_fill(B, K, D_, seed, offset, scale)
        want = (np.where(z >= 0, 1.0, -1.0).astype(np.float32) * np.float32(scale)).transpose(1, 0, 2)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (K, D_, offset, scale)
    got = host_fill(B, K, D_, seed, offset)
    # probe 0 is the single-probe stream: FF_PROBE_NOISE_INDEX, whatever K
    single = np.where(normals(seed, offset, B, D_, [_native.PROBE_NOISE_INDEX])[0] >= 0, 1.0, -1.0).astype(np.float32)
    assert np.array_equal(got[:, 0], single) and np.array_equal(host_fill(B, 1, D_, seed, offset)[:, 0], single)
    # rows are keyed by the global row: a slice with sample_offset is the rows of the whole
    lo, hi = 3, 8
    assert np.array_equal(host_fill(hi - lo, K, D_, seed, offset + lo), got[lo:hi])
    # probe k does not depend on K: the K = 2 probes are the first two of any larger set
    assert np.array_equal(host_fill(B, min(K, 2), D_, seed, offset), got[:, :min(K, 2)])


def test_probe_index_range_is_reserved_below_the_momenta():
    assert _native.HUTCH_PROBE_NOISE_BASE + _native.MAX_HUTCH_PROBES < _native.MOMENTUM_NOISE_BASE
    assert _native.MOMENTUM_NOISE_BASE + _native.MAX_MOMENTA < _native.TRACE_PROBE_NOISE_BASE < _native.PROBE_NOISE_INDEX
    header = (ROOT / "include" / "flowfusion_amd.h").read_text()
    assert f"#define FF_HUTCH_PROBE_NOISE_BASE 0x{_native.HUTCH_PROBE_NOISE_BASE:08X}u" in header
    assert f"#define FF_MAX_HUTCH_PROBES {_native.MAX_HUTCH_PROBES}" in header


# ---- argument rules ----------------------------------------------------------------------------------------------------------
def test_both_entry_points_are_exported_and_refuse_bad_arguments():
    L = _native.lib()
    header = (ROOT / "include" / "flowfusion_amd.h").read_text()
    for name in ("ff_probe_fill", "ff_probe_fill_host"):
        assert hasattr(L, name) and f"int {name}(float* out" in header
    buf = torch.zeros(8)
    p = buf.data_ptr()
    assert L.ff_probe_fill_host(p, 1, 2, 4, 0, 0, 1.0) == _native.FF_OK and bool((buf.abs() == 1).all())
    bad, ok = _native.FF_ERR_BADARG, _native.FF_OK
    # the host twin: a host buffer is its own memory
    fn = L.ff_probe_fill_host
    assert fn(None, 1, 1, 4, 0, 0, 1.0) == bad and fn(p, -1, 1, 4, 0, 0, 1.0) == bad
    assert fn(p, 1, 0, 4, 0, 0, 1.0) == bad and fn(p, 1, -3, 4, 0, 0, 1.0) == bad
    assert fn(p, 1, _native.MAX_HUTCH_PROBES + 1, 4, 0, 0, 1.0) == bad and fn(p, 1, 1, 0, 0, 0, 1.0) == bad
    assert fn(p, 0, 1, 4, 0, 0, 1.0) == ok                                 # an empty batch is nothing to do
    # the device entry point never sees an address it could write to: a null pointer (refused in every case), or a
    # host address with an EMPTY batch -- the argument rules come before the empty-batch return, and should one of them
    # regress the call returns FF_OK (the assertion fails) without a launch
    fn = L.ff_probe_fill
    assert fn(None, 1, 1, 4, 0, 0, 1.0, None) == bad and fn(None, -1, 1, 4, 0, 0, 1.0, None) == bad
    assert fn(p, 0, 0, 4, 0, 0, 1.0, None) == bad and fn(p, 0, -3, 4, 0, 0, 1.0, None) == bad
    assert fn(p, 0, _native.MAX_HUTCH_PROBES + 1, 4, 0, 0, 1.0, None) == bad and fn(p, 0, 1, 0, 0, 0, 1.0, None) == bad
    assert fn(p, 0, 1, 4, 0, 0, 1.0, None) == ok
    with pytest.raises(ValueError, match="num_probes"):
        _native.probe_fill(3, 0, 4, 0, 0, "cpu")
    assert _native.probe_fill(0, 3, 4, 0, 0, "cpu").shape == (0, 3, 4)


def _score_model(D_=16, units=(256,) * 4, **kw):
    torch.manual_seed(3)
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=0, embedding_dimensions=8, units=list(units)), D.VPSDE(),
                        no_sigma=True, **kw).eval()


def test_num_probes_refusals_name_what_to_do():
    x = torch.randn(4, 16)
    opts = dict(method="rk4", options={"step_size": 0.25})
    with pytest.raises(ValueError, match="hutchinson=True"):
        _score_model().log_prob(x, num_probes=3, **opts)                               # exact-trace model
    with pytest.raises(ValueError, match="hpp_rank"):
        _score_model(hutchpp=True).log_prob(x, num_probes=3, **opts)
    with pytest.raises(ValueError, match="xt_vecs"):
        _score_model(xtrace=True).solve_odes_forward(x, num_probes=2, **opts)
    with pytest.raises(ValueError, match="at least one"):
        _score_model(hutchinson=True).log_prob(x, num_probes=0, **opts)
    with pytest.raises(ValueError, match="num_probes <= 15"):                          # 16-column tile: 1 + K <= 16
        _score_model(hutchinson=True).log_prob(x, num_probes=16, **opts)
    with pytest.raises(ValueError, match="num_probes <= 31"):                          # 32-column tile
        _score_model(4, (64, 64), hutchinson=True).log_prob(torch.randn(4, 4), num_probes=32, **opts)
    for prec in ("bf16x2", "bf16x3"):
        with pytest.raises(ValueError, match="precision='f32'"):
            _score_model(hutchinson=True, precision=prec).log_prob(x, num_probes=2, **opts)
    pm = D.PopulationModelDiffusion(model=_score_model().model, sde=D.VPSDE())
    with pytest.raises(ValueError, match="hutchinson=True"):
        pm.log_prob(x, num_probes=2)
    pc = D.PopulationModelDiffusionConditional(model=D.MLP(4, 2, 8, [64, 64]), sde=D.VPSDE())
    with pytest.raises(ValueError, match="hutchinson=True"):
        pc.log_prob(torch.randn(3, 4), torch.randn(3, 2), num_probes=2)
    f, g = F.ODEFlow(4, [64, 64]), F.ConditionalODEFlow(4, 2, [64, 64])
    with pytest.raises(ValueError, match="hutchinson=True"):
        f.log_prob(torch.randn(3, 4), method="rk4", options={"step_size": 0.5}, num_probes=2)
    with pytest.raises(ValueError, match="hutchinson=True"):
        g.solve_ode_forward(torch.randn(3, 4), torch.randn(3, 2), method="rk4", options={"step_size": 0.5}, num_probes=2)
    with pytest.raises(ValueError, match="num_probes <= 31"):
        f.log_prob(torch.randn(3, 4), method="rk4", options={"step_size": 0.5}, hutchinson=True, num_probes=40)
    # the keyword is keyword-only on the front ends whose positional lists the reference fixes
    with pytest.raises(TypeError):
        pm.log_prob(x, 1e-5, 1e-5, 2)


def test_op_shape_rule_for_k_probes():
    chk = _native._chk_probe
    chk(None, 5, 4, _native.MODE_HUTCH, 3)
    chk(torch.zeros(5, 4), 5, 4, _native.MODE_HUTCH, 0)
    chk(torch.zeros(5, 4), 5, 4, _native.MODE_HUTCH, 1)
    chk(torch.zeros(5, 1, 4), 5, 4, _native.MODE_HUTCH, 1)
    chk(torch.zeros(5, 3, 4), 5, 4, _native.MODE_HUTCH, 3)
    for probe, count in ((torch.zeros(5, 4), 3), (torch.zeros(5, 3, 4), 0), (torch.zeros(5, 3, 4), 2), (torch.zeros(5, 12), 3),
                         (torch.zeros(3, 5, 4), 3)):
        with pytest.raises(RuntimeError, match="probe has shape"):
            chk(probe, 5, 4, _native.MODE_HUTCH, count)
    assert _native.probe_count(torch.zeros(5, 3, 4)) == 3 and _native.probe_count(torch.zeros(5, 4)) == 0
    assert _native.probe_count(None) == 0


# ---- the launcher's rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,units", [(16, [256] * 4), (2, [128] * 3), (4, [64, 64])])
def test_launch_kind_counts_tiles_of_one_plus_k_columns(dim, units, monkeypatch):
    """(batch, HUTCH, K) takes the kernel(s) that as many TILES take in any other mode: ceil(batch / (tile / (1 + K)))
    tiles, stated here through single-probe batches of the same tile count (tile / 2 samples per tile)."""
    monkeypatch.delenv("FF_COOP", raising=False)
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    plan = _native.make_plan(dim, 0, units, _native.MODE_HUTCH)
    tile = int(plan.tile)
    seen = set()
    for K in [k for k in (1, 2, 3, 7, 15, 31) if k + 1 <= tile]:
        spt = tile // (1 + K)
        for tiles in (1, 2, 700, 1024, 1025, 2048, 2049, 2148, 3071, 3072, 3073, 3200, 4096, 4100, 6144, 6200, 9000):
            for batch in (tiles * spt, tiles * spt - spt + 1):
                kind = _native.launch_kind(plan, batch, _native.MODE_HUTCH, K)
                assert kind == _native.launch_kind(plan, tiles * (tile // 2), _native.MODE_HUTCH, 0), (K, tiles, batch)
                seen.add(kind)
        assert _native.launch_kind(plan, 77, _native.MODE_HUTCH, 1) == _native.launch_kind(plan, 77, _native.MODE_HUTCH, 0)
    if units[0] >= 128:         # (the 64-wide kernels have no cooperative twin: one kind only)
        assert seen == {_native.LAUNCH_ONE_WAVE, _native.LAUNCH_TWIN, _native.LAUNCH_ONE_WAVE_AND_TWIN}
    else:
        assert seen == {_native.LAUNCH_ONE_WAVE}
    for K in (tile, tile + 5):
        with pytest.raises(RuntimeError, match="FF_ERR_BADARG"):
            _native.launch_kind(plan, 100, _native.MODE_HUTCH, K)
    assert _native.launch_kind(plan, 100, _native.MODE_HUTCH, tile - 1) in seen


# ---- what it is for: variance 1 / K, no bias ---------------------------------------------------------------------------------
def test_variance_falls_as_one_over_k_and_the_mean_stays_on_the_exact_trace():
    """8-d VP score model, 2 x 128, four rk4 steps, float64 oracle; 64 rows x 64 probe draws (seeds) from the host twin.
    A K-probe estimate is the mean of the first K per-probe estimates of a draw (the probes' indices do not depend on K).
    v_K = variance over the draws, averaged over the rows: v_1 / v_K within [K / 1.5, 1.5 K] (with torch's probes the oracle
    gives 3.12 and 7.08); |mean - exact| within 5 standard errors of the mean over rows and draws (0.3 .. 0.8 there)."""
    D_, R, S, KMAX = 8, 64, 64, 7
    torch.manual_seed(41)
    sm = D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=0, embedding_dimensions=8, units=[128, 128]), D.VPSDE(), no_sigma=True)
    meta = dict(D=D_, C=0, E=8, units=[128, 128], sde="VPSDE", sde_kw={}, no_sigma=True)
    so64 = score_oracle(meta, {k: v.detach().clone() for k, v in sm.state_dict().items()}, torch.float64)
    x = (torch.randn(R, D_) * 0.8 + 0.3).double()
    opts = {"step_size": (1.0 - float(sm.sde.epsilon)) / 4}
    probes = np.stack([host_fill(R, KMAX, D_, seed, 0) for seed in range(S)])          # [S, R, K, D]
    assert np.abs(np.stack([normals(seed, 0, R, D_, probe_indices(KMAX)) for seed in range(S)])).min() >= UNAMBIGUOUS
    e = torch.from_numpy(probes).double().reshape(S * R * KMAX, D_)
    xs = x[None, :, None, :].expand(S, R, KMAX, D_).reshape(S * R * KMAX, D_)
    with torch.no_grad():
        _, per_probe = so64.solve_odes_forward(xs, None, "rk4", opts, "hutch", e)
        _, exact = so64.solve_odes_forward(x, None, "rk4", opts, "exact", None)
    per_probe = per_probe.reshape(S, R, KMAX).numpy()
    exact = exact.reshape(R).numpy()
    var = {}
    for K in (1, 3, 7):
        est = per_probe[:, :, :K].mean(axis=2)                                          # [S, R]
        var[K] = est.var(axis=0, ddof=1).mean()
        by_draw = (est - exact[None, :]).mean(axis=1)                                   # [S]: mean over the rows
        se = by_draw.std(ddof=1) / math.sqrt(S)
        print(f"K={K}: v_K={var[K]:.6g} ratio={var[1] / var[K]:.3f} bias={by_draw.mean():.3g} = {abs(by_draw.mean()) / se:.2f} SE")
        assert abs(by_draw.mean()) <= 5 * se, (K, by_draw.mean(), se)
    for K in (3, 7):
        assert K / 1.5 <= var[1] / var[K] <= 1.5 * K, (K, var)


def test_launcher_refuses_what_it_cannot_carry_before_touching_a_gpu():
    """ff_mlp_ode_launch with tangent_count = K in FF_MODE_HUTCH: more probes than the tile has tangent columns is
    FF_ERR_BADARG; a split-precision plan (one probe per sample; it would read [B, K, D] as [B, D]) is FF_ERR_UNSUPPORTED.
    Both answers come from the argument checks, ahead of the empty-batch return: the batch here IS empty, so a regression
    of either check returns FF_OK (and fails the assertion) instead of launching a kernel on these host addresses."""
    L = _native.lib()
    buf = torch.zeros(64)
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.probe = a.dlogp_out = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode = 0, 1, _native.MODE_HUTCH
    f32 = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH)
    split = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH, precision=_native.PREC_BF16X2)
    for count, plan, want in ((16, f32, _native.FF_ERR_BADARG), (40, f32, _native.FF_ERR_BADARG),
                              (2, split, _native.FF_ERR_UNSUPPORTED), (15, split, _native.FF_ERR_UNSUPPORTED)):
        a.tangent_count = count
        assert L.ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), None) == want, count
