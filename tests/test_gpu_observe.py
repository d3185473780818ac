"""GPU tier: the log-density of noisy observations over K noise draws -- the two streaming kernels of
csrc/ff_observe.hip at their corners, and ``log_prob_noisy`` of the score models, the flows and the population wrapper /
``log_prob_noisy_sharded`` around the model's own log-density.

Anchors: torch's own fp32 ``x - noise_std * z`` of ``ff_normal_fill``'s normals for what expand writes (bitwise);
``torch.logsumexp`` in float64 on the same bits for the reduction (one fp32 rounding of a double result); ``log_prob``
itself at ``noise_std = 0, num_draws = 1`` (bitwise); the float64 oracle on the device's own expanded rows end to end; the
closed-form convolution of two Gaussians (tests/test_observe_host.py); and bitwise equalities -- chunks, slices, shards,
re-runs."""
import ctypes
import math

import numpy as np
import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import diffusion as Dm
from flowfusion_amd import flow as Fm
from flowfusion_amd.distributed import log_prob_noisy_sharded
from tests.test_observe_host import closed_form_inputs, exact_observed
from tests._util import flow_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = _native.OBS_NOISE_BASE
SENTINEL = -7.5e33
GUARD = 64
DS = [1, 3, 4, 16, 33]
CS = [0, 2, 5]
KS = [1, 3, 8, 17]
BS = [1, 37, 1000]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arena(n, misalign):
    """(arena, view of n floats): sentinel everywhere, the view 16-byte aligned or one float past alignment."""
    a = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV)
    lo = GUARD + (1 if misalign else 0)
    v = a[lo:lo + n]
    assert v.data_ptr() % 16 == (4 if misalign else 0)
    return a, v


def _guards_ok(arena, view):
    lo = (view.data_ptr() - arena.data_ptr()) // 4
    return bool((arena[:lo] == SENTINEL).all()) and bool((arena[lo + view.numel():] == SENTINEL).all())


def _placed(t, misalign):
    """A copy of ``t`` at a 16-byte aligned address or one float past it."""
    if t is None:
        return None
    _, v = _arena(t.numel(), misalign)
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def _draws(B, D, K, seed, offset):
    """[B, K, D]: noise draw k of point r, from ff_normal_fill under noise index BASE + k."""
    z = torch.empty(B, K, D, device=DEV)
    for k in range(K):
        z[:, k] = _native.normal_fill(B, D, seed, offset, DEV, noise_index=BASE + k)
    return z


def _composition(x, std, K, seed, offset):
    """The torch statement of the expansion: K fills, a separate multiply, a separate subtract -> [B K, D]."""
    B, D = x.shape
    prod = std.view(-1, 1, D) * _draws(B, D, K, seed, offset)
    return (x.view(B, 1, D) - prod).reshape(B * K, D)


def _expand_raw(x, std, cond, K, seed, offset, misalign):
    """The C entry point on inputs and outputs placed in sentinel arenas; returns (y, cond_out) after checking that no
    word outside the outputs was written."""
    B, D = x.shape
    C = 0 if cond is None else cond.shape[1]
    xs, ss, cs = _placed(x, misalign), _placed(std, misalign), _placed(cond, misalign)
    ya, y = _arena(B * K * D, misalign)
    ca, co = _arena(max(B * K * C, 1), misalign)
    rc = _native.lib().ff_observe_expand(xs.data_ptr(), ss.data_ptr(), 0 if std.dim() == 1 else D, 0 if cs is None else cs.data_ptr(),
                                        B, D, C, K, seed, offset, y.data_ptr(), co.data_ptr() if cond is not None else 0, _stream())
    assert rc == _native.FF_OK
    torch.cuda.synchronize()
    assert _guards_ok(ya, y), (B, D, K, "a word outside y was written")
    if cond is None:
        assert bool((ca == SENTINEL).all())
        return y.view(B * K, D), None
    assert _guards_ok(ca, co[:B * K * C]), (B, D, K, "a word outside cond_out was written")
    return y.view(B * K, D), co[:B * K * C].view(B * K, C)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _reference_lme(lp, K):
    """(out, ess) in float64 torch from the bits of lp [B K]."""
    lw = lp.double().view(-1, K)
    out = torch.logsumexp(lw, dim=1) - math.log(K)
    w = torch.exp(lw - lw.max(dim=1, keepdim=True).values)
    return out, w.sum(1) ** 2 / (w * w).sum(1)


def _within_one_rounding(got, ref):
    """|got - ref| <= 1.2e-7 |ref| + 1e-10: one fp32 rounding of a result computed in double."""
    return bool(((got.double() - ref).abs() <= 1.2e-7 * ref.abs() + 1e-10).all())


# ---- 1. expand, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_expand_bitwise_at_the_corners(D):
    """Every K x B of the lists, each aligned (the 16-byte body where D % 4 == 0) and one float past alignment (the scalar
    body), C and the noise_std layout cycling through their lists: bitwise the torch composition, guard words untouched."""
    g = torch.Generator(device=DEV).manual_seed(100 + D)
    n = 0
    for K in KS:
        for B in BS:
            x = torch.randn(B, D, device=DEV, generator=g) * 2
            for misalign in (False, True):
                C = CS[n % 3]
                per_row = (n // 3) % 2 == 0
                n += 1
                seed, offset = 7 + K, (2 ** 32 + 5 if not misalign else 0)
                std = torch.rand((B, D) if per_row else (D,), device=DEV, generator=g) * 1.5
                cond = torch.randn(B, C, device=DEV, generator=g) if C else None
                y, co = _expand_raw(x, std, cond, K, seed, offset, misalign)
                what = (D, K, B, C, per_row, misalign)
                assert torch.equal(_bits(y), _bits(_composition(x, std, K, seed, offset))), what
                if C:
                    assert torch.equal(_bits(co), _bits(cond.repeat_interleave(K, dim=0))), what
    assert n == 24 and torch.isfinite(y).all()
    # the binding: the same entry point on torch's current stream
    yb, cb = _native.observe_expand(x, std, K, seed, offset, cond)
    assert torch.equal(yb, y) and (cond is None or torch.equal(cb, co))


@pytest.mark.parametrize("D", DS)
def test_expand_zero_noise_empty_batch_and_offsets(D):
    g = torch.Generator(device=DEV).manual_seed(200 + D)
    B, K, seed = 37, 8, 3
    x = torch.randn(B, D, device=DEV, generator=g)
    for std in (torch.zeros(D, device=DEV), torch.zeros(B, D, device=DEV)):
        for misalign in (False, True):
            y, _ = _expand_raw(x, std, None, K, seed, 11, misalign)
            assert torch.equal(y, x.repeat_interleave(K, dim=0))
    y0, c0 = _native.observe_expand(x[:0], torch.zeros(D, device=DEV), K, seed, 0, torch.zeros(0, 2, device=DEV))
    assert y0.shape == (0, D) and c0.shape == (0, 2)
    assert _native.lib().ff_observe_expand(x.data_ptr(), x.data_ptr(), 0, 0, 0, D, 0, K, 1, 0, x.data_ptr(), 0, _stream()) == _native.FF_OK
    # rows [lo, hi) alone with sample_offset + lo: the matching rows of the larger call
    std = torch.rand(B, D, device=DEV, generator=g)
    first = 2 ** 33 + 1
    whole, _ = _native.observe_expand(x, std, K, seed, first)
    for lo, hi in ((0, 1), (5, 20), (36, 37)):
        part, _ = _native.observe_expand(x[lo:hi], std[lo:hi], K, seed, first + lo)
        assert torch.equal(_bits(part), _bits(whole[lo * K:hi * K])), (lo, hi)
    other, _ = _native.observe_expand(x, std, K, seed + 1, first)
    assert not torch.equal(other, whole)


def test_expand_grid_stride_loop_wraps():
    """B K D / 4 = 640,000 lanes of work against a grid capped at 2048 x 256: a second trip; C = 4 takes the 16-byte copy
    of the conditional."""
    B, K, D, C, seed, offset = 40000, 4, 16, 4, 21, 123456789
    assert B * K * (D // 4) > 2048 * 256
    g = torch.Generator(device=DEV).manual_seed(5)
    x, cond = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, C, device=DEV, generator=g)
    std = torch.rand(B, D, device=DEV, generator=g)
    want = _composition(x, std, K, seed, offset)
    for misalign in (False, True):
        y, co = _expand_raw(x, std, cond, K, seed, offset, misalign)
        assert torch.equal(_bits(y), _bits(want)) and torch.equal(co, cond.repeat_interleave(K, dim=0))


# ---- 2. logmeanexp -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8, 17, 4096])
def test_logmeanexp_against_float64(K):
    g = torch.Generator(device=DEV).manual_seed(300 + K)
    for B in BS:
        lp = torch.randn(B * K, device=DEV, generator=g) * 4 - 30
        lp[:K] = lp[0].clone()                                               # K equal values
        if B > 1:
            lp[K:2 * K] *= 25                                                # a spread of hundreds of nats
        ref, ref_ess = _reference_lme(lp, K)
        for misalign in (False, True):
            oa, out = _arena(B, False)
            ea, ess = _arena(B, False)
            rc = _native.lib().ff_logmeanexp(_placed(lp, misalign).data_ptr(), B, K, out.data_ptr(), ess.data_ptr(), _stream())
            assert rc == _native.FF_OK
            torch.cuda.synchronize()
            assert _guards_ok(oa, out) and _guards_ok(ea, ess)
            assert _within_one_rounding(out, ref) and _within_one_rounding(ess, ref_ess), (K, B, misalign)
            assert bool(((ess > 0) & (ess <= K * (1 + 1e-6))).all())
            if K == 1:
                assert torch.equal(_bits(out), _bits(lp)) and bool((ess == 1).all())
        # the binding; without ess; a row alone or in another batch gives the same bits
        got = _native.logmeanexp(lp, K)
        assert torch.equal(got, out)
        for lo, hi in ((0, 1), (B // 2, B), (B - 1, B)):
            assert torch.equal(_native.logmeanexp(lp[lo * K:hi * K].clone(), K), got[lo:hi]), (K, B, lo, hi)
        assert torch.equal(_native.logmeanexp(lp.view(-1, 1), K), got)


@pytest.mark.parametrize("K", [1, 3, 8, 17, 4096])
def test_logmeanexp_non_finite_rows_follow_logsumexp(K):
    B = 5
    g = torch.Generator(device=DEV).manual_seed(400 + K)
    lp = torch.randn(B * K, device=DEV, generator=g) * 2
    lp[K - 1] = float("-inf")                               # point 0: one draw of weight zero
    lp[K:2 * K] = float("-inf")                             # point 1: every draw of weight zero
    lp[2 * K + K // 2] = float("nan")                       # point 2: a NaN
    lp[3 * K + K // 3] = float("inf")                       # point 3: a +inf entry
    ref, ref_ess = _reference_lme(lp, K)
    assert ref[1] == float("-inf") and torch.isnan(ref[2]) and ref[3] == float("inf")
    ess = torch.empty(B, device=DEV)
    got = _native.logmeanexp(lp, K, None, ess)
    assert got[1] == float("-inf") and torch.isnan(ess[1]) and torch.isnan(got[2]) and torch.isnan(ess[2])
    assert got[3] == float("inf")
    keep = [4] if K == 1 else [0, 4]
    assert _within_one_rounding(got[keep], ref[keep]) and _within_one_rounding(ess[keep], ref_ess[keep])
    if K == 1:
        assert got[0] == float("-inf")


# ---- the models of the end-to-end tests ----------------------------------------------------------------------------------------
B0 = 37


def _stats(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 0.5, torch.rand(n, generator=g) + 0.5


def _score(D, hutchinson=False):
    torch.manual_seed(20 + D)
    units = [64, 64] if D == 3 else [256] * 4
    return Dm.ScoreModel(Dm.MLP(D, 0, 8, units), Dm.VPSDE(), no_sigma=True, hutchinson=hutchinson).eval()


def _flow(D):
    torch.manual_seed(30 + D)
    return Fm.ODEFlow(D, [64, 64] if D == 3 else [256] * 3, torch.nn.SiLU, *_stats(D, 31)).eval()


def _cflow(D):
    torch.manual_seed(40 + D)
    C = 2 if D == 3 else 6
    return Fm.ConditionalODEFlow(D, C, [64, 64] if D == 3 else [256] * 3, torch.nn.SiLU, *_stats(D, 41), *_stats(C, 42)).eval(), C


def _population(D):
    torch.manual_seed(50 + D)
    units = [64, 64] if D == 3 else [256] * 4
    return Dm.PopulationModelDiffusion(Dm.MLP(D, 0, 8, units), Dm.VPSDE(), *_stats(D, 51), no_sigma=True).eval()


def _points(D, seed, C=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B0, D, generator=g)
    return (x, torch.randn(B0, C, generator=g)) if C else x


SCORE_RK4 = dict(method="rk4", options={"step_size": (1.0 - 1e-3) / 10})
FLOW_RK4 = dict(method="rk4", options={"step_size": 0.25})


# ---- 3. degenerate identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 16])
def test_zero_noise_one_draw_is_log_prob_bitwise(D):
    """y = x - 0 z = x and the mean of one value is that value: the same solve on the same bits."""
    x = _points(D, 60 + D).to(DEV)
    sm = _score(D).to(DEV)
    for solver in (SCORE_RK4, {}):                                          # a fixed grid; the default adaptive method
        want = sm.log_prob(x, **solver)
        got, ess = sm.log_prob_noisy(x, 0.0, num_draws=1, seed=5, return_ess=True, **solver)
        assert got.shape == (B0, 1) and ess.shape == (B0,) and torch.equal(_bits(got), _bits(want)) and bool((ess == 1).all())
        assert torch.equal(sm.log_prob_noisy(x, torch.zeros(B0, D, device=DEV), num_draws=1, **solver), want)
    f = _flow(D).to(DEV)
    for solver in (FLOW_RK4, {}):
        want = f.log_prob(x, **solver)
        got = f.log_prob_noisy(x, 0.0, num_draws=1, seed=5, **solver)
        assert got.shape == (B0,) and torch.equal(_bits(got), _bits(want))
    fc, C = _cflow(D)
    fc = fc.to(DEV)
    xc, c = (t.to(DEV) for t in _points(D, 61 + D, C))
    for solver in (FLOW_RK4, {}):
        want = fc.log_prob(xc, c, **solver)
        got = fc.log_prob_noisy(xc, torch.zeros(D, device=DEV), c, num_draws=1, **solver)
        assert got.shape == (B0,) and torch.equal(_bits(got), _bits(want))
    pm = _population(D).to(DEV)
    xp = x * pm.scale + pm.shift
    want = pm.log_prob(xp)
    got = pm.log_prob_noisy(xp, 0.0, num_draws=1)
    assert got.shape == (B0, 1) and torch.equal(_bits(got), _bits(want)) and torch.isfinite(got).all()


# ---- 4. against float64 ------------------------------------------------------------------------------------------------------------
def _check_against_float64(got, per_row, K, what):
    """Log-sum-exp is 1-Lipschitz in the max norm, so the per-row bar of the log-density tests carries through:
    |diff| <= 2e-5 max(1, max_k |lp_k|) per point."""
    lp = per_row.double().numpy().reshape(-1, K)
    m = lp.max(1)
    want = m + np.log(np.exp(lp - m[:, None]).sum(1)) - math.log(K)
    bar = 2e-5 * np.maximum(1.0, np.abs(lp).max(1))
    diff = np.abs(got.double().cpu().numpy().reshape(-1) - want)
    print(f"\n[{what}] K={K}: max diff {diff.max():.3e}, smallest bar {bar.min():.3e}")
    assert (diff <= bar).all(), (what, K, diff.max())


@pytest.mark.parametrize("K", [3, 8])
def test_score_model_against_the_float64_oracle(K):
    from oracle import flowfusion_oracle as O
    D, seed, first = 3, 17, 1000
    sm = _score(D)
    params = O.mlp_params_from_state_dict({k: v.detach().clone() for k, v in sm.state_dict().items()})
    so64 = O.ScoreOracle(params, O.VP(dtype=torch.float64), no_sigma=True, dtype=torch.float64)
    sm = sm.to(DEV)
    x = _points(D, 70)
    std = torch.rand(B0, D, generator=torch.Generator().manual_seed(71)) * 0.5 + 0.05
    y, _ = _native.observe_expand(x.to(DEV), std.to(DEV), K, seed, first)      # the device's own draws
    per_row = so64.log_prob(y.cpu().double(), None, "rk4", SCORE_RK4["options"], "exact")
    got = sm.log_prob_noisy(x.to(DEV), std.to(DEV), num_draws=K, seed=seed, sample_offset=first, **SCORE_RK4)
    assert got.shape == (B0, 1)
    _check_against_float64(got, per_row, K, "score model, exact trace")


@pytest.mark.parametrize("K", [3, 8])
def test_flow_against_the_float64_oracle(K):
    D, seed, first = 16, 18, 2 ** 32 + 3
    f = _flow(D)
    fo64 = flow_oracle({k: v.detach().clone() for k, v in f.state_dict().items()}, torch.float64)
    f = f.to(DEV)
    x = _points(D, 72) * f.target_scale.cpu() + f.target_shift.cpu()
    std = (torch.rand(B0, D, generator=torch.Generator().manual_seed(73)) * 0.5 + 0.05) * f.target_scale.cpu()
    y, _ = _native.observe_expand(x.to(DEV), std.to(DEV), K, seed, first)
    per_row = fo64.log_prob(y.cpu().double(), None, "rk4", FLOW_RK4["options"])
    got = f.log_prob_noisy(x.to(DEV), std.to(DEV), num_draws=K, seed=seed, sample_offset=first, **FLOW_RK4)
    assert got.shape == (B0,)
    _check_against_float64(got, per_row, K, "flow")


# ---- 5. determinism: all bitwise, fixed grid ---------------------------------------------------------------------------------------
def test_chunks_slices_shards_and_reruns_are_bitwise():
    D, K, seed, first = 16, 8, 5, 2 ** 32 + 9
    sm = _score(D).to(DEV)
    x = _points(D, 80).to(DEV)
    std = (torch.rand(B0, D, generator=torch.Generator().manual_seed(81)) * 0.4).to(DEV)
    run = lambda **kw: sm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, return_ess=True, **SCORE_RK4, **kw)
    lp, ess = run()
    assert lp.shape == (B0, 1) and ess.shape == (B0,) and torch.isfinite(lp).all()
    assert bool(((ess > 0) & (ess <= K * (1 + 1e-6))).all())
    for chunk in (1, 7):
        a, b = run(chunk_points=chunk)
        assert torch.equal(a, lp) and torch.equal(b, ess), chunk
    a, b = run()                                                            # the same seed twice
    assert torch.equal(a, lp) and torch.equal(b, ess)
    old, odeint.OBSERVE_CHUNK_ROWS = odeint.OBSERVE_CHUNK_ROWS, 10 * K      # the default rule: chunk_points K <= that many rows
    try:
        a, b = run()
    finally:
        odeint.OBSERVE_CHUNK_ROWS = old
    assert torch.equal(a, lp) and torch.equal(b, ess)
    for lo, hi in ((0, 1), (11, 30), (36, 37)):                             # a rank's rows, computed alone
        a = sm.log_prob_noisy(x[lo:hi], std[lo:hi], num_draws=K, seed=seed, sample_offset=first + lo, **SCORE_RK4)
        assert torch.equal(a, lp[lo:hi]), (lo, hi)
    other = sm.log_prob_noisy(x, std, num_draws=K, seed=seed + 1, sample_offset=first, **SCORE_RK4)
    assert (other != lp).float().mean() > 0.9                               # another seed, other noise
    # the sharded entry point in one process (sample_offset = 0 there)
    want, want_ess = sm.log_prob_noisy(x, std, num_draws=K, seed=seed, return_ess=True, **SCORE_RK4)
    assert torch.equal(log_prob_noisy_sharded(sm, x, std, seed=seed, num_draws=K, **SCORE_RK4), want)
    got = log_prob_noisy_sharded(sm, local_x=x, local_noise_std=std, n_total=B0, seed=seed, num_draws=K, return_ess=True, **SCORE_RK4)
    assert torch.equal(got[0], want) and torch.equal(got[1], want_ess)
    (a, b), span = log_prob_noisy_sharded(sm, x, std, seed=seed, num_draws=K, return_ess=True, gather=False, **SCORE_RK4)
    assert span == (0, B0) and torch.equal(a, want) and torch.equal(b, want_ess)
    f = _flow(D).to(DEV)
    wf = f.log_prob_noisy(x, std, num_draws=K, seed=seed, **FLOW_RK4)
    assert torch.equal(f.log_prob_noisy(x, std, num_draws=K, seed=seed, chunk_points=7, **FLOW_RK4), wf)
    assert torch.equal(log_prob_noisy_sharded(f, x, std, seed=seed, num_draws=K, **FLOW_RK4), wf)


def test_hutchinson_models_are_chunk_invariant_too():
    """The probes of the expanded rows are keyed by the seed and the expanded global row, not drawn on the host."""
    D, K, seed, first = 16, 8, 6, 12345
    x = _points(D, 82).to(DEV)
    std = (torch.rand(D, generator=torch.Generator().manual_seed(83)) * 0.4).to(DEV)
    hm = _score(D, hutchinson=True).to(DEV)
    for probes in (1, 3):
        run = lambda **kw: hm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, num_probes=probes, **SCORE_RK4, **kw)
        lp = run()
        assert torch.isfinite(lp).all() and torch.equal(run(), lp)
        for chunk in (1, 7):
            assert torch.equal(run(chunk_points=chunk), lp), (probes, chunk)
    # the expanded rows with their philox probes, by hand
    y, _ = _native.observe_expand(x, std, K, seed, first)
    rows = hm.log_prob(y, probe="philox", seed=seed, sample_offset=first * K, num_probes=3, **SCORE_RK4)
    assert torch.equal(_native.logmeanexp(rows, K).view(-1, 1), lp)
    f = _flow(D).to(DEV)
    run = lambda **kw: f.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, hutchinson=True, **FLOW_RK4, **kw)
    assert torch.equal(run(chunk_points=5), run())
    assert not torch.equal(run(), f.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, **FLOW_RK4))


def test_adaptive_methods_refuse_chunks_and_solve_all_rows_at_once():
    D, K = 3, 4
    sm, x = _score(D).to(DEV), _points(D, 84).to(DEV)
    with pytest.raises(ValueError, match="chunk_points"):
        sm.log_prob_noisy(x, 0.1, num_draws=K, chunk_points=8)
    y, _ = _native.observe_expand(x, torch.full((D,), 0.1, device=DEV), K, 9, 0)
    want = _native.logmeanexp(sm.log_prob(y), K).view(-1, 1)                 # dopri5 on the 148 rows as one batch
    assert torch.equal(sm.log_prob_noisy(x, 0.1, num_draws=K, seed=9), want)
    pm = _population(D).to(DEV)
    xp = x * pm.scale + pm.shift
    yp, _ = _native.observe_expand(xp, torch.full((D,), 0.1, device=DEV), K, 9, 0)
    got, ess = pm.log_prob_noisy(xp, 0.1, num_draws=K, seed=9, return_ess=True)
    assert torch.equal(got, _native.logmeanexp(pm.log_prob(yp), K).view(-1, 1)) and ess.shape == (B0,)


# ---- 6. known answer ------------------------------------------------------------------------------------------------------------------
def test_closed_form_gaussian_convolution_on_the_device():
    """A flow whose last layer is zero has velocity 0: p = N(target_shift, target_scale^2), and noise of standard deviation
    sigma turns it into N(target_shift, target_scale^2 + sigma^2).  RMS error of log_prob_noisy against that closed form
    over 256 points: K = 64 at most 0.35 of K = 4 (theory 0.25; the float64 statement of the same estimator on these
    inputs, tests/test_observe_host.py and profiles/observe.txt: 0.379 and 0.088 nats, ratio 0.232); mean effective sample
    size at K = 64 in (1, 64]."""
    B, D, seed, shift, scale, sigma, x = closed_form_inputs()
    torch.manual_seed(90)
    f = Fm.ODEFlow(D, [64, 64], torch.nn.SiLU, torch.from_numpy(shift), torch.from_numpy(scale)).eval()
    with torch.no_grad():
        f.layers[-1].weight.zero_()
        f.layers[-1].bias.zero_()
    f = f.to(DEV)
    exact = exact_observed(x, shift, scale, sigma)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(sigma).to(DEV)
    rms = {}
    for K in (4, 64):
        got, ess = f.log_prob_noisy(xd, sd, num_draws=K, seed=seed, return_ess=True, **FLOW_RK4)
        rms[K] = float(np.sqrt(np.mean((got.double().cpu().numpy() - exact) ** 2)))
    ess = ess.double().cpu()
    print(f"\ngaussian convolution on the device: rms error K=4 {rms[4]:.4f}, K=64 {rms[64]:.4f} nats; mean ess {float(ess.mean()):.2f}")
    assert rms[64] <= 0.35 * rms[4], rms
    assert 1.0 < float(ess.mean()) <= 64.0
