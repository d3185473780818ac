"""GPU tier: the marginal log-density of the symplectic flows over K momentum draws -- the two streaming kernels of
csrc/ff_marginal.hip at their corners, and ``SymplecticFlowModel.log_prob_marginal`` / ``symplectic_log_prob_sharded(...,
num_momenta=K)`` around the solve.

Anchors: torch's own fp32 ``(x - shift) / scale`` and ``ff_normal_fill`` for what expand writes (bitwise); float64 torch on
the same bits for what reduce returns (one fp32 rounding of a double result); the float64 restatement of the dynamics
(tests/_symplectic_ref.py, leapfrog_f64) for the per-draw values end to end; the closed-form marginal of the rotation field
(tests/test_symplectic_marginal_host.py); and bitwise equalities -- chunks, slices, re-runs, launch kinds."""
import ctypes
import math

import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.distributed import symplectic_log_prob_sharded
from flowfusion_amd.fused import MODE_STATE
from tests.test_gpu_symplectic import _rotation_model, _warned
from tests.test_gpu_symplectic_leapfrog import _fixture_model, _grid
from tests.test_gpu_symplectic_twin import seeded_model
from tests.test_symplectic_host import EXPECTED_KERNEL
from tests.test_symplectic_leapfrog_host import IN_ENVELOPE, leapfrog_f64
from tests.test_symplectic_marginal_host import ALPHA, BETA, STEPS, closed_form_inputs, exact_marginal, rotation_leapfrog_matrix
from tests._util import max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE = _native.MOMENTUM_NOISE_BASE
SENTINEL = -7.5e33
GUARD = 64
KS = [1, 2, 5, 64, 65, 257]
BS = [1, 3, 1000]
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _logp_err(got, want):
    return max_rel(got.detach().cpu(), want.detach().cpu(), floor=1.0)


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


def _momenta(B, D, K, seed, offset):
    """[B K, D]: momentum k of point r in row r K + k, from ff_normal_fill under noise index BASE + k."""
    p = torch.empty(B, K, D, device=DEV)
    for k in range(K):
        p[:, k] = _native.normal_fill(B, D, seed, offset, DEV, noise_index=BASE + k)
    return p.view(B * K, D)


def _expand_raw(x, shift, scale, cond, K, seed, offset, misalign):
    """The C entry point on inputs and outputs placed in sentinel arenas; returns (z0, cond_out) after checking that no
    word outside the outputs was written."""
    B, D = x.shape
    C = 0 if cond is None else cond.shape[1]
    xs, cs = _placed(x, misalign), _placed(cond, misalign)
    za, z0 = _arena(B * K * 2 * D, misalign)
    ca, co = _arena(max(B * K * C, 1), misalign)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    rc = _native.lib().ff_marginal_expand(ptr(xs), ptr(shift), ptr(scale), ptr(cs), B, D, C, K, seed, offset, z0.data_ptr(),
                                         co.data_ptr() if cond is not None else 0, _stream())
    assert rc == _native.FF_OK
    torch.cuda.synchronize()
    assert _guards_ok(za, z0), (B, D, K, "a word outside z0 was written")
    if cond is None:
        assert bool((ca == SENTINEL).all())
        return z0.view(B * K, 2 * D), None
    assert _guards_ok(ca, co[:B * K * C]), (B, D, K, "a word outside cond_out was written")
    return z0.view(B * K, 2 * D), co[:B * K * C].view(B * K, C)


def _reduce_raw(z1, B, D, K, seed, offset, log_det, misalign, want_ess=True):
    zs = _placed(z1, misalign)
    oa, out = _arena(B, False)
    ea, ess = _arena(B, False)
    rc = _native.lib().ff_marginal_reduce(zs.data_ptr(), B, D, K, seed, offset, log_det, out.data_ptr(),
                                         ess.data_ptr() if want_ess else 0, _stream())
    assert rc == _native.FF_OK
    torch.cuda.synchronize()
    assert _guards_ok(oa, out) and _guards_ok(ea, ess), (B, D, K, "a word outside an output was written")
    if not want_ess:
        assert bool((ea == SENTINEL).all())
    return out.clone(), ess.clone()


def _reference_reduce(z1, p0, K, log_det):
    """(log p, ess, lw [B, K]) in float64 torch from the bits of z1 [B K, 2 D] and p0 [B K, D]."""
    D = p0.shape[1]
    lw = (-0.5 * (z1.double().pow(2).sum(1) - p0.double().pow(2).sum(1)) - D * HALF_LOG_2PI).view(-1, K)
    logp = torch.logsumexp(lw, dim=1) - math.log(K) - log_det
    m = lw.max(dim=1, keepdim=True).values
    w = torch.exp(lw - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    return logp, w.sum(1) ** 2 / (w * w).sum(1), lw


def _within_one_rounding(got, ref):
    """|got - ref| <= 1.2e-7 |ref| + 1e-10: one fp32 rounding of a result computed in double."""
    return bool(((got.double() - ref).abs() <= 1.2e-7 * ref.abs() + 1e-10).all())


# ---- the kernels at their corners ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 16, 17, 32])
def test_kernels_at_their_corners(D):
    """Every K x B of the lists: expand bitwise against torch and ff_normal_fill, reduce against float64 torch at the
    one-rounding bar, guard words untouched.  Each shape twice: aligned with shift / scale, a conditional and a global row
    above 2^32; one float past alignment (the scalar bodies) without shift / scale."""
    g = torch.Generator(device=DEV).manual_seed(100 + D)
    shift = torch.randn(D, device=DEV, generator=g) * 0.3
    scale = torch.rand(D, device=DEV, generator=g) + 0.5
    for K in KS:
        for B in BS:
            x = torch.randn(B, D, device=DEV, generator=g) * 2
            z1 = torch.randn(B * K, 2 * D, device=DEV, generator=g) * 1.2
            for misalign in (False, True):
                seed, offset = 7 + K, (2 ** 32 + 5 if not misalign else 0)
                sh, sc = (None, None) if misalign else (shift, scale)
                C = 0 if (K == 2 and not misalign) else (4 if (B + K) % 2 == 0 else 3)
                cond = torch.randn(B, C, device=DEV, generator=g) if C else None
                z0, co = _expand_raw(x, sh, sc, cond, K, seed, offset, misalign)
                q = x if misalign else (x - shift) / scale
                what = (D, K, B, misalign)
                assert torch.equal(z0[:, :D].contiguous().view(torch.int32),
                                   q.repeat_interleave(K, dim=0).contiguous().view(torch.int32)), what
                p0 = _momenta(B, D, K, seed, offset)
                assert torch.equal(z0[:, D:].contiguous().view(torch.int32), p0.view(torch.int32)), what
                if C:
                    assert torch.equal(co.view(torch.int32), cond.repeat_interleave(K, dim=0).contiguous().view(torch.int32)), what
                log_det = 0.0 if misalign else float(torch.log(scale.double()).sum())
                ref, ref_ess, _ = _reference_reduce(z1, p0, K, log_det)
                got, ess = _reduce_raw(z1, B, D, K, seed, offset, log_det, misalign, want_ess=not (misalign and K == 5))
                assert _within_one_rounding(got, ref), what
                if not (misalign and K == 5):
                    assert _within_one_rounding(ess, ref_ess), what
    # the binding: the same entry points on torch's current stream
    z0b, cob = _native.marginal_expand(x, K, seed, offset, sh, sc, cond)
    assert torch.equal(z0b, z0) and (cond is None or torch.equal(cob, co))
    assert torch.equal(_native.marginal_reduce(z1, K, seed, offset, log_det), got)


def test_grid_stride_loops_wrap():
    """B K ceil(D / 4) = 640,000 lanes of work against a grid capped at 2048 x 256: both kernels take a second trip."""
    B, K, D, C, seed, offset = 40000, 4, 16, 4, 21, 123456789
    assert B * K * (D // 4) > 2048 * 256
    g = torch.Generator(device=DEV).manual_seed(5)
    x, cond = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, C, device=DEV, generator=g)
    shift, scale = torch.randn(D, device=DEV, generator=g), torch.rand(D, device=DEV, generator=g) + 0.5
    for misalign in (False, True):
        z0, co = _expand_raw(x, shift, scale, cond, K, seed, offset, misalign)
        p0 = _momenta(B, D, K, seed, offset)
        assert torch.equal(z0[:, :D], ((x - shift) / scale).repeat_interleave(K, dim=0))
        assert torch.equal(z0[:, D:].contiguous().view(torch.int32), p0.view(torch.int32))
        assert torch.equal(co, cond.repeat_interleave(K, dim=0))
        z1 = z0 * 0.9 + 0.1
        ref, ref_ess, _ = _reference_reduce(z1, p0, K, 0.5)
        got, ess = _reduce_raw(z1, B, D, K, seed, offset, 0.5, misalign)
        assert _within_one_rounding(got, ref) and _within_one_rounding(ess, ref_ess)


@pytest.mark.parametrize("K", KS)
def test_reduce_non_finite_rows_follow_logsumexp(K):
    """A draw of weight zero (an infinity in z1) drops out; all of a point's draws at weight zero give -inf, not NaN; a NaN
    gives NaN -- torch.logsumexp in float64 on the same bits says the same."""
    D, B, seed = 3, 4, 8
    g = torch.Generator(device=DEV).manual_seed(K)
    z1 = torch.randn(B * K, 2 * D, device=DEV, generator=g)
    z1[K - 1, 2] = float("inf")
    z1[K:2 * K, 0] = float("-inf")
    z1[2 * K + K // 2, 4] = float("nan")
    p0 = _momenta(B, D, K, seed, 0)
    ref, ref_ess, lw = _reference_reduce(z1, p0, K, 0.0)
    assert ref[1] == float("-inf") and torch.isnan(ref[2])
    got, ess = _reduce_raw(z1, B, D, K, seed, 0, 0.0, False)
    assert got[1] == float("-inf") and torch.isnan(ess[1]) and torch.isnan(got[2]) and torch.isnan(ess[2])
    keep = [3] if K == 1 else [0, 3]
    assert _within_one_rounding(got[keep], ref[keep]) and _within_one_rounding(ess[keep], ref_ess[keep])
    if K == 1:
        assert got[0] == float("-inf")


# ---- K = 1 is the one-draw estimate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["leapfrog", "dopri5"])
def test_one_momentum_is_the_one_draw_log_prob(method):
    """The same solve on the same bits; only the summation differs (double here, fp32 torch ops there)."""
    meta, arrays, fm, ref = _fixture_model("sym_5d_c3_ragged")
    B, D, seed = 24, meta["D"], 91
    x, cond = arrays["sample_4"][:B].to(DEV), arrays["cond"][:B].to(DEV)
    kw = {"method": "leapfrog", "num_steps": 25} if method == "leapfrog" else {}
    got = fm.log_prob_marginal(x, cond, num_momenta=1, seed=seed, **kw)
    p0 = _native.normal_fill(B, D, seed, 0, DEV, noise_index=BASE)
    want = fm._log_prob_from(x, p0, cond, **kw)
    assert got.shape == (B,) and _logp_err(got, want) < 2e-5, _logp_err(got, want)


# ---- end to end against the float64 restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IN_ENVELOPE + ["sym_20d_outside"])
def test_marginal_against_the_float64_restatement(name):
    """The K per-draw values from the float64 restatement on the same momenta, combined in float64.  Log-sum-exp is
    1-Lipschitz in the max norm, so the per-draw bar carries through: |diff| <= 2e-5 max(1, max_k |lw_k|) per point."""
    meta, arrays, fm, ref = _fixture_model(name)
    B, K, D, seed, offset = 6, 5, meta["D"], 17, 1000
    x = arrays["sample_4"][:B]
    cond = arrays.get("cond")
    cond = None if cond is None else cond[:B]
    p0 = _momenta(B, D, K, seed, offset).cpu()
    xr = x.repeat_interleave(K, dim=0)
    cr = None if cond is None else cond.repeat_interleave(K, dim=0)
    log_det = float(torch.log(ref.scale).sum())

    def check(got, per_draw, what):
        lw = per_draw.view(B, K) + log_det
        want = torch.logsumexp(per_draw.view(B, K), dim=1) - math.log(K)
        bar = 2e-5 * lw.abs().max(dim=1).values.clamp_min(1.0)
        diff = (got.double().cpu() - want).abs()
        print(f"\n[{name}] {what}: max diff {float(diff.max()):.3e}, bar {float(bar.min()):.3e}")
        assert got.shape == (B,) and bool((diff <= bar).all()), (what, diff, bar)

    for n in (1, 4, 25):
        per_draw = ref._log_prob(xr, p0, cr, lambda z0, cond_n: leapfrog_f64(ref, z0, _grid(n).flip(0), cond_n))
        got, warned = _warned(lambda: fm.log_prob_marginal(x.to(DEV), None if cond is None else cond.to(DEV), num_momenta=K,
                                                           seed=seed, sample_offset=offset, method="leapfrog", num_steps=n))
        check(got, per_draw, f"leapfrog {n}")
    per_draw = ref.log_prob_dopri5(xr, p0, cr, 1e-5)
    got = _warned(lambda: fm.log_prob_marginal(x.to(DEV), None if cond is None else cond.to(DEV), num_momenta=K, seed=seed,
                                               sample_offset=offset))[0]
    check(got, per_draw, "dopri5")
    assert fm._fusable() == (EXPECTED_KERNEL[name] is not None)


# ---- closed form -------------------------------------------------------------------------------------------------------------
def test_closed_form_rotation_marginal_on_the_device():
    """v = [alpha p, -beta q] under four leapfrog steps: the exact marginal is Gaussian (tests/test_symplectic_marginal_host.py).
    RMS error at K = 64 at most a quarter of K = 1; mean effective sample size at K = 64 in (32, 64]."""
    B, D, seed, q_recipe = closed_form_inputs()
    fm, shift, scale = _rotation_model(D, 0, 6, [64], ALPHA, BETA)
    assert fm._fusable()
    x = (torch.from_numpy(q_recipe).double() * scale + shift).float()
    q0 = ((x.double() - shift) / scale).numpy()
    exact = exact_marginal(q0, rotation_leapfrog_matrix()) - float(torch.log(scale).sum())
    rms = {}
    for K in (1, 64):
        got, ess = fm.log_prob_marginal(x.to(DEV), num_momenta=K, seed=seed, method="leapfrog", num_steps=STEPS, return_ess=True)
        rms[K] = float(np.sqrt(np.mean((got.double().cpu().numpy() - exact) ** 2)))
    ess = ess.double().cpu()
    print(f"\nrotation marginal on the device: rms error K=1 {rms[1]:.4f}, K=64 {rms[64]:.4f} nats; mean ess {float(ess.mean()):.2f}")
    assert rms[64] <= 0.25 * rms[1], rms
    assert 32.0 < float(ess.mean()) <= 64.0 and bool(((ess > 1.0) & (ess <= 64.0 * (1 + 1e-6))).all())


# ---- invariances under method="leapfrog": all bitwise ------------------------------------------------------------------------
def _select_kind(fm, rows):
    return _native.launch_kind(fm._net().plan(MODE_STATE, select=True), rows, MODE_STATE)


@pytest.fixture(scope="module")
def wide_model():
    return seeded_model(16, 4, [128] * 2, 61)


def test_chunks_slices_and_reruns_are_bitwise(wide_model):
    fm = wide_model
    B, K, D, seed, first = 100, 16, 16, 5, 2 ** 32 + 9
    g = torch.Generator(device=DEV).manual_seed(62)
    x, cond = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, 4, device=DEV, generator=g)
    run = lambda **kw: fm.log_prob_marginal(x, cond, num_momenta=K, seed=seed, sample_offset=first, method="leapfrog",
                                            num_steps=4, return_ess=True, **kw)
    lp, ess = run()
    assert lp.shape == ess.shape == (B,) and torch.isfinite(lp).all() and bool(((ess > 0) & (ess <= K * (1 + 1e-6))).all())
    for chunk in (B, 7, 1):
        a, b = run(chunk_points=chunk)
        assert torch.equal(a, lp) and torch.equal(b, ess), chunk
    a, b = run()                                                            # a re-run with the same seed
    assert torch.equal(a, lp) and torch.equal(b, ess)
    fm.MARGINAL_CHUNK_ROWS = 40 * K                                         # the default rule: chunk_points K <= that many rows
    try:
        a, b = run()
    finally:
        del fm.MARGINAL_CHUNK_ROWS
    assert torch.equal(a, lp) and torch.equal(b, ess)
    for lo, hi in ((0, 1), (37, 70), (93, 100)):                            # a rank's rows, computed alone
        a = fm.log_prob_marginal(x[lo:hi], cond[lo:hi], num_momenta=K, seed=seed, sample_offset=first + lo, method="leapfrog",
                                 num_steps=4)
        assert torch.equal(a, lp[lo:hi]), (lo, hi)
    other = fm.log_prob_marginal(x, cond, num_momenta=K, seed=seed + 1, sample_offset=first, method="leapfrog", num_steps=4)
    assert not torch.equal(other, lp) and (other != lp).float().mean() > 0.9            # another seed, other momenta
    # a fixed-grid torchdiffeq method chunks as well
    a = fm.log_prob_marginal(x, cond, num_momenta=4, seed=seed, method="rk4", options={"step_size": 0.25})
    assert torch.equal(fm.log_prob_marginal(x, cond, num_momenta=4, seed=seed, method="rk4", options={"step_size": 0.25},
                                            chunk_points=33), a)


def test_every_launch_kind_gives_the_same_rows(wide_model):
    """One call whose 49,744 rows take the one-wavefront kernel with a tail split, against chunks of 1024 points (16,384
    rows: the one-wavefront kernel alone) with a last chunk on the twin, and against chunks of 64 points (the twin): the
    launcher's own rule is asked which kernel a row count takes; no clock is."""
    fm = wide_model
    B, K, D, seed = 3109, 16, 16, 77
    assert _select_kind(fm, B * K) == _native.LAUNCH_ONE_WAVE_AND_TWIN
    assert _select_kind(fm, 1024 * K) == _native.LAUNCH_ONE_WAVE and _select_kind(fm, (B - 3 * 1024) * K) == _native.LAUNCH_TWIN
    assert _select_kind(fm, 64 * K) == _native.LAUNCH_TWIN
    g = torch.Generator(device=DEV).manual_seed(63)
    x, cond = torch.randn(B, D, device=DEV, generator=g), torch.randn(B, 4, device=DEV, generator=g)
    run = lambda **kw: fm.log_prob_marginal(x, cond, num_momenta=K, seed=seed, method="leapfrog", num_steps=4, **kw)
    whole = run(chunk_points=B)
    assert torch.isfinite(whole).all()
    assert torch.equal(run(chunk_points=1024), whole)
    assert torch.equal(run(chunk_points=64), whole)
    assert torch.equal(fm.log_prob_marginal(x[:64], cond[:64], num_momenta=K, seed=seed, method="leapfrog", num_steps=4), whole[:64])


def test_seed_none_follows_torch_manual_seed(wide_model):
    fm = wide_model
    g = torch.Generator(device=DEV).manual_seed(64)
    x, cond = torch.randn(9, 16, device=DEV, generator=g), torch.randn(9, 4, device=DEV, generator=g)
    run = lambda: fm.log_prob_marginal(x, cond, num_momenta=4, method="leapfrog", num_steps=4)
    torch.manual_seed(5)
    a, b = run(), run()
    torch.manual_seed(5)
    assert torch.equal(run(), a) and not torch.equal(a, b)
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert torch.equal(fm.log_prob_marginal(x, cond, num_momenta=4, method="leapfrog", num_steps=4, seed=seed), a)


# ---- the sharded entry point, one rank ---------------------------------------------------------------------------------------
def test_sharded_entry_point_on_one_gpu(wide_model):
    fm = wide_model
    n, D, K, seed = 50, 16, 8, 23
    g = torch.Generator(device=DEV).manual_seed(65)
    x, cond = torch.randn(n, D, device=DEV, generator=g), torch.randn(n, 4, device=DEV, generator=g)
    one = symplectic_log_prob_sharded(fm, x, cond, seed=seed, method="leapfrog", num_steps=4)              # today's path
    assert torch.equal(one, fm._log_prob_from(x, _native.normal_fill(n, D, seed, 0, DEV), cond, method="leapfrog", num_steps=4))
    assert torch.equal(symplectic_log_prob_sharded(fm, x, cond, seed=seed, method="leapfrog", num_steps=4, num_momenta=None), one)
    want, want_ess = fm.log_prob_marginal(x, cond, num_momenta=K, seed=seed, method="leapfrog", num_steps=4, return_ess=True)
    got = symplectic_log_prob_sharded(fm, x, cond, seed=seed, method="leapfrog", num_steps=4, num_momenta=K)
    assert torch.equal(got, want) and not torch.equal(got, one)
    got, ess = symplectic_log_prob_sharded(fm, local_x=x, local_conditional=cond, n_total=n, seed=seed, method="leapfrog",
                                           num_steps=4, num_momenta=K, return_ess=True)
    assert torch.equal(got, want) and torch.equal(ess, want_ess)
    (got, ess), bounds = symplectic_log_prob_sharded(fm, x, cond, seed=seed, method="leapfrog", num_steps=4, num_momenta=K,
                                                     return_ess=True, gather=False)
    assert bounds == (0, n) and torch.equal(got, want) and torch.equal(ess, want_ess)
    # dopri5 (one rank: no exchange to enter)
    assert torch.equal(symplectic_log_prob_sharded(fm, x[:12], cond[:12], seed=seed, num_momenta=2),
                       fm.log_prob_marginal(x[:12], cond[:12], num_momenta=2, seed=seed))
    with pytest.raises(ValueError, match="return_ess"):
        symplectic_log_prob_sharded(fm, x, cond, seed=seed, return_ess=True)
