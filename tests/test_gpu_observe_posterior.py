"""GPU tier: the posterior of noisy observations -- ff_weighted_resample (csrc/ff_observe.hip) at its corners, and
``posterior_noisy`` of the score models, the flows, the population wrappers and ``posterior_noisy_sharded`` around the
model's own log-density.

Anchors: the float64 numpy statement of tests/test_observe_posterior_host.py on the device's own ``y`` and ``lp`` (the
index outside a margin of 1e-9 W of the running sum's boundaries, the samples bit for bit, the moments within one fp32
rounding of a double result); the host twin; ``log_prob_noisy`` and ``observe_expand`` for what the front ends' fields
must be (bitwise); the closed-form Gaussian posterior; and bitwise equalities -- chunks, slices, shards, re-runs."""
import numpy as np
import pytest
import torch

from flowfusion_amd import _native, odeint
from flowfusion_amd import flow as Fm
from flowfusion_amd.distributed import posterior_noisy_sharded
from tests.test_gpu_observe import (B0, DEV, FLOW_RK4, SCORE_RK4, SENTINEL, _arena, _cflow, _flow, _guards_ok, _placed, _points,
                                    _population, _score, _stream)
from tests.test_observe_host import closed_form_inputs
from tests.test_observe_posterior_host import (ULP2, check_against_reference, check_known_answer, particles, reference_resample,
                                               same)

pytestmark = pytest.mark.gpu
DS = [1, 3, 4, 16, 17, 64]
MS = [0, 1, 5, 8]
INT_SENTINEL = -77


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _resample_raw(y, lp, K, M, seed, first, misalign, want=(True, True, True, True)):
    """The C entry point on inputs and outputs placed in sentinel arenas (one float past alignment with ``misalign``:
    the scalar body); returns (samples, index, mean, var) as numpy arrays -- None where ``want`` left the output out --
    after checking that no word outside the outputs was written."""
    B, D = y.shape[0] // K, y.shape[1]
    ys, ls = _placed(y, misalign), _placed(lp, misalign)
    sa, s = _arena(max(B * M * D, 1), misalign)
    ma, mu = _arena(max(B * D, 1), misalign)
    va, var = _arena(max(B * D, 1), misalign)
    ia = torch.full((64 + B * M + 64,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = ia[64:64 + B * M]
    ptr = lambda t, on: t.data_ptr() if on else 0
    rc = _native.lib().ff_weighted_resample(ys.data_ptr(), ls.data_ptr(), B, D, K, M, seed, first, ptr(s, want[0]), ptr(idx, want[1]),
                                            ptr(mu, want[2]), ptr(var, want[3]), _stream())
    assert rc == _native.FF_OK, rc
    torch.cuda.synchronize()
    written = (want[0] and M > 0, want[1] and M > 0, want[2], want[3])
    for arena, view, n, on in ((sa, s, B * M * D, written[0]), (ma, mu, B * D, written[2]), (va, var, B * D, written[3])):
        if on and B:
            assert _guards_ok(arena, view[:n]), (B, D, K, M, "a word outside an output was written")
            assert not bool((view[:n] == SENTINEL).any())
        else:
            assert bool((arena == SENTINEL).all()), (B, D, K, M, "an output that was not asked for was written")
    assert bool((ia[:64] == INT_SENTINEL).all()) and bool((ia[64 + B * M:] == INT_SENTINEL).all())
    assert bool((idx != INT_SENTINEL).all()) if written[1] else bool((idx == INT_SENTINEL).all())
    return (s[:B * M * D].view(B, M, D).cpu().numpy() if want[0] else None, idx.view(B, M).cpu().numpy() if want[1] else None,
            mu[:B * D].view(B, D).cpu().numpy() if want[2] else None, var[:B * D].view(B, D).cpu().numpy() if want[3] else None)


def _check_against_host(got, host, ref, K):
    """Device against host twin: the index equal outside the margin, the moments within twice the bars."""
    ok = ~ref["bad"]
    assert not ((got[1] != host[1]) & ~ref["close"]).any()
    for g, h, scale in ((got[2], host[2], ref["ymax"]), (got[3], host[3], ref["dmax"])):
        assert (np.abs(g[ok].astype(np.float64) - h[ok]) <= 2 * ULP2 * scale[ok]).all()


# ---- 1. the kernel against the float64 statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8, 17, 4096])
def test_kernel_against_float64_at_the_corners(K):
    """Every D x B of the lists, M and the placement (16-byte aligned: the vector body where D % 4 == 0; one float past
    it: the scalar body) cycling so that every M meets every D: the float64 statement of the device's own y and lp, at
    most 2 pairs per case within the margin, guard words untouched; and the host twin."""
    n = 0
    for D in DS:
        for B in (1, 37):
            rng = np.random.default_rng(1000 * K + 10 * D + B)
            y, lp = particles(rng, B, K, D)
            yd, ld = torch.from_numpy(y).to(DEV), torch.from_numpy(lp).to(DEV)
            for rep in range(2):
                M, misalign = MS[(n + n // 4) % 4], bool((n // 2) % 2) if D % 4 else bool(rep)
                n += 1
                seed, first = 17 * K + n, (2 ** 32 + 3 if rep else 0)
                got = _resample_raw(yd, ld, K, M, seed, first, misalign)
                ref = reference_resample(y, lp, K, M, seed, first)
                check_against_reference(got, ref, y, K, max_close=2)
                host = tuple(t.numpy() for t in _native.weighted_resample(torch.from_numpy(y), torch.from_numpy(lp), K, M, seed, first))
                _check_against_host(got, host, ref, K)
                if K == 1:
                    assert (got[1] == 0).all() and (got[3] == 0).all() and np.array_equal(got[2].view(np.uint32), y.view(np.uint32))
    assert n == 24
    # the binding: the same entry point on torch's current stream; a point alone or in another batch gives the same bits
    out = _native.weighted_resample(yd, ld, K, M, seed, first)
    assert all(np.array_equal(a.cpu().numpy(), b, equal_nan=True) for a, b in zip(out, got))
    for lo, hi in ((0, 1), (B // 2, B), (B - 1, B)):
        part = _native.weighted_resample(yd[lo * K:hi * K].clone(), ld[lo * K:hi * K].clone(), K, M, seed, first + lo)
        assert all(torch.equal(a[lo:hi], b) for a, b in zip(out, part)), (K, lo, hi)


def test_kernel_outputs_left_out_are_not_written_and_empty_batches():
    rng = np.random.default_rng(3)
    B, K, D, M, seed = 37, 8, 16, 5, 9
    y, lp = particles(rng, B, K, D)
    yd, ld = torch.from_numpy(y).to(DEV), torch.from_numpy(lp).to(DEV)
    for misalign in (False, True):
        full = _resample_raw(yd, ld, K, M, seed, 0, misalign)
        for want in ((True, False, False, False), (False, True, False, False), (False, False, True, False),
                     (False, False, False, True), (True, True, False, False), (False, False, True, True)):
            part = _resample_raw(yd, ld, K, M, seed, 0, misalign, want)
            for a, b, on in zip(part, full, want):
                assert (a is None) if not on else np.array_equal(a, b), want
        # M = 0: samples and index are ignored, the moments are those of any M
        none = _resample_raw(yd, ld, K, 0, seed, 0, misalign)
        assert none[0].shape == (B, 0, D) and np.array_equal(none[2], full[2]) and np.array_equal(none[3], full[3])
    # B = 0: nothing is launched, nothing is written
    sa, s = _arena(M * D, False)
    for Mz in (0, M):
        rc = _native.lib().ff_weighted_resample(yd.data_ptr(), ld.data_ptr(), 0, D, K, Mz, seed, 0, s.data_ptr(), 0, s.data_ptr(),
                                                s.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == _native.FF_OK and bool((sa == SENTINEL).all())
    out = _native.weighted_resample(yd[:0], ld[:0], K, 3, seed)
    assert out[0].shape == (0, 3, D) and out[1].shape == (0, 3) and out[2].shape == (0, D)


def test_kernel_grid_stride_loop_wraps():
    """B G = 140,000 x 4 lanes at K = 3 against a grid capped at 2048 x 256: a second trip."""
    B, K, D, M, seed, first = 140000, 3, 4, 1, 21, 123456789
    assert B * 4 > 2048 * 256
    rng = np.random.default_rng(6)
    y, lp = particles(rng, B, K, D)
    yd, ld = torch.from_numpy(y).to(DEV), torch.from_numpy(lp).to(DEV)
    ref = reference_resample(y, lp, K, M, seed, first)
    for misalign in (False, True):
        check_against_reference(_resample_raw(yd, ld, K, M, seed, first, misalign), ref, y, K, max_close=2)


@pytest.mark.parametrize("K", [1, 3, 17, 4096])
def test_kernel_degenerate_points_and_equal_rows(K):
    rng = np.random.default_rng(K)
    B, D, M = 6, 5, 4
    y = rng.standard_normal((B * K, D)).astype(np.float32)
    lp = rng.standard_normal(B * K).astype(np.float32)
    lp[1 * K:2 * K] = -np.inf                            # point 1: no draw has weight
    lp[2 * K + K // 2] = np.nan                          # point 2: a NaN
    lp[3 * K + K // 3] = np.inf                          # point 3: a +inf
    s, i, mu, v = (t.cpu().numpy() for t in _native.weighted_resample(torch.from_numpy(y).to(DEV), torch.from_numpy(lp).to(DEV), K, M, 3))
    for r in (1, 2, 3):
        assert (i[r] == -1).all() and np.isnan(s[r]).all() and np.isnan(mu[r]).all() and np.isnan(v[r]).all()
    ref = reference_resample(y, lp, K, M, 3)
    check_against_reference((s, i, mu, v), ref, y, K, max_close=2)
    assert np.isfinite(s[[0, 4, 5]]).all() and np.isfinite(mu[[0, 4, 5]]).all() and (v[[0, 4, 5]] >= 0).all()
    # noise_std = 0: K equal rows give the row back
    x = (torch.randn(B, D, generator=torch.Generator().manual_seed(K)) * 50).to(DEV)
    y0, _ = _native.observe_expand(x, torch.zeros(D, device=DEV), K, 4, 0)
    s, i, mu, v = _native.weighted_resample(y0, torch.from_numpy(lp).to(DEV).nan_to_num(0.0, 1.0, -1.0), K, M, 4)
    assert torch.equal(s, x[:, None, :].expand(B, M, D)) and torch.equal(mu, x)
    assert bool((v >= 0).all()) and bool((v.double() <= 1e-24 * torch.clamp(x.double() ** 2, min=1.0)).all())


# ---- 2. every front end ------------------------------------------------------------------------------------------------------------
def _check_fields(post, x, std, cond, K, M, seed, first, want_lp, want_ess):
    B, D = x.shape
    assert type(post) is odeint.NoisyPosterior
    assert post.samples.shape == (B, M, D) and post.index.shape == (B, M) and post.index.dtype == torch.int32
    assert post.mean.shape == (B, D) and post.var.shape == (B, D) and post.ess.shape == (B,)
    assert post.log_prob.shape == want_lp.shape and torch.equal(post.log_prob, want_lp) and torch.equal(post.ess, want_ess)
    y, _ = _native.observe_expand(x, std, K, seed, first, cond)
    assert bool(((post.index >= 0) & (post.index < K)).all())
    rows = (torch.arange(B, device=DEV)[:, None] * K + post.index.long()).reshape(-1)
    assert torch.equal(post.samples.reshape(B * M, D), y[rows])
    assert torch.isfinite(post.mean).all() and bool((post.var >= 0).all())
    return y


@pytest.mark.parametrize("D", [3, 16])
def test_front_ends_fields_chunks_slices_shards_and_reruns_are_bitwise(D):
    K, M, seed, first = 8, 5, 5, 2 ** 32 + 9
    std = (torch.rand(B0, D, generator=torch.Generator().manual_seed(81)) * 0.4 + 0.05).to(DEV)
    fc, C = _cflow(D)
    xc, c = (t.to(DEV) for t in _points(D, 61 + D, C))
    x = _points(D, 80).to(DEV)
    for m, pts, args, solver in ((_score(D).to(DEV), x, (), SCORE_RK4), (_flow(D).to(DEV), x, (), FLOW_RK4),
                                 (fc.to(DEV), xc, (c,), FLOW_RK4)):
        kw = dict(num_draws=K, seed=seed, sample_offset=first, **solver)
        want_lp, want_ess = m.log_prob_noisy(pts, std, *args, return_ess=True, **kw)
        post = m.posterior_noisy(pts, std, *args, num_samples=M, **kw)
        _check_fields(post, pts, std, args[0] if args else None, K, M, seed, first, want_lp, want_ess)
        for chunk in (1, 7):
            assert same(m.posterior_noisy(pts, std, *args, num_samples=M, chunk_points=chunk, **kw), post), chunk
        assert same(m.posterior_noisy(pts, std, *args, num_samples=M, **kw), post)                  # the same seed twice
        old, odeint.OBSERVE_CHUNK_ROWS = odeint.OBSERVE_CHUNK_ROWS, 10 * K
        try:
            assert same(m.posterior_noisy(pts, std, *args, num_samples=M, **kw), post)
        finally:
            odeint.OBSERVE_CHUNK_ROWS = old
        for lo, hi in ((0, 1), (11, 30), (36, 37)):                                                 # a rank's rows, computed alone
            part = m.posterior_noisy(pts[lo:hi], std[lo:hi], *(a[lo:hi] for a in args), num_samples=M,
                                     **dict(kw, sample_offset=first + lo))
            assert same(part, odeint.NoisyPosterior(*(f[lo:hi] for f in post))), (lo, hi)
        assert not torch.equal(m.posterior_noisy(pts, std, *args, num_samples=M, **dict(kw, seed=seed + 1)).index, post.index)
        # the sharded entry point in one process (sample_offset = 0 there), gather both ways
        want = m.posterior_noisy(pts, std, *args, num_draws=K, num_samples=M, seed=seed, **solver)
        assert same(posterior_noisy_sharded(m, pts, std, *args, seed=seed, num_draws=K, num_samples=M, **solver), want)
        got, span = posterior_noisy_sharded(m, local_x=pts, local_noise_std=std, local_conditional=args[0] if args else None,
                                            n_total=B0, seed=seed, num_draws=K, num_samples=M, gather=False, **solver)
        assert span == (0, B0) and same(got, want)


@pytest.mark.parametrize("D", [3, 16])
def test_population_wrappers_return_the_units_of_x(D):
    """The wrappers' solve is adaptive dopri5: all B K rows are one solve, equal to the by-hand composition."""
    K, M, seed = 4, 3, 9
    pm = _population(D).to(DEV)
    x = _points(D, 84).to(DEV)
    xp = x * pm.scale + pm.shift
    std = 0.1 * pm.scale
    want_lp, want_ess = pm.log_prob_noisy(xp, std, num_draws=K, seed=seed, return_ess=True)
    post = pm.posterior_noisy(xp, std, num_draws=K, num_samples=M, seed=seed)
    yp = _check_fields(post, xp, std, None, K, M, seed, 0, want_lp, want_ess)
    hand = _native.weighted_resample(yp, pm.log_prob(yp), K, M, seed)
    assert all(torch.equal(a, b) for a, b in zip(hand, (post.samples, post.index, post.mean, post.var)))
    assert bool(((post.mean - xp).abs() <= 6 * std).all())                  # data space: within the noise of the observation
    with pytest.raises(ValueError, match="chunk_points"):
        pm.posterior_noisy(xp, std, num_draws=K, chunk_points=8)


def test_hutchinson_models_are_chunk_invariant_too():
    D, K, M, seed, first = 16, 8, 4, 6, 12345
    x = _points(D, 82).to(DEV)
    std = (torch.rand(D, generator=torch.Generator().manual_seed(83)) * 0.4).to(DEV)
    hm = _score(D, hutchinson=True).to(DEV)
    for probes in (1, 3):
        kw = dict(num_draws=K, seed=seed, sample_offset=first, num_probes=probes, **SCORE_RK4)
        post = hm.posterior_noisy(x, std, num_samples=M, **kw)
        want_lp, want_ess = hm.log_prob_noisy(x, std, return_ess=True, **kw)
        _check_fields(post, x, std, None, K, M, seed, first, want_lp, want_ess)
        for chunk in (1, 7):
            assert same(hm.posterior_noisy(x, std, num_samples=M, chunk_points=chunk, **kw), post), (probes, chunk)
    f = _flow(D).to(DEV)
    run = lambda **kw: f.posterior_noisy(x, std, num_draws=K, num_samples=M, seed=seed, sample_offset=first, hutchinson=True,
                                         **FLOW_RK4, **kw)
    assert same(run(chunk_points=5), run())


def test_adaptive_default_solves_all_rows_at_once():
    D, K, M = 3, 4, 2
    sm, x = _score(D).to(DEV), _points(D, 84).to(DEV)
    with pytest.raises(ValueError, match="chunk_points"):
        sm.posterior_noisy(x, 0.1, num_draws=K, chunk_points=8)
    y, _ = _native.observe_expand(x, torch.full((D,), 0.1, device=DEV), K, 9, 0)
    rows = sm.log_prob(y)                                                    # dopri5 on the 148 rows as one batch
    post = sm.posterior_noisy(x, 0.1, num_draws=K, num_samples=M, seed=9)
    ess = torch.empty(B0, device=DEV)
    assert torch.equal(post.log_prob, _native.logmeanexp(rows, K, None, ess).view(-1, 1)) and torch.equal(post.ess, ess)
    hand = _native.weighted_resample(y, rows, K, M, 9)
    assert all(torch.equal(a, b) for a, b in zip(hand, (post.samples, post.index, post.mean, post.var)))


# ---- 3. known answer ---------------------------------------------------------------------------------------------------------------
def test_known_answer_gaussian_posterior_on_the_device():
    """A flow whose last layer is zero has velocity 0: p = N(target_shift, target_scale^2), whose posterior under noise
    sigma is Gaussian in closed form.  The four assertions of tests/test_observe_posterior_host.py (the float64 statement
    there: rms of mean 0.603 / 0.150 posterior sd at K = 4 / 64; at K = 256 var / exact 0.992, pooled sample variance 1.003,
    mean ess 182)."""
    B, D, seed, shift, scale, sigma, x = closed_form_inputs()
    torch.manual_seed(90)
    f = Fm.ODEFlow(D, [64, 64], torch.nn.SiLU, torch.from_numpy(shift), torch.from_numpy(scale)).eval()
    with torch.no_grad():
        f.layers[-1].weight.zero_()
        f.layers[-1].bias.zero_()
    f = f.to(DEV)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(sigma).to(DEV)

    def posterior_of(K, M):
        post = f.posterior_noisy(xd, sd, num_draws=K, num_samples=M, seed=seed, **FLOW_RK4)
        return tuple(t.cpu().numpy() for t in (post.samples, post.mean, post.var, post.ess))

    check_known_answer(posterior_of)
