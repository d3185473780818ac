"""CPU tier of the posterior of noisy observations: ff_weighted_resample through its host twin (csrc/ff_observe.h), the
argument rules of the C entry points, the front ends' ``posterior_noisy`` around stub log-densities, and
``posterior_noisy_sharded`` over gloo.

Anchors: a float64 numpy statement of the estimator written here (uniforms from tests/_philox.py, the running sum in index
order); the rows of ff_observe_expand for what a sample must be; and a closed form independent of both -- a Gaussian prior
N(shift, scale^2) observed with noise sigma has the Gaussian posterior of mean (x s^2 + shift sigma^2) / (s^2 + sigma^2)
and variance s^2 sigma^2 / (s^2 + sigma^2)."""
import inspect
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flowfusion_amd import _native, odeint
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from tests._philox import philox4x32_10
from tests.test_observe_host import FIXED, _free_port, _row_keyed, _score, _stubbed, closed_form_inputs

ROOT = Path(__file__).resolve().parent.parent
RESAMPLE_INDEX = 0xFFFA0000
MARGIN = 1e-9               # a target within MARGIN W of a boundary of the running sum may fall either way
ULP2 = 2.0 ** -23           # one fp32 rounding (2^-24 relative) of a double result, with a factor 2 of slack


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the float64 statement -----------------------------------------------------------------------------------------------
def uniforms(seed, first, B, M):
    """u [B, M] float64: u_m of global row g = (word[m & 3] >> 8) 2^-24, word = the Philox block of counter
    (g lo, g hi, FF_OBS_RESAMPLE_NOISE_INDEX, m >> 2) under the seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = max(1, (M + 3) // 4)
    g = np.arange(B, dtype=np.uint64) + np.uint64(first)
    ctr = np.empty((B, nq, 4), dtype=np.uint32)
    ctr[..., 0] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[..., 1] = (g >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[..., 2] = np.uint32(RESAMPLE_INDEX)
    ctr[..., 3] = np.arange(nq, dtype=np.uint32)[None, :]
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(B, nq * 4)
    return (w >> np.uint32(8)).astype(np.float64)[:, :M] * 2.0 ** -24


def reference_resample(y, lp, K, M, seed, first=0):
    """The estimator in float64 numpy from y [B K, D] and lp [B K] (fp32 arrays): a dict of index [B, M] (-1 on degenerate
    points), close [B, M] (the target lies within MARGIN W of a boundary), mean, var [B, D] (NaN on degenerate points),
    bad [B], and the scales of the two bars, ymax = max_k |y_kd| and dmax = max_k (y_kd - mean_d)^2."""
    B, D_ = y.shape[0] // K, y.shape[1]
    y64, lw = y.astype(np.float64).reshape(B, K, D_), lp.astype(np.float64).reshape(B, K)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = lw.max(1) if B else np.zeros(0)
        bad = np.isnan(lw).any(1) | (lw == np.inf).any(1) | (mx == -np.inf)
        w = np.exp(lw - np.where(bad, 0.0, mx)[:, None])
        w[bad] = 1.0
        cum = np.cumsum(w, axis=1)                                              # index order
        W = cum[:, -1]
        t = uniforms(seed, first, B, M) * W[:, None]
        index = np.empty((B, M), dtype=np.int64)
        close = np.empty((B, M), dtype=bool)
        for m in range(M):
            index[:, m] = (cum > t[:, m:m + 1]).argmax(1)                       # the smallest k with cum_k > t
            close[:, m] = np.abs(cum - t[:, m:m + 1]).min(1) <= MARGIN * W
        mean = (w[:, :, None] * y64).sum(1) / W[:, None]
        dev2 = (y64 - mean[:, None, :]) ** 2
        var = (w[:, :, None] * dev2).sum(1) / W[:, None]
    index[bad] = -1
    close[bad] = False
    mean[bad] = np.nan
    var[bad] = np.nan
    return dict(index=index, close=close, mean=mean, var=var, bad=bad, ymax=np.abs(y64).max(1), dmax=dev2.max(1))


def check_against_reference(got, ref, y, K, max_close=0, slack=1.0):
    """``got`` = (samples, index, mean, var) as numpy arrays against ``reference_resample``: the index equal (at most
    ``max_close`` pairs left out, each within the margin), the samples bit for bit the rows at the index THE CODE
    returned, the moments within their bars (times ``slack``), var >= 0."""
    samples, index, mean, var = got
    B, M = index.shape
    ok = ~ref["bad"]
    differs = index != ref["index"]
    assert not (differs & ~ref["close"]).any(), np.argwhere(differs & ~ref["close"])[:5]
    assert int(ref["close"].sum()) <= max_close, int(ref["close"].sum())
    assert (index[ok] >= 0).all() and (index[ok] < K).all() and (index[~ok] == -1).all()
    rows = (np.arange(B)[:, None] * K + np.maximum(index, 0)).reshape(-1)
    want = y[rows].reshape(B, M, y.shape[1])
    assert np.array_equal(samples[ok].view(np.uint32), want[ok].view(np.uint32))
    assert np.isnan(samples[~ok]).all() and np.isnan(mean[~ok]).all() and np.isnan(var[~ok]).all()
    err_m = np.abs(mean[ok].astype(np.float64) - ref["mean"][ok])
    err_v = np.abs(var[ok].astype(np.float64) - ref["var"][ok])
    assert (err_m <= slack * ULP2 * ref["ymax"][ok]).all(), float((err_m / (ULP2 * ref["ymax"][ok] + 1e-300)).max())
    assert (err_v <= slack * ULP2 * ref["dmax"][ok]).all(), float((err_v / (ULP2 * ref["dmax"][ok] + 1e-300)).max())
    assert (var[ok] >= 0).all()


def particles(rng, B, K, D_):
    """y [B K, D] and lp = 3 randn [B K] with some -inf entries (a first and a last draw among them; a point that loses
    every draw is degenerate and checked as such)."""
    y = (rng.standard_normal((B * K, D_)) * 2 + 0.5).astype(np.float32)
    lp = (3 * rng.standard_normal(B * K)).astype(np.float32)
    if K > 1:
        drop = rng.random(B * K) < 0.15
        drop.reshape(B, K)[:, 0] &= False
        drop.reshape(B, K)[np.arange(B), rng.integers(0, K, B)] = False
        drop.reshape(B, K)[3 % B, K - 1] = True                               # a last draw of weight zero
        drop.reshape(B, K)[5 % B, 0] = True                                   # a first one
        lp[drop] = -np.inf
    return y, lp


def host_resample(y, lp, K, M, seed, first=0, **kw):
    out = _native.weighted_resample(torch.from_numpy(y), torch.from_numpy(lp), K, M, seed, first, **kw)
    return tuple(None if t is None else t.numpy() for t in out)


# ---- the host twin against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 2 ** 32 + 3])
@pytest.mark.parametrize("K", [1, 3, 8, 17, 4096])
def test_host_twin_against_float64(K, first):
    B = 37
    for D_ in (1, 3, 4, 17):
        rng = np.random.default_rng(1000 * K + D_)
        y, lp = particles(rng, B, K, D_)
        for M in (1, 5, 8):
            seed = 31 * K + M
            got = host_resample(y, lp, K, M, seed, first)
            assert got[0].shape == (B, M, D_) and got[1].shape == (B, M) and got[1].dtype == np.int32
            assert got[2].shape == (B, D_) and got[3].shape == (B, D_)
            ref = reference_resample(y, lp, K, M, seed, first)
            check_against_reference(got, ref, y, K, max_close=0)
            assert (lp.reshape(B, K)[np.arange(B)[:, None], got[1]] > -np.inf).all()      # never a row of weight zero
            if K == 1:
                assert (got[1] == 0).all() and (got[3] == 0).all()
                assert np.array_equal(got[2].view(np.uint32), y.view(np.uint32))
    # outputs left out are left out, the others keep their bits; M = 0 leaves the moments
    full = host_resample(y, lp, K, 8, seed, first)
    s, i, mu, v = host_resample(y, lp, K, 8, seed, first, want_moments=False)
    assert mu is None and v is None and np.array_equal(s, full[0]) and np.array_equal(i, full[1])
    s, i, mu, v = host_resample(y, lp, K, 0, seed, first, want_index=False)
    assert s.shape == (B, 0, 17) and i is None and np.array_equal(mu, full[2]) and np.array_equal(v, full[3])


def test_host_twin_depends_on_the_global_row_only():
    rng = np.random.default_rng(5)
    B, K, D_, M, seed = 12, 9, 5, 6, 77
    y, lp = particles(rng, B, K, D_)
    whole = host_resample(y, lp, K, M, seed, 100)
    part = host_resample(y[4 * K:9 * K], lp[4 * K:9 * K], K, M, seed, 104)
    for a, b in zip(whole, part):
        assert np.array_equal(a[4:9], b, equal_nan=True)
    assert not np.array_equal(host_resample(y, lp, K, M, seed + 1, 100)[1], whole[1])
    assert not np.array_equal(host_resample(y, lp, K, M, seed, 101)[1], whole[1])
    # the first M' samples of a longer draw are the shorter draw
    assert np.array_equal(host_resample(y, lp, K, 3, seed, 100)[1], whole[1][:, :3])
    # the index of its own: not the block the first noise draw comes from
    assert _native.OBS_RESAMPLE_NOISE_INDEX == RESAMPLE_INDEX < _native.OBS_NOISE_BASE and _native.MAX_OBS_SAMPLES == 4096


@pytest.mark.parametrize("K", [1, 3, 17, 65])
def test_degenerate_points(K):
    rng = np.random.default_rng(K)
    B, D_, M = 6, 5, 4
    y = rng.standard_normal((B * K, D_)).astype(np.float32)
    lp = rng.standard_normal(B * K).astype(np.float32)
    lp[1 * K:2 * K] = -np.inf                            # point 1: no draw has weight
    lp[2 * K + K // 2] = np.nan                          # point 2: a NaN
    lp[3 * K + K // 3] = np.inf                          # point 3: a +inf
    y[4 * K + K - 1, 2] = np.nan                         # point 4: a NaN among the PARTICLES is the caller's: not degenerate
    lp[4 * K + K - 1] = -np.inf                          # ... and at weight zero it is not chosen
    s, i, mu, v = host_resample(y, lp, K, M, 3)
    for r in (1, 2, 3):
        assert (i[r] == -1).all() and np.isnan(s[r]).all() and np.isnan(mu[r]).all() and np.isnan(v[r]).all()
    for r in (0, 5):
        assert (i[r] >= 0).all() and np.isfinite(s[r]).all() and np.isfinite(mu[r]).all() and (v[r] >= 0).all()
    if K > 1:
        assert (i[4] >= 0).all() and (i[4] != K - 1).all() and np.isfinite(s[4]).all()
    else:
        assert (i[4] == -1).all()
    ref = reference_resample(y, lp, K, M, 3)
    assert np.array_equal(i[[0, 5]], ref["index"][[0, 5]])
    if K == 1:
        assert (i[0] == 0).all() and (v[0] == 0).all() and np.array_equal(mu[0], y[0]) and np.array_equal(s[0], np.tile(y[0], (M, 1)))


def test_equal_rows_give_the_row_back():
    """noise_std = 0: the K particles of a point are the point; the weighted mean of K equal numbers is that number to a
    few ulp of double (1e-16 relative: 1e-12 of the bar on var)."""
    rng = np.random.default_rng(2)
    B, D_ = 9, 7
    x = (rng.standard_normal((B, D_)) * 50).astype(np.float32)
    for K in (1, 5, 64):
        y, _ = _native.observe_expand(torch.from_numpy(x), torch.zeros(D_), K, 4, 0)
        lp = rng.standard_normal(B * K).astype(np.float32)
        s, i, mu, v = host_resample(y.numpy(), lp, K, 3, 4)
        assert np.array_equal(s.view(np.uint32), np.repeat(x[:, None, :], 3, axis=1).view(np.uint32))
        assert np.array_equal(mu, x)
        assert (v >= 0).all() and (v <= 1e-24 * np.maximum(1.0, x.astype(np.float64) ** 2)).all()


# ---- the C entry points ----------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments_and_are_exported():
    L = _native.lib()
    for name in ("ff_weighted_resample", "ff_weighted_resample_host"):
        assert hasattr(L, name), name
    B, D_, K, M = 2, 3, 4, 2
    y, lp = torch.ones(B * K, D_), torch.zeros(B * K)
    s, idx = torch.full((B * M + 1, D_), 7.0), torch.full((B * M + 1,), 7, dtype=torch.int32)
    mu, var = torch.full((B + 1, D_), 7.0), torch.full((B + 1, D_), 7.0)
    P = lambda t: t.data_ptr()
    bad, ok, null = _native.FF_ERR_BADARG, _native.FF_OK, None
    # (the device entry point checks its arguments before anything touches a GPU)
    for fn, tail in ((L.ff_weighted_resample_host, ()), (L.ff_weighted_resample, (null,))):
        outs = (P(s), P(idx), P(mu), P(var))
        assert fn(null, P(lp), B, D_, K, M, 1, 0, *outs, *tail) == bad                              # y
        assert fn(P(y), null, B, D_, K, M, 1, 0, *outs, *tail) == bad                               # lp
        assert fn(P(y), P(lp), -1, D_, K, M, 1, 0, *outs, *tail) == bad                             # B
        for d in (0, -1):
            assert fn(P(y), P(lp), B, d, K, M, 1, 0, *outs, *tail) == bad                           # D
        for k in (0, -1, 4097):
            assert fn(P(y), P(lp), B, D_, k, M, 1, 0, *outs, *tail) == bad                          # K
        for m in (-1, 4097):
            assert fn(P(y), P(lp), B, D_, K, m, 1, 0, *outs, *tail) == bad                          # M
        assert fn(P(y), P(lp), B, D_, K, M, 1, 0, null, null, null, null, *tail) == bad             # nothing asked for
        assert fn(P(y), P(lp), 0, D_, K, M, 1, 0, *outs, *tail) == ok                               # B = 0: nothing to do
        assert fn(P(y), P(lp), 0, D_, K, 0, 1, 0, *outs, *tail) == ok
    assert (s == 7.0).all() and (idx == 7).all() and (mu == 7.0).all() and (var == 7.0).all()
    # the host twin writes exactly its outputs; M = 0 ignores samples and index
    assert L.ff_weighted_resample_host(P(y), P(lp), B, D_, K, 0, 1, 0, P(s), P(idx), P(mu), null) == ok
    assert (s == 7.0).all() and (idx == 7).all() and (mu[:B] == 1.0).all() and (mu[B] == 7.0).all() and (var == 7.0).all()
    assert L.ff_weighted_resample_host(P(y), P(lp), B, D_, K, M, 1, 0, P(s), P(idx), P(mu), P(var)) == ok
    assert (s[:B * M] == 1.0).all() and (s[B * M] == 7.0).all() and (idx[:B * M] >= 0).all() and (idx[:B * M] < K).all()
    assert idx[B * M] == 7 and (var[:B] == 0.0).all() and (var[B] == 7.0).all()
    assert L.ff_weighted_resample_host(P(y), P(lp), B, D_, K, M, 1, 0, null, P(idx), null, null) == ok
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert "#define FF_OBS_RESAMPLE_NOISE_INDEX 0xFFFA0000u" in header and "#define FF_MAX_OBS_SAMPLES 4096" in header
    for fn in ("ff_weighted_resample(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed, "
               "int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var, void* hip_stream);",
               "ff_weighted_resample_host(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M, "
               "uint64_t seed, int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var);"):
        assert "int " + fn in header, fn


def test_binding_argument_rules():
    prm = inspect.signature(_native.weighted_resample).parameters
    assert list(prm) == ["y", "lp", "num_draws", "num_samples", "seed", "sample_offset", "want_index", "want_moments"]
    assert (prm["sample_offset"].default, prm["want_index"].default, prm["want_moments"].default) == (0, True, True)
    y, lp = torch.zeros(8, 3), torch.zeros(8)
    for K in (0, 4097):
        with pytest.raises(ValueError, match="num_draws"):
            _native.weighted_resample(y, lp, K, 1, 1)
    for M in (-1, 4097):
        with pytest.raises(ValueError, match="num_samples"):
            _native.weighted_resample(y, lp, 2, M, 1)
    with pytest.raises(RuntimeError, match="y has shape"):
        _native.weighted_resample(y, lp, 3, 1, 1)
    with pytest.raises(RuntimeError, match="lp has shape"):
        _native.weighted_resample(y, torch.zeros(7), 2, 1, 1)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        _native.weighted_resample(y.double(), lp, 2, 1, 1)
    s, i, mu, v = _native.weighted_resample(torch.zeros(0, 3), torch.zeros(0), 5, 2, 1)
    assert s.shape == (0, 2, 3) and i.shape == (0, 2) and i.dtype == torch.int32 and mu.shape == (0, 3) and v.shape == (0, 3)
    s, i, mu, v = _native.weighted_resample(y, lp.view(8, 1), 4, 0, 1)
    assert s.shape == (2, 0, 3) and i.shape == (2, 0) and torch.equal(mu, torch.zeros(2, 3)) and torch.equal(v, torch.zeros(2, 3))
    s, i, mu, v = _native.weighted_resample(y, lp, 4, 0, 1, want_index=False, want_moments=False)
    assert s.shape == (2, 0, 3) and i is None and mu is None and v is None


# ---- the front ends around stub log-densities ------------------------------------------------------------------------------
FIELDS = ("samples", "log_prob", "ess", "mean", "var", "index")


def same(a, b):
    """Two NoisyPosteriors, field by field, bit for bit."""
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def check_posterior(post, x, std, cond, K, M, seed, first, want_lp, want_ess):
    B, D_ = x.shape
    assert type(post) is odeint.NoisyPosterior and post._fields == FIELDS
    assert post.samples.shape == (B, M, D_) and post.index.shape == (B, M) and post.index.dtype == torch.int32
    assert post.mean.shape == (B, D_) and post.var.shape == (B, D_) and post.ess.shape == (B,)
    assert post.log_prob.shape == want_lp.shape and torch.equal(post.log_prob, want_lp) and torch.equal(post.ess, want_ess)
    y, _ = _native.observe_expand(x, std, K, seed, first, cond)
    rows = (torch.arange(B)[:, None] * K + post.index.long()).reshape(-1)
    assert torch.equal(post.samples.reshape(B * M, D_), y[rows])
    assert (post.var >= 0).all()


def test_front_ends_keep_the_particles_log_prob_noisy_drops():
    g = torch.Generator().manual_seed(1)
    B, K, M, seed, first = 11, 4, 3, 77, 2 ** 33 + 5
    x, std, cond = torch.randn(B, 3, generator=g), torch.rand(B, 3, generator=g), torch.randn(B, 2, generator=g)
    assert D.NoisyPosterior is odeint.NoisyPosterior and F.NoisyPosterior is odeint.NoisyPosterior
    assert issubclass(odeint.NoisyPosterior, tuple) and odeint.NoisyPosterior._fields == FIELDS
    models = [(_stubbed(_score(), [], True), (), {}), (_stubbed(_score(hutchinson=True), [], True), (), {"num_probes": 2}),
              (_stubbed(_score(), [], True), (cond,), {}),
              (_stubbed(F.ODEFlow(3, [16]), [], False), (), {}), (_stubbed(F.ODEFlow(3, [16]), [], False), (), {"hutchinson": True}),
              (_stubbed(F.ConditionalODEFlow(3, 2, [16]), [], False), (cond,), {})]
    for m, args, extra in models:
        kw = dict(num_draws=K, seed=seed, sample_offset=first, **extra, **FIXED)
        want_lp, want_ess = m.log_prob_noisy(x, std, *args, return_ess=True, **kw)
        post = m.posterior_noisy(x, std, *args, num_samples=M, **kw)
        check_posterior(post, x, std, args[0] if args else None, K, M, seed, first, want_lp, want_ess)
        # chunks, and row slices with sample_offset moved: the same bits
        for chunk in (1, 7):
            assert same(m.posterior_noisy(x, std, *args, num_samples=M, chunk_points=chunk, **kw), post)
        lo, hi = 3, 9
        part = m.posterior_noisy(x[lo:hi], std[lo:hi], *(a[lo:hi] for a in args), num_samples=M,
                                 **dict(kw, sample_offset=first + lo))
        assert same(part, odeint.NoisyPosterior(*(f[lo:hi] for f in post)))
        assert not torch.equal(m.posterior_noisy(x, std, *args, num_samples=8, **dict(kw, seed=seed + 1)).index,
                               m.posterior_noisy(x, std, *args, num_samples=8, **kw).index)
        # num_samples = 0: moments only; the defaults: one sample
        p0 = m.posterior_noisy(x, std, *args, num_samples=0, **kw)
        assert p0.samples.shape == (B, 0, 3) and p0.index.shape == (B, 0) and torch.equal(p0.mean, post.mean)
        assert m.posterior_noisy(x, std, *args, **kw).samples.shape == (B, 1, 3)
        with pytest.raises(ValueError, match="chunk_points"):
            m.posterior_noisy(x, std, *args, num_draws=K, chunk_points=2, **extra)                  # the adaptive default
        with pytest.raises(ValueError, match="num_samples"):
            m.posterior_noisy(x, std, *args, num_samples=4097, **kw)
        with pytest.raises(ValueError, match=r"posterior_noisy: x must be a \[batch, dim\] float32"):
            m.posterior_noisy(x.double(), std, *args, **kw)
        e0 = m.posterior_noisy(x[:0], std[:0], *(a[:0] for a in args), num_samples=M, **kw)
        assert e0.samples.shape == (0, M, 3) and e0.index.shape == (0, M) and e0.mean.shape == (0, 3) and e0.ess.shape == (0,)
    # the Hutchinson probes are keyed as log_prob_noisy keys them
    calls = []
    hm = _stubbed(_score(hutchinson=True), calls, True)
    hm.posterior_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, chunk_points=3, num_probes=5, **FIXED)
    assert [(c["probe"], c["seed"], c["sample_offset"], c["num_probes"]) for c in calls] == \
        [("philox", seed, (first + lo) * K, 5) for lo in (0, 3, 6, 9)]
    # the default adaptive method: all B K rows, one solve; seed=None: one draw of torch's generator
    calls = []
    sm = _stubbed(_score(), calls, True)
    torch.manual_seed(5)
    a = sm.posterior_noisy(x, std, num_draws=K)
    assert [c["rows"] for c in calls] == [B * K] and calls[0]["method"] == "dopri5" and calls[0]["options"] == {"min_step": 1e-6}
    torch.manual_seed(5)
    s = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert same(sm.posterior_noisy(x, std, num_draws=K, seed=s), a)
    # the default chunk: chunk_points K <= OBSERVE_CHUNK_ROWS
    del calls[:]
    old, odeint.OBSERVE_CHUNK_ROWS = odeint.OBSERVE_CHUNK_ROWS, 5 * K + 3
    try:
        b = sm.posterior_noisy(x, std, num_draws=K, seed=s, **FIXED)
    finally:
        odeint.OBSERVE_CHUNK_ROWS = old
    assert [c["rows"] for c in calls] == [5 * K, 5 * K, K] and same(b, sm.posterior_noisy(x, std, num_draws=K, seed=s, **FIXED))


def test_population_wrappers_return_the_units_of_x():
    g = torch.Generator().manual_seed(2)
    B, K, M, seed = 6, 3, 4, 9
    x, std, cond = torch.randn(B, 3, generator=g) * 30 + 100, torch.rand(3, generator=g), torch.randn(B, 2, generator=g)
    stub = lambda rows, c, atol, rtol, num_probes, probe_rng=None: (
        rows.double().sum(1).float() + (0.0 if c is None else c.sum(1))).view(-1, 1)
    for hutch in (False, True):
        pm = D.PopulationModelDiffusion(D.MLP(3, 0, 8, [16]), D.VPSDE(), shift=torch.full((3,), 100.0), scale=torch.full((3,), 30.0),
                                        hutchinson=hutch)
        pm._log_prob = stub
        want_lp, want_ess = pm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=4, return_ess=True)
        post = pm.posterior_noisy(x, std, num_draws=K, num_samples=M, seed=seed, sample_offset=4)
        check_posterior(post, x, std, None, K, M, seed, 4, want_lp, want_ess)
        assert post.log_prob.shape == (B, 1) and (post.mean - x).abs().max() < 5          # data space: near x, not near 0
        with pytest.raises(ValueError, match="chunk_points"):
            pm.posterior_noisy(x, std, num_draws=K, chunk_points=2)
    pc = D.PopulationModelDiffusionConditional(D.MLP(3, 2, 8, [16]), D.VPSDE())
    pc._log_prob = stub
    want_lp, want_ess = pc.log_prob_noisy(x, std, cond, num_draws=K, seed=seed, return_ess=True)
    check_posterior(pc.posterior_noisy(x, std, cond, num_draws=K, num_samples=M, seed=seed), x, std, cond, K, M, seed, 0,
                    want_lp, want_ess)


def test_signatures_and_docstrings():
    KW = inspect.Parameter.KEYWORD_ONLY
    from flowfusion_amd.symplectic import SymplecticFlowModel
    assert not hasattr(SymplecticFlowModel, "posterior_noisy")
    for cls in (D.ScoreModel, F.ODEFlow, F.ConditionalODEFlow, D.PopulationModelDiffusion, D.PopulationModelDiffusionConditional):
        noisy = inspect.signature(cls.log_prob_noisy).parameters
        post = inspect.signature(cls.posterior_noisy).parameters
        # log_prob_noisy's parameters with num_samples after num_draws and without return_ess; the same defaults
        want = [n for n in noisy if n != "return_ess"]
        want.insert(want.index("num_draws") + 1, "num_samples")
        assert list(post) == want, cls
        assert post["num_samples"].default == 1 and post["num_samples"].kind is not KW
        assert all(post[n].default == noisy[n].default and post[n].kind == noisy[n].kind for n in want if n != "num_samples"), cls
        assert all(post[n].kind is KW for n in ("seed", "sample_offset", "chunk_points")), cls
        assert "ess" in cls.posterior_noisy.__doc__ and "num_draws" in cls.posterior_noisy.__doc__
    for doc in (D.ScoreModel.posterior_noisy.__doc__, F._FlowBase._posterior_noisy.__doc__):
        flat = " ".join(doc.split())
        assert "effective sample size" in flat and "raise ``num_draws``, not ``num_samples``" in flat and "clean case" in flat
        assert "before trusting ``samples``" in flat
    from flowfusion_amd.distributed import log_prob_noisy_sharded, posterior_noisy_sharded
    a, b = inspect.signature(log_prob_noisy_sharded).parameters, inspect.signature(posterior_noisy_sharded).parameters
    want = [n for n in a if n != "return_ess"]
    want.insert(want.index("num_draws") + 1, "num_samples")
    assert list(b) == want and all(b[n].default == a[n].default and b[n].kind == a[n].kind for n in want if n != "num_samples")


# ---- the sharded entry point over gloo -------------------------------------------------------------------------------------
def _worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import posterior_noisy_sharded, shard_bounds
        gathers = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, inp, **kw: (gathers.append(tuple(inp.shape)), real(out, inp, **kw))[1]
        torch.manual_seed(0)
        x, std, c = torch.randn(n, 3), torch.rand(n, 3), torch.randn(n, 2)
        lo, hi = shard_bounds(n, world, rank)
        K, M, seed = 5, 4, 9
        width = M * 3 + 2 * 3 + 2 + M
        ok = True
        for hutch in (False, True):
            m = _row_keyed(_score(hutchinson=hutch), True)
            want = m.posterior_noisy(x, std, c, num_draws=K, num_samples=M, seed=seed, **FIXED)
            del gathers[:]
            got = posterior_noisy_sharded(m, x, std, c, seed=seed, num_draws=K, num_samples=M, **FIXED)
            ok &= len(gathers) == 1 and gathers[0][1:] == (width,) and type(got) is odeint.NoisyPosterior and same(got, want)
            mine = posterior_noisy_sharded(m, local_x=x[lo:hi], local_noise_std=std[lo:hi], local_conditional=c[lo:hi], n_total=n,
                                           seed=seed, num_draws=K, num_samples=M, **FIXED)
            ok &= len(gathers) == 2 and same(mine, want)
            local, span = posterior_noisy_sharded(m, x, std, c, seed=seed, num_draws=K, num_samples=M, gather=False, **FIXED)
            ok &= span == (lo, hi) and len(gathers) == 2 and same(local, odeint.NoisyPosterior(*(f[lo:hi] for f in want)))
            # a [D] noise_std is replicated
            want1 = m.posterior_noisy(x, std[0], c, num_draws=K, num_samples=M, seed=seed, **FIXED)
            ok &= same(posterior_noisy_sharded(m, x, std[0], c, seed=seed, num_draws=K, num_samples=M, **FIXED), want1)
            fk = dict(FIXED, hutchinson=hutch)
            f = _row_keyed(F.ODEFlow(3, [16]), False)
            wantf = f.posterior_noisy(x, std, num_draws=K, num_samples=M, seed=seed, **fk)
            gotf = posterior_noisy_sharded(f, x, std, seed=seed, num_draws=K, num_samples=M, **fk)
            ok &= gotf.log_prob.shape == (n,) and same(gotf, wantf)
            fc = _row_keyed(F.ConditionalODEFlow(3, 2, [16]), False)
            ok &= same(posterior_noisy_sharded(fc, x, std, c, seed=seed, num_draws=K, num_samples=0, **fk),
                       fc.posterior_noisy(x, std, c, num_draws=K, num_samples=0, seed=seed, **fk))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 37), (3, 37)])                    # ragged shards over two and three ranks
def test_sharded_equals_the_single_process_call(world, n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    results = dict(q.get(timeout=5) for _ in range(world))
    assert results == {r: True for r in range(world)}


def test_sharded_argument_rules_and_one_process():
    from flowfusion_amd.distributed import posterior_noisy_sharded
    m = _row_keyed(_score(), True)
    x, std = torch.randn(6, 3), torch.rand(6, 3)
    with pytest.raises(ValueError, match="noise_std"):
        posterior_noisy_sharded(m, x, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std"):
        posterior_noisy_sharded(m, x, std, local_noise_std=std, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std must hold"):
        posterior_noisy_sharded(m, local_x=x, local_noise_std=std[:5], n_total=6, seed=1, **FIXED)
    want = m.posterior_noisy(x, std, num_draws=4, num_samples=3, seed=3, **FIXED)
    assert same(posterior_noisy_sharded(m, x, std, seed=3, num_draws=4, num_samples=3, **FIXED), want)
    got, span = posterior_noisy_sharded(m, local_x=x, local_noise_std=std, n_total=6, seed=3, num_draws=4, num_samples=3,
                                        gather=False, **FIXED)
    assert span == (0, 6) and same(got, want)


# ---- known answer ------------------------------------------------------------------------------------------------------------
def exact_posterior(x, shift, scale, sigma):
    """(mean, variance) [B, D] float64 of p(x_true | x) for the prior N(shift, scale^2) and noise sigma."""
    s2, n2 = scale.astype(np.float64) ** 2, sigma.astype(np.float64) ** 2
    return (x.astype(np.float64) * s2 + shift * n2) / (s2 + n2), s2 * n2 / (s2 + n2)


def check_known_answer(posterior_of):
    """The four assertions, on ``posterior_of(K, M) -> (samples, mean, var, ess)`` as numpy arrays for the inputs of
    ``closed_form_inputs()``.  The float64 statement of the estimator on these inputs gives an RMS error of ``mean`` of
    0.603 / 0.300 / 0.150 / 0.078 posterior standard deviations at K = 4 / 16 / 64 / 256 (theory: halved per factor 4), a
    mean of var / exact of 0.992, a pooled variance of the standardised samples of 1.003 and a mean ess of 182 at K = 256."""
    B, D_, seed, shift, scale, sigma, x = closed_form_inputs()
    mu, v = exact_posterior(x, shift, scale, sigma)
    rms = {}
    for K in (4, 64):
        _, mean, _, _ = posterior_of(K, 0)
        rms[K] = float(np.sqrt(np.mean((mean.astype(np.float64) - mu) ** 2 / v)))
    samples, mean, var, ess = posterior_of(256, 8)
    rms[256] = float(np.sqrt(np.mean((mean.astype(np.float64) - mu) ** 2 / v)))
    var_ratio = float(np.mean(var.astype(np.float64) / v))
    pooled = float(np.var((samples.astype(np.float64) - mu[:, None, :]) / np.sqrt(v)[:, None, :]))
    print(f"gaussian posterior: rms error of mean K=4 {rms[4]:.4f}, K=64 {rms[64]:.4f}, K=256 {rms[256]:.4f} posterior sd; "
          f"K=256: var/exact {var_ratio:.4f}, pooled sample variance {pooled:.4f}, mean ess {ess.mean():.1f}")
    assert rms[64] <= 0.35 * rms[4], rms
    assert var_ratio >= 0.9
    assert 0.9 <= pooled <= 1.1
    assert 64.0 < ess.mean() <= 256.0


def test_known_answer_gaussian_posterior():
    B, D_, seed, shift, scale, sigma, x = closed_form_inputs()
    sc = scale.astype(np.float64)

    def posterior_of(K, M):
        y = _native.observe_expand(torch.from_numpy(x), torch.from_numpy(sigma), K, seed, 0)[0]
        y64 = y.numpy().astype(np.float64)
        lp = ((-0.5 * ((y64 - shift) / sc) ** 2 - 0.5 * math.log(2 * math.pi)).sum(1) - np.log(sc).sum()).astype(np.float32)
        lp = torch.from_numpy(lp)
        ess = torch.empty(B)
        _native.logmeanexp(lp, K, None, ess)
        s, _, mean, var = _native.weighted_resample(y, lp, K, M, seed, 0)
        return s.numpy(), mean.numpy(), var.numpy(), ess.numpy()

    check_known_answer(posterior_of)
