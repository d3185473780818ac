"""CPU tier of the log-density of noisy observations: the two ends of the K-draw estimate (csrc/ff_observe.h through its
host entry points ff_observe_expand_host / ff_logmeanexp_host), the argument rules of the C entry points, the front
ends' ``log_prob_noisy`` around stub log-densities, and ``log_prob_noisy_sharded`` over gloo.

Anchors: tests/_philox.py and numpy's fp32 arithmetic for what expand writes; numpy in float64 for what the reduction
returns; and a closed form independent of both -- noise of standard deviation sigma on a Gaussian N(shift, scale^2) is the
Gaussian N(shift, scale^2 + sigma^2), so the K-draw estimate must close in on it as K grows."""
import inspect
import math
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flowfusion_amd import _native, odeint
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F
from tests._philox import normals

ROOT = Path(__file__).resolve().parent.parent
BASE = 0xFFFB0000
FILL_BAR = 2e-6             # device / libm normals against tests/_philox.py (tests/test_gpu_stream_kernels.py FILL_BAR)
KS = [1, 3, 8, 17, 65, 4096]


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


def one_rounding_bar(ref):
    """|got - ref| <= 1.2e-7 |ref| + 1e-10: one fp32 rounding (2^-24 = 6e-8 relative) of a result computed in double."""
    return 1.2e-7 * np.abs(ref) + 1e-10


def reference_logmeanexp(lp, K):
    """(out [B], ess [B]) in float64 numpy from lp [B K]; the semantics of torch.logsumexp for non-finite entries (the
    maximum replaced by 0 where it is not finite)."""
    lw = lp.astype(np.float64).reshape(-1, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = lw.max(1, keepdims=True)
        m0 = np.where(np.isfinite(m), m, 0.0)
        w = np.exp(lw - m0)
        out = np.log(w.sum(1)) + m0[:, 0] - math.log(K)
        wm = np.exp(lw - m)                                   # the weights the header defines: relative to the maximum itself
        ess = wm.sum(1) ** 2 / (wm * wm).sum(1)
    return out, ess


def host_logmeanexp(lp, K, want_ess=True):
    lp = torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32))
    ess = torch.empty(lp.numel() // K) if want_ess else None
    out = _native.logmeanexp(lp, K, None, ess)
    return out.numpy(), None if ess is None else ess.numpy()


# ---- expand ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2 ** 33 + 7])
@pytest.mark.parametrize("D_", [1, 3, 4, 5, 16, 33])
def test_host_expand_against_the_stream_and_numpy(D_, offset):
    """y = x - s z with z the stream's normal: the twin's z comes through libm and agrees with tests/_philox.py to FILL_BAR
    (relative to max(1, |z|)); the product and the difference add one fp32 rounding each (2^-24 relative, 1.2e-7 with
    slack) -- so |y - ref| <= s FILL_BAR max(1, |z|) + 1.2e-7 (|s z| + |ref|)."""
    rng = np.random.default_rng(D_)
    B, C, seed = 7, 3, 99 + D_
    x = (rng.standard_normal((B, D_)) * 2).astype(np.float32)
    cond = rng.standard_normal((B, C)).astype(np.float32)
    for K in (1, 5):
        z = normals(seed, offset, B, D_, [BASE + k for k in range(K)]).transpose(1, 0, 2).astype(np.float64)     # [B, K, D]
        for std in ((rng.random((B, D_)) * 1.5).astype(np.float32), (rng.random(D_) * 1.5).astype(np.float32)):
            for cd in (cond, None):
                y, co = _native.observe_expand(torch.from_numpy(x), torch.from_numpy(std), K, seed, offset,
                                               None if cd is None else torch.from_numpy(cd))
                y = y.numpy()
                assert y.shape == (B * K, D_) and y.dtype == np.float32 and np.isfinite(y).all()
                s = np.broadcast_to(std, (B, D_)).astype(np.float64)[:, None, :]
                ref = x.astype(np.float64)[:, None, :] - s * z
                bar = s * FILL_BAR * np.maximum(1.0, np.abs(z)) + 1.2e-7 * (np.abs(s * z) + np.abs(ref)) + 1e-30
                err = np.abs(y.reshape(B, K, D_).astype(np.float64) - ref)
                assert (err <= bar).all(), (D_, K, float((err / bar).max()))
                if cd is None:
                    assert co is None
                else:
                    assert np.array_equal(co.numpy().view(np.uint32), np.repeat(cd, K, axis=0).view(np.uint32))
        # sigma = 0: the observation itself, K times
        y0, _ = _native.observe_expand(torch.from_numpy(x), torch.zeros(D_), K, seed, offset)
        assert np.array_equal(y0.numpy(), np.repeat(x, K, axis=0))


def test_host_expand_draws_differ_by_draw_row_and_seed():
    x, s = torch.zeros(4, 8), torch.ones(8)
    a = _native.observe_expand(x, s, 3, 5, 0)[0].numpy()
    assert len({a[i].tobytes() for i in range(12)}) == 12
    assert not np.array_equal(_native.observe_expand(x, s, 3, 6, 0)[0].numpy(), a)
    assert np.array_equal(_native.observe_expand(x[:2], s, 3, 5, 2)[0].numpy(), a[6:])              # rows 2, 3 of the stream
    # a range of its own: not the momenta's, not the Hutchinson probes'
    p = _native.marginal_expand(x, 3, 5, 0)[0].numpy()[:, 8:]
    assert not np.array_equal(-a, p)
    assert _native.OBS_NOISE_BASE == BASE and BASE + _native.MAX_OBS_DRAWS <= _native.HUTCH_PROBE_NOISE_BASE


# ---- logmeanexp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_host_logmeanexp_against_float64(K):
    rng = np.random.default_rng(K)
    B = 5
    lp = (rng.standard_normal(B * K) * 4 - 30).astype(np.float32)
    lp[:K] = lp[0]                                                           # K equal values: their common value, ess = K
    lp[K:2 * K] *= 25                                                        # a spread of hundreds of nats: weights underflow
    want, want_ess = reference_logmeanexp(lp, K)
    got, ess = host_logmeanexp(lp, K)
    assert (np.abs(got - want) <= one_rounding_bar(want)).all(), (got, want)
    assert (np.abs(ess - want_ess) <= one_rounding_bar(want_ess)).all(), (ess, want_ess)
    assert ((ess > 0) & (ess <= K * (1 + 1e-6))).all()
    only, none = host_logmeanexp(lp, K, want_ess=False)
    assert none is None and np.array_equal(only, got)
    if K == 1:                                                               # one draw is its own mean, bit for bit
        assert np.array_equal(got.view(np.uint32), lp.view(np.uint32)) and (ess == 1.0).all()


@pytest.mark.parametrize("K", KS)
def test_host_logmeanexp_non_finite_rows_follow_logsumexp(K):
    rng = np.random.default_rng(100 + K)
    B = 5
    lp = (rng.standard_normal(B * K) * 2).astype(np.float32)
    lp[0 * K + (K - 1)] = -np.inf                        # point 0: one draw of weight zero (the last one)
    lp[1 * K:2 * K] = -np.inf                            # point 1: every draw of weight zero
    lp[2 * K + K // 2] = np.nan                          # point 2: a NaN
    lp[3 * K + K // 3] = np.inf                          # point 3: a +inf entry
    want, want_ess = reference_logmeanexp(lp, K)
    ref = torch.logsumexp(torch.from_numpy(lp).double().view(B, K), dim=1) - math.log(K)
    got, ess = host_logmeanexp(lp, K)
    assert np.isnan(got[2]) and np.isnan(ess[2]) and bool(torch.isnan(ref[2]))
    assert got[1] == -np.inf and np.isnan(ess[1]) and float(ref[1]) == -np.inf
    assert got[3] == np.inf and float(ref[3]) == np.inf
    assert abs(got[4] - want[4]) <= one_rounding_bar(want[4]) and abs(ess[4] - want_ess[4]) <= one_rounding_bar(want_ess[4])
    if K == 1:
        assert got[0] == -np.inf
    else:
        assert np.isfinite(got[0]) and abs(got[0] - want[0]) <= one_rounding_bar(want[0])
        assert abs(got[0] - float(ref[0])) <= one_rounding_bar(float(ref[0]))
        assert abs(ess[0] - want_ess[0]) <= one_rounding_bar(want_ess[0])


# ---- closed form -----------------------------------------------------------------------------------------------------------
def closed_form_inputs():
    """(B, D, seed, shift, scale, sigma [B, D], x [B, D]): 256 observations of N(shift, scale^2) with per-object errors of
    0.2 .. 0.6 scale, drawn from the convolved density itself.  Chosen before any device run: profiles/observe.txt holds
    the float64 estimator's two RMS values on these inputs."""
    B, D_ = 256, 3
    rng = np.random.default_rng(0)
    shift = np.array([0.4, -1.1, 2.0], dtype=np.float32)
    scale = np.array([0.7, 1.6, 1.1], dtype=np.float32)
    sigma = (scale * rng.uniform(0.2, 0.6, size=(B, D_))).astype(np.float32)
    x = (shift + np.sqrt(scale.astype(np.float64) ** 2 + sigma.astype(np.float64) ** 2) * rng.standard_normal((B, D_)))
    return B, D_, 8, shift, scale, sigma, x.astype(np.float32)


def exact_observed(x, shift, scale, sigma):
    """log N(x; shift, scale^2 + sigma^2) summed over the dimensions, float64."""
    var = scale.astype(np.float64) ** 2 + sigma.astype(np.float64) ** 2
    return (-0.5 * (x.astype(np.float64) - shift) ** 2 / var - 0.5 * np.log(2 * math.pi * var)).sum(1)


def test_closed_form_gaussian_convolution():
    """RMS error against N(shift, scale^2 + sigma^2): K = 64 at most 0.35 of K = 4 (theory: 0.25; this float64 statement of
    the same draws gives 0.379 and 0.088 nats, a ratio of 0.232); the mean effective sample size at K = 64 in (1, 64]."""
    B, D_, seed, shift, scale, sigma, x = closed_form_inputs()
    exact = exact_observed(x, shift, scale, sigma)
    sc = scale.astype(np.float64)
    rms, ess64 = {}, None
    for K in (4, 64):
        y = _native.observe_expand(torch.from_numpy(x), torch.from_numpy(sigma), K, seed, 0)[0].numpy().astype(np.float64)
        lp = (-0.5 * ((y - shift) / sc) ** 2 - 0.5 * math.log(2 * math.pi)).sum(1) - np.log(sc).sum()
        got, ess = host_logmeanexp(lp, K)
        rms[K] = float(np.sqrt(np.mean((got.astype(np.float64) - exact) ** 2)))
        ess64 = ess
    print(f"gaussian convolution: rms error K=4 {rms[4]:.4f}, K=64 {rms[64]:.4f} nats; mean ess {ess64.mean():.2f}")
    assert rms[64] <= 0.35 * rms[4], rms
    assert 1.0 < ess64.mean() <= 64.0


# ---- the C entry points ------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments_and_are_exported():
    L = _native.lib()
    for name in ("ff_observe_expand", "ff_logmeanexp", "ff_observe_expand_host", "ff_logmeanexp_host"):
        assert hasattr(L, name), name
    B, D_, C, K = 2, 3, 2, 4
    x, s, cond = torch.zeros(B, D_), torch.ones(B, D_), torch.zeros(B, C)
    y, co = torch.full((B * K + 1, D_), 7.0), torch.full((B * K + 1, C), 7.0)
    lp, out, ess = torch.zeros(B * K), torch.full((B + 1,), 7.0), torch.full((B + 1,), 7.0)
    P = lambda t: t.data_ptr()
    bad, ok = _native.FF_ERR_BADARG, _native.FF_OK
    null = None
    # (the device entry points check their arguments before anything touches a GPU)
    for fn, tail in ((L.ff_observe_expand_host, ()), (L.ff_observe_expand, (null,))):
        assert fn(null, P(s), D_, null, B, D_, 0, K, 1, 0, P(y), null, *tail) == bad                 # x
        assert fn(P(x), null, D_, null, B, D_, 0, K, 1, 0, P(y), null, *tail) == bad                 # noise_std
        assert fn(P(x), P(s), D_, null, B, D_, 0, K, 1, 0, null, null, *tail) == bad                 # y
        assert fn(P(x), P(s), D_, null, -1, D_, 0, K, 1, 0, P(y), null, *tail) == bad                # B
        assert fn(P(x), P(s), 0, null, B, 0, 0, K, 1, 0, P(y), null, *tail) == bad                   # D
        for k in (0, -1, 4097):
            assert fn(P(x), P(s), D_, null, B, D_, 0, k, 1, 0, P(y), null, *tail) == bad             # K
        for stride in (1, D_ - 1, D_ + 1, 2 * D_, -D_):
            assert fn(P(x), P(s), stride, null, B, D_, 0, K, 1, 0, P(y), null, *tail) == bad         # std_row_stride
        assert fn(P(x), P(s), D_, P(cond), B, D_, C, K, 1, 0, P(y), null, *tail) == bad              # cond without cond_out
        assert fn(P(x), P(s), D_, P(cond), B, D_, 0, K, 1, 0, P(y), P(co), *tail) == bad             # cond with C = 0
        assert fn(P(x), P(s), D_, null, 0, D_, 0, K, 1, 0, P(y), null, *tail) == ok                  # B = 0: nothing to do
        assert fn(P(x), P(s), 0, null, 0, D_, 0, K, 1, 0, P(y), null, *tail) == ok
    for fn, tail in ((L.ff_logmeanexp_host, ()), (L.ff_logmeanexp, (null,))):
        assert fn(null, B, K, P(out), null, *tail) == bad                                            # lp
        assert fn(P(lp), B, K, null, null, *tail) == bad                                             # out
        assert fn(P(lp), -1, K, P(out), null, *tail) == bad
        for k in (0, -1, 4097):
            assert fn(P(lp), B, k, P(out), null, *tail) == bad
        assert fn(P(lp), 0, K, P(out), P(ess), *tail) == ok
    assert (y == 7.0).all() and (co == 7.0).all() and (out == 7.0).all() and (ess == 7.0).all()
    # the host twins write exactly their outputs
    assert L.ff_observe_expand_host(P(x), P(s), 0, P(cond), B, D_, C, K, 1, 0, P(y), P(co)) == ok
    assert (y[B * K] == 7.0).all() and (co[B * K] == 7.0).all() and (y[:B * K] != 7.0).all() and (co[:B * K] == 0).all()
    assert L.ff_logmeanexp_host(P(lp), B, K, P(out), P(ess)) == ok
    assert out[B] == 7.0 and ess[B] == 7.0 and (out[:B] == 0).all() and (ess[:B] == K).all()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert "#define FF_OBS_NOISE_BASE 0xFFFB0000u" in header and "#define FF_MAX_OBS_DRAWS 4096" in header


def test_binding_argument_rules():
    x = torch.zeros(4, 3)
    for K in (0, 4097):
        with pytest.raises(ValueError, match="num_draws"):
            _native.observe_expand(x, torch.ones(3), K, 1)
        with pytest.raises(ValueError, match="num_draws"):
            _native.logmeanexp(torch.zeros(8), K)
    with pytest.raises(RuntimeError, match="noise_std has shape"):
        _native.observe_expand(x, torch.ones(4), 2, 1)
    with pytest.raises(RuntimeError, match="noise_std has shape"):
        _native.observe_expand(x, torch.ones(3, 3), 2, 1)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        _native.observe_expand(x.double(), torch.ones(3), 2, 1)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        _native.observe_expand(x, torch.ones(3, 4).t(), 2, 1)
    with pytest.raises(RuntimeError, match="cond has shape"):
        _native.observe_expand(x, torch.ones(3), 2, 1, cond=torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="lp has shape"):
        _native.logmeanexp(torch.zeros(7), 2)
    with pytest.raises(RuntimeError, match="out has"):
        _native.logmeanexp(torch.zeros(8), 2, out=torch.zeros(3))
    y, c = _native.observe_expand(torch.zeros(0, 3), torch.ones(3), 5, 1)
    assert y.shape == (0, 3) and c is None and _native.logmeanexp(torch.zeros(0), 5).shape == (0,)
    assert _native.logmeanexp(torch.zeros(6, 1), 3).shape == (2,)


# ---- the front ends around stub log-densities ----------------------------------------------------------------------------------
FIXED = dict(method="rk4", options={"step_size": 0.25})


def _stubbed(model, calls, column):
    """``model`` with its ``log_prob`` replaced by a row-wise function that records what it was handed."""
    def log_prob(rows, *args, **kw):
        cond = args[0] if args else kw.pop("conditional", None)
        calls.append({"rows": int(rows.shape[0]), "cond": None if cond is None else tuple(cond.shape), **kw})
        lp = rows.double().sum(1).float() + (0.0 if cond is None else cond.sum(1))
        return lp.view(-1, 1) if column else lp
    model.log_prob = log_prob
    return model


def _score(hutchinson=False):
    torch.manual_seed(3)
    return D.ScoreModel(D.MLP(n_dimensions=3, n_conditionals=0, embedding_dimensions=8, units=[16]), D.VPSDE(), no_sigma=True,
                        hutchinson=hutchinson).eval()


def _expected(x, std, cond, K, seed, first=0):
    y, ck = _native.observe_expand(x, std, K, seed, first, cond)
    lp = y.double().sum(1).float() + (0.0 if ck is None else ck.sum(1))
    ess = torch.empty(x.shape[0])
    return _native.logmeanexp(lp, K, None, ess), ess


def test_front_end_shapes_and_chunk_offsets():
    g = torch.Generator().manual_seed(1)
    B, K, seed, first = 11, 4, 77, 2 ** 33 + 5
    x, std, cond = torch.randn(B, 3, generator=g), torch.rand(B, 3, generator=g), torch.randn(B, 2, generator=g)
    want, want_ess = _expected(x, std, None, K, seed, first)
    want_c, _ = _expected(x, std, cond, K, seed, first)
    # ScoreModel, exact trace: [B, 1]; log_prob sees chunks of chunk_points K rows and no probe keywords
    calls = []
    sm = _stubbed(_score(), calls, column=True)
    lp, ess = sm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, chunk_points=4, return_ess=True, **FIXED)
    assert lp.shape == (B, 1) and ess.shape == (B,) and torch.equal(lp[:, 0], want) and torch.equal(ess, want_ess)
    assert [c["rows"] for c in calls] == [16, 16, 12] and all("probe" not in c and "seed" not in c for c in calls)
    assert all(c["atol"] == 1e-4 and c["rtol"] == 1e-4 and c["num_probes"] == 1 and c["method"] == "rk4" for c in calls)
    only = sm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, **FIXED)
    assert torch.is_tensor(only) and only.shape == (B, 1) and torch.equal(only, lp)                  # one chunk: the same bits
    assert torch.equal(sm.log_prob_noisy(x, std, cond, K, seed=seed, sample_offset=first, **FIXED)[:, 0], want_c)
    del calls[:]
    # the default adaptive method: all B K rows, one solve
    assert sm.log_prob_noisy(x, std, num_draws=K, seed=seed).shape == (B, 1)
    assert [c["rows"] for c in calls] == [B * K] and calls[0]["method"] == "dopri5" and calls[0]["options"] == {"min_step": 1e-6}
    # a Hutchinson model: philox probes under the same seed, keyed by the expanded global row
    calls = []
    hm = _stubbed(_score(hutchinson=True), calls, column=True)
    lp_h = hm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, chunk_points=3, num_probes=5, **FIXED)
    assert torch.equal(lp_h, lp)
    assert [(c["probe"], c["seed"], c["sample_offset"], c["num_probes"]) for c in calls] == \
        [("philox", seed, (first + lo) * K, 5) for lo in (0, 3, 6, 9)]
    # the default chunk: chunk_points K <= OBSERVE_CHUNK_ROWS
    calls = []
    hm = _stubbed(_score(hutchinson=True), calls, column=True)
    old, odeint.OBSERVE_CHUNK_ROWS = odeint.OBSERVE_CHUNK_ROWS, 5 * K + 3
    try:
        assert torch.equal(hm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=first, **FIXED), lp)
    finally:
        odeint.OBSERVE_CHUNK_ROWS = old
    assert [c["sample_offset"] for c in calls] == [(first + lo) * K for lo in (0, 5, 10)]
    assert odeint.OBSERVE_CHUNK_ROWS == 2 ** 22
    # the flows: [B]
    for flow, args, ref in ((F.ODEFlow(3, [16]), (), want), (F.ConditionalODEFlow(3, 2, [16]), (cond,), want_c)):
        calls = []
        f = _stubbed(flow, calls, column=False)
        a, e = f.log_prob_noisy(x, std, *args, num_draws=K, seed=seed, sample_offset=first, chunk_points=7, return_ess=True, **FIXED)
        assert a.shape == (B,) and e.shape == (B,) and torch.equal(a, ref)
        assert [c["rows"] for c in calls] == [28, 16] and all(c["hutchinson"] is False and "probe" not in c for c in calls)
        assert all(c["cond"] == (None if not args else (c["rows"], 2)) for c in calls)
        assert all(c["atol"] == 1e-5 and c["rtol"] == 1e-5 for c in calls)
        del calls[:]
        b = f.log_prob_noisy(x, std, *args, num_draws=K, seed=seed, sample_offset=first, chunk_points=7, hutchinson=True, **FIXED)
        assert b.shape == (B,) and torch.equal(b, ref)
        assert [(c["hutchinson"], c["probe"], c["seed"], c["sample_offset"]) for c in calls] == \
            [(True, "philox", seed, (first + lo) * K) for lo in (0, 7)]
    # noise_std: [D] and scalars go out as one [D] vector
    for std1 in (torch.full((3,), 0.5), 0.5, torch.tensor(0.5), torch.tensor(0.5, dtype=torch.float64)):
        got = sm.log_prob_noisy(x, std1, num_draws=K, seed=seed, sample_offset=first, **FIXED)
        assert torch.equal(got[:, 0], _expected(x, torch.full((3,), 0.5), None, K, seed, first)[0])
    # noise_std = 0, one draw: the stub's value on x itself
    assert torch.equal(sm.log_prob_noisy(x, 0.0, num_draws=1, **FIXED)[:, 0], x.double().sum(1).float())
    # seed=None: one draw of torch's generator
    torch.manual_seed(5)
    a, b = sm.log_prob_noisy(x, std, num_draws=K, **FIXED), sm.log_prob_noisy(x, std, num_draws=K, **FIXED)
    torch.manual_seed(5)
    s = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert not torch.equal(a, b) and torch.equal(sm.log_prob_noisy(x, std, num_draws=K, seed=s, **FIXED), a)
    # an empty batch
    e0 = sm.log_prob_noisy(x[:0], std[:0], num_draws=K, seed=1, return_ess=True, **FIXED)
    assert e0[0].shape == (0, 1) and e0[1].shape == (0,)


def test_population_wrappers_go_through_their_own_log_prob():
    g = torch.Generator().manual_seed(2)
    B, K, seed = 6, 3, 9
    x, std, cond = torch.randn(B, 3, generator=g), torch.rand(3, generator=g), torch.randn(B, 2, generator=g)
    for hutch in (False, True):
        pm = D.PopulationModelDiffusion(D.MLP(3, 0, 8, [16]), D.VPSDE(), shift=torch.randn(3), scale=torch.rand(3) + 0.5,
                                        hutchinson=hutch)
        calls = []
        pm._log_prob = lambda rows, c, atol, rtol, num_probes, probe_rng=None: (
            calls.append((int(rows.shape[0]), c, atol, rtol, num_probes, probe_rng)), rows.double().sum(1).float().view(-1, 1))[1]
        lp, ess = pm.log_prob_noisy(x, std, num_draws=K, seed=seed, sample_offset=4, return_ess=True, num_probes=2 if hutch else 1)
        assert lp.shape == (B, 1) and ess.shape == (B,) and torch.equal(lp[:, 0], _expected(x, std, None, K, seed, 4)[0])
        assert calls == [(B * K, None, 1e-5, 1e-5, 2 if hutch else 1, (seed, 4 * K) if hutch else None)]
        with pytest.raises(ValueError, match="chunk_points"):
            pm.log_prob_noisy(x, std, num_draws=K, chunk_points=2)
    pc = D.PopulationModelDiffusionConditional(D.MLP(3, 2, 8, [16]), D.VPSDE())
    calls = []
    pc._log_prob = lambda rows, c, atol, rtol, num_probes, probe_rng=None: (
        calls.append((int(rows.shape[0]), tuple(c.shape), probe_rng)), (rows.double().sum(1).float() + c.sum(1)).view(-1, 1))[1]
    lp = pc.log_prob_noisy(x, std, cond, num_draws=K, seed=seed)
    assert lp.shape == (B, 1) and torch.equal(lp[:, 0], _expected(x, std, cond, K, seed)[0]) and calls == [(B * K, (B * K, 2), None)]


def test_extensions_are_keyword_only_with_the_documented_defaults():
    KW = inspect.Parameter.KEYWORD_ONLY
    common = {"seed": None, "sample_offset": 0, "chunk_points": None, "return_ess": False, "num_probes": 1}
    table = {
        D.ScoreModel: (["self", "x", "noise_std", "conditional", "num_draws", "atol", "rtol", "method", "options"],
                       {"conditional": None, "num_draws": 16, "atol": 1e-4, "rtol": 1e-4, "method": "dopri5",
                        "options": {"min_step": 1e-6}}, common),
        F.ODEFlow: (["self", "x", "noise_std", "num_draws", "atol", "rtol", "method", "options"],
                    {"num_draws": 16, "atol": 1e-5, "rtol": 1e-5, "method": "dopri5", "options": None},
                    {"hutchinson": False, **common}),
        F.ConditionalODEFlow: (["self", "x", "noise_std", "conditional", "num_draws", "atol", "rtol", "method", "options"],
                               {"num_draws": 16, "atol": 1e-5, "rtol": 1e-5, "method": "dopri5", "options": None},
                               {"hutchinson": False, **common}),
        D.PopulationModelDiffusion: (["self", "x", "noise_std", "num_draws", "atol", "rtol"],
                                     {"num_draws": 16, "atol": 1e-5, "rtol": 1e-5}, common),
        D.PopulationModelDiffusionConditional: (["self", "x", "noise_std", "conditional", "num_draws", "atol", "rtol"],
                                                {"conditional": None, "num_draws": 16, "atol": 1e-5, "rtol": 1e-5}, common),
    }
    for cls, (positional, defaults, keyword) in table.items():
        prm = inspect.signature(cls.log_prob_noisy).parameters
        assert [n for n, p in prm.items() if p.kind is not KW] == positional, cls
        assert {n: p.default for n, p in prm.items() if p.kind is KW} == keyword, cls
        assert {n: prm[n].default for n in defaults} == defaults, cls
        # the solver defaults are those of the class's own log_prob
        own = inspect.signature(cls.log_prob).parameters
        assert all(own[n].default == prm[n].default for n in ("atol", "rtol", "method", "options") if n in prm), cls
        doc = cls.log_prob_noisy.__doc__
        assert doc and "noise" in doc
    for doc in (D.ScoreModel.log_prob_noisy.__doc__, F._FlowBase._log_prob_noisy.__doc__):
        assert "biased" in doc and "inside an exponent" in doc and "clean case" in doc
    from flowfusion_amd.symplectic import SymplecticFlowModel
    assert not hasattr(SymplecticFlowModel, "log_prob_noisy")
    from flowfusion_amd.distributed import log_prob_noisy_sharded
    prm = inspect.signature(log_prob_noisy_sharded).parameters
    assert [n for n, p in prm.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == ["model", "x", "noise_std", "conditional"]
    for name, default in (("local_x", None), ("local_noise_std", None), ("n_total", None), ("num_draws", 16), ("gather", True),
                          ("return_ess", False)):
        assert prm[name].kind is KW and prm[name].default == default, name


def test_every_value_error():
    x = torch.randn(5, 3)
    calls = []
    models = [(_stubbed(_score(), calls, True), ()), (_stubbed(F.ODEFlow(3, [16]), calls, False), ()),
              (_stubbed(F.ConditionalODEFlow(3, 2, [16]), calls, False), (torch.zeros(5, 2),)),
              (D.PopulationModelDiffusion(D.MLP(3, 0, 8, [16]), D.VPSDE()), ())]
    for m, args in models:
        fixed = {} if isinstance(m, D.PopulationModelDiffusion) else FIXED
        for bad in (-0.1, float("nan"), float("inf"), torch.tensor([0.1, -1e-9, 0.1]), torch.full((5, 3), float("nan")),
                    torch.tensor([[0.1, 0.2, float("inf")]]).expand(5, 3)):
            with pytest.raises(ValueError, match="finite and >= 0"):
                m.log_prob_noisy(x, bad, *args, **fixed)
        for shape in ((5,), (4, 3), (5, 3, 1), (1,)):
            with pytest.raises(ValueError, match="noise_std has shape"):
                m.log_prob_noisy(x, torch.ones(shape), *args, **fixed)
        for K in (0, -1, 4097):
            with pytest.raises(ValueError, match="num_draws"):
                m.log_prob_noisy(x, 0.1, *args, num_draws=K, **fixed)
        for xbad in (x.double(), x[0], x.view(5, 3, 1)):
            with pytest.raises(ValueError, match=r"\[batch, dim\] float32"):
                m.log_prob_noisy(xbad, 0.1, *args, **fixed)
        if fixed:
            for method in ("dopri5", "bosh3", "adaptive_heun"):
                with pytest.raises(ValueError, match="chunk_points") as e:
                    m.log_prob_noisy(x, 0.1, *args, method=method, chunk_points=2)
                assert "whole batch" in str(e.value) and "fixed-grid" in str(e.value)
            for chunk in (0, -3):
                with pytest.raises(ValueError, match="at least one data point"):
                    m.log_prob_noisy(x, 0.1, *args, chunk_points=chunk, **fixed)
    assert calls == []                                  # every refusal came before the model's log_prob


# ---- the sharded entry point over gloo ---------------------------------------------------------------------------------------
def _row_keyed(model, column):
    """``model`` with a ``log_prob`` whose value depends on each row's values, its conditional and -- for the probes of a
    Hutchinson solve -- the GLOBAL expanded row it is told."""
    def log_prob(rows, *args, probe="torch", seed=None, sample_offset=0, **kw):
        cond = args[0] if args else kw.pop("conditional", None)
        lp = rows.double().sum(1).float() + (0.0 if cond is None else cond.sum(1))
        if probe == "philox":
            g = torch.arange(rows.shape[0], dtype=torch.float64) + float(sample_offset)
            lp = lp + (0.37 * torch.sin(g + float(seed))).float()
        return lp.view(-1, 1) if column else lp
    model.log_prob = log_prob
    return model


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import log_prob_noisy_sharded, shard_bounds
        gathers = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, inp, **kw: (gathers.append(tuple(inp.shape)), real(out, inp, **kw))[1]
        torch.manual_seed(0)
        x, std, c = torch.randn(n, 3), torch.rand(n, 3), torch.randn(n, 2)
        lo, hi = shard_bounds(n, world, rank)
        K, seed = 5, 9
        ok = True
        for hutch in (False, True):
            m = _row_keyed(_score(hutchinson=hutch), True)
            want, want_ess = m.log_prob_noisy(x, std, c, num_draws=K, seed=seed, return_ess=True, **FIXED)
            del gathers[:]
            got = log_prob_noisy_sharded(m, x, std, c, seed=seed, num_draws=K, **FIXED)
            ok &= len(gathers) == 1 and got.shape == (n, 1) and torch.equal(got, want)
            got = log_prob_noisy_sharded(m, x, std, c, seed=seed, num_draws=K, return_ess=True, **FIXED)
            ok &= len(gathers) == 2 and gathers[1][1:] == (2,) and isinstance(got, tuple) and len(got) == 2
            ok &= got[0].shape == (n, 1) and got[1].shape == (n,) and torch.equal(got[0], want) and torch.equal(got[1], want_ess)
            mine = log_prob_noisy_sharded(m, local_x=x[lo:hi], local_noise_std=std[lo:hi], local_conditional=c[lo:hi], n_total=n,
                                          seed=seed, num_draws=K, return_ess=True, **FIXED)
            ok &= len(gathers) == 3 and torch.equal(mine[0], want) and torch.equal(mine[1], want_ess)
            (le, ls), span = log_prob_noisy_sharded(m, x, std, c, seed=seed, num_draws=K, gather=False, return_ess=True, **FIXED)
            ok &= span == (lo, hi) and torch.equal(le, want[lo:hi]) and torch.equal(ls, want_ess[lo:hi]) and len(gathers) == 3
            # a [D] noise_std is replicated, beside x and beside local_x
            want1 = m.log_prob_noisy(x, std[0], c, num_draws=K, seed=seed, **FIXED)
            ok &= torch.equal(log_prob_noisy_sharded(m, x, std[0], c, seed=seed, num_draws=K, **FIXED), want1)
            ok &= torch.equal(log_prob_noisy_sharded(m, None, std[0], local_x=x[lo:hi], local_conditional=c[lo:hi], n_total=n,
                                                     seed=seed, num_draws=K, **FIXED), want1)
            f = _row_keyed(F.ODEFlow(3, [16]), False)
            fk = dict(FIXED, hutchinson=hutch)
            wantf, wantf_ess = f.log_prob_noisy(x, std, num_draws=K, seed=seed, return_ess=True, **fk)
            gotf = log_prob_noisy_sharded(f, x, std, seed=seed, num_draws=K, return_ess=True, **fk)
            ok &= gotf[0].shape == (n,) and gotf[1].shape == (n,) and torch.equal(gotf[0], wantf) and torch.equal(gotf[1], wantf_ess)
            fc = _row_keyed(F.ConditionalODEFlow(3, 2, [16]), False)
            ok &= torch.equal(log_prob_noisy_sharded(fc, x, std, c, seed=seed, num_draws=K, **fk),
                              fc.log_prob_noisy(x, std, c, num_draws=K, seed=seed, **fk))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 37), (2, 64), (3, 37)])          # ragged, even, ragged over three
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


def test_sharded_argument_rules():
    from flowfusion_amd.distributed import log_prob_noisy_sharded
    m = _row_keyed(_score(), True)
    x, std = torch.randn(6, 3), torch.rand(6, 3)
    with pytest.raises(ValueError, match="noise_std"):
        log_prob_noisy_sharded(m, x, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std"):
        log_prob_noisy_sharded(m, x, std, local_noise_std=std, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std"):
        log_prob_noisy_sharded(m, x, local_noise_std=std, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std"):
        log_prob_noisy_sharded(m, None, std, local_x=x, n_total=6, seed=1, **FIXED)
    with pytest.raises(ValueError, match="local_noise_std must hold"):
        log_prob_noisy_sharded(m, local_x=x, local_noise_std=std[:5], n_total=6, seed=1, **FIXED)
    # one process: the plain call
    want = m.log_prob_noisy(x, std, num_draws=4, seed=3, **FIXED)
    assert torch.equal(log_prob_noisy_sharded(m, x, std, seed=3, num_draws=4, **FIXED), want)
    assert torch.equal(log_prob_noisy_sharded(m, local_x=x, local_noise_std=std, n_total=6, seed=3, num_draws=4, **FIXED), want)
