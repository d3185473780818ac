"""CPU tier: the two ends of the K-draw marginal log-density of the symplectic flows (csrc/ff_marginal.h through its host
entry points ff_marginal_expand_host / ff_marginal_reduce_host), and the argument rules of the public entry point.

Anchors: numpy's fp32 arithmetic and tests/_philox.py for what expand writes; a float64 numpy statement of the weights,
the log-sum-exp and the effective sample size for what reduce returns; and a closed form independent of both -- the
leapfrog of the rotation field v = [alpha p, -beta q] is a linear map M of unit determinant, so the marginal of q0 is the
Gaussian N(0, [(M^T M)^-1]_qq) and the K-draw estimate must close in on it as K grows."""
import ctypes
import math

import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
from tests._philox import normals

BASE = 0xFFFD0000
FILL_BAR = 2e-6             # device / libm normals against tests/_philox.py (tests/test_gpu_stream_kernels.py FILL_BAR)
KS = [1, 2, 5, 64, 65, 257]
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


def one_rounding_bar(ref):
    """|got - ref| <= 1.2e-7 |ref| + 1e-10: one fp32 rounding (2^-24 = 6e-8 relative) of a result computed in double."""
    return 1.2e-7 * np.abs(ref) + 1e-10


def reference_reduce(z1, p0, K, log_det=0.0):
    """(log p [B], ess [B]) in float64 numpy from z1 [B K, 2 D] and p0 [B K, D]; the semantics of torch.logsumexp for
    non-finite weights (the maximum replaced by 0 where it is not finite)."""
    z1, p0 = z1.astype(np.float64), p0.astype(np.float64)
    D = p0.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        lw = (-0.5 * ((z1 * z1).sum(1) - (p0 * p0).sum(1)) - D * HALF_LOG_2PI).reshape(-1, K)
        m = lw.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        w = np.exp(lw - m)
        with np.errstate(divide="ignore"):
            logp = np.log(w.sum(1)) + m[:, 0] - math.log(K) - log_det
            ess = w.sum(1) ** 2 / (w * w).sum(1)
    return logp, ess, lw


def host_expand(x, K, seed, offset, shift=None, scale=None, cond=None):
    z0, c = _native.marginal_expand(torch.from_numpy(x), K, seed, offset, None if shift is None else torch.from_numpy(shift),
                                    None if scale is None else torch.from_numpy(scale),
                                    None if cond is None else torch.from_numpy(cond))
    return z0.numpy(), None if c is None else c.numpy()


def host_reduce(z1, K, seed, offset, log_det=0.0, want_ess=True):
    z1 = torch.from_numpy(np.ascontiguousarray(z1, dtype=np.float32))
    ess = torch.empty(z1.shape[0] // K) if want_ess else None
    out = _native.marginal_reduce(z1, K, seed, offset, log_det, None, ess)
    return out.numpy().astype(np.float64), None if ess is None else ess.numpy().astype(np.float64)


# ---- expand ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2 ** 33 + 7])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 16, 17])
def test_host_expand_writes_q_bitwise_and_the_streams_momenta(D, offset):
    rng = np.random.default_rng(D)
    B, C, seed = 7, 3, 99 + D
    x = rng.standard_normal((B, D)).astype(np.float32) * 2
    shift = rng.standard_normal(D).astype(np.float32)
    scale = (rng.random(D) + 0.5).astype(np.float32)
    cond = rng.standard_normal((B, C)).astype(np.float32)
    for K in (1, 5):
        for sh, sc, cd in ((shift, scale, cond), (None, None, None), (shift, None, cond), (None, scale, None)):
            z0, co = host_expand(x, K, seed, offset, sh, sc, cd)
            assert z0.shape == (B * K, 2 * D) and z0.dtype == np.float32
            q = x
            if sh is not None:
                q = q - sh
            if sc is not None:
                q = q / sc
            assert q.dtype == np.float32
            assert np.array_equal(z0[:, :D].view(np.uint32), np.repeat(q, K, axis=0).view(np.uint32))
            ref = normals(seed, offset, B, D, [BASE + k for k in range(K)])            # [K, B, D]
            ref = ref.transpose(1, 0, 2).reshape(B * K, D).astype(np.float64)
            err = np.abs(z0[:, D:].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            assert np.isfinite(z0).all() and err.max() <= FILL_BAR, (D, K, err.max())
            if cd is None:
                assert co is None
            else:
                assert np.array_equal(co.view(np.uint32), np.repeat(cd, K, axis=0).view(np.uint32))


def test_host_expand_momenta_differ_by_draw_row_and_seed():
    x = np.zeros((4, 8), dtype=np.float32)
    a, _ = host_expand(x, 3, 5, 0)
    p = a[:, 8:].reshape(4, 3, 8)
    assert len({p[r, k].tobytes() for r in range(4) for k in range(3)}) == 12
    b, _ = host_expand(x, 3, 6, 0)
    assert not np.array_equal(a, b)
    c, _ = host_expand(x[:2], 3, 5, 2)                                   # rows 2, 3 of the stream
    assert np.array_equal(c, a[6:])


# ---- reduce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", [1, 3, 16, 17])
def test_host_reduce_against_float64(D, K):
    rng = np.random.default_rng(1000 * D + K)
    B, seed, offset = 5, 31, 2 ** 32 + 11
    z0, _ = host_expand(np.zeros((B, D), dtype=np.float32), K, seed, offset)
    p0 = z0[:, D:]
    z1 = (rng.standard_normal((B * K, 2 * D)) * 1.2).astype(np.float32)
    log_det = 0.37
    want, want_ess, _ = reference_reduce(z1, p0, K, log_det)
    got, ess = host_reduce(z1, K, seed, offset, log_det)
    assert (np.abs(got - want) <= one_rounding_bar(want)).all(), (got, want)
    assert (np.abs(ess - want_ess) <= one_rounding_bar(want_ess)).all(), (ess, want_ess)
    assert ((ess > 0) & (ess <= K * (1 + 1e-6))).all()
    only, none = host_reduce(z1, K, seed, offset, log_det, want_ess=False)
    assert none is None and np.array_equal(only, got)
    if K == 1:                                                       # one draw: the reference's expression, ess = 1
        assert (ess == 1.0).all()


@pytest.mark.parametrize("K", KS)
def test_host_reduce_non_finite_rows_follow_logsumexp(K):
    D, B, seed = 3, 4, 8
    rng = np.random.default_rng(K)
    z0, _ = host_expand(np.zeros((B, D), dtype=np.float32), K, seed, 0)
    p0 = z0[:, D:]
    z1 = rng.standard_normal((B * K, 2 * D)).astype(np.float32)
    z1[0 * K + (K - 1), 2] = np.inf                     # point 0: one draw of weight zero (the last one)
    z1[1 * K:2 * K, 0] = -np.inf                        # point 1: every draw of weight zero
    z1[2 * K + K // 2, 4] = np.nan                      # point 2: a NaN
    want, want_ess, lw = reference_reduce(z1, p0, K)
    assert lw[0, K - 1] == -np.inf and (lw[1] == -np.inf).all() and np.isnan(lw[2]).any()
    got, ess = host_reduce(z1, K, seed, 0)
    assert np.isnan(got[2]) and np.isnan(ess[2])
    assert got[1] == -np.inf and np.isnan(ess[1])
    assert abs(got[3] - want[3]) <= one_rounding_bar(want[3]) and abs(ess[3] - want_ess[3]) <= one_rounding_bar(want_ess[3])
    if K == 1:
        assert got[0] == -np.inf
    else:
        assert np.isfinite(got[0]) and abs(got[0] - want[0]) <= one_rounding_bar(want[0])
        assert abs(ess[0] - want_ess[0]) <= one_rounding_bar(want_ess[0])


# ---- closed form -----------------------------------------------------------------------------------------------------------
ALPHA, BETA, STEPS = 1.0, 0.6, 4


def rotation_leapfrog_matrix(alpha=ALPHA, beta=BETA, n=STEPS):
    """Per dimension, on (q, p): M = (K1 Dr K1)^n, K1 = [[1, 0], [-h beta / 2, 1]], Dr = [[1, h alpha], [0, 1]], h = 1 / n."""
    h = 1.0 / n
    K1 = np.array([[1.0, 0.0], [-0.5 * h * beta, 1.0]])
    Dr = np.array([[1.0, h * alpha], [0.0, 1.0]])
    return np.linalg.matrix_power(K1 @ Dr @ K1, n)


def exact_marginal(q0, M):
    """log N(q0; 0, s2 I) summed over the dimensions, s2 = [(M^T M)^-1]_qq (det M = 1: the joint density of (q0, p0) is
    N(M [q0; p0]), a Gaussian of precision M^T M)."""
    s2 = np.linalg.inv(M.T @ M)[0, 0]
    return (-0.5 * q0 ** 2 / s2 - 0.5 * math.log(2 * math.pi * s2)).sum(1)


def closed_form_inputs():
    B, D = 256, 3
    return B, D, 7, (1.3 * np.random.default_rng(0).standard_normal((B, D))).astype(np.float32)


def test_closed_form_rotation_marginal():
    """RMS error against the exact marginal: K = 64 at most a quarter of K = 1 (the float64 statement of the same draws
    gives 0.070 and 0.742 nats, a ratio of 0.095); the mean effective sample size at K = 64 in (32, 64] (float64: 50)."""
    B, D, seed, x = closed_form_inputs()
    M = rotation_leapfrog_matrix()
    assert abs(np.linalg.det(M) - 1.0) < 1e-12
    exact = exact_marginal(x.astype(np.float64), M)
    rms, ess64 = {}, None
    for K in (1, 64):
        z0, _ = host_expand(x, K, seed, 0)
        q, p = z0[:, :D].astype(np.float64), z0[:, D:].astype(np.float64)
        z1 = np.concatenate([M[0, 0] * q + M[0, 1] * p, M[1, 0] * q + M[1, 1] * p], axis=1)
        got, ess = host_reduce(z1, K, seed, 0)
        rms[K] = float(np.sqrt(np.mean((got - exact) ** 2)))
        if K == 64:
            ess64 = ess
    print(f"rotation marginal: rms error K=1 {rms[1]:.4f}, K=64 {rms[64]:.4f} nats; mean ess {ess64.mean():.2f}, min {ess64.min():.2f}")
    assert rms[64] <= 0.25 * rms[1], rms
    assert 32.0 < ess64.mean() <= 64.0 and ((ess64 > 1.0) & (ess64 <= 64.0 * (1 + 1e-6))).all(), (ess64.mean(), ess64.min())


# ---- arguments -------------------------------------------------------------------------------------------------------------
def _cpu_model():
    torch.manual_seed(3)
    D = 3
    return SymplecticFlowModel(SymplecticMLP(D, 0, 4, [16]), torch.zeros(D), torch.ones(D), None, None), torch.randn(5, D)


def test_log_prob_marginal_argument_rules():
    fm, x = _cpu_model()
    for K in (0, -1, 4097):
        with pytest.raises(ValueError, match="num_momenta"):
            fm.log_prob_marginal(x, num_momenta=K)
    for method in ("dopri5", "bosh3"):
        with pytest.raises(ValueError, match="leapfrog") as e:
            fm.log_prob_marginal(x, num_momenta=4, method=method, chunk_points=2)
        assert "whole batch" in str(e.value)
    with pytest.raises(ValueError, match="chunk_points"):
        fm.log_prob_marginal(x, num_momenta=4, method="leapfrog", num_steps=4, chunk_points=0)
    with pytest.raises(ValueError, match="num_steps >= 1"):
        fm.log_prob_marginal(x, num_momenta=4, method="leapfrog")
    with pytest.raises(ValueError, match="num_steps >= 1"):
        fm.log_prob_marginal(x, num_momenta=4, method="leapfrog", num_steps=0)
    with pytest.raises(ValueError, match="num_steps belongs to"):
        fm.log_prob_marginal(x, num_momenta=4, num_steps=4)
    with pytest.raises(ValueError, match="method='verlet'"):
        fm.log_prob_marginal(x, num_momenta=4, method="verlet")
    # the one-draw entry point keeps its rules (the check is shared)
    with pytest.raises(ValueError, match="num_steps belongs to"):
        fm._log_prob_from(x, torch.randn_like(x), num_steps=4)
    for K in (0, 4097):
        with pytest.raises(ValueError, match="num_momenta"):
            _native.marginal_expand(x, K, 1)
        with pytest.raises(ValueError, match="num_momenta"):
            _native.marginal_reduce(torch.zeros(4, 6), K, 1)


def test_c_entry_points_refuse_bad_arguments_and_are_exported():
    L = _native.lib()
    for name in ("ff_marginal_expand", "ff_marginal_reduce", "ff_marginal_expand_host", "ff_marginal_reduce_host"):
        assert hasattr(L, name), name
    B, D, C, K = 2, 3, 2, 4
    x, cond = torch.zeros(B, D), torch.zeros(B, C)
    z, co = torch.full((B * K + 1, 2 * D), 7.0), torch.full((B * K + 1, C), 7.0)
    out, ess = torch.full((B + 1,), 7.0), torch.full((B + 1,), 7.0)
    P = lambda t: t.data_ptr()
    bad, ok = _native.FF_ERR_BADARG, _native.FF_OK
    null = None
    # (the device entry points check their arguments before anything touches a GPU)
    for fn, tail in ((L.ff_marginal_expand_host, ()), (L.ff_marginal_expand, (null,))):
        assert fn(null, null, null, null, B, D, 0, K, 1, 0, P(z), null, *tail) == bad             # x
        assert fn(P(x), null, null, null, B, D, 0, K, 1, 0, null, null, *tail) == bad             # z0
        assert fn(P(x), null, null, null, -1, D, 0, K, 1, 0, P(z), null, *tail) == bad            # B
        assert fn(P(x), null, null, null, B, 0, 0, K, 1, 0, P(z), null, *tail) == bad             # D
        assert fn(P(x), null, null, null, B, D, 0, 0, 1, 0, P(z), null, *tail) == bad             # K
        assert fn(P(x), null, null, null, B, D, 0, 4097, 1, 0, P(z), null, *tail) == bad
        assert fn(P(x), null, null, P(cond), B, D, C, K, 1, 0, P(z), null, *tail) == bad          # cond without cond_out
        assert fn(P(x), null, null, P(cond), B, D, 0, K, 1, 0, P(z), P(co), *tail) == bad         # cond with C = 0
        assert fn(P(x), null, null, null, 0, D, 0, K, 1, 0, P(z), null, *tail) == ok              # B = 0: nothing to do
    for fn, tail in ((L.ff_marginal_reduce_host, ()), (L.ff_marginal_reduce, (null,))):
        assert fn(null, B, D, K, 1, 0, 0.0, P(out), null, *tail) == bad                           # z1
        assert fn(P(z), B, D, K, 1, 0, 0.0, null, null, *tail) == bad                             # out_logp
        assert fn(P(z), -1, D, K, 1, 0, 0.0, P(out), null, *tail) == bad
        assert fn(P(z), B, 0, K, 1, 0, 0.0, P(out), null, *tail) == bad
        assert fn(P(z), B, D, 0, 1, 0, 0.0, P(out), null, *tail) == bad
        assert fn(P(z), B, D, 4097, 1, 0, 0.0, P(out), null, *tail) == bad
        assert fn(P(z), 0, D, K, 1, 0, 0.0, P(out), P(ess), *tail) == ok
    assert (z == 7.0).all() and (co == 7.0).all() and (out == 7.0).all() and (ess == 7.0).all()
    # the host twins write exactly their outputs
    assert L.ff_marginal_expand_host(P(x), null, null, P(cond), B, D, C, K, 1, 0, P(z), P(co)) == ok
    assert (z[B * K] == 7.0).all() and (co[B * K] == 7.0).all() and (z[:B * K, :D] == 0).all() and (co[:B * K] == 0).all()
    assert L.ff_marginal_reduce_host(P(z), B, D, K, 1, 0, 0.0, P(out), P(ess)) == ok
    assert out[B] == 7.0 and ess[B] == 7.0 and torch.isfinite(out[:B]).all()
    assert _native.MOMENTUM_NOISE_BASE == BASE and _native.MOMENTUM_NOISE_BASE + _native.MAX_MOMENTA <= _native.TRACE_PROBE_NOISE_BASE
