"""CPU tier of ``SymplecticFlowModel.posterior_marginal_noisy`` (csrc/ff_marginal_posterior.hip: ff_marginal_observe_resample)
through its host twin: the twin against the float64 restatement of tests/_marginal_posterior_ref.py, against ff_observe_expand's
rows and, on weights that fp32 holds, against ff_weighted_resample_host bit for bit; degenerate points; every FF_ERR_BADARG; the
front end's refusals in their order; and the front end itself around a stand-in for the solve (the library integrates on the GPU
only: ``P.stand_in_solve``, an elementwise map, takes ``_solve_forward``'s place) -- ``log_prob`` and ``ess`` bitwise the value
method's, invariance to chunks, slices and the layout of sigma.  Two damaged restatements must miss the bar on ``mean`` a
hundredfold; the draws must come at the frequencies of their weights; the K-draw mean must close in on the closed-form
posterior of the rotation field; and both sharded entry points must equal the unsharded call over two gloo ranks."""
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
from flowfusion_amd import symplectic as S
from tests import _marginal_observe_ref as O
from tests import _marginal_posterior_ref as P
from tests._pushforward_ref import normalised_error
from tests.test_gpu_pushforward import FACTOR
from tests.test_observe_host import _free_port
from tests.test_symplectic_marginal_host import ALPHA, BETA, STEPS, rotation_leapfrog_matrix

ROOT = Path(__file__).resolve().parents[1]
OK, BAD = _native.FF_OK, _native.FF_ERR_BADARG
CPU = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the host twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.KS)
def test_twin_against_the_restatement_the_expansion_and_weighted_resample(K):
    for D in P.DS:
        P.check_cell(CPU, 3, D, K, 5)
    for B, M in ((1, 1), (17, 4), (17, 8)):
        P.check_cell(CPU, B, 4, K, M)


def test_twin_in_every_layout_of_sigma_and_one_float_off_alignment():
    for layout in ("BD", "D", "scalar"):
        P.check_cell(CPU, 3, 16, 16, 5, layout)
        P.check_cell(CPU, 3, 16, 100, 4, layout, offset=1)
    # a [D] vector is the [B, D] tensor of its copies, bit for bit
    x, std, lw = P.kernel_inputs(5, 4, 4, "D")
    a = P.run_kernel(CPU, x, std, lw, 4, 3)
    b = P.run_kernel(CPU, x, std[None, :].expand(5, 4).contiguous(), lw, 4, 3)
    assert all(torch.equal(P.bits(p), P.bits(q)) for p, q in zip(a, b))


def test_twin_depends_on_the_global_row_and_the_seed_only():
    B, D, K, M = 9, 5, 4, 6
    x, std, lw = P.kernel_inputs(B, D, K)
    whole = P.run_kernel(CPU, x, std, lw, K, M, first=100)
    part = P.run_kernel(CPU, x[3:7], std[3:7], lw[3 * K:7 * K], K, M, first=103)
    assert all(torch.equal(P.bits(a[3:7]), P.bits(b)) for a, b in zip(whole, part))
    assert not torch.equal(P.run_kernel(CPU, x, std, lw, K, M, seed=P.SEED + 1, first=100)[0], whole[0])
    assert torch.equal(P.run_kernel(CPU, x, std, lw, K, 3, first=100)[1], whole[1][:, :3])


def test_outputs_left_out_are_left_out_and_the_others_keep_their_bits():
    B, D, K, M = 5, 4, 16, 5
    x, std, lw = P.kernel_inputs(B, D, K)
    full = P.run_kernel(CPU, x, std, lw, K, M)
    for want in ((True, False, False, False), (False, True, False, False), (False, False, True, False),
                 (False, False, False, True), (True, True, False, False), (False, False, True, True)):
        got = P.run_kernel(CPU, x, std, lw, K, M, want=want)
        for g, f, w in zip(got, full, want):
            assert (g is None) == (not w) and (g is None or torch.equal(P.bits(g), P.bits(f)))
    s, i, mu, v = P.run_kernel(CPU, x, std, lw, K, 0)                                    # M = 0: the moments alone
    assert s.shape == (B, 0, D) and i.shape == (B, 0)
    assert torch.equal(P.bits(mu), P.bits(full[2])) and torch.equal(P.bits(v), P.bits(full[3]))


@pytest.mark.parametrize("K", [1, 4, 100])
def test_degenerate_points_and_one_draw(K):
    B, D, M = 6, 5, 4
    x, std, lw = P.kernel_inputs(B, D, K)
    lw = torch.where(torch.isinf(lw), torch.full_like(lw, -45.0), lw)
    clean = P.run_kernel(CPU, x, std, lw, K, M)
    lw = lw.clone()
    lw[1 * K:2 * K] = -float("inf")                      # point 1: no draw above -inf
    lw[2 * K + K // 2] = float("nan")                    # point 2: a NaN
    lw[4 * K + K - 1] = -float("inf")                    # point 4: its last draw of weight zero (K = 1: its only one)
    s, i, mu, v = P.run_kernel(CPU, x, std, lw, K, M)
    dead = [1, 2] + ([4] if K == 1 else [])
    for r in dead:
        assert bool((i[r] == -1).all() and torch.isnan(s[r]).all() and torch.isnan(mu[r]).all() and torch.isnan(v[r]).all())
    for r in (0, 3, 5):                                  # their neighbours are untouched
        assert all(torch.equal(P.bits(a[r]), P.bits(b[r])) for a, b in zip((s, i, mu, v), clean))
    if K > 1:
        assert bool((i[4] >= 0).all() and (i[4] != K - 1).all() and torch.isfinite(s[4]).all() and (v[4] >= 0).all())
    if K == 1:
        y, _ = _native.observe_expand(x, std, 1, P.SEED, P.OFFSET)
        for r in (0, 3, 5):
            assert bool((i[r] == 0).all() and (v[r] == 0).all())
            assert torch.equal(P.bits(mu[r]), P.bits(y[r])) and torch.equal(P.bits(s[r]), P.bits(y[r].expand(M, D)))


def test_noise_std_zero_gives_x_back():
    B, D, K, M = 5, 7, 16, 3
    x, _, lw = P.kernel_inputs(B, D, K)
    x = 50.0 * x
    s, i, mu, v = P.run_kernel(CPU, x, 0.0, lw, K, M)
    assert torch.equal(P.bits(s), P.bits(x[:, None, :].expand(B, M, D).contiguous())) and torch.equal(mu, x)
    assert bool((v >= 0).all() and (v.double() <= 1e-24 * torch.clamp(x.double() ** 2, min=1.0)).all())


# ---- the C entry points and the binding -----------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_their_signatures_and_refuse_bad_arguments():
    Lb = _native.lib()
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    args = ("const float* x, const float* noise_std, int32_t std_row_stride, const double* lw, int64_t B, int32_t D, int32_t K, "
            "int32_t M, uint64_t seed, int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var")
    for proto in (f"int ff_marginal_observe_resample({args}, void* hip_stream);", f"int ff_marginal_observe_resample_host({args});"):
        assert proto in header, proto
    assert hasattr(Lb, "ff_marginal_observe_resample") and hasattr(Lb, "ff_marginal_observe_resample_host")
    B, D, K, M = 2, 3, 4, 2
    x, std, lw = torch.ones(B, D), torch.zeros(B, D), torch.zeros(B * K, dtype=torch.float64)
    s, idx = torch.full((B * M + 1, D), 7.0), torch.full((B * M + 1,), 7, dtype=torch.int32)
    mu, var = torch.full((B + 1, D), 7.0), torch.full((B + 1, D), 7.0)
    p = lambda t: t.data_ptr()
    base = [("x", p(x)), ("std", p(std)), ("stride", D), ("lw", p(lw)), ("B", B), ("D", D), ("K", K), ("M", M), ("seed", 1),
            ("off", 0), ("s", p(s)), ("i", p(idx)), ("mu", p(mu)), ("var", p(var))]
    # (the device entry point checks its arguments before anything touches a GPU)
    for fn in (lambda **kw: Lb.ff_marginal_observe_resample_host(*[kw.get(n, v) for n, v in base]),
               lambda **kw: Lb.ff_marginal_observe_resample(*[kw.get(n, v) for n, v in base], None)):
        for bad in (dict(x=0), dict(std=0), dict(lw=0), dict(B=-1), dict(D=0), dict(D=-1), dict(K=0), dict(K=-1), dict(K=4097),
                    dict(M=-1), dict(M=_native.MAX_OBS_SAMPLES + 1), dict(stride=1), dict(stride=D + 1), dict(stride=-D),
                    dict(s=0, i=0, mu=0, var=0)):
            assert fn(**bad) == BAD, bad
        assert fn(B=0) == OK and fn(B=0, M=0) == OK                                      # B == 0: no launch
    assert bool((s == 7.0).all() and (idx == 7).all() and (mu == 7.0).all() and (var == 7.0).all())
    host = lambda **kw: Lb.ff_marginal_observe_resample_host(*[kw.get(n, v) for n, v in base])
    assert host(M=0, var=0) == OK                                                        # M = 0 ignores samples and index
    assert bool((s == 7.0).all() and (idx == 7).all() and (mu[:B] == 1.0).all() and (mu[B] == 7.0).all() and (var == 7.0).all())
    assert host(stride=0) == OK
    assert bool((s[:B * M] == 1.0).all() and (s[B * M] == 7.0).all() and (idx[:B * M] >= 0).all() and (idx[:B * M] < K).all())
    assert bool(idx[B * M] == 7 and (var[:B] == 0.0).all() and (var[B] == 7.0).all())
    assert host(s=0, mu=0, var=0) == OK and host(K=4096, B=0) == OK


def test_binding_argument_rules():
    prm = inspect.signature(_native.marginal_observe_resample).parameters
    assert list(prm)[:7] == ["x", "noise_std", "lw", "num_draws", "num_samples", "seed", "sample_offset"]
    assert prm["sample_offset"].default == 0
    x, std, lw = torch.zeros(2, 3), torch.zeros(3), torch.zeros(8, dtype=torch.float64)
    for K in (0, 4097):
        with pytest.raises(ValueError, match="num_draws"):
            _native.marginal_observe_resample(x, std, lw, K, 1, 1)
    for M in (-1, 4097):
        with pytest.raises(ValueError, match="num_samples"):
            _native.marginal_observe_resample(x, std, lw, 4, M, 1)
    with pytest.raises(RuntimeError, match="x has shape"):
        _native.marginal_observe_resample(x[0], std, lw, 4, 1, 1)
    with pytest.raises(RuntimeError, match="noise_std has shape"):
        _native.marginal_observe_resample(x, torch.zeros(2), lw, 4, 1, 1)
    for bad in (lw.float(), lw[:7], lw.view(2, 4)):
        with pytest.raises(RuntimeError, match="lw must be a contiguous float64"):
            _native.marginal_observe_resample(x, std, bad, 4, 1, 1)
    with pytest.raises(RuntimeError, match="contiguous float32"):
        _native.marginal_observe_resample(x.double(), std, lw, 4, 1, 1)
    with pytest.raises(RuntimeError, match="mean has"):
        _native.marginal_observe_resample(x, std, lw, 4, 1, 1, mean=torch.zeros(3))
    s, i, mu, v = _native.marginal_observe_resample(x, std, lw, 4, 0, 1)
    assert s.shape == (2, 0, 3) and i.shape == (2, 0) and i.dtype == torch.int32 and torch.equal(mu, x) and torch.equal(v, x)
    s, i, mu, v = _native.marginal_observe_resample(x[:0], std, lw[:0], 4, 2, 1)
    assert s.shape == (0, 2, 3) and i.shape == (0, 2) and mu.shape == (0, 3) and v.shape == (0, 3)
    # the binding gives the bits of the raw call
    xk, sk, lk = P.kernel_inputs(5, 4, 16)
    raw = P.run_kernel(CPU, xk, sk, lk, 16, 5)
    assert all(torch.equal(P.bits(a), P.bits(b)) for a, b in zip(raw, _native.marginal_observe_resample(xk, sk, lk, 16, 5, P.SEED, P.OFFSET)))


# ---- the method: signature, refusals and their order ------------------------------------------------------------------------------------
def test_the_method_has_the_signature_of_the_issue_and_the_old_name_stays_absent():
    sig = inspect.signature(S.SymplecticFlowModel.posterior_marginal_noisy)
    names = list(sig.parameters)
    assert names == ["self", "x", "noise_std", "conditional", "num_draws", "num_samples", "atol", "rtol", "method", "num_steps",
                     "options", "seed", "sample_offset", "chunk_points"]
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == names[8:]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert [d[n] for n in names[3:]] == [None, 16, 1, 1e-5, 1e-5, "dopri5", None, None, None, 0, None]
    # log_prob_marginal_noisy's parameters with num_samples after num_draws and without return_ess
    value = [n for n in inspect.signature(S.SymplecticFlowModel.log_prob_marginal_noisy).parameters if n != "return_ess"]
    value.insert(value.index("num_draws") + 1, "num_samples")
    assert names == value
    assert not hasattr(S.SymplecticFlowModel, "posterior_noisy")
    flat = " ".join(S.SymplecticFlowModel.posterior_marginal_noisy.__doc__.split())
    assert "effective sample size" in flat and "raise ``num_draws``, not ``num_samples``" in flat
    assert "before trusting ``samples``" in flat and "pseudo-marginal" in flat and "ONE-MOMENTUM" in flat
    from flowfusion_amd import distributed as Ds
    a = inspect.signature(Ds.symplectic_log_prob_marginal_noisy_sharded).parameters
    b = inspect.signature(Ds.symplectic_posterior_marginal_noisy_sharded).parameters
    want = [n for n in a if n != "return_ess"]
    want.insert(want.index("num_draws") + 1, "num_samples")
    assert list(b) == want and all(b[n].default == a[n].default and b[n].kind == a[n].kind for n in want if n != "num_samples")
    for n in ("x", "noise_std", "conditional", "local_x", "local_noise_std", "n_total", "local_conditional", "seed", "num_draws",
              "gather", "global_control", "return_ess", "method", "num_steps", "atol", "rtol"):
        assert n in a, n


DEVICE_CALLS = [(_native, "marginal_observe_expand"), (_native, "marginal_weigh"), (_native, "marginal_observe_resample"),
                (_native, "marginal_reduce"), (odeint, "solve_leapfrog"), (odeint, "solve")]


class Touched(Exception):
    pass


def _no_device(monkeypatch):
    def touched(*a, **kw):
        raise Touched
    for mod, name in DEVICE_CALLS:
        monkeypatch.setattr(mod, name, touched)


def test_every_refusal_comes_in_its_order_before_the_device_is_touched(monkeypatch):
    _no_device(monkeypatch)
    front, x, std, cond, _ = P.front_case(P.FRONT_CASES[0])
    call = lambda *a, x=x, std=std, cond=cond, **kw: front.posterior_marginal_noisy(x, std, cond, *a, **kw)
    nan_std = torch.full_like(std, float("nan"))
    # 1. num_draws, then num_samples, then chunk_points -- each ahead of everything behind it
    for K in (0, -3, _native.MAX_MOMENTA + 1):
        with pytest.raises(ValueError, match=f"num_draws={K}: 1 .. {_native.MAX_MOMENTA} joint"):
            call(K, -1, method="nonsense", chunk_points=0)
    for M in (-1, 4097):
        with pytest.raises(ValueError, match=f"num_samples={M}: 0 .. 4096 posterior draws"):
            call(4, M, method="nonsense", chunk_points=0)
    with pytest.raises(ValueError, match="at least one data point per chunk"):
        call(4, 2, method="nonsense", chunk_points=0)
    # 2. the method and num_steps
    with pytest.raises(ValueError, match="method='nonsense': log_prob takes 'dopri5'"):
        call(4, 2, method="nonsense", x=x.double())
    with pytest.raises(ValueError, match="num_steps belongs to method='leapfrog'"):
        call(4, 2, num_steps=3, x=x.double())
    for n in (None, 0):
        with pytest.raises(ValueError, match="method='leapfrog' needs num_steps >= 1"):
            call(4, 2, method="leapfrog", num_steps=n, x=x.double())
    # 3. x, 4. noise_std
    for bad in (x[0], x.double(), x.numpy()):
        with pytest.raises(ValueError, match=r"posterior_marginal_noisy: x must be a \[batch, dim\] float32 tensor"):
            call(4, 2, x=bad, std=nan_std)
    with pytest.raises(ValueError, match=r"noise_std has shape \(9, 3\)"):
        call(4, 2, std=std[:, :3])
    for bad in (nan_std, -std, float("inf"), -1.0):
        with pytest.raises(ValueError, match="noise_std must be finite and >= 0 everywhere"):
            call(4, 2, std=bad, chunk_points=3)
    # an adaptive method solves all B K rows at once: chunk_points raises as it does for the value
    with pytest.raises(ValueError, match=r"chunk_points with method='dopri5'.*all B \* num_draws rows.*method='leapfrog' with num_steps"):
        call(4, 2, chunk_points=3)
    # ... and a call that nothing refuses gets as far as the first device call -- in every layout of noise_std
    for s in (std, std[0].clone(), 0.25, torch.tensor(0.25)):
        with pytest.raises(Touched):
            call(4, 0, std=s)
        with pytest.raises(Touched):
            call(4, 4096, std=s, method="leapfrog", num_steps=2, chunk_points=3)


# ---- the method around a stand-in for the solve -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.FRONT_CASES, ids=O.L.front_id)
def test_front_end_keeps_what_the_value_method_drops(case, monkeypatch):
    monkeypatch.setattr(S.SymplecticFlowModel, "_solve_forward", P.stand_in_solve)
    front, x, std, cond, steps = P.front_case(case)
    B, D = x.shape
    K, M, seed, first = 4, 5, 77, 2 ** 33 + 5
    kw = dict(method="leapfrog", num_steps=steps, seed=seed, sample_offset=first)
    post = front.posterior_marginal_noisy(x, std, cond, K, M, **kw)
    assert type(post) is odeint.NoisyPosterior and post._fields == P.FIELDS
    assert post.samples.shape == (B, M, D) and post.index.shape == (B, M) and post.index.dtype == torch.int32
    assert post.mean.shape == (B, D) and post.var.shape == (B, D) and post.ess.shape == (B,) and post.log_prob.shape == (B,)
    lp, ess = front.log_prob_marginal_noisy(x, std, cond, K, return_ess=True, **kw)
    assert torch.equal(P.bits(post.log_prob), P.bits(lp)) and torch.equal(P.bits(post.ess), P.bits(ess))
    y, _ = _native.observe_expand(x, std, K, seed, first)
    rows = (torch.arange(B)[:, None] * K + post.index.long()).reshape(-1)
    assert bool((post.index >= 0).all() and (post.index < K).all() and (post.var >= 0).all())
    assert torch.equal(P.bits(post.samples.reshape(B * M, D)), P.bits(y[rows]))
    # the float64 restatement on the weights of the route: the lw of ff_marginal_weigh on the same rows
    z0, ck = _native.marginal_observe_expand(x, std, K, seed, first, front.shift, front.scale, front._norm_cond(cond))
    _, lw, _ = _native.marginal_weigh(P.stand_in_solve(front, z0, ck, None, None, None, None, None), K, seed, first)
    z, _ = O.draws(B, D, K, CPU, seed, first)
    ref = P.restate(x, std, lw, z, K, M, seed, first)
    assert not ref.near.any() and np.array_equal(post.index.numpy(), ref.index)
    fl = P.floors(x, std, lw, z, K)
    assert normalised_error(post.mean, torch.from_numpy(ref.mean)) <= FACTOR * fl["mean"]
    assert normalised_error(post.var, torch.from_numpy(ref.var)) <= FACTOR * fl["var"]
    # chunks, slices with sample_offset moved, and the layout of sigma: the same bits
    for chunk in (1, 4, B):
        assert P.same(front.posterior_marginal_noisy(x, std, cond, K, M, chunk_points=chunk, **kw), post)
    lo, hi = 2, B - 1
    part = front.posterior_marginal_noisy(x[lo:hi], std[lo:hi], None if cond is None else cond[lo:hi], K, M,
                                          **dict(kw, sample_offset=first + lo))
    assert P.same(part, P.rows_of(post, lo, hi))
    flat = front.posterior_marginal_noisy(x, std[0].clone(), cond, K, M, **kw)
    assert P.same(flat, front.posterior_marginal_noisy(x, std[0][None, :].expand(B, D).contiguous(), cond, K, M, chunk_points=2, **kw))
    assert P.same(front.posterior_marginal_noisy(x, 0.25, cond, K, M, **kw),
                  front.posterior_marginal_noisy(x, torch.full((B, D), 0.25), cond, K, M, **kw))
    assert not torch.equal(front.posterior_marginal_noisy(x, std, cond, K, 64, **dict(kw, seed=seed + 1)).index,
                           front.posterior_marginal_noisy(x, std, cond, K, 64, **kw).index)
    # num_samples = 0: the moments alone; the default: one sample; no rows: empty fields
    p0 = front.posterior_marginal_noisy(x, std, cond, K, 0, **kw)
    assert p0.samples.shape == (B, 0, D) and p0.index.shape == (B, 0) and torch.equal(P.bits(p0.mean), P.bits(post.mean))
    assert front.posterior_marginal_noisy(x, std, cond, K, **kw).samples.shape == (B, 1, D)
    e0 = front.posterior_marginal_noisy(x[:0], std[:0], None if cond is None else cond[:0], K, M, **kw)
    assert e0.samples.shape == (0, M, D) and e0.index.shape == (0, M) and e0.mean.shape == (0, D) and e0.ess.shape == (0,)
    # noise_std = 0: every sample is x, var = 0, log_prob bitwise log_prob_marginal
    pz = front.posterior_marginal_noisy(x, 0.0, cond, K, M, **kw)
    assert torch.equal(P.bits(pz.samples), P.bits(x[:, None, :].expand(B, M, D).contiguous())) and torch.equal(pz.mean, x)
    assert bool((pz.var.double() <= 1e-24 * torch.clamp(x.double() ** 2, min=1.0)).all())
    assert torch.equal(P.bits(pz.log_prob), P.bits(front.log_prob_marginal(x, cond, K, **kw)))
    # seed=None: one draw of torch's generator, as the value method draws it
    torch.manual_seed(5)
    a = front.posterior_marginal_noisy(x, std, cond, K, M, method="leapfrog", num_steps=steps)
    torch.manual_seed(5)
    s = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert P.same(a, front.posterior_marginal_noisy(x, std, cond, K, M, method="leapfrog", num_steps=steps, seed=s))


def test_an_adaptive_method_hands_all_rows_to_one_solve_and_the_default_chunk_follows_the_row_budget(monkeypatch):
    calls = []

    def solve(self, z0, c, atol, rtol, method, options, num_steps):
        calls.append((int(z0.shape[0]), method, atol, rtol))
        return P.stand_in_solve(self, z0, c, atol, rtol, method, options, num_steps)
    monkeypatch.setattr(S.SymplecticFlowModel, "_solve_forward", solve)
    front, x, std, cond, steps = P.front_case(P.FRONT_CASES[0])
    B, K = x.shape[0], 4
    a = front.posterior_marginal_noisy(x, std, cond, K, 2, 1e-4, 1e-3, seed=3)
    assert calls == [(B * K, "dopri5", 1e-4, 1e-3)]
    del calls[:]
    monkeypatch.setattr(S.SymplecticFlowModel, "MARGINAL_CHUNK_ROWS", 4 * K + 3)
    b = front.posterior_marginal_noisy(x, std, cond, K, 2, method="leapfrog", num_steps=steps, seed=3)
    assert [c[0] for c in calls] == [4 * K, 4 * K, K] and P.same(a, b)                   # (the stand-in ignores the method)


# ---- the inputs: conditions that hold with or without the feature --------------------------------------------------------------------
GPU_CELLS = [(B, D, K, M) for K in P.KS for D in P.DS for B, M in ((1, 0), (3, 1), (17, 4), (3, 5), (17, 8))] + \
            [(3, 16, 16, 5), (17, 16, 100, 4), (3, 4, 64, 8)]


def test_the_shapes_are_the_ones_the_issue_names():
    assert P.BS == (1, 3, 17) and P.KS == (1, 2, 4, 16, 64, 100) and P.DS == (1, 3, 4, 5, 16) and P.MS == (0, 1, 4, 5, 8)
    assert {c[0] for c in GPU_CELLS} == set(P.BS) and {c[3] for c in GPU_CELLS} == set(P.MS)
    assert P.FRONT_CASES is O.L.LOGP_CASES and len(P.FRONT_CASES) == 3 and sorted(c[1] for c in P.FRONT_CASES) == [0, 1, 3]
    assert FACTOR == 22.0 and P.BOUNDARY == 1e-12 and all(s == 0.2 for s in O.SIGMA.values())


def test_no_target_of_any_device_cell_lies_within_the_margin_of_a_cumulative_boundary():
    """The index of a cell is asserted EXACTLY on the device: that holds only if no target u_m W lies within 1e-12 W of a
    running sum, whichever order the sums are formed in.  The targets and the running sums depend on ``lw`` and the seed alone
    (not on the device's normals), so the condition is checked here, on the CPU, for every cell the device tier runs."""
    for B, D, K, M in GPU_CELLS:
        for layout in (("BD",) if (B, D, K, M) in GPU_CELLS[:-3] else ("BD", "D", "scalar")):
            x, std, lw = P.kernel_inputs(B, D, K, layout)
            ref = P.restate(x, std, lw, torch.zeros(B, K, D), K, M)
            assert not ref.near.any(), (B, D, K, M, layout)
            assert (ref.index >= 0).all() and (ref.index < K).all()


# ---- a wrong implementation fails -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, D, K", [(17, 5, 16), (9, 4, 4)])
def test_damaged_restatements_miss_the_bar_on_the_mean_a_hundredfold(B, D, K):
    x, std, lw = P.kernel_inputs(B, D, K)
    z, p = O.draws(B, D, K)
    ref = P.restate(x, std, lw, z, K, 0)
    bar = FACTOR * P.floors(x, std, lw, z, K)["mean"]
    for name, damaged in (("uniform weights", P.restate(x, std, lw, z, K, 0, weights="uniform")),
                          ("z from the momentum index", P.restate(x, std, lw, p, K, 0))):
        miss = normalised_error(torch.from_numpy(damaged.mean), torch.from_numpy(ref.mean)) / bar
        print(f"\n[marginal_posterior] B{B} D{D} K{K}: bar {bar:.3e}; {name} miss it by {miss:.0f}x")
        assert miss >= 100.0, (name, miss)


# ---- the statistics -------------------------------------------------------------------------------------------------------------------
def test_draws_come_at_the_frequencies_of_their_weights():
    B, D, K, M = 17, 3, 4, 4096
    x, std, lw = P.kernel_inputs(B, D, K)
    _, i, _, _ = P.run_kernel(CPU, x, std, lw, K, M)
    z, _ = O.draws(B, D, K)
    wn = P.restate(x, std, lw, z, K, 0).wn
    freq = np.stack([(i.numpy() == k).mean(1) for k in range(K)], axis=1)
    tol = 5.0 * np.sqrt(wn * (1.0 - wn) / M)
    assert (np.abs(freq - wn) <= tol).all(), float((np.abs(freq - wn) / np.maximum(tol, 1e-300)).max())
    assert (freq[wn == 0.0] == 0.0).all() and (wn == 0.0).any()                          # a draw of weight zero is never chosen


def rotation_inputs():
    """(B, D, K, seed, sigma [D], x [B, D]) of the closed-form test: observations of the rotation field's own marginal N(0, s2)
    with noise sigma."""
    B, D, K, seed = 256, 3, 64, 11
    s2 = np.linalg.inv(rotation_leapfrog_matrix().T @ rotation_leapfrog_matrix())[0, 0]
    sigma = np.array([0.3, 0.5, 0.8], dtype=np.float32)
    g = np.random.default_rng(3)
    x = (np.sqrt(s2 + sigma.astype(np.float64) ** 2) * g.standard_normal((B, D))).astype(np.float32)
    return B, D, K, seed, sigma, x


def exact_rotation_posterior(x, sigma):
    """(mean, variance) [B, D] float64 of p(x_true | x): the prior is the marginal N(0, s2 I), s2 = [(M^T M)^-1]_qq."""
    M = rotation_leapfrog_matrix()
    s2, n2 = np.linalg.inv(M.T @ M)[0, 0], sigma.astype(np.float64) ** 2
    return x.astype(np.float64) * s2 / (s2 + n2), np.broadcast_to(s2 * n2 / (s2 + n2), x.shape)


ROTATION_RMS = 0.1686       # the float64 restatement's RMS distance from the closed form, in posterior standard deviations
ROTATION_FACTOR = 1.5       # the issue's allowance for fp32 and libm


def rotation_rms(mean, x, sigma):
    mu, v = exact_rotation_posterior(x, sigma)
    return float(np.sqrt(np.mean((np.asarray(mean, dtype=np.float64) - mu) ** 2 / v)))


def test_closed_form_posterior_of_the_rotation_field():
    """The leapfrog of the rotation field v = [alpha p, -beta q] is a linear map of unit determinant, the marginal of q0 is N(0,
    s2 I), and Gaussian noise on a Gaussian marginal has the closed-form posterior of mean x s2 / (s2 + sigma^2).  The K = 64
    mean of the host twin must lie within 1.5 times the float64 restatement's own RMS distance from it at the same K, seed and
    draws.  Measured: the restatement's distance is 0.1686 posterior standard deviations (ROTATION_RMS, which the device tier
    takes as its bar too); the host twin's differs from it in the seventh digit."""
    B, D, K, seed, sigma, x = rotation_inputs()
    Mx = rotation_leapfrog_matrix()
    xt, st = torch.from_numpy(x), torch.from_numpy(sigma)
    z0, _ = _native.marginal_observe_expand(xt, st, K, seed, 0)
    q, p = z0[:, :D].double().numpy(), z0[:, D:].double().numpy()
    z1 = np.concatenate([Mx[0, 0] * q + Mx[0, 1] * p, Mx[1, 0] * q + Mx[1, 1] * p], axis=1)
    ess = torch.empty(B)
    _, lw, _ = _native.marginal_weigh(torch.from_numpy(z1.astype(np.float32)), K, seed, 0, 0.0, 0.0, None, ess)
    _, _, mean, var = _native.marginal_observe_resample(xt, st, lw, K, 0, seed, 0)
    # the restatement: the same draws, everything behind them in float64
    z, pk = O.draws(B, D, K, CPU, seed, 0)
    y64 = P.particles(xt, st, z).double().numpy()
    p64 = pk.double().numpy()
    q1, p1 = Mx[0, 0] * y64 + Mx[0, 1] * p64, Mx[1, 0] * y64 + Mx[1, 1] * p64
    lw64 = -0.5 * ((q1 ** 2).sum(-1) + (p1 ** 2).sum(-1) - (p64 ** 2).sum(-1)) - D * 0.5 * math.log(2 * math.pi)
    ref = P.restate(xt, st, lw64.reshape(-1), z, K, 0, seed, 0)
    d_ref, d_got = rotation_rms(ref.mean, x, sigma), rotation_rms(mean.numpy(), x, sigma)
    _, v = exact_rotation_posterior(x, sigma)
    print(f"\n[marginal_posterior] rotation posterior, K = {K}: rms distance of the mean from the closed form: restatement "
          f"{d_ref:.6f}, host twin {d_got:.6f} posterior sd; var / exact {float(np.mean(var.numpy() / v)):.4f}; mean ess "
          f"{float(ess.mean()):.1f}")
    assert abs(d_ref - ROTATION_RMS) <= 2e-3 * ROTATION_RMS, d_ref
    assert d_got <= ROTATION_FACTOR * d_ref, (d_got, d_ref)
    assert ALPHA == 1.0 and BETA == 0.6 and STEPS == 4


# ---- the sharded entry points over gloo -------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import (shard_bounds, symplectic_log_prob_marginal_noisy_sharded as lp_sharded,
                                                symplectic_posterior_marginal_noisy_sharded as post_sharded)
        S.SymplecticFlowModel._solve_forward = P.stand_in_solve
        gathers = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, inp, **kw: (gathers.append(tuple(inp.shape)), real(out, inp, **kw))[1]
        front, x9, std9, c9, steps = P.front_case(P.FRONT_CASES[0])                       # D 4, C 3, B 9
        D, K, M, seed = x9.shape[1], 4, 3, 9
        kw = dict(method="leapfrog", num_steps=steps)
        ok = True
        for n in (8, 9, 1):                                  # an even split, a ragged one, fewer rows than ranks
            x, std, c = x9[:n], std9[:n], c9[:n]
            lo, hi = shard_bounds(n, world, rank)
            want = front.posterior_marginal_noisy(x, std, c, K, M, seed=seed, **kw)
            want_lp, want_ess = front.log_prob_marginal_noisy(x, std, c, K, seed=seed, return_ess=True, **kw)
            del gathers[:]
            got = post_sharded(front, x, std, c, seed=seed, num_draws=K, num_samples=M, **kw)
            ok &= len(gathers) == 1 and gathers[0][1:] == (M * D + 2 * D + 2 + M,)
            ok &= type(got) is odeint.NoisyPosterior and P.same(got, want)
            mine = post_sharded(front, local_x=x[lo:hi], local_noise_std=std[lo:hi], local_conditional=c[lo:hi], n_total=n,
                                seed=seed, num_draws=K, num_samples=M, **kw)
            ok &= len(gathers) == 2 and P.same(mine, want)
            local, span = post_sharded(front, x, std, c, seed=seed, num_draws=K, num_samples=M, gather=False, **kw)
            ok &= span == (lo, hi) and len(gathers) == 2 and P.same(local, P.rows_of(want, lo, hi))
            ok &= P.same(post_sharded(front, x, std[0], c, seed=seed, num_draws=K, num_samples=0, **kw),
                         front.posterior_marginal_noisy(x, std[0], c, K, 0, seed=seed, **kw))
            del gathers[:]
            lp = lp_sharded(front, x, std, c, seed=seed, num_draws=K, **kw)
            ok &= len(gathers) == 1 and torch.equal(P.bits(lp), P.bits(want_lp))
            lp, ess = lp_sharded(front, x, std, c, seed=seed, num_draws=K, return_ess=True, **kw)
            ok &= len(gathers) == 2 and gathers[1][1:] == (2,)
            ok &= torch.equal(P.bits(lp), P.bits(want_lp)) and torch.equal(P.bits(ess), P.bits(want_ess))
            (lp, ess), span = lp_sharded(front, local_x=x[lo:hi], local_noise_std=std[lo:hi], local_conditional=c[lo:hi],
                                         n_total=n, seed=seed, num_draws=K, return_ess=True, gather=False, **kw)
            ok &= span == (lo, hi) and len(gathers) == 2
            ok &= torch.equal(P.bits(lp), P.bits(want_lp[lo:hi])) and torch.equal(P.bits(ess), P.bits(want_ess[lo:hi]))
            ok &= torch.equal(P.bits(lp_sharded(front, x, 0.25, c, seed=seed, num_draws=K, **kw)),
                              P.bits(front.log_prob_marginal_noisy(x, 0.25, c, K, seed=seed, **kw)))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_sharded_entry_points_equal_the_unsharded_call_over_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    assert dict(q.get(timeout=5) for _ in range(2)) == {0: True, 1: True}


def test_sharded_argument_rules_and_one_process(monkeypatch):
    from flowfusion_amd.distributed import symplectic_log_prob_marginal_noisy_sharded as lp_sharded
    from flowfusion_amd.distributed import symplectic_posterior_marginal_noisy_sharded as post_sharded
    monkeypatch.setattr(S.SymplecticFlowModel, "_solve_forward", P.stand_in_solve)
    front, x, std, c, steps = P.front_case(P.FRONT_CASES[0])
    kw = dict(method="leapfrog", num_steps=steps)
    for fn in (lp_sharded, post_sharded):
        with pytest.raises(ValueError, match="noise_std"):
            fn(front, x, conditional=c, seed=1, **kw)
        with pytest.raises(ValueError, match="local_noise_std"):
            fn(front, x, std, c, local_noise_std=std, seed=1, **kw)
        with pytest.raises(ValueError, match="local_noise_std must hold"):
            fn(front, local_x=x, local_noise_std=std[:5], local_conditional=c, n_total=9, seed=1, **kw)
    want = front.posterior_marginal_noisy(x, std, c, 4, 3, seed=3, **kw)
    assert P.same(post_sharded(front, x, std, c, seed=3, num_draws=4, num_samples=3, **kw), want)
    got, span = post_sharded(front, local_x=x, local_noise_std=std, local_conditional=c, n_total=9, seed=3, num_draws=4,
                             num_samples=3, gather=False, **kw)
    assert span == (0, 9) and P.same(got, want)
    lp, ess = lp_sharded(front, x, std, c, seed=3, num_draws=4, return_ess=True, **kw)
    assert torch.equal(P.bits(lp), P.bits(want.log_prob)) and torch.equal(P.bits(ess), P.bits(want.ess))
