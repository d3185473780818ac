"""GPU tier of ``SymplecticFlowModel.posterior_marginal_noisy`` (csrc/ff_marginal_posterior.hip:
marginal_observe_resample_kernel).

The kernel, cell by cell (tests/_marginal_posterior_ref.check_cell): the index against the float64 restatement on the device's own
draws (inputs that keep every target 1e-12 W away from a cumulative boundary: asserted on the CPU), the samples bit for bit
ff_observe_expand's rows, mean and var within 22 fp32 floors, guard words intact around every output, and -- on weights that fp32
holds -- all four outputs bit for bit ff_weighted_resample's on the materialised particles.  Then the method on the three fused
pair units under ``method="leapfrog"`` (C = 3, 0 and 1): ``log_prob`` and ``ess`` bitwise the value method's, chunks, slices and
layouts bitwise, ``noise_std = 0``; one adaptive call; the closed-form posterior of the rotation field at the bar of
tests/test_marginal_posterior_host.py; a one-rank sharded call."""
import numpy as np
import pytest
import torch

from flowfusion_amd import _native, odeint
from tests import _leapfrog_pull_ref as L
from tests import _marginal_observe_ref as O
from tests import _marginal_posterior_ref as P
from tests._pushforward_ref import normalised_error
from tests.test_gpu_pushforward import FACTOR
from tests.test_gpu_symplectic import _rotation_model
from tests.test_marginal_posterior_host import (ROTATION_FACTOR, ROTATION_RMS, exact_rotation_posterior, rotation_inputs,
                                                rotation_rms)
from tests.test_symplectic_marginal_host import ALPHA, BETA, STEPS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", P.KS)
def test_kernel_against_the_restatement_the_expansion_and_weighted_resample(K):
    for D in P.DS:
        for B, M in ((1, 0), (3, 1), (17, 4), (3, 5), (17, 8)):
            P.check_cell(DEV, B, D, K, M)


def test_kernel_in_every_layout_of_sigma_one_float_off_alignment_and_on_the_second_grid_trip():
    for layout in ("BD", "D", "scalar"):
        P.check_cell(DEV, 3, 16, 16, 5, layout)
        P.check_cell(DEV, 17, 16, 100, 4, layout, offset=1)               # a misaligned samples view: the scalar body at D % 4 == 0
        P.check_cell(DEV, 3, 4, 64, 8, layout, offset=1)
    # more points than the largest grid holds groups for (2048 workgroups x 256 lanes / 64 lanes per point = 8192)
    B, D, K, M = 8192 + 37, 4, 64, 4
    x, std, lw = P.kernel_inputs(B, D, K)
    whole = P.run_kernel(DEV, x, std, lw, K, M)
    tail = P.run_kernel(DEV, x[8192:], std[8192:], lw[8192 * K:], K, M, first=P.OFFSET + 8192)
    assert all(torch.equal(P.bits(a[8192:]), P.bits(b)) for a, b in zip(whole, tail))


def test_kernel_depends_on_the_global_row_only_and_agrees_with_its_host_twin():
    B, D, K, M = 9, 5, 16, 6
    x, std, lw = P.kernel_inputs(B, D, K)
    whole = P.run_kernel(DEV, x, std, lw, K, M, first=100)
    part = P.run_kernel(DEV, x[3:7], std[3:7], lw[3 * K:7 * K], K, M, first=103)
    assert all(torch.equal(P.bits(a[3:7]), P.bits(b)) for a, b in zip(whole, part))
    # the twin: the same uniforms, libm's normals (2e-6) -- the same index away from boundaries, the moments to rounding
    hs, hi, hmu, hv = P.run_kernel("cpu", x, std, lw, K, M, first=100)
    assert torch.equal(hi, whole[1])
    assert float((hmu - whole[2]).abs().max()) <= 1e-4 * float(x.abs().max())
    assert float((hs - whole[0]).abs().max()) <= 1e-4 * float(x.abs().max())


def test_outputs_left_out_are_left_out_degenerate_points_and_one_draw():
    B, D, K, M = 6, 5, 100, 4
    x, std, lw = P.kernel_inputs(B, D, K)
    lw = torch.where(torch.isinf(lw), torch.full_like(lw, -45.0), lw)
    clean = P.run_kernel(DEV, x, std, lw, K, M)
    for want in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
        got = P.run_kernel(DEV, x, std, lw, K, M, want=want)
        assert all((g is None) == (not w) and (g is None or torch.equal(P.bits(g), P.bits(f))) for g, f, w in zip(got, clean, want))
    lw = lw.clone()
    lw[1 * K:2 * K] = -float("inf")                      # point 1: no draw above -inf
    lw[2 * K + K // 2] = float("nan")                    # point 2: a NaN
    lw[4 * K + K - 1] = -float("inf")                    # point 4: its last draw of weight zero
    s, i, mu, v = P.run_kernel(DEV, x, std, lw, K, M)
    for r in (1, 2):
        assert bool((i[r] == -1).all() and torch.isnan(s[r]).all() and torch.isnan(mu[r]).all() and torch.isnan(v[r]).all())
    for r in (0, 3, 5):
        assert all(torch.equal(P.bits(a[r]), P.bits(b[r])) for a, b in zip((s, i, mu, v), clean))
    assert bool((i[4] >= 0).all() and (i[4] != K - 1).all() and torch.isfinite(s[4]).all())
    # K = 1 with a finite lw: index 0, every sample and the mean are y_0, var = 0
    x1, std1, lw1 = P.kernel_inputs(B, D, 1)
    s, i, mu, v = P.run_kernel(DEV, x1, std1, lw1, 1, M)
    y, _ = _native.observe_expand(_dev(x1), _dev(std1), 1, P.SEED, P.OFFSET)
    y = y.cpu()
    assert bool((i == 0).all() and (v == 0).all()) and torch.equal(P.bits(mu), P.bits(y))
    assert torch.equal(P.bits(s), P.bits(y[:, None, :].expand(B, M, D).contiguous()))


def test_draws_come_at_the_frequencies_of_their_weights_on_the_device():
    B, D, K, M = 17, 3, 4, 4096
    x, std, lw = P.kernel_inputs(B, D, K)
    _, i, _, _ = P.run_kernel(DEV, x, std, lw, K, M)
    z, _ = O.draws(B, D, K, DEV)
    wn = P.restate(x, std, lw, z, K, 0).wn
    freq = np.stack([(i.numpy() == k).mean(1) for k in range(K)], axis=1)
    assert (np.abs(freq - wn) <= 5.0 * np.sqrt(wn * (1.0 - wn) / M)).all()


# ---- the method -----------------------------------------------------------------------------------------------------------------------
_FRONTS = {}


def front_of(case):
    """(front end, x, noise_std [B, D], raw conditional or None -- on the device --, num_steps), made once per case."""
    key = L.front_id(case)
    if key not in _FRONTS:
        front, x, std, cond, steps = P.front_case(case)
        _FRONTS[key] = (front.to(DEV), _dev(x), _dev(std), _dev(cond), steps)
    return _FRONTS[key]


@pytest.mark.parametrize("case", P.FRONT_CASES, ids=L.front_id)
def test_method_on_the_fused_pair_units(case):
    front, x, std, cond, steps = front_of(case)
    assert front._fusable()
    B, D = x.shape
    K, M, seed, first = 4, 5, O.SEED, O.OFFSET
    kw = dict(method="leapfrog", num_steps=steps, seed=seed, sample_offset=first)
    post = front.posterior_marginal_noisy(x, std, cond, K, M, **kw)
    assert type(post) is odeint.NoisyPosterior and all(f.device.type == "cuda" for f in post)
    assert post.samples.shape == (B, M, D) and post.index.shape == (B, M) and post.index.dtype == torch.int32
    lp, ess = front.log_prob_marginal_noisy(x, std, cond, K, return_ess=True, **kw)
    assert torch.equal(P.bits(post.log_prob), P.bits(lp)) and torch.equal(P.bits(post.ess), P.bits(ess))
    y, _ = _native.observe_expand(x, std, K, seed, first)
    rows = (torch.arange(B, device=DEV)[:, None] * K + post.index.long()).reshape(-1)
    assert bool((post.index >= 0).all() and (post.index < K).all() and (post.var >= 0).all())
    assert torch.equal(P.bits(post.samples.reshape(B * M, D)), P.bits(y[rows]))
    # the float64 restatement on the lw of the route and the device's own draws
    z0, ck = _native.marginal_observe_expand(x, std, K, seed, first, _dev(front.shift), _dev(front.scale), front._norm_cond(cond))
    z1 = front._solve_forward(z0, ck, None, None, "leapfrog", None, steps)
    _, lw, _ = _native.marginal_weigh(z1, K, seed, first)
    z, _ = O.draws(B, D, K, DEV, seed, first)
    ref = P.restate(x, std, lw.cpu(), z, K, M, seed, first)
    assert not ref.near.any() and np.array_equal(post.index.cpu().numpy(), ref.index)
    fl = P.floors(x, std, lw.cpu(), z, K)
    for name in ("mean", "var"):
        err = normalised_error(getattr(post, name), torch.from_numpy(getattr(ref, name)))
        print(f"\n[marginal_posterior] {L.front_id(case)} {name}: err {err:.3e} floor {fl[name]:.3e} = {err / fl[name]:.2f} floors")
        assert err <= FACTOR * fl[name], (name, err, fl[name])
    # chunks, slices with sample_offset moved, the layouts of sigma: the same bits
    for chunk in (1, 4, B):
        assert P.same(front.posterior_marginal_noisy(x, std, cond, K, M, chunk_points=chunk, **kw), post), chunk
    lo, hi = 2, B - 1
    part = front.posterior_marginal_noisy(x[lo:hi], std[lo:hi], None if cond is None else cond[lo:hi], K, M,
                                          **dict(kw, sample_offset=first + lo))
    assert P.same(part, P.rows_of(post, lo, hi))
    layouts = (0.25, torch.tensor(0.25), torch.full((D,), 0.25), torch.full((B, D), 0.25, device=DEV))
    one = front.posterior_marginal_noisy(x, layouts[0], cond, K, M, chunk_points=4, **kw)
    assert not P.same(one, post)
    for s in layouts[1:]:
        assert P.same(front.posterior_marginal_noisy(x, s, cond, K, M, **kw), one)
    p0 = front.posterior_marginal_noisy(x, std, cond, K, 0, **kw)
    assert p0.samples.shape == (B, 0, D) and torch.equal(P.bits(p0.mean), P.bits(post.mean))
    # noise_std = 0: every sample equals x, var = 0, log_prob bitwise log_prob_marginal
    for zero in (0.0, torch.zeros(D), torch.zeros_like(std)):
        pz = front.posterior_marginal_noisy(x, zero, cond, K, M, **kw)
        assert torch.equal(P.bits(pz.samples), P.bits(x[:, None, :].expand(B, M, D).contiguous())) and torch.equal(pz.mean, x)
        assert bool((pz.var.double() <= 1e-24 * torch.clamp(x.double() ** 2, min=1.0)).all())
        l1, e1 = front.log_prob_marginal(x, cond, K, return_ess=True, **kw)
        assert torch.equal(P.bits(pz.log_prob), P.bits(l1)) and torch.equal(P.bits(pz.ess), P.bits(e1))


def test_one_adaptive_call_solves_all_rows_at_once():
    front, x, std, cond, _ = front_of(P.FRONT_CASES[0])
    x, std, cond = x[:5], std[:5], cond[:5]
    K, M, seed = 4, 3, 21
    post = front.posterior_marginal_noisy(x, std, cond, K, M, seed=seed)                  # dopri5, the default
    lp, ess = front.log_prob_marginal_noisy(x, std, cond, K, seed=seed, return_ess=True)
    assert torch.equal(P.bits(post.log_prob), P.bits(lp)) and torch.equal(P.bits(post.ess), P.bits(ess))
    y, _ = _native.observe_expand(x, std, K, seed, 0)
    rows = (torch.arange(5, device=DEV)[:, None] * K + post.index.long()).reshape(-1)
    assert torch.equal(P.bits(post.samples.reshape(5 * M, -1)), P.bits(y[rows]))
    assert bool(torch.isfinite(post.mean).all() and (post.var >= 0).all() and ((post.ess > 0) & (post.ess <= K * (1 + 1e-6))).all())
    with pytest.raises(ValueError, match="chunk_points with method='dopri5'"):
        front.posterior_marginal_noisy(x, std, cond, K, M, seed=seed, chunk_points=2)


def test_closed_form_posterior_of_the_rotation_field_on_the_device():
    """tests/test_marginal_posterior_host.py's closed form through the whole method: four leapfrog steps of the rotation
    network, K = 64.  The bar is that test's: 1.5 times the float64 restatement's RMS distance from the closed form (0.1686
    posterior standard deviations)."""
    B, D, K, seed, sigma, xw = rotation_inputs()
    fm, shift, scale = _rotation_model(D, 0, 6, [64], ALPHA, BETA)
    assert fm._fusable()
    x = (torch.from_numpy(xw).double() * scale + shift).float()
    std = (torch.from_numpy(sigma).double() * scale).float()
    post = fm.posterior_marginal_noisy(x.to(DEV), std.to(DEV), None, K, 8, method="leapfrog", num_steps=STEPS, seed=seed)
    white = lambda t: ((t.double().cpu() - shift) / scale).numpy()
    sw = (std.double() / scale).numpy()
    got = rotation_rms(white(post.mean), white(x), sw)
    mu, v = exact_rotation_posterior(white(x), sw)
    ratio = float(np.mean(post.var.double().cpu().numpy() / (scale.numpy() ** 2) / v))
    pooled = float(np.var((white(post.samples.reshape(-1, D)).reshape(B, 8, D) - mu[:, None, :]) / np.sqrt(v)[:, None, :]))
    print(f"\n[marginal_posterior] rotation posterior on the device, K = {K}: rms distance of the mean {got:.6f} posterior sd "
          f"(restatement {ROTATION_RMS}); var / exact {ratio:.4f}; pooled sample variance {pooled:.4f}; mean ess "
          f"{float(post.ess.mean()):.1f}")
    assert got <= ROTATION_FACTOR * ROTATION_RMS, got


def test_one_rank_sharded_calls():
    from flowfusion_amd.distributed import symplectic_log_prob_marginal_noisy_sharded as lp_sharded
    from flowfusion_amd.distributed import symplectic_posterior_marginal_noisy_sharded as post_sharded
    front, x, std, cond, steps = front_of(P.FRONT_CASES[2])
    kw = dict(method="leapfrog", num_steps=steps)
    want = front.posterior_marginal_noisy(x, std, cond, 4, 3, seed=3, **kw)
    assert P.same(post_sharded(front, x, std, cond, seed=3, num_draws=4, num_samples=3, **kw), want)
    got, span = post_sharded(front, local_x=x, local_noise_std=std, local_conditional=cond, n_total=x.shape[0], seed=3,
                             num_draws=4, num_samples=3, gather=False, **kw)
    assert span == (0, x.shape[0]) and P.same(got, want)
    lp, ess = lp_sharded(front, x, std, cond, seed=3, num_draws=4, return_ess=True, **kw)
    assert torch.equal(P.bits(lp), P.bits(want.log_prob)) and torch.equal(P.bits(ess), P.bits(want.ess))
