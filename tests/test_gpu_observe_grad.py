"""GPU tier of ``log_prob_noisy_grad`` (csrc/ff_observe.hip: ff_observe_keep, ff_observe_grad_reduce; odeint.log_prob_noisy_grad):
the two kernels between guard words against their host twins over the grid of tests/test_observe_grad_host.py, any cut of the
batch, the five front ends against the float64 reference (tests/_observe_grad_ref.py: ``torch.autograd.grad`` through
``logsumexp`` of the fixed-grid log-density of the K expanded rows) at the derivative families' bar, the bitwise properties, and
``min_weight``.

Tolerances.  Raw kernels: one fp32 ulp -- double sums rounded once differ from the host twin's only at a rounding tie.  The
noise draws are the exception the library documents (csrc/ff_marginal.h): the host twin's come through libm and agree with the
device's to 2e-6, not bit for bit, so ``grad_noise_std`` is held to one ulp against the float64 restatement evaluated with the
DEVICE's draws (ff_normal_fill: bitwise the kernel's), as the host twin is with its own in the host file, and against the host
twin itself to what 2e-6 in every z can move it.  Front ends: FACTOR = 22 fp32 floors of the case, as measured on the CPU
(tests/test_gpu_pushforward.py); tests/test_observe_grad_host.py shows that the floors are small, the weights neither uniform
nor one-hot, and that uniform weights or a dropped z miss the bar by more than 100x.
"""
import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from tests import _observe_grad_ref as OG
from tests import _pushforward_ref as R
from tests.test_gpu_pushforward import FACTOR, GUARD, _guarded, _payload, fp32_floor
from tests.test_observe_grad_host import GRID, NB, raw_inputs, ulps

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z_GAP = 2e-6                    # the device's normals against libm's (csrc/ff_marginal.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV).contiguous()


def device_draws(seed, offset, B, D, K):
    """z [B, K, D]: the kernel's own draws, from ff_normal_fill under the noise indices FF_OBS_NOISE_BASE + k."""
    return torch.stack([_native.normal_fill(B, D, seed, offset, DEV, noise_index=_native.OBS_NOISE_BASE + k) for k in range(K)], 1)


def raw_reduce(lp, rows, gx, gc, std, K, seed, offset, B=NB):
    """ff_observe_grad_reduce on device copies, its three outputs between guard words on NaN-prefilled buffers."""
    D, C = gx.shape[1], 0 if gc is None else gc.shape[1]
    bufs = [_guarded(B * D), _guarded(B * C) if C else None, _guarded(B * D)]
    view = lambda b, cols: None if b is None else b[GUARD:GUARD + B * cols].view(B, cols)
    _native.observe_grad_reduce(_dev(lp), _dev(rows), _dev(gx), _dev(gc), _dev(std), K, seed, offset, True, view(bufs[0], D),
                                view(bufs[1], C), view(bufs[2], D))
    torch.cuda.synchronize()
    return [None if b is None else _payload(b, (B, cols)).cpu() for b, cols in zip(bufs, (D, C, D))]


# ---- the raw kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, Dd, C, per_point", GRID)
def test_raw_kernels_against_their_host_twins(K, Dd, C, per_point):
    lp, keep, rows, gx, gc, std = raw_inputs(K, Dd, C, per_point)
    for m in (0.0, 1e-3):
        assert torch.equal(_native.observe_keep(_dev(lp), K, m).cpu(), _native.observe_keep(lp, K, m)), m
    host = _native.observe_grad_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET)
    got = raw_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET)
    line = f"\n[observe_grad] raw K {K} D {Dd} C {C} std {'[B, D]' if per_point else '[D]'}:"
    for what, a, b in (("grad_x", got[0], host[0]), ("grad_c", got[1], host[1])):
        if b is not None:
            line += f" {what} {ulps(a.numpy(), b.numpy().astype(np.float64)):.2f} ulp, bitwise {torch.equal(a, b)};"
    z = device_draws(OG.SEED, OG.OFFSET, NB, Dd, K).cpu().numpy()
    ref = OG.grad_reduce64(lp.numpy(), rows.numpy(), gx.numpy(), None, K, z)[2]
    gap = float((got[2] - host[2]).abs().max())
    wn, _ = OG.weights64(lp.numpy(), K)
    reach = np.where(rows.numpy().reshape(NB, K) >= 0, wn, 0.0).sum(axis=1).max() * float(gx.abs().max()) * Z_GAP
    line += f" grad_noise_std {ulps(got[2].numpy(), ref):.2f} ulp of float64 with the device's draws, host twin within {gap:.2e}"
    print(line + f" (2e-6 in z reaches {reach:.2e})")
    assert ulps(got[0].numpy(), host[0].numpy().astype(np.float64)) <= 1.0
    assert C == 0 or ulps(got[1].numpy(), host[1].numpy().astype(np.float64)) <= 1.0
    assert ulps(got[2].numpy(), ref) <= 1.0
    assert gap <= reach + 2.0 ** -23 * float(host[2].abs().max())


@pytest.mark.parametrize("K, Dd, C", [(3, 5, 3), (16, 16, 0), (130, 32, 3)])
def test_any_cut_of_the_batch_is_bitwise(K, Dd, C):
    lp, keep, rows, gx, gc, std = raw_inputs(K, Dd, C, True)
    whole = raw_reduce(lp, rows, gx, gc, std, K, OG.SEED, OG.OFFSET)
    keep_dev = _native.observe_keep(_dev(lp), K, 1e-3).cpu()
    for lo in range(0, NB, 11):
        hi = min(NB, lo + 11)
        seg = slice(lo * K, hi * K)
        assert torch.equal(_native.observe_keep(_dev(lp[seg]), K, 1e-3).cpu(), keep_dev[seg])
        first = int(rows[:lo * K].max()) + 1 if lo else 0
        part_rows = torch.where(rows[seg] >= 0, rows[seg] - first, -1).to(torch.int32)
        n = int(part_rows.max()) + 1
        part = raw_reduce(lp[seg], part_rows, gx[first:first + n], None if gc is None else gc[first:first + n], std[lo:hi], K,
                          OG.SEED, OG.OFFSET + lo, B=hi - lo)
        for a, b in zip(part, whole):
            assert (a is None and b is None) or torch.equal(a, b[lo:hi]), (lo, hi)


# ---- the front ends -----------------------------------------------------------------------------------------------------------------
def _call(case, front, x, std, c, opts, **more):
    args, kw = OG.call_args(case, front, x, std, c, DEV)
    return front.log_prob_noisy_grad(*args, options=opts, **dict(kw, **more))


def _value_rows(case, front, x, std, c, opts):
    """(y, cond rows, lp [B K], grad rows) of the case's expanded rows from the front end's own ``log_prob_grad``: what
    ``log_prob_noisy_grad`` reduces, through the public interface."""
    y, ck = _native.observe_expand(_dev(x), _dev(std), case.K, OG.SEED, OG.OFFSET, _dev(c))
    kw = dict(method="rk4", options=opts)
    if case.P > 0:
        kw.update(probe="philox", seed=OG.SEED, sample_offset=OG.OFFSET * case.K, num_probes=case.P)
    if case.kind == "flow":
        kw["hutchinson"] = case.P > 0
    lp, gx, gc = front.log_prob_grad(y, *(() if ck is None else (ck,)), **kw)
    return y, ck, lp.view(-1).contiguous(), gx, gc


@pytest.mark.parametrize("case", OG.CASES, ids=lambda c: c.name)
def test_front_end_against_the_float64_reference(case):
    front, _, opts = OG.case_front(case)
    front = front.to(DEV)
    x, std, c = OG.case_inputs(case)
    lp, gx, gc, ess, gs = _call(case, front, x, std, c, opts, return_ess=True, return_noise_grad=True)
    assert lp.shape == (OG.B, 1) and gx.shape == (OG.B, case.D) and gs.shape == (OG.B, case.D) and ess.shape == (OG.B,)
    assert (gc is None) == (case.C == 0) and (gc is None or gc.shape == (OG.B, case.C))
    # log_p and ess: log_prob_noisy's, bit for bit (the wrappers' log_prob_noisy is hard-wired to adaptive dopri5: theirs is
    # ff_logmeanexp of their fixed-grid log_prob_grad value on the expanded rows)
    if case.wrap is None:
        args, kw = OG.call_args(case, front, x, std, c, DEV)
        want_lp, want_ess = front.log_prob_noisy(*args, options=opts, return_ess=True, **kw)
    else:
        rows_lp = _value_rows(case, front, x, std, c, opts)[2]
        want_ess = torch.empty(OG.B, device=DEV)
        want_lp = _native.logmeanexp(rows_lp, case.K, ess=want_ess)
    assert torch.equal(lp.view(-1), want_lp.view(-1)) and torch.equal(ess, want_ess)
    stats = front.last_noisy_grad_stats
    assert stats == {"rows": OG.B * case.K, "rows_kept": OG.B * case.K, "gradient_rows": OG.B * case.K * (case.P or case.D)}
    r = OG.references(case)
    r64, r32 = r[torch.float64], r[torch.float32]
    assert float((lp.cpu().double()[:, 0] - r64.log_p).abs().max()) <= 1e-4 * float(r64.log_p.abs().max().clamp_min(1.0))
    results = [(what, R.normalised_error(got, getattr(r64, what)), fp32_floor(getattr(r32, what), getattr(r64, what)))
               for what, got in (("gx", gx), ("gc", gc), ("gs", gs)) if got is not None]
    line = f"\n[observe_grad] {case.name}: device ess {float(ess.min()):.2f} .. {float(ess.max()):.2f};"
    for what, err, floor in results:
        line += f" {what} err {err:.3e} floor {floor:.3e} ({err / floor:.2f} floors);"
    print(line)
    for what, err, floor in results:
        assert err <= FACTOR * floor, (what, err, floor, FACTOR * floor)


def test_bitwise_properties_on_a_hutchinson_model():
    case = OG.CASES[2]                       # the conditional flow, three probes per row
    front, _, opts = OG.case_front(case)
    front = front.to(DEV)
    x, std, c = OG.case_inputs(case)
    more = dict(return_ess=True, return_noise_grad=True)
    whole = _call(case, front, x, std, c, opts, **more)
    assert all(torch.equal(a, b) for a, b in zip(_call(case, front, x, std, c, opts, **more), whole))         # a re-run
    for chunk in (1, 7, OG.B):
        got = _call(case, front, x, std, c, opts, chunk_points=chunk, **more)
        assert all(torch.equal(a, b) for a, b in zip(got, whole)), chunk
    part = _call(case, front, x[8:19], std[8:19], c[8:19], opts, sample_offset=OG.OFFSET + 8, **more)
    assert all(torch.equal(a, b[8:19]) for a, b in zip(part, whole))
    # a [D] vector is the [B, D] tensor of the same values
    vec = _call(case, front, x, std[0], c, opts, **more)
    assert all(torch.equal(a, b) for a, b in zip(vec, _call(case, front, x, std[0].expand(OG.B, case.D), c, opts, **more)))
    # no noise, one draw: log_prob_grad with the counter-based probes of the same seed and offset
    one = case._replace(K=1)
    lp, gx, gc, gs = _call(one, front, x, torch.zeros(case.D), c, opts, return_noise_grad=True)
    want = front.log_prob_grad(_dev(x), _dev(c), method="rk4", options=opts, hutchinson=True, probe="philox", seed=OG.SEED,
                               sample_offset=OG.OFFSET, num_probes=case.P)
    assert torch.equal(lp, want[0]) and torch.equal(gx, want[1]) and torch.equal(gc, want[2])
    z = device_draws(OG.SEED, OG.OFFSET, OG.B, case.D, 1)[:, 0]
    assert torch.equal(gs, (-(z.double() * gx.double())).float())


def test_min_weight_skips_rows_and_keeps_the_weights_of_the_full_sum():
    case, m = OG.CUT_CASE, OG.CUT
    front, _, opts = OG.case_front(case)
    front = front.to(DEV)
    x, std, c = OG.case_inputs(case)
    full = _call(case, front, x, std, c, opts, return_noise_grad=True)
    full_stats = dict(front.last_noisy_grad_stats)
    cut = _call(case, front, x, std, c, opts, return_noise_grad=True, min_weight=m)
    stats = dict(front.last_noisy_grad_stats)
    y, ck, lp, gxr, gcr = _value_rows(case, front, x, std, c, opts)
    keep = OG.keep64(lp.cpu().numpy(), case.K, m)
    n, rows = int(keep.sum()), OG.B * case.K
    print(f"\n[observe_grad] min_weight {m}: kept {n} of {rows} rows (at 0: {full_stats['rows_kept']})")
    assert n <= 2 * rows // 3                                   # at least a third of the draws are skipped
    assert stats == {"rows": rows, "rows_kept": n, "gradient_rows": n * case.P}
    assert full_stats == {"rows": rows, "rows_kept": int(OG.keep64(lp.cpu().numpy(), case.K, 0.0).sum()),
                          "gradient_rows": full_stats["rows_kept"] * case.P}
    assert torch.equal(cut[0], full[0])                          # the value does not know about min_weight
    # bitwise the raw reduce on ALL gradient rows with the skipped ones zeroed: the weights are those of the full W
    mask = torch.from_numpy(keep).to(DEV).bool()[:, None]
    every = torch.arange(rows, dtype=torch.int32, device=DEV)
    want = _native.observe_grad_reduce(lp, every, torch.where(mask, gxr, 0.0), torch.where(mask, gcr, 0.0), _dev(std), case.K,
                                       OG.SEED, OG.OFFSET)
    for what, a, b in zip(("grad_x", "grad_c", "grad_noise_std"), cut[1:], want):
        assert torch.equal(a, b), what
    # ... and within K m max |grad lp| of the call that keeps every row
    z = device_draws(OG.SEED, OG.OFFSET, OG.B, case.D, case.K).view(rows, case.D)
    for what, a, b, g in (("grad_x", cut[1], full[1], gxr), ("grad_c", cut[2], full[2], gcr), ("grad_noise_std", cut[3], full[3], z * gxr)):
        dev, bound = float((a - b).abs().max()), case.K * m * float(g.abs().max())
        print(f"[observe_grad] min_weight {m} {what}: deviation {dev:.3e}, bound {bound:.3e}")
        assert 0.0 < dev <= bound, (what, dev, bound)
