"""Reference for the gradient of the K-momentum marginal log-density (``SymplecticFlowModel.log_prob_marginal_grad``;
csrc/ff_marginal.hip: ff_marginal_weigh, ff_marginal_grad_reduce): ``tests/_leapfrog_pull_ref.logp_map`` on each of the K momenta
of every point, stacked, composed with ``torch.logsumexp(...) - log K``, and ``torch.autograd.grad`` of the sum with respect to
``x`` and the raw ``conditional``.  float64 is the truth; float32 gives a case's floor.  The momenta are an INPUT here: the tests
hand over the ones the code under test used, read from ``marginal_expand``'s output on the same device (the host's come through
libm, the device's through the hardware: they agree to rounding, not bit for bit).

Also here: the front-end cases shared by tests/test_marginal_grad_host.py (their conditions, on the CPU) and
tests/test_gpu_marginal_grad.py (the device against them), and the float64 numpy restatement of the two kernels.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from flowfusion_amd import _native
from tests import _leapfrog_pull_ref as L
from tests._observe_grad_ref import keep64, row_of, weights64  # noqa: F401  (the keep rule and the compaction are shared)

SEED, OFFSET = 2029, 3          # the momenta's key: a non-zero first global row
KS = (2, 4)                     # momenta per point of the front-end cases
CASES = [(case, K) for case in L.LOGP_CASES for K in KS]
# the min_weight > 0 case: (front-end case, K, min_weight).  The literal comes from a float64 scan of the normalised weights of
# that case (tests/test_marginal_grad_host.py asserts what the scan promised: between a quarter and three quarters of the draws
# kept, no weight within 1e-3 relative of the threshold).
CUT_CASE, CUT_K, CUT = L.LOGP_CASES[0], 4, 0.21


def case_id(ck):
    return f"{L.front_id(ck[0])}-K{ck[1]}"


def momenta(x, K, dev="cpu", seed=SEED, sample_offset=OFFSET):
    """p0 [B, K, D] float32 on the CPU: the momenta ``marginal_expand`` writes for ``x`` on ``dev`` under (seed, sample_offset)."""
    B, D = x.shape
    z0, _ = _native.marginal_expand(x.detach().to(dev, torch.float32).contiguous(), K, seed, sample_offset)
    return z0.view(B, K, 2 * D)[:, :, D:].cpu().contiguous()


def marginal_reference(front, x, p0, cond, num_steps, dtype=torch.float64):
    """The reference of one call in ``dtype``: ``log_p`` [B], ``gx`` [B, D], ``gc`` [B, C] or None, ``ess`` [B] -- and what the
    deliberately wrong references are made of: ``lw`` [B, K], the normalised weights ``wn`` [B, K] and the rows' own gradients
    ``g`` [B, K, D] / ``h`` [B, K, C].  ``p0`` [B, K, D]: the momenta, constants of the estimate."""
    f = L.logp_map(front, dtype)
    K = int(p0.shape[1])
    xv = x.detach().to("cpu", dtype).clone().requires_grad_(True)
    cv = None if cond is None else cond.detach().to("cpu", dtype).clone().requires_grad_(True)
    pk = p0.detach().to("cpu", dtype)
    wrt = (xv,) if cv is None else (xv, cv)
    with torch.enable_grad():
        lw = torch.stack([f(xv, pk[:, k], cv, num_steps) for k in range(K)], dim=1)          # (each with - sum log scale)
        Lm = torch.logsumexp(lw, dim=1) - math.log(K)
        rows = [torch.autograd.grad(lw[:, k].sum(), wrt, retain_graph=True) for k in range(K)]
        g = torch.autograd.grad(Lm.sum(), wrt)
    wn = torch.softmax(lw.detach(), dim=1)
    return SimpleNamespace(log_p=Lm.detach(), gx=g[0], gc=None if cv is None else g[1], ess=1.0 / (wn ** 2).sum(dim=1),
                           lw=lw.detach(), wn=wn, g=torch.stack([r[0] for r in rows], dim=1),
                           h=None if cv is None else torch.stack([r[1] for r in rows], dim=1))


def weighted(ref, weights):
    """(gx, gc or None) of a reference under other weights [B, K]: the uniform, rolled and truncated variants."""
    w = weights.to(ref.g.dtype)[..., None]
    return (w * ref.g).sum(1), (None if ref.h is None else (w * ref.h).sum(1))


_REFS = {}


def references(ck, dev="cpu"):
    """{dtype: marginal_reference} of a front-end case with the momenta of ``dev``, computed once and shared."""
    key = (case_id(ck), dev)
    if key not in _REFS:
        case, K = ck
        front, _, x, _, _, cond = L.front_inputs(case)
        p0 = momenta(x, K, dev)
        _REFS[key] = {dt: marginal_reference(front, x, p0, cond, case[4], dt) for dt in (torch.float32, torch.float64)}
    return _REFS[key]


def floors(r32, r64):
    """{what: fp32 floor} of a case, ``what`` in gx / gc (where the model has a conditional)."""
    from tests.test_gpu_pushforward import fp32_floor
    out = {"gx": fp32_floor(r32.gx, r64.gx)}
    if r64.gc is not None:
        out["gc"] = fp32_floor(r32.gc, r64.gc)
    return out


# ---- the two kernels restated in float64 numpy ---------------------------------------------------------------------------------
HALF_LOG_2PI = 0.91893853320467274178


def weigh64(z1, p0, K, log_det, min_weight):
    """(log_p [B], ess [B], lw [B K], keep [B K] int32) in float64 from ``z1`` [B K, 2 D] and the momenta ``p0`` [B, K, D]."""
    z1 = np.asarray(z1, dtype=np.float64)
    p0 = np.asarray(p0, dtype=np.float64).reshape(z1.shape[0], -1)
    D = p0.shape[1]
    lw = -0.5 * ((z1 ** 2).sum(axis=1) - (p0 ** 2).sum(axis=1)) - D * HALF_LOG_2PI
    rows = lw.reshape(-1, K)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = rows.max(axis=1, keepdims=True)
        w = np.exp(rows - np.where(np.isfinite(mx), mx, 0.0))
        log_p = (mx[:, 0] + np.log(w.sum(axis=1))) - math.log(K) - log_det
        ess = w.sum(axis=1) ** 2 / (w ** 2).sum(axis=1)
    return log_p, ess, lw, keep64(lw, K, min_weight)


def grad_reduce64(lw, rows, gz_rows, gc_rows, K, scale=None, cond_scale=None):
    """(grad_x [B, D], grad_c [B, C] or None) in float64 from the kept rows' pull-backs; ``rows`` = row_of [B K], ``gz_rows``
    [n, 2 D] (the q half is taken).  Degenerate points are NaN."""
    wn, bad = weights64(lw, K)
    Bn = wn.shape[0]
    rows = np.asarray(rows).reshape(Bn, K)
    D = np.asarray(gz_rows).shape[1] // 2

    def pick(t):
        t = np.asarray(t, dtype=np.float64)
        t = t if t.shape[0] else np.zeros((1, t.shape[1]))      # (nothing kept: nothing is picked)
        return np.where((rows >= 0)[..., None], t[np.maximum(rows, 0)], 0.0)

    w = np.where(rows >= 0, wn, 0.0)[..., None]
    gx = (w * pick(np.asarray(gz_rows)[:, :D])).sum(axis=1)
    if scale is not None:
        gx = gx / np.asarray(scale, dtype=np.float64)
    gc = None
    if gc_rows is not None:
        gc = (w * pick(gc_rows)).sum(axis=1)
        if cond_scale is not None:
            gc = gc / np.asarray(cond_scale, dtype=np.float64)
    for t in (gx, gc):
        if t is not None:
            t[bad] = np.nan
    return gx, gc


# ---- the kernel cases, run by the host file on the host twins and by the GPU file on the device --------------------------------
# (D, K): the scalar and the vector body, one trip and a partial second trip of the row loop, at 1, 4 and 8 lanes per row;
# C by D: none, the scalar and the vector body of the conditional's rows
KERNEL_SHAPES = [(1, 1), (4, 65), (5, 3), (16, 17), (17, 4), (32, 9)]
KERNEL_C = {1: 0, 4: 4, 5: 3, 16: 0, 17: 1, 32: 8}
BIG = (4, 64, 1 << 14)          # (D, K, B): more lane groups than the largest grid holds, so the grid-stride loop trips twice
MIN_WEIGHT = 0.05


def ulps(got, ref64):
    """max |got - ref| in units of the fp32 spacing at the reference (NaN must meet NaN)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert (np.isnan(got) == np.isnan(ref64)).all()
    ok = ~np.isnan(ref64)
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - ref64[ok]) / np.spacing(np.abs(ref64[ok]).astype(np.float32)).astype(np.float64)).max())


def kernel_inputs(D, K, B, C, spread=0.6):
    """Synthetic (z1 [B K, 2 D], gz [B K, 2 D], gc [B K, C] or None, scale [D], cond_scale [C] or None) on the CPU: rows of
    comparable length, so that the K weights of a point are neither uniform nor one-hot, and one per point that is skipped."""
    g = torch.Generator().manual_seed(7 + 1000 * K + 10 * D + B)
    z1 = torch.randn(B * K, 2 * D, generator=g) * (1.0 + spread * torch.rand(B * K, 1, generator=g)) / math.sqrt(max(D, 1) / 2.0)
    if K > 1:
        z1[K - 1::K] *= 2.5                                    # the last draw of every point: far out, below any min_weight
    gz = torch.randn(B * K, 2 * D, generator=g)
    gc = torch.randn(B * K, C, generator=g) if C else None
    scale = 0.5 + torch.rand(D, generator=g)
    cscale = 0.5 + torch.rand(C, generator=g) if C else None
    return z1, gz, gc, scale, cscale


def run_kernels(dev, D, K, B, C, min_weight=MIN_WEIGHT, z1=None):
    """Both kernels on ``dev`` on the synthetic inputs of a cell, every row that was not kept POISONED with NaN in ``gz`` /
    ``gc`` (row_of = the row itself where kept), and once more on the compacted rows.  Everything comes back on the CPU."""
    zs, gz, gc, scale, cscale = kernel_inputs(D, K, B, C)
    z1 = zs if z1 is None else z1
    to = lambda t: None if t is None else t.to(dev)
    x = torch.zeros(B, D)
    p0 = momenta(x, K, dev)
    log_det = 0.375
    ess, ess_r = torch.empty(B, device=dev), torch.empty(B, device=dev)
    out, lw, keep = _native.marginal_weigh(to(z1), K, SEED, OFFSET, log_det, min_weight, ess=ess)
    out_r = _native.marginal_reduce(to(z1), K, SEED, OFFSET, log_det, ess=ess_r)
    kept = keep.cpu() > 0
    full_of = torch.where(kept, torch.arange(B * K, dtype=torch.int32), -1).to(torch.int32)
    gzp, gcp = gz.clone(), (None if gc is None else gc.clone())
    gzp[~kept] = float("nan")
    if gcp is not None:
        gcp[~kept] = float("nan")
    gx, gcond = _native.marginal_grad_reduce(lw, to(full_of), to(gzp), to(gcp), K, to(scale), to(cscale))
    rows = torch.nonzero(kept).view(-1)
    gx2, gcond2 = _native.marginal_grad_reduce(lw, to(row_of(keep.cpu())), to(gz[rows].contiguous()),
                                               None if gc is None else to(gc[rows].contiguous()), K, to(scale), to(cscale))
    cpu = lambda t: None if t is None else t.cpu()
    return SimpleNamespace(z1=z1, p0=p0, gz=gz, gc=gc, scale=scale, cscale=cscale, log_det=log_det, min_weight=min_weight,
                           out=cpu(out), ess=cpu(ess), out_r=cpu(out_r), ess_r=cpu(ess_r), lw=cpu(lw), keep=cpu(keep),
                           full_of=full_of, gx=cpu(gx), gcond=cpu(gcond), gx2=cpu(gx2), gcond2=cpu(gcond2))


def bits(t):
    return t.contiguous().view(torch.int32)


def check_kernels(r, K, label=""):
    """What every cell asserts of ``run_kernels``' results, on either side."""
    assert torch.equal(bits(r.out), bits(r.out_r)) and torch.equal(bits(r.ess), bits(r.ess_r)), label    # marginal_reduce's bits
    log_p, ess, lw, keep = weigh64(r.z1.numpy(), r.p0.numpy(), K, r.log_det, r.min_weight)
    size = (r.z1.double() ** 2).sum(1).numpy() + (r.p0.double() ** 2).sum(-1).reshape(-1).numpy() + 1.0
    assert r.lw.dtype == torch.float64 and (np.abs(r.lw.numpy() - lw) <= 1e-14 * size).all(), label       # double rounding
    wn, bad = weights64(lw, K)
    # (the inputs: no weight on a threshold above 0 -- at 0 the rule is wn > 0, and none of these underflows)
    assert not bad.any() and (wn > 0).all() and (r.min_weight == 0.0 or (np.abs(wn - r.min_weight) > 1e-9).all()), label
    assert r.keep.dtype == torch.int32 and (r.keep.numpy() == keep).all(), label
    assert K == 1 or r.min_weight == 0.0 or 0 < int(keep.sum()) < keep.size, label                        # some rows are skipped
    ref_x, ref_c = grad_reduce64(r.lw.numpy(), r.full_of.numpy(), np.nan_to_num(r.gz.numpy()),
                                 None if r.gc is None else r.gc.numpy(), K, r.scale.numpy(),
                                 None if r.cscale is None else r.cscale.numpy())
    assert bool(torch.isfinite(r.gx).all()) and ulps(r.gx.numpy(), ref_x) <= 1.0, (label, ulps(r.gx.numpy(), ref_x))
    assert torch.equal(bits(r.gx), bits(r.gx2)), label                             # poisoned full rows = compacted rows
    assert (r.gcond is None) == (r.gc is None)
    if r.gc is not None:
        assert bool(torch.isfinite(r.gcond).all()) and ulps(r.gcond.numpy(), ref_c) <= 1.0, (label, ulps(r.gcond.numpy(), ref_c))
        assert torch.equal(bits(r.gcond), bits(r.gcond2)), label
