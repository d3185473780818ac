"""Reference for the noisy-observation marginal of the symplectic flows (``SymplecticFlowModel.log_prob_marginal_noisy`` /
``log_prob_marginal_noisy_grad``; csrc/ff_marginal_observe.hip: ff_marginal_observe_expand, ff_marginal_observe_grad_reduce).

The estimate: ``tests/_leapfrog_pull_ref.logp_map`` on each of the K joint draws of every point -- row k starts at ``x - sigma z_k``
with momentum ``p_k`` -- stacked, composed with ``torch.logsumexp(...) - log K`` (``logp_map`` carries ``- sum log scale``), and
``torch.autograd.grad`` of the sum with respect to ``x``, the raw ``conditional`` and ``sigma``.  float64 is the truth; float32
gives a case's floor.  The draws are an INPUT: the tests hand over the ones the code under test used -- on a device
``_native.normal_fill`` under the noise indices OBS_NOISE_BASE + k and MOMENTUM_NOISE_BASE + k, on the CPU (``normal_fill`` has no
host path) the host twins' own: ``-observe_expand(0, 1)`` and ``marginal_expand``'s momentum half.

Also here: the front-end cases shared by tests/test_marginal_observe_host.py (their conditions, on the CPU) and
tests/test_gpu_marginal_observe.py (the device against them), and the two kernels' cells with their float64 numpy restatement.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from flowfusion_amd import _native
from tests import _leapfrog_pull_ref as L
from tests import _marginal_grad_ref as M
from tests._observe_grad_ref import row_of, weights64  # noqa: F401

SEED, OFFSET = M.SEED, M.OFFSET
KS = (2, 4)
CASES = [(case, K) for case in L.LOGP_CASES for K in KS]
# sigma of a front-end case: SIGMA[case] * (0.5 + u[B, D]), u seeded uniforms -- per object and dimension.  The literals come from
# a float64 scan on the CPU over 0.1, 0.2, 0.3, 0.5, 0.8 (scratch/marginal_observe_sigma_scan.py; CHANGELOG.md has the margins):
# every condition of tests/test_marginal_observe_host.py holds at all five; 0.2 keeps every floor below 1e-5 (at 0.1 one is 3e-5)
# while the K weights of a point are still spread (from 0.3 up nearly all the weight sits on one draw).
SIGMA = {L.front_id(L.LOGP_CASES[0]): 0.2, L.front_id(L.LOGP_CASES[1]): 0.2, L.front_id(L.LOGP_CASES[2]): 0.2}
# the min_weight > 0 case, as tests/_marginal_grad_ref.py: the literal from a float64 scan of that case's normalised weights
CUT_CASE, CUT_K, CUT = L.LOGP_CASES[0], 4, 0.19
GUARD, MAGIC = 64, 12345.6789


def case_id(ck):
    return f"{L.front_id(ck[0])}-K{ck[1]}"


def sigma_of(case, sigma=None):
    """noise_std [B, D] float32 of a front-end case, seeded."""
    D, B = case[0], case[5]
    s = SIGMA[L.front_id(case)] if sigma is None else sigma
    u = torch.rand(B, D, generator=torch.Generator().manual_seed(97))
    return (s * (0.5 + u)).to(torch.float32)


def draws(B, D, K, dev="cpu", seed=SEED, sample_offset=OFFSET):
    """(z [B, K, D], p [B, K, D]) float32 on the CPU: the noise and the momenta of the stream as ``dev`` computes them."""
    if torch.device(dev).type == "cuda":
        fill = lambda base: torch.stack([_native.normal_fill(B, D, seed, sample_offset, dev, noise_index=base + k)
                                         for k in range(K)], dim=1).cpu()
        return fill(_native.OBS_NOISE_BASE), fill(_native.MOMENTUM_NOISE_BASE)
    y, _ = _native.observe_expand(torch.zeros(B, D), torch.ones(D), K, seed, sample_offset)
    p, _ = _native.marginal_expand(torch.zeros(B, D), K, seed, sample_offset)
    return (-y).view(B, K, D).contiguous(), p.view(B, K, 2 * D)[:, :, D:].contiguous()


def noisy_reference(front, x, std, z, p0, cond, num_steps, dtype=torch.float64):
    """The reference of one call in ``dtype``: ``log_p`` [B], ``gx`` [B, D], ``gc`` [B, C] or None, ``gs`` [B, D], ``ess`` [B] -- and
    what the damaged references are made of: ``lw``, ``wn`` [B, K], the rows' own gradients ``g`` [B, K, D] (with respect to the
    row's start ``x - sigma z_k``) / ``h`` [B, K, C], and the draws ``z``, ``p``."""
    f = L.logp_map(front, dtype)
    K = int(z.shape[1])
    leaf = lambda t: None if t is None else t.detach().to("cpu", dtype).clone().requires_grad_(True)
    xv, sv, cv = leaf(x), leaf(std), leaf(cond)
    zk, pk = z.detach().to("cpu", dtype), p0.detach().to("cpu", dtype)
    wrt = (xv, sv) if cv is None else (xv, sv, cv)
    with torch.enable_grad():
        lw = torch.stack([f(xv - sv * zk[:, k], pk[:, k], cv, num_steps) for k in range(K)], dim=1)
        Lm = torch.logsumexp(lw, dim=1) - math.log(K)
        rows = [torch.autograd.grad(lw[:, k].sum(), wrt, retain_graph=True) for k in range(K)]
        g = torch.autograd.grad(Lm.sum(), wrt)
    wn = torch.softmax(lw.detach(), dim=1)
    return SimpleNamespace(log_p=Lm.detach(), gx=g[0], gs=g[1], gc=None if cv is None else g[2], ess=1.0 / (wn ** 2).sum(dim=1),
                           lw=lw.detach(), wn=wn, g=torch.stack([r[0] for r in rows], dim=1),
                           h=None if cv is None else torch.stack([r[2] for r in rows], dim=1), z=zk, p=pk)


def weighted(ref, weights, zed="z"):
    """(gx, gc or None, gs) of a reference under other weights [B, K] and another factor in d / d sigma: ``zed`` = "z" (the
    noise), "p" (the draws of the momentum index) or None (dropped)."""
    w = weights.to(ref.g.dtype)[..., None]
    fac = 1.0 if zed is None else getattr(ref, zed)
    return (w * ref.g).sum(1), (None if ref.h is None else (w * ref.h).sum(1)), -(w * fac * ref.g).sum(1)


_REFS = {}


def case_inputs(case):
    """(front on the CPU, x, noise_std [B, D], raw conditional or None) of a front-end case."""
    front, _, x, _, _, cond = L.front_inputs(case)
    return front, x, sigma_of(case), cond


def references(ck, dev="cpu", sigma=None):
    """{dtype: noisy_reference} of a front-end case with the draws of ``dev``, computed once and shared."""
    key = (case_id(ck), str(dev), sigma)
    if key not in _REFS:
        case, K = ck
        front, x, _, cond = case_inputs(case)
        z, p = draws(x.shape[0], x.shape[1], K, dev)
        _REFS[key] = {dt: noisy_reference(front, x, sigma_of(case, sigma), z, p, cond, case[4], dt)
                      for dt in (torch.float32, torch.float64)}
    return _REFS[key]


def floors(r32, r64):
    """{what: fp32 floor} of a case, ``what`` in gx / gs / gc (where the model has a conditional): the project's metric."""
    from tests.test_gpu_pushforward import fp32_floor
    out = {"gx": fp32_floor(r32.gx, r64.gx), "gs": fp32_floor(r32.gs, r64.gs)}
    if r64.gc is not None:
        out["gc"] = fp32_floor(r32.gc, r64.gc)
    return out


# ---- the kernels' cells -----------------------------------------------------------------------------------------------------------
bits = M.bits


def guarded(shape, dev, dtype=torch.float32, offset=0):
    """(view, whole): a contiguous ``shape`` tensor inside a buffer of MAGIC with GUARD words on either side, its first element
    ``offset`` elements past the guard."""
    n = int(np.prod(shape))
    whole = torch.full((2 * GUARD + n + offset,), MAGIC, dtype=dtype, device=dev)
    return whole[GUARD + offset:GUARD + offset + n].view(*shape), whole


def guards_intact(whole, view):
    n, start = view.numel(), view.storage_offset()
    w = whole.cpu()
    return bool((w[:start] == w[0]).all() and (w[start + n:] == w[0]).all() and float(w[0]) == float(torch.tensor(MAGIC)))


def shifted(t, dev):
    """``t`` on ``dev`` at an address one float past a 16-byte boundary: the vector body cannot take it."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    flat[1:] = t.reshape(-1).to(dev)
    return flat[1:].view(t.shape)


def expand_inputs(D, K, B, C, layout):
    g = torch.Generator().manual_seed(11 + 100 * D + K + B)
    x = torch.randn(B, D, generator=g)
    std = 0.05 + torch.rand(B, D, generator=g)
    if layout == "D":
        std = std[0].clone()
    shift, scale = torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
    cond = torch.randn(B, C, generator=g) if C else None
    return x, std, shift, scale, cond


def raw_expand(dev, x, std, shift, scale, cond, K, seed=SEED, sample_offset=OFFSET, offset=0):
    """ff_marginal_observe_expand(_host) through ctypes into guarded outputs (``offset``: x and z0 one float off alignment).
    Returns (z0, cond_out or None) on the CPU after checking the guards."""
    B, D = x.shape
    C = 0 if cond is None else cond.shape[1]
    to = lambda t: None if t is None else (shifted(t, dev) if offset else t.to(dev).contiguous())
    xd, sd, hd, cd, nd = to(x), std.to(dev).contiguous(), shift.to(dev), scale.to(dev), to(cond)
    z0, z0w = guarded((B * K, 2 * D), dev, offset=offset)
    co, cow = guarded((B * K, max(C, 1)), dev)
    p = lambda t: 0 if t is None else t.data_ptr()
    Lb = _native.lib()
    rc = _native._on_stream(torch.device(dev), Lb.ff_marginal_observe_expand, Lb.ff_marginal_observe_expand_host,
                            (p(xd), p(sd), 0 if std.dim() == 1 else D, p(hd), p(cd), p(nd), B, D, C, K, seed, sample_offset,
                             p(z0), p(co) if C else 0))
    assert rc == _native.FF_OK
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert guards_intact(z0w, z0) and guards_intact(cow, co)
    assert C > 0 or bool((co.cpu() == torch.tensor(MAGIC)).all())
    return z0.cpu().clone(), (co.cpu().clone() if C else None)


def check_expand(dev, D, K, B, C, layout="BD", offset=0):
    """The three bitwise contracts of the expand kernel on one cell (either side), guards included."""
    x, std, shift, scale, cond = expand_inputs(D, K, B, C, layout)
    to = lambda t: None if t is None else t.to(dev).contiguous()
    z0, co = raw_expand(dev, x, std, shift, scale, cond, K, offset=offset)
    y, _ = _native.observe_expand(to(x), to(std), K, SEED, OFFSET)
    via, _ = _native.marginal_expand(y, 1, SEED, OFFSET, to(shift), to(scale))
    plain, pc = _native.marginal_expand(to(x), K, SEED, OFFSET, to(shift), to(scale), to(cond))
    assert torch.equal(bits(z0[:, :D]), bits(via.cpu()[:, :D])), "q half"
    assert torch.equal(bits(z0[:, D:]), bits(plain.cpu()[:, D:])), "p half"
    assert (co is None and pc is None) or torch.equal(bits(co), bits(pc.cpu())), "cond_out"
    zero, _ = raw_expand(dev, x, torch.zeros_like(std), shift, scale, cond, K, offset=offset)
    assert torch.equal(bits(zero), bits(plain.cpu())), "noise_std = 0"
    # the binding gives the same bits
    bz, bc = _native.marginal_observe_expand(to(x), to(std), K, SEED, OFFSET, to(shift), to(scale), to(cond))
    assert torch.equal(bits(bz.cpu()), bits(z0)) and (bc is None or torch.equal(bits(bc.cpu()), bits(co)))
    return z0


def noise_grad64(lw, rows, gz_rows, z, K, scale=None):
    """grad_noise_std [B, D] in float64: -(sum_kept wn_k z_k g_q,k) / scale; ``z`` [B, K, D].  Degenerate points are NaN."""
    wn, bad = weights64(lw, K)
    Bn = wn.shape[0]
    rows = np.asarray(rows).reshape(Bn, K)
    g = np.asarray(gz_rows, dtype=np.float64)
    D = g.shape[1] // 2
    g = g[:, :D] if g.shape[0] else np.zeros((1, D))
    picked = np.where((rows >= 0)[..., None], g[np.maximum(rows, 0)], 0.0)
    w = np.where(rows >= 0, wn, 0.0)[..., None]
    gs = -(w * np.asarray(z, dtype=np.float64) * picked).sum(axis=1)
    if scale is not None:
        gs = gs / np.asarray(scale, dtype=np.float64)
    gs[bad] = np.nan
    return gs


def run_reduce(dev, D, K, B, C, min_weight=M.MIN_WEIGHT, z1=None, keep_mode="partial", offset=0, std_layout="BD"):
    """ff_marginal_observe_grad_reduce on ``dev`` on the synthetic inputs of a cell of tests/_marginal_grad_ref.py, beside
    ff_marginal_grad_reduce on the same inputs: every row that was not kept POISONED with NaN (row_of = the row itself where
    kept), once more on the compacted rows, and once without grad_noise_std.  ``keep_mode``: "partial" (what ff_marginal_weigh
    keeps at ``min_weight``), "full" or "empty".  Outputs sit between guard words; ``offset`` = 1 puts the rows one float off
    alignment.  Everything comes back on the CPU."""
    zs, gz, gc, scale, cscale = M.kernel_inputs(D, K, B, C)
    z1 = zs if z1 is None else z1
    to = lambda t: None if t is None else t.to(dev)
    rows_to = lambda t: None if t is None else (shifted(t, dev) if offset else t.to(dev).contiguous())
    z, _ = draws(B, D, K, dev)
    _, lw, keep = _native.marginal_weigh(to(z1), K, SEED, OFFSET, 0.375, min_weight)
    keep = keep.cpu()
    if keep_mode == "full":
        keep = torch.ones_like(keep)
    elif keep_mode == "empty":
        keep = torch.zeros_like(keep)
    kept = keep > 0
    full_of = torch.where(kept, torch.arange(B * K, dtype=torch.int32), -1).to(torch.int32)
    gzp, gcp = gz.clone(), (None if gc is None else gc.clone())
    gzp[~kept] = float("nan")
    if gcp is not None:
        gcp[~kept] = float("nan")
    std = torch.full((B, D) if std_layout == "BD" else (D,), float("nan"))      # (its values are not read)
    outs = lambda: (guarded((B, D), dev), guarded((B, max(C, 1)), dev), guarded((B, D), dev))
    (gx, gxw), (gcd, gcw), (gs, gsw) = outs()
    _native.marginal_observe_grad_reduce(lw, to(full_of), rows_to(gzp), rows_to(gcp), to(std), K, SEED, OFFSET, to(scale),
                                         to(cscale), True, gx, gcd if C else None, gs)
    (gx2, gx2w), (gcd2, gc2w), (gs2, gs2w) = outs()
    rows = torch.nonzero(kept).view(-1)
    _native.marginal_observe_grad_reduce(lw, to(row_of(keep)), rows_to(gz[rows].contiguous()),
                                         None if gc is None else rows_to(gc[rows].contiguous()), to(std), K, SEED, OFFSET,
                                         to(scale), to(cscale), True, gx2, gcd2 if C else None, gs2)
    (gx3, gx3w), (gcd3, gc3w), (gs3, gs3w) = outs()
    r3 = _native.marginal_observe_grad_reduce(lw, to(full_of), rows_to(gzp), rows_to(gcp), to(std), K, SEED, OFFSET, to(scale),
                                              to(cscale), False, gx3, gcd3 if C else None)
    assert r3[2] is None
    px, pc = _native.marginal_grad_reduce(lw, to(full_of), rows_to(gzp), rows_to(gcp), K, to(scale), to(cscale))
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    for view, whole in ((gx, gxw), (gcd, gcw), (gs, gsw), (gx2, gx2w), (gcd2, gc2w), (gs2, gs2w), (gx3, gx3w), (gcd3, gc3w),
                        (gs3, gs3w)):
        assert guards_intact(whole, view)
    magic = torch.tensor(MAGIC)
    assert bool((gs3.cpu() == magic).all()) and (C > 0 or bool((gcd.cpu() == magic).all()))      # what was not asked is not written
    cpu = lambda t: None if t is None else t.cpu().clone()
    cc = lambda t: cpu(t) if C else None
    return SimpleNamespace(z=z, gz=gz, gc=gc, scale=scale, cscale=cscale, lw=cpu(lw), keep=keep, full_of=full_of,
                           gx=cpu(gx), gcond=cc(gcd), gs=cpu(gs), gx2=cpu(gx2), gcond2=cc(gcd2), gs2=cpu(gs2),
                           gx3=cpu(gx3), gcond3=cc(gcd3), px=cpu(px), pc=cpu(pc))


def check_reduce(r, K, label=""):
    """What every cell asserts of ``run_reduce``'s results, on either side."""
    same = lambda a, b: (a is None and b is None) or torch.equal(bits(a), bits(b))
    # grad_x and grad_c: ff_marginal_grad_reduce's bits, with and without grad_noise_std; poisoned full rows = compacted rows
    assert same(r.gx, r.px) and same(r.gcond, r.pc), label
    assert same(r.gx3, r.px) and same(r.gcond3, r.pc), label
    assert same(r.gx2, r.gx) and same(r.gcond2, r.gcond) and same(r.gs2, r.gs), label
    ref_x, ref_c = M.grad_reduce64(r.lw.numpy(), r.full_of.numpy(), np.nan_to_num(r.gz.numpy()),
                                   None if r.gc is None else r.gc.numpy(), K, r.scale.numpy(),
                                   None if r.cscale is None else r.cscale.numpy())
    ref_s = noise_grad64(r.lw.numpy(), r.full_of.numpy(), np.nan_to_num(r.gz.numpy()), r.z.numpy(), K, r.scale.numpy())
    assert M.ulps(r.gx.numpy(), ref_x) <= 1.0, (label, M.ulps(r.gx.numpy(), ref_x))
    assert M.ulps(r.gs.numpy(), ref_s) <= 1.0, (label, M.ulps(r.gs.numpy(), ref_s))
    if r.gc is not None:
        assert M.ulps(r.gcond.numpy(), ref_c) <= 1.0, (label, M.ulps(r.gcond.numpy(), ref_c))
    if not bool((r.keep > 0).any()):
        assert bool((r.gx == 0).all() and (r.gs == 0).all()), label                 # nothing kept: a sum of nothing
