"""Reference for the gradient of the noisy-observation log-density (``log_prob_noisy_grad``; csrc/ff_observe.hip: ff_observe_keep,
ff_observe_grad_reduce): ``tests/_logp_grad_ref.LogDensity.value`` on the K expanded rows of every point, composed with
``torch.logsumexp(...) - log K``, and ``torch.autograd.grad`` of the sum with respect to ``x``, the raw ``cond`` and ``noise_std``
(per object and dimension).  The draws are the counter-based stream's (tests/_philox.py) under the noise indices
FF_OBS_NOISE_BASE + k, and the rows are ``x - noise_std z`` rounded through fp32 exactly as ``observe::perturb`` rounds them
(the product, then the difference): the rounding is a constant added to the differentiable ``x - noise_std z``, so the float64
reference is evaluated at the very rows the device expands.  float64 is the truth; float32 gives a case's floor.

Also here: the front-end cases shared by tests/test_observe_grad_host.py (their conditions, on the CPU) and
tests/test_gpu_observe_grad.py (the device against them), and the float64 numpy restatement of the two kernels.
"""
from __future__ import annotations

import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from flowfusion_amd import _native
from flowfusion_amd import diffusion as Dm
from tests import _logp_grad_ref as LG
from tests import _pushforward_ref as R
from tests._philox import normals

STEPS = 3                       # rk4 steps: the grid at which a VP model's fp32 floor is small (tests/test_gpu_logp_grad.py)
SEED, OFFSET = 2027, 5          # the noise draws' key: a non-zero first global row


def draws(seed, sample_offset, B, D, K):
    """z [B, K, D] float32: draw k of global row sample_offset + r."""
    z = normals(seed, sample_offset, B, D, [_native.OBS_NOISE_BASE + k for k in range(K)])
    return torch.from_numpy(np.ascontiguousarray(z.transpose(1, 0, 2)))


def std_rows(noise_std, B, D):
    """``noise_std`` (a scalar, [D] or [B, D]) as a [B, D] float32 tensor."""
    return torch.as_tensor(noise_std, dtype=torch.float32).expand(B, D).contiguous()


def noisy_reference(ld: LG.LogDensity, x, noise_std, cond, K, seed, sample_offset, probes, weight):
    """The reference of one call in ``ld``'s dtype: ``log_p`` [B], ``gx`` [B, D], ``gc`` [B, C] or None, ``gs`` [B, D] (the
    gradient with respect to noise_std per object and dimension), ``ess`` [B] -- and what the deliberately wrong references are
    made of: ``lp`` [B, K], the normalised weights ``wn`` [B, K], the rows' own gradients ``g`` [B, K, D] / ``h`` [B, K, C] and
    the draws ``z`` [B, K, D].  ``probes`` [B K, P, D]: those of the expanded rows; ``weight``: of each probe's integral."""
    m = ld.m
    B, D = x.shape
    z32 = draws(seed, sample_offset, B, D, K)
    s32 = std_rows(noise_std, B, D)
    y32 = x.to(torch.float32)[:, None, :] - s32[:, None, :] * z32            # two fp32 roundings: observe::perturb
    xv, sv, z = m.cast(x).clone().requires_grad_(True), m.cast(s32).clone().requires_grad_(True), m.cast(z32)
    cv = None if cond is None else m.cast(cond).clone().requires_grad_(True)
    with torch.enable_grad():
        y = xv[:, None, :] - sv[:, None, :] * z
        y = (y + (m.cast(y32) - y).detach()).reshape(B * K, D)
        crow = None if cv is None else cv.repeat_interleave(K, dim=0)
        lp = ld.value(y, crow, m.cast(probes), weight).view(B, K)
        L = torch.logsumexp(lp, dim=1) - math.log(K)
        rows = torch.autograd.grad(lp.sum(), (y,) if crow is None else (y, crow), retain_graph=True)
        g = torch.autograd.grad(L.sum(), (xv, sv) if cv is None else (xv, sv, cv))
    wn = torch.softmax(lp.detach(), dim=1)
    return SimpleNamespace(log_p=L.detach(), gx=g[0], gs=g[1], gc=None if cv is None else g[2], ess=1.0 / (wn ** 2).sum(dim=1),
                           lp=lp.detach(), wn=wn, g=rows[0].view(B, K, D), h=None if cv is None else rows[1].view(B, K, -1), z=z)


# ---- the front-end cases -------------------------------------------------------------------------------------------------------
# B = 24 points, three rk4 steps.  ``wrap``: None (the model itself), "pop" / "popc" (the population wrappers around the score
# model, with the affine of ``affine_of(D)``).  ``P``: Hutchinson probes per row (0: the exact trace).  ``std``: the scale of the
# error bars (``case_inputs``), one for all points or one per point, at which every point's effective sample size lies in
# [1.5, K - 0.5] -- found on the CPU in float64 by a scan over scales (tests/test_observe_grad_host.py asserts the outcome) and
# written here as literals, like the gains.  The score models' log-densities are broad (|grad| ~ 0.3): their weights spread
# only under error bars of several units; a Hutchinson model's weights also carry the probes' noise, whatever the error bars.
Case = namedtuple("Case", "name kind wrap D C width gain K P std")
B = 24
CASES = [
    Case("vp_hutch", "vp", None, 16, 0, (128, 128), 1.5, 8, 1, 0.3),
    Case("ve_exact", "ve", None, 5, 3, (128, 128), 2.0, 4, 0,
         (5.3, 2.7, 5.3, 5.3, 3.8, 2.7, 7.4, 3.8, 3.8, 2.7, 8.5, 3.8, 3.2, 7.4, 2.7, 3.8, 7.4, 5.3, 5.3, 2.7, 3.8, 5.3, 5.3, 5.3)),
    Case("cflow_hutch3", "flow", None, 8, 2, (128, 64, 96), 6.0, 16, 3, 0.03),
    Case("pop_hutch", "vp", "pop", 4, 0, (128, 128), 1.0, 4, 1,
         (4.4, 6.2, 12.1, 6.2, 12.1, 3.2, 6.2, 3.2, 6.2, 12.1, 4.4, 12.1, 3.2, 12.1, 4.4, 6.2, 6.2, 17.0, 2.3, 12.1, 6.2, 8.7, 12.1,
          4.4)),
    Case("popc_exact", "vp", "popc", 4, 3, (128, 128), 2.0, 4, 0,
         (7.4, 10.3, 10.3, 10.3, 10.3, 3.8, 10.3, 10.3, 7.4, 10.3, 7.4, 10.3, 3.8, 7.4, 10.3, 3.8, 10.3, 14.5, 5.3, 7.4, 10.3, 5.3,
          10.3, 7.4)),
]
# the cut-off case of ``min_weight``: error bars wide enough that most draws of most points carry no weight
CUT_CASE = CASES[2]._replace(name="cflow_cut", std=0.3)
CUT = 1e-3


def case_front(case):
    """(front end on the CPU, {dtype: LogDensity}, the options of the three-step grid)."""
    from tests.test_gpu_pushforward import affine_of, make_front, options_of
    front, ref_kw = make_front(case.kind, case.D, case.C, list(case.width), len(case.width), gain=case.gain)
    opts = options_of(front, "to_base", STEPS)
    if case.wrap is not None:
        shift, scale = affine_of(case.D)
        ref_kw = dict(ref_kw, affine=(shift, scale))
        if case.wrap == "pop":
            front = Dm.PopulationModelDiffusion(model=front.model, sde=front.sde, shift=shift, scale=scale, method="rk4",
                                                hutchinson=case.P > 0).eval()
        else:
            cshift, cscale = torch.linspace(0.2, -0.2, case.C), torch.linspace(0.7, 1.9, case.C)
            ref_kw = dict(ref_kw, cond_affine=(cshift, cscale))
            front = Dm.PopulationModelDiffusionConditional(model=front.model, sde=front.sde, shift=shift, scale=scale,
                                                           conditional_shift=cshift, conditional_scale=cscale, method="rk4").eval()
    elif case.kind != "flow":
        front.hutch = case.P > 0
    refs = {dt: LG.LogDensity(R.SolverMap(direction="to_base", method="rk4", options=opts, dtype=dt, **ref_kw))
            for dt in (torch.float32, torch.float64)}
    return front, refs, opts


def case_inputs(case, seed=83):
    """(x [B, D], noise_std [B, D], cond [B, C] or None): per-object error bars between 0.5 and 1.5 times ``case.std``."""
    g = torch.Generator().manual_seed(seed + 10 * case.D + case.C)
    x = torch.randn(B, case.D, generator=g)
    std = torch.as_tensor(case.std, dtype=torch.float32).expand(B)[:, None] * (0.5 + torch.rand(B, case.D, generator=g))
    c = torch.randn(B, case.C, generator=g) if case.C else None
    return x, std, c


def case_probes(case, device="cpu"):
    """(probes [B K, P, D] of the expanded rows, the weight of each): the counter-based +-1 probes of the value solve of
    ``log_prob_noisy`` (same seed, keyed by the expanded global row), or the D unit probes of the exact trace."""
    rows = B * case.K
    if case.P == 0:
        return torch.eye(case.D).expand(rows, case.D, case.D), 1.0
    return _native.probe_fill(rows, case.P, case.D, SEED, OFFSET * case.K, device).cpu(), 1.0 / case.P


_REFS = {}


def references(case):
    """{dtype: noisy_reference} of a case, computed once and shared."""
    if case not in _REFS:
        _, refs, _ = case_front(case)
        x, std, c = case_inputs(case)
        probes, weight = case_probes(case)
        _REFS[case] = {dt: noisy_reference(refs[dt], x, std, c, case.K, SEED, OFFSET, probes, weight) for dt in refs}
    return _REFS[case]


def call_args(case, front, x, std, c, dev):
    """(positional, keyword) arguments of the case's ``log_prob_noisy_grad`` for tensors moved to ``dev``."""
    to = lambda t: t.detach().to(dev, torch.float32).contiguous()
    args = (to(x), to(std)) + (() if c is None else (to(c),))
    kw = dict(num_draws=case.K, method="rk4", seed=SEED, sample_offset=OFFSET)
    if case.kind == "flow":
        kw["hutchinson"] = case.P > 0
    if case.P > 1:
        kw["num_probes"] = case.P
    return args, kw


# ---- the two kernels restated in float64 numpy ---------------------------------------------------------------------------------
def weights64(lp, K):
    """(normalised weights [B, K] float64 -- NaN rows for degenerate points --, degenerate [B]) of ``lp`` (B K values)."""
    lp = np.asarray(lp, dtype=np.float64).reshape(-1, K)
    bad = ~(lp < np.inf).all(axis=1) | (lp.max(axis=1) == -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(lp - lp.max(axis=1, keepdims=True))
        wn = w / w.sum(axis=1, keepdims=True)
    wn[bad] = np.nan
    return wn, bad


def keep64(lp, K, min_weight):
    wn, bad = weights64(lp, K)
    with np.errstate(invalid="ignore"):
        keep = (wn > 0) & (wn >= min_weight)
    keep[bad] = False
    return keep.reshape(-1).astype(np.int32)


def row_of(keep):
    """The order-preserving compaction the front end forms: the rank of every kept row, -1 elsewhere (int32)."""
    keep = torch.as_tensor(keep, dtype=torch.int32)
    return torch.where(keep > 0, torch.cumsum(keep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)


def grad_reduce64(lp, rows, gx_rows, gc_rows, K, z):
    """(grad_x, grad_c or None, grad_noise_std) in float64 from the kept rows' gradients; ``rows`` = row_of [B K], ``z``
    [B, K, D].  Degenerate points are NaN."""
    wn, bad = weights64(lp, K)
    Bn = wn.shape[0]
    rows = np.asarray(rows).reshape(Bn, K)
    pick = lambda t: np.where((rows >= 0)[..., None], np.asarray(t, dtype=np.float64)[np.maximum(rows, 0)], 0.0)
    w = np.where(rows >= 0, wn, 0.0)[..., None]
    gx = pick(gx_rows)
    out = [(w * gx).sum(axis=1), None if gc_rows is None else (w * pick(gc_rows)).sum(axis=1),
           -(w * np.asarray(z, dtype=np.float64) * gx).sum(axis=1)]
    for t in out:
        if t is not None:
            t[bad] = np.nan
    return out
