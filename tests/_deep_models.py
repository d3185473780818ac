"""Deep models whose network matters (tests/test_gpu_derivative_depth.py, tests/test_derivative_depth_host.py).

At torch's default initialisation a SiLU stack contracts: max |dNET/dx| of a 16-d model falls from 2.7e-3 at 4 x 256 to 9.5e-11
at 18 x 256 and 2.4e-20 at 36 x 128 (float64, measured: the VP score network of ``make_front``, seed 5, nine standard normal
rows, the middle of the span; a flow's velocity network: 4.4e-3, 1.3e-10, 3.7e-20).  A derivative kernel run on such a model
returns ``a_e seed`` plus rounding whatever it does with the hidden layers, so a deep test on it passes with any stash or ring
bug.  Multiplying the hidden-to-hidden weight matrices by a gain restores the Jacobian -- at 18 x 256: 1.4e-5 at gain 2, 0.10 at
gain 3, 5.4e2 at gain 4 -- and the critical gain depends on depth and width, so every case carries its own, found here on the
CPU in float64 and written into the test file as a literal.

``apply_gain``      the in-place multiply ``make_front`` / ``make_model`` call (gain 1.0 touches nothing);
``net_jacobian``    max |dNET/dx| in float64 over a batch, at one time;
``critical_gain``   bisects for a gain at which that maximum lies in [0.1, 10];
``swap_rows``       a copy of a parameter bundle with two output rows of ONE hidden layer's weight matrix swapped: the damage
                    every case must tell from the truth by at least 100 bars (the host file checks it on the references).
"""
from __future__ import annotations

import copy
import math

import torch

from oracle import flowfusion_oracle as fo

WINDOW = (0.1, 10.0)


def apply_gain(linears, gain):
    """Multiply the hidden-to-hidden weight matrices (every Linear but the first and the last) by ``gain``, in place."""
    if gain == 1.0:
        return
    with torch.no_grad():
        for lin in list(linears)[1:-1]:
            lin.weight.mul_(gain)


def net_function(ref_kw, t):
    """x, cond -> NET(t, x, cond) in float64 of ``make_front``'s reference keywords: the score network itself (not divided by
    sigma) or the flow's velocity network on the RAW conditional."""
    tt = torch.tensor(float(t), dtype=torch.float64)
    if ref_kw["kind"] == "flow":
        o = fo.FlowOracle(ref_kw["params"], dtype=torch.float64)
        return lambda x, c: o.dynamics(tt, x, c)
    p = ref_kw["params"].to(torch.float64)
    return lambda x, c: fo.mlp_forward(p, tt, x, c)


def net_jacobian(ref_kw, x, cond=None, t=0.5):
    """max over the batch and over the entries of |dNET/dx| at time ``t``, float64."""
    f = net_function(ref_kw, t)
    x = x.detach().to(torch.float64)
    c = None if cond is None else cond.detach().to(torch.float64)
    worst = 0.0
    for b in range(x.shape[0]):
        cb = None if c is None else c[b:b + 1]
        J = torch.func.jacfwd(lambda a: f(a[None], cb)[0])(x[b])
        worst = max(worst, float(J.abs().max()))
    return worst


def mid_time(kind):
    """The middle of the span of a model kind: (1 + epsilon) / 2 for the score models, 0.5 for a flow."""
    return 0.5 if kind == "flow" else 0.5 * (1.0 + 1e-3)


def critical_gain(kind, D, C, width, nh, x=None, cond=None, seed=5, lo=1.0, hi=8.0, target=1.0, iters=40):
    """A gain at which max |dNET/dx| of ``make_front(kind, D, C, width, nh, seed=seed, gain=.)`` at the inputs (x, cond) and the
    middle of the span lies in [0.1, 10]: bisection on log(gain) between ``lo`` and ``hi`` for |J| = ``target``, stopped at the
    first iterate within a factor 1.3 of the target (or, failing that, at the last one inside the window) and rounded to three
    decimals -- the literal a case carries.  The deep cases aim at 0.2: past the critical gain the hidden layers amplify
    from layer to layer, fp32 rounding included, and at the low end of the window the fp32 floor of a 17 .. 36 layer case stays
    under the 5e-5 the host file caps it at.  Default inputs: nine standard normal rows, seed 0."""
    from tests.test_gpu_pushforward import make_front
    if x is None:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(9, D, generator=g)
        cond = torch.randn(9, C, generator=g) if C else None
    measure = lambda gain: net_jacobian(make_front(kind, D, C, width, nh, seed=seed, gain=gain)[1], x, cond, mid_time(kind))
    inside = None
    for _ in range(iters):
        mid = round(math.exp(0.5 * (math.log(lo) + math.log(hi))), 3)
        j = measure(mid)
        if WINDOW[0] <= j <= WINDOW[1]:
            inside = mid
            if target / 1.3 <= j <= target * 1.3:
                return mid
        if hi - lo < 2e-3:
            break
        lo, hi = (mid, hi) if j < target else (lo, mid)
    if inside is not None:
        return inside
    raise RuntimeError(f"no gain in [{lo}, {hi}] lands max |J_net| in {WINDOW} for {kind} D={D} C={C} {nh} x {width}")


def swap_rows(params, layer, rows=(0, 1)):
    """A deep copy of an ``MLPParams`` / ``FlowParams`` bundle with output rows ``rows`` of hidden layer ``layer``'s weight
    matrix (``weights[layer]``: the Linear that PRODUCES hidden layer ``layer``) exchanged; the biases stay."""
    out = copy.deepcopy(params)
    w = out.weights[layer]
    i, j = rows
    w[[i, j]] = w[[j, i]]
    return out
