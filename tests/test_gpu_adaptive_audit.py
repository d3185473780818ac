"""GPU tier: an independent audit of every attempted step of the device-resident adaptive solver (csrc/ff_adaptive.hip).

"Device controller == host controller" (tests/test_gpu_device_adaptive.py) cannot see an error in the scaled-RMS reduction:
both controllers run it (csrc/ff_norm.h).  And the oracle comparisons run at the solver tolerance, which a norm that loses
a few elements still meets.  Here ``device_adaptive.TRACE`` / ``TRACE_STATE`` hand out, after every attempted step, host
clones of the solver's work buffers, and the test recomputes from them in float64 with plain torch -- the library is never
called for the expected side:

* the error ratio the controller acted on (``adapt_control_kernel``);
* its decision, and the accepted-step count;
* what ``adapt_commit_kernel`` left in (y, f0, lp, fl0) after an accepted step and after a rejection, bit for bit;
* the sum of the unit-tangent passes' divergences (``adapt_sum_kernel``), bit for bit;
* the dense output at t_end (``adapt_finish_kernel``) against torchdiffeq's `_interp_fit` / `_interp_evaluate` polynomial.

With TRACE set there is one attempt per chunk: entry k - 1 holds the state attempt k started from, entry k its proposal.
"""
import pytest
import torch

from flowfusion_amd import device_adaptive
from flowfusion_amd import diffusion as Dm

DEV = "cuda"
pytestmark = pytest.mark.gpu

S = 2048 * 256              # 16-byte elements one trip of the capped grids covers (copy_grid, the norm's grid)
RMS_BAR = 2e-6              # relative: the scaled-RMS kernel against float64 (fp32 quotients, about 3 x 2^-24 each; double sums)
FIT_EVAL_OPS = 39           # fp32 operations of fit_eval (ff_adaptive.hip): a 8, b 10, c 9, d 1, the Horner-free sum 11


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _model(D, C, hutch):
    torch.manual_seed(77)
    mlp = Dm.MLP(n_dimensions=D, n_conditionals=C, embedding_dimensions=8, units=[64, 64])
    return Dm.ScoreModel(mlp, Dm.VESDE(), no_sigma=False, hutchinson=hutch).eval().to(DEV)


def _traced(run, state=True, first=None):
    device_adaptive.TRACE, device_adaptive.TRACE_STATE, device_adaptive.TRACE_STATE_FIRST = [], state, first
    try:
        run()
        return device_adaptive.TRACE
    finally:
        device_adaptive.TRACE, device_adaptive.TRACE_STATE, device_adaptive.TRACE_STATE_FIRST = None, False, None


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rms64(err, y0, y1, atol, rtol):
    scale = atol + rtol * torch.max(y0.double().abs(), y1.double().abs())
    return float((err.double() / scale).pow(2).mean().sqrt())


def _fit_eval64(y0, y1, ym, f0, f1, dt, x):
    """torchdiffeq `_interp_fit` + `_interp_evaluate` in float64, and the sum of the absolute values of the polynomial's
    terms (every product of a coefficient, a power of x and an input that the expanded polynomial adds up)."""
    y0, y1, ym, f0, f1 = (t.double() for t in (y0, y1, ym, f0, f1))
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * ym
    b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * ym
    c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * ym
    d = dt * f0
    val = y0 + x * d + x ** 2 * c + x ** 3 * b + x ** 4 * a
    A0, A1, Am, F0, F1 = y0.abs(), y1.abs(), ym.abs(), abs(dt) * f0.abs(), abs(dt) * f1.abs()
    mag = (A0 + abs(x) * F0
           + abs(x) ** 2 * (F1 + 4 * F0 + 11 * A0 + 5 * A1 + 16 * Am)
           + abs(x) ** 3 * (5 * F0 + 3 * F1 + 18 * A0 + 14 * A1 + 32 * Am)
           + abs(x) ** 4 * (2 * F1 + 2 * F0 + 8 * A1 + 8 * A0 + 16 * Am))
    return val, mag


def _audit(trace, y_start, lp_start, atol, rtol, has_lp):
    """Every check the clones of `trace` allow; returns what was covered."""
    seen = dict(ratios=0, accepted_commits=0, rejections=0, pass_sums=0, finish=0)
    assert len(trace) >= 3 and trace[-1][-1] is not None and trace[-1][-1]["done"] == 1
    assert all(e[-1] is None or e[-1]["done"] == 0 for e in trace[:-1])
    atol32, rtol32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (atol, rtol))       # ff_adapt_config keeps them in fp32
    for k, entry in enumerate(trace):
        n_att, n_acc, t, dt, ratio = entry[:5]
        cur = entry[-1]
        assert n_att == k + 1
        acc_before = trace[k - 1][1] if k else 0
        moved = n_acc - acc_before
        assert moved in (0, 1)
        # (nothing non-finite, no min_step / max_step in these runs: the decision is the ratio's alone)
        assert moved == int(ratio <= 1.0), (k, ratio, moved)
        if cur is None:
            continue
        # ---- the sum of the unit-tangent passes, in pass order, in fp32 ---------------------------------------------
        if "aux_lp_pass" in cur:
            part = cur["aux_lp_pass"]
            assert part.shape[0] >= 2
            for j in range(4):
                s = part[0, j].clone()
                for p in range(1, part.shape[0]):
                    s = s + part[p, j]
                assert _same_bits(s, cur["aux_lp"][j]), (k, j)
            seen["pass_sums"] += 1
        prev = trace[k - 1][-1] if k else dict(y=y_start, lp=lp_start)
        if prev is None:
            continue
        # ---- the error ratio: max over the state and the log-density of rms(err / (atol + rtol max(|y0|, |y1|))) ----
        y0 = prev["y"]
        exp = _rms64(cur["aux"][3], y0, cur["aux"][0], atol32, rtol32)
        if has_lp:
            exp = max(exp, _rms64(cur["aux_lp"][3], prev["lp"], cur["aux_lp"][0], atol32, rtol32))
        assert abs(ratio - exp) <= RMS_BAR * abs(exp), (k, ratio, exp)
        if abs(exp - 1.0) > RMS_BAR:                          # (closer to 1 than the bar, float64 cannot say which side fp32 fell on)
            assert moved == int(exp <= 1.0), (k, exp, moved)
        seen["ratios"] += 1
        # ---- the commit ---------------------------------------------------------------------------------------------
        names = [("y", "aux", 0), ("f0", "aux", 1)] + ([("lp", "aux_lp", 0), ("fl0", "aux_lp", 1)] if has_lp else [])
        assert cur["commit"] == int(moved == 1 and not cur["done"])
        if cur["commit"]:
            for dst, src, j in names:
                assert _same_bits(cur[dst], cur[src][j]), (k, dst)
            seen["accepted_commits"] += 1
        elif k:                                               # rejected, or accepted and finished: the buffers keep entry k - 1's
            for dst, _, _ in names:
                assert _same_bits(cur[dst], prev[dst]), (k, dst)
            seen["rejections"] += int(moved == 0)
    # ---- the dense output at t_end ----------------------------------------------------------------------------------
    last = trace[-1][-1]
    t_now = trace[-1][2]
    x = float(torch.tensor((last["t_end"] - last["t_prev"]) / (t_now - last["t_prev"]), dtype=torch.float64).float())
    dt = float(torch.tensor(last["dt_prev"], dtype=torch.float64).float())      # the kernel's inputs: both rounded to fp32
    assert 0.0 < x <= 1.0
    outs = [("out_y", last["y"], last["aux"][0], last["aux"][2], last["f0"], last["aux"][1])]
    if has_lp:
        outs.append(("out_lp", last["lp"], last["aux_lp"][0], last["aux_lp"][2], last["fl0"], last["aux_lp"][1]))
    for name, y0, y1, ym, f0, f1 in outs:
        val, mag = _fit_eval64(y0, y1, ym, f0, f1, dt, x)
        got = last[name].reshape(-1).double()
        # derived: each of fit_eval's N = 39 fp32 operations rounds a partial result that is at most the sum of the absolute
        # values of the terms it holds (times 1 + O(N 2^-24)): the error is at most N 2^-24 (1 + ..) sum |terms| < N 2^-23 sum
        bar = 2.0 ** -23 * FIT_EVAL_OPS * mag
        ok = (got - val).abs() <= bar
        assert bool(ok.all()), (name, int((~ok).nonzero()[0]), float((got - val).abs().max()))
        seen["finish"] += 1
    return seen


CASES = {
    # name: (D, B, what, options, TRACE_STATE_FIRST)
    "single_block_state_only": (5, 300, "sample", None, None),
    "single_block_with_log_density": (5, 300, "hutch", None, None),
    "several_blocks_below_the_cap": (5, 3000, "sample", None, None),
    "above_one_trip": (5, 419_433, "sample", None, 3),
    "exact_trace_several_passes": (8, 77, "exact", None, None),
    "forced_rejection": (5, 300, "hutch", {"first_step": 0.5}, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_attempted_step_against_float64(name):
    """A VE score model, C = 2, [64, 64], default tolerances, no min_step / max_step.
    single block: B D = 1500 (the reduction runs without partials); with the Hutchinson log-density a second term of
    n = B; several blocks: B D = 15 000; above one trip: B D = 2 097 165 = 4 (S + 3) + 1, so the norm, the commit and the
    dense output take a second grid-stride trip and a scalar tail (clones of the first three attempts and the last);
    exact trace: 8 dimensions need two unit-tangent passes on this network, B = 77 leaves a tail in every [B] array;
    forced rejection: a first step of half the span, so that the rejection branch of the commit is seen."""
    D, B, what, options, first = CASES[name]
    C = 2
    sm = _model(D, C, what == "hutch")
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, D, device=DEV, generator=g)
    cond = torch.randn(B, C, device=DEV, generator=g)
    atol = rtol = 1e-4
    if what == "sample":
        y_start, lp_start, has_lp = (x * sm.sde.sigma_max).reshape(-1).cpu(), None, False
        run = lambda: sm.sample_ode_from_base(x, conditional=cond, atol=atol, rtol=rtol, options=options)
    else:
        x = x * 0.5
        y_start, lp_start, has_lp = x.reshape(-1).cpu(), torch.zeros(B), True
        torch.manual_seed(9)
        run = lambda: sm.solve_odes_forward(x, conditional=cond, atol=atol, rtol=rtol, options=options)
    trace = _traced(run, True, first)
    assert "chunks" in sm.last_solver_stats and sm.last_solver_stats["attempts"] == len(trace)      # the device loop ran
    if name == "above_one_trip":
        assert B * D == 4 * (S + 3) + 1 and sum(e[-1] is not None for e in trace) == 4
    seen = _audit(trace, y_start, lp_start, atol, rtol, has_lp)
    print(f"{name}: {len(trace)} attempts, {trace[-1][1]} accepted; audited {seen}")
    assert seen["ratios"] >= 2 and seen["accepted_commits"] >= 1 and seen["finish"] == (2 if has_lp else 1)
    if what == "exact":
        assert seen["pass_sums"] >= 3
    if name == "forced_rejection":
        assert seen["rejections"] >= 1


def test_trace_state_is_off_by_default_and_adds_nothing():
    """Without TRACE_STATE a trace entry is what it was: five numbers."""
    assert device_adaptive.TRACE_STATE is False and device_adaptive.TRACE_STATE_FIRST is None and device_adaptive.TRACE is None
    sm = _model(5, 2, False)
    g = torch.Generator(device=DEV).manual_seed(5)
    x, cond = torch.randn(64, 5, device=DEV, generator=g), torch.randn(64, 2, device=DEV, generator=g)
    trace = _traced(lambda: sm.sample_ode_from_base(x, conditional=cond), False)
    assert len(trace) >= 3 and all(len(e) == 5 for e in trace)
