"""GPU tier of ``SymplecticFlowModel.log_prob_marginal_grad`` (csrc/ff_marginal.hip: marginal_weigh_kernel,
marginal_grad_reduce_kernel; ``odeint._leapfrog_pull_from``).

The two kernels on the cells of tests/_marginal_grad_ref.py -- the same checks the host file runs on their host twins: ``log_p``
and ``ess`` bitwise ``marginal_reduce``'s, ``lw`` and ``keep`` against the float64 restatement, the gradients to one fp32 ulp with
every skipped row poisoned, K = 1, degenerate points, the second trip of the grid-stride loop -- and device against host twin,
bitwise, on the same ``lw``.  The method on the three ``LOGP_CASES`` at K = 2 and 4 against float64 autograd through the
logsumexp of the K one-draw log-densities, with the momenta the device drew; its bitwise properties (``log_p`` and ``ess``
against ``log_prob_marginal``, K = 1 against ``log_prob_leapfrog_grad``, chunks, slices, row cuts) and ``min_weight``.

Tolerance: the derivative families' rule (tests/test_gpu_pushforward.py): per case the reference runs in float64 and in fp32; the
fp32 run's normalised error against float64 is the case's floor, and the device is held to FACTOR = 22 floors.  The CPU conditions
every case meets are in tests/test_marginal_grad_host.py.
"""
import pytest
import torch

from flowfusion_amd import _native, odeint
from tests import _leapfrog_pull_ref as L
from tests import _marginal_grad_ref as M
from tests._pushforward_ref import normalised_error
from tests.test_gpu_pushforward import FACTOR

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _dev(t):
    return None if t is None else t.detach().to(DEV, torch.float32).contiguous()


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D, K", M.KERNEL_SHAPES)
def test_kernels_are_marginal_reduce_bitwise_the_float64_restatement_and_their_host_twins(D, K, B):
    C = M.KERNEL_C[D]
    r = M.run_kernels(DEV, D, K, B, C)
    M.check_kernels(r, K, (D, K, B))
    # the host twin on the device's lw: the same additions in the same order
    hx, hc = _native.marginal_grad_reduce(r.lw, M.row_of(r.keep), r.gz[r.keep > 0].contiguous(),
                                          None if r.gc is None else r.gc[r.keep > 0].contiguous(), K, r.scale, r.cscale)
    assert torch.equal(M.bits(hx), M.bits(r.gx)) and (hc is None or torch.equal(M.bits(hc), M.bits(r.gcond)))


def test_the_grid_stride_loop_takes_a_second_trip():
    D, K, B = M.BIG
    r = M.run_kernels(DEV, D, K, B, 0)
    M.check_kernels(r, K, M.BIG)
    hx, _ = _native.marginal_grad_reduce(r.lw, r.full_of, torch.nan_to_num(r.gz), None, K, r.scale)
    assert torch.equal(M.bits(hx), M.bits(r.gx))


def test_min_weight_zero_and_one_momentum():
    r = M.run_kernels(DEV, 5, 3, 3, 3, min_weight=0.0)
    assert int(r.keep.sum()) == 9
    M.check_kernels(r, 3)
    D, C, B = 5, 3, 7
    _, gz, gc, scale, cscale = M.kernel_inputs(D, 1, B, C)
    lw = torch.linspace(-30.0, 4.0, B, dtype=torch.float64)
    gx, gcond = _native.marginal_grad_reduce(lw.to(DEV), torch.arange(B, dtype=torch.int32, device=DEV), _dev(gz), _dev(gc), 1,
                                             _dev(scale), _dev(cscale))
    assert torch.equal(M.bits(gx.cpu()), M.bits(gz[:, :D] / scale)) and torch.equal(M.bits(gcond.cpu()), M.bits(gc / cscale))


def test_degenerate_points_keep_nothing_and_write_nan_while_their_neighbours_are_untouched():
    D, K, B, C = 5, 4, 5, 3
    clean = M.run_kernels(DEV, D, K, B, C, min_weight=0.0)
    z1 = clean.z1.clone()
    z1[1 * K + 2, 3] = float("nan")                            # point 1: a NaN row
    z1[3 * K:4 * K, 0] = float("inf")                          # point 3: every lw is -inf
    r = M.run_kernels(DEV, D, K, B, C, min_weight=0.0, z1=z1)
    assert r.keep.view(B, K).tolist() == [[1] * K, [0] * K, [1] * K, [0] * K, [1] * K]
    assert torch.equal(M.bits(r.out), M.bits(r.out_r)) and torch.equal(M.bits(r.ess), M.bits(r.ess_r))
    for got, ref in ((r.gx, clean.gx), (r.gcond, clean.gcond)):
        assert bool(torch.isnan(got[[1, 3]]).all())
        assert torch.equal(M.bits(got[[0, 2, 4]]), M.bits(ref[[0, 2, 4]]))


# ---- the method -----------------------------------------------------------------------------------------------------------------------
_FRONTS = {}


def front_of(case):
    """(front end on the device, x, raw conditional or None -- on the device), made once per case."""
    key = L.front_id(case)
    if key not in _FRONTS:
        front, _, x, _, _, cond = L.front_inputs(case)
        _FRONTS[key] = (front.to(DEV), _dev(x), _dev(cond))
    return _FRONTS[key]


def run(case, K, **kw):
    front, x, cond = front_of(case)
    kw = dict(dict(num_steps=case[4], seed=M.SEED, sample_offset=M.OFFSET, return_ess=True), **kw)
    out = front.log_prob_marginal_grad(x, cond, K, **kw)
    return tuple(None if t is None else t.cpu() for t in out), dict(front.last_marginal_grad_stats)


def same(a, b):
    return all((s is None and t is None) or torch.equal(M.bits(s), M.bits(t)) for s, t in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("ck", M.CASES, ids=M.case_id)
def test_gradients_match_float64_autograd_and_the_value_is_log_prob_marginal_bitwise(ck):
    case, K = ck
    front, x, cond = front_of(case)
    (lp, gx, gc, ess), stats = run(case, K)
    B = x.shape[0]
    assert stats == {"rows": B * K, "rows_kept": B * K, "launches": {"forward": 1, "backward": 1}}       # no second forward
    lp2, ess2 = front.log_prob_marginal(x, cond, K, method="leapfrog", num_steps=case[4], seed=M.SEED, sample_offset=M.OFFSET,
                                        return_ess=True)
    assert same((lp, ess), (lp2.cpu(), ess2.cpu()))
    r = M.references(ck, DEV)
    r32, r64 = r[torch.float32], r[torch.float64]
    assert (gc is None) == (r64.gc is None)
    assert float((lp.double() - r64.log_p).abs().max()) <= 1e-4 * max(1.0, float(r64.log_p.abs().max()))
    for what, floor in M.floors(r32, r64).items():
        err = normalised_error({"gx": gx, "gc": gc}[what], getattr(r64, what))
        print(f"\n[marginal_grad] {M.case_id(ck)} {what}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors")
        assert err <= FACTOR * floor, (what, err, floor)


@pytest.mark.parametrize("case", L.LOGP_CASES, ids=L.front_id)
def test_one_momentum_is_log_prob_leapfrog_grad_of_that_draw_bitwise(case):
    front, x, cond = front_of(case)
    (lp, gx, gc, ess), _ = run(case, 1)
    p0 = _dev(M.momenta(x, 1, DEV)[:, 0])
    lp1, gx1, gc1 = front.log_prob_leapfrog_grad(x, cond, case[4], momentum=p0)
    assert same((gx, gc), (gx1.cpu(), None if gc1 is None else gc1.cpu()))
    assert float((lp - lp1.cpu()).abs().max()) <= 1e-4 * max(1.0, float(lp.abs().max())) and bool((ess == 1.0).all())


@pytest.mark.parametrize("case", L.LOGP_CASES, ids=L.front_id)
def test_chunks_and_slices_are_bitwise(case):
    front, x, cond = front_of(case)
    K, B = 4, x.shape[0]
    whole, _ = run(case, K)
    for chunk in (1, 4, B):
        part, stats = run(case, K, chunk_points=chunk)
        pieces = -(-B // chunk)
        assert same(part, whole), chunk
        assert stats["launches"] == {"forward": pieces, "backward": pieces} and stats["rows_kept"] == B * K
    cut = B // 2
    kw = dict(num_steps=case[4], seed=M.SEED, return_ess=True)
    lo = front.log_prob_marginal_grad(x[:cut], None if cond is None else cond[:cut], K, sample_offset=M.OFFSET, **kw)
    hi = front.log_prob_marginal_grad(x[cut:], None if cond is None else cond[cut:], K, sample_offset=M.OFFSET + cut, **kw)
    glued = tuple(None if a is None else torch.cat([a, b]).cpu() for a, b in zip(lo, hi))
    assert same(glued, whole)


def test_row_cuts_of_the_backward_half_are_bitwise(monkeypatch):
    case, K = L.LOGP_CASES[0], 4
    whole, _ = run(case, K)
    B, D = front_of(case)[1].shape
    monkeypatch.setattr(odeint, "PROBE_BUFFER_FLOATS", 2 * 5 * D + 1)           # five rows per backward launch
    part, stats = run(case, K)
    monkeypatch.undo()
    assert same(part, whole) and stats["launches"] == {"forward": 1, "backward": -(-B * K // 5)}


def test_min_weight_skips_the_draws_of_the_float64_scan_and_truncates_as_the_reference_that_zeroes_them():
    case, K = M.CUT_CASE, M.CUT_K
    r = M.references((case, K), DEV)
    r32, r64 = r[torch.float32], r[torch.float64]
    keep = r64.wn >= M.CUT
    assert float(((r64.wn - M.CUT).abs() / M.CUT).min()) >= 1e-3               # (the device's momenta: still no weight near it)
    full, _ = run(case, K)
    (lp, gx, gc, ess), stats = run(case, K, min_weight=M.CUT)
    assert stats["rows_kept"] == int(keep.sum()) and 0.25 <= stats["rows_kept"] / stats["rows"] <= 0.75
    assert stats["launches"] == {"forward": 1, "backward": 1}
    assert same((lp, ess), (full[0], full[3]))                                  # the value does not know min_weight
    ref = M.weighted(r64, r64.wn * keep)                                        # the weights of the full W, not renormalised
    for i, (what, floor) in enumerate(sorted(M.floors(r32, r64).items(), key=lambda kv: kv[0] != "gx")):
        got, untruncated = (gx, gc)[i], (full[1], full[2])[i]
        err, moved = normalised_error(got, ref[i]), normalised_error(got, untruncated)
        print(f"\n[marginal_grad] cut-off {what}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors; "
              f"{moved:.3e} from the min_weight = 0 result")
        assert err <= FACTOR * floor, (what, err, floor)
        assert moved > FACTOR * floor, (what, moved)
    # the stated bound: at most K m max |grad lw| per entry
    bound = K * M.CUT * float(r64.g.abs().max())
    assert float((gx.double() - full[1].double()).abs().max()) <= bound
