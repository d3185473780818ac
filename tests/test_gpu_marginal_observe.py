"""GPU tier of ``SymplecticFlowModel.log_prob_marginal_noisy`` / ``log_prob_marginal_noisy_grad`` (csrc/ff_marginal_observe.hip:
marginal_observe_expand_kernel, marginal_observe_grad_reduce_kernel).

The two kernels on the cells of tests/_marginal_grad_ref.py -- the same checks the host file runs on their host twins: the expand
bitwise its two parents (and ``marginal_expand`` at ``noise_std = 0``), ``grad_x`` and ``grad_c`` bitwise ``marginal_grad_reduce``
with and without ``grad_noise_std``, all three gradients to one fp32 ulp of the float64 restatement with every skipped row
poisoned, guard words around every output, a pointer one float off alignment, empty / full / partial kept sets, K = 1, degenerate
points, the second trip of the grid-stride loop -- and device against host twin, bitwise, on the same ``lw`` and draws' indices.
The methods on the three ``LOGP_CASES`` at K = 2 and 4 against float64 autograd through the logsumexp of the K one-draw
log-densities with respect to ``x``, ``conditional`` and ``sigma``, with the draws the device made; their bitwise properties
(``noise_std = 0`` against ``log_prob_marginal`` / ``log_prob_marginal_grad``, value against gradient method, chunks, slices, the
three layouts of ``noise_std``) and ``min_weight``.

Tolerance: the derivative families' rule (tests/test_gpu_pushforward.py): the fp32 run of the reference against float64 is the
case's floor, and the device is held to FACTOR = 22 floors.  The CPU conditions every case meets are in
tests/test_marginal_observe_host.py.
"""
import pytest
import torch

from flowfusion_amd import _native
from tests import _leapfrog_pull_ref as L
from tests import _marginal_grad_ref as M
from tests import _marginal_observe_ref as O
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
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D, K", M.KERNEL_SHAPES)
def test_expand_is_its_two_parents_bitwise(D, K, B):
    O.check_expand(DEV, D, K, B, M.KERNEL_C[D], "BD")
    O.check_expand(DEV, D, K, B, M.KERNEL_C[D], "D")


def test_expand_one_float_off_alignment_the_global_row_and_the_second_grid_trip():
    O.check_expand(DEV, 16, 17, 5, 4, "BD", offset=1)
    x, std, shift, scale, cond = O.expand_inputs(16, 17, 5, 4, "BD")
    whole, wc = O.raw_expand(DEV, x, std, shift, scale, cond, 17)
    part, pc = O.raw_expand(DEV, x[2:4], std[2:4], shift, scale, cond[2:4], 17, sample_offset=O.OFFSET + 2)
    assert torch.equal(O.bits(part), O.bits(whole[2 * 17:4 * 17])) and torch.equal(O.bits(pc), O.bits(wc[2 * 17:4 * 17]))
    D, K, B = M.BIG                                            # more rows than the largest grid holds
    O.check_expand(DEV, D, K, B, 4, "BD")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D, K", M.KERNEL_SHAPES)
def test_reduce_is_marginal_grad_reduce_bitwise_the_float64_restatement_and_its_host_twin(D, K, B):
    C = M.KERNEL_C[D]
    for mode in ("partial", "full", "empty"):
        r = O.run_reduce(DEV, D, K, B, C, keep_mode=mode)
        O.check_reduce(r, K, (D, K, B, mode))
    # the host twin on the device's lw (the last mode's: nothing kept says nothing, so once more on the partial set)
    r = O.run_reduce(DEV, D, K, B, C)
    kept = r.keep > 0
    hx, hc, hs = _native.marginal_observe_grad_reduce(r.lw, O.row_of(r.keep), r.gz[kept].contiguous(),
                                                      None if r.gc is None else r.gc[kept].contiguous(), torch.ones(D), K, O.SEED,
                                                      O.OFFSET, r.scale, r.cscale)
    assert torch.equal(O.bits(hx), O.bits(r.gx)) and (hc is None or torch.equal(O.bits(hc), O.bits(r.gcond)))
    # (libm's normals and the hardware's agree to rounding, not bit for bit: the twin's grad_noise_std is within that of the device's)
    assert float((hs - r.gs).abs().max()) <= 1e-4 * max(1.0, float(r.gs.abs().max()))


def test_reduce_one_float_off_alignment_the_vector_layout_and_the_second_grid_trip():
    O.check_reduce(O.run_reduce(DEV, 16, 17, 5, 4, offset=1), 17)
    O.check_reduce(O.run_reduce(DEV, 4, 65, 5, 4, std_layout="D"), 65)
    D, K, B = M.BIG
    O.check_reduce(O.run_reduce(DEV, D, K, B, 0), K, M.BIG)


def test_one_draw_is_minus_z_g_over_scale_rounded_once():
    D, C, B = 5, 3, 7
    _, gz, gc, scale, cscale = M.kernel_inputs(D, 1, B, C)
    lw = torch.linspace(-30.0, 4.0, B, dtype=torch.float64)
    z, _ = O.draws(B, D, 1, DEV)
    gx, gcond, gs = _native.marginal_observe_grad_reduce(lw.to(DEV), torch.arange(B, dtype=torch.int32, device=DEV), _dev(gz),
                                                         _dev(gc), _dev(torch.ones(D)), 1, O.SEED, O.OFFSET, _dev(scale),
                                                         _dev(cscale))
    want = (-(z[:, 0].double() * gz[:, :D].double()) / scale.double()).float()
    assert torch.equal(O.bits(gs.cpu()), O.bits(want))
    assert torch.equal(O.bits(gx.cpu()), O.bits(gz[:, :D] / scale)) and torch.equal(O.bits(gcond.cpu()), O.bits(gc / cscale))


def test_degenerate_points_write_nan_to_all_three_while_their_neighbours_are_untouched():
    D, K, B, C = 5, 4, 5, 3
    clean = O.run_reduce(DEV, D, K, B, C, min_weight=0.0)
    z1 = M.kernel_inputs(D, K, B, C)[0].clone()
    z1[1 * K + 2, 3] = float("nan")                            # point 1: a NaN row
    z1[3 * K:4 * K, 0] = float("inf")                          # point 3: every lw is -inf
    r = O.run_reduce(DEV, D, K, B, C, min_weight=0.0, z1=z1)
    assert r.keep.view(B, K).tolist() == [[1] * K, [0] * K, [1] * K, [0] * K, [1] * K]
    for got, ref in ((r.gx, clean.gx), (r.gcond, clean.gcond), (r.gs, clean.gs)):
        assert bool(torch.isnan(got[[1, 3]]).all())
        assert torch.equal(O.bits(got[[0, 2, 4]]), O.bits(ref[[0, 2, 4]]))
    assert torch.equal(O.bits(r.gx), O.bits(r.px)) and torch.equal(O.bits(r.gcond), O.bits(r.pc))


# ---- the methods ----------------------------------------------------------------------------------------------------------------------
_FRONTS = {}


def front_of(case):
    """(front end, x, noise_std [B, D], raw conditional or None -- on the device), made once per case."""
    key = L.front_id(case)
    if key not in _FRONTS:
        front, x, std, cond = O.case_inputs(case)
        _FRONTS[key] = (front.to(DEV), _dev(x), _dev(std), _dev(cond))
    return _FRONTS[key]


def run(case, K, std=None, **kw):
    front, x, s, cond = front_of(case)
    kw = dict(dict(num_steps=case[4], seed=O.SEED, sample_offset=O.OFFSET, return_ess=True, return_noise_grad=True), **kw)
    out = front.log_prob_marginal_noisy_grad(x, s if std is None else std, cond, K, **kw)
    return tuple(None if t is None else t.cpu() for t in out), dict(front.last_marginal_noisy_grad_stats)


def same(a, b):
    return all((s is None and t is None) or torch.equal(O.bits(s), O.bits(t)) for s, t in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("ck", O.CASES, ids=O.case_id)
def test_gradients_match_float64_autograd_and_the_value_method_agrees_bitwise(ck):
    case, K = ck
    front, x, std, cond = front_of(case)
    (lp, gx, gc, ess, gs), stats = run(case, K)
    B = x.shape[0]
    assert stats == {"rows": B * K, "rows_kept": B * K, "launches": {"forward": 1, "backward": 1}}       # no second forward
    lp2, ess2 = front.log_prob_marginal_noisy(x, std, cond, K, method="leapfrog", num_steps=case[4], seed=O.SEED,
                                              sample_offset=O.OFFSET, return_ess=True)
    assert same((lp, ess), (lp2.cpu(), ess2.cpu()))
    (lp3, gx3, gc3), _ = run(case, K, return_ess=False, return_noise_grad=False)                       # the parent's reduce
    assert same((lp, gx, gc), (lp3, gx3, gc3))
    r = O.references(ck, DEV)
    r32, r64 = r[torch.float32], r[torch.float64]
    assert (gc is None) == (r64.gc is None)
    assert float((lp.double() - r64.log_p).abs().max()) <= 1e-4 * max(1.0, float(r64.log_p.abs().max()))
    assert float((ess.double() - r64.ess).abs().max()) <= 1e-3 * K
    for what, floor in O.floors(r32, r64).items():
        err = normalised_error({"gx": gx, "gc": gc, "gs": gs}[what], getattr(r64, what))
        print(f"\n[marginal_observe] {O.case_id(ck)} {what}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors")
        assert err <= FACTOR * floor, (what, err, floor)


@pytest.mark.parametrize("case", L.LOGP_CASES, ids=L.front_id)
def test_zero_noise_is_the_marginal_and_its_gradient_bitwise_in_every_layout(case):
    front, x, std, cond = front_of(case)
    K, n = 4, case[4]
    kw = dict(num_steps=n, seed=O.SEED, sample_offset=O.OFFSET, return_ess=True)
    want = tuple(None if t is None else t.cpu() for t in front.log_prob_marginal_grad(x, cond, K, **kw))
    for zero in (0.0, torch.zeros(x.shape[1]), torch.zeros_like(std)):
        (lp, gx, gc, ess, gs), _ = run(case, K, std=zero)
        assert same((lp, gx, gc, ess), want)
        assert bool(torch.isfinite(gs).all()) and float(gs.abs().max()) > 0        # d / d sigma does not vanish at sigma = 0
        lp2, ess2 = front.log_prob_marginal_noisy(x, zero, cond, K, method="leapfrog", **kw)
        lp1, ess1 = front.log_prob_marginal(x, cond, K, method="leapfrog", **kw)
        assert same((lp2.cpu(), ess2.cpu()), (lp1.cpu(), ess1.cpu()))


@pytest.mark.parametrize("case", L.LOGP_CASES, ids=L.front_id)
def test_chunks_slices_and_layouts_are_bitwise(case):
    front, x, std, cond = front_of(case)
    K, B = 4, x.shape[0]
    whole, _ = run(case, K)
    vkw = dict(method="leapfrog", num_steps=case[4], seed=O.SEED, sample_offset=O.OFFSET, return_ess=True)
    value = tuple(t.cpu() for t in front.log_prob_marginal_noisy(x, std, cond, K, **vkw))
    for chunk in (1, 4, B):
        part, stats = run(case, K, chunk_points=chunk)
        pieces = -(-B // chunk)
        assert same(part, whole), chunk
        assert stats["launches"] == {"forward": pieces, "backward": pieces} and stats["rows_kept"] == B * K
        assert same(tuple(t.cpu() for t in front.log_prob_marginal_noisy(x, std, cond, K, chunk_points=chunk, **vkw)), value)
    cut = B // 2
    kw = dict(num_steps=case[4], seed=O.SEED, return_ess=True, return_noise_grad=True)
    c = lambda lo, hi: None if cond is None else cond[lo:hi]
    lo = front.log_prob_marginal_noisy_grad(x[:cut], std[:cut], c(0, cut), K, sample_offset=O.OFFSET, **kw)
    hi = front.log_prob_marginal_noisy_grad(x[cut:], std[cut:], c(cut, B), K, sample_offset=O.OFFSET + cut, **kw)
    glued = tuple(None if a is None else torch.cat([a, b]).cpu() for a, b in zip(lo, hi))
    assert same(glued, whole)
    # the scalar, [D] and [B, D] layouts of one sigma
    D = x.shape[1]
    layouts = (0.25, torch.tensor(0.25), torch.full((D,), 0.25), torch.full((B, D), 0.25, device=DEV))
    first, _ = run(case, K, std=layouts[0], chunk_points=4)
    assert not same(first, whole)
    for s in layouts[1:]:
        assert same(run(case, K, std=s)[0], first)
        assert same(tuple(t.cpu() for t in front.log_prob_marginal_noisy(x, s, cond, K, **vkw)), (first[0], first[3]))


def test_min_weight_skips_the_draws_of_the_float64_scan_and_truncates_as_the_reference_that_zeroes_them():
    case, K = O.CUT_CASE, O.CUT_K
    r = O.references((case, K), DEV)
    r32, r64 = r[torch.float32], r[torch.float64]
    keep = r64.wn >= O.CUT
    assert float(((r64.wn - O.CUT).abs() / O.CUT).min()) >= 1e-3               # (the device's draws: still no weight near it)
    full, _ = run(case, K)
    (lp, gx, gc, ess, gs), stats = run(case, K, min_weight=O.CUT)
    assert stats["rows_kept"] == int(keep.sum()) and 0.25 <= stats["rows_kept"] / stats["rows"] <= 0.75
    assert stats["launches"] == {"forward": 1, "backward": 1}
    assert same((lp, ess), (full[0], full[3]))                                  # the value does not know min_weight
    ref = dict(zip(("gx", "gc", "gs"), O.weighted(r64, r64.wn * keep)))         # the weights of the full W, not renormalised
    got, untruncated = {"gx": gx, "gc": gc, "gs": gs}, {"gx": full[1], "gc": full[2], "gs": full[4]}
    for what, floor in O.floors(r32, r64).items():
        err, moved = normalised_error(got[what], ref[what]), normalised_error(got[what], untruncated[what])
        print(f"\n[marginal_observe] cut-off {what}: err {err:.3e} floor {floor:.3e} = {err / floor:.2f} floors; "
              f"{moved:.3e} from the min_weight = 0 result")
        assert err <= FACTOR * floor, (what, err, floor)
        assert moved > FACTOR * floor, (what, moved)
