"""GPU tier: the streaming kernels beside the fused integrator (csrc/ff_aux.hip, csrc/ff_norm.h) at their loop boundaries.

``ff_stage_combine``, ``ff_scaled_rms`` and ``ff_normal_fill`` are grid-stride loops over 16-byte elements; their grids are
capped at 2048 workgroups of 256 threads, so one trip covers ``S = 2048 * 256`` sixteen-byte elements, and the reduction
runs in a single block (no partials, no arrival counter) up to ``n = 8195``.  The shapes below sit on those two lines:
one element short of a trip, exactly a trip, one element more, the hand-over between the unrolled double trip, the single
remainder trip and the ``n % 4`` scalar tail.  Every element is compared, against a float64 statement of the operation
written in plain torch / numpy; every bar is derived where it is used.

``scaled_rms_reduce`` is shared by the host controller (``ff_scaled_rms``) and the device controller
(``adapt_control_kernel``), so a comparison of the two controllers cannot see an error in it: these tests can.
"""
import ctypes

import numpy as np
import pytest
import torch

from flowfusion_amd import _native
from tests._philox import EXTREME_ROWS, EXTREME_SEED

DEV = "cuda"
pytestmark = pytest.mark.gpu

S = 2048 * 256              # 16-byte elements one trip of a capped grid covers (stream_grid / copy_grid / kNormBlocks x 256 threads)
SOLO_MAX = 8195             # largest n the reduction runs in one block: most / 4 <= 2048 (norm_args_from_terms)
SENTINEL = -7.5e33          # guard words around an output
GUARD = 4096                # guard words behind an output (four before it)

@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_the_constants_the_shapes_depend_on():
    """kNormBlocks = 2048 is what puts the sizes below on the trip boundary; the workspace is 16 bytes (the counter word)
    plus kNormBlocks x (FF_NORM_TERMS + 1 = 4) doubles."""
    assert (int(_native.lib().ff_scaled_rms_workspace_bytes()) - 16) // (4 * 8) == 2048
    assert S == 2048 * 256 and SOLO_MAX // 4 == 2048 and (SOLO_MAX + 1) // 4 == 2049


def _guards_untouched(arena, n):
    return bool((arena[:4] == SENTINEL).all()) and bool((arena[4 + n:] == SENTINEL).all())


# ---- ff_stage_combine ---------------------------------------------------------------------------------------------------
COEFS = [0.5, 0.0, -1.25, 0.0, 3.0, 2.0 ** -10, -2.0]        # exact in fp32; two zeros: their arrays hold NaN
X_COEF = 0.75
LIVE = [s for s, c in enumerate(COEFS) if c != 0.0]
SHIFTED = 4                                                   # the term that is passed one float past alignment
COMBINE_N4 = [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S - 1]
COMBINE_NMAX = 4 * (3 * S - 1) + 3


def _combine_bar(mag, live_terms):
    """|got - ref64| <= (T + 1) 2^-23 sum |c_s k_s|, T = the live terms, x included.  Derivation: each of the T products is
    rounded once (relative 2^-24), each of the T - 1 sums once (relative 2^-24 of a partial sum, itself at most
    (1 + T 2^-24) sum |c_s k_s|): at most (2 T - 1) 2^-24 (1 + ..) sum |c_s k_s| < (T + 1) 2^-23 sum |c_s k_s|.  A fused
    multiply-add only removes roundings."""
    return (live_terms + 1) * 2.0 ** -23 * mag


def _assert_within(got, ref, bar, what):
    ok = (got.double() - ref).abs() <= bar                    # (a NaN fails the comparison)
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f"{what}: element {i} of {got.numel()}: got {got[i].item()!r}, float64 {ref[i].item()!r}, bar {bar[i].item():.3e}")


def _combine(out, x, ks, coefs, x_coef):
    """The C entry itself, every pointer handed over -- the arrays of zero coefficients too (the Python wrapper would
    leave them out): it is the entry that must not read them."""
    a = _native.CombineArgs()
    a.out, a.x, a.x_coef, a.n = out.data_ptr(), 0 if x is None else x.data_ptr(), float(x_coef), out.numel()
    for s, (k, c) in enumerate(zip(ks, coefs)):
        assert k.numel() == out.numel() and k.dtype == torch.float32 and k.is_contiguous()
        a.k[s], a.coef[s] = k.data_ptr(), float(c)
    rc = _native.lib().ff_stage_combine(ctypes.byref(a), ctypes.c_void_p(_stream()))
    assert rc == _native.FF_OK
    return out


@pytest.fixture(scope="module")
def combine_data():
    """Inputs of the largest size and their float64 products, computed once; every size uses a prefix."""
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(COMBINE_NMAX + 4, device=DEV, generator=g)
    ks = [torch.randn(COMBINE_NMAX + 4, device=DEV, generator=g) for _ in COEFS]
    for s, c in enumerate(COEFS):
        if c == 0.0:
            ks[s].fill_(float("nan"))
    prod = {s: COEFS[s] * ks[s].double() for s in LIVE}
    px = X_COEF * x.double()
    ref, mag = px.clone(), px.abs()
    for s in LIVE:
        ref += prod[s]
        mag += prod[s].abs()
    return dict(x=x, ks=ks, prod=prod, px=px, ref=ref, mag=mag)


@pytest.mark.parametrize("n4", COMBINE_N4)
def test_stage_combine_every_element_around_the_trip_boundaries(n4, combine_data):
    """n / 4 one short of one, two and three trips, exactly one and two, one more: the unrolled double trip
    (`i + stride < n4`), the single remainder trip (`if (i < n4)`) and the scalar tail (n % 4 = 0, 1, 3) hand over to each
    other in every combination.  Seven terms, two with a zero coefficient and NaN in their arrays.  Each size: all pointers
    aligned (16-byte loop), one k[s] a view one float past alignment (the whole call takes the scalar loop), in place with
    out = x and with out = k[s].  All n elements against float64 at the derived bar of `_combine_bar`; the words around
    `out` keep their sentinel."""
    d = combine_data
    T = len(LIVE) + 1
    for tail in (0, 1, 3):
        n = 4 * n4 + tail
        x, ks = d["x"][:n], [k[:n] for k in d["ks"]]
        ref, bar = d["ref"][:n], _combine_bar(d["mag"][:n], T)
        # aligned, into a sentinel-filled arena: the last float4, the tail and nothing else are written
        arena = torch.full((4 + n + GUARD,), SENTINEL, device=DEV)
        out = arena[4:4 + n]
        assert out.data_ptr() % 16 == 0 and all(k.data_ptr() % 16 == 0 for k in ks) and x.data_ptr() % 16 == 0
        _combine(out, x, ks, COEFS, X_COEF)
        _assert_within(out, ref, bar, f"aligned n={n}")
        assert _guards_untouched(arena, n), f"aligned n={n}: a word outside out[0:n] was written"
        # one term one float past alignment: the scalar loop does all of it
        ks_s = list(ks)
        ks_s[SHIFTED] = d["ks"][SHIFTED][1:n + 1]
        assert ks_s[SHIFTED].data_ptr() % 16 == 4
        ref_s = ref - d["prod"][SHIFTED][:n] + d["prod"][SHIFTED][1:n + 1]
        bar_s = _combine_bar(d["mag"][:n] - d["prod"][SHIFTED][:n].abs() + d["prod"][SHIFTED][1:n + 1].abs(), T)
        arena.fill_(SENTINEL)
        _combine(out, x, ks_s, COEFS, X_COEF)
        _assert_within(out, ref_s, bar_s, f"unaligned k[{SHIFTED}] n={n}")
        assert _guards_untouched(arena, n), f"unaligned n={n}: a word outside out[0:n] was written"
        # in place
        xin = x.clone()
        _combine(xin, xin, ks, COEFS, X_COEF)
        _assert_within(xin, ref, bar, f"out is x, n={n}")
        kin = ks[2].clone()
        _combine(kin, x, ks[:2] + [kin] + ks[3:], COEFS, X_COEF)
        _assert_within(kin, ref, bar, f"out is k[2], n={n}")


@pytest.mark.parametrize("n", [7, 4099, 4 * (S + 1) + 3])
def test_stage_combine_does_not_read_x_when_x_coef_is_zero(n, combine_data):
    """generic.py passes x = y with x_coef = 0 for the derivative and the error estimate of every attempted step, and a
    scratch as x = out for the log-density ones: x is then treated like a k[s] with a zero coefficient -- not read (NaN in it
    does not reach the output) and not part of the alignment test.  Two live terms: T = 2 in the bar of `_combine_bar`."""
    d = combine_data
    k0, k2 = d["ks"][0][:n], d["ks"][2][:n]
    ref = 2.0 * k0.double() - 1.25 * k2.double()
    bar = _combine_bar(2.0 * k0.double().abs() + 1.25 * k2.double().abs(), 2)
    nan = torch.full((n + 4,), float("nan"), device=DEV)
    for x in (nan[:n], nan[1:n + 1]):                                     # aligned, and one float past alignment
        arena = torch.full((4 + n + GUARD,), SENTINEL, device=DEV)
        out = arena[4:4 + n]
        _combine(out, x, [k0, nan[:n], k2], [2.0, 0.0, -1.25], 0.0)
        assert bool(torch.isfinite(out).all())
        _assert_within(out, ref, bar, f"x_coef = 0, n={n}")
        assert _guards_untouched(arena, n)
    out = nan[:n].clone()                                                 # out is x: written over, never read
    _combine(out, out, [k0, nan[:n], k2], [2.0, 0.0, -1.25], 0.0)
    assert bool(torch.isfinite(out).all())
    _assert_within(out, ref, bar, f"out is x, x_coef = 0, n={n}")


# ---- ff_scaled_rms ------------------------------------------------------------------------------------------------------
RMS_SIZES = [8191, 8192, 8195, 8196, 8199, 8200,
             4 * S - 1, 4 * S, 4 * S + 1, 4 * S + 4, 4 * S + 7, 8 * S, 8 * S + 5, 12 * S - 4]
RMS_NMAX = 12 * S + 8


def _positions(n):
    """Where one element can be lost: the first, the last of the float4 body, every element of the n % 4 tail, the last,
    and both sides of the seam between two trips -- of the capped grid (4 S, 8 S) and of the single block (4 x 256)."""
    body = 4 * (n // 4)
    p = {0, body - 1, n - 1} | set(range(body, n))
    for seam in (4 * 256, 4 * S, 8 * S):
        p |= {seam - 1, seam}
    return sorted(q for q in p if 0 <= q < n)


@pytest.fixture(scope="module")
def rms_data():
    g = torch.Generator(device=DEV).manual_seed(3)
    r = lambda scale: torch.randn(RMS_NMAX, device=DEV, generator=g) * scale
    return dict(ones=torch.ones(RMS_NMAX, device=DEV), err=r(1e-4), y0=r(1.0), y1=r(1.0), f0=r(1.0), f1=r(1.0),
                le=r(1e-3), l0=r(3.0), l1=r(3.0))


def _twice(terms, atol, rtol, check=None):
    """Every configuration runs twice: no floating-point atomics, so the results agree bit for bit."""
    a = _native.scaled_rms(terms, atol, rtol, check=check)
    b = _native.scaled_rms(terms, atol, rtol, check=check)
    assert a == b or all(x == y or (x != x and y != y) for x, y in zip(a, b)), (a, b)
    return a


@pytest.mark.parametrize("n", RMS_SIZES)
def test_scaled_rms_counts_every_element_exactly_once(n, rms_data):
    """Numerator and scale all ones, atol = rtol = 0.5: every quotient is exactly 1, the sum of squares is the number of
    elements the kernel visited (exact in double) and the result is sqrt(visited / n).  For n < 2^23 one element dropped or
    counted twice moves sqrt((n -+ 1) / n) = 1 -+ 1 / (2 n) off 1 by more than half an ulp of 1.0f (2^-25 below, 2^-24
    above), so it no longer rounds to 1.0f.  On the float4 body and, through a view one float past alignment, on the
    scalar body."""
    assert n < 2 ** 23
    ones = rms_data["ones"]
    for v in (ones[:n], ones[1:n + 1]):
        got = _twice([(v, None, v, None)], 0.5, 0.5)
        assert got[0] == 1.0 and got[1] == 0.0, (n, v.data_ptr() % 16, got)


@pytest.mark.parametrize("n", RMS_SIZES)
def test_scaled_rms_sees_a_spike_at_every_seam(n, rms_data):
    """Numerator zero but 2^10 at one position, scale 1: the sum of squares is exactly 2^20 if the element was visited
    once.  Bar: one float32 ulp of float32(sqrt(2^20 / n)) -- the double square root and its rounding to fp32 against
    numpy's; nothing else rounds."""
    ones = rms_data["ones"][:n]
    num = torch.zeros(n, device=DEV)
    exp = np.float32(np.sqrt(2.0 ** 20 / n))
    for p in _positions(n):
        num[p] = 1024.0
        got = _twice([(num, None, ones, None)], 0.5, 0.5)
        num[p] = 0.0
        assert abs(got[0] - float(exp)) <= float(np.spacing(exp)), (n, p, got[0], float(exp))
    assert _native.scaled_rms([(num, None, ones, None)], 0.5, 0.5)[0] == 0.0


def _rms64(num, sub, s0, s1, atol, rtol):
    if num.numel() == 0:
        return 0.0
    d = num.double() - (0.0 if sub is None else sub.double())
    scale = s0.double().abs() if s1 is None else torch.max(s0.double().abs(), s1.double().abs())
    return float((d / (atol + rtol * scale)).pow(2).mean().sqrt())


RMS_RANDOM = [(n, n // 3 + 1, n - 2, None) for n in RMS_SIZES] + [
    (SOLO_MAX, 4 * S + 7, 5000, "term 1 sets the grid"),
    (4 * S + 1, 0, 8196, "a term of no elements"),
    (4 * S + 7, 8195, 4 * S + 7, "sub one float past alignment"),
    (8199, 37, 8195, "sub one float past alignment"),
]


@pytest.mark.parametrize("n,m,k,what", RMS_RANDOM)
def test_scaled_rms_random_terms_against_float64(n, m, k, what, rms_data):
    """Three terms of different sizes (the error ratio of the state, of the log-density, and a difference of derivatives)
    against the float64 expression at the project's bar for this kernel, 2e-6 max(1, |e|).  The grid follows the largest
    term, whichever it is; a term of no elements gives 0; a term with one unaligned array takes the scalar body alone."""
    d = rms_data
    atol, rtol = 1e-5, 1e-4
    sub = d["f0"][1:k + 1] if what == "sub one float past alignment" else d["f0"][:k]
    terms = [(d["err"][:n], None, d["y0"][:n], d["y1"][:n]), (d["le"][:m], None, d["l0"][:m], d["l1"][:m]),
             (d["f1"][:k], sub, d["y0"][:k], None)]
    if what == "sub one float past alignment":
        assert sub.data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for t in terms[0] + terms[1] if t is not None)
    got = _twice(terms, atol, rtol, check=d["y1"][:n])
    for g, t in zip(got, terms):
        e = _rms64(*t, atol, rtol)
        assert abs(g - e) <= 2e-6 * max(1.0, abs(e)), (n, m, k, what, g, e)
    assert got[3] == 0.0
    if m == 0:
        assert got[1] == 0.0


def test_scaled_rms_counter_word_returns_to_zero(rms_data):
    """An arrival-counter launch, a single-block launch, the first again: were the counter word left at a value other
    than zero, no block of the next arrival-counter launch would find itself last (or a wrong one would) and its result
    would be stale or partial.  The word itself is read too."""
    d = rms_data
    big = [(d["err"][:8 * S + 5], None, d["y0"][:8 * S + 5], d["y1"][:8 * S + 5])]
    solo = [(d["err"][:SOLO_MAX], None, d["y0"][:SOLO_MAX], d["y1"][:SOLO_MAX])]
    other = [(d["f1"][:SOLO_MAX + 1], d["f0"][:SOLO_MAX + 1], d["y0"][:SOLO_MAX + 1], None)]
    ws, _ = _native.norm_workspace(torch.device(DEV, torch.cuda.current_device()), _stream())
    seq = [big, solo, big, other, solo, big, other]
    res = []
    for terms in seq:
        res.append(_native.scaled_rms(terms, 1e-5, 1e-4, check=terms[0][3] if terms[0][3] is not None else terms[0][2]))
        assert int(ws[0].item()) == 0
    assert res[0] == res[2] == res[5] and res[1] == res[4] and res[3] == res[6]
    for terms, r in ((big, res[0]), (solo, res[1]), (other, res[3])):
        e = _rms64(*terms[0], 1e-5, 1e-4)
        assert abs(r[0] - e) <= 2e-6 * max(1.0, abs(e)) and r[1] == 0.0


@pytest.mark.parametrize("n", RMS_SIZES)
def test_scaled_rms_nonfinite_flag_on_every_route(n, rms_data):
    """The finiteness check of an attempted step has three routes: folded into term 0's pass when `check` IS scale1[0]
    (what every adaptive attempt uses), a pass of its own on float4, the same on scalars (`check` unaligned).  A fourth
    configuration has `check` at scale1[0]'s address but longer than term 0: it must not be folded, or the elements behind
    term 0 go unchecked.  NaN, +inf, -inf at every position of `_positions`: the flag is 1.0; without a plant 0.0.  On the
    folded route only the flag is asserted (term 0's norm is non-finite by construction); elsewhere the norm, whose inputs
    are clean, keeps its bits."""
    d = rms_data
    atol, rtol = 1e-5, 1e-4
    err, y0, y1 = d["err"][:n], d["y0"][:n], d["y1"][:n]
    y1c = y1.clone()                                   # planted into and restored: the shared inputs stay as they are
    shifted = torch.empty(n + 4, device=DEV)[1:n + 1]
    shifted.copy_(y1)
    assert y1c.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    routes = {
        "folded": ([(err, None, y0, y1c)], y1c),
        "separate, float4": ([(err, None, y0, y1)], y1c),
        "separate, scalar": ([(err, None, y0, y1)], shifted),
        "same address, longer than term 0": ([(err[:n - 4], None, y0[:n - 4], y1c[:n - 4])], y1c),
    }
    for name, (terms, check) in routes.items():
        clean = _twice(terms, atol, rtol, check=check)
        assert clean[1] == 0.0, (n, name, clean)
        for bad in (float("nan"), float("inf"), float("-inf")):
            for p in _positions(n):
                check[p] = bad
                got = _native.scaled_rms(terms, atol, rtol, check=check)
                check[p] = y1[p]
                assert got[1] == 1.0, (n, name, bad, p, got)
                if name.startswith("separate"):
                    assert got[0] == clean[0], (n, name, bad, p, got, clean)
        assert _native.scaled_rms(terms, atol, rtol, check=check) == clean, (n, name)


# ---- ff_normal_fill -----------------------------------------------------------------------------------------------------
FILL_DIMS = [1, 2, 3, 4, 5, 8, 9, 16]
# (threads' work items = batch x ceil(dim / 4), sample_offset, scale): below one trip, into the second, into the third
FILL_TOTALS = [(S - 1, 0, 1.0), (S + 1, 2 ** 33 + 7, 1.0), (2 * S + 3, 12345678901, -2.5)]
FILL_BAR = 2e-6


def _fill_batch(total, nblk):
    """batch x nblk = total where nblk divides it (S - 1 is prime, 2 S + 3 is odd: it often does not); else the nearest
    batch on the same side of the trip boundary -- rounded down below a trip, up above one."""
    return total // nblk if total < S else -(-total // nblk)


def _fill_into_arena(batch, dim, seed, offset, noise_index, scale):
    n = batch * dim
    arena = torch.full((4 + n + GUARD,), SENTINEL, device=DEV)
    rc = _native.lib().ff_normal_fill(arena.data_ptr() + 16, batch, dim, seed, offset, noise_index, float(scale),
                                      ctypes.c_void_p(_stream()))
    assert rc == _native.FF_OK
    torch.cuda.synchronize()
    assert _guards_untouched(arena, n), f"[{batch}, {dim}]: a word outside the output was written"
    return arena[4:4 + n].view(batch, dim).cpu().numpy()


def _fill_error(got, ref, scale):
    """max over the elements of |got - scale ref| / (max(1, |ref|) |scale|) and where it is."""
    ref = ref.astype(np.float64)
    e = np.abs(got.astype(np.float64) - scale * ref) / (np.maximum(1.0, np.abs(ref)) * abs(scale))
    e = np.where(np.isfinite(got), e, np.inf)
    i = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[i]), i


@pytest.mark.parametrize("total,offset,scale", FILL_TOTALS)
@pytest.mark.parametrize("dim", FILL_DIMS)
def test_normal_fill_every_element_against_the_restatement(dim, total, offset, scale):
    """Every element of fills that end below one grid-stride trip, in the second and in the third, for row lengths that
    take the 16-byte store (dim % 4 = 0) and the scalar stores (dim 5: a full first block in a row that is not 16-byte
    aligned), with 64-bit global rows and a scale, against tests/_philox.normals (float64 log / sin / cos).  The words
    around the output keep their sentinel: the last row of a dim % 4 != 0 fill does not write past its end.
    Bar: the project's figure for this comparison (hardware log, sine and cosine against numpy), relative to
    max(1, |ref|) so that it reaches the tails some 2 M draws have: 2e-6 max(1, |ref|) |scale|."""
    from tests._philox import normals
    nblk = (dim + 3) // 4
    batch = _fill_batch(total, nblk)
    assert abs(batch * nblk - total) < nblk and (batch * nblk > S) == (total > S)
    seed, noise_index = 2024 + dim, 5 if scale == 1.0 else _native.PRIOR_NOISE_INDEX
    got = _fill_into_arena(batch, dim, seed, offset, noise_index, scale)
    ref = normals(seed, offset, batch, dim, [noise_index])[0]
    err, where = _fill_error(got, ref, scale)
    print(f"normal_fill dim={dim} batch={batch} offset={offset} scale={scale}: max error {err:.3e} at row {where[0]} column {where[1]}"
          f" (got {got[where]!r}, ref {ref[where]!r})")
    assert err <= FILL_BAR, (dim, batch, err, where)


def test_normal_fill_at_the_extremes_of_the_mapping():
    """Rows whose words sit at the ends of the Box-Muller mapping (EXTREME_ROWS; found by a search of the restatement
    over 39 M rows of seed 2024, proven on the CPU tier): a radius word of 0 -- u1 = 2^-25, the largest radius of the stream,
    5.887 -- and an angle word of 0 against the restatement at the bar above; a radius word of 0xFFFFFF, where
    fma(2^24 - 1, 2^-24, 2^-25) rounds to exactly 1.0f, log gives 0 and both normals of the pair must be zero and finite."""
    from tests._philox import normals
    for row, pair, kind in EXTREME_ROWS:
        got = _fill_into_arena(1, 4, EXTREME_SEED, row, _native.PRIOR_NOISE_INDEX, 1.0)
        ref = normals(EXTREME_SEED, row, 1, 4, [_native.PRIOR_NOISE_INDEX])[0]
        z = got[0, 2 * pair:2 * pair + 2]
        err, where = _fill_error(got, ref, 1.0)
        print(f"normal_fill row {row} ({kind}): got {got[0].tolist()}, ref {ref[0].tolist()}, max error {err:.3e}")
        assert np.isfinite(got).all() and err <= FILL_BAR, (row, kind, got, ref, err)
        if kind == "radius_max_word":
            assert z[0] == 0.0 and z[1] == 0.0, (row, z)
