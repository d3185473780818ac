"""GPU tier: kick-drift-kick leapfrog of the symplectic flows on the row-select kernel (csrc/ff_mlp_pair.hpp, SELECT).

Anchors: a float64 leapfrog written on the restatement's dynamics (tests/test_symplectic_leapfrog_host.py); a known answer
independent of every restatement -- rotation weights, for which a leapfrog step is a product of three 2 x 2 shear
matrices; the exact invertibility of the discrete map (the round trip); and bitwise equalities: twin against
one-wavefront kernel, re-runs, rows against the batch they sit in."""
import copy
import ctypes
import math
import os

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.distributed import symplectic_log_prob_sharded, symplectic_sample_sharded
from flowfusion_amd.fused import MODE_STATE
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
from tests._symplectic_ref import SymplecticRef
from tests._util import golden_names, load_golden, max_rel
from tests.test_gpu_symplectic import _rotation_model, _warned
from tests.test_gpu_symplectic_twin import pinned, seeded_model
from tests.test_symplectic_host import EXPECTED_KERNEL, build_model
from tests.test_symplectic_leapfrog_host import IN_ENVELOPE, NET_B, emulate_select, leapfrog_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE_TOL = 2e-5        # relative to max |reference state| (tests/test_gpu_symplectic.py)
STEPS = (1, 4, 25)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


def _state_err(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _logp_err(got, want):
    return max_rel(got.detach().cpu(), want.detach().cpu(), floor=1.0)


def _dev(t):
    return None if t is None else t.to(DEV)


def _grid(n):
    return torch.linspace(1.0, 0.0, n + 1)


def _fixture_model(name):
    """(meta, arrays, model on the GPU, float64 restatement), built once per fixture."""
    if name not in _cache:
        meta, arrays = load_golden(name)
        fm, sd = build_model(meta, arrays)
        _cache[name] = (meta, arrays, fm.to(DEV), SymplecticRef(sd))
    return _cache[name]


def _select_name(fm):
    return _native.kernel_name(fm._net().plan(MODE_STATE, select=True))


def _kind(fm, n):
    return _native.launch_kind(fm._net().plan(MODE_STATE, select=True), n, MODE_STATE)


class _Module64:
    """A torch module's ``forward(t, state, cond)`` in float64 on the CPU, with the ``forward`` of SymplecticRef."""

    def __init__(self, module):
        self.m = copy.deepcopy(module).double().cpu()

    def forward(self, t, state, cond_n=None):
        with torch.no_grad():
            return self.m(torch.tensor(float(t), dtype=torch.float64), state.double(), None if cond_n is None else cond_n.double())


# ---- against the float64 restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("sym_"))
def test_leapfrog_matches_the_float64_restatement(name):
    """_integrate and _sample_from(method="leapfrog") fed the fixture's prior: in-envelope shapes on their mlp_pairsel_*
    kernel without a warning, the out-of-envelope one stepped around torch with a FusedEnvelopeWarning."""
    meta, arrays, fm, ref = _fixture_model(name)
    cond = arrays.get("cond")
    cond_n = ref.norm_cond(cond)
    expect = EXPECTED_KERNEL[name]

    def run():
        out = {}
        for n in STEPS:
            z = fm._integrate(arrays[f"prior_{n}"].to(DEV), _grid(n), fm._norm_cond(_dev(cond)), "leapfrog")
            out[n] = (z, fm._sample_from(arrays[f"prior_{n}"].to(DEV), _dev(cond), n, method="leapfrog"), dict(fm.last_solver_stats))
        return out
    got, warned = _warned(run)
    assert warned == (expect is None)
    if expect is not None:
        assert _select_name(fm) == expect.replace("mlp_pair_", "mlp_pairsel_")
    for n in STEPS:
        want = leapfrog_f64(ref, arrays[f"prior_{n}"], _grid(n), cond_n)
        z, s, stats = got[n]
        assert z.shape == want.shape and s.shape == (want.shape[0], meta["D"])
        print(f"\n[{name}] leapfrog, {n} steps: state {_state_err(z, want):.3e}")
        assert _state_err(z, want) < STATE_TOL, (n, _state_err(z, want))
        assert _state_err(s, want[:, :meta["D"]] * ref.scale + ref.shift) < STATE_TOL, n
        assert stats["evaluations"] == 2 * n + 1 and (stats.get("launches") == 1) == (expect is not None)


def test_generic_route_tanh_and_foreign_modules():
    """A non-SiLU SymplecticMLP (FusedEnvelopeWarning; one network evaluated per sub-step) and a module that is not a
    SymplecticMLP (evaluated whole, the needed half taken): leapfrog stepped by the library around torch."""
    torch.manual_seed(51)
    D, C = 3, 2
    m = SymplecticMLP(D, C, 4, [32, 24], activation=torch.nn.Tanh())
    fm = SymplecticFlowModel(m, torch.randn(D) * 0.3, torch.rand(D) + 0.5, torch.randn(C), torch.rand(C) + 0.5).to(DEV)

    class Other(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin_q, self.lin_p = torch.nn.Linear(D + 1, D), torch.nn.Linear(D + 1, D)

        def forward(self, t, state, conditional):                    # separable, like every field leapfrog is meant for
            q, p = torch.chunk(state, 2, dim=-1)
            tc = t.reshape(-1, 1).expand(state.shape[0], 1)
            return torch.cat([torch.tanh(self.lin_q(torch.cat([p, tc], dim=1))), torch.sin(self.lin_p(torch.cat([q, tc], dim=1)))], dim=1)
    fo = SymplecticFlowModel(Other(), torch.zeros(D), torch.ones(D), None, None).to(DEV)
    z0 = torch.randn(33, 2 * D)
    cond_n = torch.randn(33, C)
    for model, c, warns in ((fm, cond_n, True), (fo, None, False)):
        for n in (1, 4):
            got, warned = _warned(lambda: model._integrate(z0.to(DEV), _grid(n), _dev(c), "leapfrog"))
            assert warned == (warns and n == 1)              # said once per network
            want = leapfrog_f64(_Module64(model.model), z0, _grid(n), c)
            assert _state_err(got, want) < STATE_TOL, (warns, n, _state_err(got, want))
            assert model.last_solver_stats == {"evaluations": 2 * n + 1}
        assert not model._fusable()


# ---- known answer, independent of every restatement --------------------------------------------------------------------
def shear_product(z, D, alpha, beta, grid):
    """Leapfrog of v = [alpha p, -beta q] in closed form: per step the shears p -= (h/2) beta q, q += h alpha p,
    p -= (h/2) beta q with h = t_{k+1} - t_k on the fp32 grid, in float64."""
    z = z.double()
    q, p = z[:, :D].clone(), z[:, D:].clone()
    g = [float(v) for v in grid]
    for k in range(len(g) - 1):
        h = g[k + 1] - g[k]
        p = p - 0.5 * h * beta * q
        q = q + h * alpha * p
        p = p - 0.5 * h * beta * q
    return torch.cat([q, p], dim=1)


@pytest.mark.parametrize("D,C,units", [(5, 3, [32, 32, 32]), (16, 0, [256, 256]), (2, 0, [64]), (16, 0, [256])])
def test_known_answer_rotation(D, C, units):
    """One, two and three hidden layers (the twin's exchange-buffer parity after a row has both outcomes); B = 257 takes
    the twin by default at widths 128 and 256."""
    fm, shift, scale = _rotation_model(D, C, 6, units, 0.7, 1.3)
    assert fm._fusable() and _select_name(fm).startswith("mlp_pairsel_")
    B = 257
    prior = torch.randn(B, 2 * D)
    cond = torch.randn(B, C, device=DEV) if C else None
    for n in STEPS:
        got = fm._integrate(prior.to(DEV), _grid(n), fm._norm_cond(cond), "leapfrog")
        want = shear_product(prior, D, 0.7, 1.3, _grid(n))
        assert _state_err(got, want) < STATE_TOL, (n, _state_err(got, want))
        got = fm._sample_from(prior.to(DEV), cond, n, method="leapfrog")
        assert _state_err(got, want[:, :D] * scale + shift) < STATE_TOL, n


def test_batch_of_2_20_known_answer():
    D, units = 16, [256, 256]
    fm, shift, scale = _rotation_model(D, 0, 16, units, 0.7, 1.3)
    prior = torch.randn(1 << 20, 2 * D, device=DEV)
    assert _kind(fm, 1 << 20) == _native.LAUNCH_ONE_WAVE
    got = fm._integrate(prior, _grid(4), None, "leapfrog")
    want = shear_product(prior.cpu(), D, 0.7, 1.3, _grid(4))
    assert _state_err(got, want) < STATE_TOL


# ---- the discrete map inverts exactly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IN_ENVELOPE)
def test_round_trip(name):
    """Forward on linspace(1, 0, n + 1), back on the flipped grid: the prior again within (2n + 1) 2^-23 max(|z_start|,
    |z_end|) absolute -- every undone sub-step recomputes bitwise the same network output from an untouched half, so it
    costs at most two roundings of the updated half.  Euler's round trip at n = 25 is more than 100 times that bound off."""
    meta, arrays, fm, ref = _fixture_model(name)
    cond_n = fm._norm_cond(_dev(arrays.get("cond")))
    for n in (1, 4, 25, 100):
        z0 = arrays[f"prior_{min(n, 25)}"].to(DEV)
        z1 = fm._integrate(z0, _grid(n), cond_n, "leapfrog")
        back = fm._integrate(z1, _grid(n).flip(0), cond_n, "leapfrog")
        bound = (2 * n + 1) * 2.0 ** -23 * max(float(z0.abs().max()), float(z1.abs().max()))
        err = float((back - z0).abs().max())
        print(f"\n[{name}] round trip, {n} steps: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (n, err, bound)
        if n == 25:
            e1 = fm._integrate(z0, _grid(n), cond_n, "euler")
            eback = fm._integrate(e1, _grid(n).flip(0), cond_n, "euler")
            eerr = float((eback - z0).abs().max())
            print(f"[{name}] Euler round trip, 25 steps: {eerr:.3e}")
            assert eerr > 100 * bound, (eerr, bound)


# ---- log_prob ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("sym_"))
def test_log_prob_against_the_restatement(name):
    meta, arrays, fm, ref = _fixture_model(name)
    B, D = 12, meta["D"]
    torch.manual_seed(11)
    x = arrays["sample_4"][:B]
    p0 = torch.randn(B, D)
    cond = arrays.get("cond")
    cond = None if cond is None else cond[:B]
    for n in (25, 100):
        want = ref._log_prob(x, p0, cond, lambda z0, cond_n: leapfrog_f64(ref, z0, _grid(n).flip(0), cond_n))
        lp = _warned(lambda: fm._log_prob_from(x.to(DEV), p0.to(DEV), _dev(cond), method="leapfrog", num_steps=n))[0]
        assert lp.shape == (B,)
        print(f"\n[{name}] leapfrog log_prob, {n} steps: {_logp_err(lp, want):.3e}")
        assert _logp_err(lp, want) < 2e-5, (n, _logp_err(lp, want))
        stats = fm.last_solver_stats
        assert "chunks" not in stats and "attempts" not in stats and stats["evaluations"] == 2 * n + 1, stats


@pytest.mark.parametrize("name", IN_ENVELOPE)
def test_log_prob_is_the_density_of_what_sample_applies(name):
    """z = leapfrog(z1) forward, x = q scale + shift, p0 = z's p half: log_prob(x; p0) = log N(z1) - log N(p0) -
    sum log scale -- the inverse map lands on z1 again."""
    meta, arrays, fm, ref = _fixture_model(name)
    cond = _dev(arrays.get("cond"))
    D = meta["D"]
    logn = lambda z: (-0.5 * z.double() ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
    for n in (25, 100):
        z1 = arrays["prior_25"].to(DEV)
        z = fm._integrate(z1, _grid(n), fm._norm_cond(cond), "leapfrog")
        x, p0 = z[:, :D] * fm.scale + fm.shift, z[:, D:].contiguous()
        lp = fm._log_prob_from(x, p0, cond, method="leapfrog", num_steps=n)
        want = logn(z1) - logn(p0) - torch.log(fm.scale.double()).sum()
        assert _logp_err(lp, want) < 2e-5, (n, _logp_err(lp, want))


# ---- raw launches: the row order is data -------------------------------------------------------------------------------
def select_launch(plan, wpack, x, table, cond=None, mode=MODE_STATE, k1=None, n_aux=0, status=None, gate=None, lib=None, **env):
    """One raw ff_mlp_ode_launch on a select plan (through library `lib`, default the product); returns (return code,
    x_out pre-filled with -123)."""
    out = torch.full_like(x, -123.0)
    aux = torch.empty_like(x)
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab = x.data_ptr(), out.data_ptr(), wpack.data_ptr(), table.data_ptr()
    a.batch, a.n_evals, a.mode, a.stage_slots = x.shape[0], table.shape[0], mode, 0
    if mode != MODE_STATE:
        a.probe, a.dlogp_out = aux.data_ptr(), aux.data_ptr()
    if cond is not None:
        a.cond = cond.data_ptr()
    if k1 is not None:
        a.k1_in = k1.data_ptr()
    if n_aux:
        a.n_aux = n_aux
        a.aux_out[0] = aux.data_ptr()
    if status is not None:
        a.status = status.data_ptr()
    if gate is not None:
        a.gate = gate.data_ptr()
    with pinned(**env):
        rc = (lib or _native.lib()).ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out


def hand_table(fm, selections):
    """Rows with the given network selections ("A" / "B"), distinct times and weights, every row a step end."""
    n = len(selections)
    H = int(fm._net().plan(MODE_STATE, select=True).width)
    t = torch.tensor([0.11, 0.83, 0.37, 0.59, 0.05, 0.71][:n])
    _, _, c1 = fm._schedule(t)
    rows = torch.zeros(n, 32 + H)
    ints = rows.view(torch.int32)
    rows[:, 1] = 1.0
    for e, s in enumerate(selections):
        ints[e, 3] = 1 | (NET_B if s == "B" else 0)
        rows[e, 16] = 0.05 + 0.03 * e
        rows[e, 32:] = c1[e, H:] if s == "B" else c1[e, :H]
    return rows


@pytest.mark.parametrize("D,C,units,twin", [(16, 3, [256, 200], True), (2, 0, [64], False)], ids=["256", "64"])
def test_rows_select_their_network_in_any_order(D, C, units, twin):
    fm = seeded_model(D, C, units, 52)
    net = fm._net()
    plan, wpack = net.plan(MODE_STATE, select=True), net.wpack(DEV, MODE_STATE)
    assert _native.kernel_name(plan).startswith(f"mlp_pairsel_m{16 if twin else 32}_h{256 if twin else 64}_")
    torch.manual_seed(53)
    B = 77
    x = torch.randn(B, 2 * D)
    cond = torch.randn(B, C) if C else None
    for sel in ("AABBBA", "AABBAB"):                          # the look-ahead past the last row, after an A and after a B
        tab = hand_table(fm, sel)
        want = emulate_select(plan, net.wpack("cpu", MODE_STATE), tab, x, cond)
        for coop in ((0, 1) if twin else (0,)):
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            rc, got = select_launch(plan, wpack, x.to(DEV), tab.to(DEV), _dev(cond), status=status, FF_COOP=coop)
            assert rc == 0
            assert _state_err(got, want) < STATE_TOL, (sel, coop, _state_err(got, want))
            assert int(status.item()) == 0
    # the two tables differ in their last two rows only, and the results differ: the flag, not the position, selects
    tab = hand_table(fm, "AABBBA").to(DEV)
    xd, cd = x.to(DEV), _dev(cond)
    assert not torch.equal(select_launch(plan, wpack, xd, tab, cd)[1], select_launch(plan, wpack, xd, hand_table(fm, "AABBAB").to(DEV), cd)[1])
    # refusals
    assert select_launch(plan, wpack, xd, tab, cd, mode=_native.MODE_HUTCH)[0] == _native.FF_ERR_BADARG
    assert select_launch(plan, wpack, xd, tab, cd, k1=torch.zeros_like(xd))[0] == _native.FF_ERR_BADARG
    assert select_launch(plan, wpack, xd, tab, cd, n_aux=1)[0] == _native.FF_ERR_BADARG
    # a closed gate leaves x_out untouched
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc, out = select_launch(plan, wpack, xd, tab, cd, gate=gate)
    assert rc == 0 and out.eq(-123.0).all()
    gate.fill_(1)
    rc, out = select_launch(plan, wpack, xd, tab, cd, gate=gate)
    assert rc == 0 and torch.equal(out, select_launch(plan, wpack, xd, tab, cd)[1])


# ---- the cooperative twin ------------------------------------------------------------------------------------------------
# (D, C, units, select kernel): even layer count; odd, full conditional width; ragged on the 128-wide instance; one hidden layer
TWIN_CASES = [(16, 0, [256] * 2, "mlp_pairsel_m16_h256_d8_c4_w2"), (16, 16, [256] * 3, "mlp_pairsel_m16_h256_d8_c4_w2"),
              (5, 3, [128, 100], "mlp_pairsel_m16_h128_d8_c4_w3"), (2, 0, [128], "mlp_pairsel_m16_h128_d8_c4_w3")]
TWIN_IDS = ["16d_2x256", "16d_c16_3x256", "5d_c3_ragged128", "2d_1x128"]


@pytest.mark.parametrize("D,C,units,kernel", TWIN_CASES, ids=TWIN_IDS)
def test_twin_equals_one_wavefront_kernel_bitwise(D, C, units, kernel):
    fm = seeded_model(D, C, units, 54)
    assert fm._fusable() and _select_name(fm) == kernel
    net = fm._net()
    table = fm._leapfrog_table(_grid(4)).to(DEV)
    torch.manual_seed(55)
    affine = dict(zip(("in_shift", "in_scale", "out_scale", "out_shift"),
                      (t.to(DEV) for t in (torch.randn(2 * D) * 0.1, torch.rand(2 * D) + 0.5, torch.rand(2 * D) + 0.5, torch.randn(2 * D) * 0.1))))
    for B in (1, 17, 257, 4099):
        z = torch.randn(B, 2 * D, device=DEV)
        cond = torch.randn(B, C, device=DEV) if C else None
        for maps in ({}, affine):
            with pinned(FF_COOP=0):
                assert _kind(fm, B) == _native.LAUNCH_ONE_WAVE
                one = net.integrate_select(z, table, cond=cond, **maps)[0]
            with pinned(FF_COOP=1):
                assert _kind(fm, B) == _native.LAUNCH_TWIN
                twin = net.integrate_select(z, table, cond=cond, **maps)[0]
            assert torch.isfinite(one).all() and torch.equal(twin, one), (B, bool(maps))
        with pinned(FF_COOP=0):
            assert torch.equal(net.integrate_select(z, table, cond=cond)[0], fm._integrate(z, _grid(4), cond, "leapfrog"))


@pytest.mark.parametrize("units,chip", [([256] * 3, 2048), ([128] * 3, 3072)])
def test_tail_split_is_bitwise(units, chip):
    """One round of the one-wavefront kernel and 37 tiles: the leftover rows on the twin as a second launch, the same rows."""
    D, C = 16, 4
    B = (chip + 37) * 16
    fm = seeded_model(D, C, units, 56)
    torch.manual_seed(57)
    z, cond = torch.randn(B, 2 * D, device=DEV), torch.randn(B, C, device=DEV)
    res = {}
    for split in (0, None):
        with pinned(FF_TAIL_SPLIT=split):
            assert _kind(fm, B) == (_native.LAUNCH_ONE_WAVE if split == 0 else _native.LAUNCH_ONE_WAVE_AND_TWIN)
            res[split] = fm._integrate(z, _grid(4), cond, "leapfrog")
    assert torch.isfinite(res[0]).all() and torch.equal(res[None], res[0])


def test_default_dispatch():
    """Asked of the launcher's own rule (ff_mlp_launch_kind), not of a clock."""
    assert "FF_COOP" not in os.environ and "FF_TAIL_SPLIT" not in os.environ
    for units in ([256] * 2, [128] * 2):
        fm = seeded_model(16, 0, units, 58)
        assert _kind(fm, 2048) == _native.LAUNCH_TWIN
        assert _kind(fm, 1 << 20) == _native.LAUNCH_ONE_WAVE
    fm = seeded_model(2, 0, [64], 58)
    for n in (1, 2048, 1 << 20):
        assert _kind(fm, n) == _native.LAUNCH_ONE_WAVE
    with pinned(FF_COOP=1):
        assert _kind(fm, 2048) == _native.LAUNCH_ONE_WAVE


# ---- invariances -------------------------------------------------------------------------------------------------------
def test_rerun_slices_draws_and_the_euler_default():
    meta, arrays, fm, ref = _fixture_model("sym_16d_2x256")
    D = meta["D"]
    torch.manual_seed(14)
    prior = torch.randn(4099, 2 * D, device=DEV)
    a = fm._integrate(prior, _grid(4), None, "leapfrog")
    assert torch.equal(a, fm._integrate(prior, _grid(4), None, "leapfrog"))                      # bitwise re-run
    for lo, hi in ((0, 1), (1000, 1017), (4000, 4099)):                                        # rows are independent
        assert torch.equal(fm._integrate(prior[lo:hi].contiguous(), _grid(4), None, "leapfrog"), a[lo:hi])
    x = a[:300, :D] * fm.scale + fm.shift
    p0 = a[:300, D:].contiguous()
    lp = fm._log_prob_from(x, p0, method="leapfrog", num_steps=4)
    for lo, hi in ((0, 1), (100, 117)):
        assert torch.equal(fm._log_prob_from(x[lo:hi].contiguous(), p0[lo:hi].contiguous(), method="leapfrog", num_steps=4), lp[lo:hi])
    # the public methods draw what sample / log_prob draw, in their order, on the model's device
    torch.manual_seed(3)
    x0 = torch.randn(33, 2 * D, device=DEV)
    torch.manual_seed(3)
    assert torch.equal(fm.sample_leapfrog((33, D), num_steps=4), fm._sample_from(x0, None, 4, method="leapfrog"))
    xs = arrays["sample_4"].to(DEV)
    torch.manual_seed(4)
    pd = torch.randn_like(xs)
    torch.manual_seed(4)
    assert torch.equal(fm.log_prob_leapfrog(xs, num_steps=4), fm._log_prob_from(xs, pd, method="leapfrog", num_steps=4))
    # the Euler default is what it was
    torch.manual_seed(3)
    assert torch.equal(fm.sample((33, D), num_steps=4), fm._sample_from(x0, None, 4))
    assert torch.equal(fm._sample_from(x0, None, 4), fm._sample_from(x0, None, 4, method="euler"))
    assert not torch.equal(fm._sample_from(x0, None, 4), fm._sample_from(x0, None, 4, method="leapfrog"))


def test_sharded_entry_points_on_one_gpu():
    """World 1, no process group: the sharded functions are the unsharded ones on the library's counter-based draws, and a
    shard computed alone from its own rows of the stream equals those rows of the full run."""
    D, C = 5, 3
    fm = seeded_model(D, C, [128, 100], 59)
    n, seed = 300, 17
    torch.manual_seed(60)
    cond = torch.randn(n, C, device=DEV)
    full = symplectic_sample_sharded(fm, n, seed=seed, conditional=cond, num_steps=4, method="leapfrog")
    assert full.shape == (n, D)
    assert torch.equal(full, fm._sample_from(_native.normal_fill(n, 2 * D, seed, 0, DEV), cond, 4, method="leapfrog"))
    for lo, hi in ((0, 38), (262, 300)):
        alone = fm._sample_from(_native.normal_fill(hi - lo, 2 * D, seed, lo, DEV), cond[lo:hi].contiguous(), 4, method="leapfrog")
        assert torch.equal(alone, full[lo:hi])
    x = torch.randn(n, D, device=DEV)
    lp = symplectic_log_prob_sharded(fm, x, cond, seed=seed + 1, method="leapfrog", num_steps=25)
    assert lp.shape == (n,) and torch.isfinite(lp).all()
    assert torch.equal(lp, fm._log_prob_from(x, _native.normal_fill(n, D, seed + 1, 0, DEV), cond, method="leapfrog", num_steps=25))
    assert torch.equal(symplectic_log_prob_sharded(fm, local_x=x, local_conditional=cond, n_total=n, seed=seed + 1,
                                                   method="leapfrog", num_steps=25, global_control=False), lp)
    for lo, hi in ((0, 38), (262, 300)):
        alone = fm._log_prob_from(x[lo:hi].contiguous(), _native.normal_fill(hi - lo, D, seed + 1, lo, DEV), cond[lo:hi].contiguous(),
                                  method="leapfrog", num_steps=25)
        assert torch.equal(alone, lp[lo:hi])
