"""GPU tier: the cooperative twin of the two-network kernels (csrc/ff_mlp_pair.hpp, COOP) and the launcher's choice between
it and the one-wavefront kernel.

The twin computes the same fp32 FMA chains in the same order, so everything here that compares the two kernels asks for
bitwise equality; that the twin is also RIGHT is asked of the anchors of tests/test_gpu_symplectic.py with FF_COOP=1 (the
reference's samples, scipy on the float64 restatement, the closed-form rotation)."""
import ctypes
import math
import os

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.distributed import symplectic_log_prob_sharded, symplectic_sample_sharded
from flowfusion_amd.fused import MODE_STATE
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
from tests._symplectic_ref import SymplecticRef, euler_rotation, rotation_weights
from tests._util import load_golden, max_rel
from tests.test_symplectic_host import EXPECTED_KERNEL, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE_TOL = 2e-5        # relative to max |reference state| (tests/test_gpu_symplectic.py)

# (D, C, units, kernel): even layer count; odd, full conditional width; ragged on the 128-wide instance; one hidden layer
CASES = [(16, 0, [256] * 2, "mlp_pair_m16_h256_d8_c4_w2"), (16, 16, [256] * 3, "mlp_pair_m16_h256_d8_c4_w2"),
         (5, 3, [128, 100], "mlp_pair_m16_h128_d8_c4_w3"), (2, 0, [128], "mlp_pair_m16_h128_d8_c4_w3")]
CASE_IDS = ["16d_2x256", "16d_c16_3x256", "5d_c3_ragged128", "2d_1x128"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"


class pinned:
    """FF_COOP / FF_TAIL_SPLIT set (or removed: None) for a block, restored afterwards."""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in ("FF_COOP", "FF_TAIL_SPLIT")}
        for k, v in self.env.items():
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def seeded_model(D, C, units, seed, E=16):
    torch.manual_seed(seed)
    m = SymplecticMLP(D, C, E, units)
    shift, scale = torch.randn(D) * 0.3, torch.rand(D) + 0.5
    cs = (torch.randn(C) * 0.2, torch.rand(C) + 0.5) if C else (None, None)
    return SymplecticFlowModel(m, shift, scale, *cs).to(DEV)


def _state_err(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _logp_err(got, want):
    return max_rel(got.detach().cpu(), want.detach().cpu(), floor=1.0)


def _kind(fm, n):
    return _native.launch_kind(fm._net().plan(MODE_STATE), n, MODE_STATE)


@pytest.mark.parametrize("D,C,units,kernel", CASES, ids=CASE_IDS)
def test_twin_equals_one_wavefront_kernel_bitwise(D, C, units, kernel):
    fm = seeded_model(D, C, units, 31)
    assert fm._fusable() and _native.kernel_name(fm._net().plan(MODE_STATE)) == kernel
    torch.manual_seed(32)
    for B in (1, 77, 4099):
        prior = torch.randn(B, 2 * D, device=DEV)
        cond = torch.randn(B, C, device=DEV) if C else None
        for steps in (1, 4, 25):
            with pinned(FF_COOP=0):
                assert _kind(fm, B) == _native.LAUNCH_ONE_WAVE
                one = fm._sample_from(prior, cond, steps)
            with pinned(FF_COOP=1):
                assert _kind(fm, B) == _native.LAUNCH_TWIN
                twin = fm._sample_from(prior, cond, steps)
            assert torch.isfinite(one).all() and torch.equal(twin, one), (B, steps)
        if B == 4099:
            continue
        x, p0 = torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV)
        # fixed grids with several stage slots (dopri5_fixed: the Dormand-Prince tableau on a fixed grid, all seven), then
        # the default adaptive solve (k1_in and auxiliary outputs per attempt)
        for kw in (dict(method="rk4", options={"step_size": 0.125}), dict(method="dopri5_fixed", options={"step_size": 0.25}), {}):
            res = {}
            for coop in (0, 1):
                with pinned(FF_COOP=coop):
                    lp = fm._log_prob_from(x, p0, cond, **kw)
                    st = dict(fm.last_solver_stats) if not kw else {}
                    res[coop] = (lp, st.get("attempts"), st.get("accepted"))
            assert torch.isfinite(res[0][0]).all() and torch.equal(res[1][0], res[0][0]), (B, kw)
            assert res[1][1:] == res[0][1:], (B, res[0][1:], res[1][1:])
            if not kw:
                assert res[0][1] >= res[0][2] >= 1


def raw_launch(L, plan, wpack, x, table, n_evals, cond=None, k1=None, n_aux=0, noise=None, rng=None, status=None,
               affine=None, **env):
    """One raw ff_mlp_ode_launch of a pair plan through library `L`; returns (x_out, aux_0 or None)."""
    B, D2 = x.shape
    out = torch.full_like(x, -123.0)
    aux = torch.full_like(x, -321.0) if n_aux else None
    a = _native.OdeArgs()
    a.x_in, a.x_out, a.wpack, a.etab = x.data_ptr(), out.data_ptr(), wpack.data_ptr(), table.data_ptr()
    a.batch, a.n_evals, a.mode, a.stage_slots = B, n_evals, MODE_STATE, 0
    if cond is not None:
        a.cond = cond.data_ptr()
    if k1 is not None:
        a.k1_in = k1.data_ptr()
    if n_aux:
        a.n_aux = 1
        a.aux_out[0] = aux.data_ptr()
    if noise is not None:
        a.noise, a.noise_stride = noise.data_ptr(), noise.shape[1] * noise.shape[2]
    if rng is not None:
        a.rng_seed, a.rng_sample_offset, a.rng_noise_base = rng
    if status is not None:
        a.status = status.data_ptr()
    if affine is not None:
        a.in_shift, a.in_scale, a.out_scale, a.out_shift = (t.data_ptr() for t in affine)
    with pinned(**env):
        rc = L.ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, aux


def attempt_table(fm, n_rows, noise_row=None, bad_slot_row=None):
    """Rows as an adaptive attempt has them: stage slot 0 comes in through k1_in, row i fills slot i + 1 from
    y + 0.1 k[0] + 0.05 k[i]; the last row ends a step (x += 0.2 sum_s k[s]); aux_0 = y + 0.2 sum_s k[s].  `noise_row`
    adds 0.3 * noise slab 1 to the state after that row."""
    H = int(fm._net().plan(MODE_STATE).width)
    _, _, c1 = fm._schedule(torch.linspace(0.2, 0.8, n_rows))
    rows = torch.zeros(n_rows + 2, 32 + 2 * H)
    ints = rows.view(torch.int32)
    rows[:n_rows, 1] = 1.0
    for i in range(n_rows):
        ints[i, 4] = i + 1
        rows[i, 8] = 0.1
        if i:
            rows[i, 8 + i] = 0.05
    rows[n_rows - 1, 16:16 + n_rows + 1] = 0.2
    ints[n_rows - 1, 3] = 1
    if noise_row is not None:
        ints[noise_row, 3] |= 2
        ints[noise_row, 5] = 1
        rows[noise_row, 2] = 0.3
    if bad_slot_row is not None:
        ints[bad_slot_row, 4] = 9
    rows[:n_rows, 32:] = c1
    rows[n_rows, 8:8 + n_rows + 1] = 0.2
    ints[n_rows, 3] = 1                                  # use_y of aux_0
    return rows.to(DEV)


@pytest.mark.parametrize("D,C,units,kernel", [CASES[1], CASES[2]], ids=[CASE_IDS[1], CASE_IDS[2]])
def test_raw_launches_noise_rows_affine_maps_and_status(D, C, units, kernel):
    """What no front end of the symplectic flows reaches: noise rows from a buffer and from the in-kernel stream, the
    in_/out_ affine maps, the NaN and bad-slot status bits -- one-wavefront kernel against twin, bitwise."""
    fm = seeded_model(D, C, units, 33)
    net = fm._net()
    plan, wpack, L = net.plan(MODE_STATE), net.wpack(DEV, MODE_STATE), _native.lib()
    torch.manual_seed(34)
    B = 77
    x, k1 = torch.randn(B, 2 * D, device=DEV), torch.randn(B, 2 * D, device=DEV)
    cond = torch.randn(B, C, device=DEV)
    noise = torch.randn(2, B, 2 * D, device=DEV)
    affine = tuple(t.to(DEV).contiguous() for t in (torch.randn(2 * D) * 0.1, torch.rand(2 * D) + 0.5, torch.rand(2 * D) + 0.5,
                                                    torch.randn(2 * D) * 0.1))
    tab = attempt_table(fm, 5, noise_row=2)
    for kw in (dict(noise=noise), dict(rng=(1234, 1000, 3)), dict(noise=noise, affine=affine)):
        one = raw_launch(L, plan, wpack, x, tab, 5, cond=cond, k1=k1, n_aux=1, FF_COOP=0, **kw)
        twin = raw_launch(L, plan, wpack, x, tab, 5, cond=cond, k1=k1, n_aux=1, FF_COOP=1, **kw)
        assert torch.isfinite(one[0]).all() and torch.equal(twin[0], one[0]) and torch.equal(twin[1], one[1]), list(kw)
    plain = raw_launch(L, plan, wpack, x, attempt_table(fm, 5), 5, cond=cond, k1=k1, FF_COOP=1)[0]
    assert not torch.equal(plain, twin[0])                                          # the noise row did something
    # status bits: a row naming a slot beyond those on chip; a NaN in the state
    for tab_bad, xin, bit in ((attempt_table(fm, 5, bad_slot_row=3), x, _native.STATUS_BAD_SLOT),
                              (tab, torch.where(torch.arange(B, device=DEV)[:, None] == 5, float("nan"), x), _native.STATUS_NAN)):
        got = []
        for coop in (0, 1):
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            o = raw_launch(L, plan, wpack, xin.contiguous(), tab_bad, 5, cond=cond, k1=k1, n_aux=1, noise=noise, status=status,
                           FF_COOP=coop)
            got.append((o, int(status.item())))
        assert got[0][1] == got[1][1] == bit
        for u, v in zip(got[0][0], got[1][0]):
            assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0))


@pytest.mark.parametrize("name", ["sym_16d_2x256", "sym_5d_c3_ragged"])
def test_twin_against_the_reference_and_scipy(name):
    """The anchors of tests/test_gpu_symplectic.py with the twin pinned: the reference's samples within STATE_TOL, log_prob
    within the bounds of test_log_prob_against_scipy."""
    meta, arrays = load_golden(name)
    fm, sd = build_model(meta, arrays)
    fm, ref = fm.to(DEV), SymplecticRef(sd)
    assert _native.kernel_name(fm._net().plan(MODE_STATE)) == EXPECTED_KERNEL[name]
    cond = arrays.get("cond")
    with pinned(FF_COOP=1):
        for n in meta["steps"]:
            assert _kind(fm, arrays[f"prior_{n}"].shape[0]) == _native.LAUNCH_TWIN
            got = fm._sample_from(arrays[f"prior_{n}"].to(DEV), None if cond is None else cond.to(DEV), n)
            err = _state_err(got, arrays[f"sample_{n}"])
            print(f"\n[{name}] twin sample, {n} steps: {err:.3e}")
            assert err < STATE_TOL, (n, err)
        B, D = 12, meta["D"]
        torch.manual_seed(11)
        x = arrays["sample_4"][:B]
        p0 = torch.randn(B, D)
        c = None if cond is None else cond[:B]
        want = ref.log_prob_from(x, p0, c)
        run = lambda tol: fm._log_prob_from(x.to(DEV), p0.to(DEV), None if c is None else c.to(DEV), atol=tol, rtol=tol)
        lp = run(1e-6)
        print(f"[{name}] twin log_prob at 1e-6 against scipy: {_logp_err(lp, want):.3e}")
        assert _logp_err(lp, want) < 2e-5, _logp_err(lp, want)
        assert "chunks" in fm.last_solver_stats
        lp = run(1e-5)
        dp5 = ref.log_prob_dopri5(x, p0, c, 1e-5)
        print(f"[{name}] twin log_prob at 1e-5: {_logp_err(lp, dp5):.3e} from dopri5/f64, {_logp_err(lp, want):.3e} from scipy")
        assert _logp_err(lp, dp5) < 2e-5, _logp_err(lp, dp5)
        assert _logp_err(lp, want) < max(2e-4, _logp_err(dp5, want) + 2e-5), (_logp_err(lp, want), _logp_err(dp5, want))


@pytest.mark.parametrize("D,C,units", [(16, 0, [256, 256]), (5, 3, [128, 128, 128])])
def test_twin_known_answer_rotation(D, C, units):
    """test_known_answer_rotation's closed form on the twin: v = [alpha p, -beta q] at any depth."""
    def model(alpha, beta):
        torch.manual_seed(13)
        m = SymplecticMLP(D, C, 6, units)
        m.load_state_dict({**rotation_weights(D, C, 6, units, alpha, beta), "W": m.W}, strict=True)
        shift, scale = torch.randn(D) * 0.3, torch.rand(D) + 0.5
        cs = (torch.randn(C), torch.rand(C) + 0.5) if C else (None, None)
        return SymplecticFlowModel(m, shift, scale, *cs).to(DEV), shift.double(), scale.double()
    B = 257
    with pinned(FF_COOP=1):
        fm, shift, scale = model(0.7, 1.3)
        assert _kind(fm, B) == _native.LAUNCH_TWIN
        prior = torch.randn(B, 2 * D)
        cond = torch.randn(B, C, device=DEV) if C else None
        for n in (1, 4, 25):
            got = fm._sample_from(prior.to(DEV), cond, n)
            want = euler_rotation(prior, D, 0.7, 1.3, n)[:, :D] * scale + shift
            assert _state_err(got, want) < STATE_TOL, (n, _state_err(got, want))
        fm, shift, scale = model(1.1, 1.1)
        x, p0 = torch.randn(B, D), torch.randn(B, D)
        lp = fm._log_prob_from(x.to(DEV), p0.to(DEV), cond, atol=1e-7, rtol=1e-7)
        q0 = (x.double() - shift) / scale
        want = (-0.5 * q0 ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1) - torch.log(scale).sum()
        assert _logp_err(lp, want) < 1e-4, _logp_err(lp, want)


@pytest.mark.parametrize("units,B", [([256] * 3, 2048 * 16 + 300), ([128] * 3, 3072 * 16 + 120)])
def test_tail_split_is_bitwise(units, B):
    """Whole rounds on the one-wavefront kernel and the leftover rows on the twin as a second launch: the same rows."""
    D, C = 16, 4
    fm = seeded_model(D, C, units, 35)
    torch.manual_seed(36)
    prior, cond = torch.randn(B, 2 * D, device=DEV), torch.randn(B, C, device=DEV)
    x, p0 = torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV)
    res = {}
    for split in (0, None):
        with pinned(FF_TAIL_SPLIT=split):
            assert _kind(fm, B) == (_native.LAUNCH_ONE_WAVE if split == 0 else _native.LAUNCH_ONE_WAVE_AND_TWIN)
            s = fm._sample_from(prior, cond, 4)
            lp = fm._log_prob_from(x, p0, cond)
            res[split] = (s, lp, fm.last_solver_stats["attempts"], fm.last_solver_stats["accepted"])
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[None][0], res[0][0]) and torch.equal(res[None][1], res[0][1])
    assert res[None][2:] == res[0][2:]


def test_small_batches_take_the_pair_twin_by_default():
    """Default dispatch asked of the launcher's own rule (ff_mlp_launch_kind), not of a clock; the adaptive log_prob's
    attempts go through the same launcher.  HIP-event times of both kernels are printed for the record."""
    fm = seeded_model(16, 0, [256] * 3, 37)
    assert "FF_COOP" not in os.environ and "FF_TAIL_SPLIT" not in os.environ
    assert _kind(fm, 2048) == _native.LAUNCH_TWIN
    assert _kind(fm, 1 << 20) == _native.LAUNCH_ONE_WAVE
    assert _kind(fm, 2048 * 16 + 300) == _native.LAUNCH_ONE_WAVE_AND_TWIN
    torch.manual_seed(38)
    prior = torch.randn(2048, 32, device=DEV)
    x, p0 = torch.randn(2048, 16, device=DEV), torch.randn(2048, 16, device=DEV)

    def timed(fn):
        fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    jobs = {"sample, 100 steps": lambda: fm._sample_from(prior, None, 100), "log_prob": lambda: fm._log_prob_from(x, p0)}
    for what, fn in jobs.items():
        out_def, ms_def = timed(fn)
        with pinned(FF_COOP=0):
            assert _kind(fm, 2048) == _native.LAUNCH_ONE_WAVE
            out_one, ms_one = timed(fn)
        assert torch.equal(out_def, out_one)
        print(f"\n[pair twin] 2048 x {what} (HIP events): default = twin {ms_def:.2f} ms, one-wavefront kernel {ms_one:.2f} ms "
              f"({ms_one / ms_def:.2f}x)")


def test_sharded_entry_points_on_one_gpu():
    """World 1, no process group: the sharded functions are the unsharded ones on the library's counter-based draws, and a
    shard computed alone from its own rows of the stream equals those rows of the full run."""
    D, C = 5, 3
    fm = seeded_model(D, C, [128, 100], 39)
    n, seed = 300, 17
    torch.manual_seed(40)
    cond = torch.randn(n, C, device=DEV)
    full = symplectic_sample_sharded(fm, n, seed=seed, conditional=cond, num_steps=4)
    assert full.shape == (n, D)
    assert torch.equal(full, fm._sample_from(_native.normal_fill(n, 2 * D, seed, 0, DEV), cond, 4))
    for lo, hi in ((0, 38), (38, 75), (262, 300)):
        alone = fm._sample_from(_native.normal_fill(hi - lo, 2 * D, seed, lo, DEV), cond[lo:hi].contiguous(), 4)
        assert torch.equal(alone, full[lo:hi])
    local, span = symplectic_sample_sharded(fm, n, seed=seed, local_conditional=cond, num_steps=4, gather=False)
    assert span == (0, n) and torch.equal(local, full)
    x = torch.randn(n, D, device=DEV)
    lp = symplectic_log_prob_sharded(fm, x, cond, seed=seed + 1)
    assert lp.shape == (n,) and torch.isfinite(lp).all()
    assert torch.equal(lp, fm._log_prob_from(x, _native.normal_fill(n, D, seed + 1, 0, DEV), cond))
    assert torch.equal(symplectic_log_prob_sharded(fm, local_x=x, local_conditional=cond, n_total=n, seed=seed + 1), lp)
