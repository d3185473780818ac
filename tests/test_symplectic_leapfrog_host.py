"""Leapfrog for the symplectic flows without a GPU: the table of solvers.plan_leapfrog, the select planner, the select
rows' semantics on the packed weights (a float64 emulation of the row-select loop against a float64 leapfrog written on
the restatement's dynamics, and its order against scipy), the API's errors, and the sharded entry points over gloo."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flowfusion_amd import _native, solvers
from flowfusion_amd.distributed import shard_bounds
from flowfusion_amd.fused import MODE_STATE
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
from tests._emulator import decode_wpack
from tests._symplectic_ref import SymplecticRef
from tests._util import load_golden
from tests.test_distributed_gloo import _cpu_normal_fill, _free_port
from tests.test_symplectic_host import EXPECTED_KERNEL, build_model

IN_ENVELOPE = [k for k, v in sorted(EXPECTED_KERNEL.items()) if v]
NET_B = 4           # FF_ROW_NET_B
_cache = {}


def leapfrog_f64(ref, z, grid, cond_n=None):
    """Kick-drift-kick leapfrog of v = [mlp_q(p), -mlp_p(q)] over the fp32 nodes ``grid``, in float64, written on
    ``SymplecticRef.forward`` and on nothing of the product: per step half a kick of p at t_k, a drift of q at the
    midpoint, half a kick of p at t_{k+1} (no merging of adjacent half-kicks)."""
    z = z.double().clone()
    D = z.shape[1] // 2
    g = [float(v) for v in grid]
    for k in range(len(g) - 1):
        h = g[k + 1] - g[k]
        z[:, D:] += 0.5 * h * ref.forward(g[k], z, cond_n)[:, D:]
        z[:, :D] += h * ref.forward(0.5 * (g[k] + g[k + 1]), z, cond_n)[:, :D]
        z[:, D:] += 0.5 * h * ref.forward(g[k + 1], z, cond_n)[:, D:]
    return z


def emulate_select(plan, wpack, table, x, cond):
    """The row-select kernel's evaluation loop in float64: ONE network per row, chosen by the row's flag word, its c1
    the only one the row carries; each half decoded by tests/_emulator.decode_wpack as _emulate_pair does."""
    words = _native.plan_words(plan)
    n = wpack.numel() // 2
    halves = [decode_wpack(words, wpack[:n]), decode_wpack(words, wpack[n:])]
    H, D2 = plan.width, plan.dim
    assert table.shape[1] == 32 + H
    rows = table.double()
    ints = table.view(torch.int32)
    B = x.shape[0]
    ks = torch.zeros(7, B, D2, dtype=torch.float64)
    x = x.double()
    for e in range(table.shape[0]):
        y = x + sum(rows[e, 8 + s] * ks[s] for s in range(7))
        W1, hidden, Wo, bo, dx = halves[1 if int(ints[e, 3]) & NET_B else 0]
        inp = torch.zeros(B, W1.shape[1], dtype=torch.float64)
        inp[:, :D2] = y
        if cond is not None:
            inp[:, dx:dx + cond.shape[1]] = cond.double()
        h = inp @ W1.T + rows[e, 32:32 + H]
        h = h * torch.sigmoid(h)
        for Wl, bl in hidden:
            h = h @ Wl.T + bl
            h = h * torch.sigmoid(h)
        net = (h @ Wo.T + bo)[:, :D2]
        ks[int(ints[e, 4])] = rows[e, 0] * y + rows[e, 1] * net
        if int(ints[e, 3]) & 1:
            x = x + sum(rows[e, 16 + s] * ks[s] for s in range(7))
    return x


def fixture(name):
    if name not in _cache:
        meta, arrays = load_golden(name)
        fm, sd = build_model(meta, arrays)
        _cache[name] = (meta, arrays, fm, SymplecticRef(sd))
    return _cache[name]


@pytest.mark.parametrize("n", [1, 2, 5])
def test_table_of_plan_leapfrog(n):
    grid = torch.linspace(1.0, 0.0, n + 1)
    p = solvers.plan_leapfrog(grid)
    assert p.sign == -1.0 and p.n_steps == n and p.t_eval.numel() == 2 * n + 1
    s = -grid                                            # solver time
    h = s[1:] - s[:-1]
    want_t, want_w, want_f = [grid[0]], [h[0] / 2], [1 | NET_B]
    for k in range(n):
        want_t += [(grid[k] + grid[k + 1]) / 2, grid[k + 1]]
        want_w += [h[k], (h[k] + h[k + 1]) / 2 if k + 1 < n else h[n - 1] / 2]
        want_f += [1, 1 | NET_B]
    assert torch.equal(p.t_eval, torch.stack(want_t))
    assert torch.equal(p.cout[:, 0], torch.stack(want_w)) and p.cout[:, 1:].eq(0).all() and p.cin.eq(0).all()
    assert p.flags.tolist() == want_f and p.slot.eq(0).all()
    back = solvers.plan_leapfrog(grid.flip(0))
    assert back.sign == 1.0
    assert torch.equal(back.t_eval, p.t_eval.flip(0))
    assert torch.equal(back.cout[:, 0].abs(), p.cout[:, 0].abs().flip(0))
    assert back.flags.tolist() == p.flags.flip(0).tolist()
    for bad in (torch.tensor([0.5]), torch.tensor([0.0, 0.5, 0.5, 1.0])):
        with pytest.raises(ValueError):
            solvers.plan_leapfrog(bad)


def test_leapfrog_table_rows_carry_the_selected_c1():
    meta, arrays, fm, ref = fixture("sym_5d_c3_ragged")
    grid = torch.linspace(1.0, 0.0, 4)
    table = fm._leapfrog_table(grid)
    plan = solvers.plan_leapfrog(grid)
    H = fm._net().plan(MODE_STATE, select=True).width
    assert table.shape == (7, 32 + H) and fm._net().width(MODE_STATE, select=True) == H
    _, _, c1 = fm._schedule(plan.t_eval)
    ints = table.view(torch.int32)
    for e in range(7):
        b = bool(int(ints[e, 3]) & NET_B)
        assert b == (e % 2 == 0)
        assert torch.equal(table[e, 32:], c1[e, H:] if b else c1[e, :H])
    assert table[:, 0].eq(0).all() and table[:, 1].eq(-1).all()


def test_select_planner():
    """The envelope test_planner_envelope lists for the pair planner, shape for shape; names; the tables stay as they are."""
    L = _native.lib()
    assert L.ff_pair_kernel_count() == 3
    assert not any(L.ff_kernel_name(i).decode().startswith("mlp_pair") for i in range(L.ff_kernel_count()))
    for dim, c, u in [(2, 0, [64]), (32, 16, [256, 256]), (10, 3, [100, 128]), (32, 0, [128] * 3), (4, 16, [64])]:
        pair, sel = _native.make_pair_plan(dim, c, u), _native.make_pair_plan(dim, c, u, select=True)
        assert sel.kernel_id - _native.PAIR_SELECT_KERNEL_BASE == pair.kernel_id - _native.PAIR_KERNEL_BASE
        assert (sel.width, sel.tile, sel.dregs, sel.cregs, sel.n_hidden) == (pair.width, pair.tile, pair.dregs, pair.cregs, pair.n_hidden)
        name = _native.kernel_name(sel)
        assert name.startswith("mlp_pairsel_") and name == _native.kernel_name(pair).replace("mlp_pair_", "mlp_pairsel_")
        assert _native.is_select_plan(sel) and not _native.is_select_plan(pair)
        assert _native.row_width(sel) == sel.width and _native.row_width(pair) == 2 * pair.width
        assert L.ff_mlp_pair_wpack_floats(sel) == L.ff_mlp_pair_wpack_floats(pair) > 0
        assert L.ff_mlp_wpack_floats(sel) == 0
        assert L.ff_mlp_samples_per_workgroup(sel, _native.MODE_STATE) == 4 * sel.tile
        for mode in (_native.MODE_HUTCH, _native.MODE_EXACT):
            assert L.ff_mlp_samples_per_workgroup(sel, mode) == _native.FF_ERR_BADARG
            with pytest.raises(RuntimeError):
                _native.launch_kind(sel, 77, mode)
    for dim, c, u in [(34, 0, [64]), (8, 17, [64]), (8, 0, [257])]:
        with pytest.raises(NotImplementedError):
            _native.make_pair_plan(dim, c, u, select=True)
    with pytest.raises(RuntimeError):
        _native.make_pair_plan(5, 0, [64], select=True)


@pytest.mark.parametrize("units,chip", [([256, 256], 2048), ([128, 128], 3072)])
def test_launch_kind_of_select_plans(monkeypatch, units, chip):
    monkeypatch.delenv("FF_COOP", raising=False)
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    plan = _native.make_pair_plan(32, 0, units, select=True)
    kind = lambda n: _native.launch_kind(plan, n, _native.MODE_STATE)
    assert kind(2048) == _native.LAUNCH_TWIN and kind(1 << 20) == _native.LAUNCH_ONE_WAVE
    monkeypatch.setenv("FF_COOP", "0")
    assert kind(2048) == _native.LAUNCH_ONE_WAVE
    monkeypatch.setenv("FF_COOP", "1")
    assert kind(1 << 20) == _native.LAUNCH_TWIN
    monkeypatch.delenv("FF_COOP")
    p64 = _native.make_pair_plan(4, 0, [64], select=True)
    for pin in (None, "1"):
        if pin:
            monkeypatch.setenv("FF_COOP", pin)
        assert _native.launch_kind(p64, 2048, _native.MODE_STATE) == _native.LAUNCH_ONE_WAVE
        assert _native.launch_kind(p64, 1 << 20, _native.MODE_STATE) == _native.LAUNCH_ONE_WAVE


def test_select_wpack_is_the_pair_wpack():
    meta, arrays, fm, ref = fixture("sym_5d_c3_ragged")
    net = fm._net()
    pair, sel = net.plan(MODE_STATE), net.plan(MODE_STATE, select=True)
    a = _native.pack_pair_weights(pair, net.linears, net.p_linears, net.hidden, net.x_col0, net.c_col0)
    b = _native.pack_pair_weights(sel, net.linears, net.p_linears, net.hidden, net.x_col0, net.c_col0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", IN_ENVELOPE)
def test_select_rows_on_the_pack_are_a_leapfrog(name):
    """The product's own leapfrog table run through the float64 emulation of the select loop on the product's packed
    weights, against the float64 leapfrog on the restatement's dynamics: 2e-5 of max |state| (the fp32 table and weights
    against float64 ones)."""
    meta, arrays, fm, ref = fixture(name)
    net = fm._net()
    plan = net.plan(MODE_STATE, select=True)
    wpack = net.wpack("cpu", MODE_STATE)
    cond = arrays.get("cond")
    cond_n = fm._norm_cond(cond)
    for n in (1, 4, 25):
        prior = arrays[f"prior_{n}"]
        grid = torch.linspace(1.0, 0.0, n + 1)
        got = emulate_select(plan, wpack, fm._leapfrog_table(grid), prior, cond_n)
        want = leapfrog_f64(ref, prior, grid, ref.norm_cond(cond))
        err = float((got - want).abs().max()) / float(want.abs().max())
        assert err < 2e-5, (n, err)


def test_order_two_against_scipy():
    """sym_2d: error(n = 100) / error(n = 400) of the emulated table against scipy's RK45 at rtol 1e-10 lies in [12, 20]
    (second order: 16); a wrong midpoint time or weight collapses it to about 4."""
    from scipy.integrate import solve_ivp
    meta, arrays, fm, ref = fixture("sym_2d")
    net = fm._net()
    plan, wpack = net.plan(MODE_STATE, select=True), net.wpack("cpu", MODE_STATE)
    z0 = arrays["prior_4"][:8]
    B, D2 = z0.shape

    def f(t, y):
        return ref.forward(float(t), torch.from_numpy(y.reshape(B, D2).copy()), None).reshape(-1).numpy()
    sol = solve_ivp(f, (1.0, 0.0), z0.double().reshape(-1).numpy(), method="RK45", rtol=1e-10, atol=1e-12)
    assert sol.success
    want = torch.from_numpy(sol.y[:, -1].reshape(B, D2))
    err = {}
    for n in (100, 400):
        got = emulate_select(plan, wpack, fm._leapfrog_table(torch.linspace(1.0, 0.0, n + 1)), z0, None)
        err[n] = float((got - want).abs().max())
    ratio = err[100] / err[400]
    print(f"\n[leapfrog order] error at n = 100: {err[100]:.3e}, at n = 400: {err[400]:.3e}, ratio {ratio:.2f}")
    assert 12 <= ratio <= 20, (err, ratio)


def test_api_errors():
    fm = SymplecticFlowModel(SymplecticMLP(2, 0, 4, [32]), torch.zeros(2), torch.ones(2), None, None)
    x, p0 = torch.zeros(4, 2), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="euler.*leapfrog"):
        fm._sample_from(torch.zeros(4, 4), None, 2, method="verlet")
    with pytest.raises(ValueError, match="euler.*leapfrog"):
        fm._integrate(torch.zeros(4, 4), torch.linspace(1, 0, 3), None, "rk4")
    with pytest.raises(ValueError, match="dopri5.*leapfrog"):
        fm._log_prob_from(x, p0, method="verlet")
    with pytest.raises(ValueError, match="num_steps"):
        fm._log_prob_from(x, p0, method="dopri5", num_steps=10)
    for n in (None, 0):
        with pytest.raises(ValueError, match="num_steps"):
            fm._log_prob_from(x, p0, method="leapfrog", num_steps=n)
        with pytest.raises(ValueError, match="num_steps"):
            fm.log_prob_leapfrog(x, num_steps=n)
    # CPU tensors raise as on every other route
    with pytest.raises(RuntimeError):
        fm.sample_leapfrog((4, 2), num_steps=2)
    with pytest.raises(RuntimeError):
        fm.log_prob_leapfrog(x, num_steps=3)
    with pytest.raises(RuntimeError):
        fm._integrate(torch.zeros(4, 4), torch.linspace(1, 0, 3), None, "leapfrog")
    # num_steps = 0: the prior's q half, as for Euler
    z = torch.randn(4, 4)
    assert torch.equal(fm._sample_from(z, None, 0, method="leapfrog"), z[:, :2])


# ---- sharded entry points over gloo ------------------------------------------------------------------------------------
class _RowKeyedLeapfrog:
    """Stand-in for SymplecticFlowModel on the CPU (the pattern of tests/test_symplectic_twin_host.py): row-wise maps of
    the draws it is handed, different for every method; records whether whole-batch step control was on."""

    def __init__(self, D):
        self.shift = torch.zeros(D)
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.model = self
        self.controlled = []

    def parameters(self):
        return iter([self.w])

    def _note(self):
        from flowfusion_amd.distributed import step_control_group
        self.controlled.append(step_control_group()[0])

    def _sample_from(self, x, conditional=None, num_steps=1, *, method="euler"):
        self._note()
        c = 0.0 if conditional is None else conditional.sum(1, keepdim=True)
        q, p = torch.chunk(x, 2, dim=-1)
        return torch.tanh(q) * 2 + p * float(num_steps) + c + (7.0 if method == "leapfrog" else 0.0)

    def _log_prob_from(self, x, p0, conditional=None, atol=1e-5, rtol=1e-5, method="dopri5", options=None, *, num_steps=None):
        self._note()
        assert (method, num_steps is not None) in (("dopri5", False), ("leapfrog", True))
        c = 0.0 if conditional is None else conditional.sum(1)
        return x.sum(1) + (p0 * p0).sum(1) * 3 + c + (0.0 if num_steps is None else float(num_steps))


def _leapfrog_worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import symplectic_log_prob_sharded as slp, symplectic_sample_sharded as ssm
        _native.normal_fill = _cpu_normal_fill                       # (the product draws on the device; no GPU here)
        D = 3
        torch.manual_seed(0)
        x, c = torch.randn(n, D), torch.randn(n, 2)
        lo, hi = shard_bounds(n, world, rank)
        f = _RowKeyedLeapfrog(D)
        prior = _cpu_normal_fill(n, 2 * D, 5, 0, "cpu")
        p0 = _cpu_normal_fill(n, D, 9, 0, "cpu")
        ok = True
        for steps in (1, 4):
            ok &= torch.equal(ssm(f, n, seed=5, num_steps=steps, method="leapfrog"), f._sample_from(prior, None, steps, method="leapfrog"))
        ok &= torch.equal(ssm(f, n, seed=5, conditional=c, method="leapfrog"), f._sample_from(prior, c, method="leapfrog"))
        ok &= not torch.equal(ssm(f, n, seed=5, conditional=c), f._sample_from(prior, c, method="leapfrog"))
        local, span = ssm(f, n, seed=5, local_conditional=c[lo:hi], gather=False, method="leapfrog")
        ok &= span == (lo, hi) and torch.equal(local, f._sample_from(prior, c, method="leapfrog")[lo:hi])
        # log_prob by leapfrog: a fixed grid -- no exchange whatever global_control says, ranks without rows are fine
        want = f._log_prob_from(x, p0, c, method="leapfrog", num_steps=25)
        f.controlled.clear()
        ok &= torch.equal(slp(f, x, c, seed=9, method="leapfrog", num_steps=25), want)
        ok &= torch.equal(slp(f, x, c, seed=9, method="leapfrog", num_steps=25, global_control=False), want)
        ok &= torch.equal(slp(f, local_x=x[lo:hi], local_conditional=c[lo:hi], n_total=n, seed=9, method="leapfrog", num_steps=25), want)
        local, span = slp(f, x, c, seed=9, gather=False, method="leapfrog", num_steps=25)
        ok &= span == (lo, hi) and torch.equal(local, want[lo:hi])
        ok &= f.controlled == [False] * 4
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 37), (8, 64), (8, 5)])     # ragged, even, fewer rows than ranks
def test_sharded_leapfrog_entry_points_over_gloo(world, n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_leapfrog_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    results = dict(q.get(timeout=5) for _ in range(world))
    assert results == {r: True for r in range(world)}
