"""Two-network kernels without a GPU: which kernel(s) the launcher picks for a pair plan (ff_mlp_launch_kind), and the
sharded entry points of the symplectic flows over gloo with a row-keyed stand-in model on the CPU."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flowfusion_amd import _native
from flowfusion_amd.distributed import shard_bounds
from tests.test_distributed_gloo import _cpu_normal_fill, _free_port


@pytest.fixture
def no_pins(monkeypatch):
    monkeypatch.delenv("FF_COOP", raising=False)
    monkeypatch.delenv("FF_TAIL_SPLIT", raising=False)
    return monkeypatch


# (hidden units, kernel, samples per tile, tiles the chip holds = 1024 x wavefronts per SIMD of the one-wavefront kernel)
@pytest.mark.parametrize("units,name,chip", [([256, 256], "mlp_pair_m16_h256_d8_c4_w2", 2048),
                                             ([128, 128], "mlp_pair_m16_h128_d8_c4_w3", 3072)])
def test_launch_kind_of_pair_plans(no_pins, units, name, chip):
    """Small batches take the cooperative twin, whole rounds the one-wavefront kernel, rounds plus a few tiles both; the
    pins FF_COOP / FF_TAIL_SPLIT hold for pair plans as for the others.  (Batch sizes far from the rule's crossovers.)"""
    plan = _native.make_pair_plan(32, 0, units)
    assert _native.kernel_name(plan) == name and plan.tile == 16
    kind = lambda n: _native.launch_kind(plan, n, _native.MODE_STATE)
    for n in (1, 77, 2048, 4099):
        assert kind(n) == _native.LAUNCH_TWIN, n
    # 2^20 samples: 32 whole rounds at width 256; 21 rounds and a third of one at width 128, which the one-wavefront
    # kernel finishes in a third of a round's time (one wavefront per SIMD) and the twin would not
    assert kind(1 << 20) == _native.LAUNCH_ONE_WAVE
    tail = 300 if chip == 2048 else 120
    assert kind(chip * 16 + tail) == _native.LAUNCH_ONE_WAVE_AND_TWIN
    no_pins.setenv("FF_TAIL_SPLIT", "0")
    assert kind(chip * 16 + tail) == _native.LAUNCH_ONE_WAVE
    no_pins.delenv("FF_TAIL_SPLIT")
    no_pins.setenv("FF_COOP", "0")
    assert kind(2048) == _native.LAUNCH_ONE_WAVE
    no_pins.setenv("FF_COOP", "1")
    assert kind(1 << 20) == _native.LAUNCH_TWIN


def test_launch_kind_64_wide_has_no_twin(no_pins):
    plan = _native.make_pair_plan(4, 0, [64])
    assert _native.kernel_name(plan) == "mlp_pair_m32_h64_d16_c8"
    assert _native.launch_kind(plan, 77, _native.MODE_STATE) == _native.LAUNCH_ONE_WAVE
    no_pins.setenv("FF_COOP", "1")
    assert _native.launch_kind(plan, 77, _native.MODE_STATE) == _native.LAUNCH_ONE_WAVE


def test_launch_kind_bad_arguments_still_raise(no_pins):
    plan = _native.make_pair_plan(32, 0, [256, 256])
    for args in ((77, _native.MODE_EXACT), (77, _native.MODE_HUTCH), (-1, _native.MODE_STATE)):
        with pytest.raises(RuntimeError):
            _native.launch_kind(plan, *args)
    with pytest.raises(RuntimeError):
        _native.launch_kind(plan, 77, _native.MODE_STATE, jac_out=True)
    # a twin is not an entry of the table
    L = _native.lib()
    assert L.ff_pair_kernel_count() == 3


# ---- sharded entry points over gloo ------------------------------------------------------------------------------------
class _RowKeyedSymplectic:
    """Stand-in for SymplecticFlowModel on the CPU: row-wise maps of the draws it is handed (which the entry points key by
    the GLOBAL row); records whether the whole-batch step control was on."""

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

    def _sample_from(self, x, conditional=None, num_steps=1):
        self._note()
        c = 0.0 if conditional is None else conditional.sum(1, keepdim=True)
        q, p = torch.chunk(x, 2, dim=-1)
        return torch.tanh(q) * 2 + p * float(num_steps) + c

    def _log_prob_from(self, x, p0, conditional=None, atol=1e-5, rtol=1e-5, method="dopri5", options=None):
        self._note()
        assert method == "dopri5" and options is None
        c = 0.0 if conditional is None else conditional.sum(1)
        return x.sum(1) + (p0 * p0).sum(1) * 3 + c + atol * 1e5 + rtol * 1e4


def _sym_worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import symplectic_log_prob_sharded as slp, symplectic_sample_sharded as ssm
        _native.normal_fill = _cpu_normal_fill                       # (the product draws on the device; no GPU here)
        D = 3
        torch.manual_seed(0)
        x, c = torch.randn(n, D), torch.randn(n, 2)
        lo, hi = shard_bounds(n, world, rank)
        f = _RowKeyedSymplectic(D)
        prior = _cpu_normal_fill(n, 2 * D, 5, 0, "cpu")
        p0 = _cpu_normal_fill(n, D, 9, 0, "cpu")
        ok = True
        # sample: every world size transports the same prior draws; fixed grid: no exchange, empty shards are fine
        for steps in (1, 4):
            ok &= torch.equal(ssm(f, n, seed=5, num_steps=steps), f._sample_from(prior, None, steps))
        ok &= torch.equal(ssm(f, n, seed=5, conditional=c), f._sample_from(prior, c))
        ok &= torch.equal(ssm(f, n, seed=5, local_conditional=c[lo:hi]), f._sample_from(prior, c))
        local, span = ssm(f, n, seed=5, conditional=c, gather=False)
        ok &= span == (lo, hi) and torch.equal(local, f._sample_from(prior, c)[lo:hi])
        for bad in (dict(conditional=c, local_conditional=c[lo:hi]), dict(local_conditional=c[: hi - lo + 1])):
            try:
                ssm(f, n, seed=5, **bad)
                ok = False
            except ValueError:
                pass
        ok &= not any(f.controlled)
        want = f._log_prob_from(x, p0, c)
        want_tol = f._log_prob_from(x, p0, None, 1e-6, 1e-7)
        f.controlled.clear()
        # log_prob: adaptive -- whole-batch step control when every rank has a row, a ValueError on EVERY rank (before
        # anyone enters a collective) when some rank has none; global_control=False enters no exchange
        if n >= world:
            ok &= torch.equal(slp(f, x, c, seed=9), want)
            ok &= torch.equal(slp(f, x, seed=9, atol=1e-6, rtol=1e-7), want_tol)
            ok &= torch.equal(slp(f, local_x=x[lo:hi], local_conditional=c[lo:hi], n_total=n, seed=9), want)
            local, span = slp(f, x, c, seed=9, gather=False)
            ok &= span == (lo, hi) and torch.equal(local, want[lo:hi])
            ok &= f.controlled == [world > 1] * 4
        else:
            for call in (lambda: slp(f, x, c, seed=9), lambda: slp(f, local_x=x[lo:hi], n_total=n, seed=9)):
                try:
                    call()
                    ok = False
                except ValueError as e:
                    ok &= "at least one row per rank" in str(e)
            ok &= f.controlled == []
        for bad in (dict(x=x, local_x=x[lo:hi]), dict(local_x=x[lo:hi]), dict(local_x=x[: hi - lo + 1], n_total=n),
                    dict(x=x, local_conditional=c[lo:hi]), dict(local_x=x[lo:hi], n_total=n, conditional=c)):
            try:
                slp(f, **bad)
                ok = False
            except ValueError as e:
                ok &= "at least one row per rank" not in str(e)
        f.controlled.clear()
        got = slp(f, x, c, seed=9, global_control=False)
        ok &= f.controlled == [False] and torch.equal(got, want)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 64), (2, 37), (8, 64), (8, 37), (8, 5)])     # even, ragged, fewer rows than ranks
def test_symplectic_sharded_entry_points_over_gloo(world, n):
    """distributed.symplectic_sample_sharded / symplectic_log_prob_sharded: the prior and the momentum draw keyed by the
    GLOBAL row, the conditional sliced per rank, one all-gather at the end, whole-batch step control for the adaptive
    log_prob -- and a clean ValueError on every rank when a shard would be empty under that control."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sym_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    results = dict(q.get(timeout=5) for _ in range(world))
    assert results == {r: True for r in range(world)}
