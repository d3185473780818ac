"""The calling conventions of the seven `*_sharded` entry points (flowfusion_amd/distributed.py), without a process group:
one rank owns every row, so each valid way to pass the data must give exactly the unsharded result, and each invalid
combination must raise the exception type it always raised.  The models are row-keyed stand-ins (results depend on each
row's values, its conditional and the global row or seed it is told), as in tests/test_distributed_gloo.py, which with
tests/test_symplectic_*_host.py covers more than one rank."""
from types import SimpleNamespace

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd import distributed as Dd

N, DIM, SEED = 7, 3, 9
FIXED = {"method": "rk4", "options": {"step_size": 0.1}}


def _cpu_normal_fill(batch, dim, seed, sample_offset, device, noise_index=0xFFFFFFFF, scale=1.0):
    """ff_normal_fill's stream on the CPU (tests/_philox.py restates it): keyed by the global row, like the device's."""
    from tests import _philox
    return torch.from_numpy(_philox.normals(seed, sample_offset, batch, dim, [noise_index])[0].copy()) * scale


class _RowKeyed:
    """Everything the seven entry points ask of a ScoreModel, an ODEFlow or a SymplecticFlowModel."""
    hutch = True
    target_dimension = DIM
    shift = None
    sde = SimpleNamespace(sigma_max=2.0)

    def __init__(self):
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.model = self

    def parameters(self):
        return iter([self.w])

    def _net(self):
        return SimpleNamespace(dim=2 * DIM)

    @staticmethod
    def _rows(x, cond, offset, *more):
        g = torch.arange(x.shape[0], dtype=torch.float32) + float(offset)
        c = 0.0 if cond is None else cond.sum(1)
        return torch.tanh(x).sum(1) + 1000.0 * g + c + float(sum(more))

    def _sample_sde_from(self, x, noise, cond, steps, rng):
        assert noise is None
        return x * 2 + self._rows(x, cond, rng[1], steps, rng[0])[:, None]

    def log_prob(self, x, conditional=None, hutchinson=False, probe="torch", seed=0, sample_offset=0, **solver):
        assert solver == FIXED and probe == "philox"
        return self._rows(x, conditional, sample_offset, seed).view(-1, 1)

    def sample_ode_from_base(self, z, conditional=None, **solver):
        assert solver == FIXED
        return z * 3 + self._rows(z, conditional, 0)[:, None], None

    def sample(self, xT, conditional=None, **solver):
        assert solver == FIXED
        return xT * 4 + self._rows(xT, conditional, 0)[:, None]

    def _sample_from(self, x, cond, num_steps, method="euler"):
        return x * 5 + self._rows(x, cond, 0, num_steps, method == "leapfrog")[:, None]

    def _log_prob_from(self, rows, p0, cond, atol, rtol, method="dopri5", num_steps=None):
        return self._rows(rows, cond, 0, atol, rtol, num_steps or 0) + p0.sum(1)


@pytest.fixture
def data(monkeypatch):
    monkeypatch.setattr(_native, "normal_fill", _cpu_normal_fill)        # (the product draws on the device; no GPU here)
    torch.manual_seed(0)
    return SimpleNamespace(m=_RowKeyed(), x=torch.randn(N, DIM), c=torch.randn(N, 2),
                           fill=lambda dim, scale=1.0: _cpu_normal_fill(N, dim, SEED, 0, "cpu", scale=scale))


# (entry point, its keyword arguments besides the data, the unsharded result for the conditional `c` or None)
SAMPLERS = {
    "sample_sde": (lambda m, **kw: Dd.sample_sde_sharded(m, (N, DIM), steps=4, seed=SEED, **kw),
                   lambda d, c: d.m._sample_sde_from(d.fill(DIM, 2.0), None, c, 4, rng=(SEED, 0))),
    "sample_ode": (lambda m, **kw: Dd.sample_ode_sharded(m, N, DIM, seed=SEED, **kw, **FIXED),
                   lambda d, c: d.m.sample_ode_from_base(d.fill(DIM), conditional=c, **FIXED)[0]),
    "flow_sample": (lambda m, **kw: Dd.flow_sample_sharded(m, N, seed=SEED, **kw, **FIXED),
                    lambda d, c: d.m.sample(d.fill(DIM), c, **FIXED)),
    "symplectic_sample": (lambda m, **kw: Dd.symplectic_sample_sharded(m, N, seed=SEED, num_steps=3, method="leapfrog", **kw),
                          lambda d, c: d.m._sample_from(d.fill(2 * DIM), c, 3, method="leapfrog")),
}
LOG_PROBS = {
    "log_prob": (lambda m, **kw: Dd.log_prob_sharded(m, seed=SEED, **kw, **FIXED),
                 lambda d, c: d.m.log_prob(d.x, conditional=c, probe="philox", seed=SEED, sample_offset=0, **FIXED)),
    "flow_log_prob": (lambda m, **kw: Dd.flow_log_prob_sharded(m, seed=SEED, hutchinson=True, **kw, **FIXED),
                      lambda d, c: d.m.log_prob(d.x, c, hutchinson=True, probe="philox", seed=SEED, sample_offset=0, **FIXED)),
    "symplectic_log_prob": (lambda m, **kw: Dd.symplectic_log_prob_sharded(m, seed=SEED, atol=1e-3, rtol=1e-4, **kw),
                            lambda d, c: d.m._log_prob_from(d.x, d.fill(DIM), c, 1e-3, 1e-4, method="dopri5")),
}


def _same(got, want, gather):
    if not gather:
        local, span = got
        return span == (0, N) and torch.equal(local, want)
    return torch.is_tensor(got) and torch.equal(got, want)


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_samplers_take_the_full_or_the_local_conditional(name, data):
    call, unsharded = SAMPLERS[name]
    for gather in (True, False):
        assert _same(call(data.m, gather=gather), unsharded(data, None), gather)
        assert _same(call(data.m, conditional=data.c, gather=gather), unsharded(data, data.c), gather)
        assert _same(call(data.m, local_conditional=data.c, gather=gather), unsharded(data, data.c), gather)
    for bad in (dict(conditional=data.c, local_conditional=data.c), dict(local_conditional=data.c[:-1])):
        with pytest.raises(ValueError):
            call(data.m, **bad)


def test_sample_sde_sharded_refuses_other_than_batch_by_dim(data):
    for shape in ((N,), (N, DIM, DIM)):
        with pytest.raises(NotImplementedError):
            Dd.sample_sde_sharded(data.m, shape, steps=4, seed=SEED)


@pytest.mark.parametrize("name", sorted(LOG_PROBS))
def test_log_probs_take_the_full_or_the_local_batch(name, data):
    call, unsharded = LOG_PROBS[name]
    x, c = data.x, data.c
    for gather in (True, False):
        assert _same(call(data.m, x=x, gather=gather), unsharded(data, None), gather)
        assert _same(call(data.m, x=x, conditional=c, gather=gather), unsharded(data, c), gather)
        assert _same(call(data.m, local_x=x, n_total=N, gather=gather), unsharded(data, None), gather)
        assert _same(call(data.m, local_x=x, n_total=N, local_conditional=c, gather=gather), unsharded(data, c), gather)
    for bad in (dict(x=x, local_x=x, n_total=N),                               # both
                dict(), dict(n_total=N),                                       # neither
                dict(local_x=x),                                               # local rows without n_total
                dict(local_x=x[:-1], n_total=N), dict(local_x=x, n_total=N + 1),            # not exactly this rank's rows
                dict(x=x, local_conditional=c),
                dict(local_x=x, n_total=N, conditional=c),
                dict(x=x, conditional=c, local_conditional=c), dict(local_x=x, n_total=N, conditional=c, local_conditional=c),
                dict(local_x=x, n_total=N, local_conditional=c[:-1])):
        with pytest.raises(ValueError):
            call(data.m, **bad)


def test_shard_sizes_are_the_spans_of_shard_bounds():
    for n, world in ((0, 3), (5, 8), (37, 8), (64, 8)):
        assert Dd.shard_sizes(n, world) == [hi - lo for lo, hi in (Dd.shard_bounds(n, world, r) for r in range(world))]
