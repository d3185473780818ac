"""CPU tier of the per-probe Hutchinson output (ff_mlp_ode_launch_probes; ``return_stderr=True`` on the front ends): the
entry point's signature and every refusal of its argument check without a GPU, the standard-error function against
numpy in float64, the front ends' ValueErrors from CPU-resident models, and the sharded entry points over gloo -- two
columns, ragged shards, exactly one gather."""
import ctypes
import math
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from flowfusion_amd import _native, solvers, trace_estimators
from flowfusion_amd import diffusion as D
from flowfusion_amd import flow as F

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module", autouse=True)
def _lib(built_library):
    return built_library


# ---- the C entry point -----------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_with_its_signature():
    L = _native.lib()
    assert hasattr(L, "ff_mlp_ode_launch_probes")
    header = " ".join((ROOT / "include" / "flowfusion_amd.h").read_text().split())
    assert ("int ff_mlp_ode_launch_probes(const ff_mlp_plan_t* plan, const ff_ode_args* args, float* dlogp_probe_out "
            "/* [batch, K], K = max(1, args->tangent_count) */, void* hip_stream);") in header
    assert L.ff_mlp_ode_launch_probes.argtypes == [ctypes.POINTER(_native.PlanStruct), ctypes.POINTER(_native.OdeArgs),
                                                   ctypes.c_void_p, ctypes.c_void_p]
    # the new pointer is an argument, not a field of ff_ode_args (tests/test_abi.py pins the struct itself)
    assert [f[0] for f in _native.OdeArgs._fields_][-1] == "gate"


def _args(buf, mode=_native.MODE_HUTCH, count=0):
    """Launch arguments every check passes, on HOST addresses with an EMPTY batch: the refusals under test come ahead of
    the empty-batch return, so a check that regressed answers FF_OK (the assertion fails) and nothing is launched."""
    a = _native.OdeArgs()
    a.x_in = a.x_out = a.probe = a.dlogp_out = a.wpack = a.etab = buf.data_ptr()
    a.batch, a.n_evals, a.mode, a.tangent_count = 0, 1, mode, count
    return a


def test_every_refusal_of_the_argument_check_without_a_gpu():
    L = _native.lib()
    BAD, UNS, OK = _native.FF_ERR_BADARG, _native.FF_ERR_UNSUPPORTED, _native.FF_OK
    buf = torch.zeros(64)
    out = buf.data_ptr()
    tangent = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH)             # 16-column tile
    state = _native.make_plan(16, 0, [256] * 4, _native.MODE_STATE)
    tile32 = _native.make_plan(4, 0, [64, 64], _native.MODE_HUTCH)
    call = lambda plan, a, ptr=out: L.ff_mlp_ode_launch_probes(ctypes.byref(plan), ctypes.byref(a), ptr, None)
    plain = lambda plan, a: L.ff_mlp_ode_launch(ctypes.byref(plan), ctypes.byref(a), None)
    # what passes: every K a tile holds; a NULL output is ff_mlp_ode_launch
    for plan, counts in ((tangent, (0, 1, 2, 15)), (tile32, (0, 1, 31))):
        for count in counts:
            assert call(plan, _args(buf, count=count)) == OK, count
    assert call(tangent, _args(buf, _native.MODE_EXACT, 8), None) == plain(tangent, _args(buf, _native.MODE_EXACT, 8)) == OK
    assert call(state, _args(buf, _native.MODE_STATE), None) == plain(state, _args(buf, _native.MODE_STATE)) == OK
    assert L.ff_mlp_ode_launch_probes(ctypes.byref(tangent), None, out, None) == BAD       # (nullargs)
    # mode != FF_MODE_HUTCH
    assert call(tangent, _args(buf, _native.MODE_EXACT)) == BAD
    assert call(tangent, _args(buf, _native.MODE_STATE)) == BAD
    assert call(state, _args(buf, _native.MODE_STATE)) == BAD
    assert call(tangent, _args(buf, 7)) == BAD                                      # (badmode)
    # K + 1 > plan.tile: the existing answer
    for plan, count in ((tangent, 16), (tangent, 40), (tile32, 32)):
        assert call(plan, _args(buf, count=count)) == plain(plan, _args(buf, count=count)) == BAD, count
    # what an attempt launch carries per sample, and the Jacobian output
    for field in ("k1_in", "kl1_in", "dlogp_in", "jac_out"):
        a = _args(buf, count=3)
        setattr(a, field, buf.data_ptr())
        assert call(tangent, a) == BAD, field
    a = _args(buf, count=3)
    a.n_aux = 1
    a.aux_out[0] = a.aux_lp_out[0] = buf.data_ptr()
    assert call(tangent, a) == BAD and plain(tangent, a) == OK
    # a split-precision plan
    for prec in (_native.PREC_BF16X2,):
        split = _native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH, precision=prec)
        for count in (0, 1, 3):
            assert call(split, _args(buf, count=count)) == UNS, count
        assert call(split, _args(buf), None) == plain(split, _args(buf)) == OK
    # pair and select plans: what their argument check answers to a divergence mode
    for select in (False, True):
        pair = _native.make_pair_plan(8, 0, [128, 128], select=select)
        assert call(pair, _args(buf, count=3)) == plain(pair, _args(buf, count=3)) == BAD
        assert call(pair, _args(buf, _native.MODE_STATE)) == BAD


# ---- the standard error ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 7, 15, 31])
def test_stderr_function_against_numpy_in_float64(K):
    g = torch.Generator().manual_seed(100 + K)
    d = torch.randn(53, K, generator=g) * 40.0 + 300.0 * torch.randn(53, 1, generator=g)
    d[5] = d[5, 0]                                         # K equal values
    d[6] = 0.0
    d[7] = 3.0e4 + torch.arange(K, dtype=torch.float32) * 1e-3       # a small spread on a large mean
    got = trace_estimators.hutchinson_stderr(d)
    assert got.dtype == torch.float32 and got.shape == (53,) and got.device == d.device
    want = np.std(d.numpy().astype(np.float64), axis=1, ddof=1) / math.sqrt(K)
    assert float(got[5]) == 0.0 and float(got[6]) == 0.0 and not bool(torch.isnan(got).any())
    # to fp32 rounding: the float64 value rounded once (half an ulp), plus the last bits in which two float64 summation
    # orders may differ -- one ulp of fp32 in all
    err = np.abs(got.numpy().astype(np.float64) - want)
    assert np.all(err <= np.abs(want) * 2.0 ** -23), float((err / np.maximum(np.abs(want), 1e-300)).max())


def test_stderr_function_refuses_one_column():
    with pytest.raises(ValueError, match="K >= 2"):
        trace_estimators.hutchinson_stderr(torch.zeros(4, 1))
    with pytest.raises(ValueError, match="K >= 2"):
        trace_estimators.hutchinson_stderr(torch.zeros(4))


# ---- the front ends' refusals ------------------------------------------------------------------------------------------------
def _score_model(D_=16, units=(256,) * 4, **kw):
    torch.manual_seed(3)
    return D.ScoreModel(D.MLP(n_dimensions=D_, n_conditionals=0, embedding_dimensions=8, units=list(units)), D.VPSDE(),
                        no_sigma=True, **kw).eval()


def test_return_stderr_refusals_name_the_way_out():
    x = torch.randn(4, 16)
    fixed = dict(method="rk4", options={"step_size": 0.25})
    hm = _score_model(hutchinson=True)
    # fewer than two probes
    for call in (lambda: hm.log_prob(x, return_stderr=True, **fixed),
                 lambda: hm.solve_odes_forward(x, num_probes=1, return_stderr=True, **fixed),
                 lambda: _score_model().log_prob(x, return_stderr=True, **fixed)):
        with pytest.raises(ValueError, match=r"num_probes=K with K >= 2"):
            call()
    # models without Hutchinson probes, split precision: the num_probes messages
    with pytest.raises(ValueError, match="hutchinson=True"):
        _score_model().log_prob(x, num_probes=3, return_stderr=True, **fixed)
    with pytest.raises(ValueError, match="hpp_rank"):
        _score_model(hutchpp=True).log_prob(x, num_probes=3, return_stderr=True, **fixed)
    with pytest.raises(ValueError, match="xt_vecs"):
        _score_model(xtrace=True).solve_odes_forward(x, num_probes=2, return_stderr=True, **fixed)
    with pytest.raises(ValueError, match="precision='f32'"):
        _score_model(hutchinson=True, precision="bf16x2").log_prob(x, num_probes=2, return_stderr=True, **fixed)
    # adaptive methods: the defaults, and every member of ALL_ADAPTIVE
    def adaptive_message(call):
        with pytest.raises(ValueError) as info:
            call()
        msg = str(info.value)
        for piece in ("defaults", "adaptive", 'method="rk4"', '"dopri5_fixed"', 'options={"step_size": h}', "grid_constructor",
                      "estimate alone", "still available adaptively"):
            assert piece in msg, (piece, msg)
    adaptive_message(lambda: hm.log_prob(x, num_probes=3, return_stderr=True))
    adaptive_message(lambda: hm.solve_odes_forward(x, num_probes=3, return_stderr=True))
    for method in solvers.ALL_ADAPTIVE:
        adaptive_message(lambda: hm.log_prob(x, num_probes=3, return_stderr=True, method=method))
    # the flows
    f, g = F.ODEFlow(4, [64, 64]), F.ConditionalODEFlow(4, 2, [64, 64])
    xf, cf = torch.randn(3, 4), torch.randn(3, 2)
    ff = dict(method="rk4", options={"step_size": 0.5})
    with pytest.raises(ValueError, match=r"num_probes=K with K >= 2"):
        f.log_prob(xf, hutchinson=True, return_stderr=True, **ff)
    with pytest.raises(ValueError, match=r"num_probes=K with K >= 2"):
        g.solve_ode_forward(xf, cf, return_stderr=True, **ff)
    with pytest.raises(ValueError, match="hutchinson=True"):
        f.log_prob(xf, num_probes=2, return_stderr=True, **ff)
    with pytest.raises(ValueError, match="hutchinson=True"):
        g.log_prob(xf, cf, num_probes=2, return_stderr=True, **ff)
    adaptive_message(lambda: f.log_prob(xf, hutchinson=True, num_probes=2, return_stderr=True))
    adaptive_message(lambda: g.solve_ode_forward(xf, cf, hutchinson=True, num_probes=2, return_stderr=True, method="bosh3"))
    # keyword only, and not a keyword of the population wrappers (adaptive dopri5, like the reference's)
    with pytest.raises(TypeError):
        D.PopulationModelDiffusion(model=_score_model().model, sde=D.VPSDE(), hutchinson=True).log_prob(x, return_stderr=True)
    assert "return_stderr" in D.PopulationModelDiffusion.log_prob.__doc__
    assert "return_stderr" in D.PopulationModelDiffusionConditional.log_prob.__doc__


def test_sharded_entry_points_take_the_keyword_by_name():
    import inspect
    from flowfusion_amd.distributed import flow_log_prob_sharded, log_prob_sharded
    for fn in (log_prob_sharded, flow_log_prob_sharded):
        prm = inspect.signature(fn).parameters["return_stderr"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is False, fn


def test_fifth_op_is_registered_with_a_fake():
    op = torch.ops.flowfusion_amd.mlp_ode_probes
    from torch._subclasses.fake_tensor import FakeTensorMode
    plan = _native.plan_words(_native.make_plan(16, 0, [256] * 4, _native.MODE_HUTCH), 4)
    with FakeTensorMode():
        x, probe = torch.empty(9, 16), torch.empty(9, 3, 16)
        y, dl, d, st = op(x, None, probe, torch.empty(10), torch.empty(12, 32 + 256), None, None, None, None, plan, 3)
        assert y.shape == (9, 16) and dl.shape == (9,) and d.shape == (9, 3) and st.shape == (1,)
        y, dl, d, st = op(x, None, torch.empty(9, 16), torch.empty(10), torch.empty(12, 32 + 256), None, None, None, None, plan)
        assert d.shape == (9, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros(2, 16), None, torch.zeros(2, 16), torch.zeros(10), torch.zeros(12, 288), None, None, None, None, plan)


# ---- the sharded entry points over gloo --------------------------------------------------------------------------------------
class _RowKeyedModel:
    """Stand-in for a Hutchinson ScoreModel whose estimate and standard error depend on each row's values, its conditional
    and the GLOBAL row it is told."""
    hutch = True

    def log_prob(self, rows, conditional=None, probe="torch", seed=None, sample_offset=0, return_stderr=False, **solver):
        assert probe == "philox" and solver == {"method": "rk4", "options": {"step_size": 0.1}, "num_probes": 3}
        g = torch.arange(rows.shape[0], dtype=torch.float32) + float(sample_offset)
        c = 0.0 if conditional is None else conditional.sum(1)
        lp = (rows.sum(1) + 1000.0 * g + float(seed) + c).view(-1, 1)
        return (lp, (rows[:, :1].abs() + 0.25 * g.view(-1, 1))) if return_stderr else lp


class _RowKeyedFlow:
    target_dimension = 3

    def log_prob(self, x, conditional=None, hutchinson=False, probe="torch", seed=None, sample_offset=0, return_stderr=False,
                 **solver):
        assert probe == "philox" and hutchinson
        g = torch.arange(x.shape[0], dtype=torch.float32) + float(sample_offset)
        c = 0.0 if conditional is None else conditional.sum(1)
        lp = x.sum(1) + 1000.0 * g + float(seed) + c
        return (lp, x[:, 0].abs() + 0.25 * g) if return_stderr else lp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flowfusion_amd.distributed import flow_log_prob_sharded, log_prob_sharded, shard_bounds
        gathers = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda out, inp, **kw: (gathers.append(tuple(inp.shape)), real(out, inp, **kw))[1]
        torch.manual_seed(0)
        x, c = torch.randn(n, 3), torch.randn(n, 2)
        lo, hi = shard_bounds(n, world, rank)
        kw = {"method": "rk4", "options": {"step_size": 0.1}, "num_probes": 3}
        ok = True
        m = _RowKeyedModel()
        want = m.log_prob(x, conditional=c, probe="philox", seed=9, sample_offset=0, return_stderr=True, **kw)
        got = log_prob_sharded(m, x, c, seed=9, return_stderr=True, **kw)
        ok &= len(gathers) == 1 and gathers[0][1:] == (2,)
        ok &= isinstance(got, tuple) and len(got) == 2 and got[0].shape == (n, 1) and got[1].shape == (n, 1)
        ok &= torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        ok &= torch.equal(log_prob_sharded(m, x, c, seed=9, **kw), want[0]) and len(gathers) == 2       # (without it: as before)
        mine = log_prob_sharded(m, local_x=x[lo:hi], local_conditional=c[lo:hi], n_total=n, seed=9, return_stderr=True, **kw)
        ok &= torch.equal(mine[0], want[0]) and torch.equal(mine[1], want[1]) and len(gathers) == 3
        (le, ls), span = log_prob_sharded(m, x, c, seed=9, gather=False, return_stderr=True, **kw)
        ok &= span == (lo, hi) and torch.equal(le, want[0][lo:hi]) and torch.equal(ls, want[1][lo:hi]) and len(gathers) == 3
        f = _RowKeyedFlow()
        fk = {"method": "rk4", "options": {"step_size": 0.1}, "num_probes": 3, "hutchinson": True}
        wantf = f.log_prob(x, c, probe="philox", seed=9, sample_offset=0, return_stderr=True, **fk)
        gotf = flow_log_prob_sharded(f, x, c, seed=9, return_stderr=True, **fk)
        ok &= len(gathers) == 4 and gotf[0].shape == (n,) and gotf[1].shape == (n,)
        ok &= torch.equal(gotf[0], wantf[0]) and torch.equal(gotf[1], wantf[1])
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [37, 64])          # ragged, even
def test_sharded_log_prob_returns_both_columns_in_one_gather(n):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    results = dict(q.get(timeout=5) for _ in range(world))
    assert results == {r: True for r in range(world)}
