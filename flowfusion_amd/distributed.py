"""Multi-GPU execution of the sampling / log-density path: one process per GPU, batch sharding,
one collective at the end (adaptive solves: plus the exchange of their error norms, `global_step_control`).

The reference is single-process (no torch.distributed anywhere in flowfusion/).  Samples are
independent -- nothing on the path couples two rows of the batch -- so the batch axis is cut into
contiguous, balanced shards, every rank integrates its shard with the fused kernel (weights and the
evaluation table are a few MB and simply replicated), and the results meet in a single RCCL
all-gather over xGMI (backend "nccl" is RCCL on ROCm).  Fixed-grid solves use no other collective.  Adaptive solves have
one real exchange step: torchdiffeq chooses ONE step size for the whole batch from a norm over all of it, so the sums of
squares behind each norm are all-reduced (8 doubles) when a batch is cut over ranks -- `global_step_control`.
"""
from __future__ import annotations

import contextlib
import contextvars
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

# ---- the one exchange step of the path: step control of an ADAPTIVE solve over several shards of one batch -----------------
# (a context variable: the setting belongs to the solve that entered the context, not to every host thread of the process)
_STEP_CONTROL: contextvars.ContextVar = contextvars.ContextVar("ff_step_control", default=(False, None))


@contextlib.contextmanager
def global_step_control(group=None):
    """Adaptive solves inside this context control their step size from the error norm of the WHOLE batch, as torchdiffeq
    does for the batch it is handed (one step size for all samples: diffusion.py:631-639, 744-752; flow.py:299-303,
    371-382), although each rank holds only a shard: the sums of squares behind every norm are summed over ``group``
    (an RCCL all-reduce of 8 doubles per norm, enqueued between the reduction kernel and the controller kernel -- no host
    synchronisation on the device-side controller).  Every rank then takes the same accept / reject decisions and the same
    steps, so a sample's result does not depend on the sharding beyond the rounding of those sums.  Every rank must enter
    the same solves in the same order, each with at least one row.  Outside the context (the default) a rank controls its
    steps from its own rows.  Fixed-grid solves need none of this."""
    if not dist.is_initialized():
        raise RuntimeError("global_step_control needs an initialised torch.distributed process group")
    token = _STEP_CONTROL.set((True, group))
    try:
        yield
    finally:
        _STEP_CONTROL.reset(token)


def step_control_group():
    """(active, group) of the enclosing ``global_step_control`` context."""
    return _STEP_CONTROL.get()


def _is_adaptive(method) -> bool:
    from . import solvers
    return method in solvers.ALL_ADAPTIVE


def _step_control(n: int, group, global_control: bool, method):
    """The context a sharded solve runs in.  Batch-global step control needs every rank in the exchange, and an empty
    shard has no launch to hang the exchange on: its peers would wait in the all-reduce for ever.  ``n`` and ``world``
    are known to every rank, so every rank raises here, before anyone enters a collective."""
    world = _shard(n, group)[0]
    if not (global_control and world > 1 and _is_adaptive(method)):
        return contextlib.nullcontext()
    if n < world:
        raise ValueError(f"global step control over {world} ranks needs at least one row per rank, the batch has {n}: use fewer "
                         "ranks, a fixed-grid method, or global_control=False (every rank then steps from its own rows)")
    return global_step_control(group)


def sum_over_ranks_(values: torch.Tensor, group=None) -> torch.Tensor:
    """In-place sum of a small tensor over the ranks, ordered with the current stream.  RCCL reduces device tensors in
    place; the gloo rehearsal (several ranks on one card, CPU tests) goes through the host."""
    if dist.get_backend(group) == "nccl" or not values.is_cuda:
        dist.all_reduce(values, group=group)
    else:
        host = values.cpu()
        dist.all_reduce(host, group=group)
        values.copy_(host)
    return values


def sum_over_ranks(values: List[float], device, group=None) -> List[float]:
    """Host-side form (the host step controller): python floats in, their sums over the ranks out."""
    on = device if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.tensor(values, dtype=torch.float64, device=on)
    dist.all_reduce(t, group=group)
    return [float(v) for v in t.cpu()]


def shard_bounds(n: int, world: int, rank: int) -> Tuple[int, int]:
    """Rows [lo, hi) of an n-row batch owned by `rank`: contiguous, sizes differ by at most one."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_sizes(n: int, world: int):
    return [hi - lo for lo, hi in (shard_bounds(n, world, r) for r in range(world))]


# ---- what every sharded entry point below does before and after its solve ---------------------------------------------------
def _shard(n: int, group) -> Tuple[int, int, int, int]:
    """(world, rank, lo, hi): the rows [lo, hi) of an n-row batch this rank owns (one rank without a process group)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    return (world, rank) + shard_bounds(n, world, rank)


def _local_rows(full, local, lo, hi, what):
    if local is not None:
        if full is not None or local.shape[0] != hi - lo:
            raise ValueError(f"local_{what} must hold exactly this rank's rows [{lo}, {hi}) (and excludes `{what}`)")
        return local.contiguous()
    return None if full is None else full[lo:hi].contiguous()


def _local_batch(x, local_x, n_total, conditional, local_conditional, group):
    """(n, lo, hi, rows, cond) of a log-density entry point: ``x`` (and ``conditional``) are the full tensors, every rank
    slicing its rows -- or ``local_x`` (and ``local_conditional``) this rank's rows already, with ``n_total`` the size of
    the whole batch."""
    if (x is None) == (local_x is None):
        raise ValueError("pass either the full batch `x` or this rank's rows `local_x` (with n_total)")
    if x is None and n_total is None:
        raise ValueError("local_x needs n_total")
    if x is not None and local_conditional is not None:
        raise ValueError("local_conditional goes with local_x")
    if x is None and conditional is not None:
        raise ValueError("local_x goes with local_conditional, not the full `conditional`")
    n = int(x.shape[0] if x is not None else n_total)
    _, _, lo, hi = _shard(n, group)
    return n, lo, hi, _local_rows(x, local_x, lo, hi, "x"), _local_rows(conditional, local_conditional, lo, hi, "conditional")


def _finish(local, n: int, group, gather: bool):
    """The one collective at the end: the gathered [n, ...] result, or with ``gather=False`` this rank's rows and their
    bounds.  ``local``: a tensor, or an ``(estimate, stderr)`` pair of equal shapes ([rows, 1] or [rows]) -- the two travel
    as the columns of ONE [rows, 2] tensor, so the single all-gather stays single, and come back in their own shapes."""
    world, _, lo, hi = _shard(n, group)
    if not gather:
        return local, (lo, hi)
    if world == 1:
        return local
    if torch.is_tensor(local):
        return gather_rows(local, n, group)
    est, se = local
    out = gather_rows(torch.stack([est.reshape(-1), se.reshape(-1)], dim=1), n, group)
    return tuple(col.reshape((-1,) + tuple(est.shape[1:])) for col in (out[:, 0], out[:, 1]))


def _sample_sharded(run, n_total, dim, seed, dev, conditional, local_conditional, group, gather, control=None, scale=1.0):
    """What every sampling entry point below does: shard, draw this rank's rows of the base samples from the counter-based
    stream (``ff_normal_fill`` keyed by ``seed`` and the GLOBAL row), take its rows of the conditional, run
    ``run(z, cond, lo)`` -- under ``_step_control(.., *control)`` where ``control = (global_control, method)`` -- and finish."""
    from . import _native
    n = int(n_total)
    _, _, lo, hi = _shard(n, group)
    z = _native.normal_fill(hi - lo, int(dim), int(seed), lo, dev, scale=scale)
    cond = _local_rows(conditional, local_conditional, lo, hi, "conditional")
    with contextlib.nullcontext() if control is None else _step_control(n, group, *control):
        local = run(z, cond, lo)
    return _finish(local, n, group, gather)


def _log_prob_sharded(log_prob, randomised, x, conditional, seed, group, gather, local_x, n_total, local_conditional,
                      global_control, return_stderr, solver):
    """What ``log_prob_sharded`` and ``flow_log_prob_sharded`` do: ``log_prob(rows, cond, **solver, **extra)`` on this
    rank's rows, ``extra`` keying the probes of a ``randomised`` model by ``seed`` and the global row."""
    n, lo, hi, rows, cond = _local_batch(x, local_x, n_total, conditional, local_conditional, group)
    extra = {"probe": "philox", "seed": int(seed), "sample_offset": lo} if randomised else {}
    if return_stderr:
        extra["return_stderr"] = True
    with _step_control(n, group, global_control, solver.get("method", "dopri5")):
        local = log_prob(rows, cond, **solver, **extra)
    return _finish(local, n, group, gather)


def gather_rows(local: torch.Tensor, n_total: int, group=None) -> torch.Tensor:
    """All-gather the row shards produced under `shard_bounds` back into the full [n_total, ...]
    tensor on every rank (one collective; ragged shards are padded to the largest)."""
    world = dist.get_world_size(group)
    sizes = shard_sizes(n_total, world)
    if world == 1:
        return local
    if local.is_cuda and dist.get_backend(group) != "nccl":
        # (the gloo rehearsal of the multi-rank path -- several ranks on one card, CPU tests -- gathers through the host)
        return gather_rows(local.cpu(), n_total, group).to(local.device)
    if len(set(sizes)) == 1:
        out = local.new_empty((n_total,) + tuple(local.shape[1:]))
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    mx = max(sizes)
    pad = local.new_zeros((mx,) + tuple(local.shape[1:]))
    pad[: local.shape[0]] = local
    buf = local.new_empty((world * mx,) + tuple(local.shape[1:]))
    dist.all_gather_into_tensor(buf, pad, group=group)
    return torch.cat([buf[r * mx: r * mx + sizes[r]] for r in range(world)], dim=0)


def run_sharded(fn: Callable[..., torch.Tensor], inputs: Sequence[Optional[torch.Tensor]], group=None,
                gather: bool = True):
    """Apply `fn(*row_slices)` to this rank's shard of every [B, ...] input and (optionally) gather.

    Every rank passes the same full-batch `inputs` (or `None` entries); rank r computes rows
    ``shard_bounds(B, world, r)``.  With ``gather=False`` the local result is returned together
    with its bounds, for consumers that keep the data distributed.
    """
    n = next(t.shape[0] for t in inputs if t is not None)
    _, _, lo, hi = _shard(n, group)
    local = fn(*[None if t is None else t[lo:hi].contiguous() for t in inputs])
    if not gather:
        return local, (lo, hi)
    if isinstance(local, (tuple, list)):
        return type(local)(gather_rows(t, n, group) if torch.is_tensor(t) else t for t in local)
    return gather_rows(local, n, group)


def sample_sde_sharded(score_model, shape, conditional: Optional[torch.Tensor] = None, steps: int = 100,
                       seed: int = 0, group=None, gather: bool = True, local_conditional: Optional[torch.Tensor] = None):
    """Euler-Maruyama sampling (``ScoreModel.sample_sde``) of a [B, dim] batch over all ranks, with the
    same result for any number of ranks: both the prior draw and the per-step noise come from the library's
    counter-based stream keyed by ``seed`` and the GLOBAL row index (prior: ``ff_normal_fill`` with the reserved
    noise index; steps: ``noise="philox"``), so a rank only ever touches its own rows.  One all-gather at the
    end.  ``conditional`` is the full [B, C] tensor (every rank slices its rows); ``local_conditional`` is this rank's
    [hi - lo, C] rows already (a consumer that never materialises the full batch)."""
    batch, *dims = shape
    if len(dims) != 1:
        raise NotImplementedError("sample_sde_sharded: only [batch, dim] states are supported")
    sde = score_model.sde
    scale = float(sde.sigma_max) if hasattr(sde, "sigma_max") else 1.0      # the prior is Normal(0, scale) (diffusion.py:1003, 1093)
    run = lambda x, cond, lo: score_model._sample_sde_from(x, None, cond, steps, rng=(int(seed), lo))
    return _sample_sharded(run, batch, dims[0], seed, next(score_model.model.parameters()).device, conditional,
                           local_conditional, group, gather, scale=scale)


def log_prob_sharded(score_model, x: Optional[torch.Tensor] = None, conditional: Optional[torch.Tensor] = None,
                     seed: int = 0, group=None, gather: bool = True, local_x: Optional[torch.Tensor] = None,
                     n_total: Optional[int] = None, local_conditional: Optional[torch.Tensor] = None,
                     global_control: bool = True, *, return_stderr: bool = False, **solver):
    """``ScoreModel.log_prob`` of a [B, dim] batch over all ranks; one all-gather of the [B, 1] result at the end.

    ``x`` (and ``conditional``) are the full tensors, every rank slicing its rows -- or ``local_x`` (and
    ``local_conditional``) are this rank's rows already, with ``n_total`` the size of the whole batch.  A Hutchinson,
    Hutch++ or XTrace model takes its probes from the library's counter-based stream keyed by ``seed`` and the GLOBAL row
    (``probe="philox"``), so with a fixed-grid ``method`` a row's result does not depend on the number of ranks; the
    exact trace needs no random numbers.  ``**solver`` (atol, rtol, method, options, num_probes) goes to ``log_prob``
    unchanged: ``num_probes=K`` averages K counter-based probes per global row (``ff_probe_fill``), whatever the sharding.
    Under an adaptive ``method`` (the reference's default) the step size comes from the error norm of the WHOLE batch, as
    torchdiffeq takes it (``global_step_control``: one small all-reduce per norm; every rank needs at least one row);
    results then agree across world sizes to the rounding of those norms.  ``global_control=False``: every rank
    controls its steps from its own rows (agreement to the solver tolerances only).
    ``return_stderr=True`` (keyword only; ``num_probes=K >= 2`` and a fixed-grid ``method``, see
    ``ScoreModel.solve_odes_forward``): returns ``(log_p [B, 1], stderr [B, 1])``; the two are gathered as the columns of
    one [rows, 2] tensor, so there is still one all-gather.  With ``gather=False`` it returns
    ``((log_p, stderr), (lo, hi))``: this rank's rows of both, and their bounds."""
    randomised = any(getattr(score_model, k, False) for k in ("hutch", "hutchpp", "xtrace"))
    return _log_prob_sharded(lambda rows, cond, **kw: score_model.log_prob(rows, conditional=cond, **kw), randomised, x,
                             conditional, seed, group, gather, local_x, n_total, local_conditional, global_control,
                             return_stderr, solver)


def sample_ode_sharded(score_model, n_total: int, dim: int, seed: int = 0, conditional: Optional[torch.Tensor] = None,
                       group=None, gather: bool = True, local_conditional: Optional[torch.Tensor] = None,
                       global_control: bool = True, **solver):
    """``ScoreModel.sample_ode_from_base`` of ``n_total`` base samples over all ranks: the base samples are standard
    normals of the library's counter-based stream keyed by ``seed`` and the GLOBAL row (``ff_normal_fill``), so every world
    size transports the same points and a rank only ever touches its rows; one all-gather at the end.  ``**solver`` (atol,
    rtol, method, options) goes to ``sample_ode_from_base`` unchanged; with an adaptive method (the reference's default)
    and ``global_control`` the step size comes from the error norm of the whole batch (``global_step_control``)."""
    run = lambda z, cond, lo: score_model.sample_ode_from_base(z, conditional=cond, **solver)[0]
    return _sample_sharded(run, n_total, dim, seed, next(score_model.model.parameters()).device, conditional,
                           local_conditional, group, gather, control=(global_control, solver.get("method", "dopri5")))


# ---- the flows (flowfusion/flow.py:259-306, 386-438; 750-799, 885-941) -- BASELINE configs[3] is worded "sharded over 8xMI355X"
def flow_sample_sharded(flow, n_total: int, seed: int = 0, conditional: Optional[torch.Tensor] = None, group=None,
                        gather: bool = True, local_conditional: Optional[torch.Tensor] = None, global_control: bool = True,
                        **solver):
    """``ODEFlow.sample`` / ``ConditionalODEFlow.sample`` of ``n_total`` base samples over all ranks.  The base samples
    are standard normals of the library's counter-based stream keyed by ``seed`` and the GLOBAL row (``ff_normal_fill``):
    every world size transports the same points and a rank only ever touches its own rows.  ``conditional`` is the raw
    [n_total, C] tensor (every rank slices its rows) or ``local_conditional`` this rank's rows; the flow normalises it
    itself (flow.py:771-777).  One all-gather at the end (north_star: "a single RCCL gather"; ``gather=False`` keeps the
    shard and returns its bounds).  ``**solver`` (method, options, atol, rtol) goes to ``sample`` unchanged; under an
    adaptive method -- the reference's default -- the step size comes from the error norm of the whole batch
    (``global_step_control``), ``global_control=False``: from the rank's own rows."""
    from .flow import _DEFAULT_SAMPLE_METHOD
    run = lambda xT, cond, lo: flow.sample(xT, **solver) if cond is None else flow.sample(xT, cond, **solver)
    return _sample_sharded(run, n_total, flow.target_dimension, seed, next(flow.parameters()).device, conditional,
                           local_conditional, group, gather,
                           control=(global_control, solver.get("method") or _DEFAULT_SAMPLE_METHOD))


def flow_log_prob_sharded(flow, x: Optional[torch.Tensor] = None, conditional: Optional[torch.Tensor] = None, seed: int = 0,
                          group=None, gather: bool = True, local_x: Optional[torch.Tensor] = None,
                          n_total: Optional[int] = None, local_conditional: Optional[torch.Tensor] = None,
                          global_control: bool = True, *, return_stderr: bool = False, **solver):
    """``ODEFlow.log_prob`` / ``ConditionalODEFlow.log_prob`` of a [B, dim] batch over all ranks; one all-gather of the
    [B] result at the end.  ``x`` (and ``conditional``) are the full tensors, every rank slicing its rows -- or ``local_x``
    (and ``local_conditional``) this rank's rows already, with ``n_total`` the size of the whole batch.  With
    ``hutchinson=True`` the probe comes from the library's counter-based stream keyed by ``seed`` and the GLOBAL row
    (``probe="philox"``), so a row's result does not depend on the number of ranks; the exact trace (the reference's
    default, flow.py:158-161) needs no random numbers; ``num_probes=K`` (with ``hutchinson=True``) goes to ``log_prob``
    with the rest of ``**solver``: K counter-based probes per global row.  Step control as in ``flow_sample_sharded``.
    ``return_stderr=True`` (with ``hutchinson=True``, ``num_probes=K >= 2`` and a fixed-grid ``method``): returns
    ``(log_p [B], stderr [B])``, gathered as the columns of one [rows, 2] tensor -- still one all-gather; with
    ``gather=False``, ``((log_p, stderr), (lo, hi))``: this rank's rows of both, and their bounds."""
    log_prob = lambda rows, cond, **kw: flow.log_prob(rows, **kw) if cond is None else flow.log_prob(rows, cond, **kw)
    return _log_prob_sharded(log_prob, bool(solver.get("hutchinson")), x, conditional, seed, group, gather, local_x, n_total,
                             local_conditional, global_control, return_stderr, solver)


# ---- noisy observations: score models and flows alike (extension; no counterpart in the reference) --------------------------
def log_prob_noisy_sharded(model, x: Optional[torch.Tensor] = None, noise_std=None, conditional: Optional[torch.Tensor] = None,
                           *, local_x: Optional[torch.Tensor] = None, local_noise_std: Optional[torch.Tensor] = None,
                           n_total: Optional[int] = None, local_conditional: Optional[torch.Tensor] = None, seed: int = 0,
                           num_draws: int = 16, group=None, gather: bool = True, global_control: bool = True,
                           return_ess: bool = False, **solver):
    """``log_prob_noisy`` (``ScoreModel``, ``ODEFlow``, ``ConditionalODEFlow``) of a [B, dim] batch of observations over all
    ranks; one all-gather at the end, of the model's own result shape ([B, 1] for a score model, [B] for a flow).  ``x``
    (with ``noise_std`` and ``conditional``) are the full tensors, every rank slicing its rows of the contiguous balanced
    shards -- or ``local_x`` (with ``local_noise_std`` / ``local_conditional``) this rank's rows already, with ``n_total``
    the size of the whole batch.  A [B, D] ``noise_std`` is cut like ``x``; a [D] vector or a scalar is replicated (pass it
    as ``noise_std`` with ``local_x`` too).  The noise draws -- and the probes of a Hutchinson model -- are keyed by
    ``seed`` and the GLOBAL row (``sample_offset`` = the rank's first row), so with a fixed-grid ``method`` a row's result
    is bitwise independent of the number of ranks.  Under an adaptive ``method`` (the default) every rank's ``local * K``
    rows are one solve whose step size comes from the error norm of the WHOLE expanded batch (``global_step_control``;
    every rank needs at least one row), ``global_control=False``: from the rank's own rows.  ``**solver`` (atol, rtol,
    method, options, hutchinson, num_probes, chunk_points) goes to ``log_prob_noisy`` unchanged.  ``return_ess=True``:
    ``(log_p, ess [B])``, the two gathered as the columns of one [rows, 2] tensor -- still one all-gather; with
    ``gather=False`` ``((log_p, ess), (lo, hi))``: this rank's rows of both, and their bounds."""
    if local_noise_std is not None and (noise_std is not None or local_x is None):
        raise ValueError("local_noise_std holds this rank's [rows, dim] of a per-object noise_std: it goes with local_x and "
                         "excludes `noise_std` (which then is a [dim] vector or a scalar, the same on every rank)")
    if local_noise_std is None and noise_std is None:
        raise ValueError("pass noise_std (or local_noise_std with local_x)")

    def run(rows, cond, probe, seed, sample_offset, **kw):
        std = _local_noise_std(noise_std, local_noise_std, local_x, sample_offset, sample_offset + rows.shape[0])
        out = model.log_prob_noisy(rows, std, *(() if cond is None else (cond,)), num_draws=num_draws, seed=seed,
                                   sample_offset=sample_offset, return_ess=return_ess, **kw)
        return (out[0], out[1].view_as(out[0])) if return_ess else out

    # (randomised: `_log_prob_sharded` hands `run` the seed and the rank's first row -- the noise needs them with any model)
    res = _log_prob_sharded(run, True, x, conditional, seed, group, gather, local_x, n_total, local_conditional, global_control,
                            False, solver)
    if not return_ess:
        return res
    if not gather:
        (lp, ess), span = res
        return (lp, ess.reshape(-1)), span
    return res[0], res[1].reshape(-1)


def _local_noise_std(noise_std, local_noise_std, local_x, lo, hi):
    """This rank's ``noise_std`` for the rows [lo, hi): ``local_noise_std``, its rows of a [B, D] one, or the replicated
    vector / scalar (the rules of ``log_prob_noisy_sharded``)."""
    if local_noise_std is not None:
        if local_noise_std.shape[0] != hi - lo:
            raise ValueError(f"local_noise_std must hold exactly this rank's rows [{lo}, {hi})")
        return local_noise_std
    if torch.is_tensor(noise_std) and noise_std.dim() == 2:
        if local_x is not None:
            raise ValueError("a per-object noise_std beside local_x is local_noise_std (this rank's rows)")
        return noise_std[lo:hi]
    return noise_std


def posterior_noisy_sharded(model, x: Optional[torch.Tensor] = None, noise_std=None, conditional: Optional[torch.Tensor] = None,
                            *, local_x: Optional[torch.Tensor] = None, local_noise_std: Optional[torch.Tensor] = None,
                            n_total: Optional[int] = None, local_conditional: Optional[torch.Tensor] = None, seed: int = 0,
                            num_draws: int = 16, num_samples: int = 1, group=None, gather: bool = True,
                            global_control: bool = True, **solver):
    """``posterior_noisy`` (``ScoreModel``, ``ODEFlow``, ``ConditionalODEFlow``) of a [B, dim] batch of observations over all
    ranks: a ``NoisyPosterior`` of the whole batch on every rank -- with ``gather=False`` ``(NoisyPosterior of this rank's
    rows, (lo, hi))``.  ``x`` / ``local_x`` / ``noise_std`` / ``local_noise_std`` / ``n_total`` / ``conditional`` /
    ``local_conditional``, the keying of the noise draws, the resampling uniforms and a Hutchinson model's probes by
    ``seed`` and the GLOBAL row, and the step control of an adaptive ``method``: exactly ``log_prob_noisy_sharded``; on a
    fixed grid every row of every field is bitwise independent of the number of ranks.  ONE all-gather: the fields travel
    as the columns of one [rows, M D + 2 D + 2 + M] fp32 tensor (samples, mean, var, log_prob, ess, index -- indices up to
    4095 are exact in fp32) and come back in their own shapes and dtypes.  ``**solver`` (atol, rtol, method, options,
    hutchinson, num_probes, chunk_points) goes to ``posterior_noisy`` unchanged."""
    if local_noise_std is not None and (noise_std is not None or local_x is None):
        raise ValueError("local_noise_std holds this rank's [rows, dim] of a per-object noise_std: it goes with local_x and "
                         "excludes `noise_std` (which then is a [dim] vector or a scalar, the same on every rank)")
    if local_noise_std is None and noise_std is None:
        raise ValueError("pass noise_std (or local_noise_std with local_x)")
    from .odeint import NoisyPosterior
    M = int(num_samples)
    lp_shape = []

    def run(rows, cond, probe, seed, sample_offset, **kw):
        std = _local_noise_std(noise_std, local_noise_std, local_x, sample_offset, sample_offset + rows.shape[0])
        post = model.posterior_noisy(rows, std, *(() if cond is None else (cond,)), num_draws=num_draws, num_samples=M,
                                     seed=seed, sample_offset=sample_offset, **kw)
        n = rows.shape[0]
        lp_shape.append(tuple(post.log_prob.shape[1:]))
        return torch.cat([post.samples.reshape(n, -1), post.mean, post.var, post.log_prob.reshape(n, 1),
                          post.ess.reshape(n, 1), post.index.to(torch.float32)], dim=1)

    res = _log_prob_sharded(run, True, x, conditional, seed, group, gather, local_x, n_total, local_conditional, global_control,
                            False, solver)
    packed, span = res if not gather else (res, None)
    n, D = packed.shape[0], (packed.shape[1] - 2 - M) // (M + 2)
    samples, mean, var, lp, ess, index = torch.split(packed, [M * D, D, D, 1, 1, M], dim=1)
    post = NoisyPosterior(samples.reshape(n, M, D), lp.reshape((n,) + lp_shape[0]), ess.reshape(n), mean.contiguous(),
                          var.contiguous(), index.to(torch.int32))
    return post if gather else (post, span)


# ---- the symplectic flows (flowfusion/symplectic.py:166-253) ------------------------------------------------------------------
def symplectic_sample_sharded(model, n_total: int, seed: int = 0, conditional: Optional[torch.Tensor] = None,
                              num_steps: int = 1, group=None, gather: bool = True,
                              local_conditional: Optional[torch.Tensor] = None, method: str = "euler"):
    """``SymplecticFlowModel.sample`` of ``n_total`` prior draws over all ranks.  This rank's rows of the prior [q | p]
    are standard normals of the library's counter-based stream keyed by ``seed`` and the GLOBAL row (``ff_normal_fill``
    with its default noise index, the one reserved for prior draws) -- NOT torch's generator, which the unsharded
    ``sample`` keeps drawing from as the reference does -- so every world size transports the same points and a rank only
    ever touches its own rows.  ``symplectic_log_prob_sharded`` draws its momenta from the same stream and index: pass
    different seeds where the two draws must be unrelated.  The grid is fixed (``num_steps`` steps of ``method``: "euler" or
    "leapfrog"), so there is no
    collective but the final all-gather (``gather=False`` keeps the shard and returns its bounds); a rank without rows is
    fine.  ``conditional`` is the raw [n_total, C] tensor (every rank slices its rows) or ``local_conditional`` this
    rank's rows.  More than one rank over RCCL has not been run on hardware, like everything else multi-rank here."""
    # the joint state is [q | p]: 2 D columns (a model built without `shift` is asked for its networks' state width)
    dim = 2 * int(model.shift.numel()) if model.shift is not None else int(model._net().dim)
    run = lambda x, cond, lo: model._sample_from(x, cond, int(num_steps), **({} if method == "euler" else {"method": method}))
    return _sample_sharded(run, n_total, dim, seed, next(model.model.parameters()).device, conditional, local_conditional,
                           group, gather)


def symplectic_log_prob_sharded(model, x: Optional[torch.Tensor] = None, conditional: Optional[torch.Tensor] = None,
                                seed: int = 0, group=None, gather: bool = True, local_x: Optional[torch.Tensor] = None,
                                n_total: Optional[int] = None, local_conditional: Optional[torch.Tensor] = None,
                                global_control: bool = True, atol: float = 1e-5, rtol: float = 1e-5,
                                method: str = "dopri5", num_steps: Optional[int] = None,
                                num_momenta: Optional[int] = None, return_ess: bool = False):
    """``SymplecticFlowModel.log_prob`` of a [B, D] batch over all ranks; one all-gather of the [B] result at the end.
    ``x`` (and ``conditional``) are the full tensors, every rank slicing its rows -- or ``local_x`` (and
    ``local_conditional``) this rank's rows already, with ``n_total`` the size of the whole batch.  The momentum draw
    ``p0`` comes from the library's counter-based stream keyed by ``seed`` and the GLOBAL row (``ff_normal_fill`` with its
    default noise index, the one reserved for prior draws; not torch's generator, which the unsharded ``log_prob`` keeps
    using as the reference does).  ``symplectic_sample_sharded`` draws from the same stream and index: pass different
    seeds where the two draws must be unrelated.  The solve is adaptive dopri5: with ``global_control`` the step size
    comes from the error norm of the WHOLE batch (``global_step_control``; every rank needs at least one row), so every
    rank takes the same steps and a row's result does not depend on the world size beyond the rounding of those norms;
    ``global_control=False``: every rank steps from its own rows and enters no exchange.  ``method="leapfrog"`` with
    ``num_steps``: the fixed flipped grid of ``sample(.., method="leapfrog")`` in one launch per rank -- no collective but the
    final gather, ``global_control`` is ignored, ranks without rows are fine and a row's result is bitwise independent of
    the world size.  ``num_momenta=K`` (an integer): the marginal over K momentum draws per data point instead
    (``SymplecticFlowModel.log_prob_marginal`` with this ``seed`` and ``sample_offset`` = the rank's first row; the momenta
    are keyed by the global row under noise indices of their own), with ``return_ess=True`` the gathered
    ``(log_p, ess)``; step control and the leapfrog invariance as above.  More than one rank over RCCL has
    not been run on hardware, like everything else multi-rank here."""
    from . import _native
    n, lo, hi, rows, cond = _local_batch(x, local_x, n_total, conditional, local_conditional, group)
    if num_momenta is not None:
        with _step_control(n, group, global_control, method):
            local = model.log_prob_marginal(rows, cond, int(num_momenta), atol, rtol, method=method, num_steps=num_steps,
                                            seed=int(seed), sample_offset=lo, return_ess=return_ess)
        if not return_ess:
            return _finish(local, n, group, gather)
        if not gather:
            return tuple(local), (lo, hi)
        return tuple(_finish(t, n, group, True) for t in local)
    if return_ess:
        raise ValueError("return_ess goes with num_momenta (the one-draw estimate has no weights to count)")
    p0 = _native.normal_fill(hi - lo, int(rows.shape[1]), int(seed), lo, rows.device)
    with _step_control(n, group, global_control, method):
        local = model._log_prob_from(rows, p0, cond, atol, rtol, method=method,
                                     **({} if num_steps is None else {"num_steps": num_steps}))
    return _finish(local, n, group, gather)


def _noise_std_args(noise_std, local_noise_std, local_x):
    """The refusals every noisy sharded entry point shares (``log_prob_noisy_sharded``'s rules)."""
    if local_noise_std is not None and (noise_std is not None or local_x is None):
        raise ValueError("local_noise_std holds this rank's [rows, dim] of a per-object noise_std: it goes with local_x and "
                         "excludes `noise_std` (which then is a [dim] vector or a scalar, the same on every rank)")
    if local_noise_std is None and noise_std is None:
        raise ValueError("pass noise_std (or local_noise_std with local_x)")


def symplectic_log_prob_marginal_noisy_sharded(model, x: Optional[torch.Tensor] = None, noise_std=None,
                                               conditional: Optional[torch.Tensor] = None, *,
                                               local_x: Optional[torch.Tensor] = None,
                                               local_noise_std: Optional[torch.Tensor] = None, n_total: Optional[int] = None,
                                               local_conditional: Optional[torch.Tensor] = None, seed: int = 0,
                                               num_draws: int = 16, group=None, gather: bool = True,
                                               global_control: bool = True, return_ess: bool = False, atol: float = 1e-5,
                                               rtol: float = 1e-5, method: str = "dopri5", num_steps: Optional[int] = None):
    """``SymplecticFlowModel.log_prob_marginal_noisy`` of a [B, D] batch of observations over all ranks; ONE all-gather of the
    [B] result at the end.  ``x`` / ``local_x`` / ``noise_std`` / ``local_noise_std`` / ``n_total`` / ``conditional`` /
    ``local_conditional`` exactly as ``log_prob_noisy_sharded`` takes them: the full tensors, every rank slicing its rows of the
    contiguous balanced shards, or this rank's rows already; a [B, D] ``noise_std`` is cut like ``x``, a [D] vector or a scalar
    is replicated.  The joint (noise, momentum) draws are keyed by ``seed`` and the GLOBAL row (``sample_offset`` = the rank's
    first row).  ``method="leapfrog"`` with ``num_steps``: a fixed grid -- no collective but the final gather,
    ``global_control`` is ignored, ranks without rows are fine and a row's result is bitwise independent of the world size.
    Under an adaptive ``method`` (the default) every rank's ``local * K`` rows are one solve whose step size comes from the
    error norm of the WHOLE expanded batch (``global_step_control``; every rank needs at least one row),
    ``global_control=False``: from the rank's own rows.  ``return_ess=True``: ``(log_p, ess)``, the two gathered as the columns
    of one [rows, 2] tensor -- still one all-gather; with ``gather=False`` ``((log_p, ess), (lo, hi))``.  More than one rank
    over RCCL has not been run on hardware, like everything else multi-rank here."""
    _noise_std_args(noise_std, local_noise_std, local_x)
    n, lo, hi, rows, cond = _local_batch(x, local_x, n_total, conditional, local_conditional, group)
    std = _local_noise_std(noise_std, local_noise_std, local_x, lo, hi)
    with _step_control(n, group, global_control, method):
        local = model.log_prob_marginal_noisy(rows, std, cond, int(num_draws), atol, rtol, method=method, num_steps=num_steps,
                                              seed=int(seed), sample_offset=lo, return_ess=return_ess)
    return _finish(tuple(local) if return_ess else local, n, group, gather)


def symplectic_posterior_marginal_noisy_sharded(model, x: Optional[torch.Tensor] = None, noise_std=None,
                                                conditional: Optional[torch.Tensor] = None, *,
                                                local_x: Optional[torch.Tensor] = None,
                                                local_noise_std: Optional[torch.Tensor] = None, n_total: Optional[int] = None,
                                                local_conditional: Optional[torch.Tensor] = None, seed: int = 0,
                                                num_draws: int = 16, num_samples: int = 1, group=None, gather: bool = True,
                                                global_control: bool = True, atol: float = 1e-5, rtol: float = 1e-5,
                                                method: str = "dopri5", num_steps: Optional[int] = None):
    """``SymplecticFlowModel.posterior_marginal_noisy`` of a [B, D] batch of observations over all ranks: a ``NoisyPosterior``
    of the whole batch on every rank -- with ``gather=False`` ``(NoisyPosterior of this rank's rows, (lo, hi))``.  The batch
    arguments, the keying of the joint draws and the resampling uniforms by ``seed`` and the GLOBAL row, and the step control
    of an adaptive ``method``: exactly ``symplectic_log_prob_marginal_noisy_sharded``; with ``method="leapfrog"`` every row of
    every field is bitwise independent of the number of ranks, and ranks without rows are fine.  ONE all-gather: the fields
    travel as the columns of one [rows, M D + 2 D + 2 + M] fp32 tensor (samples, mean, var, log_prob, ess, index -- indices up
    to 4095 and -1 are exact in fp32), as in ``posterior_noisy_sharded``, and come back in their own shapes and dtypes."""
    _noise_std_args(noise_std, local_noise_std, local_x)
    from .odeint import NoisyPosterior
    M = int(num_samples)
    n, lo, hi, rows, cond = _local_batch(x, local_x, n_total, conditional, local_conditional, group)
    std = _local_noise_std(noise_std, local_noise_std, local_x, lo, hi)
    with _step_control(n, group, global_control, method):
        post = model.posterior_marginal_noisy(rows, std, cond, int(num_draws), M, atol, rtol, method=method,
                                              num_steps=num_steps, seed=int(seed), sample_offset=lo)
    k, D = hi - lo, int(rows.shape[1])
    local = torch.cat([post.samples.reshape(k, M * D), post.mean, post.var, post.log_prob.reshape(k, 1),
                       post.ess.reshape(k, 1), post.index.to(torch.float32)], dim=1)
    res = _finish(local, n, group, gather)
    packed, span = res if not gather else (res, None)
    rows_out = packed.shape[0]
    samples, mean, var, lp, ess, index = torch.split(packed, [M * D, D, D, 1, 1, M], dim=1)
    post = NoisyPosterior(samples.reshape(rows_out, M, D), lp.reshape(rows_out), ess.reshape(rows_out), mean.contiguous(),
                          var.contiguous(), index.to(torch.int32))
    return post if gather else (post, span)
