"""Hutch++ / XTrace solves outside the device-resident adaptive path (device_adaptive.py, which is where the reference's
default-argument calls run since round 4).

* ``run_table_recorded``: FIXED grids -- the state never depends on the divergence, so the whole table runs as one fused
  launch per tangent pass with the Jacobian of every row recorded (``ff_ode_args.jac_all``), ONE ``ff_trace_estimate``
  launch turns them into estimates, and the rows are combined with the tableau's weights.
* ``run_table_products``: the same solves WITHOUT the Jacobians (opt-in, ``products="vjp"``) -- two sweeps of the products
  unit (``ff_mlp_ode_launch_vjp``: ``A v = a v + b J_net^T v`` of every row, as the reference's reverse-mode estimators
  obtain them) with ``ff_trace_basis`` between and ``ff_trace_combine`` after them.
* ``rhs_div`` / ``make_step`` / ``run_table``: row-by-row execution -- each right-hand side one launch
  (``flowfusion_amd::mlp_rhs_jac``: the value and its full Jacobian from unit tangents, the network still fused), the
  estimate by ``div_fn``, the Runge-Kutta bookkeeping (the kernel's ``cin`` / ``cout`` / slot semantics) on the host.  This
  is the HOST-controller route of an adaptive estimator solve (``FF_HOST_CONTROLLER=1``, SDE classes the device controller
  does not know, Jacobians beyond the memory budget) and what the CPU tests drive with the kernel-semantics emulator.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import _native
from ._native import MODE_EXACT, f32_on
from .fused import FusedNet, exact_trace_passes
from .solvers import FLAG_STEP_END, MAX_SLOTS, ROW_A, ROW_B, ROW_CIN, ROW_COUT, ROW_FLAGS, ROW_HDR, ROW_SLOT


def row_weights(table: torch.Tensor) -> torch.Tensor:
    """Weight of every evaluation row's divergence in the integral over a (CPU) fixed-grid table: the step-update
    coefficients applied to the slot the row's right-hand side sits in ([n], float32)."""
    n = int(table.shape[0])
    ints = table.view(torch.int32)
    w = torch.zeros(n, dtype=torch.float64)
    owner = {}
    for e in range(n):
        owner[int(ints[e, ROW_SLOT])] = e
        if int(ints[e, ROW_FLAGS]) & FLAG_STEP_END:
            for s in range(MAX_SLOTS):
                c = float(table[e, ROW_COUT][s])
                if c != 0.0 and s in owner:
                    w[owner[s]] += c
    return w.to(torch.float32)


def sum_rows(t: torch.Tensor) -> torch.Tensor:
    """[n, b] -> [b]: the sum over the rows by pairwise halving, elementwise additions only -- the order of every column's
    sum depends on n alone, so a batch cut into chunks sums to the same bits (a reduction kernel's order may depend on how
    many columns it serves)."""
    if t.shape[0] == 0:
        return t.new_zeros(t.shape[1:])
    while t.shape[0] > 1:
        if t.shape[0] & 1:
            t = torch.cat([t, torch.zeros_like(t[:1])])
        t = t[0::2] + t[1::2]
    return t[0]


class RowStepper:
    def __init__(self, net: FusedNet, device, cond: Optional[torch.Tensor],
                 div_fn: Callable[[torch.Tensor], torch.Tensor], launcher=None):
        """``div_fn(A)`` maps A[b] = J[b]^T ([B, D, D]) to the divergence estimate [B].  ``launcher(y, rows, first,
        count, jac) -> rhs`` replaces the GPU launch in the CPU tests."""
        self.net = net
        self.device = device
        self.div_fn = div_fn
        plan = net.plan(MODE_EXACT)
        self.width = int(plan.width)
        self.passes = exact_trace_passes(net.dim, plan.tile)
        cond_d = f32_on(cond, device) if net.cond_dim > 0 else None
        if launcher is None:
            words = _native.plan_words(plan)
            wpack = net.wpack(device, MODE_EXACT)
            launcher = lambda y, rows, first, count, jac: torch.ops.flowfusion_amd.mlp_rhs_jac(
                y, cond_d, wpack, rows.to(device), words, first, count, jac)
        self.launcher = launcher
        self.n_evals = 0

    def rhs_div(self, y: torch.Tensor, a: float, b: float, c1: torch.Tensor):
        """(rhs [B, D], divergence estimate [B]) of  a*y + b*NET(y; c1)."""
        rows = torch.zeros(3, ROW_HDR + self.width, dtype=torch.float32)
        rows[0, ROW_A], rows[0, ROW_B] = a, b
        rows[0, ROW_HDR:ROW_HDR + c1.numel()] = c1
        rows[1, ROW_CIN.start] = 1.0                       # auxiliary output 0 = stage slot 0 = the right-hand side
        y = y.contiguous()
        jac = torch.empty(y.shape[0], self.net.dim, self.net.dim, dtype=torch.float32, device=y.device)
        rhs = None
        for first, count in self.passes:
            rhs = self.launcher(y, rows, first, count, jac)
        self.n_evals += 1
        return rhs, self.div_fn(jac)

    def run_table(self, x: torch.Tensor, table: torch.Tensor):
        """Fixed-grid integration over the rows of a (CPU) evaluation table; returns (x_final, dlogp [B])."""
        ints = table.view(torch.int32)
        ks = [torch.zeros_like(x) for _ in range(MAX_SLOTS)]
        kl = [torch.zeros(x.shape[0], device=x.device) for _ in range(MAX_SLOTS)]
        lp = torch.zeros(x.shape[0], device=x.device)
        for e in range(table.shape[0]):
            cin, cout = table[e, ROW_CIN], table[e, ROW_COUT]
            y = x.clone()
            for s in range(MAX_SLOTS):
                if float(cin[s]) != 0.0:
                    y = y + float(cin[s]) * ks[s]
            slot = int(ints[e, ROW_SLOT])
            ks[slot], kl[slot] = self.rhs_div(y, float(table[e, ROW_A]), float(table[e, ROW_B]), table[e, ROW_HDR:])
            if int(ints[e, ROW_FLAGS]) & FLAG_STEP_END:
                for s in range(MAX_SLOTS):
                    if float(cout[s]) != 0.0:
                        x = x + float(cout[s]) * ks[s]
                        lp = lp + float(cout[s]) * kl[s]
        return x, lp

    def run_table_recorded(self, x: torch.Tensor, table: torch.Tensor, div_rows, cond=None, max_bytes: int = 1 << 30):
        """Fixed-grid integration WITHOUT host stepping: the state never depends on the divergence, so the whole table
        runs as one fused launch per tangent pass with the Jacobian of every row recorded (ff_ode_args.jac_all), the
        estimator is evaluated for all rows at once (``div_rows(A [n, b, D, D], lo, hi) -> [n, b]`` for samples
        lo..hi), and the estimates are combined with the weights the tableau gives each row.  The batch is cut so that
        a chunk's Jacobians stay under ``max_bytes``.  Returns (x_final, dlogp [B])."""
        n, D, B = int(table.shape[0]), self.net.dim, int(x.shape[0])
        w = row_weights(table).to(x.device)
        dev = x.device
        plan = self.net.plan(MODE_EXACT)
        words = _native.plan_words(plan)
        wpack = self.net.wpack(dev, MODE_EXACT)
        tab = table.to(dev)
        cond_d = f32_on(cond, dev) if self.net.cond_dim > 0 else None
        chunk = max(1, min(B, max_bytes // max(1, n * D * D * 4)))
        outs, lps = [], []
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            xc = x[lo:hi].contiguous()
            cc = None if cond_d is None else cond_d[lo:hi].contiguous()
            jac = torch.empty(n, hi - lo, D, D, dtype=torch.float32, device=dev)
            for first, count in self.passes:
                xo = torch.ops.flowfusion_amd.mlp_ode_jacobians(xc, cc, wpack, tab, words, first, count, jac)
            outs.append(xo)
            lps.append((w[:, None] * div_rows(jac, lo, hi)).sum(dim=0))
            self.n_evals += n
        return torch.cat(outs), torch.cat(lps)

    def run_table_products(self, x: torch.Tensor, table: torch.Tensor, kind: str, probes, cond=None,
                           max_bytes: int = 1 << 30, stage_slots: int = 0, launcher=None):
        """``run_table_recorded`` without the recorded Jacobians: Hutch++ / XTrace from J^T v products, as the reference
        computes them (diffusion.py:356-398, :419-455).  The state never depends on the divergence, so per chunk of samples
        the solve runs TWICE on the products unit (``FusedNet.vjp_products``), with one streaming launch after each sweep:

        1. sweep 1: ``Y[e, b, c] = A(y_e) p_c`` for the solve's sketch probes (S of ``probes = (S, G)``, or O of ``(O,)``);
        2. ``_native.trace_basis``: Householder QR of every ``Y[e, b]``, the second sweep's seeds ``Q | U`` (or ``Q``, and R);
        3. sweep 2: ``Z[e, b, c] = A(y_e) seed[e, b, c]``, seeds per evaluation row;
        4. ``_native.trace_combine``: the estimate ``div[e, b]``; the rows are combined with ``row_weights``.

        ``probes`` as the reference stores them ([n_probes, B, D]).  The batch is cut so that a chunk's seed and product
        buffers, ``rows * n * (K1 + 2 K2) * D * 4`` bytes (K1 sketch probes, K2 second-sweep seeds), stay under
        ``max_bytes``; samples are independent, so the cut does not change a bit of the result.  ``launcher(x, cond, table,
        seeds, per_row) -> (x_out, prod [n, b, K, D])`` replaces the GPU launch in the CPU tests (the streaming steps then
        run through their host twins).  Returns (x_final, dlogp [B])."""
        code, p0, p1, r, m = _native.trace_kind_and_probes(kind, probes)
        n, D, B = int(table.shape[0]), int(x.shape[1]), int(x.shape[0])
        K2 = r + m if code == _native.TRACE_HUTCHPP else r
        dev = x.device
        host = dev.type == "cpu"
        w = row_weights(table).to(dev)
        tab = table.to(dev)
        if launcher is None:
            def launcher(xc, cc, tab, seeds, per_row):
                out = self.net.vjp_products(xc, tab, seeds, per_row=per_row, cond=cc, stage_slots=stage_slots)
                return out[0], out[1]
        cond_d = f32_on(cond, dev) if cond is not None else None
        chunk = max(1, min(B, max_bytes // max(1, n * (r + 2 * K2) * D * 4)))
        outs, lps = [], []
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            xc = x[lo:hi].contiguous()
            cc = None if cond_d is None else cond_d[lo:hi].contiguous()
            pc = tuple(f32_on(P[:, lo:hi], dev) for P in probes)
            xo, Y = launcher(xc, cc, tab, pc[0].permute(1, 0, 2).contiguous(), False)
            basis, rfac = _native.trace_basis(Y, kind, pc, host=host)
            _, Z = launcher(xc, cc, tab, basis, True)
            div = _native.trace_combine(basis, rfac, Z, kind, pc, host=host)
            outs.append(xo)
            lps.append(sum_rows(w[:, None] * div))
            self.n_evals += 2 * n
        return torch.cat(outs), torch.cat(lps)

    def make_step(self, schedule, sign: float):
        """Step function for ``adaptive.Dopri5`` (same contract as ``FusedNet.make_step``)."""
        def step(y, k1, lp0, kl1, t_rows, cin, slots, tail, use_y, n_aux):
            a, b, c1 = schedule(sign * t_rows)
            ks = [torch.zeros_like(y) for _ in range(MAX_SLOTS)]
            kl = [torch.zeros(y.shape[0], device=y.device) for _ in range(MAX_SLOTS)]
            if k1 is not None:
                ks[0] = k1
            if kl1 is not None:
                kl[0] = kl1
            for i in range(int(t_rows.numel())):
                yi = y.clone()
                for s in range(MAX_SLOTS):
                    if float(cin[i, s]) != 0.0:
                        yi = yi + float(cin[i, s]) * ks[s]
                slot = int(slots[i])
                ks[slot], kl[slot] = self.rhs_div(yi, float(sign * a[i]), float(sign * b[i]), c1[i])
            aux = torch.zeros(n_aux, *y.shape, device=y.device)
            aux_lp = torch.zeros(n_aux, y.shape[0], device=y.device)
            for j in range(n_aux):
                if (use_y >> j) & 1:
                    aux[j] = aux[j] + y
                    if lp0 is not None:
                        aux_lp[j] = aux_lp[j] + lp0
                for s in range(MAX_SLOTS):
                    cj = float(tail[j, s])
                    if cj != 0.0:
                        aux[j] = aux[j] + cj * ks[s]
                        aux_lp[j] = aux_lp[j] + cj * kl[s]
            return aux, aux_lp
        return step
