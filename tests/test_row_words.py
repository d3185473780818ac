"""The evaluation rows the host steppers write, byte for byte against a construction by literal word index (the layout of
ff::RowHdr in csrc/ff_layout.h and of the two auxiliary rows of ff_ode_args in include/flowfusion_amd.h, restated here and
independent of the names flowfusion_amd/solvers.py gives the words)."""
import torch
from torch import nn

from flowfusion_amd import adaptive
from flowfusion_amd.fused import MODE_STATE, FusedNet
from flowfusion_amd.host_stepper import RowStepper

D, H = 3, 40          # 40 hidden units: the first-layer bias c1 is narrower than the width the kernel pads it to


def _net():
    torch.manual_seed(0)
    return FusedNet([nn.Linear(1 + D, H), nn.Linear(H, H), nn.Linear(H, D)], D, 0, x_col0=1, c_col0=1 + D)


def _schedule(t):
    """A fake schedule: (a, b, c1) of the real times ``t``, every row and word different."""
    return 2.0 * t, t + 1.0, torch.outer(t, torch.arange(1.0, H + 1.0)) + 0.25


def _same_bytes(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_attempt_table_of_make_step_word_by_word(built_library):
    net = _net()
    width = net.width(MODE_STATE)
    assert width > H
    seen = []

    def capture(y, k1, kl1, lp0, etab, n_aux, first, count):
        seen.append(etab.clone())
        return torch.zeros(n_aux, *y.shape), torch.zeros(n_aux, 0)

    sign = -1.0
    step = net.make_step(_schedule, sign, MODE_STATE, "cpu", launcher=capture)
    handed = []
    solver = adaptive.Dopri5(lambda *args: handed.append(args) or step(*args), False, 1e-5, 1e-5)
    y = torch.randn(5, D)
    solver._attempt(0.25, 0.125, 0.375, y, None, torch.randn(5, D), None)          # one dopri5 attempt: stages 2..7
    (_, _, _, _, ts, cin, slots, tail, use_y, n_aux), (got,) = handed[0], seen
    assert (ts.numel(), tuple(cin.shape), slots.tolist(), tuple(tail.shape), use_y, n_aux) == (6, (6, 8), [1, 2, 3, 4, 5, 6], (4, 8), 0b0101, 4)
    a, b, c1 = _schedule(sign * ts)
    want = torch.zeros(6 + 2, 32 + width, dtype=torch.float32)
    ints = want.view(torch.int32)
    for i in range(6):
        want[i, 0] = sign * a[i]
        want[i, 1] = sign * b[i]
        ints[i, 4] = i + 1
        for s in range(8):
            want[i, 8 + s] = cin[i, s]
        for h in range(H):
            want[i, 32 + h] = c1[i, h]
    for s in range(8):
        want[6, 8 + s], want[6, 16 + s] = tail[0, s], tail[1, s]
        want[7, 8 + s], want[7, 16 + s] = tail[2, s], tail[3, s]
    ints[6, 3] = 0b0101
    assert _same_bytes(got, want)


def test_three_row_table_of_rhs_div_word_by_word(built_library):
    net = _net()
    seen = []

    def capture(y, rows, first, count, jac):
        seen.append((rows.clone(), first, count))
        return torch.zeros_like(y)

    stepper = RowStepper(net, "cpu", None, lambda jac: torch.zeros(jac.shape[0]), launcher=capture)
    c1 = torch.arange(1.0, H + 1.0) * 0.5
    stepper.rhs_div(torch.randn(5, D), -1.5, 0.75, c1)
    want = torch.zeros(3, 32 + stepper.width, dtype=torch.float32)
    want[0, 0], want[0, 1] = -1.5, 0.75
    for h in range(H):
        want[0, 32 + h] = c1[h]
    want[1, 8] = 1.0
    assert [(f, c) for _, f, c in seen] == stepper.passes and all(_same_bytes(rows, want) for rows, _, _ in seen)
