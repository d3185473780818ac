"""Symplectic flows without a GPU: the mirror of the reference's classes against its fixtures, the host schedule, the
two-network planner and the pair weight pack, decoded half by half and emulated in float64."""
import inspect
import math

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.fused import MODE_STATE, FusedEnvelopeWarning
from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
from tests._emulator import decode_wpack
from tests._symplectic_ref import SymplecticRef, euler_rotation, rotation_weights
from tests._util import golden_names, load_golden

CASES = golden_names("sym_")
EXPECTED_KERNEL = {"sym_2d": "mlp_pair_m32_h64_d16_c8", "sym_16d_2x256": "mlp_pair_m16_h256_d8_c4_w2",
                   "sym_5d_c3_ragged": "mlp_pair_m16_h128_d8_c4_w3", "sym_20d_outside": None}


def build_model(meta, arrays):
    """The product's model with a fixture's weights (loaded strictly); returns (model, state_dict)."""
    D, C, E, units = meta["D"], meta["C"], meta["E"], meta["units"]
    m = SymplecticMLP(D, C, E, units)
    fm = SymplecticFlowModel(m, torch.zeros(D), torch.ones(D), torch.zeros(C) if C else None, torch.ones(C) if C else None)
    sd = {k[3:]: v for k, v in arrays.items() if k.startswith("sd.")}
    fm.load_state_dict(sd, strict=True)
    return fm, sd


def test_fixtures_present():
    assert CASES == sorted(EXPECTED_KERNEL)


@pytest.mark.parametrize("name", CASES)
def test_signatures_and_state_dict_layout(name):
    meta, arrays = load_golden(name)
    sigs = meta["signatures"]
    assert str(inspect.signature(SymplecticMLP.__init__)) == sigs["SymplecticMLP.__init__"]
    assert str(inspect.signature(SymplecticMLP.forward)) == sigs["SymplecticMLP.forward"]
    assert str(inspect.signature(SymplecticFlowModel.__init__)) == sigs["SymplecticFlowModel.__init__"]
    assert str(inspect.signature(SymplecticFlowModel.sample)) == sigs["SymplecticFlowModel.sample"]
    assert str(inspect.signature(SymplecticFlowModel.log_prob)) == sigs["SymplecticFlowModel.log_prob"]
    fm, _ = build_model(meta, arrays)
    assert list(fm.state_dict().keys()) == meta["state_dict_keys"]
    assert list(fm.model.state_dict().keys()) == meta["mlp_state_dict_keys"]


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference(name):
    meta, arrays = load_golden(name)
    fm, sd = build_model(meta, arrays)
    cond = arrays.get("cond")
    cond_n = fm._norm_cond(cond)
    with torch.no_grad():
        for t, want in ((arrays["t_vec"], arrays["fwd_vec"]), (arrays["t_scalar"], arrays["fwd_scalar"])):
            got = fm.model(t, arrays["state"], cond_n)
            assert got.shape == want.shape
            assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    # the float64 restatement the GPU tests rely on agrees with the reference's forward and sampler
    ref = SymplecticRef(sd)
    got = ref.forward(arrays["t_vec"], arrays["state"], ref.norm_cond(cond))
    assert float((got - arrays["fwd_vec"].double()).abs().max()) < 1e-5 * max(1.0, float(arrays["fwd_vec"].abs().max()))
    for n in meta["steps"]:
        want = arrays[f"sample_{n}"].double()
        got = ref.sample_from(arrays[f"prior_{n}"], cond, n)
        assert float((got - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max())), n


@pytest.mark.parametrize("name", CASES)
def test_routes_and_planner(name):
    """In-envelope shapes land on the expected pair instance; the out-of-envelope fixture is refused by the planner
    and the front end says so."""
    meta, arrays = load_golden(name)
    fm, _ = build_model(meta, arrays)
    D, units = meta["D"], meta["units"]
    expect = EXPECTED_KERNEL[name]
    if expect is None:
        with pytest.raises(NotImplementedError):
            _native.make_pair_plan(2 * D, meta["C"], units)
        with pytest.warns(FusedEnvelopeWarning):
            assert not fm._fusable()
        return
    assert fm._fusable()
    plan = fm._net().plan(MODE_STATE)
    assert _native.kernel_name(plan) == expect
    assert _native.is_pair_plan(plan) and _native.row_width(plan) == 2 * plan.width
    assert _native.lib().ff_mlp_wpack_floats(plan) == 0          # the single-network calls do not take a pair plan
    with pytest.raises(NotImplementedError):
        fm._net().plan(_native.MODE_EXACT)


def test_planner_envelope():
    L = _native.lib()
    names = {L.ff_pair_kernel_name(i).decode() for i in range(L.ff_pair_kernel_count())}
    assert names == {v for v in EXPECTED_KERNEL.values() if v}
    for dim, c, u in [(2, 0, [64]), (32, 16, [256, 256]), (10, 3, [100, 128]), (32, 0, [128] * 3), (4, 16, [64])]:
        _native.make_pair_plan(dim, c, u)
    for dim, c, u in [(34, 0, [64]), (8, 17, [64]), (8, 0, [257])]:
        with pytest.raises(NotImplementedError):
            _native.make_pair_plan(dim, c, u)
    with pytest.raises(RuntimeError):
        _native.make_pair_plan(5, 0, [64])                       # odd state: no [q | p] split


def test_silu_only_and_other_modules_take_the_generic_route():
    m = SymplecticMLP(3, 0, 4, [32], activation=torch.nn.Tanh())
    fm = SymplecticFlowModel(m, torch.zeros(3), torch.ones(3), None, None)
    with pytest.warns(FusedEnvelopeWarning):
        assert not fm._fusable()

    class Other(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(6, 6)

        def forward(self, t, state, conditional):
            return self.lin(state)
    assert not SymplecticFlowModel(Other(), torch.zeros(3), torch.ones(3), None, None)._fusable()


def test_cpu_tensors_raise():
    fm = SymplecticFlowModel(SymplecticMLP(2, 0, 4, [32]), torch.zeros(2), torch.ones(2), None, None)
    with pytest.raises(RuntimeError):
        fm.sample((4, 2), num_steps=2)
    with pytest.raises(RuntimeError):
        fm.log_prob(torch.zeros(4, 2))


@pytest.mark.parametrize("name", ["sym_5d_c3_ragged", "sym_16d_2x256"])
def test_host_c1_is_the_first_layer_time_part(name):
    meta, arrays = load_golden(name)
    fm, sd = build_model(meta, arrays)
    D, C = meta["D"], meta["C"]
    H = fm._net().plan(MODE_STATE).width
    t = torch.tensor([0.0, 0.13, 0.5, 0.77, 1.0])
    a, b, c1 = fm._schedule(t)
    assert a.eq(0).all() and b.eq(1).all() and c1.shape == (5, 2 * H)
    ref = SymplecticRef(sd)
    arg = t.double()[:, None] * ref.W[None, :] * 2 * math.pi
    emb = torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)
    for i, layers in enumerate(ref.nets):
        w0, b0 = layers[0]
        want = emb @ w0[:, D + C:].T + b0            # the first layer's pre-activation with zero state / conditional inputs
        h = w0.shape[0]
        assert float((c1[:, i * H:i * H + h].double() - want).abs().max()) < 1e-5 * max(1.0, float(want.abs().max()))
        assert c1[:, i * H + h:(i + 1) * H].eq(0).all()


def _emulate_pair(plan, wpack, table, x, cond, k1=None, n_aux=0):
    """The pair kernel's evaluation loop in float64, each half decoded by tests/_emulator.decode_wpack.  ``k1``: stage slot
    0 as the caller supplies it (k1_in).  ``n_aux`` = 1: the table's last two rows are the auxiliary rows of an adaptive
    attempt, not evaluations, and the return value is (x, aux_0) with aux_0 = use_y x + sum_s cin[s] k[s] of the first."""
    words = _native.plan_words(plan)
    n = wpack.numel() // 2
    halves = [decode_wpack(words, wpack[:n]), decode_wpack(words, wpack[n:])]
    H, D2 = plan.width, plan.dim
    rows = table.double()
    ints = table.view(torch.int32)
    B = x.shape[0]
    ks = torch.zeros(7, B, D2, dtype=torch.float64)
    if k1 is not None:
        ks[0] = k1.double()
    x = x.double()
    n_evals = table.shape[0] - (2 if n_aux else 0)
    for e in range(n_evals):
        y = x + sum(rows[e, 8 + s] * ks[s] for s in range(7))
        net = torch.zeros(B, D2, dtype=torch.float64)
        for i, (W1, hidden, Wo, bo, dx) in enumerate(halves):
            inp = torch.zeros(B, W1.shape[1], dtype=torch.float64)
            inp[:, :D2] = y
            if cond is not None:
                inp[:, dx:dx + cond.shape[1]] = cond.double()
            h = inp @ W1.T + rows[e, 32 + i * H:32 + (i + 1) * H]
            h = h * torch.sigmoid(h)
            for Wl, bl in hidden:
                h = h @ Wl.T + bl
                h = h * torch.sigmoid(h)
            net += (h @ Wo.T + bo)[:, :D2]
        ks[int(ints[e, 4])] = rows[e, 0] * y + rows[e, 1] * net
        if int(ints[e, 3]) & 1:
            x = x + sum(rows[e, 16 + s] * ks[s] for s in range(7))
    if n_aux:
        use_y = float(int(ints[n_evals, 3]) & 1)
        return x, use_y * x + sum(rows[n_evals, 8 + s] * ks[s] for s in range(7))
    return x


@pytest.mark.parametrize("name", ["sym_2d", "sym_5d_c3_ragged", "sym_16d_2x256"])
def test_pair_pack_reproduces_the_euler_sample(name):
    meta, arrays = load_golden(name)
    fm, sd = build_model(meta, arrays)
    net = fm._net()
    plan = net.plan(MODE_STATE)
    wpack = net.wpack("cpu", MODE_STATE)
    cond = arrays.get("cond")
    cond_n = fm._norm_cond(cond)
    ref = SymplecticRef(sd)
    for n in (1, 4):
        prior = arrays[f"prior_{n}"]
        table = fm._ode_table(torch.linspace(1.0, 0.0, n + 1), "euler", None, MODE_STATE)
        z = _emulate_pair(plan, wpack, table, prior, cond_n)
        got = z[:, :meta["D"]] * ref.scale + ref.shift
        want = ref.sample_from(prior, cond, n)
        assert float((got - want).abs().max()) < 1e-5 * max(1.0, float(want.abs().max())), n


def test_known_answer_weights_restated():
    """The rotation construction the GPU test uses, checked on the CPU module: v = [alpha p, -beta q]."""
    D, C, E, units, alpha, beta = 5, 3, 6, [32, 32, 32], 0.7, 1.3
    m = SymplecticMLP(D, C, E, units)
    m.load_state_dict({**rotation_weights(D, C, E, units, alpha, beta), "W": m.W}, strict=True)
    z = torch.randn(64, 2 * D)
    with torch.no_grad():
        v = m(torch.rand(64), z, torch.randn(64, C))
    want = torch.cat([alpha * z[:, D:], -beta * z[:, :D]], dim=1)
    assert float((v - want).abs().max()) < 1e-5 * float(want.abs().max())
    zz = euler_rotation(z, D, 1.0, 1.0, 1)
    assert torch.allclose(zz, torch.cat([z[:, :D] - z[:, D:], z[:, D:] + z[:, :D]], dim=1).double())
