"""The instance table of the two-network kernels (csrc/ff_mlp_pair.hpp): tests/test_pair_instance_table.py on the CPU,
tests/test_gpu_pair_instances.py on the GPU.  The pair family is not in the ``ff_kernel_count`` table, so tests/_instances.py
does not reach it; this is the same idea for ``ff_pair_kernel_count`` / ``ff_pair_kernel_name`` (build.py ``PAIR_INSTANCES``,
their row-select variants ``PAIR_SELECT_INSTANCES`` and the cooperative twins of both).

Every instance has three rows, each a network shape ``ff_mlp_pair_plan`` (and ``ff_mlp_pair_select_plan``) must land on it.
``D`` is per half: the state [q | p] has 2D dimensions.

* ``top``: the largest state, conditional width and hidden width the instance holds, five hidden layers of ragged widths
  (H - 1, H, just above the next narrower instance, H, H - 1): every state and conditional register live, the last of each
  full;
* ``bottom``: the smallest shape that still lands on it -- one state dimension per half, no conditional input, one hidden
  layer one unit wider than the next narrower instance holds (one unit on the narrowest);
* ``split``: an even number of layers (the twin's exchange buffers alternate over the whole launch, not per network), an odd
  D (the q | p boundary falls inside a register where a register holds two features, and off the four-register groups
  elsewhere) and a lone conditional input.

The table is static on purpose: an instance added to the build without rows here fails test_pair_instance_table.py by name.

Inputs.  Default-initialised networks give a field of about a fortieth of the state, and a solved state that is almost all
prior: a weight-path error of a few percent then stays under any bar the fp32 arithmetic allows.  ``gained_model`` draws
weights N(0, 1.5^2 / fan_in) and biases N(0, 0.3^2) instead, which makes the field as large as the state; ``controls`` are
the four 1e-3 perturbations of the edge weights a comparison on these inputs must see."""
import math
from collections import namedtuple

import torch

Row = namedtuple("Row", "kernel corner D C units")


def R(*a):
    return Row(*a)


ROWS = [
    R('mlp_pair_m32_h64_d16_c8', 'top', 16, 16, (63, 64, 33, 64, 63)),
    R('mlp_pair_m32_h64_d16_c8', 'bottom', 1, 0, (1,)),
    R('mlp_pair_m32_h64_d16_c8', 'split', 15, 1, (33, 50)),
    R('mlp_pair_m16_h128_d8_c4_w3', 'top', 16, 16, (127, 128, 65, 128, 127)),
    R('mlp_pair_m16_h128_d8_c4_w3', 'bottom', 1, 0, (65,)),
    R('mlp_pair_m16_h128_d8_c4_w3', 'split', 15, 1, (65, 100)),
    R('mlp_pair_m16_h256_d8_c4_w2', 'top', 16, 16, (255, 256, 129, 256, 255)),
    R('mlp_pair_m16_h256_d8_c4_w2', 'bottom', 1, 0, (129,)),
    R('mlp_pair_m16_h256_d8_c4_w2', 'split', 15, 1, (129, 200)),
]
CORNERS = ("top", "bottom", "split")
SEED = 111                          # of gained_model and draw, every row (101-110 each miss a condition of
                                    # test_the_bars_can_tell_on_these_inputs at a bottom row)
E = 16                              # time features
STEPS = 3                           # Euler / leapfrog steps of the grid linspace(1, 0, STEPS + 1)
RK4_STEP = 0.25                     # fixed-grid RK4 over [0, 1]: four steps, four stage slots each

PAIR, SELECT = "pair", "select"
ONE_WAVE, TWIN, TAIL = "one_wave", "twin", "one_wave+twin"

Entry = namedtuple("Entry", "tile width wps coop select")


def registry():
    """{pair kernel name: Entry(tile, width, wavefronts per SIMD, has cooperative twins, has a row-select variant)} as
    build.py declares it."""
    from flowfusion_amd import build as B
    return {B._pair_name(*i): Entry(i[0], i[1], i[4], B._has_coop(i[1]), i in B.PAIR_SELECT_INSTANCES) for i in B.PAIR_INSTANCES}


def variants(entry):
    return [PAIR] + ([SELECT] if entry.select else [])


def variant_name(kernel, variant):
    """The name ff_plan_kernel_name gives the variant's plan."""
    return kernel if variant == PAIR else kernel.replace("mlp_pair_", "mlp_pairsel_", 1)


def launch_kinds(entry):
    """The launch kinds an instance serves, pair and select alike: its one-wavefront kernel (FF_COOP=0), its cooperative
    twin (FF_COOP=1) and, with both, whole rounds of the chip on the one-wavefront kernel and the leftover tiles on the twin."""
    return [ONE_WAVE] + ([TWIN, TAIL] if entry.coop else [])


def chip_tiles(entry):
    """Tiles the chip runs at once on the one-wavefront kernel: 1024 SIMDs x wavefronts per SIMD."""
    return 1024 * entry.wps


def solve_modes(variant, kind):
    """What the GPU test runs on a variant in a launch kind.  ``attempt`` (k1_in, attempt-style rows, aux_out[0]) is a raw
    launch, which takes one kernel: not the tail split."""
    if variant == SELECT:
        return ["leapfrog", "leapfrog_logp"]
    return ["euler", "rk4"] + ([] if kind == TAIL else ["attempt"])


def expected_coverage():
    """{(kernel name of the variant, variant, launch kind, mode)} the GPU test must pass."""
    return {(variant_name(name, v), v, kind, mode) for name, e in registry().items() for v in variants(e)
            for kind in launch_kinds(e) for mode in solve_modes(v, kind)}


def plan_row(row, select=False, D=None, C=None, units=None):
    """(kernel name, plan) the pair planner picks for a row, or for a shape next to it; (None, None) where no instance
    holds the shape."""
    from flowfusion_amd import _native as N
    try:
        p = N.make_pair_plan(2 * (row.D if D is None else D), row.C if C is None else C,
                             list(row.units if units is None else units), select=select)
    except NotImplementedError:
        return None, None
    return N.kernel_name(p), p


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def gained_model(row, seed=None):
    """SymplecticFlowModel on the CPU for a row: tests/test_gpu_symplectic_twin.seeded_model's construction (E = 16, its
    shift / scale draws), then every Linear of mlp_q and of mlp_p redrawn: weight ~ N(0, 1.5^2 / fan_in), bias ~ N(0, 0.3^2)."""
    from flowfusion_amd.symplectic import SymplecticFlowModel, SymplecticMLP
    D, C = row.D, row.C
    torch.manual_seed(SEED if seed is None else seed)
    m = SymplecticMLP(D, C, E, list(row.units))
    shift, scale = torch.randn(D) * 0.3, torch.rand(D) + 0.5
    cs = (torch.randn(C) * 0.2, torch.rand(C) + 0.5) if C else (None, None)
    with torch.no_grad():
        for net in (m.mlp_q_dynamics, m.mlp_p_dynamics):
            for l in net:
                if isinstance(l, torch.nn.Linear):
                    l.weight.normal_(0.0, 1.5 / math.sqrt(l.in_features))
                    l.bias.normal_(0.0, 0.3)
    return SymplecticFlowModel(m, shift, scale, *cs).eval()


CONTROLS = ("out_row_q", "out_row_p", "cond_col", "state_col")


def controls(state_dict, D, C):
    """{name: perturbed copy of the state_dict}: x 1.001 on the last output row of mlp_q, of mlp_p, on the last conditional
    column of both first layers (none when C = 0) and on the last state column of both first layers -- the weights the last
    state and conditional registers of a top corner carry."""
    nets = ("mlp_q_dynamics", "mlp_p_dynamics")
    last = max(int(k.split(".")[2]) for k in state_dict if k.startswith(f"model.{nets[0]}.") and k.endswith(".weight"))
    out = {}

    def copy():
        return {k: v.detach().clone() for k, v in state_dict.items()}
    for name, net in zip(CONTROLS[:2], nets):
        sd = copy()
        sd[f"model.{net}.{last}.weight"][D - 1, :] *= 1.001
        out[name] = sd
    for name, col in ((CONTROLS[2], D + C - 1 if C else None), (CONTROLS[3], D - 1)):
        if col is None:
            continue
        sd = copy()
        for net in nets:
            sd[f"model.{net}.0.weight"][:, col] *= 1.001
        out[name] = sd
    return out


def batch(tiles, tile):
    return tiles * tile - 1                                    # (a partly filled last tile)


def batches(kind, corner, tile, chip):
    """The smallest batches that reach the edges: the one-wavefront kernel's workgroup holds four tiles, so 5 / 7 tiles are
    one / three tiles past a multiple of it; the twin runs a tile per workgroup; the tail split needs a whole round of the
    chip and a few tiles."""
    if kind == ONE_WAVE:
        return [1, batch(5, tile)] if corner == "top" else [batch(7, tile)]
    if kind == TWIN:
        return [1, batch(3, tile)]
    return [batch(chip + 3, tile)]


def control_batch(tile):
    return batch(5, tile)


def sample_rows(B, tile, chip, seed):
    """At most 32 rows of a batch of B (the idea of tests/test_gpu_instances._sample_rows): the first tile, the boundaries
    of the first workgroups, the last row of the whole rounds of the chip and the first rows past it, the last two rows, and
    seeded others.  Rows of fixed-grid solves are independent of each other."""
    want = {0, 1, tile - 1, tile, 4 * tile - 1, 4 * tile, chip * tile - 1, chip * tile, chip * tile + 1, B - 2, B - 1}
    rows = sorted(i for i in want if 0 <= i < B)
    g = torch.Generator().manual_seed(seed)
    for i in torch.randperm(B, generator=g).tolist():
        if len(rows) >= 32:
            break
        if i not in rows:
            rows.append(i)
    return torch.tensor(sorted(rows))


def draw(row, B, seed=None):
    """Seeded inputs of a batch: (z [B, 2D], x [B, D], p0 [B, D], k1 [B, 2D], raw conditional [B, C] or None)."""
    seed = SEED if seed is None else seed
    g = torch.Generator().manual_seed(1000 * seed + B % 1000 + 7 * row.D + row.C)
    n = lambda *s: torch.randn(*s, generator=g)
    return n(B, 2 * row.D), n(B, row.D), n(B, row.D), n(B, 2 * row.D), (n(B, row.C) if row.C else None)


# ---- the solves, written on a right-hand side forward(t, z, cond_n); they keep the dtype of z ----------------------------
def grid():
    return torch.linspace(1.0, 0.0, STEPS + 1)


def euler(forward, z, nodes, cond_n):
    """x + v(t_k, x) (t_{k+1} - t_k) over the fp32 nodes."""
    g = [float(v) for v in nodes]
    for k in range(len(g) - 1):
        z = z + forward(g[k], z, cond_n) * (g[k + 1] - g[k])
    return z


def leapfrog(forward, z, nodes, cond_n):
    """Kick-drift-kick, as tests/test_symplectic_leapfrog_host.leapfrog_f64 has it."""
    z = z.clone()
    D = z.shape[1] // 2
    g = [float(v) for v in nodes]
    for k in range(len(g) - 1):
        h = g[k + 1] - g[k]
        z[:, D:] += 0.5 * h * forward(g[k], z, cond_n)[:, D:]
        z[:, :D] += h * forward(0.5 * (g[k] + g[k + 1]), z, cond_n)[:, :D]
        z[:, D:] += 0.5 * h * forward(g[k + 1], z, cond_n)[:, D:]
    return z


def rk4_38(forward, z, nodes, cond_n):
    """Kutta's 3/8 rule: what torchdiffeq -- and so ``method="rk4"`` here -- calls rk4 (its rk4_alt_step_func)."""
    g = [float(v) for v in nodes]
    for k in range(len(g) - 1):
        t0, t1 = g[k], g[k + 1]
        h = t1 - t0
        k1 = forward(t0, z, cond_n)
        k2 = forward(t0 + h / 3, z + h * k1 / 3, cond_n)
        k3 = forward(t0 + 2 * h / 3, z + h * (k2 - k1 / 3), cond_n)
        k4 = forward(t1, z + h * (k1 - k2 + k3), cond_n)
        z = z + h * (k1 + 3 * (k2 + k3) + k4) / 8
    return z


def rk4_classic(forward, z, nodes, cond_n):
    """The classical fourth-order Runge-Kutta method (weights 1/6, 1/3, 1/3, 1/6): ``method="rk4_classic"`` here."""
    g = [float(v) for v in nodes]
    for k in range(len(g) - 1):
        t0, t1 = g[k], g[k + 1]
        h = t1 - t0
        k1 = forward(t0, z, cond_n)
        k2 = forward(t0 + h / 2, z + h * k1 / 2, cond_n)
        k3 = forward(t0 + h / 2, z + h * k2 / 2, cond_n)
        k4 = forward(t1, z + h * k3, cond_n)
        z = z + h * (k1 + 2 * (k2 + k3) + k4) / 6
    return z


def rk4_nodes():
    n = int(round(1.0 / RK4_STEP))
    return [i * RK4_STEP for i in range(n)] + [1.0]


def log_density(z1, p0, scale):
    """log N(z1) - log N(p0) - sum log scale, in float64."""
    logn = lambda z: (-0.5 * z.double() ** 2 - 0.5 * math.log(2 * math.pi)).sum(-1)
    return logn(z1) - logn(p0) - torch.log(scale.double()).sum()


def fp32_forward(fm):
    """The product's torch module as a right-hand side ``forward(t, z, cond_n)`` in fp32: the arithmetic floor of the bars."""
    def forward(t, z, cond_n):
        with torch.no_grad():
            return fm.model(torch.tensor(t, dtype=torch.float32), z, cond_n)
    return forward


def rel_to_max(got, want):
    """max |got - want| / max |want|: the whole state against the reference's largest entry."""
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
