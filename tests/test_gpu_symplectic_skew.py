"""GPU tier: a DETERMINISTIC guard for the LDS sharing of the two-network cooperative twin (csrc/ff_mlp_pair.hpp, COOP).

The twin's four wavefronts share one copy of the stage slots and two activation-exchange buffers.  Three places need care
(the header of ff_mlp_pair.hpp): the zero fill of the slots against the caller's first stage, the exchange-buffer index
over the whole launch, and net A's output while net B runs -- the one-wavefront kernel parks it in the row's stage slot,
which in a twin a fast wavefront overwrites with the finished right-hand side before a slow one has read it back.

As in tests/test_gpu_skew.py the skew is built in (csrc/ff_skew.h; flowfusion_amd/build.py VARIANTS, test-only libraries):
wavefront 0 of every workgroup is held back with s_sleep at those three places.  Single process, one run per case:
  * `skew`        the twin as the product has it: bitwise the product's one-wavefront kernel;
  * `skew_unfix`  the twin that parks net A in the shared slot: WRONG numbers (else this file guards nothing).
Only the 128-wide instance is built into the variants."""
import ctypes

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.fused import MODE_STATE
from tests.test_gpu_symplectic_twin import DEV, attempt_table, raw_launch, seeded_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"
    from flowfusion_amd import build
    if not all(build.variant_lib(v).exists() for v in ("skew", "skew_unfix")):
        build.build()                                     # (normally built by __graft_entry__.build() with the product)
    return {"product": built_library, "skew": _native.load_library(build.variant_lib("skew")),
            "unfix": _native.load_library(build.variant_lib("skew_unfix"))}


def _plan(L, net):
    """The pair plan `L` makes for `net` -- kernel ids are per library, the packed layout must be the product's."""
    ref = net.plan(MODE_STATE)
    hidden = [int(l.out_features) for l in net.linears[:-1]]
    p = _native.PlanStruct()
    rc = L.ff_mlp_pair_plan(net.dim, net.cond_dim, len(hidden), (ctypes.c_int * len(hidden))(*hidden), ctypes.byref(p))
    assert rc == 0, rc
    for f in ("dim", "cond_dim", "n_hidden", "width", "dregs", "cregs", "tile", "precision"):
        assert getattr(p, f) == getattr(ref, f), f
    assert L.ff_plan_kernel_name(ctypes.byref(p)) == b"mlp_pair_m16_h128_d8_c4_w3"
    return p


@pytest.mark.parametrize("units", [[128, 128], [128, 100, 128]], ids=["even", "odd"])
def test_pair_twin_under_skew(libs, units):
    D, C = 5, 3
    fm = seeded_model(D, C, units, 41)
    net = fm._net()
    wpack = net.wpack(DEV, MODE_STATE)
    torch.manual_seed(42)
    B = 200                                              # 13 tiles: the twin's regime
    x, k1 = torch.randn(B, 2 * D, device=DEV), torch.randn(B, 2 * D, device=DEV)
    cond = torch.randn(B, C, device=DEV)
    tab = attempt_table(fm, 5)
    kw = dict(cond=cond, k1=k1, n_aux=1)
    ref = raw_launch(libs["product"], net.plan(MODE_STATE), wpack, x, tab, 5, FF_COOP=0, **kw)      # one-wavefront kernel
    assert torch.isfinite(ref[0]).all() and (ref[1] - x).abs().max() > 1e-3                        # the attempt did something
    twin = raw_launch(libs["product"], net.plan(MODE_STATE), wpack, x, tab, 5, FF_COOP=1, **kw)
    assert torch.equal(twin[0], ref[0]) and torch.equal(twin[1], ref[1])
    # without k1_in the late zero fill has nothing to wipe: a plain fixed-grid table (several evaluations, so that the
    # exchange buffers of consecutive evaluations meet) beside the attempt table
    grid = fm._ode_table(torch.tensor([0.0, 1.0]), "rk4", {"step_size": 0.25}, MODE_STATE).to(DEV)
    ref_g = raw_launch(libs["product"], net.plan(MODE_STATE), wpack, x, grid, grid.shape[0], cond=cond, FF_COOP=0)
    for _ in range(3):
        got = raw_launch(libs["skew"], _plan(libs["skew"], net), wpack, x, tab, 5, FF_COOP=1, **kw)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        got = raw_launch(libs["skew"], _plan(libs["skew"], net), wpack, x, grid, grid.shape[0], cond=cond, FF_COOP=1)
        assert torch.equal(got[0], ref_g[0])
    # the un-fixed twin's one-wavefront kernel is the product's (the skew touches only the twin) ...
    same = raw_launch(libs["unfix"], _plan(libs["unfix"], net), wpack, x, tab, 5, FF_COOP=0, **kw)
    assert torch.equal(same[0], ref[0]) and torch.equal(same[1], ref[1])
    # ... and its twin, parking net A's output in the shared slot, reads the finished right-hand side back instead
    bad = raw_launch(libs["unfix"], _plan(libs["unfix"], net), wpack, x, tab, 5, FF_COOP=1, **kw)
    assert not torch.equal(bad[1], ref[1]), "the skewed twin that parks net A in the shared stage slot must lose it"
    bad = raw_launch(libs["unfix"], _plan(libs["unfix"], net), wpack, x, grid, grid.shape[0], cond=cond, FF_COOP=1)
    assert not torch.equal(bad[0], ref_g[0])
