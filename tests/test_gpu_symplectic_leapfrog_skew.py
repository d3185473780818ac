"""GPU tier: the row-select cooperative twin (csrc/ff_mlp_pair.hpp, SELECT + COOP) with a wavefront held back.

The select twin shares the pair twin's barrier sequence -- the zero-fill barrier and the exchange-buffer index that
alternates over the whole launch -- and parks nothing (a row runs one network), so it has no hazard of its own and there
is no un-fixed variant to see fail.  This file asks that the `skew` build of the 128-wide select twin (csrc/ff_skew.h;
flowfusion_amd/build.py VARIANTS: wavefront 0 of every workgroup held back at the shared places) is bitwise the
product's one-wavefront kernel on a 9-row leapfrog table, with an even and an odd number of layers per row (the
exchange buffer a row starts on alternates, or does not)."""
import ctypes

import pytest
import torch

from flowfusion_amd import _native
from flowfusion_amd.fused import MODE_STATE
from tests.test_gpu_symplectic_leapfrog import select_launch
from tests.test_gpu_symplectic_twin import DEV, seeded_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def skew_lib(built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"
    from flowfusion_amd import build
    if not build.variant_lib("skew").exists():
        build.build()                                     # (normally built by __graft_entry__.build() with the product)
    return _native.load_library(build.variant_lib("skew"))


def _plan(L, net):
    """The select plan `L` makes for `net` -- kernel ids are per library, the packed layout must be the product's."""
    ref = net.plan(MODE_STATE, select=True)
    hidden = [int(l.out_features) for l in net.linears[:-1]]
    p = _native.PlanStruct()
    rc = L.ff_mlp_pair_select_plan(net.dim, net.cond_dim, len(hidden), (ctypes.c_int * len(hidden))(*hidden), ctypes.byref(p))
    assert rc == 0, rc
    for f in ("dim", "cond_dim", "n_hidden", "width", "dregs", "cregs", "tile", "precision"):
        assert getattr(p, f) == getattr(ref, f), f
    assert L.ff_plan_kernel_name(ctypes.byref(p)) == b"mlp_pairsel_m16_h128_d8_c4_w3"
    return p


@pytest.mark.parametrize("units", [[128, 128], [128, 100, 128]], ids=["even", "odd"])
def test_select_twin_under_skew(skew_lib, units):
    D, C = 5, 3
    fm = seeded_model(D, C, units, 61)
    net = fm._net()
    wpack = net.wpack(DEV, MODE_STATE)
    torch.manual_seed(62)
    B = 200                                              # 13 tiles: the twin's regime
    x, cond = torch.randn(B, 2 * D, device=DEV), torch.randn(B, C, device=DEV)
    tab = fm._leapfrog_table(torch.linspace(1.0, 0.0, 5)).to(DEV)
    assert tab.shape[0] == 9
    plan = net.plan(MODE_STATE, select=True)
    rc, ref = select_launch(plan, wpack, x, tab, cond, FF_COOP=0)                    # the product's one-wavefront kernel
    assert rc == 0 and torch.isfinite(ref).all() and (ref - x).abs().max() > 1e-3
    rc, twin = select_launch(plan, wpack, x, tab, cond, FF_COOP=1)
    assert rc == 0 and torch.equal(twin, ref)
    sp = _plan(skew_lib, net)
    for _ in range(3):
        rc, got = select_launch(sp, wpack, x, tab, cond, lib=skew_lib, FF_COOP=1)
        assert rc == 0 and torch.equal(got, ref)
