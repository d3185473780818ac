// ff_pull_registry.h -- table of the compiled pull-back units (mlp_pull_kernel, ff_mlp_pull.hpp; filled by generated code).
// A header of its own beside ff_registry.h: only the pull launchers, the generated table and ff_api.cpp include it, so the
// translation units of every other kernel are untouched by it.
#pragma once
#include "ff_registry.h"

namespace ff {

// pull-back family (ff_mlp_pull_plan): SiLU, fp32, ONE wavefront per workgroup and per tile, no twin; a pull plan's kernel_id
// is FF_PULL_KERNEL_BASE + the index into this table
struct PullKernelEntry {
    int tile;       // MFMA columns per wavefront
    int H;          // hidden width on chip
    int dregs;      // state registers
    int cregs;      // conditional registers
    int wps;        // (kept for the shape of the fp32 tables; the stash in LDS bounds the occupancy, not this)
    LaunchFn launch;        // NULL: the library carries no pull kernels (test variants)
    const char* name;
};
extern const PullKernelEntry g_pull_kernels[];
extern const int g_n_pull_kernels;

} // namespace ff
