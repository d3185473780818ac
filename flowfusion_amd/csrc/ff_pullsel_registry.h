// ff_pullsel_registry.h -- table of the compiled row-select pull-back units (mlp_pullsel_kernel, ff_mlp_pullsel.hpp; filled by
// generated code).  A header of its own beside ff_pull_registry.h: only the select pull launchers, the generated table and
// ff_api.cpp include it, so the translation units of every other kernel are untouched by it.
#pragma once
#include "ff_pull_registry.h"

namespace ff {

// one sibling per pull-back unit, same shape; a pull-select plan's kernel_id is FF_PULL_SELECT_KERNEL_BASE + the index into this
// table (ff_mlp_pull_select_plan)
extern const PullKernelEntry g_pullsel_kernels[];
extern const int g_n_pullsel_kernels;

} // namespace ff
