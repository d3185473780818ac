// ff_pushsel_registry.h -- table of the compiled row-select push-forward units (mlp_pushsel_kernel, ff_mlp_pushsel.hpp; filled
// by generated code).  A header of its own beside ff_registry.h: only the select push launchers, the generated table and
// ff_api.cpp include it, so the translation units of every other kernel are untouched by it.
#pragma once
#include "ff_registry.h"

namespace ff {

// one sibling per push-forward unit, same shape; a push-select plan's kernel_id is FF_PUSH_SELECT_KERNEL_BASE + the index into
// this table (ff_mlp_push_select_plan)
extern const PushKernelEntry g_pushsel_kernels[];
extern const int g_n_pushsel_kernels;

} // namespace ff
