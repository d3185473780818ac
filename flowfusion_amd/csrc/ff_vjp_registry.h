// ff_vjp_registry.h -- table of the compiled products units (mlp_vjp_kernel, ff_mlp_vjp.hpp; filled by generated code).
// A header of its own beside ff_pull_registry.h: only the products launchers, the generated table and ff_api.cpp include it,
// so the translation units of every other kernel are untouched by it.
#pragma once
#include "ff_pull_registry.h"

namespace ff {

// products family (ff_mlp_ode_launch_vjp): entry i is the sibling of g_pull_kernels[i] -- same shape, same two weight packs, a
// pull plan launches it -- and its kernel id is FF_VJP_KERNEL_BASE + i (a name space of its own: no plan carries it)
extern const PullKernelEntry g_vjp_kernels[];
extern const int g_n_vjp_kernels;

} // namespace ff
