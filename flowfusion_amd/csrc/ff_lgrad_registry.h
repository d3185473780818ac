// ff_lgrad_registry.h -- table of the compiled log-density gradient units (mlp_lgrad_kernel, ff_mlp_lgrad.hpp; filled by generated
// code).  A header of its own beside ff_dadj_registry.h: only their launchers, the generated table and ff_api.cpp include it, so
// the translation units of every other kernel are untouched by it.
#pragma once
#include "ff_pull_registry.h"

namespace ff {

// entry i is the sibling of g_pull_kernels[i] -- same shape, same two weight packs, a pull plan launches it
// (ff_mlp_ode_launch_logp_grad) -- and its kernel id is FF_LGRAD_KERNEL_BASE + i (a name space of its own: no plan carries it)
extern const PullKernelEntry g_lgrad_kernels[];
extern const int g_n_lgrad_kernels;

} // namespace ff
