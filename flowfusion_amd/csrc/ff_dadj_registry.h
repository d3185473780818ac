// ff_dadj_registry.h -- tables of the compiled record and discrete-adjoint units (mlp_rec_kernel, mlp_dadj_kernel, ff_mlp_dadj.hpp;
// filled by generated code).  A header of its own beside ff_vjp_registry.h: only their launchers, the generated table and
// ff_api.cpp include it, so the translation units of every other kernel are untouched by it.
#pragma once
#include "ff_pull_registry.h"

namespace ff {

// entry i of either table is the sibling of g_pull_kernels[i] -- same shape, same two weight packs, a pull plan launches it
// (ff_mlp_ode_launch_record, ff_mlp_ode_launch_pull_discrete) -- and its kernel id is FF_REC_KERNEL_BASE + i or
// FF_DADJ_KERNEL_BASE + i (name spaces of their own: no plan carries them)
extern const PullKernelEntry g_rec_kernels[];
extern const int g_n_rec_kernels;
extern const PullKernelEntry g_dadj_kernels[];
extern const int g_n_dadj_kernels;

} // namespace ff
