// ff_registry.h -- table of compiled kernel instantiations (filled by generated code).
#pragma once
#include <hip/hip_runtime_api.h>
#include "ff_kernel_args.h"

namespace ff {

constexpr int kMaxDevices = 64;   // launchers keep one "attribute set" flag per device of the process

typedef int (*LaunchFn)(const KernelArgs* args, unsigned grid, unsigned lds_bytes, hipStream_t stream);

struct KernelEntry {
    int tile;       // MFMA columns per wavefront: 32 (32x32x2) or 16 (16x16x4)
    int H;          // hidden width on chip
    int dregs;      // state registers  (covers dim <= dregs * 64/tile)
    int cregs;      // conditional registers
    int tangents;   // 1: divergence-capable instantiation
    int act;        // FF_ACT_* code of the hidden activation this instantiation has compiled in (0 = SiLU; 9 = any
                    // non-SiLU activation, chosen at run time)
    LaunchFn launch;
    const char* name;
    LaunchFn launch_coop;   // cooperative twin for small batches (one tile per workgroup, ff_mlp_ode.hpp COOP) or NULL
    int wps;        // wavefronts per SIMD the one-wavefront kernel is built for (its launch bound): 1024 * wps tiles run at once
};

// defined in the generated ff_table.cpp
extern const KernelEntry g_kernels[];
extern const int g_n_kernels;

// split-precision family (FF_PREC_BF16X3 / FF_PREC_BF16X2, ff_mlp_ode_split.hpp): width <= 256, dim <= 16, cond <= 16
struct SplitKernelEntry {
    int n_hidden;   // hidden layers (compile-time in this family)
    int tangents;   // 0: state only; 1: Hutchinson (value / tangent column pairs); 2: exact trace (a value column + unit tangents)
    int parts;      // bf16 parts per fp32 operand: 3 (truncation, six products) or 2 (round to nearest, three products)
    int dt;         // 16-dimension tiles of the state: 1 (dim <= 16, 7 stage slots) or 2 (dim <= 32, 4 stage slots)
    int width;      // on-chip layer width: 256 or 128
    LaunchFn launch;
    const char* name;
};
extern const SplitKernelEntry g_split_kernels[];
extern const int g_n_split_kernels;

// the launchers of one kernel shape: the one-wavefront kernel and its cooperative twin for small batches (one tile per
// workgroup), and the name the kernel goes by
struct Launchers {
    LaunchFn one_wave;      // NULL: the library carries no kernel of this kind
    LaunchFn coop;          // NULL: no twin
    const char* name;
};

// two-network family (ff_mlp_pair.hpp, ff_mlp_pair_plan): state-only, SiLU; a pair plan's kernel_id is
// FF_PAIR_KERNEL_BASE + the index into this table
struct PairKernelEntry {
    int tile;       // MFMA columns per wavefront
    int H;          // hidden width on chip (each network)
    int dregs;      // state registers
    int cregs;      // conditional registers
    int wps;        // wavefronts per SIMD (launch bound)
    Launchers pair;
    // row-select variant of the same shape (ff_mlp_pair_select_plan: kernel_id FF_PAIR_SELECT_KERNEL_BASE + the index): a row
    // runs one of the two networks.  Not entries of a table of their own; one_wave NULL where a library carries none.
    Launchers select;
};
extern const PairKernelEntry g_pair_kernels[];
extern const int g_n_pair_kernels;

// push-forward family (mlp_ode_kernel PUSH, ff_mlp_push_plan): SiLU, fp32, one wavefront per tile, no twin; a push plan's
// kernel_id is FF_PUSH_KERNEL_BASE + the index into this table
struct PushKernelEntry {
    int tile;       // MFMA columns per wavefront
    int H;          // hidden width on chip
    int dregs;      // state registers
    int cregs;      // conditional registers
    int wps;        // wavefronts per SIMD (launch bound)
    LaunchFn launch;        // NULL: the library carries no push kernels (test variants)
    const char* name;
};
extern const PushKernelEntry g_push_kernels[];
extern const int g_n_push_kernels;

} // namespace ff
