// ff_trace_prod.hip -- Hutch++ / XTrace divergence estimates from J^T v PRODUCTS, the two streaming launches between and
// after the two sweeps of ff_mlp_ode_launch_vjp (gfx950).
//
// The route (host_stepper.RowStepper.run_table_products): sweep 1 writes Y = A P for the solve's probes at every evaluation
// row; ff_trace_basis factorises every Y and writes the second sweep's seeds; sweep 2 writes Z = A seeds; ff_trace_combine
// forms the estimates out[e][b].  The arithmetic is ff_trace_prod.h's, which is ff_trace_est.h's with the products read
// instead of summed.
//
// Roofline: HBM.  An item reads and writes (2 r + m) D floats (Hutch++) or 2 m D (XTrace) per launch -- not D D as the
// recorded-Jacobian kernel of ff_trace.hip -- so both launches are plain one-thread-per-item kernels on global memory with
// the factorisation's scratch laid out item-fastest (consecutive lanes on consecutive words).  Their loads are dependent and
// uncoalesced in the vectors themselves; what they move is 1 / D of what the sweeps compute for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_trace_prod.h"

namespace ff {

__global__ __launch_bounds__(256) void trace_basis_kernel(const ff_trace_prod_args a, long long items)
{
    if (a.gate && *(const volatile int32_t*)a.gate == 0) return;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= items) return;
    trace::basis(a.kind, trace::prod_item(a, t, a.workspace + t, (size_t)items));
}

__global__ __launch_bounds__(256) void trace_combine_kernel(const ff_trace_prod_args a, long long items)
{
    if (a.gate && *(const volatile int32_t*)a.gate == 0) return;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= items) return;
    a.out[t] = trace::combine(a.kind, trace::prod_item(a, t, a.workspace + t, (size_t)items));
}

} // namespace ff

// what both launches need; `second`: the combine launch
static int prod_args_ok(const ff_trace_prod_args* a, bool second)
{
    if (!a || !a->probes0 || !a->basis || !a->workspace) return FF_ERR_BADARG;
    if (a->kind != FF_TRACE_HUTCHPP && a->kind != FF_TRACE_XTRACE) return FF_ERR_BADARG;
    if (a->dim < 1 || a->n_rows < 0 || a->batch < 0 || a->r < 1 || a->r > a->dim) return FF_ERR_BADARG;
    if (a->kind == FF_TRACE_HUTCHPP && (a->m < 1 || !a->probes1)) return FF_ERR_BADARG;
    if (a->kind == FF_TRACE_XTRACE && !a->rfac) return FF_ERR_BADARG;
    if (second ? (!a->prod || !a->out) : !a->y) return FF_ERR_BADARG;
    return FF_OK;
}

extern "C" size_t ff_trace_prod_workspace_floats(int32_t kind, int32_t dim, int32_t r, int64_t items)
{
    if (dim < 1 || r < 1 || items < 0) return 0;
    return ff::trace::prod_workspace_per_item(kind, dim, r) * (size_t)items;
}

static int prod_launch(const ff_trace_prod_args* a, bool second, void* hip_stream)
{
    const int rc = prod_args_ok(a, second);
    if (rc != FF_OK) return rc;
    const long long items = (long long)a->n_rows * a->batch;
    if (items == 0) return FF_OK;
    const long long grid = (items + 255) / 256;
    if (grid > 0x7fffffffll) return FF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)hip_stream;
    if (second) hipLaunchKernelGGL(ff::trace_combine_kernel, dim3((unsigned)grid), dim3(256), 0, s, *a, items);
    else hipLaunchKernelGGL(ff::trace_basis_kernel, dim3((unsigned)grid), dim3(256), 0, s, *a, items);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_trace_basis(const ff_trace_prod_args* a, void* hip_stream) { return prod_launch(a, false, hip_stream); }
extern "C" int ff_trace_combine(const ff_trace_prod_args* a, void* hip_stream) { return prod_launch(a, true, hip_stream); }

// the same arithmetic on the host, HOST pointers (tests without a GPU); `workspace` needs one item's floats only
static int prod_host(const ff_trace_prod_args* a, bool second)
{
    const int rc = prod_args_ok(a, second);
    if (rc != FF_OK) return rc;
    const long long items = (long long)a->n_rows * a->batch;
    for (long long t = 0; t < items; ++t) {
        const ff::trace::ProdItem p = ff::trace::prod_item(*a, t, a->workspace, 1);
        if (second) a->out[t] = ff::trace::combine(a->kind, p);
        else ff::trace::basis(a->kind, p);
    }
    return FF_OK;
}

extern "C" int ff_trace_basis_host(const ff_trace_prod_args* a) { return prod_host(a, false); }
extern "C" int ff_trace_combine_host(const ff_trace_prod_args* a) { return prod_host(a, true); }
