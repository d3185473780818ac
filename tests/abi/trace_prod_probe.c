/* trace_prod_probe.c -- compiled as C11 by tests/test_estimator_products_host.py against include/flowfusion_amd.h and linked
 * with libflowfusion_amd.so: prints the layout of ff_trace_prod_args for the comparison with the ctypes mirror
 * (flowfusion_amd/_native.py TraceProdArgs) and runs the two host twins of the products route from C, without a GPU. */
#include <stddef.h>
#include <stdio.h>
#include "flowfusion_amd.h"

#define OFF(f) printf("offsetof " #f " %zu\n", offsetof(ff_trace_prod_args, f))

int main(void)
{
    printf("sizeof %zu\n", sizeof(ff_trace_prod_args));
    OFF(kind); OFF(dim); OFF(n_rows); OFF(r); OFF(m); OFF(reserved); OFF(batch); OFF(probes0); OFF(probes1); OFF(y); OFF(basis);
    OFF(rfac); OFF(prod); OFF(out); OFF(workspace); OFF(gate);

    /* Hutch++ with a full-rank sketch IS the trace: A = [[1, 2], [3, 4]], S = (e1 + e2, e1 - e2); the products by hand */
    const float A[4] = {1.f, 2.f, 3.f, 4.f}, S[4] = {1.f, 1.f, 1.f, -1.f}, G[2] = {1.f, -1.f};
    float y[4], basis[6], prod[6], ws[16], out = 0.f;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 2; ++i) y[c * 2 + i] = A[i * 2] * S[c * 2] + A[i * 2 + 1] * S[c * 2 + 1];
    ff_trace_prod_args t = {0};
    t.kind = FF_TRACE_HUTCHPP; t.dim = 2; t.n_rows = 1; t.r = 2; t.m = 1; t.batch = 1;
    t.probes0 = S; t.probes1 = G; t.y = y; t.basis = basis; t.prod = prod; t.out = &out; t.workspace = ws;
    if (ff_trace_prod_workspace_floats(FF_TRACE_HUTCHPP, 2, 2, 1) > 16) return 1;
    printf("basis %d\n", ff_trace_basis_host(&t));
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 2; ++i) prod[c * 2 + i] = A[i * 2] * basis[c * 2] + A[i * 2 + 1] * basis[c * 2 + 1];
    int rc = ff_trace_combine_host(&t);
    printf("combine %d %.5f\n", rc, (double)out);
    t.basis = NULL;
    printf("nullbasis %d\n", ff_trace_basis_host(&t));
    printf("nullcombine %d\n", ff_trace_combine_host(&t));
    ff_ode_args a = {0};
    ff_mlp_plan_t plan = {0};
    printf("nullvjp %d\n", ff_mlp_ode_launch_vjp(&plan, &a, NULL, 0, NULL, NULL));
    return 0;
}
