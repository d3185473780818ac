// Stand-alone host check of ff_trace_basis_host / ff_trace_combine_host under AddressSanitizer and
// UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -Iflowfusion_amd/csrc flowfusion_amd/csrc/ff_trace_prod.hip tests/sanitize/trace_prod_host_main.cpp \
//         -fsanitize=address,undefined -o trace_prod_host_asan && ./trace_prod_host_asan
//
// Every buffer is a heap allocation of exactly the documented size, so a read or write one element outside it is reported.
// Shapes (D, r, m): the corners of tests/test_estimator_products_host.py -- one dimension, r = D, more residual probes than
// dimensions, fifteen sketch columns, 32 dimensions -- both kinds, two rows, three samples.  The matrices are diagonal, so
// the products are formed here without a matrix, and Hutch++ with r = D must return the trace.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "flowfusion_amd.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int shapes[][3] = {{1, 1, 2}, {5, 2, 3}, {5, 5, 1}, {16, 1, 1}, {16, 4, 4}, {32, 3, 2}, {16, 15, 1}, {3, 2, 7}};
    const int n = 2, B = 3;
    uint32_t rng = 12345u;
    auto coin = [&]() { rng = rng * 1664525u + 1013904223u; return (rng >> 16) & 1u ? 1.f : -1.f; };
    for (const auto& sh : shapes) {
        const int D = sh[0], r = sh[1], m = sh[2];
        for (int kind = FF_TRACE_HUTCHPP; kind <= FF_TRACE_XTRACE; ++kind) {
            const int K2 = kind == FF_TRACE_HUTCHPP ? r + m : r;
            const size_t items = (size_t)n * B;
            std::vector<float> diag(items * D), S((size_t)r * B * D), G((size_t)m * B * D), y(items * r * D), basis(items * K2 * D),
                rfac(items * r * r), prod(items * K2 * D), out(items), ws(ff_trace_prod_workspace_floats(kind, D, r, 1));
            for (size_t i = 0; i < diag.size(); ++i) diag[i] = 0.5f + 0.25f * (float)(i % 7);
            // probes: sample b's sketch probes are made independent by construction (a sign pattern per column and dimension)
            for (int c = 0; c < r; ++c)
                for (int b = 0; b < B; ++b)
                    for (int d = 0; d < D; ++d) S[((size_t)c * B + b) * D + d] = (d == c) ? -1.f : 1.f;
            for (auto& v : G) v = coin();
            for (size_t t = 0; t < items; ++t)
                for (int c = 0; c < r; ++c)
                    for (int d = 0; d < D; ++d) y[(t * r + c) * D + d] = diag[t * D + d] * S[((size_t)c * B + t % B) * D + d];
            ff_trace_prod_args a = {};
            a.kind = kind; a.dim = D; a.n_rows = n; a.r = r; a.m = m; a.batch = B;
            a.probes0 = S.data(); a.probes1 = kind == FF_TRACE_HUTCHPP ? G.data() : nullptr;
            a.y = y.data(); a.basis = basis.data(); a.rfac = kind == FF_TRACE_XTRACE ? rfac.data() : nullptr;
            a.prod = prod.data(); a.out = out.data(); a.workspace = ws.data();
            CHECK(ff_trace_basis_host(&a) == FF_OK);
            for (size_t t = 0; t < items; ++t)
                for (int c = 0; c < K2; ++c)
                    for (int d = 0; d < D; ++d) prod[(t * K2 + c) * D + d] = diag[t * D + d] * basis[(t * K2 + c) * D + d];
            CHECK(ff_trace_combine_host(&a) == FF_OK);
            for (size_t t = 0; t < items; ++t) {
                CHECK(out[t] == out[t] || D < 3);              // finite where the sketch has full rank (D >= 3: the columns differ)
                if (kind == FF_TRACE_HUTCHPP && r == D) {
                    float tr = 0.f;
                    for (int d = 0; d < D; ++d) tr += diag[t * D + d];
                    CHECK(fabsf(out[t] - tr) <= 1e-4f * fabsf(tr));
                }
            }
            a.r = D + 1;
            CHECK(ff_trace_basis_host(&a) == FF_ERR_BADARG && ff_trace_combine_host(&a) == FF_ERR_BADARG);
        }
    }
    printf(failures ? "trace_prod host twins: %d FAILED\n" : "trace_prod host twins: clean (%d failures)\n", failures);
    return failures ? 1 : 0;
}
