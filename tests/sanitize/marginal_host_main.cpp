// Stand-alone host check of ff_marginal_expand_host / ff_marginal_reduce_host under AddressSanitizer and
// UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -Iflowfusion_amd/csrc flowfusion_amd/csrc/ff_marginal.hip tests/sanitize/marginal_host_main.cpp \
//         -fsanitize=address,undefined -o marginal_host_asan && ./marginal_host_asan
//
// Every buffer is a heap allocation of exactly the documented size, so a read or write one element outside it is
// reported; the shapes are those of tests/test_symplectic_marginal_host.py (K at and around the lane-group sizes, D that
// are no multiple of four, a global row above 2^32, with and without shift / scale / cond / ess).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "flowfusion_amd.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int Ks[] = {1, 2, 5, 64, 65, 257}, Ds[] = {1, 3, 16, 17, 32};
    const int64_t offsets[] = {0, ((int64_t)1 << 33) + 7};
    for (int K : Ks)
        for (int D : Ds)
            for (int64_t off : offsets)
                for (int with = 0; with < 2; ++with) {
                    const int64_t B = 3;
                    const int C = 3;
                    std::vector<float> x(B * D), shift(D), scale(D), cond(B * C), z0(B * K * 2 * D), co(B * K * C), lp(B), ess(B);
                    for (size_t i = 0; i < x.size(); ++i) x[i] = 0.37f * (float)(i % 11) - 1.5f;
                    for (int d = 0; d < D; ++d) { shift[d] = 0.1f * d; scale[d] = 0.5f + 0.03f * d; }
                    for (size_t i = 0; i < cond.size(); ++i) cond[i] = (float)i;
                    CHECK(ff_marginal_expand_host(x.data(), with ? shift.data() : nullptr, with ? scale.data() : nullptr,
                                                  with ? cond.data() : nullptr, B, D, C, K, 7, off, z0.data(),
                                                  with ? co.data() : nullptr) == FF_OK);
                    CHECK(ff_marginal_reduce_host(z0.data(), B, D, K, 7, off, 0.25, lp.data(), with ? ess.data() : nullptr) == FF_OK);
                    // z1 = z0: the momenta cancel, every weight is N(q0), so log p = log N(q0) - log_det and ess = K
                    for (int64_t r = 0; r < B; ++r) {
                        double s = 0.0;
                        for (int d = 0; d < D; ++d) s += (double)z0[r * K * 2 * D + d] * (double)z0[r * K * 2 * D + d];
                        const double want = -0.5 * s - 0.5 * D * log(2.0 * M_PI) - 0.25;
                        CHECK(fabs((double)lp[r] - want) <= 1e-5 * fmax(1.0, fabs(want)));
                        if (with) CHECK(fabs((double)ess[r] - K) <= 1e-4 * K);
                    }
                }
    // the closed-form shapes: B = 256, D = 3, K = 64; non-finite rows
    {
        const int64_t B = 256;
        const int D = 3, K = 64;
        std::vector<float> x(B * D, 0.5f), z(B * K * 2 * D), lp(B), ess(B);
        CHECK(ff_marginal_expand_host(x.data(), nullptr, nullptr, nullptr, B, D, 0, K, 7, 0, z.data(), nullptr) == FF_OK);
        z[5] = INFINITY;
        z[(size_t)K * 2 * D + 1] = NAN;
        for (int k = 0; k < K; ++k) z[(size_t)(2 * K + k) * 2 * D] = -INFINITY;
        CHECK(ff_marginal_reduce_host(z.data(), B, D, K, 7, 0, 0.0, lp.data(), ess.data()) == FF_OK);
        CHECK(isfinite(lp[0]) && isnan(lp[1]) && lp[2] == -INFINITY && isnan(ess[2]) && isfinite(lp[3]));
    }
    CHECK(ff_marginal_expand_host(nullptr, nullptr, nullptr, nullptr, 1, 1, 0, 1, 0, 0, nullptr, nullptr) == FF_ERR_BADARG);
    CHECK(ff_marginal_reduce_host(nullptr, 1, 1, 1, 0, 0, 0.0, nullptr, nullptr) == FF_ERR_BADARG);
    printf(failures ? "marginal host check: %d failures\n" : "marginal host check: ok\n", failures);
    return failures ? 1 : 0;
}
