// Stand-alone host check of ff_observe_expand_host / ff_logmeanexp_host under AddressSanitizer and
// UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -Iflowfusion_amd/csrc flowfusion_amd/csrc/ff_observe.hip tests/sanitize/observe_host_main.cpp \
//         -fsanitize=address,undefined -o observe_host_asan && ./observe_host_asan
//
// Every buffer is a heap allocation of exactly the documented size, so a read or write one element outside it is
// reported; the shapes are those of tests/test_observe_host.py (K at and around the lane-group sizes and at the maximum, D
// that are no multiple of four, a global row above 2^32, both noise_std layouts, with and without cond / ess).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "flowfusion_amd.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int Ks[] = {1, 3, 8, 17, 65, 4096}, Ds[] = {1, 3, 4, 16, 33};
    const int64_t offsets[] = {0, ((int64_t)1 << 33) + 7};
    for (int K : Ks)
        for (int D : Ds)
            for (int64_t off : offsets)
                for (int with = 0; with < 2; ++with) {
                    const int64_t B = 3;
                    const int C = 3;
                    // with: a row of noise_std per point, cond and ess; without: one [D] vector of zeros
                    std::vector<float> x(B * D), std_(with ? B * D : D), cond(B * C), y(B * K * D), co(B * K * C), out(B), ess(B);
                    for (size_t i = 0; i < x.size(); ++i) x[i] = 0.37f * (float)(i % 11) - 1.5f;
                    for (size_t i = 0; i < std_.size(); ++i) std_[i] = with ? 0.05f * (float)(1 + i % 7) : 0.0f;
                    for (size_t i = 0; i < cond.size(); ++i) cond[i] = (float)i;
                    CHECK(ff_observe_expand_host(x.data(), std_.data(), with ? D : 0, with ? cond.data() : nullptr, B, D, C, K, 7,
                                                 off, y.data(), with ? co.data() : nullptr) == FF_OK);
                    for (int64_t r = 0; r < B; ++r)
                        for (int k = 0; k < K; ++k)
                            for (int d = 0; d < D; ++d) {
                                const float v = y[(r * K + k) * D + d];
                                if (with) CHECK(fabsf(v - x[r * D + d]) <= 8.0f * std_[r * D + d]);      // |z| < 6 in this stream
                                else CHECK(v == x[r * D + d]);
                            }
                    if (with)
                        for (int64_t i = 0; i < B * K * C; ++i) CHECK(co[i] == cond[(i / C / K) * C + i % C]);
                    // the mean of K equal values is that value, every weight 1
                    std::vector<float> lp(B * K);
                    for (int64_t r = 0; r < B; ++r)
                        for (int k = 0; k < K; ++k) lp[r * K + k] = -3.5f * (float)(r + 1);
                    CHECK(ff_logmeanexp_host(lp.data(), B, K, out.data(), with ? ess.data() : nullptr) == FF_OK);
                    for (int64_t r = 0; r < B; ++r) {
                        CHECK(fabs((double)out[r] + 3.5 * (double)(r + 1)) <= 1e-6 * 3.5 * (double)(r + 1));
                        if (with) CHECK(fabs((double)ess[r] - K) <= 1e-6 * K);
                    }
                }
    // non-finite rows
    {
        const int64_t B = 4;
        const int K = 64;
        std::vector<float> lp(B * K, -2.0f), out(B), ess(B);
        lp[5] = -INFINITY;
        lp[K + 1] = NAN;
        for (int k = 0; k < K; ++k) lp[2 * K + k] = -INFINITY;
        lp[3 * K + 7] = INFINITY;
        CHECK(ff_logmeanexp_host(lp.data(), B, K, out.data(), ess.data()) == FF_OK);
        CHECK(isfinite(out[0]) && isnan(out[1]) && out[2] == -INFINITY && isnan(ess[2]) && out[3] == INFINITY);
    }
    CHECK(ff_observe_expand_host(nullptr, nullptr, 0, nullptr, 1, 1, 0, 1, 0, 0, nullptr, nullptr) == FF_ERR_BADARG);
    CHECK(ff_logmeanexp_host(nullptr, 1, 1, nullptr, nullptr) == FF_ERR_BADARG);
    printf(failures ? "observe host check: %d failures\n" : "observe host check: ok\n", failures);
    return failures ? 1 : 0;
}
