// Stand-alone host check of ff_weighted_resample_host under AddressSanitizer and UndefinedBehaviorSanitizer (host code
// only; nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -Iflowfusion_amd/csrc flowfusion_amd/csrc/ff_observe.hip tests/sanitize/observe_posterior_host_main.cpp \
//         -fsanitize=address,undefined -o observe_posterior_host_asan && ./observe_posterior_host_asan
//
// Every buffer is a heap allocation of exactly the documented size, so a read or write one element outside it is
// reported; the shapes are those of tests/test_observe_posterior_host.py (K at and around the lane-group sizes and at the
// maximum, D that are no multiple of four, M that are no multiple of the four uniforms of a block, M = 0 and the maximum,
// a global row above 2^32, every output left out in turn) and the non-finite rows.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "flowfusion_amd.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int Ks[] = {1, 3, 8, 17, 65, 4096}, Ds[] = {1, 3, 4, 17}, Ms[] = {0, 1, 5, 8, 4096};
    const int64_t offsets[] = {0, ((int64_t)1 << 32) + 3};
    for (int K : Ks)
        for (int D : Ds)
            for (int M : Ms)
                for (int64_t off : offsets) {
                    if (M == 4096 && (K > 17 || D != 3)) continue;                  // (the largest M once per small K)
                    const int64_t B = 3;
                    std::vector<float> y(B * K * D), lp(B * K), s(B * M * D), mean(B * D), var(B * D);
                    std::vector<int32_t> idx(B * M);
                    for (size_t i = 0; i < y.size(); ++i) y[i] = 0.37f * (float)(i % 11) - 1.5f;
                    for (size_t i = 0; i < lp.size(); ++i) lp[i] = i % 5 == 3 && K > 1 ? -INFINITY : -0.5f * (float)(i % 7);
                    CHECK(ff_weighted_resample_host(y.data(), lp.data(), B, D, K, M, 7, off, s.data(), idx.data(), mean.data(),
                                                    var.data()) == FF_OK);
                    for (int64_t r = 0; r < B; ++r) {
                        for (int m = 0; m < M; ++m) {
                            const int32_t k = idx[r * M + m];
                            CHECK(k >= 0 && k < K);
                            if (k < 0 || k >= K) continue;
                            CHECK(lp[r * K + k] > -INFINITY);                           // never a row of weight zero
                            for (int d = 0; d < D; ++d) CHECK(s[(r * M + m) * D + d] == y[(r * K + k) * D + d]);
                        }
                        for (int d = 0; d < D; ++d) {
                            CHECK(mean[r * D + d] >= -1.5f && mean[r * D + d] <= 0.37f * 10.f - 1.5f + 1e-6f);
                            CHECK(var[r * D + d] >= 0.f && var[r * D + d] <= 3.7f * 3.7f);
                            if (K == 1) CHECK(mean[r * D + d] == y[r * D + d] && var[r * D + d] == 0.f);
                        }
                    }
                    // every output left out in turn: the others keep their bits
                    for (int skip = 0; skip < 4; ++skip) {
                        std::vector<float> s2(B * M * D), mean2(B * D), var2(B * D);
                        std::vector<int32_t> idx2(B * M);
                        CHECK(ff_weighted_resample_host(y.data(), lp.data(), B, D, K, M, 7, off, skip == 0 ? nullptr : s2.data(),
                                                        skip == 1 ? nullptr : idx2.data(), skip == 2 ? nullptr : mean2.data(),
                                                        skip == 3 ? nullptr : var2.data()) == FF_OK);
                        if (skip != 0) CHECK(s2 == s);
                        if (skip != 1) CHECK(idx2 == idx);
                        if (skip != 2) CHECK(mean2 == mean);
                        if (skip != 3) CHECK(var2 == var);
                    }
                }
    // non-finite rows: the point alone is degenerate
    {
        const int64_t B = 5;
        const int K = 64, D = 5, M = 6;
        std::vector<float> y(B * K * D, 0.25f), lp(B * K, -2.0f), s(B * M * D), mean(B * D), var(B * D);
        std::vector<int32_t> idx(B * M);
        lp[5] = -INFINITY;
        lp[K + 1] = NAN;
        for (int k = 0; k < K; ++k) lp[2 * K + k] = -INFINITY;
        lp[3 * K + 7] = INFINITY;
        CHECK(ff_weighted_resample_host(y.data(), lp.data(), B, D, K, M, 1, 0, s.data(), idx.data(), mean.data(), var.data()) == FF_OK);
        for (int64_t r = 0; r < B; ++r) {
            const bool bad = r >= 1 && r <= 3;
            for (int m = 0; m < M; ++m) CHECK(bad ? idx[r * M + m] == -1 : (idx[r * M + m] >= 0 && idx[r * M + m] < K && (r || idx[m] != 5)));
            for (int i = 0; i < M * D; ++i) CHECK(bad ? isnan(s[r * M * D + i]) : s[r * M * D + i] == 0.25f);
            for (int d = 0; d < D; ++d) CHECK(bad ? isnan(mean[r * D + d]) && isnan(var[r * D + d]) : mean[r * D + d] == 0.25f && var[r * D + d] == 0.f);
        }
    }
    std::vector<float> one(1, 0.f);
    int32_t i1 = 0;
    CHECK(ff_weighted_resample_host(nullptr, one.data(), 1, 1, 1, 1, 0, 0, one.data(), &i1, nullptr, nullptr) == FF_ERR_BADARG);
    CHECK(ff_weighted_resample_host(one.data(), one.data(), 1, 1, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == FF_ERR_BADARG);
    CHECK(ff_weighted_resample_host(one.data(), one.data(), 1, 1, 1, 4097, 0, 0, one.data(), &i1, nullptr, nullptr) == FF_ERR_BADARG);
    CHECK(ff_weighted_resample_host(one.data(), one.data(), 0, 1, 1, 1, 0, 0, one.data(), &i1, nullptr, nullptr) == FF_OK);
    printf(failures ? "observe posterior host check: %d failures\n" : "observe posterior host check: ok\n", failures);
    return failures ? 1 : 0;
}
