// Stand-alone host check of ff_probe_fill_host under AddressSanitizer and UndefinedBehaviorSanitizer (host code only;
// nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Iinclude -Iflowfusion_amd/csrc flowfusion_amd/csrc/ff_probe.hip tests/sanitize/probe_host_main.cpp \
//         -fsanitize=address,undefined -o probe_host_asan && ./probe_host_asan
//
// Every buffer is a heap allocation of exactly the documented size ([batch, K, dim] floats), so a write one element
// outside it is reported; the shapes are those of tests/test_hutchinson_multi_host.py (D that are no multiple of four,
// K = 1, a global row above 2^32) and the largest K the entry point takes.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "flowfusion_amd.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

int main()
{
    const int Ks[] = {1, 2, 15, 31, FF_MAX_HUTCH_PROBES}, Ds[] = {1, 3, 5, 16, 17};
    const int64_t offsets[] = {0, ((int64_t)1 << 33) + 7};
    for (int K : Ks)
        for (int D : Ds)
            for (int64_t off : offsets) {
                const int64_t B = K > 1000 ? 1 : 5;
                const float scale = 1.0f / sqrtf((float)K);
                std::vector<float> out((size_t)B * K * D, 0.f), one((size_t)B * D, 0.f), part((size_t)2 * K * D, 0.f);
                CHECK(ff_probe_fill_host(out.data(), B, K, D, 7, off, scale) == FF_OK);
                for (float v : out) CHECK(v == scale || v == -scale);
                // probe 0 is the single-probe fill; a slice is keyed by the global row
                CHECK(ff_probe_fill_host(one.data(), B, 1, D, 7, off, scale) == FF_OK);
                for (int64_t r = 0; r < B; ++r)
                    for (int d = 0; d < D; ++d) CHECK(one[r * D + d] == out[(size_t)r * K * D + d]);
                if (B >= 4) {
                    CHECK(ff_probe_fill_host(part.data(), 2, K, D, 7, off + 2, scale) == FF_OK);
                    for (size_t i = 0; i < part.size(); ++i) CHECK(part[i] == out[(size_t)2 * K * D + i]);
                }
            }
    float x = 0.f;
    CHECK(ff_probe_fill_host(&x, 0, 1, 1, 0, 0, 1.f) == FF_OK && x == 0.f);
    CHECK(ff_probe_fill_host(nullptr, 1, 1, 1, 0, 0, 1.f) == FF_ERR_BADARG);
    CHECK(ff_probe_fill_host(&x, -1, 1, 1, 0, 0, 1.f) == FF_ERR_BADARG);
    CHECK(ff_probe_fill_host(&x, 1, 0, 1, 0, 0, 1.f) == FF_ERR_BADARG);
    CHECK(ff_probe_fill_host(&x, 1, FF_MAX_HUTCH_PROBES + 1, 1, 0, 0, 1.f) == FF_ERR_BADARG);
    CHECK(ff_probe_fill_host(&x, 1, 1, 0, 0, 0, 1.f) == FF_ERR_BADARG);
    printf(failures ? "probe host check: %d failures\n" : "probe host check: ok\n", failures);
    return failures ? 1 : 0;
}
