// Stand-alone host check of ff_mlp_pull_plan / ff_mlp_pull_wpack under AddressSanitizer and UndefinedBehaviorSanitizer (host
// code only; nothing here touches a GPU, and nothing is loaded into python):
//
//   hipcc -x c++ -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__=1 -I/opt/rocm/include -Iinclude -Iflowfusion_amd/csrc \
//         -fsanitize=address,undefined -fno-omit-frame-pointer flowfusion_amd/csrc/ff_api.cpp tests/sanitize/pull_wpack_main.cpp \
//         -o pull_wpack_asan && ./pull_wpack_asan
//
// The kernel tables the C API reads are defined HERE (the generated ff_table.cpp names every launcher of the library): the
// three pull-back units with a launcher that is never called, and empty tables for the other families.  Every weight, bias
// and output buffer is a heap allocation of exactly the documented size, so a read or write one element outside it is
// reported.  Shapes: the corners of the three units -- D 1 / 16 / 17 / 32, C 0 / 1 / 16, 1 and 4 hidden layers of widths
// 1 / 32 / 128 / 129 / 256, ragged widths, the first layer's x and conditional columns at the ends of a wider input, the
// deepest networks the planner takes (36 x 128, 18 x 256) -- and one step past them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "flowfusion_amd.h"
#include "ff_pull_registry.h"

namespace ff {
static int never_launched(const KernelArgs*, unsigned, unsigned, hipStream_t) { return 1; }
const KernelEntry g_kernels[] = {{0, 0, 0, 0, 0, 0, nullptr, "", nullptr, 0}};
const int g_n_kernels = 0;
const SplitKernelEntry g_split_kernels[] = {{0, 0, 0, 0, 0, nullptr, ""}};
const int g_n_split_kernels = 0;
const PairKernelEntry g_pair_kernels[] = {{0, 0, 0, 0, 0, {nullptr, nullptr, ""}, {nullptr, nullptr, ""}}};
const int g_n_pair_kernels = 0;
const PushKernelEntry g_push_kernels[] = {{0, 0, 0, 0, 0, nullptr, ""}};
const int g_n_push_kernels = 0;
const PullKernelEntry g_pull_kernels[] = {
    {16, 128, 4, 4, 1, never_launched, "mlp_pull_m16_h128_d4_c4"},
    {16, 256, 4, 4, 1, never_launched, "mlp_pull_m16_h256_d4_c4"},
    {16, 256, 8, 4, 1, never_launched, "mlp_pull_m16_h256_d8_c4"},
};
const int g_n_pull_kernels = 3;
}

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// packs a network of the given shape from exactly-sized heap buffers; returns the sum of the pack (so that every word is read)
static double pack(int D, int C, const std::vector<int>& hidden, int lead, int unit)
{
    const int NH = (int)hidden.size(), in0 = lead + D + C;
    ff_mlp_plan_t plan;
    CHECK(ff_mlp_pull_plan(D, C, NH, hidden.data(), FF_ACT_SILU, FF_PREC_F32, &plan) == FF_OK);
    CHECK(plan.kernel_id == FF_PULL_KERNEL_BASE + unit);
    std::vector<std::vector<float>> W(NH + 1), b(NH + 1);
    std::vector<const float*> Wp(NH + 1), bp(NH + 1);
    for (int l = 0; l <= NH; ++l) {
        const int rows = l < NH ? hidden[l] : D, cols = l == 0 ? in0 : hidden[l - 1];
        W[l].resize((size_t)rows * cols);
        b[l].resize((size_t)rows);
        for (size_t i = 0; i < W[l].size(); ++i) W[l][i] = (float)((int)((i * 2654435761u) >> 20 & 255) - 128) / 64.f;
        for (size_t i = 0; i < b[l].size(); ++i) b[l][i] = (float)i / 8.f;
        Wp[l] = W[l].data();
        bp[l] = b[l].data();
    }
    const size_t n = ff_mlp_pull_wpack_floats(&plan);
    CHECK(n > 0 && ff_mlp_wpack_floats(&plan) == 0);
    std::vector<float> out(n, -1.f);
    // x columns right behind `lead` time columns, the conditional columns at the end of the input
    CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead, lead + D, out.data()) == FF_OK);
    double sum = 0.0, wsum = 0.0;
    for (float v : out) sum += v;
    // the refusals: a column range past the input, a width past the unit, a missing layer, the other packer
    CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead + C + 1, lead, out.data()) == FF_ERR_BADARG);
    if (C > 0) CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead, lead + D + 1, out.data()) == FF_ERR_BADARG);
    CHECK(ff_mlp_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead, lead + D, out.data()) == FF_ERR_BADARG);
    CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead, lead + D, nullptr) == FF_ERR_BADARG);
    std::vector<int> wide(hidden);
    wide[0] = plan.width + 1;
    CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), wide.data(), in0, lead, lead + D, out.data()) == FF_ERR_BADARG);
    const float* keep = Wp[NH];
    Wp[NH] = nullptr;
    CHECK(ff_mlp_pull_wpack(&plan, Wp.data(), bp.data(), hidden.data(), in0, lead, lead + D, out.data()) == FF_ERR_BADARG);
    Wp[NH] = keep;
    // every weight the network reads appears twice in the pack (forward and transposed), every bias of layers 2 .. once
    // (the first layer's bias travels in the evaluation rows): the pack's sum says nothing was dropped or doubled
    for (int l = 0; l <= NH; ++l) {
        const int rows = l < NH ? hidden[l] : D, cols = l == 0 ? in0 : hidden[l - 1];
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c)
                if (l > 0 || (c >= lead && c < lead + D + C)) wsum += 2.0 * W[l][(size_t)r * cols + c];
        if (l > 0) for (float v : b[l]) wsum += v;
    }
    CHECK(sum > wsum - 1e-3 * (1.0 + (wsum < 0 ? -wsum : wsum)) && sum < wsum + 1e-3 * (1.0 + (wsum < 0 ? -wsum : wsum)));
    return sum;
}

int main()
{
    pack(1, 0, {1}, 0, 0);
    pack(1, 0, {32}, 3, 0);
    pack(16, 16, {128, 128, 128, 128}, 1, 0);
    pack(16, 1, {128, 32, 7, 128}, 17, 0);
    pack(4, 0, std::vector<int>(36, 128), 1, 0);
    pack(1, 16, {129}, 0, 1);
    pack(16, 16, {256, 256, 256, 256}, 17, 1);
    pack(3, 1, {64, 200}, 1, 1);
    pack(16, 0, std::vector<int>(18, 256), 1, 1);
    pack(17, 0, {1}, 0, 2);
    pack(32, 16, {256, 256, 256, 256}, 17, 2);
    pack(17, 16, {128}, 1, 2);
    pack(32, 1, {32, 256, 1, 256}, 3, 2);
    // one step past the envelope
    ff_mlp_plan_t plan;
    const int w19[19] = {256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256, 256};
    CHECK(ff_mlp_pull_plan(16, 0, 19, w19, FF_ACT_SILU, FF_PREC_F32, &plan) == FF_ERR_UNSUPPORTED);
    CHECK(ff_mlp_pull_plan(32, 0, 18, w19, FF_ACT_SILU, FF_PREC_F32, &plan) == FF_ERR_UNSUPPORTED);
    const int one[1] = {257};
    CHECK(ff_mlp_pull_plan(4, 0, 1, one, FF_ACT_SILU, FF_PREC_F32, &plan) == FF_ERR_UNSUPPORTED);
    CHECK(ff_mlp_pull_wpack_floats(&plan) == 0 && ff_mlp_pull_wpack_floats(nullptr) == 0);
    printf(failures ? "pull wpack host check: %d failures\n" : "pull wpack host check: ok\n", failures);
    return failures ? 1 : 0;
}
