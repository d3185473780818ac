// ff_probe.hip -- the probes of a K-probe Hutchinson launch (gfx950).
//
//   ff_probe_fill   out[r][k][d] = +-scale, the sign of z(seed, global row, index_k, d) of the library's counter-based
//                   stream: index_0 = FF_PROBE_NOISE_INDEX (the single-probe stream), index_k = FF_HUTCH_PROBE_NOISE_BASE + k.
//                   Written in torch ops: K ff_normal_fill launches, stack, where, mul -- here one write-only pass.
//
// A streaming kernel in the style of ff_aux.hip / ff_marginal.hip (roofline: HBM writes): one thread per (row, probe,
// block of four dimensions), grid-stride, 16-byte stores where the pointer and D allow, no LDS, no atomics.  The normals
// are ff_marginal.h's normals4 -- on the device the code of ff_normal_fill, bit for bit -- shared with the host twin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal.h"

namespace ff {
namespace probe {

typedef float v4f __attribute__((ext_vector_type(4)));

FF_HD uint32_t probe_index(int k) { return k == 0 ? FF_PROBE_NOISE_INDEX : FF_HUTCH_PROBE_NOISE_BASE + (uint32_t)k; }

// (z >= 0 ? scale : -scale: -0.0f counts as +, as in torch.where(z >= 0, 1, -1))
FF_HD void signs4(uint64_t seed, uint64_t gs, int k, uint32_t blk, float scale, float (&s)[4])
{
    float z[4];
    marginal::normals4(seed, gs, probe_index(k), blk, z);
    for (int j = 0; j < 4; ++j) s[j] = z[j] >= 0.f ? scale : -scale;
}

__global__ __launch_bounds__(256) void probe_fill_kernel(float* __restrict__ out, long long rows, int K, int dim, int nblk,
                                                         unsigned long long seed, long long sample_offset, float scale, int vec)
{
    // rows = batch K; item i = (row, blk), row = r K + k
    const long long total = rows * nblk;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / nblk;
        const int blk = (int)(i - row * nblk);
        const long long r = row / K;
        const int k = (int)(row - r * K);
        float s[4];
        signs4(seed, (unsigned long long)(r + sample_offset), k, (uint32_t)blk, scale, s);
        float* o = out + row * dim + 4 * blk;
        if (vec) {
            *(v4f*)o = v4f{s[0], s[1], s[2], s[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * blk + j < dim) o[j] = s[j];
        }
    }
}

static bool args_ok(const float* out, int64_t batch, int32_t K, int32_t dim)
{
    return out && batch >= 0 && dim >= 1 && K >= 1 && K <= FF_MAX_HUTCH_PROBES;
}

} // namespace probe
} // namespace ff

extern "C" int ff_probe_fill(float* out, int64_t batch, int32_t K, int32_t dim, uint64_t seed, int64_t sample_offset, float scale,
                             void* hip_stream)
{
    if (!ff::probe::args_ok(out, batch, K, dim)) return FF_ERR_BADARG;
    if (batch == 0) return FF_OK;
    const int nblk = (dim + 3) / 4;
    const long long rows = (long long)batch * K, want = (rows * nblk + 255) / 256;
    // a few workgroups per CU (256 CUs) saturate HBM with 16-byte accesses; never more than needed (ff_aux.hip)
    const unsigned grid = (unsigned)(want > 256 * 8 ? 256 * 8 : want);
    const int vec = (dim & 3) == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(ff::probe::probe_fill_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, out, rows, (int)K, (int)dim,
                       nblk, (unsigned long long)seed, (long long)sample_offset, scale, vec);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twin (CPU tests): the same header, in index order ----------------------------------------------------------
extern "C" int ff_probe_fill_host(float* out, int64_t batch, int32_t K, int32_t dim, uint64_t seed, int64_t sample_offset, float scale)
{
    if (!ff::probe::args_ok(out, batch, K, dim)) return FF_ERR_BADARG;
    const int nblk = (dim + 3) / 4;
    for (int64_t r = 0; r < batch; ++r)
        for (int k = 0; k < K; ++k)
            for (int blk = 0; blk < nblk; ++blk) {
                float s[4];
                ff::probe::signs4(seed, (uint64_t)(sample_offset + r), k, (uint32_t)blk, scale, s);
                for (int j = 0; j < 4 && 4 * blk + j < dim; ++j) out[(r * K + k) * dim + 4 * blk + j] = s[j];
            }
    return FF_OK;
}
