// ff_observe.hip -- the two ends of the K-draw log-density of noisy observations (gfx950), around any log-density.
//
//   ff_observe_expand   y[r K + k] = x[r] - noise_std[r] * z(r, k), cond_out[r K + k] = cond[r]: the K de-noised candidates
//                       of observation r, its draws from the library's counter-based stream under the noise indices
//                       FF_OBS_NOISE_BASE + k.  Written in torch ops: K ff_normal_fill launches, a stack, repeat_interleave,
//                       a multiply and a subtract over [B K, D] temporaries -- here one pass, write-only beyond x, noise_std
//                       and cond.
//   ff_logmeanexp       out[r] = logsumexp_k lp[r K + k] - log K and the effective sample size of the K weights.  Written
//                       in torch ops: a float64 copy, logsumexp, a max, an exp and two sums -- here one read of lp.
//
// Both are streaming kernels in the style of ff_marginal.hip (roofline: HBM): grid-stride loops, 16-byte accesses where
// the pointers and D allow (a scalar body otherwise, same arithmetic in the same order), consecutive lanes on consecutive
// addresses, no LDS, no atomics.  A row of the expansion is shared by P = lanes_per_row(D) lanes (one block of four
// dimensions each); a data point of the reduction by a group of G = lanes_per_point(K) lanes (draws k = lane, lane + G,
// ..), whose states meet by an xor-butterfly inside the group, so a point's result is fixed by K and its own data: not by
// the grid, the batch or its place.  The arithmetic is ff_observe.h, shared with the host twins below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_observe.h"

namespace ff {
namespace observe {

typedef float v4f __attribute__((ext_vector_type(4)));

struct ExpandArgs {
    const float* x;
    const float* noise_std;
    const float* cond;
    float* y;
    float* cond_out;
    long long rows;                 // B K
    long long stride_r;             // the grid's row stride / K ...
    int stride_k;                   // ... and % K: (r, k) advance without a division per trip
    int std_stride;                 // 0: one [D] vector, D: a row per data point
    int D, C, K;
    unsigned long long seed;
    long long sample_offset;
    int log_p;                      // log2 of the lanes per row
    int vec, cvec;                  // the state / the conditional rows move as 16-byte elements
};

__global__ __launch_bounds__(256) void observe_expand_kernel(const ExpandArgs a)
{
    const int P = 1 << a.log_p, D = a.D, C = a.C, K = a.K, nblk = (D + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = (int)(gtid & (P - 1));
    long long row = gtid >> a.log_p;
    if (row >= a.rows) return;
    const long long nrows = ((long long)gridDim.x * blockDim.x) >> a.log_p;
    long long r = row / K;
    int k = (int)(row - r * K);
    for (; row < a.rows; row += nrows) {
        const unsigned long long gs = (unsigned long long)(a.sample_offset + r);
        const float* xr = a.x + r * D;
        const float* sr = a.noise_std + r * a.std_stride;
        float* yr = a.y + row * D;
        for (int blk = sub; blk < nblk; blk += P) {
            float z[4];
            normals4(a.seed, gs, FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
            const int d0 = 4 * blk;
            if (a.vec) {
                const v4f xv = *(const v4f*)(xr + d0), sv = *(const v4f*)(sr + d0);
                *(v4f*)(yr + d0) = v4f{perturb(xv[0], sv[0], z[0]), perturb(xv[1], sv[1], z[1]),
                                       perturb(xv[2], sv[2], z[2]), perturb(xv[3], sv[3], z[3])};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < D) yr[d0 + j] = perturb(xr[d0 + j], sr[d0 + j], z[j]);
            }
        }
        if (a.cond) {
            const float* cr = a.cond + r * C;
            float* co = a.cond_out + row * C;
            if (a.cvec)
                for (int c = sub; c < C / 4; c += P) ((v4f*)co)[c] = ((const v4f*)cr)[c];
            else
                for (int c = sub; c < C; c += P) co[c] = cr[c];
        }
        r += a.stride_r;
        k += a.stride_k;
        if (k >= K) { k -= K; ++r; }
    }
}

struct ReduceArgs {
    const float* lp;
    float* out;
    float* out_ess;
    long long B;
    int K;
    int log_g;                      // log2 of the lanes per data point
};

__global__ __launch_bounds__(256) void logmeanexp_kernel(const ReduceArgs a)
{
    const int G = 1 << a.log_g, K = a.K;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    // (the bound is uniform over a group -- and, with G dividing 64, the groups of a wavefront run the same trips or
    // fall out together only at the end: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const float* lr = a.lp + pt * K;
        Lse st = lse_empty();
        float only = 0.f;
        for (int k = lane; k < K; k += G) {
            only = lr[k];
            lse_add(st, (double)only);
        }
        for (int off = 1; off < G; off <<= 1) {
            Lse o;
            o.m = __shfl_xor(st.m, off);
            o.s1 = __shfl_xor(st.s1, off);
            o.s2 = __shfl_xor(st.s2, off);
            st = lse_merge(st, o);
        }
        if (lane == 0) lme_finish(st, K, only, a.out + pt, a.out_ess ? a.out_ess + pt : nullptr);
    }
}

static unsigned stream_grid(long long threads)
{
    // a few workgroups per CU (256 CUs) saturate HBM with 16-byte accesses; never more than needed (ff_aux.hip)
    const long long want = (threads + 255) / 256;
    const long long cap = 256 * 8;
    return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

static int log2_of(int pow2)
{
    int l = 0;
    while ((1 << l) < pow2) ++l;
    return l;
}

static bool expand_args_ok(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond, int64_t B,
                           int32_t D, int32_t C, int32_t K, const float* y, const float* cond_out)
{
    if (!x || !noise_std || !y || B < 0 || D < 1 || K < 1 || K > kMaxDraws) return false;
    if (std_row_stride != 0 && std_row_stride != D) return false;
    if (cond && (C < 1 || !cond_out)) return false;
    return true;
}

static bool reduce_args_ok(const float* lp, int64_t B, int32_t K, const float* out)
{
    return lp && out && B >= 0 && K >= 1 && K <= kMaxDraws;
}

} // namespace observe
} // namespace ff

using namespace ff::observe;

extern "C" int ff_observe_expand(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond,
                                 int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* y,
                                 float* cond_out, void* hip_stream)
{
    if (!expand_args_ok(x, noise_std, std_row_stride, cond, B, D, C, K, y, cond_out)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    ExpandArgs a;
    a.x = x; a.noise_std = noise_std; a.cond = cond; a.y = y; a.cond_out = cond ? cond_out : nullptr;
    a.rows = (long long)B * K;
    a.std_stride = std_row_stride;
    a.D = D; a.C = cond ? C : 0; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset;
    const int P = ff::marginal::lanes_per_row(D);
    a.log_p = log2_of(P);
    a.vec = (D & 3) == 0 && (((uintptr_t)x | (uintptr_t)noise_std | (uintptr_t)y) & 15) == 0;
    a.cvec = cond && (C & 3) == 0 && (((uintptr_t)cond | (uintptr_t)cond_out) & 15) == 0;
    const unsigned grid = stream_grid(a.rows * P);
    const long long nrows = ((long long)grid * 256) >> a.log_p;
    a.stride_r = nrows / K;
    a.stride_k = (int)(nrows % K);
    hipLaunchKernelGGL(observe_expand_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_logmeanexp(const float* lp, int64_t B, int32_t K, float* out, float* out_ess, void* hip_stream)
{
    if (!reduce_args_ok(lp, B, K, out)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    ReduceArgs a;
    a.lp = lp; a.out = out; a.out_ess = out_ess;
    a.B = B; a.K = K;
    const int G = lanes_per_point(K);
    a.log_g = log2_of(G);
    hipLaunchKernelGGL(logmeanexp_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twins (CPU tests): the same header, rows and draws in index order ---------------------------------------
extern "C" int ff_observe_expand_host(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond,
                                      int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset,
                                      float* y, float* cond_out)
{
    if (!expand_args_ok(x, noise_std, std_row_stride, cond, B, D, C, K, y, cond_out)) return FF_ERR_BADARG;
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r)
        for (int k = 0; k < K; ++k) {
            const int64_t row = r * K + k;
            for (int blk = 0; blk < nblk; ++blk) {
                float z[4];
                normals4(seed, (uint64_t)(sample_offset + r), FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
                for (int j = 0; j < 4 && 4 * blk + j < D; ++j) {
                    const int d = 4 * blk + j;
                    y[row * D + d] = perturb(x[r * D + d], noise_std[r * std_row_stride + d], z[j]);
                }
            }
            if (cond)
                for (int c = 0; c < C; ++c) cond_out[row * C + c] = cond[r * C + c];
        }
    return FF_OK;
}

extern "C" int ff_logmeanexp_host(const float* lp, int64_t B, int32_t K, float* out, float* out_ess)
{
    if (!reduce_args_ok(lp, B, K, out)) return FF_ERR_BADARG;
    for (int64_t r = 0; r < B; ++r) {
        Lse st = lse_empty();
        for (int k = 0; k < K; ++k) lse_add(st, (double)lp[r * K + k]);
        lme_finish(st, K, lp[r * K], out + r, out_ess ? out_ess + r : nullptr);
    }
    return FF_OK;
}
