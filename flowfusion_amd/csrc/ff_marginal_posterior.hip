// ff_marginal_posterior.hip -- the per-object posterior of a NOISY observation under a symplectic flow (gfx950), behind the
// launches of its marginal likelihood: ff_marginal_observe_expand -> the solve -> ff_marginal_weigh -> this.
//
//   ff_marginal_observe_resample   the posterior of observation r from the K joint draws of its marginal and their
//                        log-weights lw (double, ff_marginal_weigh's): M multinomial draws of the candidates y_k = x -
//                        noise_std z_k by the weights exp(lw_k - max lw) (the candidates, and their indices) and the weighted
//                        mean and variance.  Written with the existing kernels: ff_observe_expand into a [B K, D] particle
//                        buffer, the lw rounded to fp32, ff_weighted_resample -- here one pass over lw, x and noise_std: the
//                        weights stay in double and NO row of y is ever read from memory, every candidate is regenerated from
//                        the counter-based stream (marginal::normals4 of block d0 / 4, then observe::perturb) where a moment or
//                        a sample needs it, as ff_marginal_observe_grad_reduce regenerates z.
//
// The lane layout is weighted_resample_kernel's (ff_observe.hip) line by line: a group of G = lanes_per_point(K) lanes per
// point, every lane a CONTIGUOUS segment of ceil(K / G) draws, the running sum of the weights as the __shfl_up scan of the
// segment sums plus the lane's own running sum, four targets (one Philox block) per walk, a minimum over the group, the last
// draw of positive weight for a target within rounding of W; the moments one block of four dimensions at a time, a butterfly
// over the lanes, one division per point.  Given the same particles and weights every output is that kernel's, bit for bit.
// A streaming kernel in the style of ff_marginal.hip: grid-stride loops, 16-byte stores where the pointers and D allow (a
// scalar body otherwise, same arithmetic in the same order), no LDS, no atomics.  A point's result is fixed by (K, D) and its
// own data: not by the grid, the batch or its place.  The arithmetic is ff_marginal_posterior.h (over ff_marginal.h,
// ff_observe.h and ff_marginal_observe.h), shared with the host twin below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal_posterior.h"

namespace ff {
namespace marginal_posterior {

typedef float v4f __attribute__((ext_vector_type(4)));

struct ResampleArgs {
    const float* x;
    const float* noise_std;
    const double* lw;
    float* samples;
    int32_t* index;
    float* mean;
    float* var;
    long long B;
    int std_stride;                 // 0: one [D] vector, D: a row per data point
    int D, K, M;
    unsigned long long seed;
    long long sample_offset;
    int log_g;                      // log2 of the lanes per data point
    int seg;                        // draws per lane: lane l holds the draws [l seg, (l + 1) seg) below K
    int xvec;                       // x and noise_std are read as 16-byte elements
    int vec;                        // samples move as 16-byte elements
};

__global__ __launch_bounds__(256) void marginal_observe_resample_kernel(const ResampleArgs a)
{
    using marginal::lse_factor;
    using marginal::max_add;
    using observe::group_sum4;
    using observe::load_block;
    using observe::moment1_add;
    using observe::moment2_add;
    using observe::resample_targets;
    const int G = 1 << a.log_g, K = a.K, D = a.D, M = a.M, nblk = (D + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    const int k0 = lane * a.seg < K ? lane * a.seg : K, k1 = k0 + a.seg < K ? k0 + a.seg : K;
    const float qnan = __builtin_nanf("");
    // (the bound is uniform over a group -- and, with G dividing 64, the groups of a wavefront run the same trips or fall
    // out together only at the end: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const double* lr = a.lw + pt * K;
        const float* xr = a.x + pt * D;
        const float* nr = a.noise_std + pt * a.std_stride;
        const unsigned long long gs = (unsigned long long)(a.sample_offset + pt);
        float* sr = a.samples ? a.samples + pt * M * D : nullptr;
        int32_t* ir = a.index ? a.index + pt * M : nullptr;

        // the maximum (exact in any order) and whether the point has a posterior at all
        double m = -INFINITY;
        int bad = 0;
        for (int k = k0; k < k1; ++k) max_add(m, bad, lr[k]);
        for (int off = 1; off < G; off <<= 1) {
            const double o = __shfl_xor(m, off);
            m = o > m ? o : m;
            bad |= __shfl_xor(bad, off);
        }
        if (point_degenerate(bad, m)) {
            if (sr)
                for (long long i = lane; i < (long long)M * D; i += G) sr[i] = qnan;
            if (ir)
                for (int s = lane; s < M; s += G) ir[s] = -1;
            for (int d = lane; d < D; d += G) {
                if (a.mean) a.mean[pt * D + d] = qnan;
                if (a.var) a.var[pt * D + d] = qnan;
            }
            continue;
        }

        // the lane's segment: its sum and its last draw of positive weight; then the scan of the segment sums
        double s = 0.0, w_first = 0.0;
        int last = -1;
        for (int k = k0; k < k1; ++k) {
            const double w = lse_factor(lr[k], m);
            if (k == k0) w_first = w;
            s += w;
            if (w > 0.0) last = k;
        }
        double inc = s;
        for (int off = 1; off < G; off <<= 1) {
            const double o = __shfl_up(inc, off, G);
            if (lane >= off) inc += o;
            const int l = __shfl_xor(last, off);
            last = l > last ? l : last;
        }
        double excl = __shfl_up(inc, 1, G);
        if (lane == 0) excl = 0.0;
        const double W = __shfl(excl + s, G - 1, G);          // the running sum as the last lane sees it at its last draw
        const double rW = 1.0 / W;                            // one division per point: the moments are sums times 1 / W

        if (M > 0 && (sr || ir))
            for (int m0 = 0; m0 < M; m0 += 4) {
                double t[4];
                resample_targets(a.seed, gs, (uint32_t)(m0 >> 2), W, t);
                int c[4] = {K, K, K, K};
                double run = 0.0;
                for (int k = k0; k < k1; ++k) {
                    const double w = k == k0 ? w_first : lse_factor(lr[k], m);
                    run += w;
                    const double cum = excl + run;
                    if (w > 0.0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (cum > t[j] && k < c[j]) c[j] = k;
                    }
                }
                for (int off = 1; off < G; off <<= 1)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int o = __shfl_xor(c[j], off);
                        c[j] = o < c[j] ? o : c[j];
                    }
                // (a target within rounding of W that no lane's running sum exceeds: the last draw of positive weight)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c[j] >= K) c[j] = last;
                const int nrow = M - m0 < 4 ? M - m0 : 4;
                if (ir && lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nrow) ir[m0 + j] = c[j];
                if (sr)
                    for (int u = lane; u < nrow * nblk; u += G) {
                        const int j = u / nblk, blk = u - j * nblk, d0 = 4 * blk;
                        const int src = j == 0 ? c[0] : j == 1 ? c[1] : j == 2 ? c[2] : c[3];
                        float xb[4], sb[4], v[4];
                        load_block(xr, d0, D, a.xvec, xb);
                        load_block(nr, d0, D, a.xvec, sb);
                        particle_block(xb, sb, a.seed, gs, src, blk, D, v);       // the chosen candidate, regenerated
                        float* to = sr + (long long)(m0 + j) * D;
                        if (a.vec) {
                            *(v4f*)(to + d0) = v4f{v[0], v[1], v[2], v[3]};
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (d0 + i < D) to[d0 + i] = v[i];
                        }
                    }
            }

        if (a.mean || a.var)
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = 4 * blk;
                double acc[4] = {0.0, 0.0, 0.0, 0.0}, mu[4];
                float xb[4], sb[4];
                load_block(xr, d0, D, a.xvec, xb);
                load_block(nr, d0, D, a.xvec, sb);
                for (int k = k0; k < k1; ++k) {
                    float v[4];
                    particle_block(xb, sb, a.seed, gs, k, blk, D, v);
                    moment1_add(acc, k == k0 ? w_first : lse_factor(lr[k], m), v);
                }
                group_sum4(acc, G);
#pragma unroll
                for (int j = 0; j < 4; ++j) mu[j] = acc[j] * rW;
                if (a.mean && lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (d0 + j < D) a.mean[pt * D + d0 + j] = (float)mu[j];
                if (!a.var) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = 0.0;
                for (int k = k0; k < k1; ++k) {
                    float v[4];
                    particle_block(xb, sb, a.seed, gs, k, blk, D, v);
                    moment2_add(acc, k == k0 ? w_first : lse_factor(lr[k], m), v, mu);
                }
                group_sum4(acc, G);
                if (lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (d0 + j < D) a.var[pt * D + d0 + j] = (float)(acc[j] * rW);
            }
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

} // namespace marginal_posterior
} // namespace ff

using namespace ff::marginal_posterior;

extern "C" int ff_marginal_observe_resample(const float* x, const float* noise_std, int32_t std_row_stride, const double* lw,
                                            int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed, int64_t sample_offset,
                                            float* samples, int32_t* index, float* mean, float* var, void* hip_stream)
{
    if (!resample_args_ok(x, noise_std, std_row_stride, lw, B, D, K, M, samples, index, mean, var)) return FF_ERR_BADARG;
    if (M == 0) { samples = nullptr; index = nullptr; }
    if (B == 0 || !(samples || index || mean || var)) return FF_OK;
    ResampleArgs a;
    a.x = x; a.noise_std = noise_std; a.lw = lw;
    a.samples = samples; a.index = index; a.mean = mean; a.var = var;
    a.B = B; a.std_stride = std_row_stride;
    a.D = D; a.K = K; a.M = M;
    a.seed = seed; a.sample_offset = sample_offset;
    const int G = ff::observe::lanes_per_point(K);
    a.log_g = log2_of(G);
    a.seg = (K + G - 1) / G;
    a.xvec = (D & 3) == 0 && (((uintptr_t)x | (uintptr_t)noise_std) & 15) == 0;
    a.vec = (D & 3) == 0 && ((uintptr_t)samples & 15) == 0;
    hipLaunchKernelGGL(marginal_observe_resample_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twin (CPU tests): the same headers, the draws in index order as ff_weighted_resample_host -------------------
extern "C" int ff_marginal_observe_resample_host(const float* x, const float* noise_std, int32_t std_row_stride,
                                                 const double* lw, int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed,
                                                 int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var)
{
    if (!resample_args_ok(x, noise_std, std_row_stride, lw, B, D, K, M, samples, index, mean, var)) return FF_ERR_BADARG;
    using ff::marginal::lse_factor;
    using ff::marginal::max_add;
    using ff::observe::moment1_add;
    using ff::observe::moment2_add;
    using ff::observe::resample_targets;
    if (M == 0) { samples = nullptr; index = nullptr; }
    const float qnan = nanf("");
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r) {
        const double* lr = lw + r * K;
        const float* xr = x + r * D;
        const float* nr = noise_std + r * std_row_stride;
        const uint64_t gs = (uint64_t)(sample_offset + r);
        float* sr = samples ? samples + r * M * D : nullptr;
        int32_t* ir = index ? index + r * M : nullptr;
        const auto block_of = [&](const float* row, int d0, float (&b)[4]) {
            for (int j = 0; j < 4; ++j) b[j] = d0 + j < D ? row[d0 + j] : 0.f;
        };
        double m = -INFINITY;
        int bad = 0;
        for (int k = 0; k < K; ++k) max_add(m, bad, lr[k]);
        if (point_degenerate(bad, m)) {
            for (int64_t i = 0; sr && i < (int64_t)M * D; ++i) sr[i] = qnan;
            for (int s = 0; ir && s < M; ++s) ir[s] = -1;
            for (int d = 0; d < D; ++d) {
                if (mean) mean[r * D + d] = qnan;
                if (var) var[r * D + d] = qnan;
            }
            continue;
        }
        double W = 0.0;
        int last = -1;
        for (int k = 0; k < K; ++k) {
            const double w = lse_factor(lr[k], m);
            W += w;
            if (w > 0.0) last = k;
        }
        const double rW = 1.0 / W;
        for (int m0 = 0; (sr || ir) && m0 < M; m0 += 4) {
            double t[4];
            resample_targets(seed, gs, (uint32_t)(m0 >> 2), W, t);
            int c[4] = {K, K, K, K};
            double cum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double w = lse_factor(lr[k], m);
                cum += w;
                if (w > 0.0)
                    for (int j = 0; j < 4; ++j)
                        if (cum > t[j] && k < c[j]) c[j] = k;
            }
            for (int j = 0; j < 4 && m0 + j < M; ++j) {
                const int src = c[j] >= K ? last : c[j];
                if (ir) ir[m0 + j] = src;
                for (int blk = 0; sr && blk < nblk; ++blk) {
                    float xb[4], sb[4], v[4];
                    block_of(xr, 4 * blk, xb);
                    block_of(nr, 4 * blk, sb);
                    particle_block(xb, sb, seed, gs, src, blk, D, v);
                    for (int i = 0; i < 4 && 4 * blk + i < D; ++i) sr[(int64_t)(m0 + j) * D + 4 * blk + i] = v[i];
                }
            }
        }
        for (int blk = 0; (mean || var) && blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, mu[4];
            float xb[4], sb[4], v[4];
            block_of(xr, d0, xb);
            block_of(nr, d0, sb);
            for (int k = 0; k < K; ++k) {
                particle_block(xb, sb, seed, gs, k, blk, D, v);
                moment1_add(acc, lse_factor(lr[k], m), v);
            }
            for (int j = 0; j < 4; ++j) mu[j] = acc[j] * rW;
            for (int j = 0; mean && j < 4 && d0 + j < D; ++j) mean[r * D + d0 + j] = (float)mu[j];
            if (!var) continue;
            for (int j = 0; j < 4; ++j) acc[j] = 0.0;
            for (int k = 0; k < K; ++k) {
                particle_block(xb, sb, seed, gs, k, blk, D, v);
                moment2_add(acc, lse_factor(lr[k], m), v, mu);
            }
            for (int j = 0; j < 4 && d0 + j < D; ++j) var[r * D + d0 + j] = (float)(acc[j] * rW);
        }
    }
    return FF_OK;
}
