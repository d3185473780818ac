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
//   ff_weighted_resample  the posterior of observation r from the same K rows and their log-densities: M multinomial
//                       draws (rows copied bit for bit, and their indices) and the weighted mean and variance.  Written
//                       in torch ops: a float64 softmax, a cumsum, a searchsorted, a gather and the weighted moments over
//                       [B K, D] temporaries, on torch's generator -- here one pass over lp and y, uniforms from the
//                       counter-based stream.  A group of G lanes per point as in the reduction, but every lane holds a
//                       CONTIGUOUS segment of ceil(K / G) draws: the running sum of the weights is the scan of the
//                       segment sums over the group plus the lane's own running sum, so the draw a target falls on is
//                       found by one walk of every lane over its segment (four targets -- one Philox block -- per walk)
//                       and a minimum over the group.  The moments take one block of four dimensions at a time: every
//                       lane adds its segment, a butterfly adds the lanes; the variance is a second pass about the mean.
//
//   ff_observe_keep     which of the K rows of a point carry weight in the GRADIENT of its log-mean-exp: keep[r K + k] =
//                       (normalised weight > 0 and >= min_weight), from the reduction's own state and butterfly.
//   ff_observe_grad_reduce  the gradient of the log-mean-exp from the kept rows' own gradients: sum_k w_k g_k / W for x and
//                       the conditional, -sum_k w_k z_k g_k / W for noise_std with z regenerated, one block of four
//                       dimensions at a time as the moments above.  Written in torch ops: a float64 softmax, K
//                       ff_normal_fill launches, two weighted sums over [B K, D] temporaries -- here one pass over lp and
//                       the kept rows; a row that was not kept is not read.
//
// All are streaming kernels in the style of ff_marginal.hip (roofline: HBM): grid-stride loops, 16-byte accesses where
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

struct ResampleArgs {
    const float* y;
    const float* lp;
    float* samples;
    int32_t* index;
    float* mean;
    float* var;
    long long B;
    int D, K, M;
    unsigned long long seed;
    long long sample_offset;
    int log_g;                      // log2 of the lanes per data point
    int seg;                        // draws per lane: lane l holds the draws [l seg, (l + 1) seg) below K
    int vec;                        // y and samples move as 16-byte elements
};

__global__ __launch_bounds__(256) void weighted_resample_kernel(const ResampleArgs a)
{
    const int G = 1 << a.log_g, K = a.K, D = a.D, M = a.M, nblk = (D + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    const int k0 = lane * a.seg < K ? lane * a.seg : K, k1 = k0 + a.seg < K ? k0 + a.seg : K;
    const float qnan = __builtin_nanf("");
    // (the bound is uniform over a group, as in logmeanexp_kernel: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const float* lr = a.lp + pt * K;
        const float* yr = a.y + pt * K * D;
        float* sr = a.samples ? a.samples + pt * M * D : nullptr;
        int32_t* ir = a.index ? a.index + pt * M : nullptr;

        // the maximum (exact in any order) and whether the point has a posterior at all
        float mx = -INFINITY;
        int bad = 0;
        for (int k = k0; k < k1; ++k) {
            const float v = lr[k];
            bad |= weight_bad(v);
            mx = v > mx ? v : mx;
        }
        for (int off = 1; off < G; off <<= 1) {
            const float o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
            bad |= __shfl_xor(bad, off);
        }
        if (bad || mx == -INFINITY) {
            if (sr)
                for (long long i = lane; i < (long long)M * D; i += G) sr[i] = qnan;
            if (ir)
                for (int m = lane; m < M; m += G) ir[m] = -1;
            for (int d = lane; d < D; d += G) {
                if (a.mean) a.mean[pt * D + d] = qnan;
                if (a.var) a.var[pt * D + d] = qnan;
            }
            continue;
        }

        // the lane's segment: its sum and its last draw of positive weight; then the scan of the segment sums
        const double m = (double)mx;
        double s = 0.0, w_first = 0.0;
        int last = -1;
        for (int k = k0; k < k1; ++k) {
            const double w = weight(lr[k], m);
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
                resample_targets(a.seed, (unsigned long long)(a.sample_offset + pt), (uint32_t)(m0 >> 2), W, t);
                int c[4] = {K, K, K, K};
                double run = 0.0;
                for (int k = k0; k < k1; ++k) {
                    const double w = k == k0 ? w_first : weight(lr[k], m);
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
                        const int j = u / nblk, d0 = 4 * (u - j * nblk);
                        const int src = j == 0 ? c[0] : j == 1 ? c[1] : j == 2 ? c[2] : c[3];
                        const float* from = yr + (long long)src * D;
                        float* to = sr + (long long)(m0 + j) * D;
                        if (a.vec) {
                            *(v4f*)(to + d0) = *(const v4f*)(from + d0);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (d0 + i < D) to[d0 + i] = from[d0 + i];
                        }
                    }
            }

        if (a.mean || a.var)
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = 4 * blk;
                double acc[4] = {0.0, 0.0, 0.0, 0.0}, mu[4];
                for (int k = k0; k < k1; ++k) {
                    float v[4];
                    load_block(yr + (long long)k * D, d0, D, a.vec, v);
                    moment1_add(acc, k == k0 ? w_first : weight(lr[k], m), v);
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
                    load_block(yr + (long long)k * D, d0, D, a.vec, v);
                    moment2_add(acc, k == k0 ? w_first : weight(lr[k], m), v, mu);
                }
                group_sum4(acc, G);
                if (lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (d0 + j < D) a.var[pt * D + d0 + j] = (float)(acc[j] * rW);
            }
    }
}

struct KeepArgs {
    const float* lp;
    int32_t* keep;
    long long B;
    int K;
    double min_weight;
    int log_g;                      // log2 of the lanes per data point
};

__global__ __launch_bounds__(256) void observe_keep_kernel(const KeepArgs a)
{
    const int G = 1 << a.log_g, K = a.K;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    // (the bound is uniform over a group, as in logmeanexp_kernel: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const float* lr = a.lp + pt * K;
        int32_t* kr = a.keep + pt * K;
        Lse st = lse_empty();
        int bad = 0;
        for (int k = lane; k < K; k += G) {
            const float v = lr[k];
            bad |= weight_bad(v);
            lse_add(st, (double)v);
        }
        for (int off = 1; off < G; off <<= 1) {
            Lse o;
            o.m = __shfl_xor(st.m, off);
            o.s1 = __shfl_xor(st.s1, off);
            o.s2 = __shfl_xor(st.s2, off);
            st = lse_merge(st, o);
            bad |= __shfl_xor(bad, off);
        }
        const bool none = point_degenerate(bad, st.m);
        for (int k = lane; k < K; k += G) kr[k] = none ? 0 : keep_draw(lr[k], st.m, st.s1, a.min_weight);
    }
}

struct GradReduceArgs {
    const float* lp;
    const int32_t* row_of;
    const float* gx_rows;
    const float* gc_rows;
    float* grad_x;
    float* grad_c;
    float* grad_noise_std;
    long long B;
    int D, C, K;
    unsigned long long seed;
    long long sample_offset;
    int log_g;                      // log2 of the lanes per data point
    int seg;                        // draws per lane: lane l holds the draws [l seg, (l + 1) seg) below K
    int vec, cvec;                  // gx_rows / gc_rows move as 16-byte elements
};

__global__ __launch_bounds__(256) void observe_grad_reduce_kernel(const GradReduceArgs a)
{
    const int G = 1 << a.log_g, K = a.K, D = a.D, C = a.C, nblk = (D + 3) / 4, ncblk = (C + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    const int k0 = lane * a.seg < K ? lane * a.seg : K, k1 = k0 + a.seg < K ? k0 + a.seg : K;
    const float qnan = __builtin_nanf("");
    // (the bound is uniform over a group, as in logmeanexp_kernel: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const float* lr = a.lp + pt * K;
        const int32_t* ro = a.row_of + pt * K;
        const unsigned long long gs = (unsigned long long)(a.sample_offset + pt);

        float mx = -INFINITY;
        int bad = 0;
        for (int k = k0; k < k1; ++k) {
            const float v = lr[k];
            bad |= weight_bad(v);
            mx = v > mx ? v : mx;
        }
        for (int off = 1; off < G; off <<= 1) {
            const float o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
            bad |= __shfl_xor(bad, off);
        }
        if (point_degenerate(bad, (double)mx)) {
            for (int d = lane; d < D; d += G) {
                a.grad_x[pt * D + d] = qnan;
                if (a.grad_noise_std) a.grad_noise_std[pt * D + d] = qnan;
            }
            if (a.gc_rows)
                for (int c = lane; c < C; c += G) a.grad_c[pt * C + c] = qnan;
            continue;
        }

        // the weights of the full sum W, kept or not: the lane's segment in index order, then the butterfly
        const double m = (double)mx;
        double W = 0.0;
        for (int k = k0; k < k1; ++k) W += weight(lr[k], m);
        for (int off = 1; off < G; off <<= 1) W += __shfl_xor(W, off);
        const double rW = 1.0 / W;                            // one division per point: the gradients are sums times 1 / W

        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, accz[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = k0; k < k1; ++k) {
                const int row = ro[k];
                if (row < 0) continue;
                const double w = weight(lr[k], m);
                float g[4];
                load_block(a.gx_rows + (long long)row * D, d0, D, a.vec, g);
                moment1_add(acc, w, g);
                if (a.grad_noise_std) {
                    float z[4];
                    normals4(a.seed, gs, FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
                    noise_add(accz, w, z, g);
                }
            }
            group_sum4(acc, G);
            if (a.grad_noise_std) group_sum4(accz, G);
            if (lane == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < D) {
                        a.grad_x[pt * D + d0 + j] = (float)(acc[j] * rW);
                        if (a.grad_noise_std) a.grad_noise_std[pt * D + d0 + j] = (float)-(accz[j] * rW);
                    }
        }
        if (a.gc_rows)
            for (int blk = 0; blk < ncblk; ++blk) {
                const int c0 = 4 * blk;
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                for (int k = k0; k < k1; ++k) {
                    const int row = ro[k];
                    if (row < 0) continue;
                    float g[4];
                    load_block(a.gc_rows + (long long)row * C, c0, C, a.cvec, g);
                    moment1_add(acc, weight(lr[k], m), g);
                }
                group_sum4(acc, G);
                if (lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < C) a.grad_c[pt * C + c0 + j] = (float)(acc[j] * rW);
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

static bool resample_args_ok(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M,
                             const float* samples, const int32_t* index, const float* mean, const float* var)
{
    if (!y || !lp || B < 0 || D < 1 || K < 1 || K > kMaxDraws || M < 0 || M > kMaxSamples) return false;
    return samples || index || mean || var;
}

static bool keep_args_ok(const float* lp, int64_t B, int32_t K, double min_weight, const int32_t* keep)
{
    return lp && keep && B >= 0 && K >= 1 && K <= kMaxDraws && min_weight >= 0.0 && min_weight < 1.0;
}

static bool grad_reduce_args_ok(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows,
                                const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K,
                                const float* grad_x, const float* grad_c)
{
    if (!lp || !row_of || !gx_rows || !noise_std || !grad_x || B < 0 || D < 1 || K < 1 || K > kMaxDraws) return false;
    if (std_row_stride != 0 && std_row_stride != D) return false;
    if (gc_rows && (C < 1 || !grad_c)) return false;
    return true;
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

extern "C" int ff_weighted_resample(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M,
                                    uint64_t seed, int64_t sample_offset, float* samples, int32_t* index, float* mean,
                                    float* var, void* hip_stream)
{
    if (!resample_args_ok(y, lp, B, D, K, M, samples, index, mean, var)) return FF_ERR_BADARG;
    if (M == 0) { samples = nullptr; index = nullptr; }
    if (B == 0 || !(samples || index || mean || var)) return FF_OK;
    ResampleArgs a;
    a.y = y; a.lp = lp; a.samples = samples; a.index = index; a.mean = mean; a.var = var;
    a.B = B; a.D = D; a.K = K; a.M = M;
    a.seed = seed; a.sample_offset = sample_offset;
    const int G = lanes_per_point(K);
    a.log_g = log2_of(G);
    a.seg = (K + G - 1) / G;
    a.vec = (D & 3) == 0 && (((uintptr_t)y | (uintptr_t)samples) & 15) == 0;
    hipLaunchKernelGGL(weighted_resample_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_observe_keep(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep, void* hip_stream)
{
    if (!keep_args_ok(lp, B, K, min_weight, keep)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    KeepArgs a;
    a.lp = lp; a.keep = keep;
    a.B = B; a.K = K;
    a.min_weight = min_weight;
    const int G = lanes_per_point(K);
    a.log_g = log2_of(G);
    hipLaunchKernelGGL(observe_keep_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_observe_grad_reduce(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows,
                                      const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C,
                                      int32_t K, uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c,
                                      float* grad_noise_std, void* hip_stream)
{
    if (!grad_reduce_args_ok(lp, row_of, gx_rows, gc_rows, noise_std, std_row_stride, B, D, C, K, grad_x, grad_c))
        return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    GradReduceArgs a;
    a.lp = lp; a.row_of = row_of; a.gx_rows = gx_rows; a.gc_rows = gc_rows;
    a.grad_x = grad_x; a.grad_c = gc_rows ? grad_c : nullptr; a.grad_noise_std = grad_noise_std;
    a.B = B; a.D = D; a.C = gc_rows ? C : 0; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset;
    const int G = lanes_per_point(K);
    a.log_g = log2_of(G);
    a.seg = (K + G - 1) / G;
    a.vec = (D & 3) == 0 && ((uintptr_t)gx_rows & 15) == 0;
    a.cvec = gc_rows && (C & 3) == 0 && ((uintptr_t)gc_rows & 15) == 0;
    hipLaunchKernelGGL(observe_grad_reduce_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream,
                       a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twins (CPU tests): the same header, rows and draws in index order ---------------------------------------
extern "C" int ff_observe_keep_host(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep)
{
    if (!keep_args_ok(lp, B, K, min_weight, keep)) return FF_ERR_BADARG;
    for (int64_t r = 0; r < B; ++r) {
        const float* lr = lp + r * K;
        Lse st = lse_empty();
        bool bad = false;
        for (int k = 0; k < K; ++k) {
            bad = bad || weight_bad(lr[k]);
            lse_add(st, (double)lr[k]);
        }
        const bool none = point_degenerate(bad, st.m);
        for (int k = 0; k < K; ++k) keep[r * K + k] = none ? 0 : keep_draw(lr[k], st.m, st.s1, min_weight);
    }
    return FF_OK;
}

extern "C" int ff_observe_grad_reduce_host(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows,
                                           const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C,
                                           int32_t K, uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c,
                                           float* grad_noise_std)
{
    if (!grad_reduce_args_ok(lp, row_of, gx_rows, gc_rows, noise_std, std_row_stride, B, D, C, K, grad_x, grad_c))
        return FF_ERR_BADARG;
    const float qnan = nanf("");
    if (!gc_rows) C = 0;
    const int nblk = (D + 3) / 4, ncblk = (C + 3) / 4;
    for (int64_t r = 0; r < B; ++r) {
        const float* lr = lp + r * K;
        const int32_t* ro = row_of + r * K;
        float mx = -INFINITY;
        bool bad = false;
        for (int k = 0; k < K; ++k) {
            bad = bad || weight_bad(lr[k]);
            mx = lr[k] > mx ? lr[k] : mx;
        }
        if (point_degenerate(bad, (double)mx)) {
            for (int d = 0; d < D; ++d) {
                grad_x[r * D + d] = qnan;
                if (grad_noise_std) grad_noise_std[r * D + d] = qnan;
            }
            for (int c = 0; c < C; ++c) grad_c[r * C + c] = qnan;
            continue;
        }
        const double m = (double)mx;
        double W = 0.0;
        for (int k = 0; k < K; ++k) W += weight(lr[k], m);
        const double rW = 1.0 / W;
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, accz[4] = {0.0, 0.0, 0.0, 0.0};
            float g[4], z[4];
            for (int k = 0; k < K; ++k) {
                if (ro[k] < 0) continue;
                const double w = weight(lr[k], m);
                for (int j = 0; j < 4; ++j) g[j] = d0 + j < D ? gx_rows[(int64_t)ro[k] * D + d0 + j] : 0.f;
                moment1_add(acc, w, g);
                if (grad_noise_std) {
                    normals4(seed, (uint64_t)(sample_offset + r), FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
                    noise_add(accz, w, z, g);
                }
            }
            for (int j = 0; j < 4 && d0 + j < D; ++j) {
                grad_x[r * D + d0 + j] = (float)(acc[j] * rW);
                if (grad_noise_std) grad_noise_std[r * D + d0 + j] = (float)-(accz[j] * rW);
            }
        }
        for (int blk = 0; blk < ncblk; ++blk) {
            const int c0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            float g[4];
            for (int k = 0; k < K; ++k) {
                if (ro[k] < 0) continue;
                for (int j = 0; j < 4; ++j) g[j] = c0 + j < C ? gc_rows[(int64_t)ro[k] * C + c0 + j] : 0.f;
                moment1_add(acc, weight(lr[k], m), g);
            }
            for (int j = 0; j < 4 && c0 + j < C; ++j) grad_c[r * C + c0 + j] = (float)(acc[j] * rW);
        }
    }
    return FF_OK;
}

extern "C" int ff_weighted_resample_host(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M,
                                         uint64_t seed, int64_t sample_offset, float* samples, int32_t* index, float* mean,
                                         float* var)
{
    if (!resample_args_ok(y, lp, B, D, K, M, samples, index, mean, var)) return FF_ERR_BADARG;
    if (M == 0) { samples = nullptr; index = nullptr; }
    const float qnan = nanf("");
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r) {
        const float* lr = lp + r * K;
        const float* yr = y + r * K * D;
        float* sr = samples ? samples + r * M * D : nullptr;
        int32_t* ir = index ? index + r * M : nullptr;
        float mx = -INFINITY;
        bool bad = false;
        for (int k = 0; k < K; ++k) {
            bad = bad || weight_bad(lr[k]);
            mx = lr[k] > mx ? lr[k] : mx;
        }
        if (bad || mx == -INFINITY) {
            for (int64_t i = 0; sr && i < (int64_t)M * D; ++i) sr[i] = qnan;
            for (int m = 0; ir && m < M; ++m) ir[m] = -1;
            for (int d = 0; d < D; ++d) {
                if (mean) mean[r * D + d] = qnan;
                if (var) var[r * D + d] = qnan;
            }
            continue;
        }
        const double m = (double)mx;
        double W = 0.0;
        int last = -1;
        for (int k = 0; k < K; ++k) {
            const double w = weight(lr[k], m);
            W += w;
            if (w > 0.0) last = k;
        }
        const double rW = 1.0 / W;
        for (int m0 = 0; (sr || ir) && m0 < M; m0 += 4) {
            double t[4];
            resample_targets(seed, (uint64_t)(sample_offset + r), (uint32_t)(m0 >> 2), W, t);
            int c[4] = {K, K, K, K};
            double cum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double w = weight(lr[k], m);
                cum += w;
                if (w > 0.0)
                    for (int j = 0; j < 4; ++j)
                        if (cum > t[j] && k < c[j]) c[j] = k;
            }
            for (int j = 0; j < 4 && m0 + j < M; ++j) {
                const int src = c[j] >= K ? last : c[j];
                if (ir) ir[m0 + j] = src;
                for (int d = 0; sr && d < D; ++d) sr[(int64_t)(m0 + j) * D + d] = yr[(int64_t)src * D + d];
            }
        }
        for (int blk = 0; (mean || var) && blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, mu[4];
            float v[4];
            for (int k = 0; k < K; ++k) {
                for (int j = 0; j < 4; ++j) v[j] = d0 + j < D ? yr[(int64_t)k * D + d0 + j] : 0.f;
                moment1_add(acc, weight(lr[k], m), v);
            }
            for (int j = 0; j < 4; ++j) mu[j] = acc[j] * rW;
            for (int j = 0; mean && j < 4 && d0 + j < D; ++j) mean[r * D + d0 + j] = (float)mu[j];
            if (!var) continue;
            for (int j = 0; j < 4; ++j) acc[j] = 0.0;
            for (int k = 0; k < K; ++k) {
                for (int j = 0; j < 4; ++j) v[j] = d0 + j < D ? yr[(int64_t)k * D + d0 + j] : 0.f;
                moment2_add(acc, weight(lr[k], m), v, mu);
            }
            for (int j = 0; j < 4 && d0 + j < D; ++j) var[r * D + d0 + j] = (float)(acc[j] * rW);
        }
    }
    return FF_OK;
}

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
