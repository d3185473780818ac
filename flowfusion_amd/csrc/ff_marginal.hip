// ff_marginal.hip -- the two ends of the K-draw marginal log-density of the symplectic flows (gfx950), around the solve.
//
//   ff_marginal_expand   z0[r K + k] = [(x[r] - shift) / scale | p0(r, k)], cond_out[r K + k] = cond[r]: the K starting
//                        states of data point r, its momenta drawn from the library's counter-based stream under the noise
//                        indices FF_MOMENTUM_NOISE_BASE + k (reference: `q0 = (x - shift) / scale`, `p0 = randn_like(q0)`,
//                        `z0 = cat([q0, p0])`, flowfusion/symplectic.py:204-253, once per draw).  Written in torch ops:
//                        K ff_normal_fill launches, repeat_interleave, cat -- here one pass, write-only beyond x.
//   ff_marginal_reduce   out[r] = logsumexp_k(log N(z1[r K + k]) - log N(p0(r, k))) - log K - log_det and the effective
//                        sample size of the K weights; p0 regenerated from the stream, never stored.  Written in torch
//                        ops: two Normal.log_prob, two sums, logsumexp over [B K, 2 D] temporaries -- here one read of z1.
//
//   ff_marginal_weigh    ff_marginal_reduce that also keeps what the GRADIENT needs: every row's lw in double, and keep[r K + k]
//                        = (normalised weight > 0 and >= min_weight), from the point's merged state once every lane holds it.
//   ff_marginal_grad_reduce  the gradient of the estimate from the kept rows' pull-backs of -z1: sum_k w_k g_q,k / W / scale
//                        for x and sum_k w_k gamma_k / W / conditional_scale for the conditional, the q half of a [n][2 D]
//                        row read in place.  Written in torch ops: a float64 softmax, a slice copy, two weighted sums over
//                        [B K, D] temporaries and two divisions -- here one pass over lw and the kept rows; a row that was
//                        not kept is not read.  A group of observe::lanes_per_point(K) lanes with contiguous segments of
//                        draws, as ff_observe_grad_reduce (whose lane helpers it shares: ff_observe.h).
//
// All are streaming kernels in the style of ff_aux.hip (roofline: HBM): grid-stride loops, 16-byte accesses where the
// pointers and D allow (a scalar body otherwise, same arithmetic in the same order), consecutive lanes on consecutive
// addresses, no LDS, no atomics.  A row is shared by P = lanes_per_row(D) lanes (one block of four dimensions each), a
// data point by a group of G = P min(64 / P, K rounded up to a power of two) lanes; sums cross lanes by xor-butterflies
// inside the group, so a point's result is fixed by (K, D) and its own data: not by the grid, the batch or its place.
// The arithmetic is ff_marginal.h, shared with the host twins below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal.h"
#include "ff_observe.h"

namespace ff {
namespace marginal {

typedef float v4f __attribute__((ext_vector_type(4)));

struct ExpandArgs {
    const float* x;
    const float* shift;
    const float* scale;
    const float* cond;
    float* z0;
    float* cond_out;
    long long rows;                 // B K
    long long stride_r;             // the grid's row stride / K ...
    int stride_k;                   // ... and % K: (r, k) advance without a division per trip
    int D, C, K;
    unsigned long long seed;
    long long sample_offset;
    int log_p;                      // log2 of the lanes per row
    int vec, cvec;                  // the state / the conditional rows move as 16-byte elements
};

__global__ __launch_bounds__(256) void marginal_expand_kernel(const ExpandArgs a)
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
        float* zr = a.z0 + row * 2 * D;
        for (int blk = sub; blk < nblk; blk += P) {
            float p0[4];
            normals4(a.seed, gs, FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
            const int d0 = 4 * blk;
            if (a.vec) {
                const v4f xv = *(const v4f*)(xr + d0);
                *(v4f*)(zr + d0) = v4f{whiten(xv[0], a.shift, a.scale, d0), whiten(xv[1], a.shift, a.scale, d0 + 1),
                                       whiten(xv[2], a.shift, a.scale, d0 + 2), whiten(xv[3], a.shift, a.scale, d0 + 3)};
                *(v4f*)(zr + D + d0) = v4f{p0[0], p0[1], p0[2], p0[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < D) {
                        zr[d0 + j] = whiten(xr[d0 + j], a.shift, a.scale, d0 + j);
                        zr[D + d0 + j] = p0[j];
                    }
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
    const float* z1;
    float* out_logp;
    float* out_ess;
    long long B;
    int D, K;
    unsigned long long seed;
    long long sample_offset;
    double log_det;
    int log_p, log_g;               // log2 of the lanes per row and per data point
    int vec;
};

__global__ __launch_bounds__(256) void marginal_reduce_kernel(const ReduceArgs a)
{
    const int P = 1 << a.log_p, G = 1 << a.log_g, R = G >> a.log_p, D = a.D, K = a.K, nblk = (D + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1)), sub = lane & (P - 1), rowlane = lane >> a.log_p;
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const unsigned long long gs = (unsigned long long)(a.sample_offset + pt);
        Lse st = lse_empty();
        for (int k0 = 0; k0 < K; k0 += R) {
            const int k = k0 + rowlane;
            double t = 0.0;
            if (k < K) {
                const float* zr = a.z1 + (pt * K + k) * 2 * D;
                for (int blk = sub; blk < nblk; blk += P) {
                    const int d0 = 4 * blk;
                    float zq[4] = {0.f, 0.f, 0.f, 0.f}, zp[4] = {0.f, 0.f, 0.f, 0.f}, p0[4];
                    if (a.vec) {
                        const v4f vq = *(const v4f*)(zr + d0), vp = *(const v4f*)(zr + D + d0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { zq[j] = vq[j]; zp[j] = vp[j]; }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (d0 + j < D) { zq[j] = zr[d0 + j]; zp[j] = zr[D + d0 + j]; }
                    }
                    normals4(a.seed, gs, FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                    t += unit_sum(zq, zp, p0, D - d0);
                }
            }
            // the row's units: a butterfly over its P lanes (every lane of the group takes part, k < K or not)
            for (int off = P >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (k < K) lse_add(st, log_weight(t, D));
        }
        // the rows' states: a butterfly over the group's R row lanes
        for (int off = P; off < G; off <<= 1) {
            Lse o;
            o.m = __shfl_xor(st.m, off);
            o.s1 = __shfl_xor(st.s1, off);
            o.s2 = __shfl_xor(st.s2, off);
            st = lse_merge(st, o);
        }
        if (lane == 0) lse_finish(st, K, a.log_det, a.out_logp + pt, a.out_ess ? a.out_ess + pt : nullptr);
    }
}

struct WeighArgs {
    const float* z1;
    float* out_logp;
    float* out_ess;
    double* lw;
    int32_t* keep;
    long long B;
    int D, K;
    unsigned long long seed;
    long long sample_offset;
    double log_det, min_weight;
    int log_p, log_g;               // log2 of the lanes per row and per data point
    int vec;
};

// marginal_reduce_kernel -- its lanes, units, states and butterflies, so out_logp and out_ess are its bits -- that also
// leaves lw and keep.  The first lane of a row stores the row's lw and, after the merge, reads back what it stored itself:
// no other lane's store is ever read, so no fence and no second kernel.
__global__ __launch_bounds__(256) void marginal_weigh_kernel(const WeighArgs a)
{
    const int P = 1 << a.log_p, G = 1 << a.log_g, R = G >> a.log_p, D = a.D, K = a.K, nblk = (D + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1)), sub = lane & (P - 1), rowlane = lane >> a.log_p;
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const unsigned long long gs = (unsigned long long)(a.sample_offset + pt);
        double* lr = a.lw + pt * K;
        int32_t* kr = a.keep + pt * K;
        Lse st = lse_empty();
        for (int k0 = 0; k0 < K; k0 += R) {
            const int k = k0 + rowlane;
            double t = 0.0;
            if (k < K) {
                const float* zr = a.z1 + (pt * K + k) * 2 * D;
                for (int blk = sub; blk < nblk; blk += P) {
                    const int d0 = 4 * blk;
                    float zq[4] = {0.f, 0.f, 0.f, 0.f}, zp[4] = {0.f, 0.f, 0.f, 0.f}, p0[4];
                    if (a.vec) {
                        const v4f vq = *(const v4f*)(zr + d0), vp = *(const v4f*)(zr + D + d0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { zq[j] = vq[j]; zp[j] = vp[j]; }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (d0 + j < D) { zq[j] = zr[d0 + j]; zp[j] = zr[D + d0 + j]; }
                    }
                    normals4(a.seed, gs, FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                    t += unit_sum(zq, zp, p0, D - d0);
                }
            }
            for (int off = P >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (k < K) {
                const double lw = log_weight(t, D);
                lse_add(st, lw);
                if (sub == 0) lr[k] = lw;
            }
        }
        for (int off = P; off < G; off <<= 1) {
            Lse o;
            o.m = __shfl_xor(st.m, off);
            o.s1 = __shfl_xor(st.s1, off);
            o.s2 = __shfl_xor(st.s2, off);
            st = lse_merge(st, o);
        }
        if (lane == 0) lse_finish(st, K, a.log_det, a.out_logp + pt, a.out_ess ? a.out_ess + pt : nullptr);
        // (a + b == b + a in lse_merge: every lane holds the same merged state)
        const bool none = lse_degenerate(st);
        if (sub == 0)
            for (int k = rowlane; k < K; k += R) kr[k] = none ? 0 : keep_weight(lr[k], st.m, st.s1, a.min_weight);
    }
}

struct GradReduceArgs {
    const double* lw;
    const int32_t* row_of;
    const float* gz_rows;
    const float* gc_rows;
    const float* scale;
    const float* cond_scale;
    float* grad_x;
    float* grad_c;
    long long B;
    int D, C, K;
    int log_g;                      // log2 of the lanes per data point
    int seg;                        // draws per lane: lane l holds the draws [l seg, (l + 1) seg) below K
    int vec, cvec;                  // gz_rows / gc_rows move as 16-byte elements
};

__global__ __launch_bounds__(256) void marginal_grad_reduce_kernel(const GradReduceArgs a)
{
    using observe::group_sum4;
    using observe::load_block;
    using observe::moment1_add;
    const int G = 1 << a.log_g, K = a.K, D = a.D, C = a.C, nblk = (D + 3) / 4, ncblk = (C + 3) / 4;
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gtid & (G - 1));
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> a.log_g;
    const int k0 = lane * a.seg < K ? lane * a.seg : K, k1 = k0 + a.seg < K ? k0 + a.seg : K;
    const float qnan = __builtin_nanf("");
    // (the bound is uniform over a group -- and, with G dividing 64, the groups of a wavefront run the same trips or fall
    // out together only at the end: the shuffles below always find their partners)
    for (long long pt = gtid >> a.log_g; pt < a.B; pt += ngroups) {
        const double* lr = a.lw + pt * K;
        const int32_t* ro = a.row_of + pt * K;

        double m = -INFINITY;
        int bad = 0;
        for (int k = k0; k < k1; ++k) max_add(m, bad, lr[k]);
        for (int off = 1; off < G; off <<= 1) {
            const double o = __shfl_xor(m, off);
            m = o > m ? o : m;
            bad |= __shfl_xor(bad, off);
        }
        if (bad || m == -INFINITY) {
            for (int d = lane; d < D; d += G) a.grad_x[pt * D + d] = qnan;
            if (a.gc_rows)
                for (int c = lane; c < C; c += G) a.grad_c[pt * C + c] = qnan;
            continue;
        }

        // the weights of the full sum W, kept or not: the lane's segment in index order, then the butterfly
        // (the lane's first weight is kept: with K <= 64 it is the only one, and no block recomputes its exp)
        const double w_first = k0 < k1 ? lse_factor(lr[k0], m) : 0.0;
        double W = 0.0;
        for (int k = k0; k < k1; ++k) W += k == k0 ? w_first : lse_factor(lr[k], m);
        for (int off = 1; off < G; off <<= 1) W += __shfl_xor(W, off);
        const double rW = 1.0 / W;                            // one division per point: the gradients are sums times 1 / W

        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = k0; k < k1; ++k) {
                const int row = ro[k];
                if (row < 0) continue;
                float g[4];
                load_block(a.gz_rows + (long long)row * 2 * D, d0, D, a.vec, g);         // the q half, in place
                moment1_add(acc, k == k0 ? w_first : lse_factor(lr[k], m), g);
            }
            group_sum4(acc, G);
            if (lane == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < D) a.grad_x[pt * D + d0 + j] = grad_finish(acc[j], rW, a.scale, d0 + j);
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
                    moment1_add(acc, k == k0 ? w_first : lse_factor(lr[k], m), g);
                }
                group_sum4(acc, G);
                if (lane == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c0 + j < C) a.grad_c[pt * C + c0 + j] = grad_finish(acc[j], rW, a.cond_scale, c0 + j);
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

// lanes per data point of the reduction: P lanes per row times the rows side by side, K rounded up to a power of two
static int lanes_per_point(int D, int K)
{
    const int P = lanes_per_row(D);
    int g = P;
    while (g < 64 && g / P < K) g *= 2;
    return g;
}

static bool expand_args_ok(const float* x, const float* cond, int64_t B, int32_t D, int32_t C, int32_t K,
                           const float* z0, const float* cond_out)
{
    if (!x || !z0 || B < 0 || D < 1 || K < 1 || K > kMaxMomenta) return false;
    if (cond && (C < 1 || !cond_out)) return false;
    return true;
}

static bool reduce_args_ok(const float* z1, int64_t B, int32_t D, int32_t K, const float* out_logp)
{
    return z1 && out_logp && B >= 0 && D >= 1 && K >= 1 && K <= kMaxMomenta;
}

static bool weigh_args_ok(const float* z1, int64_t B, int32_t D, int32_t K, double min_weight, const float* out_logp,
                          const double* lw_out, const int32_t* keep)
{
    return reduce_args_ok(z1, B, D, K, out_logp) && lw_out && keep && min_weight >= 0.0 && min_weight < 1.0;
}

static bool grad_reduce_args_ok(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows, int64_t B,
                                int32_t D, int32_t C, int32_t K, const float* grad_x, const float* grad_c)
{
    if (!lw || !row_of || !gz_rows || !grad_x || B < 0 || D < 1 || K < 1 || K > kMaxMomenta) return false;
    if (gc_rows && (C < 1 || !grad_c)) return false;
    return true;
}

} // namespace marginal
} // namespace ff

using namespace ff::marginal;

extern "C" int ff_marginal_expand(const float* x, const float* shift, const float* scale, const float* cond, int64_t B,
                                  int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0,
                                  float* cond_out, void* hip_stream)
{
    if (!expand_args_ok(x, cond, B, D, C, K, z0, cond_out)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    ExpandArgs a;
    a.x = x; a.shift = shift; a.scale = scale; a.cond = cond; a.z0 = z0; a.cond_out = cond ? cond_out : nullptr;
    a.rows = (long long)B * K;
    a.D = D; a.C = cond ? C : 0; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset;
    const int P = lanes_per_row(D);
    a.log_p = log2_of(P);
    a.vec = (D & 3) == 0 && (((uintptr_t)x | (uintptr_t)z0) & 15) == 0;
    a.cvec = cond && (C & 3) == 0 && (((uintptr_t)cond | (uintptr_t)cond_out) & 15) == 0;
    const unsigned grid = stream_grid(a.rows * P);
    const long long nrows = ((long long)grid * 256) >> a.log_p;
    a.stride_r = nrows / K;
    a.stride_k = (int)(nrows % K);
    hipLaunchKernelGGL(marginal_expand_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_marginal_reduce(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                                  double log_det, float* out_logp, float* out_ess, void* hip_stream)
{
    if (!reduce_args_ok(z1, B, D, K, out_logp)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    ReduceArgs a;
    a.z1 = z1; a.out_logp = out_logp; a.out_ess = out_ess;
    a.B = B; a.D = D; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset; a.log_det = log_det;
    const int G = lanes_per_point(D, K);
    a.log_p = log2_of(lanes_per_row(D));
    a.log_g = log2_of(G);
    a.vec = (D & 3) == 0 && ((uintptr_t)z1 & 15) == 0;
    hipLaunchKernelGGL(marginal_reduce_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_marginal_weigh(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                                 double log_det, double min_weight, float* out_logp, float* out_ess, double* lw_out,
                                 int32_t* keep, void* hip_stream)
{
    if (!weigh_args_ok(z1, B, D, K, min_weight, out_logp, lw_out, keep)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    WeighArgs a;
    a.z1 = z1; a.out_logp = out_logp; a.out_ess = out_ess; a.lw = lw_out; a.keep = keep;
    a.B = B; a.D = D; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset; a.log_det = log_det; a.min_weight = min_weight;
    const int G = lanes_per_point(D, K);
    a.log_p = log2_of(lanes_per_row(D));
    a.log_g = log2_of(G);
    a.vec = (D & 3) == 0 && ((uintptr_t)z1 & 15) == 0;
    hipLaunchKernelGGL(marginal_weigh_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_marginal_grad_reduce(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                                       const float* scale, const float* cond_scale, int64_t B, int32_t D, int32_t C, int32_t K,
                                       float* grad_x, float* grad_c, void* hip_stream)
{
    if (!grad_reduce_args_ok(lw, row_of, gz_rows, gc_rows, B, D, C, K, grad_x, grad_c)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    GradReduceArgs a;
    a.lw = lw; a.row_of = row_of; a.gz_rows = gz_rows; a.gc_rows = gc_rows;
    a.scale = scale; a.cond_scale = cond_scale;
    a.grad_x = grad_x; a.grad_c = gc_rows ? grad_c : nullptr;
    a.B = B; a.D = D; a.C = gc_rows ? C : 0; a.K = K;
    const int G = ff::observe::lanes_per_point(K);
    a.log_g = log2_of(G);
    a.seg = (K + G - 1) / G;
    a.vec = (D & 3) == 0 && ((uintptr_t)gz_rows & 15) == 0;
    a.cvec = gc_rows && (C & 3) == 0 && ((uintptr_t)gc_rows & 15) == 0;
    hipLaunchKernelGGL(marginal_grad_reduce_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twins (CPU tests): the same header, rows and units in index order ----------------------------------------
extern "C" int ff_marginal_expand_host(const float* x, const float* shift, const float* scale, const float* cond, int64_t B,
                                       int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0,
                                       float* cond_out)
{
    if (!expand_args_ok(x, cond, B, D, C, K, z0, cond_out)) return FF_ERR_BADARG;
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r)
        for (int k = 0; k < K; ++k) {
            const int64_t row = r * K + k;
            float* zr = z0 + row * 2 * D;
            for (int d = 0; d < D; ++d) zr[d] = whiten(x[r * D + d], shift, scale, d);
            for (int blk = 0; blk < nblk; ++blk) {
                float p0[4];
                normals4(seed, (uint64_t)(sample_offset + r), FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                for (int j = 0; j < 4 && 4 * blk + j < D; ++j) zr[D + 4 * blk + j] = p0[j];
            }
            if (cond)
                for (int c = 0; c < C; ++c) cond_out[row * C + c] = cond[r * C + c];
        }
    return FF_OK;
}

extern "C" int ff_marginal_reduce_host(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed,
                                       int64_t sample_offset, double log_det, float* out_logp, float* out_ess)
{
    if (!reduce_args_ok(z1, B, D, K, out_logp)) return FF_ERR_BADARG;
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r) {
        Lse st = lse_empty();
        for (int k = 0; k < K; ++k) {
            const float* zr = z1 + (r * K + k) * 2 * D;
            double t = 0.0;
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = 4 * blk;
                float zq[4] = {0.f, 0.f, 0.f, 0.f}, zp[4] = {0.f, 0.f, 0.f, 0.f}, p0[4];
                for (int j = 0; j < 4 && d0 + j < D; ++j) { zq[j] = zr[d0 + j]; zp[j] = zr[D + d0 + j]; }
                normals4(seed, (uint64_t)(sample_offset + r), FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                t += unit_sum(zq, zp, p0, D - d0);
            }
            lse_add(st, log_weight(t, D));
        }
        lse_finish(st, K, log_det, out_logp + r, out_ess ? out_ess + r : nullptr);
    }
    return FF_OK;
}

extern "C" int ff_marginal_weigh_host(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                                      double log_det, double min_weight, float* out_logp, float* out_ess, double* lw_out,
                                      int32_t* keep)
{
    if (!weigh_args_ok(z1, B, D, K, min_weight, out_logp, lw_out, keep)) return FF_ERR_BADARG;
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r) {
        Lse st = lse_empty();
        for (int k = 0; k < K; ++k) {
            const float* zr = z1 + (r * K + k) * 2 * D;
            double t = 0.0;
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = 4 * blk;
                float zq[4] = {0.f, 0.f, 0.f, 0.f}, zp[4] = {0.f, 0.f, 0.f, 0.f}, p0[4];
                for (int j = 0; j < 4 && d0 + j < D; ++j) { zq[j] = zr[d0 + j]; zp[j] = zr[D + d0 + j]; }
                normals4(seed, (uint64_t)(sample_offset + r), FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                t += unit_sum(zq, zp, p0, D - d0);
            }
            lw_out[r * K + k] = log_weight(t, D);
            lse_add(st, lw_out[r * K + k]);
        }
        lse_finish(st, K, log_det, out_logp + r, out_ess ? out_ess + r : nullptr);
        const bool none = lse_degenerate(st);
        for (int k = 0; k < K; ++k) keep[r * K + k] = none ? 0 : keep_weight(lw_out[r * K + k], st.m, st.s1, min_weight);
    }
    return FF_OK;
}

// (the device's order of additions, lane by lane: segment sums in index order, then the butterfly's tree -- given the same
// lw the two differ only where libm's exp and the device's differ in the last bit of a double)
extern "C" int ff_marginal_grad_reduce_host(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                                            const float* scale, const float* cond_scale, int64_t B, int32_t D, int32_t C,
                                            int32_t K, float* grad_x, float* grad_c)
{
    if (!grad_reduce_args_ok(lw, row_of, gz_rows, gc_rows, B, D, C, K, grad_x, grad_c)) return FF_ERR_BADARG;
    using ff::observe::moment1_add;
    const float qnan = nanf("");
    if (!gc_rows) C = 0;
    const int G = ff::observe::lanes_per_point(K), seg = (K + G - 1) / G;
    // the q half of a gz row (stride 2 D) or a gc row (stride C): cols columns summed into out[r][..] over unit[..]
    const auto weighted = [&](const double* lr, const int32_t* ro, double m, double rW, const float* rows, int stride, int cols,
                              const float* unit, float* out) {
        for (int c0 = 0; c0 < cols; c0 += 4) {
            double part[64][4];
            for (int l = 0; l < G; ++l) {
                for (int j = 0; j < 4; ++j) part[l][j] = 0.0;
                for (int k = l * seg; k < (l + 1) * seg && k < K; ++k) {
                    if (ro[k] < 0) continue;
                    float g[4];
                    for (int j = 0; j < 4; ++j) g[j] = c0 + j < cols ? rows[(int64_t)ro[k] * stride + c0 + j] : 0.f;
                    moment1_add(part[l], lse_factor(lr[k], m), g);
                }
            }
            for (int off = 1; off < G; off <<= 1)
                for (int l = 0; l < G; l += 2 * off)
                    for (int j = 0; j < 4; ++j) part[l][j] += part[l + off][j];
            for (int j = 0; j < 4 && c0 + j < cols; ++j) out[c0 + j] = grad_finish(part[0][j], rW, unit, c0 + j);
        }
    };
    for (int64_t r = 0; r < B; ++r) {
        const double* lr = lw + r * K;
        const int32_t* ro = row_of + r * K;
        double m = -INFINITY;
        int bad = 0;
        for (int k = 0; k < K; ++k) max_add(m, bad, lr[k]);
        if (bad || m == -INFINITY) {
            for (int d = 0; d < D; ++d) grad_x[r * D + d] = qnan;
            for (int c = 0; c < C; ++c) grad_c[r * C + c] = qnan;
            continue;
        }
        double part[64];
        for (int l = 0; l < G; ++l) {
            part[l] = 0.0;
            for (int k = l * seg; k < (l + 1) * seg && k < K; ++k) part[l] += lse_factor(lr[k], m);
        }
        for (int off = 1; off < G; off <<= 1)
            for (int l = 0; l < G; l += 2 * off) part[l] += part[l + off];
        const double rW = 1.0 / part[0];
        weighted(lr, ro, m, rW, gz_rows, 2 * D, D, scale, grad_x + r * D);
        if (C) weighted(lr, ro, m, rW, gc_rows, C, C, cond_scale, grad_c + r * C);
    }
    return FF_OK;
}
