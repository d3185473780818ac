// ff_marginal_observe.hip -- the two ends of the K-draw marginal log-density of NOISY observations under a symplectic flow
// (gfx950), around the leapfrog launches and ff_marginal_weigh.
//
//   ff_marginal_observe_expand       z0[r K + k] = [((x[r] - noise_std[r] z(r, k)) - shift) / scale | p0(r, k)],
//                        cond_out[r K + k] = cond[r]: the K joint draws of observation r, its noise under the noise indices
//                        FF_OBS_NOISE_BASE + k and its momenta under FF_MOMENTUM_NOISE_BASE + k, both keyed by the global
//                        row.  Written with the existing kernels: ff_observe_expand -> ff_marginal_expand(K = 1), which keys
//                        every momentum by the EXPANDED row -- here one pass, write-only beyond x, noise_std and cond.  The
//                        q half is ff_observe_expand's row through ff_marginal_expand's formula, the p half and cond_out are
//                        ff_marginal_expand(x, K)'s: bit for bit.
//   ff_marginal_observe_grad_reduce  ff_marginal_grad_reduce -- its lanes, segments, order of additions and butterfly: grad_x and
//                        grad_c are its bits -- that in the same pass forms the gradient with respect to noise_std,
//                        -(sum_k w_k z_k g_q,k / W) / scale, with z regenerated from the stream; a row that was not kept is
//                        not read.
//
// Streaming kernels in the style of ff_marginal.hip (roofline: HBM): grid-stride loops, 16-byte accesses where the pointers
// and D allow (a scalar body otherwise, same arithmetic in the same order), consecutive lanes on consecutive addresses, no
// LDS, no atomics.  A row of the expansion is shared by P = lanes_per_row(D) lanes (one block of four dimensions each), a
// data point of the reduction by a group of observe::lanes_per_point(K) lanes with contiguous segments of draws; sums cross
// lanes by xor-butterflies inside the group, so a point's result is fixed by (K, D) and its own data: not by the grid, the
// batch or its place.  The arithmetic is ff_marginal_observe.h (over ff_marginal.h and ff_observe.h), shared with the host
// twins below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal_observe.h"

namespace ff {
namespace marginal_observe {

typedef float v4f __attribute__((ext_vector_type(4)));

struct ExpandArgs {
    const float* x;
    const float* noise_std;
    const float* shift;
    const float* scale;
    const float* cond;
    float* z0;
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

__global__ __launch_bounds__(256) void marginal_observe_expand_kernel(const ExpandArgs a)
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
        float* zr = a.z0 + row * 2 * D;
        for (int blk = sub; blk < nblk; blk += P) {
            float z[4], p0[4];
            normals4(a.seed, gs, FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
            normals4(a.seed, gs, FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
            const int d0 = 4 * blk;
            if (a.vec) {
                const v4f xv = *(const v4f*)(xr + d0), sv = *(const v4f*)(sr + d0);
                *(v4f*)(zr + d0) = v4f{start_q(xv[0], sv[0], z[0], a.shift, a.scale, d0),
                                       start_q(xv[1], sv[1], z[1], a.shift, a.scale, d0 + 1),
                                       start_q(xv[2], sv[2], z[2], a.shift, a.scale, d0 + 2),
                                       start_q(xv[3], sv[3], z[3], a.shift, a.scale, d0 + 3)};
                *(v4f*)(zr + D + d0) = v4f{p0[0], p0[1], p0[2], p0[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < D) {
                        zr[d0 + j] = start_q(xr[d0 + j], sr[d0 + j], z[j], a.shift, a.scale, d0 + j);
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

struct GradReduceArgs {
    const double* lw;
    const int32_t* row_of;
    const float* gz_rows;
    const float* gc_rows;
    const float* scale;
    const float* cond_scale;
    float* grad_x;
    float* grad_c;
    float* grad_noise_std;
    long long B;
    int D, C, K;
    unsigned long long seed;
    long long sample_offset;
    int log_g;                      // log2 of the lanes per data point
    int seg;                        // draws per lane: lane l holds the draws [l seg, (l + 1) seg) below K
    int vec, cvec;                  // gz_rows / gc_rows move as 16-byte elements
};

// marginal_grad_reduce_kernel (ff_marginal.hip) line by line for grad_x and grad_c; accz beside acc takes the same weight and
// the same row, times the regenerated noise.
__global__ __launch_bounds__(256) void marginal_observe_grad_reduce_kernel(const GradReduceArgs a)
{
    using marginal::grad_finish;
    using marginal::lse_factor;
    using marginal::max_add;
    using observe::group_sum4;
    using observe::load_block;
    using observe::moment1_add;
    using observe::noise_add;
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
        const unsigned long long gs = (unsigned long long)(a.sample_offset + pt);

        double m = -INFINITY;
        int bad = 0;
        for (int k = k0; k < k1; ++k) max_add(m, bad, lr[k]);
        for (int off = 1; off < G; off <<= 1) {
            const double o = __shfl_xor(m, off);
            m = o > m ? o : m;
            bad |= __shfl_xor(bad, off);
        }
        if (bad || m == -INFINITY) {
            for (int d = lane; d < D; d += G) {
                a.grad_x[pt * D + d] = qnan;
                if (a.grad_noise_std) a.grad_noise_std[pt * D + d] = qnan;
            }
            if (a.gc_rows)
                for (int c = lane; c < C; c += G) a.grad_c[pt * C + c] = qnan;
            continue;
        }

        // the weights of the full sum W, kept or not: the lane's segment in index order, then the butterfly
        const double w_first = k0 < k1 ? lse_factor(lr[k0], m) : 0.0;
        double W = 0.0;
        for (int k = k0; k < k1; ++k) W += k == k0 ? w_first : lse_factor(lr[k], m);
        for (int off = 1; off < G; off <<= 1) W += __shfl_xor(W, off);
        const double rW = 1.0 / W;                            // one division per point: the gradients are sums times 1 / W

        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = 4 * blk;
            double acc[4] = {0.0, 0.0, 0.0, 0.0}, accz[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = k0; k < k1; ++k) {
                const int row = ro[k];
                if (row < 0) continue;
                const double w = k == k0 ? w_first : lse_factor(lr[k], m);
                float g[4];
                load_block(a.gz_rows + (long long)row * 2 * D, d0, D, a.vec, g);         // the q half, in place
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
                        a.grad_x[pt * D + d0 + j] = grad_finish(acc[j], rW, a.scale, d0 + j);
                        if (a.grad_noise_std) a.grad_noise_std[pt * D + d0 + j] = noise_grad_finish(accz[j], rW, a.scale, d0 + j);
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

} // namespace marginal_observe
} // namespace ff

using namespace ff::marginal_observe;

extern "C" int ff_marginal_observe_expand(const float* x, const float* noise_std, int32_t std_row_stride, const float* shift,
                                          const float* scale, const float* cond, int64_t B, int32_t D, int32_t C, int32_t K,
                                          uint64_t seed, int64_t sample_offset, float* z0, float* cond_out, void* hip_stream)
{
    if (!expand_args_ok(x, noise_std, std_row_stride, cond, B, D, C, K, z0, cond_out)) return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    ExpandArgs a;
    a.x = x; a.noise_std = noise_std; a.shift = shift; a.scale = scale; a.cond = cond;
    a.z0 = z0; a.cond_out = cond ? cond_out : nullptr;
    a.rows = (long long)B * K;
    a.std_stride = std_row_stride;
    a.D = D; a.C = cond ? C : 0; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset;
    const int P = ff::marginal::lanes_per_row(D);
    a.log_p = log2_of(P);
    a.vec = (D & 3) == 0 && (((uintptr_t)x | (uintptr_t)noise_std | (uintptr_t)z0) & 15) == 0;
    a.cvec = cond && (C & 3) == 0 && (((uintptr_t)cond | (uintptr_t)cond_out) & 15) == 0;
    const unsigned grid = stream_grid(a.rows * P);
    const long long nrows = ((long long)grid * 256) >> a.log_p;
    a.stride_r = nrows / K;
    a.stride_k = (int)(nrows % K);
    hipLaunchKernelGGL(marginal_observe_expand_kernel, dim3(grid), dim3(256), 0, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

extern "C" int ff_marginal_observe_grad_reduce(const double* lw, const int32_t* row_of, const float* gz_rows,
                                               const float* gc_rows, const float* scale, const float* cond_scale,
                                               const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C,
                                               int32_t K, uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c,
                                               float* grad_noise_std, void* hip_stream)
{
    if (!grad_reduce_args_ok(lw, row_of, gz_rows, gc_rows, noise_std, std_row_stride, B, D, C, K, grad_x, grad_c))
        return FF_ERR_BADARG;
    if (B == 0) return FF_OK;
    GradReduceArgs a;
    a.lw = lw; a.row_of = row_of; a.gz_rows = gz_rows; a.gc_rows = gc_rows;
    a.scale = scale; a.cond_scale = cond_scale;
    a.grad_x = grad_x; a.grad_c = gc_rows ? grad_c : nullptr; a.grad_noise_std = grad_noise_std;
    a.B = B; a.D = D; a.C = gc_rows ? C : 0; a.K = K;
    a.seed = seed; a.sample_offset = sample_offset;
    const int G = ff::observe::lanes_per_point(K);
    a.log_g = log2_of(G);
    a.seg = (K + G - 1) / G;
    a.vec = (D & 3) == 0 && ((uintptr_t)gz_rows & 15) == 0;
    a.cvec = gc_rows && (C & 3) == 0 && ((uintptr_t)gc_rows & 15) == 0;
    hipLaunchKernelGGL(marginal_observe_grad_reduce_kernel, dim3(stream_grid((long long)B * G)), dim3(256), 0,
                       (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? FF_OK : FF_ERR_HIP;
}

// ---- the host twins (CPU tests): the same headers, rows and blocks in index order ---------------------------------------
extern "C" int ff_marginal_observe_expand_host(const float* x, const float* noise_std, int32_t std_row_stride,
                                               const float* shift, const float* scale, const float* cond, int64_t B, int32_t D,
                                               int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0,
                                               float* cond_out)
{
    if (!expand_args_ok(x, noise_std, std_row_stride, cond, B, D, C, K, z0, cond_out)) return FF_ERR_BADARG;
    const int nblk = (D + 3) / 4;
    for (int64_t r = 0; r < B; ++r)
        for (int k = 0; k < K; ++k) {
            const int64_t row = r * K + k;
            float* zr = z0 + row * 2 * D;
            for (int blk = 0; blk < nblk; ++blk) {
                float z[4], p0[4];
                normals4(seed, (uint64_t)(sample_offset + r), FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
                normals4(seed, (uint64_t)(sample_offset + r), FF_MOMENTUM_NOISE_BASE + (uint32_t)k, (uint32_t)blk, p0);
                for (int j = 0; j < 4 && 4 * blk + j < D; ++j) {
                    const int d = 4 * blk + j;
                    zr[d] = start_q(x[r * D + d], noise_std[r * std_row_stride + d], z[j], shift, scale, d);
                    zr[D + d] = p0[j];
                }
            }
            if (cond)
                for (int c = 0; c < C; ++c) cond_out[row * C + c] = cond[r * C + c];
        }
    return FF_OK;
}

// (the device's order of additions, lane by lane: segment sums in index order, then the butterfly's tree -- as
// ff_marginal_grad_reduce_host, so given the same lw grad_x and grad_c are that twin's bits)
extern "C" int ff_marginal_observe_grad_reduce_host(const double* lw, const int32_t* row_of, const float* gz_rows,
                                                    const float* gc_rows, const float* scale, const float* cond_scale,
                                                    const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D,
                                                    int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* grad_x,
                                                    float* grad_c, float* grad_noise_std)
{
    if (!grad_reduce_args_ok(lw, row_of, gz_rows, gc_rows, noise_std, std_row_stride, B, D, C, K, grad_x, grad_c))
        return FF_ERR_BADARG;
    using ff::marginal::grad_finish;
    using ff::marginal::lse_factor;
    using ff::marginal::max_add;
    using ff::observe::moment1_add;
    using ff::observe::noise_add;
    const float qnan = nanf("");
    if (!gc_rows) C = 0;
    const int G = ff::observe::lanes_per_point(K), seg = (K + G - 1) / G;
    // the q half of a gz row (stride 2 D) or a gc row (stride C): cols columns summed into out[..] over unit[..]; with
    // zout, the same rows times the noise of global row gs into zout[..]
    const auto weighted = [&](const double* lr, const int32_t* ro, double m, double rW, const float* rows, int stride, int cols,
                              const float* unit, float* out, uint64_t gs, float* zout) {
        for (int c0 = 0; c0 < cols; c0 += 4) {
            double part[64][4], partz[64][4];
            for (int l = 0; l < G; ++l) {
                for (int j = 0; j < 4; ++j) part[l][j] = partz[l][j] = 0.0;
                for (int k = l * seg; k < (l + 1) * seg && k < K; ++k) {
                    if (ro[k] < 0) continue;
                    const double w = lse_factor(lr[k], m);
                    float g[4];
                    for (int j = 0; j < 4; ++j) g[j] = c0 + j < cols ? rows[(int64_t)ro[k] * stride + c0 + j] : 0.f;
                    moment1_add(part[l], w, g);
                    if (zout) {
                        float z[4];
                        normals4(seed, gs, FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)(c0 >> 2), z);
                        noise_add(partz[l], w, z, g);
                    }
                }
            }
            for (int off = 1; off < G; off <<= 1)
                for (int l = 0; l < G; l += 2 * off)
                    for (int j = 0; j < 4; ++j) {
                        part[l][j] += part[l + off][j];
                        partz[l][j] += partz[l + off][j];
                    }
            for (int j = 0; j < 4 && c0 + j < cols; ++j) {
                out[c0 + j] = grad_finish(part[0][j], rW, unit, c0 + j);
                if (zout) zout[c0 + j] = noise_grad_finish(partz[0][j], rW, unit, c0 + j);
            }
        }
    };
    for (int64_t r = 0; r < B; ++r) {
        const double* lr = lw + r * K;
        const int32_t* ro = row_of + r * K;
        double m = -INFINITY;
        int bad = 0;
        for (int k = 0; k < K; ++k) max_add(m, bad, lr[k]);
        if (bad || m == -INFINITY) {
            for (int d = 0; d < D; ++d) {
                grad_x[r * D + d] = qnan;
                if (grad_noise_std) grad_noise_std[r * D + d] = qnan;
            }
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
        weighted(lr, ro, m, rW, gz_rows, 2 * D, D, scale, grad_x + r * D, (uint64_t)(sample_offset + r),
                 grad_noise_std ? grad_noise_std + r * D : nullptr);
        if (C) weighted(lr, ro, m, rW, gc_rows, C, C, cond_scale, grad_c + r * C, 0, nullptr);
    }
    return FF_OK;
}
