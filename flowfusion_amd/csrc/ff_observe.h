// ff_observe.h -- the arithmetic of the K-draw log-density of noisy observations, shared by the gfx950 kernels
// (ff_observe.hip: observe_expand_kernel / logmeanexp_kernel / weighted_resample_kernel / observe_keep_kernel /
// observe_grad_reduce_kernel) and the host entry points the CPU tests call (ff_observe_expand_host / ff_logmeanexp_host /
// ff_weighted_resample_host / ff_observe_keep_host / ff_observe_grad_reduce_host, compiled from the host pass of the same
// file).
//
// An observation xhat = x + n, n ~ N(0, diag(sigma^2)) with sigma known per object and dimension, has the convolved
// density p_obs(xhat | sigma) = E_{z ~ N(0, I)}[p(xhat - sigma z)]; the extension estimates it from K draws per point,
// combined by log-sum-exp:
//     y_k = xhat - sigma z_k,       log p_obs = logsumexp_k log p(y_k) - log K
// The K draws of point r are the normals of the library's counter-based stream (ff_philox.h) for global row
// sample_offset + r under the noise indices FF_OBS_NOISE_BASE + k.  Between the two ends runs whatever log-density the
// caller has: nothing here knows the model.
//
// The perturbation is two fp32 roundings (the product, then the difference: never a fused multiply-add), so the torch
// composition `x - noise_std * z` of ff_normal_fill's normals gives the same bits.  The log-sum-exp and the effective
// sample size run in double on the running state of ff_marginal.h (Lse: the semantics of torch.logsumexp in float64 for
// NaN and infinities) and are rounded to fp32 once; the device merges the states of a point's lanes by a butterfly, the
// host adds in index order: both are fixed by K alone, the two agree to double rounding.
#pragma once
#include <math.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal.h"

namespace ff {
namespace observe {

using marginal::Lse;
using marginal::lse_add;
using marginal::lse_empty;
using marginal::lse_merge;
using marginal::normals4;

constexpr int kMaxDraws = FF_MAX_OBS_DRAWS;             // FF_OBS_NOISE_BASE + k stays below the Hutchinson probes' range

// y = x - s z: the product rounded, then the difference rounded
FF_HD float perturb(float x, float s, float z)
{
#pragma clang fp contract(off)
    const float p = s * z;
    return x - p;
}

// out = m + log s1 - log K;  ess = s1^2 / s2 (NaN where no draw has weight: 0 / 0).  One draw is its own mean: `only`,
// the value as it was read, goes out bit for bit.
FF_HD void lme_finish(const Lse& a, int K, float only, float* out, float* ess)
{
#pragma clang fp contract(off)
    *out = K == 1 ? only : (float)(a.m + log(a.s1) - log((double)K));
    if (ess) *ess = (float)(a.s1 * a.s1 / a.s2);
}

// lanes that share one data point in the reduction: K rounded up to a power of two, at most a wavefront
FF_HD int lanes_per_point(int K)
{
    int g = 1;
    while (g < K && g < 64) g *= 2;
    return g;
}

// ---- the posterior of a point from its K weighted particles (ff_weighted_resample) ------------------------------------
// The K rows y_k with weights w_k = exp(lp_k - max lp) are a self-normalised importance sample of p(x | xhat, sigma):
// M multinomial draws (index m: the smallest k of positive weight whose running sum exceeds u_m W) and the weighted mean
// and variance, all sums in double.  The uniforms are integer arithmetic on the raw words of the stream: the same bits
// on host and device.
constexpr int kMaxSamples = FF_MAX_OBS_SAMPLES;

// a point without a posterior: a NaN or +inf among its log-weights (not (v < inf)), or none above -inf (max = -inf, W = 0)
FF_HD bool weight_bad(float lp) { return !(lp < INFINITY); }

// w = exp(lp - max) in double: 1 for the maximum itself, 0 for -inf
FF_HD double weight(float lp, double mx) { return exp((double)lp - mx); }

// u in [0, 1) from a raw word: its upper 24 bits
FF_HD double resample_uniform(uint32_t word) { return (double)(word >> 8) * 0x1p-24; }

// the four targets u_m W of the samples m = 4 q .. 4 q + 3 of global row gs
FF_HD void resample_targets(uint64_t seed, uint64_t gs, uint32_t q, double W, double (&t)[4])
{
#pragma clang fp contract(off)
    uint32_t w[4];
    marginal::words4(seed, gs, FF_OBS_RESAMPLE_NOISE_INDEX, q, w);
    for (int j = 0; j < 4; ++j) t[j] = resample_uniform(w[j]) * W;
}

// one draw's share of a block of four dimensions: acc += w v (first moment), acc += w (v - mean)^2 (second, about the
// double mean: never negative)
FF_HD void moment1_add(double (&acc)[4], double w, const float (&v)[4])
{
#pragma clang fp contract(off)
    for (int j = 0; j < 4; ++j) acc[j] += w * (double)v[j];
}
FF_HD void moment2_add(double (&acc)[4], double w, const float (&v)[4], const double (&mean)[4])
{
#pragma clang fp contract(off)
    for (int j = 0; j < 4; ++j) {
        const double d = (double)v[j] - mean[j];
        acc[j] += w * (d * d);
    }
}

// ---- the gradient of the K-draw log-density (ff_observe_keep / ff_observe_grad_reduce) ------------------------------------
// L = logsumexp_k lp_k - log K has dL / d lp_k = wn_k = w_k / W, the normalised weight of draw k, so with y_k = xhat -
// sigma z_k the gradients of L are the wn-weighted sums of the rows' own gradients g_k = grad_y lp_k (and grad_c lp_k),
// and dL / d sigma_d = -sum_k wn_k z_kd g_kd.  A draw whose normalised weight is 0, or below the caller's min_weight, adds
// nothing (at most min_weight |g_k|): it is not KEPT, and its gradient row is never computed or read.

// a point without a gradient: what has no posterior (weight_bad, or no draw above -inf)
FF_HD bool point_degenerate(bool bad, double mx) { return bad || mx == -INFINITY; }

// draw k of a point with maximum mx and weight sum W is kept iff its normalised weight is positive and >= min_weight
FF_HD int32_t keep_draw(float lp, double mx, double W, double min_weight)
{
#pragma clang fp contract(off)
    const double wn = weight(lp, mx) / W;
    return wn > 0.0 && wn >= min_weight ? 1 : 0;
}

// one draw's share of a block of four dimensions of dL / d sigma, before the sign: acc += w (z g) -- the product of two
// floats is exact in double
FF_HD void noise_add(double (&acc)[4], double w, const float (&z)[4], const float (&g)[4])
{
#pragma clang fp contract(off)
    for (int j = 0; j < 4; ++j) acc[j] += w * ((double)z[j] * (double)g[j]);
}

#if defined(__HIPCC__)
// ---- what the lane groups of the weighted sums share on the device (ff_observe.hip; ff_marginal.hip: marginal_grad_reduce_kernel)
// the (up to four) dimensions 4 blk .. of one row, zero beyond D
__device__ __forceinline__ void load_block(const float* row, int d0, int D, int vec, float (&v)[4])
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    if (vec) {
        const v4f t = *(const v4f*)(row + d0);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d0 + j < D ? row[d0 + j] : 0.f;
    }
}

__device__ __forceinline__ void group_sum4(double (&acc)[4], int G)
{
    for (int off = 1; off < G; off <<= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += __shfl_xor(acc[j], off);       // (a + b == b + a: every lane holds the same bits)
}
#endif

} // namespace observe
} // namespace ff
