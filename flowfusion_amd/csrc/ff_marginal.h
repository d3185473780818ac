// ff_marginal.h -- the arithmetic of the K-draw marginal log-density of the symplectic flows, shared by the gfx950
// kernels (ff_marginal.hip: marginal_expand_kernel / marginal_reduce_kernel) and the host entry points the CPU tests
// call (ff_marginal_expand_host / ff_marginal_reduce_host, compiled from the host pass of the same file) -- and, further
// down, of its gradient (marginal_weigh_kernel / marginal_grad_reduce_kernel and their _host twins).
//
// What is restated here, and from where: SymplecticFlowModel.log_prob, flowfusion/symplectic.py:204-253, draws ONE
// momentum p0 per data point and returns log N(z1) - log N(p0) - sum log scale.  The flow preserves volume in [q | p],
// so that is a one-draw importance estimate of the marginal p(q0) = E_{p0 ~ N}[N(Phi(q0, p0)) / N(p0)]; the extension
// averages K draws per point, combined by log-sum-exp:
//     lw_k = -1/2 (sum_{2D} z1_k^2 - sum_D p0_k^2) - (D / 2) log 2 pi,      log p = logsumexp_k lw_k - log K - log_det
// The K momenta of data point r are the normals of the library's counter-based stream (ff_philox.h) for global row
// sample_offset + r under the noise indices FF_MOMENTUM_NOISE_BASE + k: the reduction regenerates them instead of
// reading them back.
//
// Sums of squares, the log-sum-exp and the effective sample size run in double and are rounded to fp32 once.  One unit
// of work is a block of four dimensions of one row, (z1 q-block, z1 p-block, p0 block) -> one double; the device adds a
// row's units by a butterfly over the lanes that hold them and merges the rows' log-sum-exp states by another, the host
// adds and merges them in index order: both are fixed by (K, D) alone, the two agree to double rounding.
// Transcendentals of the normals come from libm on the host and from the hardware on the GPU (as tests/_philox.py and
// ff_normal_fill: they agree to 2e-6, not bit for bit); on each side expand and reduce use the same ones.
#pragma once
#include <math.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_layout.h"
#if defined(__HIPCC__)
#include "ff_philox.h"
#endif

namespace ff {
namespace marginal {

constexpr int kMaxMomenta = 4096;                       // FF_MOMENTUM_NOISE_BASE + k stays below the trace-probe range
constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(2 pi) / 2

// the four normals z(seed, global row gs, noise index, 4 blk .. 4 blk + 3) of the stream: on the device the code of
// ff_normal_fill, bit for bit; on the host the same words through libm
FF_HD void normals4(uint64_t seed, uint64_t gs, uint32_t noise_index, uint32_t blk, float (&z)[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t c[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), noise_index, blk};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    box_muller(c[0], c[1], z[0], z[1]);
    box_muller(c[2], c[3], z[2], z[3]);
#else
    uint32_t c[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), noise_index, blk};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    for (int h = 0; h < 2; ++h) {
        const float u1 = fmaf((float)(c[2 * h] >> 8), 0x1p-24f, 0x1p-25f);      // (0, 1]
        const float u2 = (float)(c[2 * h + 1] >> 8) * 0x1p-24f;                 // [0, 1): a turn
        const double rad = (double)(float)sqrt(-2.0 * log((double)u1));
        const double ang = 6.283185307179586476925 * (double)u2;
        z[2 * h] = (float)(rad * cos(ang));
        z[2 * h + 1] = (float)(rad * sin(ang));
    }
#endif
}

// the four raw words of the same block of the stream, for consumers that want uniforms, not normals: integer arithmetic
// on both sides, so host and device agree bit for bit
FF_HD void words4(uint64_t seed, uint64_t gs, uint32_t noise_index, uint32_t blk, uint32_t (&w)[4])
{
    w[0] = (uint32_t)gs; w[1] = (uint32_t)(gs >> 32); w[2] = noise_index; w[3] = blk;
#if defined(__HIP_DEVICE_COMPILE__)
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
#else
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * w[0], p1 = (uint64_t)0xCD9E8D57u * w[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ w[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ w[3] ^ k1;
        w[0] = n0; w[1] = (uint32_t)p1; w[2] = n2; w[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
#endif
}

// q0 = (x - shift) / scale as torch computes it: one fp32 subtraction, one correctly rounded fp32 division
FF_HD float whiten(float x, const float* shift, const float* scale, int d)
{
    float v = x;
    if (shift) v = v - shift[d];
    if (scale) v = v / scale[d];
    return v;
}

// one unit: sum over the (up to four) dimensions 4 blk + j < D of  zq^2 + zp^2 - p0^2  in double, in index order
FF_HD double unit_sum(const float (&zq)[4], const float (&zp)[4], const float (&p0)[4], int n)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int j = 0; j < 4; ++j)
        if (j < n) {
            s += (double)zq[j] * (double)zq[j];
            s += (double)zp[j] * (double)zp[j];
            s -= (double)p0[j] * (double)p0[j];
        }
    return s;
}

FF_HD double log_weight(double row_sum, int D) { return -0.5 * row_sum - (double)D * kHalfLog2Pi; }

// running log-sum-exp of the log-weights seen so far: m = their maximum, s1 = sum exp(lw - m), s2 = sum exp(lw - m)^2.
// The semantics of torch.logsumexp in float64: a NaN makes s1 NaN for good, -inf adds nothing, all -inf leaves
// (m, s1) = (-inf, 0) and finishes as -inf -- no -inf - -inf is ever formed.
struct Lse {
    double m, s1, s2;
};
FF_HD Lse lse_empty() { return Lse{-INFINITY, 0.0, 0.0}; }

FF_HD double lse_factor(double m_part, double m) { return m_part == m ? 1.0 : exp(m_part - m); }

FF_HD void lse_add(Lse& a, double lw)
{
#pragma clang fp contract(off)
    if (lw > a.m) {
        const double e = lse_factor(a.m, lw);             // exp(-inf) = 0 for the first finite one
        a.s1 = a.s1 * e + 1.0;
        a.s2 = a.s2 * (e * e) + 1.0;
        a.m = lw;
    } else if (!(lw == -INFINITY)) {                      // (a NaN comes here and stays)
        const double w = lse_factor(lw, a.m);
        a.s1 += w;
        a.s2 += w * w;
    }
}

FF_HD Lse lse_merge(const Lse& a, const Lse& b)
{
#pragma clang fp contract(off)
    const double m = a.m > b.m ? a.m : b.m;               // neither is ever NaN
    const double ea = lse_factor(a.m, m), eb = lse_factor(b.m, m);
    const double p1 = a.s1 * ea, q1 = b.s1 * eb, p2 = a.s2 * (ea * ea), q2 = b.s2 * (eb * eb);
    return Lse{m, p1 + q1, p2 + q2};
}

// log p = m + log s1 - log K - log_det;  ess = s1^2 / s2 (NaN where no draw has weight: 0 / 0)
FF_HD void lse_finish(const Lse& a, int K, double log_det, float* logp, float* ess)
{
#pragma clang fp contract(off)
    *logp = (float)(a.m + log(a.s1) - log((double)K) - log_det);
    if (ess) *ess = (float)(a.s1 * a.s1 / a.s2);
}

// ---- the gradient of the K-draw marginal (ff_marginal_weigh / ff_marginal_grad_reduce) -------------------------------------
// With the momenta fixed, L = logsumexp_k lw_k - log K - log_det has dL / d lw_k = wn_k = exp(lw_k - max lw) / W, so its
// gradients are the wn-weighted sums of the rows' own gradients of lw_k = log N(z1_k) - log N(p0_k): the q half of the
// pull-back of -z1_k through the solve, and its conditional part.  A draw whose normalised weight is 0, or below the
// caller's min_weight, adds nothing (at most min_weight |g_k|): it is not KEPT, and its row is never pulled back or read.

// a point without a gradient: a NaN among its lw (s1 is NaN) or none above -inf (s1 = 0)
FF_HD bool lse_degenerate(const Lse& a) { return !(a.s1 > 0.0); }

// draw k of a point whose merged state is (m, s1) is kept iff its normalised weight is positive and >= min_weight: the
// rule of observe::keep_draw on the double lw
FF_HD int32_t keep_weight(double lw, double m, double s1, double min_weight)
{
#pragma clang fp contract(off)
    const double wn = lse_factor(lw, m) / s1;
    return wn > 0.0 && wn >= min_weight ? 1 : 0;
}

// the maximum of the lw seen so far (exact in any order) and whether a NaN was among them
FF_HD void max_add(double& m, int& bad, double lw)
{
    bad |= lw != lw;
    m = lw > m ? lw : m;
}

// one entry of a gradient: the weighted sum times 1 / W, over the unit of that column (scale[d] / conditional_scale[c];
// NULL: 1), all in double, rounded to fp32 once.  At K = 1 the sum is the row's own float and W = 1: a division of two
// floats through double is the correctly rounded fp32 quotient.
FF_HD float grad_finish(double sum, double rW, const float* unit, int d)
{
#pragma clang fp contract(off)
    double v = sum * rW;
    if (unit) v = v / (double)unit[d];
    return (float)v;
}

// lanes that share one row on the device: the power of two >= ceil(D / 4), at most a wavefront
FF_HD int lanes_per_row(int D)
{
    const int nblk = (D + 3) / 4;
    int p = 1;
    while (p < nblk && p < 64) p *= 2;
    return p;
}

} // namespace marginal
} // namespace ff
