// ff_observe.h -- the arithmetic of the K-draw log-density of noisy observations, shared by the gfx950 kernels
// (ff_observe.hip: observe_expand_kernel / logmeanexp_kernel) and the host entry points the CPU tests call
// (ff_observe_expand_host / ff_logmeanexp_host, compiled from the host pass of the same file).
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

} // namespace observe
} // namespace ff
