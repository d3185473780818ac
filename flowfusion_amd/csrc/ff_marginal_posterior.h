// ff_marginal_posterior.h -- the arithmetic of the per-object posterior of a NOISY observation under a symplectic flow, from
// the K joint draws of its marginal likelihood; shared by the gfx950 kernel (ff_marginal_posterior.hip:
// marginal_observe_resample_kernel) and the host entry point the CPU tests call (ff_marginal_observe_resample_host, compiled
// from the host pass of the same file).
//
// The flow preserves volume in [q | p], so the joint draw (z_k, p_k) of data point r carries the weight w_k = N(z1_k) / N(p_k):
// an unbiased one-momentum estimate of p(xhat - sigma z_k).  The K candidates y_k = xhat - sigma z_k with these weights are a
// pseudo-marginal, self-normalised importance sample of p(x | xhat, sigma) ~ p(x) N(xhat; x, diag sigma^2): M multinomial
// draws and the weighted mean and variance, as ff_weighted_resample forms them from a particle buffer and fp32 log-weights.
// Here the log-weights are ff_marginal_weigh's, in double, and there is no particle buffer: the expansion writes whitened
// [q | p] rows, which the solve consumes.  A particle is REGENERATED where it is needed,
//     y_k[d] = fl(x[d] - fl(sigma[d] z_kd)),   z_kd = z(seed, global row, FF_OBS_NOISE_BASE + k, d)
// bit for bit ff_observe_expand's row (observe::perturb on marginal::normals4), in the units of x.
//
// Everything else is ff_marginal.h and ff_observe.h, used as they are: the weights are marginal::lse_factor about the maximum
// of marginal::max_add, the targets observe::resample_targets, the moments observe::moment1_add / moment2_add one block of
// four dimensions at a time, times the double 1 / W, rounded to fp32 once.
#pragma once
#include <math.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal.h"
#include "ff_observe.h"
#include "ff_marginal_observe.h"

namespace ff {
namespace marginal_posterior {

using marginal::normals4;

constexpr int kMaxDraws = marginal_observe::kMaxDraws;
constexpr int kMaxSamples = observe::kMaxSamples;

// the block of four dimensions 4 blk .. of candidate k of global row gs, zero beyond D (what observe::load_block returns for
// the same block of ff_observe_expand's row): xb / sb are that block of x and noise_std
FF_HD void particle_block(const float (&xb)[4], const float (&sb)[4], uint64_t seed, uint64_t gs, int k, int blk, int D,
                          float (&v)[4])
{
    float z[4];
    normals4(seed, gs, FF_OBS_NOISE_BASE + (uint32_t)k, (uint32_t)blk, z);
    for (int j = 0; j < 4; ++j) v[j] = 4 * blk + j < D ? observe::perturb(xb[j], sb[j], z[j]) : 0.f;
}

// a point without a posterior: a NaN among its lw (marginal::max_add's flag), or none above -inf
FF_HD bool point_degenerate(int bad, double m) { return bad || m == -INFINITY; }

FF_HD bool resample_args_ok(const float* x, const float* noise_std, int32_t std_row_stride, const double* lw, int64_t B,
                            int32_t D, int32_t K, int32_t M, const float* samples, const int32_t* index, const float* mean,
                            const float* var)
{
    if (!x || !noise_std || !lw || B < 0 || D < 1 || K < 1 || K > kMaxDraws || M < 0 || M > kMaxSamples) return false;
    if (std_row_stride != 0 && std_row_stride != D) return false;
    return samples || index || mean || var;
}

} // namespace marginal_posterior
} // namespace ff
