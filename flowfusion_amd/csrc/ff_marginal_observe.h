// ff_marginal_observe.h -- the arithmetic of the K-draw marginal log-density of NOISY observations under a symplectic
// flow, shared by the gfx950 kernels (ff_marginal_observe.hip: marginal_observe_expand_kernel /
// marginal_observe_grad_reduce_kernel) and the host entry points the CPU tests call (ff_marginal_observe_expand_host /
// ff_marginal_observe_grad_reduce_host, compiled from the host pass of the same file).
//
// An observation xhat = x + n, n ~ N(0, diag(sigma^2)), of a model whose density is itself a marginal over the momentum:
//     p_obs(xhat | sigma) = E_{z, p}[N(Phi([((xhat - sigma z) - shift) / scale | p])) / N(p)] / prod scale
// One draw k of data point r is a JOINT draw: the noise z_k under the noise index FF_OBS_NOISE_BASE + k and the momentum
// p_k under FF_MOMENTUM_NOISE_BASE + k, both of global row sample_offset + r.  The rows are what ff_marginal_weigh already
// reduces (it regenerates p_k under the same keys); what is new is the starting state and d / d sigma:
//     z0[r K + k] = [fl(fl(fl(xhat - fl(sigma z_k)) - shift) / scale) | p_k]        (perturb, then whiten: four roundings)
//     dL / d sigma_d = -(sum_k w_k z_kd g_q,kd / W) / scale_d                         (dq0 / d sigma = -z / scale)
// Everything else is ff_marginal.h and ff_observe.h, used as they are: the q half is observe::perturb then marginal::whiten,
// the weighted sums are observe::moment1_add / noise_add over marginal::lse_factor weights, finished by
// marginal::grad_finish.
#pragma once
#include <math.h>
#include <stdint.h>
#include "flowfusion_amd.h"
#include "ff_marginal.h"
#include "ff_observe.h"

namespace ff {
namespace marginal_observe {

using marginal::normals4;

constexpr int kMaxDraws = marginal::kMaxMomenta < observe::kMaxDraws ? marginal::kMaxMomenta : observe::kMaxDraws;

// q0 of one draw: the de-noised candidate of ff_observe_expand, whitened as ff_marginal_expand whitens x
FF_HD float start_q(float x, float s, float z, const float* shift, const float* scale, int d)
{
    return marginal::whiten(observe::perturb(x, s, z), shift, scale, d);
}

// one entry of dL / d sigma: minus the weighted sum of z g_q times 1 / W over scale[d] (NULL: 1), all in double, rounded
// to fp32 once.  At K = 1 the sum is the exact product z g and W = 1: -z g / scale rounded once.
FF_HD float noise_grad_finish(double sum, double rW, const float* scale, int d)
{
#pragma clang fp contract(off)
    double v = sum * rW;
    if (scale) v = v / (double)scale[d];
    return (float)-v;
}

// the union of ff_observe_expand's and ff_marginal_expand's refusals
FF_HD bool expand_args_ok(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond, int64_t B,
                          int32_t D, int32_t C, int32_t K, const float* z0, const float* cond_out)
{
    if (!x || !noise_std || !z0 || B < 0 || D < 1 || K < 1 || K > kMaxDraws) return false;
    if (std_row_stride != 0 && std_row_stride != D) return false;
    if (cond && (C < 1 || !cond_out)) return false;
    return true;
}

// the union of ff_marginal_grad_reduce's and ff_observe_grad_reduce's refusals
FF_HD bool grad_reduce_args_ok(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                               const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K,
                               const float* grad_x, const float* grad_c)
{
    if (!lw || !row_of || !gz_rows || !noise_std || !grad_x || B < 0 || D < 1 || K < 1 || K > kMaxDraws) return false;
    if (std_row_stride != 0 && std_row_stride != D) return false;
    if (gc_rows && (C < 1 || !grad_c)) return false;
    return true;
}

} // namespace marginal_observe
} // namespace ff
