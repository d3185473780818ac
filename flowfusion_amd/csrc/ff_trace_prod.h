// ff_trace_prod.h -- the Hutch++ and XTrace divergence estimators of ff_trace_est.h from matrix-vector PRODUCTS instead of the
// matrix: shared by the gfx950 kernels (ff_trace_prod.hip: ff_trace_basis, ff_trace_combine) and their host twins.
//
// ff_trace_est.h estimates from A = J^T on hand and sums every product A v itself.  Here the products come from outside
// (ff_mlp_ode_launch_vjp: A v = a v + b J_net^T v of every evaluation row, which is how the reference obtains them,
// flowfusion/diffusion.py:356-398 and :419-455), in two rounds with a factorisation between them:
//     basis    Y = A P is given (P = S for Hutch++, O for XTrace).  Q = thin_qr(Y), the SAME thin_qr.  Hutch++ also forms
//              u_g = g - Q (Q^T g) for its m probes G; XTrace keeps the r x r factor R.  Out: the second round's seeds
//              [q_0 .. q_{r-1} | u_0 .. u_{m-1}] (Hutch++) or [q_0 .. q_{r-1}] (XTrace).
//     combine  Z = A [Q | U] is given.  Hutch++: sum_c q_c^T (A q_c) + mean_g u_g^T (A u_g)   (:381-400);
//              XTrace: the leave-one-out combination from (Q, R, O, A Q)                        (:451-481).
// Every expression is ff_trace_est.h's, in its order, in fp32, with every `matvec` result read instead of summed: on a
// matrix whose products are exact the two agree bit for bit (tests/test_estimator_products_host.py).
//
// One work item = one (evaluation row, sample).  Its vectors are rows of [.][D] arrays (element (c, i) at [c * D + i]); its
// scratch is addressed through a base and a stride like ff_trace_est.h's (`W(i) = ws[i stride]`): plain on the host, item-
// fastest in global memory on the device.
#pragma once
#include "ff_trace_est.h"

namespace ff {
namespace trace {

// floats of workspace per work item: the Q storage of thin_qr with its reflector scalars, then Hutch++'s Q^T g, or XTrace's
// R (basis) and its five r x r matrices (combine)
FF_HD size_t prod_workspace_per_item(int kind, int D, int r)
{
    const size_t d = (size_t)D, k = (size_t)r;
    return kind == FF_TRACE_XTRACE ? d * k + k + 5 * k * k : d * k + 2 * k;
}

struct ProdItem {
    const float* y;          // [r][D]   A P                        (basis)
    float* basis;            // [K2][D]  Q | U (Hutch++), Q (XTrace) (basis writes, combine reads)
    float* rfac;             // [r][r]   R (XTrace)                  (basis writes, combine reads)
    const float* prod;       // [K2][D]  A (Q | U)                   (combine)
    const float* p0;         // probes S or O: element (c, i) at p0[c * pstride0 + i]
    size_t pstride0;
    const float* p1;         // probes G: element (c, i) at p1[c * pstride1 + i]
    size_t pstride1;
    float* ws;               // workspace base of this item
    size_t stride;           // floats between consecutive workspace words of this item
    int D, r, m;
};

#define FF_PW(i) p.ws[(size_t)(i) * p.stride]
#define FF_PQ(i, c) FF_PW((i) * r + (c))
#define FF_PB(c, i) p.basis[(size_t)(c) * D + (i)]
#define FF_PZ(c, i) p.prod[(size_t)(c) * D + (i)]
#define FF_PP0(c, i) p.p0[(size_t)(c) * p.pstride0 + (i)]

// the seeds of the second round from the first round's products (hutchpp / xtrace of ff_trace_est.h up to their first
// product with Q)
FF_HD void basis(int kind, const ProdItem& p)
{
#pragma clang fp contract(off)
    const int D = p.D, r = p.r, m = p.m;
    const int tau0 = D * r, w0 = tau0 + r;           // (XTrace: w0 = R0)
    Item it;
    it.A = nullptr; it.astride = 0; it.p0 = nullptr; it.pstride0 = it.pk0 = 0; it.p1 = nullptr; it.pstride1 = it.pk1 = 0;
    it.ws = p.ws; it.stride = p.stride; it.D = D; it.r = r; it.m = m;
    for (int c = 0; c < r; ++c)                      // the sketch Y = A P, into the Q storage
        for (int i = 0; i < D; ++i) FF_PQ(i, c) = p.y[(size_t)c * D + i];
    const bool xt = kind == FF_TRACE_XTRACE;
    thin_qr<0>(it, tau0, xt ? w0 : -1);
    for (int c = 0; c < r; ++c)
        for (int i = 0; i < D; ++i) FF_PB(c, i) = FF_PQ(i, c);
    if (xt) {
        for (int a = 0; a < r * r; ++a) p.rfac[a] = FF_PW(w0 + a);
        return;
    }
    // u = (I - Q Q^T) g for every g                                             (:388-394)
    for (int g = 0; g < m; ++g) {
        const float* gv = p.p1 + (size_t)g * p.pstride1;
        for (int c = 0; c < r; ++c) {
            float s = 0.f;
            for (int i = 0; i < D; ++i) s += FF_PQ(i, c) * gv[i];
            FF_PW(w0 + c) = s;
        }
        for (int i = 0; i < D; ++i) {
            float s = 0.f;
            for (int c = 0; c < r; ++c) s += FF_PQ(i, c) * FF_PW(w0 + c);
            FF_PB(r + g, i) = gv[i] - s;
        }
    }
}

// flowfusion/diffusion.py:381-400 from (Q, U, A Q, A U)
FF_HD float hutchpp_combine(const ProdItem& p)
{
#pragma clang fp contract(off)
    const int D = p.D, r = p.r, m = p.m;
    float trace_range = 0.f;                                                     // sum_c q_c^T A q_c  (:381-386)
    for (int c = 0; c < r; ++c)
        for (int i = 0; i < D; ++i) trace_range += FF_PB(c, i) * FF_PZ(c, i);
    float trace_rest = 0.f;                                                      // u^T A u            (:396-398)
    for (int g = 0; g < m; ++g)
        for (int i = 0; i < D; ++i) trace_rest += FF_PB(r + g, i) * FF_PZ(r + g, i);
    return trace_range + trace_rest / (float)m;                                  // (:400)
}

// flowfusion/diffusion.py:451-481 from (Q, R, O, A Q)
FF_HD float xtrace_combine(const ProdItem& p)
{
#pragma clang fp contract(off)
    const int D = p.D, k = p.r;
    const int H0 = 0, Wm0 = H0 + k * k, T0 = Wm0 + k * k, S0 = T0 + k * k, X0 = S0 + k * k;
#define FF_M(base, a, b) FF_PW((base) + (a) * k + (b))
#define FF_R(a, b) p.rfac[(a) * k + (b)]
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) { FF_M(H0, a, b) = 0.f; FF_M(T0, a, b) = 0.f; }
    // Z = A Q is given; H = Q^T Z (:451), T = Z^T O (:455), W = Q^T O (:453)
    for (int c = 0; c < k; ++c)
        for (int i = 0; i < D; ++i) {
            const float z = FF_PZ(c, i);
            for (int a = 0; a < k; ++a) {
                FF_M(H0, a, c) += FF_PB(a, i) * z;
                FF_M(T0, c, a) += z * FF_PP0(a, i);
            }
        }
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            float s = 0.f;
            for (int i = 0; i < D; ++i) s += FF_PB(a, i) * FF_PP0(b, i);
            FF_M(Wm0, a, b) = s;
        }
    // S^T = R^-1 by back substitution (:457), rows to unit length (:459); S(a, i) = Rinv(i, a) is stored directly
    for (int col = 0; col < k; ++col) {
        for (int a = k - 1; a >= 0; --a) {
            float s = a == col ? 1.f : 0.f;
            for (int b = a + 1; b < k; ++b) s -= FF_R(a, b) * FF_M(S0, col, b);   // Rinv(b, col) sits at S(col, b)
            FF_M(S0, col, a) = s / FF_R(a, a);
        }
    }
    for (int i = 0; i < k; ++i) {
        float ss = 0.f;
        for (int a = 0; a < k; ++a) ss += FF_M(S0, a, i) * FF_M(S0, a, i);
        const float nrm = sqrtf(ss);
        for (int a = 0; a < k; ++a) FF_M(S0, a, i) = FF_M(S0, a, i) / nrm;
    }
    float tr_h = 0.f;
    for (int a = 0; a < k; ++a) tr_h += FF_M(H0, a, a);                          // (:463)
    float total = 0.f;
    for (int i = 0; i < k; ++i) {
        float sw = 0.f;
        for (int a = 0; a < k; ++a) sw += FF_M(S0, a, i) * FF_M(Wm0, a, i);
        for (int a = 0; a < k; ++a) FF_M(X0, a, i) = FF_M(Wm0, a, i) - sw * FF_M(S0, a, i);     // (:467)
        float shs = 0.f, xhx = 0.f, sr = 0.f, tx = 0.f;
        for (int a = 0; a < k; ++a) {
            float hs = 0.f, hx = 0.f;
            for (int b = 0; b < k; ++b) {
                hs += FF_M(H0, a, b) * FF_M(S0, b, i);
                hx += FF_M(H0, a, b) * FF_M(X0, b, i);
            }
            shs += FF_M(S0, a, i) * hs;                                          // (:469)
            xhx += FF_M(X0, a, i) * hx;                                          // (:471)
            sr += FF_M(S0, a, i) * FF_R(a, i);                                   // (:475)
            tx += FF_M(T0, a, i) * FF_M(X0, a, i);                               // (:477)
        }
        total += tr_h - shs + sw * sr - tx + xhx;                                // (:479)
    }
    return total / (float)k;                                                     // (:481)
#undef FF_M
#undef FF_R
}

#undef FF_PW
#undef FF_PQ
#undef FF_PB
#undef FF_PZ
#undef FF_PP0

FF_HD float combine(int kind, const ProdItem& p) { return kind == FF_TRACE_XTRACE ? xtrace_combine(p) : hutchpp_combine(p); }

// the item (row e, sample b) of a launch: t = e * batch + b
template <class Args>
FF_HD ProdItem prod_item(const Args& a, long long t, float* ws, size_t stride)
{
    const long long b = t % a.batch;
    const size_t D = (size_t)a.dim, K2 = (size_t)(a.kind == FF_TRACE_XTRACE ? a.r : a.r + a.m);
    ProdItem p;
    p.y = a.y ? a.y + (size_t)t * a.r * D : nullptr;
    p.basis = a.basis + (size_t)t * K2 * D;
    p.rfac = a.rfac ? a.rfac + (size_t)t * a.r * a.r : nullptr;
    p.prod = a.prod ? a.prod + (size_t)t * K2 * D : nullptr;
    p.p0 = a.probes0 + (size_t)b * D; p.pstride0 = (size_t)a.batch * D;
    p.p1 = a.probes1 ? a.probes1 + (size_t)b * D : nullptr; p.pstride1 = (size_t)a.batch * D;
    p.ws = ws; p.stride = stride;
    p.D = a.dim; p.r = a.r; p.m = a.m;
    return p;
}

} // namespace trace
} // namespace ff
