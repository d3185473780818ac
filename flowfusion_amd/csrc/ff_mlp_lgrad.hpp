// ff_mlp_lgrad.hpp -- the gradient of a fixed-grid Hutchinson log-density with respect to the state and the conditional inputs
// (gfx950): the transposed row program of mlp_dadj_kernel (ff_mlp_dadj.hpp) with the divergence integral in it -- reverse mode
// over the forward-mode tangent, from recorded stage states.  One kernel, one instance per pull-back shape; a PULL plan launches
// it with its two weight packs (ff_mlp_pull_wpack), as it launches the record and discrete-adjoint units.
//
// The forward program over the rows e = 0 .. E-1 of an ordinary table, with one probe eps per sample row:
//     y_e = x + sum_s cin_e[s] k[s];   k[slot_e] = a_e y_e + b_e NET(y_e, c);   kl[slot_e] = a_e eps.eps + b_e eps^T J_net(y_e, c) eps
//     FLAG_STEP_END:  x += sum_s cout_e[s] k[s];   lp += sum_s cout_e[s] kl[s]
// mlp_lgrad_kernel (ff_mlp_ode_launch_logp_grad) runs the table from e = E-1 down to 0 on the state adjoint slots kb[s] (LDS, zero
// at the start), the scalar adjoint slots kd[s] of the divergence (registers, zero at the start) and xb = cotangent_in * out_scale:
//     1. FLAG_STEP_END:  kb[s] += cout_e[s] xb;   kd[s] += cout_e[s]                       every kept slot
//     2. rb = kb[slot_e];  kb[slot_e] = 0;   w_e = kd[slot_e] * dlogp_cotangent[sample];  kd[slot_e] = 0
//     3. yb = a_e rb + b_e (J_net^T rb + w_e grad_y (eps^T J_net eps));   gamma += b_e ((dNET/dc)^T rb + w_e grad_c (eps^T J_net eps))
//     4. xb += yb;  kb[s] += cin_e[s] yb                                                   every kept slot
// and hands back grad_x_out = xb / in_scale, grad_cond_out = gamma.  (a_e eps.eps has no gradient.)
//
// Columns: exactly TWO per sample, 8 samples per 16-column tile, one wavefront per workgroup.
//   net A  role 0 the value column [y_e | cond] (y_e from the record, loaded a row ahead), role 1 the tangent column [eps | 0]
//          with zero bias: FF_MODE_HUTCH's activation path, h' = SiLU'(z) z' with the slope fetched from the value lane by
//          ds_bpermute.  A second ds_bpermute beside it fetches SiLU''(z) = s (1 - s) (2 + z (1 - 2 s)).  Two words per hidden
//          unit and sample go to the stash, one writer each: the value lane parks SiLU'(z), the tangent lane t = SiLU''(z) z'.
//   net B  role 0 the g column, seeded rb; role 1 the u column, seeded eps.  With ub the u column's activation cotangent of a
//          unit:  u: ub -> SiLU'(z) ub (pull_stage);   g: gb -> SiLU'(z) gb + w_e t ub.  The g lane fetches ub from lane + 1 by one
//          ds_bpermute per register at the stage that reads the stash, and consumes it a stage later.  The g column's output
//          registers are J_net^T rb + w_e grad (eps^T J_net eps), state part and conditional part; the u column's are discarded.
// The weight ring across A -> B -> the next row, the c1 prefetch running backwards (clamped at row 0), the record read a row
// ahead, the two fence / wave-barrier pairs around the stash, FF_STATUS_BAD_SLOT, FF_STATUS_NOISE_ROW and the gate are
// mlp_dadj_kernel's.  Outputs are written by the g lanes only.
//
// LDS = slots x DREGS x 256 bytes of adjoint slots + 64 x n_hidden x H bytes of stash (lgrad_lds_bytes, ff_api.cpp).
//
// KernelArgs keeps its size and its fields.  The launch refuses the divergence side, noise and a first stage from the caller, so
// these fields carry the launch's own (ff_api.cpp fills them):
//     probe          cotangent_in     [batch, dim]   cotangent of the final state
//     dlogp_out      grad_x_out       [batch, dim]
//     jac_out        grad_cond_out    [batch, cond_dim] or NULL
//     k1_in          record_in        [n_evals, batch, dim]
//     kl1_in         probe_in         [batch, dim]   the Hutchinson probe of each row
//     dlogp_in       dlogp_cotangent  [batch] or NULL (= 1): the weight of the row's divergence integral
//     tangent_first  the stage slots kept, 1 .. kSlots (ff_ode_args.stage_slots, 0 = all kSlots)
//     n_tangent      1
//     x_in, x_out    not read, not written
#pragma once
#include "ff_mlp_ode.hpp"

namespace ff {

// Net A's activation of 4 registers in the five stages of act_stage<TANGENTS>: value lanes P = SiLU(pre), tangent lanes
// P = SiLU'(z of the value lane) pre.  Stage 3 also sends SiLU'' across; after stage 4, g.dv holds SiLU'(z) and g.h SiLU''(z) of
// the sample's value lane on both lanes.
template <int STAGE>
__device__ __forceinline__ void lgrad_act_stage(ActGroup& g, float* __restrict__ dst, bool is_tan, int value_lane_bytes)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (STAGE == 0) {
            g.t[i] = g.pre[i] * -1.44269504088896340736f;
        } else if constexpr (STAGE == 1) {
            g.t[i] = __builtin_amdgcn_exp2f(g.t[i]);
        } else if constexpr (STAGE == 2) {
            g.r[i] = __builtin_amdgcn_rcpf(1.0f + g.t[i]);
        } else if constexpr (STAGE == 3) {
            const float a = g.pre[i], s = g.r[i];
            // silu'(a) = s (1 + a (1 - s));  silu''(a) = s (1 - s) (2 + a (1 - 2 s))
            const float w = __builtin_fmaf(-a, s, a);
            const float d = __builtin_fmaf(s, w, s);
            const float ss = __builtin_fmaf(-s, s, s);
            const float dd = ss * __builtin_fmaf(a, __builtin_fmaf(-2.0f, s, 1.0f), 2.0f);
            g.dv[i] = __builtin_amdgcn_ds_bpermute(value_lane_bytes, __builtin_bit_cast(int, d));
            g.h[i] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(value_lane_bytes, __builtin_bit_cast(int, dd)));
        } else {
            dst[i] = g.pre[i] * (is_tan ? __builtin_bit_cast(float, g.dv[i]) : g.r[i]);
        }
    }
}

template <int TILE, int H, int DREGS, int CREGS, int RING>
__global__ __launch_bounds__(64) void mlp_lgrad_kernel(const KernelArgs args)
{
    static_assert(kChunkPad % RING == 0, "ring must divide the chunk padding");
    static_assert(TILE == 16, "two columns per sample on the 16-column tile");
    typedef Tile<TILE> T;
    constexpr int NB = H / 32;                       // logical blocks per hidden layer
    constexpr int RB = T::RB;                        // registers per logical block
    constexpr int GPB = RB / 4;                      // activation groups per logical block
    constexpr int K1 = DREGS + CREGS;                // operand registers of net A's first layer = output registers of net B
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);     // output blocks of net A
    constexpr int NOB_T = blocks_for_regs(TILE, K1);          // output blocks of net B
    constexpr int KH = NB * RB;                      // operand registers of a hidden layer
    constexpr int R4 = DREGS / 4;
    constexpr int SPW = TILE / 2;                    // samples per tile

    if (args.gate && *(const volatile int*)args.gate == 0) return;

    const int lane = threadIdx.x & 63;
    const int qd = lane >> T::SHIFT;                 // lane group (k index of the MFMA operands)
    const int col = lane & (TILE - 1);
    const int lane16 = lane * 16;
    const int q16 = qd * 16;
    const long long wave = (long long)blockIdx.x;    // one tile per workgroup, one wavefront per workgroup
    const int D = args.dim, C = args.cond_dim;

    // ---- column roles: two adjacent columns per sample ------------------------------------------------------------------------
    const int s_in_wave = col >> 1;
    const int role = col & 1;                        // 0 = value (net A) / g (net B), 1 = tangent (net A) / u (net B)
    const bool is_tan = role != 0;
    bool col_live = true;
    long long sample = wave * SPW + s_in_wave;
    if (sample >= args.batch) { sample = args.batch - 1; col_live = false; }
    const int q16b = is_tan ? 0x7ffffff0 : q16;      // bias offset of net A: out of range = zero on the tangent columns
    const int value_lane_bytes = (lane & ~1) * 4;    // the sample's role-0 lane of this lane group
    const int u_lane_bytes = (lane | 1) * 4;         // its role-1 lane

    // ---- g lanes: xb = cotangent * out_scale, gamma = 0, the weight of the divergence; tangent lanes: the probe -----------------
    float xb[DREGS], eps[DREGS];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) {
        const int d = feat_of_reg(TILE, r, qd);
        float v = 0.f, p = 0.f;
        if (d < D) {
            if (is_tan) {
                p = args.kl1_in[sample * D + d];                                 // probe_in
            } else {
                v = args.probe[sample * D + d];                                  // cotangent_in
                if (args.out_scale) v = v * args.out_scale[d];
            }
        }
        xb[r] = v;
        eps[r] = p;
    }
    const float wgt = is_tan ? 0.f : (args.dlogp_in ? args.dlogp_in[sample] : 1.0f);      // dlogp_cotangent
    float gam[CREGS > 0 ? CREGS : 1];
#pragma unroll
    for (int r = 0; r < (CREGS > 0 ? CREGS : 1); ++r) gam[r] = 0.f;
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, is_tan, r);
    }
    // value lanes: the recorded stage state of row e is at rec0 + e * rec_row (record_in)
    const float* const rec0 = args.k1_in + sample * D;
    const long long rec_row = args.batch * D;
    const int E = args.n_evals;
    float ynext[DREGS];          // y of the row about to run, loaded a row ahead
#pragma unroll
    for (int r = 0; r < DREGS; ++r) {
        const int d = feat_of_reg(TILE, r, qd);
        ynext[r] = (!is_tan && d < D && E > 0) ? rec0[(long long)(E - 1) * rec_row + d] : 0.f;
    }

    // ---- LDS: adjoint slots (each lane its own words), then the stash: two words per hidden unit and sample -------------------
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + lane;
    const int nslots = args.tangent_first;           // stage slots kept (1 .. kSlots: the launcher's)
    f32x4* const stash = lds_slots + (size_t)nslots * R4 * 64;      // [n_hidden][KH / 4][2][NQ * SPW] groups of 4 words
    constexpr int srow = T::NQ * SPW;
    const int sidx = qd * SPW + s_in_wave;           // the place of (lane group, sample)
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        if (s < nslots) {
#pragma unroll
            for (int j = 0; j < R4; ++j) ks[(s * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    float kd[kSlots];            // the divergence's adjoint slots: the same on every lane
#pragma unroll
    for (int s = 0; s < kSlots; ++s) kd[s] = 0.f;

    const Layout L = make_layout(TILE, H, DREGS, CREGS, args.n_hidden);
    // net B's layout: an ordinary network with K1 state registers and no conditional ones (ff_mlp_pull.hpp)
    const Layout LT = make_layout(TILE, H, K1, 0, args.n_hidden);
    constexpr int CB = 1024 * T::PHYS;               // bytes per chunk
    const int sub_bytes = (int)(L.total_floats * 4); // net B's pack starts here
    const Stream ws = make_stream(args.wpack, args.wpack_floats);
    const Stream ts = make_stream(args.etab, (long long)args.n_evals * args.etab_stride);
    const int out_sbyte = L.chunk_off_out() * CB;    // (== LT.chunk_off_out() * CB)
    const int NH = args.n_hidden;

    f32x4 ring[RING][T::PHYS];
#pragma unroll
    for (int i = 0; i < RING; ++i)
#pragma unroll
        for (int p = 0; p < T::PHYS; ++p) ring[i][p] = sload(ws, lane16, i * CB + p * 1024);

    float P[KH];                 // operand registers of a hidden layer
    // hidden accumulators: net A's hold the bias of the layer about to run (the LAST row's c1 to start with); net B's start from zero
    BlockAcc<TILE> hacc[NB];
    {
        const int last_byte = (E > 0 ? E - 1 : 0) * args.etab_stride * 4;
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16b, last_byte + 128 + o * 128);
    }

    bool bad_slot = false, bad_noise = false;
    for (int e = E - 1; e >= 0; --e) {
        const int prev_row = e > 0 ? e - 1 : 0;     // the row that runs next; at e == 0 nothing before the table is read
        HdrPtr hdr = (HdrPtr)(args.etab + (size_t)e * args.etab_stride);
        const float a_e = hdr->a, b_e = hdr->b;
        const uint32_t flags = hdr->flags;
        const int slot = hdr->slot;

        // 1. the transpose of the step's end: every kept slot takes cout[s] xb, and cout[s] on the divergence side
        if (flags & 1u) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                const f32x4 v = f32x4{xb[4 * j], xb[4 * j + 1], xb[4 * j + 2], xb[4 * j + 3]};
#pragma unroll
                for (int s = 0; s < kSlots; ++s)
                    if (s < nslots) ks[(s * R4 + j) * 64] += hdr->cout[s] * v;
            }
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (s < nslots) kd[s] += hdr->cout[s];
        }
        // 2. the cotangents of this row's right-hand side and of its divergence leave their slots
        const bool slot_ok = (unsigned)slot < (unsigned)nslots;
        bad_slot |= !slot_ok;
        float rb[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) rb[r] = 0.f;
        float w_e = 0.f;
        if (slot_ok) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                const f32x4 v = ks[(slot * R4 + j) * 64];
                ks[(slot * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) rb[4 * j + i] = v[i];
            }
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                w_e = (slot == s) ? kd[s] : w_e;
                kd[s] = (slot == s) ? 0.f : kd[s];
            }
        }
        const float om = w_e * wgt;                 // (zero on the u lanes)

        float op[K1];            // first-layer operand: net A [y_e | cond] / [eps | 0], net B [rb | 0] / [eps | 0]
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = is_tan ? eps[r] : ynext[r];
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = CREGS > 0 ? cnd[r - DREGS] : 0.f;
        // the recorded state of the row that runs next: in flight behind this row's networks
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            ynext[r] = (!is_tan && d < D) ? rec0[(long long)prev_row * rec_row + d] : 0.f;
        }

        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last block,
        // activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        ActGroup ag[12];
        // net A, after stage 4: hidden layer `lyr`, group `grp` of its KH / 4 -- the value lane parks SiLU'(z), the tangent lane
        // SiLU''(z) z'
        auto park_words = [&](const ActGroup& g, int lyr, int grp) __attribute__((always_inline)) {
            f32x4 d;
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = is_tan ? g.h[i] * g.pre[i] : __builtin_bit_cast(float, g.dv[i]);
            stash[(size_t)((lyr * (KH / 4) + grp) * 2 + role) * srow + sidx] = d;
        };
        // net B: u lane  pre * SiLU'(z);  g lane  pre * SiLU'(z) + om * t * (pre of the u lane)
        auto pull_stage = [&](auto kk, ActGroup& g, float* dst, int lyr, int grp) __attribute__((always_inline)) {
            constexpr int k = decltype(kk)::value;
            if constexpr (k == 3) {
                const size_t at = (size_t)((lyr * (KH / 4) + grp) * 2) * srow + sidx;
                const f32x4 d = stash[at];
                const f32x4 t = stash[at + srow];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g.r[i] = d[i];
                    g.t[i] = t[i];
                    g.dv[i] = __builtin_amdgcn_ds_bpermute(u_lane_bytes, __builtin_bit_cast(int, g.pre[i]));
                }
            } else if constexpr (k == 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float base = g.pre[i] * g.r[i];
                    dst[i] = is_tan ? base : __builtin_fmaf(om * g.t[i], __builtin_bit_cast(float, g.dv[i]), base);
                }
            }
        };
        // stages of the previous layer's parked block (stash layer `lyr`): group gi starts at slot gi*(16*PHYS/GPB)
        auto prev_slot = [&](auto net_b, auto mm, int lyr) __attribute__((always_inline)) {
            constexpr bool TRANSPOSED = decltype(net_b)::value;
            constexpr int M = decltype(mm)::value;
            static_for<kActStages>([&](auto kk) {
                constexpr int k = kActStages - 1 - decltype(kk)::value;     // oldest group first
                constexpr int step = 16 * T::PHYS / GPB;
                constexpr int s0 = M - k * T::PHYS;
                if constexpr (s0 >= 0 && s0 < 16 * T::PHYS && s0 % step == 0) {
                    constexpr int gi = s0 / step;
                    if constexpr (k == 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) ag[gi].pre[i] = pend[4 * gi + i];
                    }
                    if constexpr (TRANSPOSED) {
                        pull_stage(std::integral_constant<int, k>{}, ag[gi], &P[(NB - 1) * RB + 4 * gi], lyr, (NB - 1) * GPB + gi);
                    } else {
                        lgrad_act_stage<k>(ag[gi], &P[(NB - 1) * RB + 4 * gi], is_tan, value_lane_bytes);
                        if constexpr (k == 4) park_words(ag[gi], lyr, (NB - 1) * GPB + gi);
                    }
                }
            });
        };
        // stages of this layer's own blocks 0 .. NB-2 (geometry G; stash layer `lyr`), hung on slot M
        auto own_slot = [&](auto net_b, auto geom, auto mm, const BlockAcc<TILE> (&acc)[NB], int lyr) __attribute__((always_inline)) {
            constexpr bool TRANSPOSED = decltype(net_b)::value;
            constexpr LayerGeom G = decltype(geom)::value;
            constexpr int M = decltype(mm)::value;
            static_for<kActStages>([&](auto kk) {
                constexpr int k = kActStages - 1 - decltype(kk)::value;     // oldest group first
                constexpr int id = act_group_at(G, T::PHYS, GPB, M, k);
                if constexpr (id >= 0) {
                    constexpr int blk = id / GPB, gi = id % GPB;
                    if constexpr (k == 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) ag[4 + id % 8].pre[i] = acc[blk].reg(4 * gi + i);
                    }
                    if constexpr (TRANSPOSED) {
                        pull_stage(std::integral_constant<int, k>{}, ag[4 + id % 8], &P[blk * RB + 4 * gi], lyr, id);
                    } else {
                        lgrad_act_stage<k>(ag[4 + id % 8], &P[blk * RB + 4 * gi], is_tan, value_lane_bytes);
                        if constexpr (k == 4) park_words(ag[4 + id % 8], lyr, id);
                    }
                }
            });
        };
        auto refill = [&](int byte, auto ob) {
            constexpr int o = decltype(ob)::value;
            if constexpr (o >= 2) hacc[o - 2] = load_bias_acc<TILE>(ws, q16b, byte + (o - 2) * 128);
        };
        auto park = [&](const BlockAcc<TILE>& acc) {
#pragma unroll
            for (int r = 0; r < RB; ++r) pend[r] = acc.reg(r);
        };
        auto park_and_refill = [&](int byte, const BlockAcc<TILE>& acc) {
            park(acc);
            if constexpr (NB >= 2) hacc[NB - 2] = load_bias_acc<TILE>(ws, q16b, byte + (NB - 2) * 128);
            hacc[NB - 1] = load_bias_acc<TILE>(ws, q16b, byte + (NB - 1) * 128);
        };
        constexpr std::false_type NET_A{};
        constexpr std::true_type NET_B{};
        using G1 = GeomTag<TILE, K1, NB>;
        using GH = GeomTag<TILE, KH, NB>;

        // ==== net A at the recorded state, value and tangent: the two words of every hidden unit, parked on the way ============
        {
            const int nbyte = (int)(L.bias_off_hid(0) * 4);
            run_layer<TILE, RING, K1, NB, false, false>(
                ring, ws, lane16, 0, op, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(NET_A, G1{}, mm, acc, 0); },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        for (int l = 0; l < NH - 1; ++l) {
            const int sbyte = L.chunk_off_hid(l) * CB;
            // (after the last hidden layer nothing reads hacc's bias: net B's first layer starts from zero)
            const int nbyte = (int)(L.bias_off_hid(l + 1) * 4);
            run_layer<TILE, RING, KH, NB, false, false>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(NET_A, mm, l);
                    own_slot(NET_A, GH{}, mm, acc, l + 1);
                },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        {
            // the output layer's place in the stream: its slots activate the last hidden block and park its words, and the
            // ring moves on to net B's first layer.  NET(y, c) and its tangent are not needed: nobody reads oacc.
            BlockAcc<TILE> oacc[NOB_OUT];
            constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
            run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
                ring, ws, lane16, out_sbyte, P, oacc, [&](auto) {},
                [&](auto mm, const BlockAcc<TILE> (&)[NOB_OUT]) { prev_slot(NET_A, mm, NH - 1); },
                [&](const BlockAcc<TILE>&) {}, sub_bytes);
        }
        // every word of this row is parked before a lane of net B reads one (one wavefront: program order of its DS
        // instructions; the fence keeps the compiler from moving them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ==== net B: the transposed network on the g and u columns ===============================================================
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = is_tan ? eps[r] : rb[r];
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = 0.f;
        run_layer<TILE, RING, K1, NB, false, true>(
            ring, ws, lane16, sub_bytes, op, hacc, [&](auto) {},
            [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(NET_B, G1{}, mm, acc, NH - 1); },
            [&](const BlockAcc<TILE>& acc) { park(acc); });
        for (int l = 0; l < NH - 1; ++l) {
            const int sbyte = sub_bytes + LT.chunk_off_hid(l) * CB;
            run_layer<TILE, RING, KH, NB, false, true>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto) {},
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(NET_B, mm, NH - 1 - l);
                    own_slot(NET_B, GH{}, mm, acc, NH - 2 - l);
                },
                [&](const BlockAcc<TILE>& acc) { park(acc); });
        }
        BlockAcc<TILE> tacc[NOB_T];
        // the hidden accumulators are idle from here on: fetch the c1 of the row that runs next, e - 1 (clamped at the table's start)
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16b, prev_row * args.etab_stride * 4 + 128 + o * 128);
        // the ring wraps to net A's first layer of the next row
        run_layer<TILE, RING, KH, NOB_T, true, true>(
            ring, ws, lane16, sub_bytes + out_sbyte, P, tacc, [&](auto) {},
            [&](auto mm, const BlockAcc<TILE> (&)[NOB_T]) { prev_slot(NET_B, mm, 0); },
            [&](const BlockAcc<TILE>&) {}, 0);
        // the next row's net A overwrites the stash only after every read of this row
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // 3. the cotangent of the stage state and of the conditional inputs (zero on the u column)
        float yb[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const float jt = tacc[r / RB].reg(r % RB);                       // (J_net^T rb + w_e grad_y (eps^T J_net eps))[feature of register r]
            yb[r] = is_tan ? 0.f : __builtin_fmaf(a_e, rb[r], b_e * jt);
        }
        if constexpr (CREGS > 0) {
#pragma unroll
            for (int r = DREGS; r < K1; ++r) {
                const float jc = tacc[r / RB].reg(r % RB);                   // the same of conditional feature r - DREGS
                gam[r - DREGS] = is_tan ? 0.f : __builtin_fmaf(b_e, jc, gam[r - DREGS]);
            }
        }
        // 4. the transpose of the stage input: xb and every kept slot take their share of yb
#pragma unroll
        for (int j = 0; j < R4; ++j) {
            const f32x4 v = f32x4{yb[4 * j], yb[4 * j + 1], yb[4 * j + 2], yb[4 * j + 3]};
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (s < nslots) ks[(s * R4 + j) * 64] += hdr->cin[s] * v;
#pragma unroll
            for (int i = 0; i < 4; ++i) xb[4 * j + i] += v[i];
        }
        bad_noise |= (flags & 2u) != 0;            // the record launch left the noise out: reported
    }

    // ---- epilogue: the gradients, from the g lanes -------------------------------------------------------------------------------
    if (col_live && !is_tan) {
        float* const gx = args.dlogp_out + sample * D;                       // grad_x_out
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            if (d < D) {
                float v = xb[r];
                if (args.in_scale) v = v / args.in_scale[d];
                gx[d] = v;
            }
        }
        if constexpr (CREGS > 0) {
            if (args.jac_out) {                                              // grad_cond_out
                float* const gc = args.jac_out + sample * C;
#pragma unroll
                for (int r = 0; r < CREGS; ++r) {
                    const int d = feat_of_reg(TILE, r, qd);
                    if (d < C) gc[d] = gam[r];
                }
            }
        }
    }
    if (args.status && bad_slot) {
        if (lane == 0) atomicOr(args.status, kStatusBadSlot);
    }
    if (args.status && bad_noise) {
        if (lane == 0) atomicOr(args.status, kStatusNoiseRow);
    }
}

} // namespace ff
