// ff_mlp_dadj.hpp -- the exact discrete adjoint of a fixed-grid solve (gfx950): the transpose of the map the sampler applies,
// from recorded stage states.  Two kernels, one instance of each per pull-back shape; a PULL plan launches them with its two
// weight packs (ff_mlp_pull_wpack), as it launches the products units.
//
// The forward solve is a program over the rows e = 0 .. E-1 of an ordinary table:
//     y_e = x + sum_s cin_e[s] k[s];   r_e = a_e y_e + b_e NET(y_e, c);   k[slot_e] = r_e;   FLAG_STEP_END: x += sum_s cout_e[s] k[s]
//
// mlp_rec_kernel (ff_mlp_ode_launch_record) runs it and writes every stage state down.  Every column of the tile is a sample; only
// net A runs (the ordinary half of the pull pack; the weight ring wraps from its output layer to its first layer), with the
// state algebra of mlp_vjp_kernel's value column: stage slots in LDS (DREGS words per slot and lane), cin / cout,
// rhs = fma(a_e, y, b_e NET), the affine prologue and epilogue, x_out, the status word.  At every row, before the network,
//     rec[(e * batch + sample) * D + d] = y_e[d]            in the integrated state's units (after the input map)
// A row with FF_ROW_NOISE: the noise is left out and FF_STATUS_NOISE_ROW reported.  This is the thinner variant: no slope
// stash, no second network, no dead cotangent columns -- LDS = slots x DREGS x 256 bytes.
//
// mlp_dadj_kernel (ff_mlp_ode_launch_pull_discrete) runs the SAME table from e = E-1 down to 0 on adjoint slots kb[s] (zero at
// the start) and xb = w * out_scale:
//     1. FLAG_STEP_END:  kb[s] += cout_e[s] xb                               every kept slot
//     2. rb = kb[slot_e];  kb[slot_e] = 0
//     3. yb = a_e rb + b_e J_net(y_e, c)^T rb;   gamma += b_e (dNET/dc)(y_e, c)^T rb
//     4. xb += yb;  kb[s] += cin_e[s] yb                                     every kept slot (after 2: a row may read its own slot)
// and hands back cot_x_out = xb / in_scale, cot_cond_out = gamma.  Columns as in the pull kernel, 1 + K per sample, one wavefront
// per workgroup.  Per row the value lane loads y_e from the record (the load of row e - 1 is issued a row ahead) and runs net A
// to park SiLU'(z_l) in the stash; the cotangent lanes run net B on rb.  Net A's output layer is kept in the chunk stream: the
// last hidden block is activated, and its slopes parked, on that layer's slots, and the ring walks on to net B behind it.  Its
// result is read by nobody, so the compiler drops its MFMAs; its chunks still pass through the ring.  The stash and the two
// fence / wave-barrier pairs around it are the pull kernel's.  Adjoint slots: DREGS words per lane and slot in LDS; gamma stays in
// CREGS registers.  LDS = slots x DREGS x 256 bytes + the stash, never more than the pull launch's at the same shape.
// The table's c1 prefetch runs backwards: the "next" row is e - 1, and at e = 0 the read is clamped to row 0 (nothing before the
// table's start is addressed).  A row that names a slot beyond the kept ones contributes nothing (the forward kernels store
// nothing for it) and sets FF_STATUS_BAD_SLOT; a row with FF_ROW_NOISE sets FF_STATUS_NOISE_ROW (the noise is additive: it has
// no part in the transpose, but the record launch left it out, so the results belong to another map).
//
// KernelArgs keeps its size and its fields.  Both launches refuse the divergence side, noise and a first stage from the caller,
// so these fields carry the launches' own (ff_api.cpp fills them):
//   record launch     dlogp_out      record_out    [n_evals, batch, dim]
//                     tangent_first  the stage slots kept in LDS, 1 .. kSlots (ff_ode_args.stage_slots, 0 = all kSlots)
//                     n_tangent      0: every column is a sample
//   discrete pull     probe          cotangent_in  [batch, K, dim]
//                     dlogp_out      cot_x_out     [batch, K, dim]
//                     jac_out        cot_cond_out  [batch, K, cond_dim] or NULL
//                     k1_in          record_in     [n_evals, batch, dim]
//                     tangent_first  the stage slots kept in LDS, as above
//                     x_in, x_out    not read, not written
#pragma once
#include "ff_mlp_ode.hpp"

namespace ff {

template <int TILE, int H, int DREGS, int CREGS, int RING>
__global__ __launch_bounds__(64) void mlp_rec_kernel(const KernelArgs args)
{
    static_assert(kChunkPad % RING == 0, "ring must divide the chunk padding");
    typedef Tile<TILE> T;
    constexpr int NB = H / 32;                       // logical blocks per hidden layer
    constexpr int RB = T::RB;                        // registers per logical block
    constexpr int GPB = RB / 4;                      // activation groups per logical block
    constexpr int K1 = DREGS + CREGS;                // operand registers of the first layer
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);     // output blocks
    constexpr int KH = NB * RB;                      // operand registers of a hidden layer
    constexpr int R4 = DREGS / 4;

    if (args.gate && *(const volatile int*)args.gate == 0) return;

    const int lane = threadIdx.x & 63;
    const int qd = lane >> T::SHIFT;                 // lane group (k index of the MFMA operands)
    const int col = lane & (TILE - 1);
    const int lane16 = lane * 16;
    const int q16 = qd * 16;
    const long long wave = (long long)blockIdx.x;    // one tile per workgroup, one wavefront per workgroup
    const int D = args.dim;
    const ActSpec aspec = {0.f, 0.f, 0.f, 0};

    // every column is a sample
    bool col_live = true;
    long long sample = wave * TILE + col;
    if (sample >= args.batch) { sample = args.batch - 1; col_live = false; }

    float x[DREGS];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) x[r] = state_reg<TILE>(args, sample, qd, false, 0, r);
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, false, r);
    }
    float* const rec0 = args.dlogp_out + sample * D;                                      // record_out, row 0 of this sample
    const long long rec_row = args.batch * D;

    // ---- LDS: stage slots (each lane its own words) ----------------------------------------------------------------------
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + lane;
    const int nslots = args.tangent_first;           // stage slots kept (1 .. kSlots: the launcher's)
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        if (s < nslots) {
#pragma unroll
            for (int j = 0; j < R4; ++j) ks[(s * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    const Layout L = make_layout(TILE, H, DREGS, CREGS, args.n_hidden);
    constexpr int CB = 1024 * T::PHYS;               // bytes per chunk
    const Stream ws = make_stream(args.wpack, args.wpack_floats);
    const Stream ts = make_stream(args.etab, (long long)args.n_evals * args.etab_stride);
    const int out_sbyte = L.chunk_off_out() * CB;
    const int out_bias_byte = (int)(L.bias_off_out() * 4);
    const int NH = args.n_hidden;

    f32x4 ring[RING][T::PHYS];
#pragma unroll
    for (int i = 0; i < RING; ++i)
#pragma unroll
        for (int p = 0; p < T::PHYS; ++p) ring[i][p] = sload(ws, lane16, i * CB + p * 1024);

    float P[KH];                 // operand registers of a hidden layer
    // hidden accumulators: they hold the bias of the layer about to run (row 0's c1 to start with)
    BlockAcc<TILE> hacc[NB];
#pragma unroll
    for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16, 128 + o * 128);

    bool bad_slot = false, bad_noise = false;
    for (int e = 0; e < args.n_evals; ++e) {
        const int row_byte = e * args.etab_stride * 4;
        HdrPtr hdr = (HdrPtr)(args.etab + (size_t)e * args.etab_stride);
        const float a_e = hdr->a, b_e = hdr->b;
        const uint32_t flags = hdr->flags;
        const int slot = hdr->slot;

        // stage input of the state, written down before the network runs
        float y[DREGS];
#pragma unroll
        for (int j = 0; j < R4; ++j) {
            f32x4 v = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (s < nslots) v += hdr->cin[s] * ks[(s * R4 + j) * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * j + i] = v[i];
        }
        if (col_live) {
            float* const ro = rec0 + (long long)e * rec_row;
#pragma unroll
            for (int r = 0; r < DREGS; ++r) {
                const int d = feat_of_reg(TILE, r, qd);
                if (d < D) ro[d] = y[r];
            }
        }
        float op[K1];            // first-layer operand [y | cond]
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = y[r];
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = CREGS > 0 ? cnd[r - DREGS] : 0.f;

        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last block,
        // activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        BiasBlk<TILE> bias[2];
        ActGroup ag[12];
        // stages of the previous layer's parked block: group gi starts at slot gi*(16*PHYS/GPB)
        auto prev_slot = [&](auto mm) __attribute__((always_inline)) {
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
                    act_stage<false, 0, k>(ag[gi], &P[(NB - 1) * RB + 4 * gi], false, 0, aspec);
                }
            });
        };
        // stages of this layer's own blocks 0 .. NB-2 (geometry G), hung on slot M
        auto own_slot = [&](auto geom, auto mm, const BlockAcc<TILE> (&acc)[NB]) __attribute__((always_inline)) {
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
                    act_stage<false, 0, k>(ag[4 + id % 8], &P[blk * RB + 4 * gi], false, 0, aspec);
                }
            });
        };
        auto refill = [&](int byte, auto ob) {
            constexpr int o = decltype(ob)::value;
            if constexpr (o >= 2) hacc[o - 2] = load_bias_acc<TILE>(ws, q16, byte + (o - 2) * 128);
        };
        auto park_and_refill = [&](int byte, const BlockAcc<TILE>& acc) {
#pragma unroll
            for (int r = 0; r < RB; ++r) pend[r] = acc.reg(r);
            if constexpr (NB >= 2) hacc[NB - 2] = load_bias_acc<TILE>(ws, q16, byte + (NB - 2) * 128);
            hacc[NB - 1] = load_bias_acc<TILE>(ws, q16, byte + (NB - 1) * 128);
        };
        using G1 = GeomTag<TILE, K1, NB>;
        using GH = GeomTag<TILE, KH, NB>;

        {
            const int nbyte = (int)(L.bias_off_hid(0) * 4);
            run_layer<TILE, RING, K1, NB, false, false>(
                ring, ws, lane16, 0, op, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(G1{}, mm, acc); },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        for (int l = 0; l < NH - 1; ++l) {
            const int sbyte = L.chunk_off_hid(l) * CB;
            const int nbyte = (int)(L.bias_off_hid(l + 1) * 4);
            run_layer<TILE, RING, KH, NB, false, false>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(mm);
                    own_slot(GH{}, mm, acc);
                },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        // the hidden accumulators are idle from here on: fetch the next row's c1 (a row past the table reads as zeros)
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16, row_byte + args.etab_stride * 4 + 128 + o * 128);
        float fnet[DREGS];       // NET(y, c)
        {
            BlockAcc<TILE> oacc[NOB_OUT];
            constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
            // the ring wraps to the first layer of the next row
            run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
                ring, ws, lane16, out_sbyte, P, oacc,
                [&](auto ob) {
                    constexpr int o = decltype(ob)::value;
                    bias[o & 1] = load_bias<TILE>(ws, q16, out_bias_byte + o * 128);
                },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NOB_OUT]) {
                    prev_slot(mm);
                    if constexpr (NOB_OUT > 1) {          // finished output blocks: plain bias add
                        constexpr LayerGeom GO = layer_geom(KH, NOB_OUT, RB / 4);
                        constexpr int M = decltype(mm)::value;
                        constexpr int id = act_group_at(GO, T::PHYS, GPB, M, 0);
                        if constexpr (id >= 0) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                constexpr int blk = id / GPB, r0 = 4 * (id % GPB);
                                if constexpr (blk * RB + r0 < DREGS) fnet[blk * RB + r0 + i] = acc[blk].reg(r0 + i) + bias[blk & 1].reg(r0 + i);
                            }
                        }
                    }
                },
                [&](const BlockAcc<TILE>& acc) {
#pragma unroll
                    for (int r = 0; r < RB; ++r)
                        if ((NOB_OUT - 1) * RB + r < DREGS) fnet[(NOB_OUT - 1) * RB + r] = acc.reg(r) + bias[(NOB_OUT - 1) & 1].reg(r);
                },
                0);
        }

        // ---- the right-hand side and the stage bookkeeping -------------------------------------------------------------------
        float rhs[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) rhs[r] = __builtin_fmaf(a_e, y[r], b_e * fnet[r]);
        const bool slot_ok = (unsigned)slot < (unsigned)nslots;
        bad_slot |= !slot_ok;
        if (slot_ok) {
#pragma unroll
            for (int j = 0; j < R4; ++j)
                ks[(slot * R4 + j) * 64] = f32x4{rhs[4 * j], rhs[4 * j + 1], rhs[4 * j + 2], rhs[4 * j + 3]};
        }
        if (flags & 1u) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                f32x4 v = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
#pragma unroll
                for (int s = 0; s < kSlots; ++s)
                    if (s < nslots) v += hdr->cout[s] * ks[(s * R4 + j) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[4 * j + i] = v[i];
            }
        }
        bad_noise |= (flags & 2u) != 0;            // a noise row is not part of the recorded map: left out, and reported
    }

    // ---- epilogue: the final state -----------------------------------------------------------------------------------------
    bool bad = false;
    if (col_live) {
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            if (d < D) {
#pragma clang fp contract(off)      // x * scale + shift as two roundings, like the reference's torch expression
                float v = x[r];
                bad |= (v != v);
                if (args.out_scale) v = v * args.out_scale[d];
                if (args.out_shift) v = v + args.out_shift[d];
                args.x_out[sample * D + d] = v;
            }
        }
    }
    if (args.status && __any(bad)) {
        if (lane == 0) atomicOr(args.status, kStatusNaN);
    }
    if (args.status && bad_slot) {
        if (lane == 0) atomicOr(args.status, kStatusBadSlot);
    }
    if (args.status && bad_noise) {
        if (lane == 0) atomicOr(args.status, kStatusNoiseRow);
    }
}

template <int TILE, int H, int DREGS, int CREGS, int RING>
__global__ __launch_bounds__(64) void mlp_dadj_kernel(const KernelArgs args)
{
    static_assert(kChunkPad % RING == 0, "ring must divide the chunk padding");
    typedef Tile<TILE> T;
    constexpr int NB = H / 32;                       // logical blocks per hidden layer
    constexpr int RB = T::RB;                        // registers per logical block
    constexpr int GPB = RB / 4;                      // activation groups per logical block
    constexpr int K1 = DREGS + CREGS;                // operand registers of net A's first layer = output registers of net B
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);     // output blocks of net A
    constexpr int NOB_T = blocks_for_regs(TILE, K1);          // output blocks of net B
    constexpr int KH = NB * RB;                      // operand registers of a hidden layer
    constexpr int R4 = DREGS / 4;

    if (args.gate && *(const volatile int*)args.gate == 0) return;

    const int lane = threadIdx.x & 63;
    const int qd = lane >> T::SHIFT;                 // lane group (k index of the MFMA operands)
    const int col = lane & (TILE - 1);
    const int lane16 = lane * 16;
    const int q16 = qd * 16;
    const long long wave = (long long)blockIdx.x;    // one tile per workgroup, one wavefront per workgroup
    const int D = args.dim, C = args.cond_dim;
    const ActSpec aspec = {0.f, 0.f, 0.f, 0};

    // ---- column roles: value column + n_tangent cotangent columns per sample ------------------------------------------
    const int ncol = 1 + args.n_tangent;
    const int spw = TILE / ncol;                     // samples per tile
    int s_in_wave = col / ncol;
    int role = col - s_in_wave * ncol;               // 0 = value column, k >= 1 = cotangent k - 1
    bool col_live = true;
    bool stasher = true;                             // a value lane that owns a place in the stash
    if (s_in_wave >= spw) { s_in_wave = 0; role = 0; col_live = false; stasher = false; }
    const bool is_cot = role != 0;
    stasher = stasher && !is_cot;
    long long sample = wave * spw + s_in_wave;
    if (sample >= args.batch) { sample = args.batch - 1; col_live = false; }
    const int q16b = is_cot ? 0x7ffffff0 : q16;      // bias offset of net A: out of range = zero on the cotangent columns

    // ---- cotangent lanes: xb = w * out_scale, gamma = 0; value lanes: zeros -------------------------------------------------
    float xb[DREGS];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) xb[r] = 0.f;
    if (is_cot) {
        const float* const wp = args.probe + (sample * args.n_tangent + (role - 1)) * D;      // cotangent_in
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            float v = 0.f;
            if (d < D) {
                v = wp[d];
                if (args.out_scale) v = v * args.out_scale[d];
            }
            xb[r] = v;
        }
    }
    float gam[CREGS > 0 ? CREGS : 1];
#pragma unroll
    for (int r = 0; r < (CREGS > 0 ? CREGS : 1); ++r) gam[r] = 0.f;
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, is_cot, r);
    }
    // value lanes: the recorded stage state of row e is at rec0 + e * rec_row (record_in)
    const float* const rec0 = args.k1_in + sample * D;
    const long long rec_row = args.batch * D;
    const int E = args.n_evals;
    float ynext[DREGS];          // y of the row about to run, loaded a row ahead
#pragma unroll
    for (int r = 0; r < DREGS; ++r) {
        const int d = feat_of_reg(TILE, r, qd);
        ynext[r] = (!is_cot && d < D && E > 0) ? rec0[(long long)(E - 1) * rec_row + d] : 0.f;
    }

    // ---- LDS: adjoint slots (each lane its own words), then the slope stash ---------------------------------------------
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + lane;
    const int nslots = args.tangent_first;           // stage slots kept (1 .. kSlots: the launcher's)
    f32x4* const stash = lds_slots + (size_t)nslots * R4 * 64;      // [n_hidden][KH / 4][NQ * spw] groups of 4 slopes
    const int srow = T::NQ * spw;
    const int sidx = qd * spw + s_in_wave;           // the place of (lane group, sample): written by its value lane
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        if (s < nslots) {
#pragma unroll
            for (int j = 0; j < R4; ++j) ks[(s * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

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

        // 1. the transpose of the step's end: every kept slot takes cout[s] xb
        if (flags & 1u) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                const f32x4 v = f32x4{xb[4 * j], xb[4 * j + 1], xb[4 * j + 2], xb[4 * j + 3]};
#pragma unroll
                for (int s = 0; s < kSlots; ++s)
                    if (s < nslots) ks[(s * R4 + j) * 64] += hdr->cout[s] * v;
            }
        }
        // 2. the cotangent of this row's right-hand side leaves its slot
        const bool slot_ok = (unsigned)slot < (unsigned)nslots;
        bad_slot |= !slot_ok;
        float rb[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) rb[r] = 0.f;
        if (slot_ok) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                const f32x4 v = ks[(slot * R4 + j) * 64];
                ks[(slot * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) rb[4 * j + i] = v[i];
            }
        }

        float op[K1];            // first-layer operand: net A [y_e | cond] on the value column, net B [rb | 0] on the others
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = ynext[r];      // (zero on the cotangent columns)
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = CREGS > 0 ? cnd[r - DREGS] : 0.f;
        // the recorded state of the row that runs next: in flight behind this row's networks
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            ynext[r] = (!is_cot && d < D) ? rec0[(long long)prev_row * rec_row + d] : 0.f;
        }

        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last block,
        // activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        ActGroup ag[12];
        // net A: SiLU on every lane; the value lanes park SiLU' of hidden layer `lyr`, group `grp` of its KH / 4
        auto park_slope = [&](const ActGroup& g, int lyr, int grp) __attribute__((always_inline)) {
            f32x4 d;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // silu'(a) = s (1 + a (1 - s)),  s = sigmoid(a)
                const float w = __builtin_fmaf(-g.pre[i], g.r[i], g.pre[i]);
                d[i] = __builtin_fmaf(g.r[i], w, g.r[i]);
            }
            if (stasher) stash[(size_t)(lyr * (KH / 4) + grp) * srow + sidx] = d;
        };
        // net B: the cotangent of a pre-activation = the cotangent of the activation times the stashed slope
        auto pull_stage = [&](auto kk, ActGroup& g, float* dst, int lyr, int grp) __attribute__((always_inline)) {
            constexpr int k = decltype(kk)::value;
            if constexpr (k == 3) {
                const f32x4 d = stash[(size_t)(lyr * (KH / 4) + grp) * srow + sidx];
#pragma unroll
                for (int i = 0; i < 4; ++i) g.r[i] = d[i];
            } else if constexpr (k == 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[i] = g.pre[i] * g.r[i];
            }
        };
        // stages of the previous layer's parked block (slope layer `lyr`): group gi starts at slot gi*(16*PHYS/GPB)
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
                        act_stage<false, 0, k>(ag[gi], &P[(NB - 1) * RB + 4 * gi], false, 0, aspec);
                        if constexpr (k == 3) park_slope(ag[gi], lyr, (NB - 1) * GPB + gi);
                    }
                }
            });
        };
        // stages of this layer's own blocks 0 .. NB-2 (geometry G; slope layer `lyr`), hung on slot M
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
                        act_stage<false, 0, k>(ag[4 + id % 8], &P[blk * RB + 4 * gi], false, 0, aspec);
                        if constexpr (k == 3) park_slope(ag[4 + id % 8], lyr, id);
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

        // ==== net A at the recorded state: the slopes of every hidden layer, parked on the way =================================
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
            // the output layer's place in the stream: its slots activate the last hidden block and park its slopes, and the
            // ring moves on to net B's first layer.  NET(y, c) itself is not needed: nobody reads oacc.
            BlockAcc<TILE> oacc[NOB_OUT];
            constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
            run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
                ring, ws, lane16, out_sbyte, P, oacc, [&](auto) {},
                [&](auto mm, const BlockAcc<TILE> (&)[NOB_OUT]) { prev_slot(NET_A, mm, NH - 1); },
                [&](const BlockAcc<TILE>&) {}, sub_bytes);
        }
        // every slope of this row is parked before a cotangent lane reads one (one wavefront: program order of its DS
        // instructions; the fence keeps the compiler from moving them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ==== net B: the transposed network on the cotangent columns ===========================================================
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = is_cot ? rb[r] : 0.f;
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

        // 3. the cotangent of the stage state and of the conditional inputs (zero on the value column)
        float yb[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const float jt = tacc[r / RB].reg(r % RB);                       // (J_net^T rb)[feature of register r]
            yb[r] = is_cot ? __builtin_fmaf(a_e, rb[r], b_e * jt) : 0.f;
        }
        if constexpr (CREGS > 0) {
#pragma unroll
            for (int r = DREGS; r < K1; ++r) {
                const float jc = tacc[r / RB].reg(r % RB);                   // ((dNET/dc)^T rb)[conditional feature of register r - DREGS]
                gam[r - DREGS] = is_cot ? __builtin_fmaf(b_e, jc, gam[r - DREGS]) : 0.f;
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

    // ---- epilogue: the cotangents ---------------------------------------------------------------------------------------------
    if (col_live && is_cot) {
        const long long row = sample * args.n_tangent + (role - 1);
        float* const gx = args.dlogp_out + row * D;                          // cot_x_out
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
            if (args.jac_out) {                                              // cot_cond_out
                float* const gc = args.jac_out + row * C;
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
