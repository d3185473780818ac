// ff_mlp_pushsel.hpp -- the push-forward unit of ff_mlp_ode.hpp whose table rows choose between TWO networks (gfx950).
//
// The symplectic flows' leapfrog (solvers.plan_leapfrog; ff_mlp_pair.hpp SELECT) is a sequence of shears: a row moves one half
// of the joint state [q | p] by w f(other half, c, t) and leaves the other half bitwise alone.  The forward-mode form of such a
// row is
//     dq' = dq + w (J_f(p) dp + df/dc dc),   dp' = dp          (or the kick, its mirror image)
// which is what the PUSH stage algebra of mlp_ode_kernel, rhs = a_e v + b_e J_net (v, c), computes on a select row (a_e = 0):
// the tangent columns run through the same weight operands as their value column, take SiLU'(pre of the value column) across
// lanes and keep their conditional part, and the select pack's structural zeros (zero rows and zero bias on the other half of
// the output) leave the other half of every tangent column bitwise alone, as they do for the value column.  What leaves in
// tangent_out is the derivative of the discrete leapfrog map, d z_out / d (z_in, cond) . tangent.
//
// The body is the one-wavefront PUSH path of mlp_ode_kernel with the SELECT row semantics of mlp_pair_kernel: a row runs ONE
// network -- mlp_p's pack, at byte offset sub_bytes of the weight stream, if its flag word has FF_ROW_NET_B, mlp_q's at 0
// otherwise -- and carries only that network's c1 (row stride FF_ROW_HDR + width).  The weight stream holds two forward packs
// back to back (ff_mlp_push_select_wpack), each what ff_mlp_wpack makes of that network embedded in [q | p] as ff_mlp_pair_wpack
// embeds it.  The row's pack is read through the bounds-checked table stream, as mlp_pair_kernel's row_pack is: the row after
// the last reads as zeros.  The weight ring's wrap at the output layer and the pre-load of the next c1 target the NEXT ROW's
// network, whichever that is (rows need not alternate).  The value column runs the FMA chains of mlp_pair_kernel<..., SELECT> on
// the 16-column tile: its state is that kernel's bit for bit.
//
// Left out: the cooperative twin, the wide variant, run-time activations (SiLU only), the divergence bookkeeping, jac_out,
// auxiliary outputs, k1_in and noise.  A noise row is reported through kStatusNoiseRow as the push units report it, a row
// naming a slot beyond kSlots through kStatusBadSlot.  Each wavefront owns its tile and its stage slots: no barrier, no
// inter-wave hazard.  Same KernelArgs, same column roles, same launch geometry as the push units (ff_mlp_ode_launch_push_select).
#pragma once
#include "ff_mlp_ode.hpp"

namespace ff {

constexpr uint32_t kPushRowNetB = 4u;                 // FF_ROW_NET_B

template <int TILE, int H, int DREGS, int CREGS, int WPS, int RING>
__global__ __launch_bounds__(256, WPS) void mlp_pushsel_kernel(const KernelArgs args)
{
    static_assert(kChunkPad % RING == 0, "ring must divide the chunk padding");
    typedef Tile<TILE> T;
    constexpr int NB = H / 32;                       // logical blocks per hidden layer
    constexpr int RB = T::RB;                        // registers per logical block
    constexpr int GPB = RB / 4;                      // activation groups per logical block
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);
    constexpr int K1 = DREGS + CREGS;
    constexpr int KH = NB * RB;                      // operand registers of a hidden layer
    constexpr int R4 = DREGS / 4;

    if (args.gate && *(const volatile int*)args.gate == 0) return;

    const int lane = threadIdx.x & 63;
    const int qd = lane >> T::SHIFT;                 // lane group (k index of the MFMA operands)
    const int col = lane & (TILE - 1);
    const int lane16 = lane * 16;
    const int q16 = qd * 16;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;      // tile index: one per wavefront
    const int D = args.dim;
    const ActSpec aspec = {0.f, 0.f, 0.f, 0};

    // ---- column roles: value column + n_tangent tangent columns per sample ----------------------------------------------
    const int ncol = 1 + args.n_tangent;
    const int samples_per_wave = TILE / ncol;
    int s_in_wave = col / ncol;
    int role = col - s_in_wave * ncol;               // 0 = value column, j >= 1 = tangent j - 1
    bool col_live = true;                            // column carries a sample that must be written back
    if (s_in_wave >= samples_per_wave) { s_in_wave = 0; role = 0; col_live = false; }
    const bool is_tangent = role != 0;
    const int value_lane_bytes = ((qd << T::SHIFT) | (s_in_wave * ncol)) * 4;
    long long sample = wave * samples_per_wave + s_in_wave;
    if (sample >= args.batch) { sample = args.batch - 1; col_live = false; }
    const int q16b = is_tangent ? 0x7ffffff0 : q16;  // bias offset: out of range = zero on the tangent columns

    // ---- state (value columns) / tangent vectors: a tangent column starts from its tangent's state part and keeps its
    // conditional part -------------------------------------------------------------------------------------------------------
    float x[DREGS];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) x[r] = state_reg<TILE>(args, sample, qd, is_tangent, role, r);
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, is_tangent, r);
    }
    if (is_tangent) {
#pragma unroll
        for (int r = 0; r < DREGS; ++r) x[r] = push_state_reg<TILE>(args, sample, qd, role, r);
        if constexpr (CREGS > 0) {
#pragma unroll
            for (int r = 0; r < CREGS; ++r) cnd[r] = push_cond_reg<TILE>(args, sample, qd, role, r);
        }
    }

    // stage slots in LDS, one set per wavefront (each lane only ever touches its own words, so no barrier is needed)
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + (size_t)(threadIdx.x >> 6) * kSlots * R4 * 64 + lane;
    init_stage_slots<TILE, DREGS, false, false>(args, ks, sample, qd, is_tangent, false);

    const Layout L = make_layout(TILE, H, DREGS, CREGS, args.n_hidden);
    constexpr int CB = 1024 * T::PHYS;               // bytes per chunk
    const int sub_bytes = (int)(L.total_floats * 4);   // one network's pack: mlp_p's starts here
    const Stream ws = make_stream(args.wpack, args.wpack_floats);
    const Stream ts = make_stream(args.etab, (long long)args.n_evals * args.etab_stride);
    // The pack (byte offset in the weight stream) of the network that table row `e` runs.  Read through the bounds-checked
    // table stream: the row after the last one reads as zeros (mlp_q), whatever lies behind the buffer.
    auto row_pack = [&](int e) __attribute__((always_inline)) {
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__builtin_amdgcn_raw_buffer_load_b32(ts.rsrc, 0, e * args.etab_stride * 4 + 12, 0));      // RowHdr::flags
        return (f & kPushRowNetB) ? sub_bytes : 0;
    };
    int sb_row = row_pack(0);                        // this row's network; the ring and hacc already hold its head
    const int out_sbyte = L.chunk_off_out() * CB;
    const int out_bias_byte = (int)(L.bias_off_out() * 4);

    // prefetch ring: the first RING chunks of the layer 1 of row 0's network
    f32x4 ring[RING][T::PHYS];
#pragma unroll
    for (int i = 0; i < RING; ++i)
#pragma unroll
        for (int p = 0; p < T::PHYS; ++p) ring[i][p] = sload(ws, lane16, sb_row + i * CB + p * 1024);

    float P[KH];                 // operand registers of a hidden layer
    // hidden accumulators: they hold the bias of the layer about to run (row 0's c1 to start with); tangent lanes fetch
    // through an out-of-range offset (q16b) and start from zero
    BlockAcc<TILE> hacc[NB];
#pragma unroll
    for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16b, 128 + o * 128);

    bool bad_slot = false, bad_noise = false;
    for (int e = 0; e < args.n_evals; ++e) {
        const int row_byte = e * args.etab_stride * 4;
        HdrPtr hdr = (HdrPtr)(args.etab + (size_t)e * args.etab_stride);
        const float a_e = hdr->a, b_e = hdr->b;
        const uint32_t flags = hdr->flags;
        const int slot = hdr->slot;
        const int sb = sb_row;                       // this row's pack in the weight stream
        const int sb_next = row_pack(e + 1);         // the NEXT row's network (prefetch target of the output layer)

        // stage input  y = x + sum_s cin[s] * k[s]
        float y[K1];
#pragma unroll
        for (int j = 0; j < R4; ++j) {
            f32x4 v = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
#pragma unroll
            for (int s = 0; s < kSlots; ++s) v += hdr->cin[s] * ks[(s * R4 + j) * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * j + i] = v[i];
        }
        if constexpr (CREGS > 0) {
#pragma unroll
            for (int r = 0; r < CREGS; ++r) y[DREGS + r] = cnd[r];
        }

        float net[NOB_OUT * RB];
        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last block,
        // activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        BiasBlk<TILE> bias[2];   // output layer only (tangent lanes read zeros through q16b)
        ActGroup ag[12];         // in-flight groups: [0,4) parked block of the previous layer, 4 + id % 8 own blocks
        auto prev_slot = [&](auto mm) {
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
                    act_stage<true, 0, k>(ag[gi], &P[(NB - 1) * RB + 4 * gi], is_tangent, value_lane_bytes, aspec);
                }
            });
        };
        auto own_slot = [&](auto geom, auto mm, const BlockAcc<TILE> (&acc)[NB]) {
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
                    act_stage<true, 0, k>(ag[4 + id % 8], &P[blk * RB + 4 * gi], is_tangent, value_lane_bytes, aspec);
                }
            });
        };
        auto refill = [&](int byte, auto ob) {
            constexpr int o = decltype(ob)::value;
            if constexpr (o >= 2) hacc[o - 2] = load_bias_acc<TILE>(ws, q16b, byte + (o - 2) * 128);
        };
        auto park_and_refill = [&](int byte, const BlockAcc<TILE>& acc) {
#pragma unroll
            for (int r = 0; r < RB; ++r) pend[r] = acc.reg(r);
            if constexpr (NB >= 2) hacc[NB - 2] = load_bias_acc<TILE>(ws, q16b, byte + (NB - 2) * 128);
            hacc[NB - 1] = load_bias_acc<TILE>(ws, q16b, byte + (NB - 1) * 128);
        };
        // ---- layer 1: [y | cond] -> H, bias c1 of this row's network (already in hacc) ------------------------------------
        {
            using G1 = GeomTag<TILE, K1, NB>;
            const int nbyte = sb + (int)(L.bias_off_hid(0) * 4);
            run_layer<TILE, RING, K1, NB, false, false>(
                ring, ws, lane16, sb, y, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(G1{}, mm, acc); },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        // ---- hidden -> hidden ---------------------------------------------------------------------------------------------
        for (int l = 0; l < args.n_hidden - 1; ++l) {
            using GH = GeomTag<TILE, KH, NB>;
            const int sbyte = sb + L.chunk_off_hid(l) * CB;
            // next layer's bias; after the last hidden layer nothing reads hacc before the output layer replaces it with
            // the next row's c1, so whatever this fetches then is ignored
            const int nbyte = sb + (int)(L.bias_off_hid(l + 1) * 4);
            run_layer<TILE, RING, KH, NB, false, false>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(mm);
                    own_slot(GH{}, mm, acc);
                },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        // ---- output layer -------------------------------------------------------------------------------------------------
        // the hidden accumulators are idle from here to the next row's first layer: fetch its only c1 now (a row past the
        // table reads as zeros); the ring moves on to the layer 1 of the next row's network
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16b, row_byte + args.etab_stride * 4 + 128 + o * 128);
        BlockAcc<TILE> oacc[NOB_OUT];
        constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
        run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
            ring, ws, lane16, sb + out_sbyte, P, oacc,
            [&](auto ob) {
                constexpr int o = decltype(ob)::value;
                bias[o & 1] = load_bias<TILE>(ws, q16b, sb + out_bias_byte + o * 128);
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
                            net[blk * RB + r0 + i] = acc[blk].reg(r0 + i) + bias[blk & 1].reg(r0 + i);
                        }
                    }
                }
            },
            [&](const BlockAcc<TILE>& acc) {
#pragma unroll
                for (int r = 0; r < RB; ++r)
                    net[(NOB_OUT - 1) * RB + r] = acc.reg(r) + bias[(NOB_OUT - 1) & 1].reg(r);
            },
            sb_next);

        // ---- RHS and stage bookkeeping: the tangent columns take the value column's stage algebra ------------------------
        float rhs[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) rhs[r] = __builtin_fmaf(a_e, y[r], b_e * net[r]);
        // (a row naming a slot beyond the kSlots on chip is refused: nothing is stored, the status word says so)
        const bool slot_ok = (unsigned)slot < (unsigned)kSlots;
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
                for (int s = 0; s < kSlots; ++s) v += hdr->cout[s] * ks[(s * R4 + j) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[4 * j + i] = v[i];
            }
        }
        sb_row = sb_next;
        bad_noise |= (flags & 2u) != 0;            // a noise row has no tangent form: left out, and reported
    }

    // ---- epilogue: final state from the value columns, every live tangent column its own vector ------------------------
    bool bad = false;
    if (col_live && !is_tangent) {
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
    // through the linear part of the output map (no shift: it is a derivative)
    if (col_live && is_tangent) {
        float* const tp = args.tangent_out + (sample * args.n_tangent + (role - 1)) * D;
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            if (d < D) {
                float v = x[r];
                if (args.out_scale) v = v * args.out_scale[d];
                tp[d] = v;
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

} // namespace ff
