// ff_mlp_pullsel.hpp -- the pull-back unit of ff_mlp_pull.hpp whose table rows choose between TWO networks (gfx950).
//
// The symplectic flows' leapfrog (solvers.plan_leapfrog; ff_mlp_pair.hpp SELECT) is a sequence of shears: a row moves one half
// of the joint state [q | p] by w f(other half, c, t) and leaves the other half bitwise alone.  The transpose of such a row is
//     lambda_q = lambda_q',   lambda_p = lambda_p' + w J_f(p)^T lambda_q',   gamma += w (df/dc)^T lambda_q'
// and because the network's input half is unchanged by the row, the backward sweep can recompute f from the state it holds,
// un-shear with q = q' - w f(p) and take the slopes for J^T from that same evaluation.  That is the row program of
// mlp_pull_kernel on the table of the REVERSED grid: the value column retraces the state, net A parks SiLU'(z), net B runs
// the transposed network on the cotangent columns.  On shear rows the retracing adjoint is the exact discrete adjoint of the
// forward leapfrog (to rounding in the retraced state); nothing is recorded.
//
// What differs from mlp_pull_kernel: a row runs ONE network pair -- net A forward plus net B transposed of mlp_p if its flag
// word has FF_ROW_NET_B, of mlp_q otherwise.  The weight stream holds two pull packs back to back, [A_q | B_q | A_p | B_p]
// (ff_mlp_pull_select_wpack): each is what ff_mlp_pull_wpack makes of that network embedded in the whole joint state exactly as
// ff_mlp_pair_wpack embeds it (mlp_q: state columns on the p half, output rows 0..D-1; mlp_p: columns on the q half, rows
// D..2D-1, output weights and bias negated).  The row's pack base is (flags & FF_ROW_NET_B) ? bytes of one pull pack : 0, read
// through the bounds-checked table stream as mlp_pair_kernel's row_pack does: the row after the last reads as zeros.  The
// ring's wrap at net B's output layer and the pre-load of the next c1 target the NEXT row's network, whichever that is (rows
// need not alternate).  Rows carry only their own network's c1: stride FF_ROW_HDR + width.  gamma accumulates from both
// networks, because both read the conditional.
//
// Everything else is the pull kernel's, line for line: 1 + K columns per sample, value lanes [y | 0], cotangent lanes
// [alpha | gamma], the stash, the two fence / wave-barrier pairs, the stage algebra with cin / cout, the affine maps, gate, the
// status word, FF_STATUS_BAD_SLOT, FF_STATUS_NOISE_ROW, the KernelArgs fields a pull launch reuses (probe = cotangent_in,
// dlogp_out = cot_x_out, jac_out = cot_cond_out, tangent_first = stage slots kept), one wavefront per workgroup, the LDS
// formula.  A leapfrog table names slot 0 only: one stage slot.
#pragma once
#include "ff_mlp_ode.hpp"

namespace ff {

constexpr uint32_t kPullRowNetB = 4u;                 // FF_ROW_NET_B

template <int TILE, int H, int DREGS, int CREGS, int RING>
__global__ __launch_bounds__(64) void mlp_pullsel_kernel(const KernelArgs args)
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
    constexpr int R4 = DREGS / 4, R4T = K1 / 4;

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

    // ---- state: value lanes [y | 0], cotangent lanes [alpha | gamma] -------------------------------------------------
    float x[K1];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) x[r] = state_reg<TILE>(args, sample, qd, is_cot, role, r);
    if (is_cot) {
        const float* const wp = args.probe + (sample * args.n_tangent + (role - 1)) * D;      // cotangent_in
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            float v = 0.f;
            if (d < D) {
                v = wp[d];
                if (args.in_scale) v = v * args.in_scale[d];
            }
            x[r] = v;
        }
    }
#pragma unroll
    for (int r = DREGS; r < K1; ++r) x[r] = 0.f;
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, is_cot, r);
    }

    // ---- LDS: stage slots (each lane its own words), then the slope stash -----------------------------------------------
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + lane;
    const int nslots = args.tangent_first;           // stage slots kept (1 .. kSlots: the launcher's)
    f32x4* const stash = lds_slots + (size_t)nslots * R4T * 64;     // [n_hidden][KH / 4][NQ * spw] groups of 4 slopes
    const int srow = T::NQ * spw;
    const int sidx = qd * spw + s_in_wave;           // the place of (lane group, sample): written by its value lane
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        if (s < nslots) {
#pragma unroll
            for (int j = 0; j < R4T; ++j) ks[(s * R4T + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    const Layout L = make_layout(TILE, H, DREGS, CREGS, args.n_hidden);
    // net B's layout: an ordinary network with K1 state registers and no conditional ones -- the same first-layer and
    // hidden geometry as net A (the chunk offsets below serve both), NOB_T output blocks
    const Layout LT = make_layout(TILE, H, K1, 0, args.n_hidden);
    constexpr int CB = 1024 * T::PHYS;               // bytes per chunk
    const int sub_bytes = (int)(L.total_floats * 4); // net B's pack starts here, within a pull pack
    const int pack_bytes = (int)((L.total_floats + LT.total_floats) * 4);      // one pull pack: mlp_p's starts here
    const Stream ws = make_stream(args.wpack, args.wpack_floats);
    const Stream ts = make_stream(args.etab, (long long)args.n_evals * args.etab_stride);
    const int out_sbyte = L.chunk_off_out() * CB;    // (== LT.chunk_off_out() * CB)
    const int out_bias_byte = (int)(L.bias_off_out() * 4);
    const int NH = args.n_hidden;
    // the pull pack (byte offset in the weight stream) of the network that table row `e` runs.  Read through the bounds-checked
    // table stream: the row after the last one reads as zeros (mlp_q), whatever lies behind the buffer.
    auto row_pack = [&](int e) __attribute__((always_inline)) {
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__builtin_amdgcn_raw_buffer_load_b32(ts.rsrc, 0, e * args.etab_stride * 4 + 12, 0));      // RowHdr::flags
        return (f & kPullRowNetB) ? pack_bytes : 0;
    };
    int sb_row = row_pack(0);                        // this row's network; the ring and hacc already hold its head

    f32x4 ring[RING][T::PHYS];
#pragma unroll
    for (int i = 0; i < RING; ++i)
#pragma unroll
        for (int p = 0; p < T::PHYS; ++p) ring[i][p] = sload(ws, lane16, sb_row + i * CB + p * 1024);

    float P[KH];                 // operand registers of a hidden layer
    // hidden accumulators: net A's hold the bias of the layer about to run (row 0's c1 to start with); net B's start from zero
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
        const int sb_next = row_pack(e + 1);         // the NEXT row's network: prefetch target of net B's output layer
        const int sb_b = sb_row + sub_bytes;         // this row's transposed network

        // stage input of the state / of alpha (gamma enters no right-hand side)
        float y[DREGS];
#pragma unroll
        for (int j = 0; j < R4; ++j) {
            f32x4 v = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
#pragma unroll
            for (int s = 0; s < kSlots; ++s)
                if (s < nslots) v += hdr->cin[s] * ks[(s * R4T + j) * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * j + i] = v[i];
        }
        float op[K1];            // first-layer operand: net A [y | cond] on the value column, net B [alpha | 0] on the others
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = is_cot ? 0.f : y[r];
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = CREGS > 0 ? cnd[r - DREGS] : 0.f;

        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last block,
        // activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        BiasBlk<TILE> bias[2];
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

        // ==== net A: the forward network (mlp_ode_kernel's layers), slopes parked on the way ===============================
        {
            const int nbyte = sb_row + (int)(L.bias_off_hid(0) * 4);
            run_layer<TILE, RING, K1, NB, false, false>(
                ring, ws, lane16, sb_row, op, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(NET_A, G1{}, mm, acc, 0); },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        for (int l = 0; l < NH - 1; ++l) {
            const int sbyte = sb_row + L.chunk_off_hid(l) * CB;
            // (after the last hidden layer nothing reads hacc's bias: net B's first layer starts from zero)
            const int nbyte = sb_row + (int)(L.bias_off_hid(l + 1) * 4);
            run_layer<TILE, RING, KH, NB, false, false>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto ob) { refill(nbyte, ob); },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(NET_A, mm, l);
                    own_slot(NET_A, GH{}, mm, acc, l + 1);
                },
                [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
        }
        float fnet[DREGS];       // NET(y, c): kept across net B
        {
            BlockAcc<TILE> oacc[NOB_OUT];
            constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
            // the ring moves on to net B's first layer
            run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
                ring, ws, lane16, sb_row + out_sbyte, P, oacc,
                [&](auto ob) {
                    constexpr int o = decltype(ob)::value;
                    bias[o & 1] = load_bias<TILE>(ws, q16b, sb_row + out_bias_byte + o * 128);
                },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NOB_OUT]) {
                    prev_slot(NET_A, mm, NH - 1);
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
                sb_b);
        }
        // every slope of this row is parked before a cotangent lane reads one (one wavefront: program order of its DS
        // instructions; the fence keeps the compiler from moving them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ==== net B: the transposed network on the cotangent columns ===========================================================
#pragma unroll
        for (int r = 0; r < DREGS; ++r) op[r] = is_cot ? y[r] : 0.f;
#pragma unroll
        for (int r = DREGS; r < K1; ++r) op[r] = 0.f;
        run_layer<TILE, RING, K1, NB, false, true>(
            ring, ws, lane16, sb_b, op, hacc, [&](auto) {},
            [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(NET_B, G1{}, mm, acc, NH - 1); },
            [&](const BlockAcc<TILE>& acc) { park(acc); });
        for (int l = 0; l < NH - 1; ++l) {
            const int sbyte = sb_b + LT.chunk_off_hid(l) * CB;
            run_layer<TILE, RING, KH, NB, false, true>(
                ring, ws, lane16, sbyte, P, hacc, [&](auto) {},
                [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                    prev_slot(NET_B, mm, NH - 1 - l);
                    own_slot(NET_B, GH{}, mm, acc, NH - 2 - l);
                },
                [&](const BlockAcc<TILE>& acc) { park(acc); });
        }
        BlockAcc<TILE> tacc[NOB_T];
        // the hidden accumulators are idle from here on: fetch the next row's c1 (a row past the table reads as zeros)
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16b, row_byte + args.etab_stride * 4 + 128 + o * 128);
        // the ring wraps to net A's first layer of the next row's network
        run_layer<TILE, RING, KH, NOB_T, true, true>(
            ring, ws, lane16, sb_b + out_sbyte, P, tacc, [&](auto) {},
            [&](auto mm, const BlockAcc<TILE> (&)[NOB_T]) { prev_slot(NET_B, mm, 0); },
            [&](const BlockAcc<TILE>&) {}, sb_next);
        // the next row's net A overwrites the stash only after every read of this row
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- right-hand sides and stage bookkeeping -------------------------------------------------------------------------
        float rhs[K1];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const float jt = tacc[r / RB].reg(r % RB);                       // (J_net^T alpha)[feature of register r]
            const float v = __builtin_fmaf(a_e, y[r], b_e * (is_cot ? jt : fnet[r]));
            rhs[r] = is_cot ? -v : v;
        }
#pragma unroll
        for (int r = DREGS; r < K1; ++r) {
            const float jc = tacc[r / RB].reg(r % RB);                       // ((dNET/dc)^T alpha)[conditional feature of register r - DREGS]
            rhs[r] = is_cot ? -(b_e * jc) : 0.f;
        }
        const bool slot_ok = (unsigned)slot < (unsigned)nslots;
        bad_slot |= !slot_ok;
        if (slot_ok) {
#pragma unroll
            for (int j = 0; j < R4T; ++j)
                ks[(slot * R4T + j) * 64] = f32x4{rhs[4 * j], rhs[4 * j + 1], rhs[4 * j + 2], rhs[4 * j + 3]};
        }
        if (flags & 1u) {
#pragma unroll
            for (int j = 0; j < R4T; ++j) {
                f32x4 v = f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]};
#pragma unroll
                for (int s = 0; s < kSlots; ++s)
                    if (s < nslots) v += hdr->cout[s] * ks[(s * R4T + j) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[4 * j + i] = v[i];
            }
        }
        bad_noise |= (flags & 2u) != 0;            // a noise row has no adjoint form: left out, and reported
        sb_row = sb_next;
    }

    // ---- epilogue: the retraced state, the cotangents ---------------------------------------------------------------------
    bool bad = false;
    if (col_live && !is_cot) {
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
    if (col_live && is_cot) {
        const long long row = sample * args.n_tangent + (role - 1);
        float* const gx = args.dlogp_out + row * D;                          // cot_x_out
#pragma unroll
        for (int r = 0; r < DREGS; ++r) {
            const int d = feat_of_reg(TILE, r, qd);
            if (d < D) {
                float v = x[r];
                if (args.out_scale) v = v / args.out_scale[d];
                gx[d] = v;
            }
        }
        if constexpr (CREGS > 0) {
            if (args.jac_out) {                                              // cot_cond_out
                float* const gc = args.jac_out + row * C;
#pragma unroll
                for (int r = 0; r < CREGS; ++r) {
                    const int d = feat_of_reg(TILE, r, qd);
                    if (d < C) gc[d] = x[DREGS + r];
                }
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
