// ff_mlp_pair.hpp -- fused integrator of a right-hand side made of TWO networks of one shape (gfx950).
//
// One launch integrates  dy/ds = a_e * y + b_e * (NET_A(y, cond; c1A_e) + NET_B(y, cond; c1B_e))  for every sample over
// all evaluation rows e.  The symplectic flows (flowfusion_amd/symplectic.py; reference flowfusion/symplectic.py:80-122)
// are such a right-hand side: v = [mlp_q(p, cond, t), -mlp_p(q, cond, t)].  The structure lives in the host packer
// (ff_mlp_pair_wpack): NET_A is mlp_q with its state columns on the p half and zeros on the q half, writing output rows
// 0..D-1; NET_B is mlp_p with its columns on the q half, writing rows D..2D-1 with its output weights and bias negated.
// Each half is an ordinary network over the whole state, packed as ff_mlp_wpack packs one, and the two packs lie back to
// back.  An evaluation row holds FF_ROW_HDR header words, then c1 of net A, then c1 of net B (width words each).
//
// The body is the one-wavefront path of mlp_ode_kernel (ff_mlp_ode.hpp), state-only (the divergence of such a field is
// zero by construction, so no tangent columns) and SiLU only, with the network part run twice per evaluation: net A's
// layers, then net B's, whose output is added to A's.  The weight ring runs across the A -> B boundary (A's output layer
// prefetches B's first chunks) and B's output layer wraps to A's first layer of the next evaluation, so the pair costs
// what one network of twice the depth costs; the stage bookkeeping runs once, after B.
//
// COOP (small batches; widths whose layers split four ways): one tile per WORKGROUP, as in mlp_ode_kernel<..., COOP>.  Each of
// the four wavefronts computes NB / 4 logical blocks of every hidden layer of net A, then of net B, trading activations through
// two alternating LDS buffers with one barrier per layer; both output layers are computed by every wavefront; wavefront 0
// writes the outputs.  Same packed weights, same table, the same fp32 FMA chain per output row: bitwise the one-wavefront
// kernel's results.  The stage slots are ONE copy shared by the four wavefronts, which brings three hazards:
//   * the zero fill of the slots needs a barrier before k1_in is stored (a late wavefront would wipe it: init_stage_slots);
//   * the exchange-buffer index alternates over the whole launch, not per evaluation or per network;
//   * net A's output is NOT parked in the row's stage slot while net B runs (no barrier lies between a fast wavefront's store
//     of the finished right-hand side into that slot and a slow wavefront's read of the parked value): it stays in registers.
// tests/test_gpu_symplectic_skew.py holds a wavefront back at each of the three (ff_skew.h; -DFF_DEBUG_UNFIX parks net A in
// the shared slot again, so that the test can see the third go wrong).
//
// SELECT (row-select variant, ff_mlp_pair_select_plan): a row runs ONE network, chosen by the row -- net B if its flag word
// has FF_ROW_NET_B, net A otherwise -- and carries only that network's c1 (row stride FF_ROW_HDR + width).  The other half
// of the network output is exact zero (zero rows and zero bias in the pack), so with a_e = 0 the row's right-hand side and
// its STEP_END update move one half of the state and leave the other bitwise alone: the shears of a kick-drift-kick
// leapfrog (solvers.plan_leapfrog).  Same packed weights, same KernelArgs, same stage bookkeeping.  The weight ring's wrap
// at the output layer and the pre-load of the next c1 target the NEXT ROW's network, whichever that is (rows need not
// alternate): its flag word is read through the bounds-checked table stream, so the row after the last reads as zeros.
// The cooperative SELECT twin shares the zero-fill barrier and the launch-wide exchange-buffer alternation with the pair
// twin; the third hazard does not exist here: there is no second network per row, so nothing is parked.
#pragma once
#include "ff_mlp_ode.hpp"

namespace ff {

constexpr uint32_t kRowNetB = 4u;                     // FF_ROW_NET_B (SELECT rows)

template <int TILE, int H, int DREGS, int CREGS, int WPS, int RING, bool COOP = false, bool SELECT = false>
__global__ __launch_bounds__(256, WPS) void mlp_pair_kernel(const KernelArgs args)
{
    static_assert(kChunkPad % RING == 0, "ring must divide the chunk padding");
    static_assert(!COOP || (H / 32) % 4 == 0, "the cooperative twin splits the blocks of a layer four ways");
    typedef Tile<TILE> T;
    constexpr int NB = H / 32;                       // logical blocks per hidden layer
    constexpr int RB = T::RB;                        // registers per logical block
    constexpr int GPB = RB / 4;                      // activation groups per logical block
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);
    constexpr int K1 = DREGS + CREGS;
    constexpr int KH = NB * RB;                      // operand registers of a hidden layer
    constexpr int R4 = DREGS / 4;
    constexpr int NSUB = SELECT ? 1 : 2;             // networks per evaluation row

    if (args.gate && *(const volatile int*)args.gate == 0) return;

    const int lane = threadIdx.x & 63;
    const int qd = lane >> T::SHIFT;
    const int col = lane & (TILE - 1);
    const int lane16 = lane * 16;
    const int q16 = qd * 16;
    // tile index: one per wavefront, or one per workgroup in the cooperative twin
    const long long wave = COOP ? (long long)blockIdx.x : (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    [[maybe_unused]] const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // wavefront of the workgroup
    const int D = args.dim;
    const ActSpec aspec = {0.f, 0.f, 0.f, 0};

    long long sample = wave * TILE + col;
    bool col_live = true;
    if (sample >= args.batch) { sample = args.batch - 1; col_live = false; }

    float x[DREGS];
#pragma unroll
    for (int r = 0; r < DREGS; ++r) x[r] = state_reg<TILE>(args, sample, qd, false, 0, r);
    float cnd[CREGS > 0 ? CREGS : 1];
    if constexpr (CREGS > 0) {
#pragma unroll
        for (int r = 0; r < CREGS; ++r) cnd[r] = cond_reg<TILE>(args, sample, qd, false, r);
    }

    // Runge-Kutta stage slots in LDS, one set per wavefront (each lane touches only its own words); the cooperative twin
    // keeps one copy (its four wavefronts hold the same tile and store the same values), followed by two exchange buffers
    extern __shared__ __attribute__((aligned(16))) f32x4 lds_slots[];
    f32x4* const ks = lds_slots + (size_t)(COOP ? 0 : (threadIdx.x >> 6)) * kSlots * R4 * 64 + lane;
    [[maybe_unused]] f32x4* const exch = lds_slots + (size_t)kSlots * R4 * 64 + lane;      // COOP: 2 x (KH / 4) x 64 words of 16 bytes
    // zero fill; all of the twin's fills before anybody stores the caller's first stage (init_stage_slots, ff_ode_frame.hpp)
    init_stage_slots<TILE, DREGS, COOP, COOP>(args, ks, sample, qd, false, wv == kSkewWave);

    const Layout L = make_layout(TILE, H, DREGS, CREGS, args.n_hidden);
    constexpr int CB = 1024 * T::PHYS;               // bytes per chunk
    const int sub_bytes = (int)(L.total_floats * 4);   // one network's pack: net B's starts here
    const Stream ws = make_stream(args.wpack, args.wpack_floats);
    const Stream ts = make_stream(args.etab, (long long)(args.n_evals + (args.n_aux > 0 ? 2 : 0)) * args.etab_stride);
    // SELECT: the pack (byte offset in the weight stream) of the network that table row `e` runs.  Read through the
    // bounds-checked table stream: the row after the last one reads as zeros (net A), whatever lies behind the buffer.
    [[maybe_unused]] auto row_pack = [&](int e) __attribute__((always_inline)) {
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__builtin_amdgcn_raw_buffer_load_b32(ts.rsrc, 0, e * args.etab_stride * 4 + 12, 0));      // RowHdr::flags
        return (f & kRowNetB) ? sub_bytes : 0;
    };
    [[maybe_unused]] int sb_row = 0;                   // SELECT: this row's network; the ring and hacc already hold its head
    if constexpr (SELECT) sb_row = row_pack(0);
    const int out_sbyte = L.chunk_off_out() * CB;
    const int out_bias_byte = (int)(L.bias_off_out() * 4);

    // cooperative twin: wavefront wv owns logical blocks [wv * NBW, (wv + 1) * NBW) of every hidden layer and visits its
    // chunks of a layer group-major, every visiting list padded to a multiple of RING (coop_layer, ff_ode_frame.hpp).
    // visit_byte is the frame's coop_byte kept as a lambda of this kernel: with the function, the 256-wide twins allocate
    // 157 / 140 VGPRs for 143 / 130 (profiles/frame_refactor.txt).
    constexpr int NBW = COOP ? NB / 4 : NB;
    [[maybe_unused]] const int ob0 = wv * NBW;
    constexpr LayerGeom CG1 = layer_geom(K1, NB, RB / 4), CGH = layer_geom(KH, NB, RB / 4), CGO = layer_geom(KH, NOB_OUT, RB / 4);
    auto visit_byte = [&](const LayerGeom& G, int sbyte, int i, int nm, int b0) __attribute__((always_inline)) {
        const int g = i / nm, j = i % nm;
        return sbyte + chunk_index(G, g < G.G ? g : 0, b0 + j) * CB;      // (padding visits re-read a real chunk)
    };

    // prefetch ring: the first RING chunks of net A's layer 1 (of this wavefront's visiting list in the cooperative twin);
    // SELECT: of the layer 1 of row 0's network
    f32x4 ring[RING][T::PHYS];
#pragma unroll
    for (int i = 0; i < RING; ++i)
#pragma unroll
        for (int p = 0; p < T::PHYS; ++p)
            ring[i][p] = sload(ws, lane16, (COOP ? visit_byte(CG1, sb_row, i, NBW, ob0) : sb_row + i * CB) + p * 1024);

    float P[KH];                 // operand registers of a hidden layer
    // hidden accumulators: they hold the bias of the layer about to run (row 0's c1 of net A to start with)
    BlockAcc<TILE> hacc[COOP ? 1 : NB];
    if constexpr (!COOP) {
#pragma unroll
        for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16, 128 + o * 128);
    }

    bool bad_slot = false;
    // cooperative twin: the exchange buffer of the NEXT activation hand-over; it alternates over the whole launch
    [[maybe_unused]] int xbuf = 0;
    for (int e = 0; e < args.n_evals; ++e) {
        const int row_byte = e * args.etab_stride * 4;
        HdrPtr hdr = (HdrPtr)(args.etab + (size_t)e * args.etab_stride);
        const float a_e = hdr->a, b_e = hdr->b;
        const uint32_t flags = hdr->flags;
        const int slot = hdr->slot;
        [[maybe_unused]] int sb_next = 0;            // SELECT: the NEXT row's network (prefetch target of the output layer)
        if constexpr (SELECT) sb_next = row_pack(e + 1);

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

        // NET_A + NET_B (the rows of the other half are exact zeros in each).
        const bool slot_ok = (unsigned)slot < (unsigned)kSlots;
        float net[NOB_OUT * RB];
        if constexpr (COOP) {
            // ---- cooperative evaluation: NB / 4 blocks of every layer per wavefront, activations exchanged through LDS --
            // the layer and the activation exchange of the twin: coop_layer / coop_exchange, ff_ode_frame.hpp
            auto layer = [&](auto tag, const auto& Bop, auto& acc, int sbyte, int b0, auto&& next) __attribute__((always_inline)) {
                coop_layer<TILE, H, DREGS, CREGS, RING, false, decltype(tag)::value>(ring, ws, lane16, exch, Bop, acc, sbyte, b0, next);
            };
            auto exchange = [&](const BlockAcc<TILE> (&acc)[NBW], int buf) __attribute__((always_inline)) {
                coop_exchange<TILE, H, false, 0, false>(acc, exch, buf, ob0, P, wv == kSkewWave, false, 0, aspec);
            };
            // Net A's output while net B runs.  In registers: the stage slots are shared, and a fast wavefront stores the
            // row's finished right-hand side into the slot before a slow one would have read a value parked there.
            [[maybe_unused]] float net_a[DREGS];
            static_for<NSUB>([&](auto ss) {
                constexpr int sub = decltype(ss)::value;
                const int sb = SELECT ? sb_row : sub * sub_bytes;          // this network's pack in the weight stream
                auto next_hidden_or_out = [&](int l_next, auto kk, auto sl) __attribute__((always_inline)) {
                    // visit k of the layer after a hidden-side layer: hidden layer l_next, or the output layer
                    constexpr int k = decltype(kk)::value, rs = decltype(sl)::value;
                    const bool is_hid = l_next < args.n_hidden - 1;
                    const int byte = is_hid ? visit_byte(CGH, sb + L.chunk_off_hid(l_next) * CB, k, NBW, ob0)
                                            : visit_byte(CGO, sb + out_sbyte, k, NOB_OUT, 0);
                    static_for<T::PHYS>([&](auto pp) {
                        constexpr int p = decltype(pp)::value;
                        ring[rs][p] = sload(ws, lane16, byte + p * 1024);
                    });
                };
                BlockAcc<TILE> cacc[NBW];
                // layer 1: bias c1 of this network from the evaluation row
                const int c1_byte = row_byte + 128 + sub * H * 4;
#pragma unroll
                for (int j = 0; j < NBW; ++j) cacc[j] = load_bias_acc<TILE>(ts, q16, c1_byte + (ob0 + j) * 128);
                layer(std::integral_constant<int, 0>{}, y, cacc, sb, ob0,
                      [&](auto kk, auto sl) { next_hidden_or_out(0, kk, sl); });
                for (int l = 0; l < args.n_hidden - 1; ++l) {
                    BlockAcc<TILE> nacc[NBW];                            // this layer's bias: requested before the exchange
                    const int bbyte = sb + (int)(L.bias_off_hid(l) * 4);
#pragma unroll
                    for (int j = 0; j < NBW; ++j) nacc[j] = load_bias_acc<TILE>(ws, q16, bbyte + (ob0 + j) * 128);
                    exchange(cacc, xbuf);
                    xbuf ^= 1;
#pragma unroll
                    for (int j = 0; j < NBW; ++j) cacc[j] = nacc[j];
                    layer(std::integral_constant<int, 1>{}, P, cacc, sb + L.chunk_off_hid(l) * CB, ob0,
                          [&](auto kk, auto sl) { next_hidden_or_out(l + 1, kk, sl); });
                }
                BiasBlk<TILE> obias[NOB_OUT];
#pragma unroll
                for (int o = 0; o < NOB_OUT; ++o) obias[o] = load_bias<TILE>(ws, q16, sb + out_bias_byte + o * 128);
                exchange(cacc, xbuf);
                xbuf ^= 1;
                // output layer: every wavefront computes all of it; the ring moves on to net B's layer 1 (after net A) or
                // to net A's layer 1 of the next evaluation
                BlockAcc<TILE> oacc[NOB_OUT];
                layer(std::integral_constant<int, 2>{}, P, oacc, sb + out_sbyte, 0, [&](auto kk, auto sl) {
                    constexpr int k = decltype(kk)::value, rs = decltype(sl)::value;
                    static_for<T::PHYS>([&](auto pp) {
                        constexpr int p = decltype(pp)::value;
                        ring[rs][p] = sload(ws, lane16, visit_byte(CG1, SELECT ? sb_next : (sub == 0 ? sub_bytes : 0), k, NBW, ob0) + p * 1024);
                    });
                });
#pragma unroll
                for (int o = 0; o < NOB_OUT; ++o)
#pragma unroll
                    for (int r = 0; r < RB; ++r) net[o * RB + r] = oacc[o].reg(r) + obias[o].reg(r);
                if constexpr (sub == 0 && !SELECT) {
#if defined(FF_DEBUG_UNFIX)
                    // (test builds: the one-wavefront kernel's parking place, which four wavefronts share here)
                    if (slot_ok) {
#pragma unroll
                        for (int j = 0; j < R4; ++j)
                            ks[(slot * R4 + j) * 64] = f32x4{net[4 * j], net[4 * j + 1], net[4 * j + 2], net[4 * j + 3]};
                    }
#else
#pragma unroll
                    for (int r = 0; r < DREGS; ++r) net_a[r] = net[r];
#endif
                }
            });
            FF_SKEW_HOLD(wv == kSkewWave, 2);           // (test builds: late to pick net A's output up again)
            if (!SELECT && slot_ok) {
#if defined(FF_DEBUG_UNFIX)
#pragma unroll
                for (int j = 0; j < R4; ++j) {
                    const f32x4 na = ks[(slot * R4 + j) * 64];
#pragma unroll
                    for (int i = 0; i < 4; ++i) net[4 * j + i] = na[i] + net[4 * j + i];
                }
#else
#pragma unroll
                for (int r = 0; r < DREGS; ++r) net[r] = net_a[r] + net[r];
#endif
            }
        } else {
        // One wavefront per tile.  Net A's output is parked in this row's stage slot while net B runs (nothing reads that
        // slot before the row stores its right-hand side there), so that it holds no registers across the second network.
        // the activation pipeline of mlp_ode_kernel's one-wavefront path: `pend` = the previous layer's parked last
        // block, activated into P[(NB-1)*RB ..] behind the first MFMAs of the next layer
        float pend[RB];
        BiasBlk<TILE> bias[2];
        ActGroup ag[12];
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
                    act_stage<false, 0, k>(ag[gi], &P[(NB - 1) * RB + 4 * gi], false, 0, aspec);
                }
            });
        };
        auto own_slot = [&](auto geom, auto mm, const BlockAcc<TILE> (&acc)[NB]) {
            constexpr LayerGeom G = decltype(geom)::value;
            constexpr int M = decltype(mm)::value;
            static_for<kActStages>([&](auto kk) {
                constexpr int k = kActStages - 1 - decltype(kk)::value;
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

        static_for<NSUB>([&](auto ss) {
            constexpr int sub = decltype(ss)::value;
            const int sb = SELECT ? sb_row : sub * sub_bytes;          // this network's pack in the weight stream
            // ---- layer 1: [y | cond] -> H, bias c1 of this network (already in hacc) -----------------------------
            {
                using G1 = GeomTag<TILE, K1, NB>;
                const int nbyte = sb + (int)(L.bias_off_hid(0) * 4);
                run_layer<TILE, RING, K1, NB, false, false>(
                    ring, ws, lane16, sb, y, hacc, [&](auto ob) { refill(nbyte, ob); },
                    [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) { own_slot(G1{}, mm, acc); },
                    [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
            }
            // ---- hidden -> hidden ----------------------------------------------------------------------------
            for (int l = 0; l < args.n_hidden - 1; ++l) {
                using GH = GeomTag<TILE, KH, NB>;
                const int sbyte = sb + L.chunk_off_hid(l) * CB;
                const int nbyte = sb + (int)(L.bias_off_hid(l + 1) * 4);
                run_layer<TILE, RING, KH, NB, false, false>(
                    ring, ws, lane16, sbyte, P, hacc, [&](auto ob) { refill(nbyte, ob); },
                    [&](auto mm, const BlockAcc<TILE> (&acc)[NB]) {
                        prev_slot(mm);
                        own_slot(GH{}, mm, acc);
                    },
                    [&](const BlockAcc<TILE>& acc) { park_and_refill(nbyte, acc); });
            }
            // ---- output layer ------------------------------------------------------------------------------------
            // the hidden accumulators take the next network's c1: net B's of this row after net A, net A's of the
            // next row after net B (a row past the table reads as zeros); SELECT: the next row's only c1
            const int c1_next = (sub == 0 && !SELECT) ? row_byte + 128 + H * 4 : row_byte + args.etab_stride * 4 + 128;
#pragma unroll
            for (int o = 0; o < NB; ++o) hacc[o] = load_bias_acc<TILE>(ts, q16, c1_next + o * 128);
            BlockAcc<TILE> oacc[NOB_OUT];
            constexpr int OUT_LAST_PHYS = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;   // tiles with state rows
            // the ring moves on to net B's layer 1 (after net A) or to net A's layer 1 of the next evaluation
            run_layer<TILE, RING, KH, NOB_OUT, true, true, (OUT_LAST_PHYS < T::PHYS ? OUT_LAST_PHYS : T::PHYS)>(
                ring, ws, lane16, sb + out_sbyte, P, oacc,
                [&](auto ob) {
                    constexpr int o = decltype(ob)::value;
                    bias[o & 1] = load_bias<TILE>(ws, q16, sb + out_bias_byte + o * 128);
                },
                [&](auto mm, const BlockAcc<TILE> (&acc)[NOB_OUT]) {
                    prev_slot(mm);
                    if constexpr (NOB_OUT > 1) {          // finished output blocks: bias add
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
                SELECT ? sb_next : (sub == 0 ? sub_bytes : 0));
            if constexpr (sub == 0 && !SELECT) {
                if (slot_ok) {
#pragma unroll
                    for (int j = 0; j < R4; ++j)
                        ks[(slot * R4 + j) * 64] = f32x4{net[4 * j], net[4 * j + 1], net[4 * j + 2], net[4 * j + 3]};
                }
            }
        });
        if (!SELECT && slot_ok) {
#pragma unroll
            for (int j = 0; j < R4; ++j) {
                const f32x4 na = ks[(slot * R4 + j) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) net[4 * j + i] = na[i] + net[4 * j + i];
            }
        }
        }   // !COOP

        // ---- RHS and stage bookkeeping: once per evaluation, after both networks ---------------------------------
        float rhs[DREGS];
#pragma unroll
        for (int r = 0; r < DREGS; ++r) rhs[r] = __builtin_fmaf(a_e, y[r], b_e * net[r]);
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
        if constexpr (SELECT) sb_row = sb_next;
        if (flags & 2u) {
            // noise rows: read where they are used (two networks' worth of registers are live across the evaluation)
            float nz[DREGS];
            if (args.noise) {
                const float* np = args.noise + (size_t)hdr->noise_idx * args.noise_stride + sample * D;
#pragma unroll
                for (int r = 0; r < DREGS; ++r) {
                    const int d = feat_of_reg(TILE, r, qd);
                    nz[r] = (d < D) ? np[d] : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < R4; ++j) {
                    const f32x4 z = noise_draw4<TILE>(args, hdr, sample, qd, j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) nz[4 * j + i] = z[i];
                }
            }
            const float gn = hdr->gn;
#pragma unroll
            for (int r = 0; r < DREGS; ++r) x[r] = __builtin_fmaf(gn, nz[r], x[r]);
        }
    }

    // ---- epilogue: auxiliary outputs (adaptive attempts), final state -----------------------------------------------
    const bool writer = col_live && (!COOP || wv == 0);
    if (args.n_aux > 0) {
        HdrPtr t0h = (HdrPtr)(args.etab + (size_t)args.n_evals * args.etab_stride);
        HdrPtr t1h = (HdrPtr)(args.etab + (size_t)(args.n_evals + 1) * args.etab_stride);
        const uint32_t use_y = t0h->flags;
        static_for<kAux>([&](auto jj) {
            constexpr int j = decltype(jj)::value;
            if (j < args.n_aux) {
                HdrPtr th = (j < 2) ? t0h : t1h;
                float c[kSlots];
#pragma unroll
                for (int s = 0; s < kSlots; ++s) c[s] = (j & 1) ? th->cout[s] : th->cin[s];
                const float uy = ((use_y >> j) & 1u) ? 1.f : 0.f;
#pragma unroll
                for (int q4 = 0; q4 < R4; ++q4) {
                    f32x4 v = uy * f32x4{x[4 * q4], x[4 * q4 + 1], x[4 * q4 + 2], x[4 * q4 + 3]};
#pragma unroll
                    for (int s = 0; s < kSlots; ++s) v += c[s] * ks[(s * R4 + q4) * 64];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int d = feat_of_reg(TILE, 4 * q4 + i, qd);
                        if (writer && d < D && args.aux_out[j]) args.aux_out[j][sample * D + d] = v[i];
                    }
                }
            }
        });
    }
    bool bad = false;
    if (writer) {
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
}

} // namespace ff
