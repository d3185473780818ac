// ff_ode_frame.hpp -- the pieces mlp_ode_kernel (ff_mlp_ode.hpp) and mlp_pair_kernel (ff_mlp_pair.hpp) share.
//
// Included by ff_mlp_ode.hpp below its primitives (f32x4, Tile, Stream, BlockAcc, act_stage, static_for; ff_layout.h,
// ff_kernel_args.h, ff_philox.h, ff_skew.h).  Here stand the pieces that are the same in both kernels AND leave every
// instance's registers and spills where they were: one register of the state / conditional load, the stage-slot
// set-up, the cooperative twin's layer and activation exchange, the in-kernel noise draw.  The rest of the common code
// is still written out in each kernel (CHANGELOG.md has why).
#pragma once

namespace ff {

typedef const __attribute__((address_space(4))) RowHdr* HdrPtr;   // scalar (SMEM) loads of a row's header

// ---- state and conditional inputs ---------------------------------------------------------------------------------------
// One register of the state / of the conditional inputs; the kernels keep the loop over their registers, so that the
// arrays stay their own (a register array handed to a helper by reference is split into registers only after inlining,
// and mlp_ode_m16_h256_d16_c4_t0 then allocates 347 VGPRs for 336).
// Value columns: x = (x_in - in_shift) / in_scale, cnd = cond.  Tangent columns (is_tangent; role j >= 1 = tangent j-1):
// x = the unit vector of dimension tangent_first + role - 1, cnd = 0; a Hutchinson column (unit_tangents == 0) gets 0 here
// and its probe from probe_reg, in a pass of the kernel's own behind the conditional inputs.  (The probe's address in this
// function's branch, in any spelling, moved scratch on the 256-wide tangent units: profiles/hutch_multi_resources.txt.)
template <int TILE>
__device__ __forceinline__ float state_reg(const KernelArgs& args, long long sample, int qd, bool is_tangent, int role, int r)
{
    const int D = args.dim;
    const int d = feat_of_reg(TILE, r, qd);
    float v = 0.f;
    if (d < D) {
        if (!is_tangent) {
            v = args.x_in[sample * D + d];
            if (args.in_shift) v = v - args.in_shift[d];
            if (args.in_scale) v = v / args.in_scale[d];
        } else if (args.unit_tangents) {
            v = (d == args.tangent_first + role - 1) ? 1.0f : 0.0f;
        }
    }
    return v;
}
// One register of a Hutchinson tangent column: probe role - 1 of the sample's n_tangent probes, probe [batch, n_tangent, dim]
// (n_tangent == 1: the sample's one probe).
template <int TILE>
__device__ __forceinline__ float probe_reg(const KernelArgs& args, long long sample, int qd, int role, int r)
{
    const int d = feat_of_reg(TILE, r, qd);
    return d < args.dim ? args.probe[(sample * args.n_tangent + (role - 1)) * args.dim + d] : 0.f;
}
template <int TILE>
__device__ __forceinline__ float cond_reg(const KernelArgs& args, long long sample, int qd, bool is_tangent, int r)
{
    const int C = args.cond_dim;
    const int d = feat_of_reg(TILE, r, qd);
    return (d < C && !is_tangent) ? args.cond[sample * C + d] : 0.f;
}
// Push-forward units (mlp_ode_kernel PUSH): one register of a tangent column's start vector, state part and conditional
// part.  unit_tangents == 0: probe[sample, role - 1, :] / cond_tangent[sample, role - 1, :] (NULL = zero).  unit_tangents
// == 1: the unit vector j = tangent_first + role - 1 of the combined space [0, D + C) -- j < D the state unit vector e_j,
// j >= D a zero state part and the conditional unit vector e_{j - D}.  The state part goes through the linear part of the
// input map, v / in_scale[d] (no shift: it is a derivative); the conditional part is taken as it is.
template <int TILE>
__device__ __forceinline__ float push_state_reg(const KernelArgs& args, long long sample, int qd, int role, int r)
{
    const int D = args.dim;
    const int d = feat_of_reg(TILE, r, qd);
    float v = 0.f;
    if (d < D) {
        if (args.unit_tangents) v = (d == args.tangent_first + role - 1) ? 1.0f : 0.0f;
        else if (args.probe) v = args.probe[(sample * args.n_tangent + (role - 1)) * D + d];
        if (args.in_scale) v = v / args.in_scale[d];
    }
    return v;
}
template <int TILE>
__device__ __forceinline__ float push_cond_reg(const KernelArgs& args, long long sample, int qd, int role, int r)
{
    const int C = args.cond_dim;
    const int d = feat_of_reg(TILE, r, qd);
    float v = 0.f;
    if (d < C) {
        if (args.unit_tangents) v = (args.dim + d == args.tangent_first + role - 1) ? 1.0f : 0.0f;
        else if (args.cond_tangent) v = args.cond_tangent[(sample * args.n_tangent + (role - 1)) * C + d];
    }
    return v;
}
// ---- stage slots ----------------------------------------------------------------------------------------------------------
// Zero fill of the Runge-Kutta stage slots `ks` (LDS; each lane only ever touches its own words), then the caller's first
// stage (k1_in: FSAL of the previous step) into slot 0.
// Cooperative twin: the four wavefronts share ONE copy of the slots.  Everything they store there later is the same value
// from each of them, so late or repeated stores are harmless -- except this zero fill: a wavefront that starts late would
// wipe the caller's first stage between another wavefront's store and its first read.  BARRIER: all fills first.  (The
// kernel passes it: a test build of mlp_ode_kernel drops it again to show that the skew test can see the hole.)
// `skewed` = this wavefront is the one a test build holds back (ff_skew.h).
template <int TILE, int DREGS, bool COOP, bool BARRIER>
__device__ __forceinline__ void init_stage_slots(const KernelArgs& args, f32x4* ks, long long sample, int qd, bool is_tangent,
                                                 [[maybe_unused]] bool skewed)
{
    constexpr int R4 = DREGS / 4;
    FF_SKEW_HOLD(COOP && skewed, 1);          // (test builds: this wavefront starts late ...)
#pragma unroll
    for (int s = 0; s < kSlots; ++s)
#pragma unroll
        for (int j = 0; j < R4; ++j) ks[(s * R4 + j) * 64] = f32x4{0.f, 0.f, 0.f, 0.f};
    FF_SKEW_HOLD(COOP && skewed, 2);          // (... and lingers between its zero fill and its first store)
    if constexpr (BARRIER) __syncthreads();
    if (args.k1_in) {
#pragma unroll
        for (int j = 0; j < R4; ++j) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = feat_of_reg(TILE, 4 * j + i, qd);
                if (d < args.dim && !is_tangent) v[i] = args.k1_in[sample * args.dim + d];
            }
            ks[j * 64] = v;
        }
    }
    FF_SKEW_HOLD(COOP && !skewed, 2);         // (test builds: the others wait between that store and their first read)
}

// ---- cooperative twin: a wavefront's share of a layer ---------------------------------------------------------------------
// Wavefront wv owns logical blocks [wv * NBW, (wv + 1) * NBW) of every hidden layer (NBW = NB / 4, ob0 = wv * NBW) and
// visits its chunks of a layer group-major: visit i = (group i / nm, own block i % nm) -> chunk_index() of ff_layout.h in
// the SAME packed stream.  Every layer's visiting list is padded to a multiple of RING, so a layer always starts at ring
// slot 0.  coop_byte: byte offset of visit i of a layer whose chunk 0 lies at `sbyte`.
template <int TILE>
__device__ __forceinline__ int coop_byte(const LayerGeom& G, int sbyte, int i, int nm, int b0)
{
    const int g = i / nm, j = i % nm;
    return sbyte + chunk_index(G, g < G.G ? g : 0, b0 + j) * (1024 * Tile<TILE>::PHYS);      // (padding visits re-read a real chunk)
}

// The twin's machinery; the kernels call it through one-line lambdas of their own.
// One layer of this wavefront's share: acc[j] += W[block b0 + j, :] . Bop over the layer's groups, in ascending group
// order (the order of the one-wavefront kernel: same FMA chain per output row).  KIND: 0 = layer 1, 1 = hidden, 2 = output
// (every wavefront computes all of it, from zero accumulators).  WIDE: the operands of a hidden / output layer are read
// from the exchange buffer `exch`, group by group, instead of from Bop.
// next(k, slot): request visit k of the NEXT layer into ring slot `slot`.
template <int TILE, int H, int DREGS, int CREGS, int RING, bool WIDE, int KIND, class BOp, class Acc, class NextFn>
__device__ __forceinline__ void coop_layer(f32x4 (&ring)[RING][Tile<TILE>::PHYS], const Stream& ws, int lane16, const f32x4* exch,
                                           const BOp& Bop, Acc& acc, int sbyte, int b0, NextFn&& next)
{
    typedef Tile<TILE> T;
    constexpr int NB = H / 32, RBQ = T::RB / 4, NBW = NB / 4, KH = NB * T::RB, K1 = DREGS + CREGS;
    constexpr int NOB_OUT = blocks_for_regs(TILE, DREGS);
    constexpr LayerGeom G = KIND == 0 ? layer_geom(K1, NB, RBQ) : (KIND == 1 ? layer_geom(KH, NB, RBQ) : layer_geom(KH, NOB_OUT, RBQ));
    constexpr int NM = KIND == 2 ? NOB_OUT : NBW;
    constexpr int NV = KIND == 0 ? (G.G * NBW + RING - 1) / RING * RING : G.G * NM;      // layer 1: padded visits
    static_assert(NV % RING == 0, "visiting lists are multiples of the ring length");
    constexpr int OUT_LAST = (DREGS * T::NQ - (NOB_OUT - 1) * 32 + TILE - 1) / TILE;
    constexpr int LAST_PHYS = KIND == 2 ? (OUT_LAST < T::PHYS ? OUT_LAST : T::PHYS) : T::PHYS;
    // WIDE: the operands of group g come from the exchange buffer, requested one group ahead
    constexpr bool LDS_B = WIDE && KIND != 0;
    f32x4 bq = f32x4{0.f, 0.f, 0.f, 0.f}, bq_next = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (LDS_B) bq_next = exch[0];
    static_for<NV>([&](auto ii) {
        constexpr int i = decltype(ii)::value;
        constexpr int slot = i % RING, g = i / NM, j = i % NM;
        if constexpr (g < G.G) {
            if constexpr (LDS_B && j == 0) {
                bq = bq_next;
                if constexpr (g + 1 < G.G) bq_next = exch[(g + 1) * 64];
            }
            static_for<4>([&](auto qq) {
                constexpr int q = decltype(qq)::value;
                float bop;
                if constexpr (LDS_B) bop = bq[q];
                else bop = Bop[4 * g + q];
                static_for<T::PHYS>([&](auto pp) {
                    constexpr int p = decltype(pp)::value;
                    if constexpr (KIND == 2 && j == NM - 1 && p >= LAST_PHYS) {
                        if constexpr (g == 0 && q == 0) acc[j].v[p] = T::zero();
                    } else if constexpr (KIND == 2 && g == 0 && q == 0)
                        acc[j].v[p] = T::mfma(ring[slot][p][q], bop, T::zero());
                    else
                        acc[j].v[p] = T::mfma(ring[slot][p][q], bop, acc[j].v[p]);
                });
            });
        }
        constexpr int nxt = i + RING;
        if constexpr (nxt < NV) {
            static_for<T::PHYS>([&](auto pp) {
                constexpr int p = decltype(pp)::value;
                ring[slot][p] = sload(ws, lane16, coop_byte<TILE>(G, sbyte, nxt, NM, b0) + p * 1024);
            });
        } else {
            next(std::integral_constant<int, nxt - NV>{}, std::integral_constant<int, slot>{});
        }
        __builtin_amdgcn_sched_barrier(0x2 | 0x4 | 0x400 | 0x80);
    });
}

// Activate this wavefront's blocks (ob0 ..) and trade them for everybody else's through exchange buffer `buf` of `exch`
// (2 x (KH / 4) x 64 slots; WIDE: one buffer): P <- all KH operand registers (WIDE: they stay in the buffer).
// `skewed`: test builds hold this wavefront back (ff_skew.h).
template <int TILE, int H, bool TANGENTS, int ACT, bool WIDE>
__device__ __forceinline__ void coop_exchange(const BlockAcc<TILE> (&acc)[H / 128], f32x4* exch, int buf, int ob0,
                                              float (&P)[WIDE ? 4 : H / 32 * Tile<TILE>::RB], [[maybe_unused]] bool skewed,
                                              bool is_tangent, int value_lane_bytes, const ActSpec& aspec)
{
    constexpr int NBW = H / 128, RBQ = Tile<TILE>::RB / 4, KH = H / 32 * Tile<TILE>::RB;
    f32x4* const xb = exch + (size_t)(WIDE ? 0 : buf) * (KH / 4) * 64;
    if constexpr (WIDE) __syncthreads();         // one buffer: the layer that read it has finished everywhere
    static_for<NBW>([&](auto jj) {
        constexpr int j = decltype(jj)::value;
        static_for<RBQ>([&](auto rr) {
            constexpr int r4 = decltype(rr)::value;
            ActGroup ag;
            float out[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ag.pre[i] = acc[j].reg(4 * r4 + i);
            static_for<kActStages>([&](auto kk) {
                act_stage<TANGENTS, ACT, decltype(kk)::value>(ag, out, is_tangent, value_lane_bytes, aspec);
            });
            xb[((ob0 + j) * RBQ + r4) * 64] = f32x4{out[0], out[1], out[2], out[3]};
        });
    });
    __syncthreads();
    FF_SKEW_HOLD(skewed, 2);       // (test builds: late to read what the others are about to overwrite)
    if constexpr (!WIDE) {
#pragma unroll
        for (int k4 = 0; k4 < KH / 4; ++k4) {
            const f32x4 v = xb[k4 * 64];
#pragma unroll
            for (int i = 0; i < 4; ++i) P[4 * k4 + i] = v[i];
        }
    }
}

// ---- noise of a row (FF_ROW_NOISE) drawn in the kernel (ff_ode_args) ---------------------------------------------------------
// Philox4x32-10 keyed by rng_seed, counter = (global sample index, noise index of the row, block of four dimensions) --
// registers 4j..4j+3 of a lane are dimensions 4*blk..4*blk+3 -- and Box-Muller: the four normals of register group j
// (the kernels keep the loop over their groups, as for state_reg)
template <int TILE>
__device__ __forceinline__ f32x4 noise_draw4(const KernelArgs& args, HdrPtr hdr, long long sample, int qd, int j)
{
    const unsigned long long gs = (unsigned long long)(sample + args.rng_sample_offset);
    uint32_t c[4] = {(uint32_t)gs, (uint32_t)(gs >> 32), (uint32_t)(hdr->noise_idx + args.rng_noise_base),
                     (uint32_t)(feat_of_reg(TILE, 4 * j, qd) >> 2)};
    philox4x32_10(c, (uint32_t)args.rng_seed, (uint32_t)(args.rng_seed >> 32));
    float z0, z1, z2, z3;
    box_muller(c[0], c[1], z0, z1);
    box_muller(c[2], c[3], z2, z3);
    return f32x4{z0, z1, z2, z3};
}

} // namespace ff
