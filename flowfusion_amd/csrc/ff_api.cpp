// ff_api.cpp -- C ABI of libflowfusion_amd.so (see include/flowfusion_amd.h).
#include <hip/hip_runtime_api.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include "flowfusion_amd.h"
#include "ff_layout.h"
#include "ff_split_layout.h"
#include "ff_registry.h"
#include "ff_pull_registry.h"
#include "ff_pullsel_registry.h"
#include "ff_pushsel_registry.h"
#include "ff_vjp_registry.h"
#include "ff_dadj_registry.h"
#include "ff_lgrad_registry.h"
#include "ff_adapt_logic.h"

static_assert(FF_MAX_SLOTS == ff::kSlots, "slot count mismatch between header and kernel");
static_assert(FF_MAX_AUX == ff::kAux, "aux count mismatch between header and kernel");
static_assert(FF_ROW_HDR * 4 == sizeof(ff::RowHdr), "row header mismatch");
static_assert(FF_STATUS_NAN == ff::kStatusNaN && FF_STATUS_BAD_SLOT == ff::kStatusBadSlot && FF_STATUS_NOISE_ROW == ff::kStatusNoiseRow,
              "status bits mismatch");
static_assert(sizeof(ff_adapt_state) == 128, "controller state is 128 bytes");

static thread_local int t_last_hip_error = 0;

extern "C" const char* ff_version(void) { return "flowfusion_amd 0.4 gfx950 (f32 MFMA 16x16x4 / 32x32x2, opt-in bf16x3 / bf16x2 split on 16x16x32 bf16; in-register layer chaining; device-side adaptive step control; Hutch++ / XTrace estimator kernels)"; }

extern "C" int ff_kernel_count(void) { return ff::g_n_kernels + ff::g_n_split_kernels; }

// ids [0, n) are the fp32 instantiations (plan.kernel_id of an FF_PREC_F32 plan), [n, n + m) the split-precision ones
extern "C" const char* ff_kernel_name(int id)
{
    if (id < 0 || id >= ff::g_n_kernels + ff::g_n_split_kernels) return NULL;
    return id < ff::g_n_kernels ? ff::g_kernels[id].name : ff::g_split_kernels[id - ff::g_n_kernels].name;
}

extern "C" int ff_last_hip_error(void) { return t_last_hip_error; }

// tangent columns per sample for a mode; `tile` bounds how many unit tangents one launch can carry
static int tangents_of_mode(int mode, int dim, int tile, int* n_tangent, int* unit)
{
    switch (mode) {
    case FF_MODE_STATE: *n_tangent = 0; *unit = 0; return 0;
    case FF_MODE_HUTCH: *n_tangent = 1; *unit = 0; return 0;
    case FF_MODE_EXACT: *n_tangent = dim < tile - 1 ? dim : tile - 1; *unit = 1; return 0;
    default: return FF_ERR_BADARG;
    }
}

static inline int split_parts(int precision) { return precision == FF_PREC_BF16X2 ? 2 : 3; }

// the widest hidden layer, or -1 if a width is not positive
static int widest(int n_hidden, const int* hidden_widths)
{
    int wmax = 0;
    for (int i = 0; i < n_hidden; ++i) {
        if (hidden_widths[i] < 1) return -1;
        if (hidden_widths[i] > wmax) wmax = hidden_widths[i];
    }
    return wmax;
}

static int fill_plan(ff_mlp_plan_t* plan, int dim, int cond_dim, int n_hidden, int width, int dregs, int cregs, int kernel_id,
                     int tile, int activation)
{
    memset(plan, 0, sizeof(*plan));
    plan->dim = dim;
    plan->cond_dim = cond_dim;
    plan->n_hidden = n_hidden;
    plan->width = width;
    plan->dregs = dregs;
    plan->cregs = cregs;
    plan->kernel_id = kernel_id;
    plan->tile = tile;
    plan->activation = activation;
    return FF_OK;
}

// The entry of an fp32 table (single-network or pair) that serves a network, or -1.  Preference among the entries that
// fit (and that `also` accepts): narrowest width first (it dominates the FLOPs); at equal width the 16x16x4
// two-waves-per-SIMD kernels (measured ~3% faster than 32x32x2 at width 256), then fewer first-layer k-steps.
template <class Entry, class Also>
static int best_entry(const Entry* table, int n, int dim, int cond_dim, int wmax, Also also)
{
    int best = -1;
    for (int i = 0; i < n; ++i) {
        const Entry& k = table[i];
        const int need_d = ff::regs_for(k.tile, dim);
        const int need_c = cond_dim > 0 ? ff::regs_for(k.tile, cond_dim) : 0;
        if (k.H < wmax || k.dregs < need_d || k.cregs < need_c || !also(k)) continue;
        if (best < 0) { best = i; continue; }
        const Entry& b = table[best];
        const int kc = (k.dregs + k.cregs) * (64 / k.tile), bc = (b.dregs + b.cregs) * (64 / b.tile);     // first-layer features covered
        if (k.H < b.H || (k.H == b.H && (k.tile < b.tile || (k.tile == b.tile && kc < bc)))) best = i;
    }
    return best;
}

// FF_PREC_BF16X3 / FF_PREC_BF16X2: the split-precision family (ff_mlp_ode_split.hpp) -- SiLU, width <= 256, dim <= 16,
// cond_dim <= 16, state-only or Hutchinson, the number of hidden layers compiled in
static int plan_split(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode, int activation,
                      int precision, ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 1 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    if (mode != FF_MODE_STATE && mode != FF_MODE_HUTCH && mode != FF_MODE_EXACT) return FF_ERR_BADARG;
    if (activation < 0 || activation >= FF_ACT_COUNT) return FF_ERR_BADARG;
    if (activation != FF_ACT_SILU || dim > 32 || cond_dim > 16) return FF_ERR_UNSUPPORTED;
    const int need_dt = dim > 16 ? 2 : 1;              // 16-dimension tiles of the state
    const int wmax = widest(n_hidden, hidden_widths);
    if (wmax < 0) return FF_ERR_BADARG;
    if (wmax > ff::split::kWidth) return FF_ERR_UNSUPPORTED;
    const int need_t = mode == FF_MODE_STATE ? 0 : (mode == FF_MODE_HUTCH ? 1 : 2);
    int best = -1;                                     // the narrowest instantiation that holds the network
    for (int i = 0; i < ff::g_n_split_kernels; ++i) {
        const ff::SplitKernelEntry& k = ff::g_split_kernels[i];
        if (k.n_hidden == n_hidden && k.tangents == need_t && k.parts == split_parts(precision) && k.dt == need_dt &&
            k.width >= wmax && (best < 0 || k.width < ff::g_split_kernels[best].width))
            best = i;
    }
    if (best < 0) return FF_ERR_UNSUPPORTED;
    // 4 dimensions x 2 column blocks per lane and 16-dimension tile; exact trace: a sample and its unit tangents share a
    // column block of 16
    fill_plan(plan, dim, cond_dim, n_hidden, ff::g_split_kernels[best].width, 8 * need_dt, cond_dim > 0 ? 8 : 0, best,
              need_t == 2 ? 16 : 32, FF_ACT_SILU);
    plan->precision = precision;
    return FF_OK;
}

extern "C" int ff_mlp_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                           ff_mlp_plan_t* plan)
{
    return ff_mlp_plan_act(dim, cond_dim, n_hidden, hidden_widths, mode, FF_ACT_SILU, NULL, plan);
}

extern "C" int ff_mlp_plan_act(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                               int activation, const float* act_param, ff_mlp_plan_t* plan)
{
    return ff_mlp_plan_prec(dim, cond_dim, n_hidden, hidden_widths, mode, activation, act_param, FF_PREC_F32, plan);
}

extern "C" int ff_mlp_plan_prec(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                                int activation, const float* act_param, int precision, ff_mlp_plan_t* plan)
{
    if (precision != FF_PREC_F32 && precision != FF_PREC_BF16X3 && precision != FF_PREC_BF16X2) return FF_ERR_BADARG;
    if (precision != FF_PREC_F32) return plan_split(dim, cond_dim, n_hidden, hidden_widths, mode, activation, precision, plan);
    if (!plan || !hidden_widths || dim < 1 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    if (activation < 0 || activation >= FF_ACT_COUNT) return FF_ERR_BADARG;
    if (mode != FF_MODE_STATE && mode != FF_MODE_HUTCH && mode != FF_MODE_EXACT) return FF_ERR_BADARG;
    const int wmax = widest(n_hidden, hidden_widths);
    if (wmax < 0) return FF_ERR_BADARG;
    const int need_t = mode != FF_MODE_STATE;
    const int best = best_entry(ff::g_kernels, ff::g_n_kernels, dim, cond_dim, wmax, [&](const ff::KernelEntry& k) {
        return k.tangents == need_t && (k.act == activation || (k.act == 9 && activation != FF_ACT_SILU));
    });
    if (best < 0) return FF_ERR_UNSUPPORTED;
    const ff::KernelEntry& k = ff::g_kernels[best];
    fill_plan(plan, dim, cond_dim, n_hidden, k.H, k.dregs, k.cregs, best, k.tile, activation);
    if (act_param) { plan->act_param[0] = act_param[0]; plan->act_param[1] = act_param[1]; }
    return FF_OK;
}

// ---- what a plan launches, as data ------------------------------------------------------------------------------------
// describe() validates a plan once and says everything the code below needs to know about its family: the launcher,
// ff_mlp_launch_kind and the small queries read the description and never ask which family they serve.
enum PlanFamily { kF32 = 1, kSplit, kPair, kSelect, kPush, kPull, kPullSel, kPushSel };

struct LaunchDesc {
    PlanFamily family;
    const char* name;          // of the kernel (the one-wavefront kernel's where there are two)
    ff::LaunchFn one_wave;     // a wavefront per tile, four tiles per workgroup; NULL: the wide catch-all, cooperative always
    ff::LaunchFn coop;         // the cooperative twin, a tile per workgroup; NULL: none
    int wps;                   // wavefronts per SIMD of the one-wavefront kernel: 1024 * wps tiles run at once
    double c0, per_round, least;   // the twin's line (choose_launch): max(least, c0 + tiles / (per_round * chip))
    int tangents;              // != 0: the kernel carries tangent columns and serves FF_MODE_HUTCH / FF_MODE_EXACT, not FF_MODE_STATE
    bool state_only;           // a family without a divergence: FF_MODE_STATE without jac_out is all it takes, and probe, dlogp_*,
                               // kl1_in and aux_lp_out do not reach the kernel
    int nets;                  // networks in the packed weights (wpack_floats = nets x the layout's)
    int row_nets;              // c1 vectors in an evaluation row (etab_stride = FF_ROW_HDR + row_nets x width)
    int exchange;              // exchange buffers of the cooperative kernel in LDS
    // what the family's argument check refuses (kept per family as found; CHANGELOG.md lists the asymmetries)
    int max_aux;               // largest n_aux
    bool takes_k1;             // k1_in
    bool checks_noise_stride;  // noise_stride >= batch * dim where `noise` is set
    bool empty_batch_first;    // an empty batch is FF_OK before n_aux, k1_in, noise_stride and jac_out are looked at
    const ff::SplitKernelEntry* split;      // kSplit: the entry (that family keeps its own launch geometry, launch_split)
    bool products;             // kPull: the launch runs the plan's products sibling (ff_mlp_ode_launch_vjp sets it: ff_mlp_vjp.hpp)
    bool record, discrete;     // kPull: the plan's record / discrete-adjoint sibling (ff_mlp_ode_launch_record, _pull_discrete: ff_mlp_dadj.hpp)
    bool logp_grad;            // kPull: the plan's log-density gradient sibling (ff_mlp_ode_launch_logp_grad: ff_mlp_lgrad.hpp)
};

// The row-select pull-back table is a WEAK reference: a program that links this file with kernel tables of its own from before
// these units (tests/sanitize/pull_wpack_main.cpp) still links, and sees a library without them.
namespace ff {
extern const PullKernelEntry g_pullsel_kernels[] __attribute__((weak));
extern const int g_n_pullsel_kernels __attribute__((weak));
}
static int n_pullsel_kernels() { return &ff::g_n_pullsel_kernels ? ff::g_n_pullsel_kernels : 0; }

// The row-select push-forward table: weak for the same reason.
namespace ff {
extern const PushKernelEntry g_pushsel_kernels[] __attribute__((weak));
extern const int g_n_pushsel_kernels __attribute__((weak));
}
static int n_pushsel_kernels() { return &ff::g_n_pushsel_kernels ? ff::g_n_pushsel_kernels : 0; }

static bool shape_ok(const ff_mlp_plan_t* p, int tile, int H, int dregs, int cregs)
{
    const int per_reg = 64 / tile;
    return H == p->width && dregs == p->dregs && cregs == p->cregs && tile == p->tile && p->n_hidden >= 1 && p->dim >= 1 &&
           p->dim <= per_reg * p->dregs && p->cond_dim >= 0 && p->cond_dim <= per_reg * p->cregs;
}

// the twin's line of a single-network kernel (the comment above choose_launch)
static void twin_line(LaunchDesc* d, int wps)
{
    d->wps = wps;
    d->least = wps >= 3 ? 0.22 : (wps == 2 ? 0.30 : 0.35);
    d->c0 = wps == 1 ? 0.20 : 0.10;
    d->per_round = 0.95;
}

// false: not a plan of this library.  Kernel ids: [0, g_n_kernels) fp32 or, by the plan's precision, [0, g_n_split_kernels);
// FF_PAIR_KERNEL_BASE + i a pair plan, FF_PAIR_SELECT_KERNEL_BASE + i a select plan, the same index into the pair table.
static bool describe(const ff_mlp_plan_t* p, LaunchDesc* d)
{
    memset(d, 0, sizeof(*d));
    if (!p || p->kernel_id < 0) return false;
    if (p->precision == FF_PREC_BF16X3 || p->precision == FF_PREC_BF16X2) {
        if (p->kernel_id >= ff::g_n_split_kernels) return false;
        const ff::SplitKernelEntry& k = ff::g_split_kernels[p->kernel_id];
        if (!(k.parts == split_parts(p->precision) && p->width == k.width && p->tile == (k.tangents == 2 ? 16 : 32) &&
              p->dregs == 8 * k.dt && p->cregs == (p->cond_dim > 0 ? 8 : 0) && p->n_hidden == k.n_hidden &&
              p->activation == FF_ACT_SILU && p->dim >= 1 && p->dim <= 16 * k.dt && p->cond_dim >= 0 && p->cond_dim <= 16))
            return false;
        d->family = kSplit; d->name = k.name; d->one_wave = k.launch; d->row_nets = 1; d->split = &k;
        return true;
    }
    if (p->precision != FF_PREC_F32) return false;
    if (p->kernel_id < ff::g_n_kernels) {
        const ff::KernelEntry& k = ff::g_kernels[p->kernel_id];
        if (!shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation < 0 || p->activation >= FF_ACT_COUNT ||
            !(p->activation == k.act || (k.act == 9 && p->activation != FF_ACT_SILU)))
            return false;
        d->family = kF32; d->name = k.name; d->one_wave = k.launch; d->coop = k.launch_coop;
        twin_line(d, k.wps > 0 ? k.wps : 1);
        d->tangents = k.tangents; d->nets = 1; d->row_nets = 1;
        d->exchange = k.launch ? 2 : 1;
        d->max_aux = FF_MAX_AUX; d->takes_k1 = true; d->empty_batch_first = true;
        return true;
    }
    if (p->kernel_id >= FF_PUSH_SELECT_KERNEL_BASE) {
        // row-select push-forward units (ff_mlp_pushsel.hpp): the push units' geometry over a joint state [q | p]; the packed
        // weights are two forward packs, a row of the table carries the c1 of the one network it runs
        const int index = p->kernel_id - FF_PUSH_SELECT_KERNEL_BASE;
        if (index >= n_pushsel_kernels()) return false;
        const ff::PushKernelEntry& k = ff::g_pushsel_kernels[index];
        if (!k.launch || !shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation != FF_ACT_SILU || p->dim % 2 != 0) return false;
        d->family = kPushSel; d->name = k.name; d->one_wave = k.launch;
        twin_line(d, k.wps);
        d->tangents = 1; d->nets = 2; d->row_nets = 1; d->exchange = 2;
        return true;
    }
    if (p->kernel_id >= FF_PULL_SELECT_KERNEL_BASE) {
        // row-select pull-back units (ff_mlp_pullsel.hpp): the pull units' geometry over a joint state [q | p]; the packed weights
        // are two pull packs, a row of the table carries the c1 of the one network it runs
        const int index = p->kernel_id - FF_PULL_SELECT_KERNEL_BASE;
        if (index >= n_pullsel_kernels()) return false;
        const ff::PullKernelEntry& k = ff::g_pullsel_kernels[index];
        if (!k.launch || !shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation != FF_ACT_SILU || p->dim % 2 != 0) return false;
        d->family = kPullSel; d->name = k.name; d->one_wave = k.launch;
        twin_line(d, k.wps);
        d->tangents = 1; d->nets = 2; d->row_nets = 1; d->exchange = 2;
        return true;
    }
    if (p->kernel_id >= FF_PULL_KERNEL_BASE) {
        // pull-back units (ff_mlp_pull.hpp): a wavefront per workgroup and per tile, whole fixed-grid solves only; the packed
        // weights are the forward network's and the transposed network's (pull_layout), back to back
        const int index = p->kernel_id - FF_PULL_KERNEL_BASE;
        if (index >= ff::g_n_pull_kernels) return false;
        const ff::PullKernelEntry& k = ff::g_pull_kernels[index];
        if (!k.launch || !shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation != FF_ACT_SILU) return false;
        d->family = kPull; d->name = k.name; d->one_wave = k.launch;
        twin_line(d, k.wps);
        d->tangents = 1; d->nets = 1; d->row_nets = 1; d->exchange = 2;
        return true;
    }
    if (p->kernel_id >= FF_PUSH_KERNEL_BASE) {
        // push-forward units: the Hutchinson kernels' shapes with the tangent columns integrated; one wavefront per tile, whole
        // fixed-grid solves only (no first stage from the caller, no auxiliary outputs)
        const int index = p->kernel_id - FF_PUSH_KERNEL_BASE;
        if (index >= ff::g_n_push_kernels) return false;
        const ff::PushKernelEntry& k = ff::g_push_kernels[index];
        if (!k.launch || !shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation != FF_ACT_SILU) return false;
        d->family = kPush; d->name = k.name; d->one_wave = k.launch;
        twin_line(d, k.wps);
        d->tangents = 1; d->nets = 1; d->row_nets = 1; d->exchange = 2;
        return true;
    }
    const bool select = p->kernel_id >= FF_PAIR_SELECT_KERNEL_BASE;
    const int index = p->kernel_id - (select ? FF_PAIR_SELECT_KERNEL_BASE : FF_PAIR_KERNEL_BASE);
    if (index < 0 || index >= ff::g_n_pair_kernels) return false;
    const ff::PairKernelEntry& k = ff::g_pair_kernels[index];
    const ff::Launchers& l = select ? k.select : k.pair;
    if (!l.one_wave || !shape_ok(p, k.tile, k.H, k.dregs, k.cregs) || p->activation != FF_ACT_SILU || p->dim % 2 != 0) return false;
    d->family = select ? kSelect : kPair; d->name = l.name; d->one_wave = l.one_wave; d->coop = l.coop;
    twin_line(d, k.wps);
    if (k.wps >= 3) { d->c0 = 0.03; d->per_round = 0.85; }      // the 128-wide pair and select twins' own line
    d->state_only = true; d->nets = 2; d->exchange = 2;
    d->row_nets = select ? 1 : 2;                                // a select row carries the c1 of the one network it runs
    d->max_aux = select ? 0 : FF_MAX_AUX; d->takes_k1 = !select; // no first stage from the caller, no auxiliary outputs
    d->checks_noise_stride = true;
    return true;
}

static ff::Layout plan_layout(const ff_mlp_plan_t* p)
{
    return ff::make_layout(p->tile, p->width, p->dregs, p->cregs, p->n_hidden);
}

// The transposed network of a pull plan (ff_mlp_pull.hpp, net B): an ordinary network whose state registers are the forward
// network's state AND conditional registers, without conditional inputs of its own.
static ff::Layout pull_layout(const ff_mlp_plan_t* p)
{
    return ff::make_layout(p->tile, p->width, p->dregs + p->cregs, 0, p->n_hidden);
}

// Dynamic LDS of one pull tile with K cotangent columns per sample: `slots` stage slots (dregs + cregs words per slot and
// lane), then the slope stash, n_hidden x width words for each of its tile / (1 + K) samples.
static size_t pull_lds_bytes(const ff_mlp_plan_t* p, int K, int n_slots = ff::kSlots)
{
    const size_t slots = (size_t)n_slots * ((p->dregs + p->cregs) / 4) * 64 * 16;
    return slots + (size_t)(p->tile / (1 + K)) * p->n_hidden * p->width * 4;
}
constexpr size_t kPullLdsLimit = 160u * 1024u;      // LDS of a compute unit = the most a workgroup can ask for

// The same of a products tile (ff_mlp_vjp.hpp): the stash is the pull tile's, a stage slot holds dregs words per lane -- the
// seed columns integrate nothing and no conditional part is carried.
static size_t vjp_lds_bytes(const ff_mlp_plan_t* p, int K, int n_slots = ff::kSlots)
{
    const size_t slots = (size_t)n_slots * (p->dregs / 4) * 64 * 16;
    return slots + (size_t)(p->tile / (1 + K)) * p->n_hidden * p->width * 4;
}

// The same of a record tile (ff_mlp_dadj.hpp): stage slots of dregs words per lane and nothing else.  A discrete-adjoint tile
// takes vjp_lds_bytes: adjoint slots of dregs words per lane and the pull tile's stash.
static size_t rec_lds_bytes(const ff_mlp_plan_t* p, int n_slots = ff::kSlots)
{
    return (size_t)n_slots * (p->dregs / 4) * 64 * 16;
}

// The same of a log-density gradient tile (ff_mlp_lgrad.hpp): adjoint slots of dregs words per lane, then two words per hidden
// unit for each of its tile / 2 rows.
static size_t lgrad_lds_bytes(const ff_mlp_plan_t* p, int n_slots = ff::kSlots)
{
    const size_t slots = (size_t)n_slots * (p->dregs / 4) * 64 * 16;
    return slots + (size_t)(p->tile / 2) * p->n_hidden * p->width * 2 * 4;
}

extern "C" const char* ff_plan_kernel_name(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) ? d.name : NULL;
}

// ff_adaptive.hip: plans ff_mlp_ode_adaptive takes -- every valid plan but the select plans (fixed tables only)
namespace ff {
bool plan_steps_adaptively(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) && d.family != kSelect && d.family != kPush && d.family != kPull && d.family != kPullSel && d.family != kPushSel;
}
}

extern "C" int ff_pair_kernel_count(void) { return ff::g_n_pair_kernels; }

extern "C" const char* ff_pair_kernel_name(int index)
{
    return index >= 0 && index < ff::g_n_pair_kernels ? ff::g_pair_kernels[index].pair.name : NULL;
}

extern "C" int ff_mlp_row_width(const ff_mlp_plan_t* plan)
{
    if (!plan) return -1;
    LaunchDesc d;
    return describe(plan, &d) ? d.row_nets * plan->width : plan->width;
}

extern "C" int ff_push_kernel_count(void) { return ff::g_n_push_kernels; }

extern "C" const char* ff_push_kernel_name(int index)
{
    return index >= 0 && index < ff::g_n_push_kernels ? ff::g_push_kernels[index].name : NULL;
}

// the smallest push-forward unit that holds the network (best_entry's preference: narrowest width, then fewest first-layer
// features): SiLU, fp32
extern "C" int ff_mlp_push_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision,
                                ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 1 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    if (activation < 0 || activation >= FF_ACT_COUNT) return FF_ERR_BADARG;
    if (precision != FF_PREC_F32 && precision != FF_PREC_BF16X3 && precision != FF_PREC_BF16X2) return FF_ERR_BADARG;
    const int wmax = widest(n_hidden, hidden_widths);
    if (wmax < 0) return FF_ERR_BADARG;
    if (activation != FF_ACT_SILU || precision != FF_PREC_F32) return FF_ERR_UNSUPPORTED;
    const int best = best_entry(ff::g_push_kernels, ff::g_n_push_kernels, dim, cond_dim, wmax,
                                [](const ff::PushKernelEntry& k) { return k.launch != nullptr; });
    if (best < 0) return FF_ERR_UNSUPPORTED;
    const ff::PushKernelEntry& k = ff::g_push_kernels[best];
    return fill_plan(plan, dim, cond_dim, n_hidden, k.H, k.dregs, k.cregs, FF_PUSH_KERNEL_BASE + best, k.tile, FF_ACT_SILU);
}

extern "C" int ff_pushsel_kernel_count(void) { return n_pushsel_kernels(); }

extern "C" const char* ff_pushsel_kernel_name(int index)
{
    return index >= 0 && index < n_pushsel_kernels() ? ff::g_pushsel_kernels[index].name : NULL;
}

// the push plan of the joint state (one envelope, one preference), carried over to the sibling unit
extern "C" int ff_mlp_push_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 2 || dim % 2 != 0 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    const int rc = ff_mlp_push_plan(dim, cond_dim, n_hidden, hidden_widths, FF_ACT_SILU, FF_PREC_F32, plan);
    if (rc != FF_OK) return rc;
    const ff::PushKernelEntry& k = ff::g_push_kernels[plan->kernel_id - FF_PUSH_KERNEL_BASE];
    bool found = false;
    for (int i = 0; i < n_pushsel_kernels() && !found; ++i) {
        const ff::PushKernelEntry& s = ff::g_pushsel_kernels[i];
        if (s.launch && s.tile == k.tile && s.H == k.H && s.dregs == k.dregs && s.cregs == k.cregs) {
            plan->kernel_id = FF_PUSH_SELECT_KERNEL_BASE + i;
            found = true;
        }
    }
    if (!found) { memset(plan, 0, sizeof(*plan)); return FF_ERR_UNSUPPORTED; }
    return FF_OK;
}

// two forward packs back to back: mlp_q's, then mlp_p's
extern "C" size_t ff_mlp_push_select_wpack_floats(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) && d.family == kPushSel ? 2 * plan_layout(plan).total_floats : 0;
}

extern "C" int ff_pull_kernel_count(void) { return ff::g_n_pull_kernels; }

extern "C" const char* ff_pull_kernel_name(int index)
{
    return index >= 0 && index < ff::g_n_pull_kernels ? ff::g_pull_kernels[index].name : NULL;
}

// The products table is a WEAK reference here: a program that links this file with kernel tables of its own from before the
// products units (tests/sanitize/pull_wpack_main.cpp) still links, and sees a library without products units.
namespace ff {
extern const PullKernelEntry g_vjp_kernels[] __attribute__((weak));
extern const int g_n_vjp_kernels __attribute__((weak));
}
static int n_vjp_kernels() { return &ff::g_n_vjp_kernels ? ff::g_n_vjp_kernels : 0; }

extern "C" int ff_vjp_kernel_count(void) { return n_vjp_kernels(); }

extern "C" const char* ff_vjp_kernel_name(int index)
{
    return index >= 0 && index < n_vjp_kernels() ? ff::g_vjp_kernels[index].name : NULL;
}

// The record and discrete-adjoint tables: weak for the same reason.
namespace ff {
extern const PullKernelEntry g_rec_kernels[] __attribute__((weak));
extern const int g_n_rec_kernels __attribute__((weak));
extern const PullKernelEntry g_dadj_kernels[] __attribute__((weak));
extern const int g_n_dadj_kernels __attribute__((weak));
}
static int n_rec_kernels() { return &ff::g_n_rec_kernels ? ff::g_n_rec_kernels : 0; }
static int n_dadj_kernels() { return &ff::g_n_dadj_kernels ? ff::g_n_dadj_kernels : 0; }

extern "C" int ff_rec_kernel_count(void) { return n_rec_kernels(); }

extern "C" const char* ff_rec_kernel_name(int index)
{
    return index >= 0 && index < n_rec_kernels() ? ff::g_rec_kernels[index].name : NULL;
}

extern "C" int ff_dadj_kernel_count(void) { return n_dadj_kernels(); }

extern "C" const char* ff_dadj_kernel_name(int index)
{
    return index >= 0 && index < n_dadj_kernels() ? ff::g_dadj_kernels[index].name : NULL;
}

// The log-density gradient table: weak for the same reason.
namespace ff {
extern const PullKernelEntry g_lgrad_kernels[] __attribute__((weak));
extern const int g_n_lgrad_kernels __attribute__((weak));
}
static int n_lgrad_kernels() { return &ff::g_n_lgrad_kernels ? ff::g_n_lgrad_kernels : 0; }

extern "C" int ff_lgrad_kernel_count(void) { return n_lgrad_kernels(); }

extern "C" const char* ff_lgrad_kernel_name(int index)
{
    return index >= 0 && index < n_lgrad_kernels() ? ff::g_lgrad_kernels[index].name : NULL;
}

// floats of the record of a solve: one stage state per evaluation row and sample; 0 for arguments that describe none
extern "C" size_t ff_mlp_record_floats(int64_t batch, int32_t n_evals, int32_t dim)
{
    if (batch < 0 || n_evals < 0 || dim < 0) return 0;
    return (size_t)batch * (size_t)n_evals * (size_t)dim;
}

// the smallest pull-back unit that holds the network (best_entry's preference), SiLU, fp32 -- and whose slope stash fits the
// LDS at its largest, one cotangent per sample
extern "C" int ff_mlp_pull_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision,
                                ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 1 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    if (activation < 0 || activation >= FF_ACT_COUNT) return FF_ERR_BADARG;
    if (precision != FF_PREC_F32 && precision != FF_PREC_BF16X3 && precision != FF_PREC_BF16X2) return FF_ERR_BADARG;
    const int wmax = widest(n_hidden, hidden_widths);
    if (wmax < 0) return FF_ERR_BADARG;
    if (activation != FF_ACT_SILU || precision != FF_PREC_F32) return FF_ERR_UNSUPPORTED;
    const int best = best_entry(ff::g_pull_kernels, ff::g_n_pull_kernels, dim, cond_dim, wmax,
                                [](const ff::PullKernelEntry& k) { return k.launch != nullptr; });
    if (best < 0) return FF_ERR_UNSUPPORTED;
    const ff::PullKernelEntry& k = ff::g_pull_kernels[best];
    fill_plan(plan, dim, cond_dim, n_hidden, k.H, k.dregs, k.cregs, FF_PULL_KERNEL_BASE + best, k.tile, FF_ACT_SILU);
    if (pull_lds_bytes(plan, 1) > kPullLdsLimit) { memset(plan, 0, sizeof(*plan)); return FF_ERR_UNSUPPORTED; }
    return FF_OK;
}

extern "C" size_t ff_mlp_pull_wpack_floats(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) && d.family == kPull ? plan_layout(plan).total_floats + pull_layout(plan).total_floats : 0;
}

extern "C" int ff_pullsel_kernel_count(void) { return n_pullsel_kernels(); }

extern "C" const char* ff_pullsel_kernel_name(int index)
{
    return index >= 0 && index < n_pullsel_kernels() ? ff::g_pullsel_kernels[index].name : NULL;
}

// the pull plan of the joint state (one envelope, one preference, the same depth ceilings), carried over to the sibling unit
extern "C" int ff_mlp_pull_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 2 || dim % 2 != 0 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    const int rc = ff_mlp_pull_plan(dim, cond_dim, n_hidden, hidden_widths, FF_ACT_SILU, FF_PREC_F32, plan);
    if (rc != FF_OK) return rc;
    const int index = plan->kernel_id - FF_PULL_KERNEL_BASE;
    const ff::PullKernelEntry& k = ff::g_pull_kernels[index];
    bool found = false;
    for (int i = 0; i < n_pullsel_kernels() && !found; ++i) {
        const ff::PullKernelEntry& s = ff::g_pullsel_kernels[i];
        if (s.launch && s.tile == k.tile && s.H == k.H && s.dregs == k.dregs && s.cregs == k.cregs) {
            plan->kernel_id = FF_PULL_SELECT_KERNEL_BASE + i;
            found = true;
        }
    }
    if (!found) { memset(plan, 0, sizeof(*plan)); return FF_ERR_UNSUPPORTED; }
    return FF_OK;
}

// two pull packs back to back: [A_q | B_q | A_p | B_p]
extern "C" size_t ff_mlp_pull_select_wpack_floats(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) && d.family == kPullSel ? 2 * (plan_layout(plan).total_floats + pull_layout(plan).total_floats) : 0;
}

extern "C" int ff_mlp_pair_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan)
{
    const int rc = ff_mlp_pair_plan(dim, cond_dim, n_hidden, hidden_widths, plan);      // one envelope, one preference
    if (rc != FF_OK) return rc;
    const int index = plan->kernel_id - FF_PAIR_KERNEL_BASE;
    if (ff::g_pair_kernels[index].select.one_wave == nullptr) { memset(plan, 0, sizeof(*plan)); return FF_ERR_UNSUPPORTED; }
    plan->kernel_id = FF_PAIR_SELECT_KERNEL_BASE + index;
    return FF_OK;
}

extern "C" int ff_mlp_pair_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan)
{
    if (!plan || !hidden_widths || dim < 2 || dim % 2 != 0 || cond_dim < 0 || n_hidden < 1) return FF_ERR_BADARG;
    const int wmax = widest(n_hidden, hidden_widths);
    if (wmax < 0) return FF_ERR_BADARG;
    const int best = best_entry(ff::g_pair_kernels, ff::g_n_pair_kernels, dim, cond_dim, wmax, [](const ff::PairKernelEntry&) { return true; });
    if (best < 0) return FF_ERR_UNSUPPORTED;
    const ff::PairKernelEntry& k = ff::g_pair_kernels[best];
    return fill_plan(plan, dim, cond_dim, n_hidden, k.H, k.dregs, k.cregs, FF_PAIR_KERNEL_BASE + best, k.tile, FF_ACT_SILU);
}

extern "C" size_t ff_mlp_pair_wpack_floats(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    return describe(plan, &d) && d.nets == 2 && d.family != kPullSel && d.family != kPushSel ? 2 * plan_layout(plan).total_floats : 0;
}

extern "C" size_t ff_mlp_wpack_floats(const ff_mlp_plan_t* plan)
{
    LaunchDesc d;
    if (!describe(plan, &d)) return 0;
    if (d.family == kSplit) return ff::split::total_words(plan->n_hidden, split_parts(plan->precision), plan->dregs / 8, plan->width);
    if (d.family == kPull || d.family == kPullSel) return 0;      // (two packs: ff_mlp_pull_wpack_floats; four: ff_mlp_pull_select_wpack_floats)
    return d.nets == 1 ? plan_layout(plan).total_floats : 0;
}

// three-way bf16 split by truncation: v = hi + mid + lo exactly (8 + 8 + 8 significand bits)
static inline uint16_t bf16_top(float v, float* rest)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint32_t t = u & 0xFFFF0000u;
    float tf;
    memcpy(&tf, &t, 4);
    *rest = v - tf;
    return (uint16_t)(t >> 16);
}

// round-to-nearest-even bf16 of v (weights are finite), and what is left
static inline uint16_t bf16_rne(float v, float* rest)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint32_t t = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    float tf;
    memcpy(&tf, &t, 4);
    *rest = v - tf;
    return (uint16_t)(t >> 16);
}

// FF_PREC_BF16X3 / BF16X2 packing: the fragment stream of ff_split_layout.h followed by the fp32 biases.  Three parts:
// truncation (hi + mid + lo = the fp32 weight exactly); two parts: round to nearest (hi + mid = the weight to 16 bits)
static int wpack_split(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b,
                       const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out)
{
    namespace sp = ff::split;
    const int D = plan->dim, C = plan->cond_dim, H = plan->width, NH = plan->n_hidden;
    const int NP = split_parts(plan->precision), DT = plan->dregs / 8;
    uint32_t* words = (uint32_t*)out;
    const int NR = sp::row_tiles(H), NS = sp::ksteps(H);
    memset(out, 0, sp::total_words(NH, NP, DT, H) * 4);
    size_t group = 0;                                  // running group index in the stream
    // one group: fragments [hi, mid, lo] of 16-row tile rt; element (quad q, j) multiplies input column col(q, j)
    auto put_group = [&](const float* Wl, int rows, int ld, int rt, auto col) {
        uint32_t* g = words + group * (NP * sp::kFragBytes / 4);
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int row = 16 * rt + (lane & 15), c = col(lane >> 4, j);
                const float v = (row < rows && c >= 0) ? Wl[(size_t)row * ld + c] : 0.f;
                float r1, r2, r3;
                uint16_t part[3];
                if (NP == 3) {
                    part[0] = bf16_top(v, &r1); part[1] = bf16_top(r1, &r2); part[2] = bf16_top(r2, &r3);
                } else {
                    part[0] = bf16_rne(v, &r1); part[1] = bf16_rne(r1, &r2); part[2] = 0;
                }
                for (int p = 0; p < NP; ++p) {
                    uint32_t& w = g[p * 256 + lane * 4 + (j >> 1)];
                    w = (j & 1) ? ((w & 0x0000FFFFu) | ((uint32_t)part[p] << 16)) : ((w & 0xFFFF0000u) | part[p]);
                }
            }
        ++group;
    };
    // layer 1: ONE k-step -- features 0..15 the state dimensions, 16..31 the conditional inputs; states of up to 32
    // dimensions: TWO k-steps -- features 0..31 the state, then 0..15 the conditional inputs
    for (int s1 = 0; s1 < DT; ++s1)
        for (int rt = 0; rt < NR; ++rt)
            put_group(W[0], hidden_widths[0], in_features0, rt, [&](int q, int j) {
                const int f = sp::kidx(0, q, j);
                if (DT == 1) return f < 16 ? (f < D ? x_col0 + f : -1) : (f - 16 < C ? c_col0 + f - 16 : -1);
                return s1 == 0 ? (f < D ? x_col0 + f : -1) : (f < C ? c_col0 + f : -1);
            });
    // hidden -> hidden, k-major: k-step s, row tile rt
    for (int l = 1; l < NH; ++l) {
        const int win = hidden_widths[l - 1], wout = hidden_widths[l];
        for (int s = 0; s < NS; ++s)
            for (int rt = 0; rt < NR; ++rt)
                put_group(W[l], wout, win, rt, [&](int q, int j) {
                    const int kk = sp::kidx(s, q, j);
                    return kk < win ? kk : -1;
                });
        float* bo = out + sp::stream_words(NH, NP, DT, H) + (size_t)(l - 1) * H;
        for (int row = 0; row < wout; ++row) bo[row] = b[l][row];
    }
    // output layer: DT row tiles (the state's dimensions), k-major
    {
        const int win = hidden_widths[NH - 1];
        for (int s = 0; s < NS; ++s)
            for (int t = 0; t < DT; ++t)
                put_group(W[NH], D, win, t, [&](int q, int j) {
                    const int kk = sp::kidx(s, q, j);
                    return kk < win ? kk : -1;
                });
        float* bo = out + sp::stream_words(NH, NP, DT, H) + (size_t)(NH - 1) * H;
        for (int row = 0; row < D; ++row) bo[row] = b[NH][row];
    }
    return group == (size_t)sp::granules_per_eval(NH, DT, H) * sp::granule_groups(H) ? FF_OK : FF_ERR_BADARG;
}

static int wpack_f32(const ff::Layout& L, int D, int C, const float* const* W, const float* const* b,
                     const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out);

extern "C" int ff_mlp_wpack(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b,
                            const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out)
{
    LaunchDesc d;
    if (!describe(plan, &d) || d.nets == 2 || d.family == kPull) return FF_ERR_BADARG;
    if (d.family == kSplit) {
        if (!W || !b || !hidden_widths || !out) return FF_ERR_BADARG;
        const int D = plan->dim, C = plan->cond_dim, NH = plan->n_hidden;
        if (x_col0 < 0 || x_col0 + D > in_features0) return FF_ERR_BADARG;
        if (C > 0 && (c_col0 < 0 || c_col0 + C > in_features0)) return FF_ERR_BADARG;
        for (int i = 0; i < NH; ++i)
            if (hidden_widths[i] < 1 || hidden_widths[i] > plan->width) return FF_ERR_BADARG;
        for (int i = 0; i <= NH; ++i)
            if (!W[i] || (i > 0 && !b[i])) return FF_ERR_BADARG;
        return wpack_split(plan, W, b, hidden_widths, in_features0, x_col0, c_col0, out);
    }
    if (!W || !b || !hidden_widths || !out) return FF_ERR_BADARG;
    const int D = plan->dim, C = plan->cond_dim, H = plan->width, NH = plan->n_hidden;
    if (x_col0 < 0 || x_col0 + D > in_features0) return FF_ERR_BADARG;
    if (C > 0 && (c_col0 < 0 || c_col0 + C > in_features0)) return FF_ERR_BADARG;
    for (int i = 0; i < NH; ++i)
        if (hidden_widths[i] < 1 || hidden_widths[i] > H) return FF_ERR_BADARG;
    for (int i = 0; i <= NH; ++i)
        if (!W[i] || (i > 0 && !b[i])) return FF_ERR_BADARG;
    return wpack_f32(plan_layout(plan), D, C, W, b, hidden_widths, in_features0, x_col0, c_col0, out);
}

// The fp32 packing of one network of layout L (arguments checked by the callers): D state / network outputs, C conditional
// inputs (ff_layout.h: the chunks of every layer in consumption order, then the biases).
static int wpack_f32(const ff::Layout& L, int D, int C, const float* const* W, const float* const* b,
                     const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out)
{
    const int NH = L.n_hidden;
    const int TL = L.tile, PHYS = ff::tile_phys(TL), CF = L.chunk_fl;
    memset(out, 0, L.total_floats * sizeof(float));

    // Fill the chunks of one layer in consumption order (ff_layout.h).  `kcol(r, h)` maps operand
    // register r on lane-half h to a column of `Wl` (or -1 for padding), rows beyond `rows` are zero.
    auto fill = [&](const ff::LayerGeom& G, float* o, const float* Wl, int rows, int ld, auto kcol) {
        for (int c = 0; c < G.NC; ++c) {
            const int g = ff::chunk_group(G, c), ob = ff::chunk_block(G, c);
            for (int p = 0; p < PHYS; ++p)
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < 4; ++q) {
                        const int row = ob * 32 + TL * p + (lane & (TL - 1));
                        const int col = kcol(4 * g + q, lane / TL);
                        o[(size_t)c * CF + ((size_t)p * 64 + lane) * 4 + q] =
                            (row < rows && col >= 0) ? Wl[(size_t)row * ld + col] : 0.f;
                    }
        }
    };
    // first layer: operand registers = [state | conditional]
    fill(L.g1, out, W[0], hidden_widths[0], in_features0, [&](int r, int h) {
        if (r < L.dregs) {
            const int d = ff::feat_of_reg(TL, r, h);
            return d < D ? x_col0 + d : -1;
        }
        const int d = ff::feat_of_reg(TL, r - L.dregs, h);
        return d < C ? c_col0 + d : -1;
    });
    // hidden -> hidden
    for (int l = 1; l < NH; ++l) {
        const int win = hidden_widths[l - 1], wout = hidden_widths[l];
        fill(L.gh, out + (size_t)L.chunk_off_hid(l - 1) * CF, W[l], wout, win, [&](int r, int h) {
            const int k = ff::feat_of_reg(TL, r, h);
            return k < win ? k : -1;
        });
        float* bo = out + L.bias_off_hid(l - 1);
        for (int row = 0; row < wout; ++row) bo[row] = b[l][row];
    }
    // output layer
    {
        const int win = hidden_widths[NH - 1];
        fill(L.go, out + (size_t)L.chunk_off_out() * CF, W[NH], D, win, [&](int r, int h) {
            const int k = ff::feat_of_reg(TL, r, h);
            return k < win ? k : -1;
        });
        float* bo = out + L.bias_off_out();
        for (int row = 0; row < D; ++row) bo[row] = b[NH][row];
    }
    return FF_OK;
}

// Pull packing (ff_mlp_pull.hpp): the forward network as ff_mlp_wpack packs it, then the transposed network as an ordinary
// network of pull_layout -- first layer W_out^T (D -> h_L), hidden layers W_L^T .. W_2^T, output layer the x and c columns of
// W_1 as rows -- with zero biases.  Its "state" is the combined feature space of the forward network's first-layer registers:
// feature F sits on register R, lane group q with feat_of_reg(R, q) == F; R < dregs is state dimension F, R >= dregs the
// conditional input feat_of_reg(R - dregs, q).
extern "C" int ff_mlp_pull_wpack(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b, const int* hidden_widths,
                                 int in_features0, int x_col0, int c_col0, float* out)
{
    LaunchDesc d;
    if (!describe(plan, &d) || d.family != kPull || !W || !b || !hidden_widths || !out) return FF_ERR_BADARG;
    const int D = plan->dim, C = plan->cond_dim, H = plan->width, NH = plan->n_hidden;
    if (x_col0 < 0 || x_col0 + D > in_features0) return FF_ERR_BADARG;
    if (C > 0 && (c_col0 < 0 || c_col0 + C > in_features0)) return FF_ERR_BADARG;
    for (int i = 0; i < NH; ++i)
        if (hidden_widths[i] < 1 || hidden_widths[i] > H) return FF_ERR_BADARG;
    for (int i = 0; i <= NH; ++i)
        if (!W[i] || (i > 0 && !b[i])) return FF_ERR_BADARG;
    const ff::Layout L = plan_layout(plan), LT = pull_layout(plan);
    int rc = wpack_f32(L, D, C, W, b, hidden_widths, in_features0, x_col0, c_col0, out);
    if (rc != FF_OK) return rc;
    const int NQ = ff::tile_nq(plan->tile), K1 = plan->dregs + plan->cregs, FB = NQ * K1;      // combined features
    const int h0 = hidden_widths[0], hl = hidden_widths[NH - 1];
    // combined feature -> column of W_1 (>= 0), and -> row of W_out (>= 0), or -1
    int* const col1 = (int*)malloc((size_t)FB * sizeof(int));
    int* const rowo = (int*)malloc((size_t)FB * sizeof(int));
    float* const wf = (float*)calloc((size_t)hl * FB, sizeof(float));              // first layer  [h_L x FB] = W_out^T
    float* const wl = (float*)calloc((size_t)FB * h0, sizeof(float));              // output layer [FB x h_1] = W_1^T
    float* const zb = (float*)calloc((size_t)(H > FB ? H : FB), sizeof(float));    // zero biases
    float* const wt = (float*)calloc((size_t)(NH > 1 ? NH - 1 : 1) * H * H, sizeof(float));      // hidden layers, transposed
    const float** const Wl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    const float** const bl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    int* const hw = (int*)calloc((size_t)NH, sizeof(int));
    rc = (col1 && rowo && wf && wl && zb && wt && Wl && bl && hw) ? FF_OK : FF_ERR_BADARG;
    if (rc == FF_OK) {
        for (int F = 0; F < FB; ++F) col1[F] = rowo[F] = -1;
        for (int R = 0; R < K1; ++R)
            for (int q = 0; q < NQ; ++q) {
                const int F = ff::feat_of_reg(plan->tile, R, q);
                if (F < 0 || F >= FB) { rc = FF_ERR_BADARG; continue; }
                if (R < plan->dregs) {
                    if (F < D) { col1[F] = x_col0 + F; rowo[F] = F; }
                } else {
                    const int c = ff::feat_of_reg(plan->tile, R - plan->dregs, q);
                    if (c < C) col1[F] = c_col0 + c;
                }
            }
    }
    if (rc == FF_OK) {
        for (int F = 0; F < FB; ++F) {
            if (rowo[F] >= 0)
                for (int k = 0; k < hl; ++k) wf[(size_t)k * FB + F] = W[NH][(size_t)rowo[F] * hl + k];
            if (col1[F] >= 0)
                for (int k = 0; k < h0; ++k) wl[(size_t)F * h0 + k] = W[0][(size_t)k * in_features0 + col1[F]];
        }
        // transposed hidden layer j = 1 .. NH - 1 is W[NH - j]^T: hidden_widths[NH - j] -> hidden_widths[NH - j - 1]
        for (int j = 0; j < NH; ++j) hw[j] = hidden_widths[NH - 1 - j];
        Wl[0] = wf; bl[0] = nullptr;
        for (int j = 1; j < NH; ++j) {
            const float* const src = W[NH - j];
            const int win = hidden_widths[NH - j], wout = hidden_widths[NH - j - 1];      // of the TRANSPOSED layer
            float* const dst = wt + (size_t)(j - 1) * H * H;
            for (int r = 0; r < wout; ++r)
                for (int k = 0; k < win; ++k) dst[(size_t)r * win + k] = src[(size_t)k * wout + r];
            Wl[j] = dst; bl[j] = zb;
        }
        Wl[NH] = wl; bl[NH] = zb;
        rc = wpack_f32(LT, FB, 0, Wl, bl, hw, FB, 0, 0, out + L.total_floats);
    }
    free(col1); free(rowo); free(wf); free(wl); free(zb); free(wt); free(Wl); free(bl); free(hw);
    return rc;
}

// Pull-select packing (ff_mlp_pullsel.hpp): each network embedded in the whole joint state [q | p] exactly as ff_mlp_pair_wpack
// embeds it, then packed as ff_mlp_pull_wpack packs a network -- mlp_q's pull pack, then mlp_p's.
extern "C" int ff_mlp_pull_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                                        const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                                        int x_col0, int c_col0, float* out)
{
    LaunchDesc d;
    if (!describe(plan, &d) || d.family != kPullSel || !Wq || !bq || !Wp || !bp || !hidden_widths || !out) return FF_ERR_BADARG;
    const int D2 = plan->dim, Dh = D2 / 2, C = plan->cond_dim, H = plan->width, NH = plan->n_hidden;
    if (x_col0 < 0 || x_col0 + Dh > in_features0) return FF_ERR_BADARG;
    if (C > 0 && (c_col0 < 0 || c_col0 + C > in_features0)) return FF_ERR_BADARG;
    for (int i = 0; i < NH; ++i)
        if (hidden_widths[i] < 1 || hidden_widths[i] > H) return FF_ERR_BADARG;
    for (int i = 0; i <= NH; ++i)
        if (!Wq[i] || !Wp[i] || (i > 0 && (!bq[i] || !bp[i]))) return FF_ERR_BADARG;
    // the sibling pull plan: same shape, the pull family's id -- what ff_mlp_pull_wpack takes
    ff_mlp_plan_t pp = *plan;
    pp.kernel_id = -1;
    for (int i = 0; i < ff::g_n_pull_kernels; ++i) {
        const ff::PullKernelEntry& k = ff::g_pull_kernels[i];
        if (k.launch && k.tile == plan->tile && k.H == plan->width && k.dregs == plan->dregs && k.cregs == plan->cregs) { pp.kernel_id = FF_PULL_KERNEL_BASE + i; break; }
    }
    if (pp.kernel_id < 0) return FF_ERR_BADARG;
    const size_t half_floats = plan_layout(plan).total_floats + pull_layout(plan).total_floats;
    const int h0 = hidden_widths[0], hl = hidden_widths[NH - 1], in1 = D2 + C;
    float* const w1 = (float*)calloc((size_t)h0 * in1, sizeof(float));
    float* const wo = (float*)calloc((size_t)D2 * hl, sizeof(float));
    float* const bo = (float*)calloc((size_t)D2, sizeof(float));
    const float** const Wl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    const float** const bl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    int rc = (w1 && wo && bo && Wl && bl) ? FF_OK : FF_ERR_BADARG;
    for (int half = 0; half < 2 && rc == FF_OK; ++half) {
        const float* const* W = half ? Wp : Wq;
        const float* const* b = half ? bp : bq;
        const int in_col = half ? 0 : Dh;        // state columns this network reads: p (mlp_q) or q (mlp_p)
        const int out_row = half ? Dh : 0;       // state rows it writes
        const float sgn = half ? -1.f : 1.f;
        memset(w1, 0, (size_t)h0 * in1 * sizeof(float));
        memset(wo, 0, (size_t)D2 * hl * sizeof(float));
        memset(bo, 0, (size_t)D2 * sizeof(float));
        for (int r = 0; r < h0; ++r) {
            for (int dd = 0; dd < Dh; ++dd) w1[(size_t)r * in1 + in_col + dd] = W[0][(size_t)r * in_features0 + x_col0 + dd];
            for (int c = 0; c < C; ++c) w1[(size_t)r * in1 + D2 + c] = W[0][(size_t)r * in_features0 + c_col0 + c];
        }
        for (int r = 0; r < Dh; ++r) {
            for (int k = 0; k < hl; ++k) wo[(size_t)(out_row + r) * hl + k] = sgn * W[NH][(size_t)r * hl + k];
            bo[out_row + r] = sgn * b[NH][r];
        }
        Wl[0] = w1; bl[0] = nullptr;
        for (int l = 1; l < NH; ++l) { Wl[l] = W[l]; bl[l] = b[l]; }
        Wl[NH] = wo; bl[NH] = bo;
        rc = ff_mlp_pull_wpack(&pp, Wl, bl, hidden_widths, in1, 0, D2, out + (size_t)half * half_floats);
    }
    free(w1); free(wo); free(bo); free(Wl); free(bl);
    return rc;
}

// Push-select packing (ff_mlp_pushsel.hpp): two forward packs, each network embedded in the whole joint state [q | p] and packed
// exactly as ff_mlp_pair_wpack embeds and packs it.
static int pair_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq, const float* const* Wp,
                      const float* const* bp, const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out);

extern "C" int ff_mlp_push_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                                        const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                                        int x_col0, int c_col0, float* out)
{
    LaunchDesc d;
    if (!describe(plan, &d) || d.family != kPushSel) return FF_ERR_BADARG;
    return pair_wpack(plan, Wq, bq, Wp, bp, hidden_widths, in_features0, x_col0, c_col0, out);
}

// Pair packing: each reference network becomes an ordinary network over the whole state [q | p] (its first layer reads
// its own half -- p for mlp_q, q for mlp_p -- and has zero columns on the other; its output layer writes its own half,
// negated for mlp_p, and zero rows on the other), packed by wpack_f32; net A's pack, then net B's.
extern "C" int ff_mlp_pair_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                                 const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                                 int x_col0, int c_col0, float* out)
{
    LaunchDesc d;
    if (!describe(plan, &d) || d.nets != 2 || d.family == kPullSel || d.family == kPushSel) return FF_ERR_BADARG;
    return pair_wpack(plan, Wq, bq, Wp, bp, hidden_widths, in_features0, x_col0, c_col0, out);
}

// (the plan is one of two networks: the callers have looked)
static int pair_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq, const float* const* Wp,
                      const float* const* bp, const int* hidden_widths, int in_features0, int x_col0, int c_col0, float* out)
{
    if (!Wq || !bq || !Wp || !bp || !hidden_widths || !out) return FF_ERR_BADARG;
    const int D2 = plan->dim, Dh = D2 / 2, C = plan->cond_dim, H = plan->width, NH = plan->n_hidden;
    if (x_col0 < 0 || x_col0 + Dh > in_features0) return FF_ERR_BADARG;
    if (C > 0 && (c_col0 < 0 || c_col0 + C > in_features0)) return FF_ERR_BADARG;
    for (int i = 0; i < NH; ++i)
        if (hidden_widths[i] < 1 || hidden_widths[i] > H) return FF_ERR_BADARG;
    for (int i = 0; i <= NH; ++i)
        if (!Wq[i] || !Wp[i] || (i > 0 && (!bq[i] || !bp[i]))) return FF_ERR_BADARG;
    const ff::Layout L = plan_layout(plan);
    const int h0 = hidden_widths[0], hl = hidden_widths[NH - 1], in1 = D2 + C;
    float* const w1 = (float*)calloc((size_t)h0 * in1, sizeof(float));
    float* const wo = (float*)calloc((size_t)D2 * hl, sizeof(float));
    float* const bo = (float*)calloc((size_t)D2, sizeof(float));
    const float** const Wl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    const float** const bl = (const float**)calloc((size_t)NH + 1, sizeof(float*));
    int rc = (w1 && wo && bo && Wl && bl) ? FF_OK : FF_ERR_BADARG;
    for (int half = 0; half < 2 && rc == FF_OK; ++half) {
        const float* const* W = half ? Wp : Wq;
        const float* const* b = half ? bp : bq;
        const int in_col = half ? 0 : Dh;        // state columns this network reads: p (mlp_q) or q (mlp_p)
        const int out_row = half ? Dh : 0;       // state rows it writes
        const float sgn = half ? -1.f : 1.f;
        memset(w1, 0, (size_t)h0 * in1 * sizeof(float));
        memset(wo, 0, (size_t)D2 * hl * sizeof(float));
        memset(bo, 0, (size_t)D2 * sizeof(float));
        for (int r = 0; r < h0; ++r) {
            for (int d = 0; d < Dh; ++d) w1[(size_t)r * in1 + in_col + d] = W[0][(size_t)r * in_features0 + x_col0 + d];
            for (int c = 0; c < C; ++c) w1[(size_t)r * in1 + D2 + c] = W[0][(size_t)r * in_features0 + c_col0 + c];
        }
        for (int r = 0; r < Dh; ++r) {
            for (int k = 0; k < hl; ++k) wo[(size_t)(out_row + r) * hl + k] = sgn * W[NH][(size_t)r * hl + k];
            bo[out_row + r] = sgn * b[NH][r];
        }
        Wl[0] = w1; bl[0] = nullptr;
        for (int l = 1; l < NH; ++l) { Wl[l] = W[l]; bl[l] = b[l]; }
        Wl[NH] = wo; bl[NH] = bo;
        rc = wpack_f32(L, D2, C, Wl, bl, hidden_widths, in1, 0, D2, out + (size_t)half * L.total_floats);
    }
    free(w1); free(wo); free(bo); free(Wl); free(bl);
    return rc;
}

extern "C" int ff_mlp_samples_per_workgroup(const ff_mlp_plan_t* plan, int mode)
{
    LaunchDesc d;
    if (!describe(plan, &d)) return FF_ERR_BADARG;
    if (d.family == kSplit) {
        const int kt = d.split->tangents;
        if (mode == FF_MODE_STATE && kt == 0) return 128;
        if (mode == FF_MODE_HUTCH && kt == 1) return 64;
        if (mode == FF_MODE_EXACT && kt == 2) return 8 * (16 / (1 + (plan->dim < 15 ? plan->dim : 15)));
        return FF_ERR_BADARG;
    }
    if (d.state_only && mode != FF_MODE_STATE) return FF_ERR_BADARG;
    int nt, unit;
    int rc = tangents_of_mode(mode, plan->dim, plan->tile, &nt, &unit);
    if (rc) return rc;
    if (d.family == kPull || d.family == kPullSel) return plan->tile / (1 + nt);      // a tile per workgroup
    return (d.one_wave ? 4 : 1) * (plan->tile / (1 + nt));      // (the wide catch-all: a tile per workgroup)
}

// The kernels' argument block from the caller's: the one place that knows the field list.  `lp`: the divergence-side
// pointers go along (LaunchDesc::state_only families leave them out).  etab_stride and wpack_floats are the caller's.
static ff::KernelArgs fill_args(const ff_mlp_plan_t* plan, const ff_ode_args* a, bool lp, int n_tangent, int unit_tangents,
                                int tangent_first)
{
    ff::KernelArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.x_in = a->x_in; ka.x_out = a->x_out; ka.cond = a->cond; ka.noise = a->noise; ka.wpack = a->wpack; ka.etab = a->etab;
    ka.in_shift = a->in_shift; ka.in_scale = a->in_scale; ka.out_scale = a->out_scale; ka.out_shift = a->out_shift;
    ka.status = a->status; ka.gate = a->gate; ka.batch = a->batch; ka.noise_stride = a->noise_stride;
    ka.n_evals = a->n_evals; ka.n_hidden = plan->n_hidden; ka.dim = plan->dim; ka.cond_dim = plan->cond_dim;
    ka.n_tangent = n_tangent; ka.unit_tangents = unit_tangents; ka.tangent_first = tangent_first;
    ka.k1_in = a->k1_in; ka.n_aux = a->n_aux;
    for (int j = 0; j < FF_MAX_AUX; ++j) ka.aux_out[j] = a->aux_out[j];
    if (lp) {
        ka.probe = a->probe; ka.dlogp_out = a->dlogp_out; ka.dlogp_in = a->dlogp_in; ka.kl1_in = a->kl1_in;
        for (int j = 0; j < FF_MAX_AUX; ++j) ka.aux_lp_out[j] = a->aux_lp_out[j];
    }
    ka.rng_seed = a->rng_seed; ka.rng_sample_offset = a->rng_sample_offset; ka.rng_noise_base = a->rng_noise_base;
    ka.jac_out = a->jac_out;
    ka.jac_all = a->jac_out && a->jac_all ? 1 : 0;
    ka.act_kind = plan->activation; ka.act_p0 = plan->act_param[0]; ka.act_p1 = plan->act_param[1];
    return ka;
}

// FF_PREC_BF16X3 / BF16X2 launch: state-only (Euler-Maruyama noise rows included) / Hutchinson integration of a table
static int launch_split(const ff_mlp_plan_t* plan, const ff::SplitKernelEntry& k, const ff_ode_args* a, void* hip_stream)
{
    if (!a->x_in || !a->x_out || !a->wpack || !a->etab || a->batch < 0 || a->n_evals < 0) return FF_ERR_BADARG;
    if (plan->cond_dim > 0 && !a->cond) return FF_ERR_BADARG;
    if (a->mode != FF_MODE_STATE && a->mode != FF_MODE_HUTCH && a->mode != FF_MODE_EXACT) return FF_ERR_BADARG;
    if (k.tangents != (a->mode == FF_MODE_STATE ? 0 : (a->mode == FF_MODE_HUTCH ? 1 : 2))) return FF_ERR_BADARG;
    if (a->mode == FF_MODE_HUTCH && !a->probe) return FF_ERR_BADARG;
    if (a->mode == FF_MODE_HUTCH && a->tangent_count > 1) return FF_ERR_UNSUPPORTED;      // one probe per sample in this family
    if (a->mode != FF_MODE_STATE && !a->dlogp_out) return FF_ERR_BADARG;
    int nt = k.tangents == 1 ? 1 : 0, tfirst = 0;
    if (a->mode == FF_MODE_EXACT) {                     // unit tangents of dimensions [tfirst, tfirst + nt): at most 15 per launch
        nt = plan->dim < 15 ? plan->dim : 15;
        tfirst = a->tangent_first;
        if (a->tangent_count > 0) nt = a->tangent_count;
        else if (plan->dim > nt) return FF_ERR_BADARG;      // must be split by the caller
        if (tfirst < 0 || tfirst + nt > plan->dim || nt + 1 > 16) return FF_ERR_BADARG;
    }
    // what this family does not carry: the Jacobian output; noise rows with tangent columns
    if (a->jac_out || (a->noise && k.tangents)) return FF_ERR_UNSUPPORTED;
    if (a->noise && a->noise_stride < a->batch * (int64_t)plan->dim) return FF_ERR_BADARG;
    if (a->n_aux < 0 || a->n_aux > FF_MAX_AUX) return FF_ERR_BADARG;
    // stage slots: the table's promise must fit what the kernel keeps on chip (a row naming a slot beyond it would
    // land on the parked stage input and the state: the kernel refuses such a row, FF_STATUS_BAD_SLOT)
    if (a->stage_slots < 0 || a->stage_slots > FF_MAX_SLOTS) return FF_ERR_BADARG;
    if (a->stage_slots > ff::split::slots_on_chip(k.dt)) return FF_ERR_UNSUPPORTED;
    if (a->batch == 0) return FF_OK;
    ff::KernelArgs ka = fill_args(plan, a, true, nt, a->mode == FF_MODE_EXACT ? 1 : 0, tfirst);
    ka.etab_stride = FF_ROW_HDR + plan->width;
    if ((size_t)(a->n_evals + 2) * ka.etab_stride * 4 > 0x7fffffffull) return FF_ERR_UNSUPPORTED;
    ka.wpack_floats = (int)ff::split::total_words(k.n_hidden, k.parts, k.dt, k.width);
    const long long spw = k.tangents == 0 ? 128 : (k.tangents == 1 ? 64 : 8 * (16 / (1 + nt)));
    const long long grid = (a->batch + spw - 1) / spw;
    if (grid > 0x7fffffffll) return FF_ERR_UNSUPPORTED;
    const unsigned lds = (unsigned)ff::split::lds_map(plan->width, plan->n_hidden, k.parts, k.dt).total;
    const int herr = k.launch(&ka, (unsigned)grid, lds, (hipStream_t)hip_stream);
    if (herr != 0) { t_last_hip_error = herr; return FF_ERR_HIP; }
    return FF_OK;
}

// Which kernel(s) serve a launch of `tiles` tiles (16 or 32 columns each) of an f32 plan.
//
// Small batches: when the tiles of the batch would leave at least half the chip's 1024 SIMDs without one, the
// cooperative twin (one tile per WORKGROUP, the layer's rows split over its four wavefronts) finishes an evaluation
// in about a third of the time.  Same packed weights, bitwise the same results.  FF_COOP=0 / 1 pins the choice.
// One rule for whole launches and for tails (below), fitted to measurements at widths 128 / 256 / 512 (profiles/r03/:
// tail_split.txt, tail_margin.txt, coop_threshold.txt; in units of a full round of the one-wavefront kernel):
//   one-wavefront kernel, n tiles:  ceil(n / 1024) / wps      (n tiles run with that many wavefronts per SIMD; a wavefront
//                                                              does not finish sooner for having fewer neighbours)
//   twin, n tiles:                  max(least, c0 + n / (0.95 chip)),  chip = 1024 wps tiles in flight,
//                                   c0 = 0.10 (0.20 at one wavefront per SIMD), least = 0.22 / 0.30 / 0.35 for wps = 3 / 2 / 1
// The twin serves whatever it is faster at.
// Two-network kernels (profiles/pair_twin.txt; the same rule in the same units -- an evaluation is two networks on the
// one-wavefront kernel and on the twin alike -- with a line of their own where the measurement asked for one, which
// describe() puts into their descriptions): at two wavefronts per SIMD (width 256) the constants
// above pick the faster kernel at every measured tile count and stay.  At three (width 128) the twin's line is steeper and
// starts lower -- c0 = 0.03, 0.85 of a chip's worth per round: with 0.10 / 0.95 the rule took the one-wavefront kernel at
// 768 tiles (5 % slower there) and the twin at 2560 (7 % slower).
// Row-select kernels (profiles/pair_select.txt; a row is ONE network on the one-wavefront kernel and on the twin alike, so
// the units carry over): they cross where the pair kernels of their width do.  Width 256 keeps the constants above (the
// faster kernel at all ten measured sizes); width 128 with 0.10 / 0.95 took the one-wavefront kernel at 768 tiles, 6 %
// slower there than the twin, and takes the pair instance's 0.03 / 0.85.
// The tail of a launch.  The chip runs 1024 * wps tiles at once; the tiles left over after the full rounds run as a last
// round with w = ceil(leftover / 1024) wavefronts per SIMD, which takes w / wps of a full round's time (measured: the
// dispatcher fills SIMDs evenly, a wavefront does not finish sooner for having fewer neighbours than wps allows).
// The cooperative twin -- a tile per workgroup, bitwise the same results -- gets through about 0.8-0.9 of a chip's worth
// of tiles in a round's time and never needs less than ~0.3 of it.  Whenever that is the shorter of the two, the
// leftover rows go to the twin as a second launch (profiles/r03/tail_split.txt: up to +34 % just above a whole number of
// rounds, +5 % at eight rounds).  FF_TAIL_SPLIT=0 switches it off (A/B runs, tests).
struct LaunchChoice {
    bool coop;                 // the main launch is the cooperative twin (or the wide catch-all)
    long long main_tiles;      // tiles of the main launch
    long long tail_tiles;      // tiles of a second launch on the twin (0 = none)
};

static LaunchChoice choose_launch(const LaunchDesc& d, long long tiles, bool jac_out)
{
    const long long chip = 1024ll * d.wps;
    auto twin_wins = [&](long long n) {
        const double one_wave = (double)((n + 1023) / 1024) / (double)d.wps;
        const double line = d.c0 + n / (d.per_round * (double)chip);
        return (line > d.least ? line : d.least) < one_wave;
    };
    bool coop = d.coop != nullptr && tiles <= chip && twin_wins(tiles);
    if (const char* pin = getenv("FF_COOP")) coop = d.coop != nullptr && atoi(pin) != 0;
    if (d.one_wave == nullptr) coop = true;                // wide catch-all: cooperative at every batch size, one exchange buffer
    long long tail_tiles = 0;
    if (!coop && d.coop != nullptr && !jac_out) {
        const long long rem = tiles % chip;
        const char* pin = getenv("FF_TAIL_SPLIT");
        if (tiles > chip && rem > 0 && !(pin && atoi(pin) == 0) && twin_wins(rem)) tail_tiles = rem;
    }
    return LaunchChoice{coop, tiles - tail_tiles, tail_tiles};
}

// What ff_mlp_ode_launch would enqueue for `batch` samples in `mode`: FF_LAUNCH_* (see the header).
extern "C" int ff_mlp_launch_kind(const ff_mlp_plan_t* plan, int64_t batch, int32_t mode, int32_t tangent_count, int32_t jac_out)
{
    LaunchDesc d;
    if (!describe(plan, &d)) return FF_ERR_BADARG;
    if (d.family == kSplit) return FF_LAUNCH_ONE_WAVE;
    if (batch < 0 || (d.state_only && (mode != FF_MODE_STATE || jac_out))) return FF_ERR_BADARG;
    int nt, unit;
    const int rc = tangents_of_mode(mode, plan->dim, plan->tile, &nt, &unit);
    if (rc) return rc;
    if ((mode == FF_MODE_EXACT || mode == FF_MODE_HUTCH) && tangent_count > 0) nt = tangent_count;   // (Hutchinson: K probes)
    if (nt + 1 > plan->tile) return FF_ERR_BADARG;
    const long long spt = plan->tile / (1 + nt);
    const LaunchChoice ch = choose_launch(d, (batch + spt - 1) / spt, jac_out != 0);
    return ch.coop ? FF_LAUNCH_TWIN : (ch.tail_tiles ? FF_LAUNCH_ONE_WAVE_AND_TWIN : FF_LAUNCH_ONE_WAVE);
}

// Geometry and enqueue of every fp32 family: `ka` filled for the whole batch, `spt` samples per tile.  One-wavefront
// kernel, cooperative twin, or full rounds on the first and the leftover rows on the twin (choose_launch).
static int enqueue(const LaunchDesc& d, const ff_mlp_plan_t* plan, ff::KernelArgs ka, long long spt, bool jac_out, hipStream_t stream)
{
    const long long batch = ka.batch;
    if (d.family == kPull || d.family == kPullSel) {
        // a wavefront per workgroup and per tile; LDS = stage slots + the slope stash of the tile's samples
        const long long tiles = (batch + spt - 1) / spt;
        const size_t lds = d.record ? rec_lds_bytes(plan, ka.tangent_first)
                         : d.logp_grad ? lgrad_lds_bytes(plan, ka.tangent_first)
                                    : (d.products || d.discrete ? vjp_lds_bytes : pull_lds_bytes)(plan, ka.n_tangent, ka.tangent_first);
        if (lds > kPullLdsLimit || tiles > 0x7fffffffll) return FF_ERR_UNSUPPORTED;
        const int herr = d.one_wave(&ka, (unsigned)tiles, (unsigned)lds, stream);
        if (herr != 0) { t_last_hip_error = herr; return FF_ERR_HIP; }
        return FF_OK;
    }
    const LaunchChoice ch = choose_launch(d, (batch + spt - 1) / spt, jac_out);
    const bool coop = ch.coop;
    const long long main_tiles = ch.main_tiles, tail_tiles = ch.tail_tiles;
    const unsigned slots = ff::kSlots * (plan->dregs / 4) * 64 * 16;
    const unsigned kh = (plan->width / 32) * ff::tile_rb(plan->tile);                 // operand registers of a hidden layer
    const unsigned lds_coop = slots + (unsigned)d.exchange * (kh / 4) * 64 * 16, lds_wave = 4u * slots;
    if ((coop || tail_tiles ? lds_coop : 0u) > 160u * 1024u || (!coop ? lds_wave : 0u) > 160u * 1024u) return FF_ERR_UNSUPPORTED;
    const long long grid = coop ? main_tiles : (main_tiles + 3) / 4;
    if (grid > 0x7fffffffll) return FF_ERR_UNSUPPORTED;
    if (tail_tiles) ka.batch = main_tiles * spt;                                       // (full tiles only: < batch)
    int herr = (coop ? d.coop : d.one_wave)(&ka, (unsigned)grid, coop ? lds_coop : lds_wave, stream);
    if (herr == 0 && tail_tiles) {
        // the same launch over rows [row0, batch): every per-row array moves on by row0 rows, the counter-based noise by
        // row0 samples (an array the family does not pass is NULL here and stays NULL)
        const long long row0 = main_tiles * spt, D = plan->dim, C = plan->cond_dim;
        ff::KernelArgs t = ka;
        t.batch = batch - row0;
        t.x_in += row0 * D; t.x_out += row0 * D;
        if (t.cond) t.cond += row0 * C;
        if (t.probe) t.probe += row0 * D * (t.unit_tangents ? 1 : t.n_tangent);       // Hutchinson probes: [batch, n_tangent, dim]
        if (t.dlogp_probe_out) t.dlogp_probe_out += row0 * t.n_tangent;                // per-probe divergences: [batch, n_tangent]
        if (d.family == kPush || d.family == kPushSel) {
            // (push plans have no twin today, so they never get here; a cooperative push unit would.  Their two pointers share
            // the places of dlogp_out and noise: ff_kernel_args.h)
            if (t.cond_tangent) t.cond_tangent += row0 * t.n_tangent * C;              // [batch, n_tangent, cond_dim]
            t.tangent_out += row0 * t.n_tangent * D;                                   // [batch, n_tangent, dim]
        } else {
            if (t.dlogp_out) t.dlogp_out += row0;
            if (t.noise) t.noise += row0 * D;
        }
        if (t.dlogp_in) t.dlogp_in += row0;
        if (t.k1_in) t.k1_in += row0 * D;
        if (t.kl1_in) t.kl1_in += row0;
        for (int j = 0; j < FF_MAX_AUX; ++j) {
            if (t.aux_out[j]) t.aux_out[j] += row0 * D;
            if (t.aux_lp_out[j]) t.aux_lp_out[j] += row0;
        }
        t.rng_sample_offset += row0;
        herr = d.coop(&t, (unsigned)tail_tiles, lds_coop, stream);
    }
    if (herr != 0) { t_last_hip_error = herr; return FF_ERR_HIP; }
    return FF_OK;
}

// What ff_mlp_ode_launch_push adds to a launch (NULL: not a push launch).
struct PushIo {
    const float* cond_tangent;
    float* tangent_out;
    bool select;               // ff_mlp_ode_launch_push_select: the plan must be a push-select plan, and only there may it be one
};

// What ff_mlp_ode_launch_pull adds to a launch (NULL: not a pull launch).
struct PullIo {
    const float* cotangent_in;
    float* cot_x_out;
    float* cot_cond_out;
    bool select;               // ff_mlp_ode_launch_pull_select: the plan must be a pull-select plan, and only there may it be one
};

// What ff_mlp_ode_launch_vjp adds to a launch (NULL: not a products launch).
struct VjpIo {
    const float* seed_in;
    int64_t seed_row_stride;
    float* prod_out;
};

// What ff_mlp_ode_launch_record adds to a launch (NULL: not a record launch).
struct RecIo {
    float* record_out;
};

// What ff_mlp_ode_launch_pull_discrete adds to a launch (NULL: not a discrete-adjoint launch).
struct DadjIo {
    const float* record_in;
    const float* cotangent_in;
    float* cot_x_out;
    float* cot_cond_out;
};

// What ff_mlp_ode_launch_logp_grad adds to a launch (NULL: not a log-density gradient launch).
struct LgradIo {
    const float* record_in;
    const float* probe_in;
    const float* dlogp_cotangent;
    const float* cotangent_in;
    float* grad_x_out;
    float* grad_cond_out;
};

// ff_mlp_ode_launch (probe_out == NULL), ff_mlp_ode_launch_probes, ff_mlp_ode_launch_push(_select), ff_mlp_ode_launch_pull(_select),
// ff_mlp_ode_launch_vjp, ff_mlp_ode_launch_record, ff_mlp_ode_launch_pull_discrete and ff_mlp_ode_launch_logp_grad: one argument
// check, one launch path
static int launch_ode(const ff_mlp_plan_t* plan, const ff_ode_args* a, float* probe_out, void* hip_stream, const PushIo* push = nullptr,
                      const PullIo* pull = nullptr, const VjpIo* vjp = nullptr, const RecIo* rec = nullptr, const DadjIo* dadj = nullptr,
                      const LgradIo* lgrad = nullptr)
{
    LaunchDesc d;
    if (!a || !describe(plan, &d)) return FF_ERR_BADARG;
    if ((pull || vjp || rec || dadj || lgrad) && d.family == kSplit) return FF_ERR_UNSUPPORTED;
    // pull plans launch through their own entries, and only they
    if ((d.family == kPull) != ((pull != nullptr && !pull->select) || vjp != nullptr || rec != nullptr || dadj != nullptr || lgrad != nullptr)) return FF_ERR_BADARG;
    // pull-select plans through theirs, and only they
    if ((d.family == kPullSel) != (pull != nullptr && pull->select)) return FF_ERR_BADARG;
    if (rec) {
        // a whole fixed-grid solve of the state that writes every stage state down: a state-only launch's arguments, the pull
        // launch's refusals.  No cotangent columns: no stash, and the tile's columns are all samples
        const int index = plan->kernel_id - FF_PULL_KERNEL_BASE;
        if (index < 0 || index >= n_rec_kernels() || !ff::g_rec_kernels[index].launch) return FF_ERR_BADARG;
        if (!rec->record_out || a->mode != FF_MODE_STATE) return FF_ERR_BADARG;
        if (a->probe || a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        d.record = true; d.tangents = 0; d.one_wave = ff::g_rec_kernels[index].launch; d.name = ff::g_rec_kernels[index].name;
    }
    if (dadj) {
        // the transposed row program over a record: K cotangents as given, the FORWARD launch's table and maps
        const int index = plan->kernel_id - FF_PULL_KERNEL_BASE;
        if (index < 0 || index >= n_dadj_kernels() || !ff::g_dadj_kernels[index].launch) return FF_ERR_BADARG;
        if (!dadj->record_in || !dadj->cotangent_in || !dadj->cot_x_out || a->mode != FF_MODE_HUTCH) return FF_ERR_BADARG;
        if (a->tangent_count < 1 || a->tangent_count + 1 > plan->tile) return FF_ERR_BADARG;
        if (a->probe || a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        if (dadj->cot_cond_out && plan->cond_dim == 0) return FF_ERR_BADARG;
        const int ns = a->stage_slots > 0 && a->stage_slots <= FF_MAX_SLOTS ? a->stage_slots : FF_MAX_SLOTS;
        if (vjp_lds_bytes(plan, a->tangent_count, ns) > kPullLdsLimit) return FF_ERR_UNSUPPORTED;      // the stash does not fit
        d.discrete = true; d.one_wave = ff::g_dadj_kernels[index].launch; d.name = ff::g_dadj_kernels[index].name;
    }
    if (lgrad) {
        // the transposed row program with the divergence integral in it: one probe and one final cotangent per row, the FORWARD
        // launch's table and maps
        const int index = plan->kernel_id - FF_PULL_KERNEL_BASE;
        if (index < 0 || index >= n_lgrad_kernels() || !ff::g_lgrad_kernels[index].launch) return FF_ERR_BADARG;
        if (!lgrad->record_in || !lgrad->probe_in || !lgrad->cotangent_in || !lgrad->grad_x_out || a->mode != FF_MODE_HUTCH) return FF_ERR_BADARG;
        if (a->tangent_count < 0 || a->tangent_count > 1) return FF_ERR_BADARG;
        if (a->probe || a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        if (lgrad->grad_cond_out && plan->cond_dim == 0) return FF_ERR_BADARG;
        const int ns = a->stage_slots > 0 && a->stage_slots <= FF_MAX_SLOTS ? a->stage_slots : FF_MAX_SLOTS;
        if (lgrad_lds_bytes(plan, ns) > kPullLdsLimit) return FF_ERR_UNSUPPORTED;      // the stash does not fit
        d.logp_grad = true; d.one_wave = ff::g_lgrad_kernels[index].launch; d.name = ff::g_lgrad_kernels[index].name;
    }
    if (vjp) {
        // whole fixed-grid solves of the state with K products per evaluation row: the pull launch's refusals, its own buffers
        const int index = plan->kernel_id - FF_PULL_KERNEL_BASE;
        if (index < 0 || index >= n_vjp_kernels() || !ff::g_vjp_kernels[index].launch) return FF_ERR_BADARG;
        if (!vjp->seed_in || !vjp->prod_out || a->mode != FF_MODE_HUTCH) return FF_ERR_BADARG;
        if (a->tangent_count < 1 || a->tangent_count + 1 > plan->tile) return FF_ERR_BADARG;
        if (a->probe || a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        if (vjp->seed_row_stride != 0 && vjp->seed_row_stride != a->batch * (int64_t)a->tangent_count * plan->dim) return FF_ERR_BADARG;
        const int ns = a->stage_slots > 0 && a->stage_slots <= FF_MAX_SLOTS ? a->stage_slots : FF_MAX_SLOTS;
        if (vjp_lds_bytes(plan, a->tangent_count, ns) > kPullLdsLimit) return FF_ERR_UNSUPPORTED;      // the stash does not fit
        d.products = true; d.one_wave = ff::g_vjp_kernels[index].launch; d.name = ff::g_vjp_kernels[index].name;
    }
    if (pull) {
        // whole fixed-grid adjoint solves: K cotangents as given, nothing of the divergence side, no attempt launches, no noise
        if (!pull->cotangent_in || !pull->cot_x_out || a->mode != FF_MODE_HUTCH) return FF_ERR_BADARG;
        if (a->tangent_count < 1 || a->tangent_count + 1 > plan->tile) return FF_ERR_BADARG;
        if (a->probe || a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        if (pull->cot_cond_out && plan->cond_dim == 0) return FF_ERR_BADARG;
        const int ns = a->stage_slots > 0 && a->stage_slots <= FF_MAX_SLOTS ? a->stage_slots : FF_MAX_SLOTS;
        if (pull_lds_bytes(plan, a->tangent_count, ns) > kPullLdsLimit) return FF_ERR_UNSUPPORTED;      // the stash does not fit
    }
    if (push && d.family == kSplit) return FF_ERR_UNSUPPORTED;
    if ((d.family == kPush) != (push != nullptr && !push->select)) return FF_ERR_BADARG;      // push plans launch through their own entry, and only they
    if ((d.family == kPushSel) != (push != nullptr && push->select)) return FF_ERR_BADARG;    // push-select plans through theirs, and only they
    if (push) {
        // whole fixed-grid solves of the state and its tangents: nothing of the divergence side, no attempt launches, no noise
        if (!push->tangent_out || a->mode == FF_MODE_STATE || a->tangent_count < 0) return FF_ERR_BADARG;
        if (a->dlogp_out || a->k1_in || a->kl1_in || a->dlogp_in || a->jac_out || a->n_aux > 0 || a->noise) return FF_ERR_BADARG;
        if (push->cond_tangent && (plan->cond_dim == 0 || a->mode == FF_MODE_EXACT)) return FF_ERR_BADARG;
    }
    if (probe_out) {
        // per-probe divergences: Hutchinson launches of the fp32 single-network family that are whole solves (an attempt
        // launch carries a sample's stage-0 divergence on ONE lane: kl1_in / dlogp_in / aux_lp_out have no per-probe form)
        if (a->mode != FF_MODE_HUTCH) return FF_ERR_BADARG;
        if (d.family == kSplit) return FF_ERR_UNSUPPORTED;
        if (a->k1_in || a->kl1_in || a->dlogp_in || a->n_aux > 0 || a->jac_out) return FF_ERR_BADARG;
    }
    if (d.family == kSplit) return launch_split(plan, *d.split, a, hip_stream);
    // (a discrete-adjoint launch reads the record instead of a state and writes none)
    if (((!a->x_in || !a->x_out) && !dadj && !lgrad) || !a->wpack || !a->etab || a->batch < 0 || a->n_evals < 0) return FF_ERR_BADARG;
    if (plan->cond_dim > 0 && !a->cond) return FF_ERR_BADARG;
    int nt, unit;
    int rc = tangents_of_mode(a->mode, plan->dim, plan->tile, &nt, &unit);
    if (rc) return rc;
    int tfirst = 0;
    if (a->mode == FF_MODE_EXACT) {
        // (a push launch: the unit tangents run over the state's dimensions, then the conditional inputs)
        const int span = push ? plan->dim + plan->cond_dim : plan->dim;
        if (push) nt = span < plan->tile - 1 ? span : plan->tile - 1;
        tfirst = a->tangent_first;
        if (a->tangent_count > 0) nt = a->tangent_count;
        else if (span > nt) return FF_ERR_BADARG;           // must be split by the caller
        if (tfirst < 0 || tfirst + nt > span || nt + 1 > plan->tile) return FF_ERR_BADARG;
    }
    if (a->mode == FF_MODE_HUTCH && a->tangent_count > 1) {      // K probes (tangents, cotangents) per sample: [batch, K, dim]
        nt = a->tangent_count;
        if (nt + 1 > plan->tile) return FF_ERR_BADARG;
    }
    // (a state-only family has no tangent kernels: every mode but FF_MODE_STATE ends here, divergence-free by construction)
    if ((a->mode != FF_MODE_STATE) != (d.tangents != 0)) return FF_ERR_BADARG;
    if (a->mode == FF_MODE_HUTCH && !a->probe && !push && !pull && !vjp && !dadj && !lgrad) return FF_ERR_BADARG;      // (push: no state tangents = zero)
    if (a->mode != FF_MODE_STATE && !a->dlogp_out && !push && !pull && !vjp && !dadj && !lgrad) return FF_ERR_BADARG;
    if (a->stage_slots < 0 || a->stage_slots > FF_MAX_SLOTS) return FF_ERR_BADARG;
    if (a->batch == 0 && d.empty_batch_first) return FF_OK;
    if (a->n_aux < 0 || a->n_aux > d.max_aux || (a->k1_in && !d.takes_k1)) return FF_ERR_BADARG;
    if (a->jac_out && a->mode != FF_MODE_EXACT) return FF_ERR_BADARG;
    if (d.checks_noise_stride && a->noise && a->noise_stride < a->batch * (int64_t)plan->dim) return FF_ERR_BADARG;
    if (a->batch == 0) return FF_OK;

    ff::KernelArgs ka = fill_args(plan, a, !d.state_only, nt, unit, tfirst);
    ka.etab_stride = FF_ROW_HDR + d.row_nets * plan->width;
    const size_t wpack_floats = (size_t)d.nets * plan_layout(plan).total_floats +
                                (pull || vjp || rec || dadj || lgrad ? (size_t)d.nets * pull_layout(plan).total_floats : 0);
    if (wpack_floats * 4 > 0x7fffffffull) return FF_ERR_UNSUPPORTED;
    if ((size_t)(a->n_evals + 2) * ka.etab_stride * 4 > 0x7fffffffull) return FF_ERR_UNSUPPORTED;
    ka.wpack_floats = (int)wpack_floats;
    ka.dlogp_probe_out = probe_out;
    if (push) { ka.cond_tangent = push->cond_tangent; ka.tangent_out = push->tangent_out; }
    // (a pull launch takes none of the three, so they carry its own pointers: ff_mlp_pull.hpp)
    if (pull) {
        ka.probe = pull->cotangent_in; ka.dlogp_out = pull->cot_x_out; ka.jac_out = pull->cot_cond_out;
        ka.tangent_first = a->stage_slots > 0 ? a->stage_slots : FF_MAX_SLOTS;      // the stage slots the kernel keeps in LDS
    }
    // (nor does a products launch, which takes no noise either: ff_mlp_vjp.hpp)
    if (vjp) {
        ka.probe = vjp->seed_in; ka.dlogp_out = vjp->prod_out; ka.noise_stride = vjp->seed_row_stride;
        ka.tangent_first = a->stage_slots > 0 ? a->stage_slots : FF_MAX_SLOTS;
    }
    // (the record and discrete-adjoint launches: ff_mlp_dadj.hpp)
    if (rec) {
        ka.dlogp_out = rec->record_out;
        ka.tangent_first = a->stage_slots > 0 ? a->stage_slots : FF_MAX_SLOTS;
    }
    if (dadj) {
        ka.probe = dadj->cotangent_in; ka.dlogp_out = dadj->cot_x_out; ka.jac_out = dadj->cot_cond_out; ka.k1_in = dadj->record_in;
        ka.tangent_first = a->stage_slots > 0 ? a->stage_slots : FF_MAX_SLOTS;
    }
    // (the log-density gradient launch: ff_mlp_lgrad.hpp)
    if (lgrad) {
        ka.probe = lgrad->cotangent_in; ka.dlogp_out = lgrad->grad_x_out; ka.jac_out = lgrad->grad_cond_out; ka.k1_in = lgrad->record_in;
        ka.kl1_in = lgrad->probe_in; ka.dlogp_in = lgrad->dlogp_cotangent;
        ka.tangent_first = a->stage_slots > 0 ? a->stage_slots : FF_MAX_SLOTS;
    }
    return enqueue(d, plan, ka, plan->tile / (1 + nt), a->jac_out != nullptr, (hipStream_t)hip_stream);
}

extern "C" int ff_mlp_ode_launch(const ff_mlp_plan_t* plan, const ff_ode_args* a, void* hip_stream)
{
    return launch_ode(plan, a, nullptr, hip_stream);
}

extern "C" int ff_mlp_ode_launch_probes(const ff_mlp_plan_t* plan, const ff_ode_args* a, float* dlogp_probe_out, void* hip_stream)
{
    return launch_ode(plan, a, dlogp_probe_out, hip_stream);
}

extern "C" int ff_mlp_ode_launch_push(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* cond_tangent, float* tangent_out,
                                      void* hip_stream)
{
    const PushIo io = {cond_tangent, tangent_out, false};
    return launch_ode(plan, a, nullptr, hip_stream, &io);
}

extern "C" int ff_mlp_ode_launch_push_select(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* cond_tangent, float* tangent_out,
                                             void* hip_stream)
{
    const PushIo io = {cond_tangent, tangent_out, true};
    return launch_ode(plan, a, nullptr, hip_stream, &io);
}

extern "C" int ff_mlp_ode_launch_pull(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* cotangent_in, float* cot_x_out,
                                      float* cot_cond_out, void* hip_stream)
{
    const PullIo io = {cotangent_in, cot_x_out, cot_cond_out, false};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, &io);
}

extern "C" int ff_mlp_ode_launch_pull_select(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* cotangent_in, float* cot_x_out,
                                             float* cot_cond_out, void* hip_stream)
{
    const PullIo io = {cotangent_in, cot_x_out, cot_cond_out, true};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, &io);
}

extern "C" int ff_mlp_ode_launch_vjp(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* seed_in, int64_t seed_row_stride,
                                     float* prod_out, void* hip_stream)
{
    const VjpIo io = {seed_in, seed_row_stride, prod_out};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, nullptr, &io);
}

extern "C" int ff_mlp_ode_launch_record(const ff_mlp_plan_t* plan, const ff_ode_args* a, float* record_out, void* hip_stream)
{
    const RecIo io = {record_out};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, nullptr, nullptr, &io);
}

extern "C" int ff_mlp_ode_launch_pull_discrete(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* record_in,
                                               const float* cotangent_in, float* cot_x_out, float* cot_cond_out, void* hip_stream)
{
    const DadjIo io = {record_in, cotangent_in, cot_x_out, cot_cond_out};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, nullptr, nullptr, nullptr, &io);
}

extern "C" int ff_mlp_ode_launch_logp_grad(const ff_mlp_plan_t* plan, const ff_ode_args* a, const float* record_in, const float* probe_in,
                                           const float* dlogp_cotangent, const float* cotangent_in, float* grad_x_out,
                                           float* grad_cond_out, void* hip_stream)
{
    const LgradIo io = {record_in, probe_in, dlogp_cotangent, cotangent_in, grad_x_out, grad_cond_out};
    return launch_ode(plan, a, nullptr, hip_stream, nullptr, nullptr, nullptr, nullptr, nullptr, &io);
}

// ---- the device-side adaptive controller's arithmetic, on the host (tests without a GPU; ff_adapt_logic.h) ------------
extern "C" int ff_adapt_host_row(const ff_adapt_config* c, float t_real, float* a_out, float* b_out, float* c1_out)
{
    if (!c || !a_out || !b_out || !c1_out || !c->w0t || !c->b0 || c->h_real < 1 || c->n_tcols < 1 || c->n_tcols > 64) return FF_ERR_BADARG;
    if (c->sched != FF_SCHED_FLOW && (!c->emb_w || c->n_tcols != 2 * c->n_emb)) return FF_ERR_BADARG;
    float a, b, feat[64];
    ff::adapt::schedule_ab(*c, t_real, &a, &b);
    *a_out = c->sign * a;
    *b_out = c->sign * b;
    for (int k = 0; k < c->n_tcols; ++k) feat[k] = ff::adapt::time_feature(*c, t_real, k);
    for (int h = 0; h < c->h_real; ++h) c1_out[h] = ff::adapt::c1_from_features(*c, feat, h);
    return FF_OK;
}

extern "C" int ff_adapt_host_transition(const ff_adapt_config* c, ff_adapt_state* s, int32_t phase, const float* norms)
{
    if (!c || !s || (phase != ff::adapt::kPhaseFirst && !norms)) return FF_ERR_BADARG;
    switch (phase) {
    case ff::adapt::kPhaseInit1:
        s->d0 = (double)norms[0];
        return ff::adapt::transition(*c, *s, phase, norms + 1, 1) == ff::adapt::kRowsDerivAtH0 ? 1 : 0;
    case ff::adapt::kPhaseInit2:
        return ff::adapt::transition(*c, *s, phase, norms, 1) == ff::adapt::kRowsAttempt ? 1 : 0;
    case ff::adapt::kPhaseStep:
        return ff::adapt::transition(*c, *s, phase, norms, 2) == ff::adapt::kRowsAttempt ? 1 : 0;
    case ff::adapt::kPhaseFirst:
        return ff::adapt::transition(*c, *s, phase, norms, 0) == ff::adapt::kRowsAttempt ? 1 : 0;
    default:
        return FF_ERR_BADARG;
    }
}
