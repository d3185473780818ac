// launch_records.cpp -- what the C ABI enqueues, recorded on the CPU (tests/test_launch_records.py).
//
// ff_api.cpp calls no HIP function itself, only the LaunchFn pointers of the generated kernel table.  The test links
// it against a copy of that table whose launchers call ff_test_record() below instead of the GPU, and this driver
// sweeps plans x batches x arguments x FF_COOP / FF_TAIL_SPLIT pins through the public C ABI alone.  Every launch is
// printed as the launcher's name, its grid and LDS bytes and every KernelArgs field that is not zero; a pointer is
// printed as its byte offset from the pointer the driver passed for that argument, so the text holds no address.
// The device pointers are made-up addresses: nothing on this path reads through them.
//
//   launch_records           per section (plan x pin) its line count and an FNV-1a digest; the text of the planner and packer sections
//                            and of the headline plan's batch sweep
//   launch_records --full    the text of every section (megabytes: for comparing two trees, not committed)
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "flowfusion_amd.h"
#include "ff_kernel_args.h"

static std::string g_text;                  // the section being written
static const ff_ode_args* g_cur = nullptr;  // arguments of the call in flight (the recorder's pointer bases)
static bool g_full = false;

static void put(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void put(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_text += buf;
}

static void put_ptr(const char* name, const void* p, const void* base)
{
    if (!p) return;
    if (!base) { put(" %s=WILD", name); return; }
    put(" %s+%lld", name, (long long)((intptr_t)p - (intptr_t)base));
}

static void put_int(const char* name, long long v) { if (v) put(" %s=%lld", name, v); }

extern "C" int ff_test_record(const char* name, const ff::KernelArgs* k, unsigned grid, unsigned lds)
{
    const ff_ode_args* a = g_cur;
    put(" > %s g=%u l=%u", name + 7 /* "launch_" */, grid, lds);
    put_ptr("x_in", k->x_in, a->x_in); put_ptr("x_out", k->x_out, a->x_out); put_ptr("cond", k->cond, a->cond);
    put_ptr("probe", k->probe, a->probe); put_ptr("dlogp_out", k->dlogp_out, a->dlogp_out);
    put_ptr("noise", k->noise, a->noise); put_ptr("wpack", k->wpack, a->wpack); put_ptr("etab", k->etab, a->etab);
    put_ptr("in_shift", k->in_shift, a->in_shift); put_ptr("in_scale", k->in_scale, a->in_scale);
    put_ptr("out_scale", k->out_scale, a->out_scale); put_ptr("out_shift", k->out_shift, a->out_shift);
    put_ptr("status", k->status, a->status);
    put_int("batch", k->batch); put_int("noise_stride", k->noise_stride); put_int("n_evals", k->n_evals);
    put_int("n_hidden", k->n_hidden); put_int("dim", k->dim); put_int("cond_dim", k->cond_dim);
    put_int("n_tangent", k->n_tangent); put_int("unit_tangents", k->unit_tangents);
    put_int("tangent_first", k->tangent_first); put_int("etab_stride", k->etab_stride);
    put_int("wpack_floats", k->wpack_floats);
    put_ptr("k1_in", k->k1_in, a->k1_in); put_ptr("kl1_in", k->kl1_in, a->kl1_in); put_ptr("dlogp_in", k->dlogp_in, a->dlogp_in);
    for (int j = 0; j < ff::kAux; ++j) {
        char n[24];
        snprintf(n, sizeof(n), "aux_out%d", j); put_ptr(n, k->aux_out[j], a->aux_out[j]);
        snprintf(n, sizeof(n), "aux_lp_out%d", j); put_ptr(n, k->aux_lp_out[j], a->aux_lp_out[j]);
    }
    put_int("n_aux", k->n_aux); put_int("rng_seed", (long long)k->rng_seed); put_int("rng_sample_offset", k->rng_sample_offset);
    put_int("rng_noise_base", k->rng_noise_base);
    put_ptr("jac_out", k->jac_out, a->jac_out); put_int("jac_all", k->jac_all); put_int("act_kind", k->act_kind);
    if (k->act_p0 != 0.f || k->act_p1 != 0.f) put(" act_p=%g,%g", k->act_p0, k->act_p1);
    put_ptr("gate", k->gate, a->gate);
    return 0;
}

static uint64_t fnv(const void* data, size_t n, uint64_t h = 1469598103934665603ull)
{
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static void end_section(const char* title, bool show)
{
    size_t lines = 0;
    for (char c : g_text) lines += c == '\n';
    printf("== %s lines=%zu fnv=%016llx\n", title, lines, (unsigned long long)fnv(g_text.data(), g_text.size()));
    if (show || g_full) fputs(g_text.c_str(), stdout);
    g_text.clear();
}

// ---- arguments ----------------------------------------------------------------------------------------------------
template <class T> static T* dev(int slot) { return (T*)(uintptr_t)(0x100000000000ull + (uint64_t)slot * 0x010000000000ull); }

static ff_ode_args base_args(const ff_mlp_plan_t& p, int mode, long long batch)
{
    ff_ode_args a;
    memset(&a, 0, sizeof(a));
    a.x_in = dev<float>(1); a.x_out = dev<float>(2); a.wpack = dev<float>(3); a.etab = dev<float>(4);
    if (p.cond_dim > 0) a.cond = dev<float>(5);
    if (mode == FF_MODE_HUTCH) a.probe = dev<float>(6);
    if (mode != FF_MODE_STATE) a.dlogp_out = dev<float>(7);
    a.batch = batch; a.n_evals = 8; a.mode = mode;
    const int most = p.precision == FF_PREC_F32 ? p.tile - 1 : 15;     // unit tangents one launch carries
    if (mode == FF_MODE_EXACT && p.dim > most) a.tangent_count = most;
    return a;
}

static void launch(const char* what, const ff_mlp_plan_t& p, const ff_ode_args& a, bool null_plan = false, bool null_args = false)
{
    g_cur = &a;
    put("%s b=%lld kind=%d", what, (long long)a.batch,
        ff_mlp_launch_kind(&p, a.batch, a.mode, a.tangent_count, a.jac_out != nullptr));
    const int rc = ff_mlp_ode_launch(null_plan ? nullptr : &p, null_args ? nullptr : &a, dev<void>(30));
    put(" rc=%d\n", rc);
}

struct Case { const char* title; ff_mlp_plan_t plan; int mode; bool show; };

static long long samples_per_tile(const ff_mlp_plan_t& p, int mode)
{
    if (p.precision != FF_PREC_F32) { const int s = ff_mlp_samples_per_workgroup(&p, mode); return s > 0 ? s : 1; }
    const int nt = mode == FF_MODE_STATE ? 0 : (mode == FF_MODE_HUTCH ? 1 : (p.dim < p.tile - 1 ? p.dim : p.tile - 1));
    return p.tile / (1 + nt);
}

static std::vector<long long> batches(long long spt)
{
    std::vector<long long> tiles = {0, 1, 255, 256, 257, 700, 768, 778, 896};
    for (long long chip : {1024ll, 2048ll, 3072ll})
        for (long long t : {chip - 1, chip, chip + 1, chip + 300, 2 * chip + 1, 8 * chip + 700}) tiles.push_back(t);
    std::vector<long long> out;
    for (long long t : tiles)
        for (long long r : {-1ll, 0ll, 1ll})
            if (t * spt + r >= 0) out.push_back(t * spt + r);
    out.push_back(1ll << 20);
    return out;
}

static void queries(const Case& c)
{
    const ff_mlp_plan_t& p = c.plan;
    const char* n = ff_plan_kernel_name(&p);
    put("plan dim=%d cond=%d nh=%d width=%d dregs=%d cregs=%d id=%d tile=%d act=%d prec=%d name=%s row_width=%d\n", p.dim,
        p.cond_dim, p.n_hidden, p.width, p.dregs, p.cregs, p.kernel_id, p.tile, p.activation, p.precision, n ? n : "(null)",
        ff_mlp_row_width(&p));
    put("spw %d %d %d bad %d wpack %zu pair_wpack %zu\n", ff_mlp_samples_per_workgroup(&p, 0),
        ff_mlp_samples_per_workgroup(&p, 1), ff_mlp_samples_per_workgroup(&p, 2), ff_mlp_samples_per_workgroup(&p, 7),
        ff_mlp_wpack_floats(&p), ff_mlp_pair_wpack_floats(&p));
    for (long long b : {-1ll, 0ll, 1000ll, 40000ll})
        put("kind b=%lld: %d %d %d bad %d tc3 %d jac %d\n", b, ff_mlp_launch_kind(&p, b, 0, 0, 0), ff_mlp_launch_kind(&p, b, 1, 0, 0),
            ff_mlp_launch_kind(&p, b, 2, 0, 0), ff_mlp_launch_kind(&p, b, 7, 0, 0), ff_mlp_launch_kind(&p, b, 2, 3, 0),
            ff_mlp_launch_kind(&p, b, 2, 0, 1));
}

static void argument_variants(const Case& c)
{
    const ff_mlp_plan_t& p = c.plan;
    const long long spt = samples_per_tile(p, c.mode);
    for (long long b : {spt + 1, 1324 * spt - 1, 2348 * spt + 1, 3372 * spt, 1ll << 20}) {
        ff_ode_args a = base_args(p, c.mode, b);
        launch("plain", p, a);
        if (p.cond_dim > 0) { a.cond = nullptr; launch("nocond", p, a); a = base_args(p, c.mode, b); }
        a.noise = dev<float>(8); a.noise_stride = b * p.dim + 64; launch("noise", p, a);
        a = base_args(p, c.mode, b);
        a.rng_seed = 0x1234567ull; a.rng_sample_offset = 1000000007ll; a.rng_noise_base = 5; launch("rng", p, a);
        a = base_args(p, c.mode, b);
        a.k1_in = dev<float>(9); a.kl1_in = dev<float>(10); a.dlogp_in = dev<float>(11); launch("k1", p, a);
        a = base_args(p, c.mode, b);
        for (int j = 0; j < FF_MAX_AUX; ++j) { a.aux_out[j] = dev<float>(12 + j); a.aux_lp_out[j] = dev<float>(16 + j); }
        launch("auxptr", p, a);
        a.n_aux = 4; launch("aux4", p, a);
        a.n_aux = 8; launch("aux8", p, a);
        a.n_aux = 2; a.k1_in = dev<float>(9); a.kl1_in = dev<float>(10); a.dlogp_in = dev<float>(11); a.stage_slots = 7;
        launch("step", p, a);
        a = base_args(p, c.mode, b);
        a.jac_out = dev<float>(20); launch("jac", p, a);
        a.jac_all = 1; launch("jacall", p, a);
        a = base_args(p, c.mode, b);
        a.gate = dev<int32_t>(21); a.status = dev<uint32_t>(22); launch("gate", p, a);
        a.in_shift = dev<float>(23); a.in_scale = dev<float>(24); a.out_scale = dev<float>(25); a.out_shift = dev<float>(26);
        launch("affine", p, a);
        if (c.mode == FF_MODE_EXACT) {
            a = base_args(p, c.mode, b);
            a.tangent_count = 3; a.tangent_first = 2; launch("tangents", p, a);
            a.tangent_first = p.dim - 2; launch("tangents_past", p, a);
            a.tangent_count = p.tile; a.tangent_first = 0; launch("tangents_many", p, a);
        }
        for (int m = 0; m < 3; ++m)
            if (m != c.mode) { a = base_args(p, m, b); a.probe = dev<float>(6); a.dlogp_out = dev<float>(7); launch("othermode", p, a); }
    }
}

static void invalid_calls(const Case& c)
{
    const ff_mlp_plan_t& p = c.plan;
    const long long b = 1000;
    ff_ode_args a = base_args(p, c.mode, b);
    launch("null_plan", p, a, true); launch("null_args", p, a, false, true);
    a.x_in = nullptr; launch("no_x_in", p, a); a = base_args(p, c.mode, b);
    a.x_out = nullptr; launch("no_x_out", p, a); a = base_args(p, c.mode, b);
    a.wpack = nullptr; launch("no_wpack", p, a); a = base_args(p, c.mode, b);
    a.etab = nullptr; launch("no_etab", p, a); a = base_args(p, c.mode, b);
    a.cond = nullptr; launch("no_cond", p, a); a = base_args(p, c.mode, b);
    a.probe = nullptr; launch("no_probe", p, a); a = base_args(p, c.mode, b);
    a.dlogp_out = nullptr; launch("no_dlogp_out", p, a); a = base_args(p, c.mode, b);
    a.batch = -1; launch("neg_batch", p, a); a = base_args(p, c.mode, b);
    a.n_evals = -1; launch("neg_evals", p, a); a = base_args(p, c.mode, b);
    a.mode = 3; launch("bad_mode", p, a); a.mode = -1; launch("bad_mode", p, a); a = base_args(p, c.mode, b);
    for (int n : {-1, 9, 1}) { a.n_aux = n; launch("n_aux", p, a); }
    a = base_args(p, c.mode, 0);
    for (int n : {-1, 9, 1}) { a.n_aux = n; launch("n_aux_empty", p, a); }
    a.n_aux = 0; a.jac_out = dev<float>(20); launch("jac_empty", p, a);
    a = base_args(p, c.mode, b);
    for (int s : {-1, 5, 7, 8}) { a.stage_slots = s; launch("stage_slots", p, a); }
    a = base_args(p, c.mode, b);
    a.k1_in = dev<float>(9); launch("k1_in", p, a); a = base_args(p, c.mode, b);
    a.noise = dev<float>(8); a.noise_stride = b * p.dim - 1; launch("short_noise", p, a);
    a.noise_stride = b * p.dim; launch("exact_noise", p, a); a = base_args(p, c.mode, b);
    a.n_evals = 0x7fffffff - 2; launch("huge_table", p, a); a = base_args(p, c.mode, b);
    a.batch = 0x7fffffffffffll; launch("huge_batch", p, a); a = base_args(p, c.mode, b);
    // a plan struct with one field corrupted
    struct { const char* what; int32_t ff_mlp_plan_t::*field; int delta; } edits[] = {
        {"width", &ff_mlp_plan_t::width, 32}, {"tile", &ff_mlp_plan_t::tile, 16}, {"tile", &ff_mlp_plan_t::tile, -16},
        {"dregs", &ff_mlp_plan_t::dregs, 4}, {"cregs", &ff_mlp_plan_t::cregs, 4}, {"dim", &ff_mlp_plan_t::dim, 1},
        {"dim", &ff_mlp_plan_t::dim, 200}, {"cond_dim", &ff_mlp_plan_t::cond_dim, 100}, {"n_hidden", &ff_mlp_plan_t::n_hidden, -100},
        {"activation", &ff_mlp_plan_t::activation, 1}, {"activation", &ff_mlp_plan_t::activation, 20},
        {"precision", &ff_mlp_plan_t::precision, 1}, {"precision", &ff_mlp_plan_t::precision, 2}, {"precision", &ff_mlp_plan_t::precision, 7},
    };
    auto probe_plan = [&](const char* what, const ff_mlp_plan_t& q) {
        const char* n = ff_plan_kernel_name(&q);
        put("corrupt %s: name=%s row_width=%d spw=%d wpack=%zu pair_wpack=%zu ", what, n ? n : "(null)", ff_mlp_row_width(&q),
            ff_mlp_samples_per_workgroup(&q, c.mode), ff_mlp_wpack_floats(&q), ff_mlp_pair_wpack_floats(&q));
        launch("", q, base_args(q, c.mode, b));
    };
    for (auto& e : edits) {
        ff_mlp_plan_t q = p;
        q.*(e.field) += e.delta;
        probe_plan(e.what, q);
    }
    const int n_f32 = ff_kernel_count(), n_pair = ff_pair_kernel_count();
    for (int id : {-1, n_f32 - 1, n_f32, n_f32 + 1, FF_PAIR_KERNEL_BASE - 1, FF_PAIR_KERNEL_BASE, FF_PAIR_KERNEL_BASE + n_pair - 1,
                   FF_PAIR_KERNEL_BASE + n_pair, FF_PAIR_SELECT_KERNEL_BASE - 1, FF_PAIR_SELECT_KERNEL_BASE,
                   FF_PAIR_SELECT_KERNEL_BASE + n_pair - 1, FF_PAIR_SELECT_KERNEL_BASE + n_pair, 0x30000, 0x7fffffff}) {
        ff_mlp_plan_t q = p;
        q.kernel_id = id;
        probe_plan("kernel_id", q);
    }
    for (int id = 0; id < 80; ++id) {        // just past each family's range, whatever the tables' sizes
        ff_mlp_plan_t q = p;
        q.kernel_id = id;
        const char* n = ff_plan_kernel_name(&q);
        if (n) put("id %d also names %s\n", id, n);
    }
}

static void sweep(const Case& c)
{
    char title[160];
    queries(c);
    argument_variants(c);
    invalid_calls(c);
    snprintf(title, sizeof(title), "%s arguments", c.title);
    end_section(title, false);
    const struct { const char* coop; const char* tail; } pins[] = {{nullptr, nullptr}, {"0", nullptr}, {"1", nullptr},
                                                                    {nullptr, "0"}, {"0", "0"}, {"1", "0"}};
    for (auto& pin : pins) {
        if (pin.coop) setenv("FF_COOP", pin.coop, 1); else unsetenv("FF_COOP");
        if (pin.tail) setenv("FF_TAIL_SPLIT", pin.tail, 1); else unsetenv("FF_TAIL_SPLIT");
        for (long long b : batches(samples_per_tile(c.plan, c.mode))) {
            ff_ode_args a = base_args(c.plan, c.mode, b);
            for (int j = 0; j < FF_MAX_AUX; ++j) { a.aux_out[j] = dev<float>(12 + j); a.aux_lp_out[j] = dev<float>(16 + j); }
            a.n_aux = c.plan.kernel_id >= FF_PAIR_SELECT_KERNEL_BASE ? 0 : 2;
            launch("", c.plan, a);
        }
        snprintf(title, sizeof(title), "%s batches FF_COOP=%s FF_TAIL_SPLIT=%s", c.title, pin.coop ? pin.coop : "-", pin.tail ? pin.tail : "-");
        end_section(title, c.show && !pin.coop && !pin.tail);
    }
    unsetenv("FF_COOP"); unsetenv("FF_TAIL_SPLIT");
}

// ---- packing ------------------------------------------------------------------------------------------------------
static void packing(const ff_mlp_plan_t& p, const char* title, bool pair)
{
    const int NH = p.n_hidden, D = pair ? p.dim / 2 : p.dim, in0 = D + p.cond_dim + 3, h = p.width - 5;
    std::vector<int> widths(NH, h);
    std::vector<std::vector<float>> store;
    uint32_t s = 12345u;
    auto tensor = [&](size_t n) {
        store.emplace_back(n);
        for (float& v : store.back()) { s = s * 1664525u + 1013904223u; v = (float)(int)(s >> 8) / (float)(1 << 23) - 1.0f; }
        return (const float*)store.back().data();
    };
    std::vector<const float*> W[2], B[2];
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l <= NH; ++l) {
            const int rows = l == NH ? D : h, cols = l == 0 ? in0 : h;
            W[net].push_back(tensor((size_t)rows * cols));
            B[net].push_back(tensor(rows));
        }
    const size_t n = pair ? ff_mlp_pair_wpack_floats(&p) : ff_mlp_wpack_floats(&p);
    std::vector<float> out(n + 1, 7.f);
    const int rc = pair ? ff_mlp_pair_wpack(&p, W[0].data(), B[0].data(), W[1].data(), B[1].data(), widths.data(), in0, 2, 2 + D, out.data())
                        : ff_mlp_wpack(&p, W[0].data(), B[0].data(), widths.data(), in0, 2, 2 + D, out.data());
    put("pack %s rc=%d floats=%zu fnv=%016llx guard=%g\n", title, rc, n, (unsigned long long)fnv(out.data(), n * 4), out[n]);
    // refusals of the packers
    put("pack %s bad: %d %d %d %d\n", title,
        pair ? ff_mlp_pair_wpack(&p, W[0].data(), B[0].data(), nullptr, B[1].data(), widths.data(), in0, 2, 2 + D, out.data())
             : ff_mlp_wpack(&p, nullptr, B[0].data(), widths.data(), in0, 2, 2 + D, out.data()),
        pair ? ff_mlp_pair_wpack(&p, W[0].data(), B[0].data(), W[1].data(), B[1].data(), widths.data(), in0, in0, 2 + D, out.data())
             : ff_mlp_wpack(&p, W[0].data(), B[0].data(), widths.data(), in0, in0, 2 + D, out.data()),
        ff_mlp_wpack(&p, W[0].data(), B[0].data(), widths.data(), in0, 2, 2 + D, pair ? out.data() : nullptr),
        ff_mlp_pair_wpack(&p, W[0].data(), B[0].data(), W[1].data(), B[1].data(), widths.data(), in0, 2, 2 + D, pair ? nullptr : out.data()));
}

int main(int argc, char** argv)
{
    g_full = argc > 1 && strcmp(argv[1], "--full") == 0;
    unsetenv("FF_COOP"); unsetenv("FF_TAIL_SPLIT");
    put("%s\n", ff_version());
    for (int i = -1; i <= ff_kernel_count(); ++i) { const char* n = ff_kernel_name(i); put("kernel %d %s\n", i, n ? n : "(null)"); }
    for (int i = -1; i <= ff_pair_kernel_count(); ++i) { const char* n = ff_pair_kernel_name(i); put("pair kernel %d %s\n", i, n ? n : "(null)"); }
    end_section("tables", false);

    const int w256[4] = {256, 256, 256, 256}, w128[3] = {128, 128, 128}, w64[2] = {64, 64}, w512[5] = {512, 512, 512, 512, 512};
    const int w700[2] = {700, 700}, w2000[2] = {2000, 2000}, w100[3] = {100, 120, 90};
    const float leaky[2] = {0.1f, 0.f}, softplus[2] = {1.5f, 20.f};
    std::vector<Case> cases;
    auto add = [&](const char* title, int rc, const ff_mlp_plan_t& p, int mode, bool show = false) {
        put("planner %s rc=%d\n", title, rc);
        if (rc == FF_OK) cases.push_back(Case{title, p, mode, show});
    };
    ff_mlp_plan_t p;
    auto f32 = [&](const char* t, int dim, int cond, int nh, const int* w, int mode, bool show = false) {
        memset(&p, 0xee, sizeof(p)); add(t, ff_mlp_plan(dim, cond, nh, w, mode, &p), p, mode, show);
    };
    auto act = [&](const char* t, int dim, int cond, int nh, const int* w, int mode, int kind, const float* par) {
        memset(&p, 0xee, sizeof(p)); add(t, ff_mlp_plan_act(dim, cond, nh, w, mode, kind, par, &p), p, mode);
    };
    auto prec = [&](const char* t, int dim, int cond, int nh, const int* w, int mode, int pr, bool show = false) {
        memset(&p, 0xee, sizeof(p)); add(t, ff_mlp_plan_prec(dim, cond, nh, w, mode, FF_ACT_SILU, nullptr, pr, &p), p, mode, show);
    };
    auto pair = [&](const char* t, int dim, int cond, int nh, const int* w, bool select, bool show = false) {
        memset(&p, 0xee, sizeof(p));
        add(t, select ? ff_mlp_pair_select_plan(dim, cond, nh, w, &p) : ff_mlp_pair_plan(dim, cond, nh, w, &p), p, FF_MODE_STATE, show);
    };
    f32("headline state", 16, 0, 4, w256, FF_MODE_STATE, true);
    f32("headline hutch", 16, 0, 4, w256, FF_MODE_HUTCH);
    f32("headline exact", 16, 0, 4, w256, FF_MODE_EXACT);
    f32("headline exact d5", 5, 0, 4, w256, FF_MODE_EXACT);
    f32("h128 w3 state", 8, 0, 3, w128, FF_MODE_STATE);
    f32("h128 w3 cond exact", 8, 3, 3, w128, FF_MODE_EXACT);
    f32("h128 narrow-net", 10, 2, 3, w100, FF_MODE_HUTCH);
    f32("h64 m32 state", 4, 0, 2, w64, FF_MODE_STATE);
    f32("h64 m32 cond exact", 30, 5, 2, w64, FF_MODE_EXACT);
    f32("h256 d32 c32", 32, 32, 4, w256, FF_MODE_STATE);
    f32("h256 d64 one wave per SIMD", 64, 4, 4, w256, FF_MODE_HUTCH);
    f32("h512 state", 64, 4, 5, w512, FF_MODE_STATE);
    f32("h512 exact", 64, 4, 5, w512, FF_MODE_EXACT);
    f32("wide state", 100, 40, 2, w700, FF_MODE_STATE);
    f32("wide exact", 100, 40, 2, w700, FF_MODE_EXACT);
    act("leaky_relu state", 16, 4, 4, w256, FF_MODE_STATE, FF_ACT_LEAKY_RELU, leaky);
    act("softplus hutch", 16, 4, 4, w256, FF_MODE_HUTCH, FF_ACT_SOFTPLUS, softplus);
    act("tanh h512", 64, 4, 5, w512, FF_MODE_STATE, FF_ACT_TANH, nullptr);
    act("gelu m32", 30, 5, 3, w128, FF_MODE_EXACT, FF_ACT_GELU, nullptr);
    prec("bf16x3 d16 state", 16, 0, 4, w256, FF_MODE_STATE, FF_PREC_BF16X3);
    prec("bf16x2 d16 state", 16, 4, 4, w256, FF_MODE_STATE, FF_PREC_BF16X2);
    prec("bf16x2 d16 hutch", 16, 0, 3, w128, FF_MODE_HUTCH, FF_PREC_BF16X2);
    prec("bf16x2 d16 exact", 16, 0, 4, w256, FF_MODE_EXACT, FF_PREC_BF16X2);
    prec("bf16x2 d7 exact", 7, 0, 4, w256, FF_MODE_EXACT, FF_PREC_BF16X2);
    prec("bf16x2 d32 state", 32, 0, 4, w256, FF_MODE_STATE, FF_PREC_BF16X2);
    prec("bf16x3 d32 (refused)", 32, 0, 4, w256, FF_MODE_STATE, FF_PREC_BF16X3);
    prec("bf16x2 d32 hutch (refused)", 32, 0, 4, w256, FF_MODE_HUTCH, FF_PREC_BF16X2);
    prec("precision 5 (refused)", 16, 0, 4, w256, FF_MODE_STATE, 5);
    pair("pair h256", 16, 0, 4, w256, false);
    pair("pair h256 cond", 32, 16, 4, w256, false);
    pair("pair h128", 16, 3, 3, w128, false);
    pair("pair h64", 6, 0, 2, w64, false);
    pair("select h256", 16, 0, 4, w256, true);
    pair("select h128", 16, 3, 3, w128, true);
    pair("select h64", 6, 0, 2, w64, true);
    pair("pair odd dim (refused)", 15, 0, 4, w256, false);
    pair("select odd dim (refused)", 15, 0, 4, w256, true);
    pair("pair width 2000 (refused)", 16, 0, 2, w2000, false);
    pair("pair 65 cond (refused)", 16, 65, 4, w256, false);
    pair("pair dim 34 (refused)", 34, 0, 4, w256, false);
    f32("width 2000 (refused)", 16, 0, 2, w2000, FF_MODE_STATE);
    f32("65 cond (refused)", 16, 65, 4, w256, FF_MODE_STATE);
    f32("dim 0 (refused)", 0, 0, 4, w256, FF_MODE_STATE);
    f32("mode 3 (refused)", 16, 0, 4, w256, 3);
    act("activation 9 (refused)", 16, 0, 4, w256, FF_MODE_STATE, 9, nullptr);
    put("planner null: %d %d %d\n", ff_mlp_plan(16, 0, 4, w256, 0, nullptr), ff_mlp_pair_plan(16, 0, 4, w256, nullptr),
        ff_mlp_plan(16, 0, 4, nullptr, 0, &p));
    end_section("planners", true);

    for (const Case& c : cases) sweep(c);

    for (const Case& c : cases) {
        if (!strcmp(c.title, "h128 w3 cond exact")) packing(c.plan, c.title, false);
        if (!strcmp(c.title, "bf16x2 d16 state") || !strcmp(c.title, "bf16x3 d16 state")) packing(c.plan, c.title, false);
        if (!strcmp(c.title, "pair h128") || !strcmp(c.title, "select h64")) packing(c.plan, c.title, true);
    }
    end_section("packing", true);
    return 0;
}
