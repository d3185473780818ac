/*
 * flowfusion_amd.h -- C ABI of the MI355X (gfx950) sampling / log-density hot path.
 *
 * This is the drop-in boundary for flowfusion's probability-flow ODE / reverse-SDE
 * sampling and log-density path.  The reference (Cosmo-Pop/flowfusion) is pure Python
 * and has no FFI; what a native replacement has to take over is the time-stepping loop
 * that the reference delegates to torchdiffeq / runs in Python:
 *
 *   ScoreModel.sample_ode_from_base   flowfusion/diffusion.py:566-640  (odeint call :631-639)
 *   ScoreModel.solve_odes_forward     flowfusion/diffusion.py:642-754  (odeint call :744-752)
 *   ScoreModel.sample_sde             flowfusion/diffusion.py:510-563  (Python EM loop :543-562)
 *   ScoreModel.forward (ODE RHS)      flowfusion/diffusion.py:281-334,505-508
 *   MLP.forward                       flowfusion/diffusion.py:82-121
 *   ODEFlow.sample / solve_ode_forward            flowfusion/flow.py:259-306, 308-384
 *   ConditionalODEFlow.sample / solve_ode_forward flowfusion/flow.py:750-799, 801-883
 *   ODEFlow.dynamics / ConditionalODEFlow.dynamics flowfusion/flow.py:89-120, 553-596
 *
 * One fused kernel family ("mlp_ode") covers all of them.  It integrates, for every
 * sample independently,
 *
 *        dy/ds = a_e * y + b_e * NET(y, cond ; c1_e)            (e = RHS evaluation index)
 *
 * where NET is the Linear/SiLU stack of the reference's MLP with the part of the first
 * layer that depends only on time (time embedding or the raw `t` column, plus bias)
 * pre-reduced on the host into the per-evaluation vector c1_e, and (a_e, b_e) are the
 * scalar SDE schedule terms (-beta/2, -g^2/(2 sigma), ...; 0 and 1 for the flows).  The
 * whole explicit Runge-Kutta / Euler-Maruyama loop runs on-chip: the state is read from
 * HBM once and written once.
 *
 * Conventions: all pointers in ff_ode_args are DEVICE pointers to contiguous fp32
 * row-major arrays owned by the caller; launchers enqueue on the given hipStream_t and
 * return immediately (0 = enqueued, <0 = error, nothing enqueued); no global state, safe
 * to call from several host threads on different streams.
 */
#ifndef FLOWFUSION_AMD_H
#define FLOWFUSION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FF_OK               0
#define FF_ERR_BADARG      -1   /* null pointer / negative size / inconsistent plan        */
#define FF_ERR_UNSUPPORTED -2   /* no gfx950 kernel instantiation covers this shape        */
#define FF_ERR_HIP         -3   /* HIP runtime refused the launch (see ff_last_hip_error)  */
#define FF_ERR_EXCHANGE    -4   /* the caller's ff_adapt_buffers.exchange hook returned non-zero */

#define FF_MAX_SLOTS   7        /* Runge-Kutta stage slots kept on chip (dopri5 + FSAL)    */
#define FF_MAX_AUX     4        /* auxiliary linear-combination outputs per launch         */
#define FF_ROW_HDR     32       /* 4-byte words in the header of one evaluation row        */

/* mode flags for ff_ode_args.mode */
#define FF_MODE_STATE      0    /* integrate the state only (`tile` samples per wavefront) */
#define FF_MODE_HUTCH      1    /* state + Hutchinson divergence e^T J e in forward mode
                                   (16 samples + 16 tangent columns per wavefront)         */
#define FF_MODE_EXACT      2    /* state + exact divergence tr J by unit tangents (reference
                                   default: diffusion.py:483-503, flow.py:158-161); see
                                   ff_ode_args.tangent_first/count                          */

/* Hidden-layer activation (the `activation` argument of the reference constructors,
 * diffusion.py:38,77,118; flow.py:41,70; 478,518).  FF_ACT_SILU, the reference default, has
 * instantiations of its own; the others run on instantiations that select the function at
 * run time.  Values and slopes follow torch.nn's definitions. */
#define FF_ACT_SILU        0    /* a * sigmoid(a)                                          */
#define FF_ACT_TANH        1
#define FF_ACT_SIGMOID     2
#define FF_ACT_RELU        3
#define FF_ACT_LEAKY_RELU  4    /* act_param[0] = negative_slope                           */
#define FF_ACT_ELU         5    /* act_param[0] = alpha                                    */
#define FF_ACT_SOFTPLUS    6    /* act_param[0] = beta, act_param[1] = threshold           */
#define FF_ACT_GELU        7    /* a * Phi(a); erf by a 1.5e-7-accurate rational form      */
#define FF_ACT_GELU_TANH   8    /* nn.GELU(approximate="tanh")                             */
#define FF_ACT_COUNT       9

/* Arithmetic of the Linear layers (ff_mlp_plan_t.precision).
 *   FF_PREC_F32     exact fp32 FMA chains on the f32 MFMAs -- what the reference computes; the default.
 *   FF_PREC_BF16X3  opt-in: every operand is split into three bf16 parts (hi + mid + lo carry 24 mantissa
 *                   bits) and a product is the sum of the six bf16 MFMAs whose parts' exponents sum to more than
 *                   2^-24 (hi.hi, hi.mid, mid.hi, hi.lo, mid.mid, lo.hi), accumulated in fp32: fp32-class
 *                   accuracy (error ~1e-7 relative to sum |w||x|, like an fp32 dot product) at the bf16 matrix
 *                   rate.  SiLU networks of 1-4 hidden layers up to 256 wide, dim <= 16, cond_dim <= 16; state-only
 *                   solves (FF_MODE_STATE: noise rows and the adaptive-step fields included); see DESIGN.md section 3.2.
 *   FF_PREC_BF16X2  opt-in: two bf16 parts by round-to-nearest (hi + mid = the operand to 16 significand bits) and
 *                   the three products hi.hi, hi.mid, mid.hi: operands rounded to 2^-17 relative (TF32 keeps 2^-11),
 *                   unbiased, fp32 accumulation; error of a 256-term layer ~4e-7 relative to sum |w||x| in the mean
 *                   (fp32: 2e-8) at half the MFMAs of FF_PREC_BF16X3.  Same networks, every mode (jac_out excepted)
 *                   and, state-only, states of up to 32 dimensions (those plans keep 4 stage slots on chip instead of
 *                   FF_MAX_SLOTS: tables must not name a slot >= 4). */
#define FF_PREC_F32        0
#define FF_PREC_BF16X3     1
#define FF_PREC_BF16X2     2

/* bits OR-ed into ff_ode_args.status by a launch */
#define FF_STATUS_NAN      1u   /* a final state holds a NaN                                */
#define FF_STATUS_BAD_SLOT 2u   /* an evaluation row named a stage slot the kernel does not
                                   keep on chip (>= FF_MAX_SLOTS; >= 4 for the plans with four
                                   slots): that row's right-hand side was NOT stored,
                                   the results are invalid                                  */
#define FF_STATUS_NOISE_ROW 4u  /* ff_mlp_ode_launch_push / _pull only: the table holds a row with
                                   FF_ROW_NOISE, which has no tangent form: the results are invalid */

/* evaluation-row flag bits (word 3 of the row header) */
#define FF_ROW_STEP_END    1u   /* after this evaluation: y += sum_s cout[s] * k[s]        */
#define FF_ROW_NOISE       2u   /* after the step update: y += gn * noise[noise_index]     */
#define FF_ROW_NET_B       4u   /* select plans (ff_mlp_pair_select_plan) only: this row runs
                                   net B (-mlp_p, state rows D..2D-1); without it, net A
                                   (mlp_q, rows 0..D-1).  Other plans ignore the bit           */

/*
 * Kernel plan for one network shape: which compiled instantiation serves it and how its
 * weights are tiled.  Filled by ff_mlp_plan; treat as opaque apart from reading.
 */
typedef struct ff_mlp_plan_t {
    int32_t dim;         /* D  state dimension = network outputs                          */
    int32_t cond_dim;    /* C  conditional inputs (0 = unconditional)                     */
    int32_t n_hidden;    /* number of hidden (Linear+SiLU) layers, >= 1                   */
    int32_t width;       /* common padded hidden width used on chip (multiple of 32)      */
    int32_t dregs;       /* state registers per lane, padded to the kernel's              */
    int32_t cregs;       /* conditional registers per lane                                */
    int32_t kernel_id;   /* index into the compiled instantiation table                   */
    int32_t tile;        /* MFMA columns per wavefront: 32 (32x32x2 f32) or 16 (16x16x4)  */
    int32_t activation;  /* FF_ACT_*                                                      */
    float   act_param[2];/* parameters of the activation (see FF_ACT_*), else 0           */
    int32_t precision;   /* FF_PREC_*: arithmetic of the Linear layers (0 = exact fp32, the default)     */
} ff_mlp_plan_t;

/* Arguments of one fused integration launch. */
typedef struct ff_ode_args {
    const float* x_in;       /* [batch, dim]  initial state                                */
    float*       x_out;      /* [batch, dim]  final state                                  */
    const float* cond;       /* [batch, cond_dim] or NULL                                  */
    const float* probe;      /* [batch, dim]  Hutchinson probe e (FF_MODE_HUTCH) or NULL;
                                [batch, K, dim] with tangent_count = K > 1 (see there)     */
    float*       dlogp_out;  /* [batch]       integrated divergence (modes 1,2) or NULL    */
    const float* noise;      /* [n_noise, batch, dim] standard normals (EM); NULL = in-kernel
                                noise (rng_* below) if the table has FF_ROW_NOISE rows      */
    const float* wpack;      /* packed weights, ff_mlp_wpack_floats() floats               */
    const float* etab;       /* [n_evals, FF_ROW_HDR + width] evaluation rows              */
    const float* in_shift;   /* [dim] or NULL: y0 = (x_in - in_shift) / in_scale           */
    const float* in_scale;   /* [dim] or NULL                                              */
    const float* out_scale;  /* [dim] or NULL: x_out = y * out_scale + out_shift           */
    const float* out_shift;  /* [dim] or NULL                                              */
    uint32_t*    status;     /* device word, OR-ed with FF_STATUS_* bits; NULL ok                */
    int64_t      batch;      /* number of samples                                          */
    int64_t      noise_stride; /* floats between consecutive noise slabs (>= batch*dim)    */
    int32_t      n_evals;    /* rows in etab                                               */
    int32_t      mode;       /* FF_MODE_*                                                  */
    int32_t      tangent_first;  /* FF_MODE_EXACT: this launch carries the unit tangents of   */
    int32_t      tangent_count;  /* dimensions [first, first+count); count 0 = all `dim`.  A
                                    trace over more dimensions than fit one wavefront
                                    (count + 1 <= plan.tile) is the sum of dlogp_out over
                                    several launches, each of which also returns x_out.
                                    FF_MODE_HUTCH: 0 or 1 = one probe per sample; K > 1 = K
                                    probes per sample, `probe` is [batch, K, dim] and
                                    dlogp_out the integral of sum_k p_k^T J p_k (scale the
                                    probes by 1/sqrt(K) for the mean): tile / (1 + K)
                                    samples per tile, K + 1 <= plan.tile (FF_ERR_BADARG
                                    beyond).  FF_PREC_F32 plans only: a split-precision plan
                                    answers FF_ERR_UNSUPPORTED for every K > 1, whether or
                                    not K + 1 would fit a tile.  The K terms one by one (not
                                    only their sum): ff_mlp_ode_launch_probes below.         */
    /* --- adaptive stepping support (all optional; zero / NULL when unused) ---------------------
     * One attempt of an embedded Runge-Kutta step is one launch: the first stage k[0] is supplied
     * by the caller (FSAL), the evaluation rows fill the other slots WITHOUT a STEP_END flag, and
     * the results leave as linear combinations of the slots,
     *     aux_j = use_y_j * y_in + sum_s coef_j[s] * k[s]          j < n_aux <= FF_MAX_AUX
     * (new state, last stage, dense-output midpoint, error estimate).  Their coefficients live in
     * two extra rows appended to etab (so etab has n_evals + 2 rows): row n_evals carries coef_0
     * in its cin words, coef_1 in its cout words and the use_y bits in its flags word; row
     * n_evals+1 carries coef_2 / coef_3 the same way.  With a divergence mode the same
     * combinations of the divergence slots (and use_y_j * dlogp_in) go to aux_lp_out[j]. */
    const float* k1_in;      /* [batch, dim]  stage slot 0 (derivative at the step start) or NULL */
    const float* kl1_in;     /* [batch]       divergence of stage slot 0 or NULL                  */
    const float* dlogp_in;   /* [batch]       integrated divergence at the step start or NULL     */
    float*       aux_out[FF_MAX_AUX];     /* [batch, dim] each, or NULL                            */
    float*       aux_lp_out[FF_MAX_AUX];  /* [batch] each, or NULL                                 */
    int32_t      n_aux;
    int32_t      rng_noise_base;  /* added to the rows' noise_index in the Philox counter          */
    /* --- in-kernel noise (FF_MODE_STATE; used by FF_ROW_NOISE rows when `noise` is NULL) ---------
     * The standard normal of (global sample g = rng_sample_offset + row, noise index n =
     * rng_noise_base + the row header's noise_index, dimension d) is word d%4 of
     *     Philox4x32-10( counter = (g lo, g hi, n, d/4), key = (rng_seed lo, rng_seed hi) )
     * turned into normals pairwise by Box-Muller: u1 = ((w_a >> 8) + 0.5) 2^-24, u2 = (w_b >> 8) 2^-24,
     * z_a = sqrt(-2 ln u1) cos(2 pi u2), z_b = sqrt(-2 ln u1) sin(2 pi u2), (a, b) = (0, 1), (2, 3).
     * Keyed by the GLOBAL sample index, the stream of a sample does not depend on how a batch is cut
     * into launches or shards: 1-, 2-, 4- and 8-GPU runs of one seed give the same samples. */
    uint64_t     rng_seed;
    int64_t      rng_sample_offset;
    /* --- Jacobian output (FF_MODE_EXACT; optional) -----------------------------------------------
     * jac_out[b][j][i] = d rhs_i / d y_j of the LAST evaluation row, for the unit tangents j of this
     * launch (rows tangent_first .. tangent_first + count - 1; several launches fill the matrix).
     * Row j is the product J^T e_j that the reference's Hutch++ / XTrace estimators obtain by
     * reverse mode (`vjp_fn`, diffusion.py:360-372, 431-443); with the whole matrix on hand those
     * estimators are small per-sample linear algebra (flowfusion_amd/trace_estimators.py). */
    float*       jac_out;
    int32_t      jac_all;    /* 0: jac_out = [batch][dim][dim], the Jacobian of the LAST evaluation row (above);
                                1: jac_out = [n_evals][batch][dim][dim], the Jacobian of EVERY row.  The state never
                                depends on the divergence, so one launch can integrate a whole fixed-grid table and
                                hand back everything the Hutch++ / XTrace estimators need; they are then evaluated
                                for all rows at once and combined with the tableau's weights by the caller. */
    int32_t      stage_slots; /* stage slots the table uses (highest slot index + 1, <= FF_MAX_SLOTS); 0 = unknown.
                                 Plans whose kernel keeps fewer slots on chip than FF_MAX_SLOTS (FF_PREC_BF16X2 with dim > 16:
                                 4) require the table to stay within them (a larger value is FF_ERR_UNSUPPORTED).  A row that
                                 names a slot the kernel does not keep is refused by the kernel (FF_STATUS_BAD_SLOT, nothing
                                 stored).  With a correct hint the results do not depend on it. */
    const int32_t* gate;     /* optional DEVICE word read when the kernel starts: 0 = this launch does nothing.  For launches
                                enqueued ahead of a decision taken on the device (ff_mlp_ode_adaptive); NULL = run. */
} ff_ode_args;

/* Library / build identification: returns e.g. "flowfusion_amd 0.1 gfx950". */
const char* ff_version(void);

/* Number of compiled kernel instantiations, and a printable description of each (ids [0, n_f32) are the fp32
 * family in ff_mlp_plan_t.kernel_id order, the split-precision family follows). */
int ff_kernel_count(void);
const char* ff_kernel_name(int kernel_id);
/* Name of the instantiation a plan selects (either family), NULL for an invalid plan. */
const char* ff_plan_kernel_name(const struct ff_mlp_plan_t* plan);

/*
 * Choose the kernel instantiation for a network: `hidden_widths[n_hidden]` are the
 * reference's `units` / `hidden_units` (diffusion.py:61-72, flow.py:64-71).  Widths are
 * padded with zero rows/columns up to a compiled width; FF_ERR_UNSUPPORTED if none fits.
 */
int ff_mlp_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                ff_mlp_plan_t* plan_out);

/* The same for a network whose hidden layers use `activation` (FF_ACT_*) with parameters
 * `act_param[2]` (NULL = zeros); ff_mlp_plan(...) is ff_mlp_plan_act(..., FF_ACT_SILU, NULL, ...). */
int ff_mlp_plan_act(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                    int activation, const float* act_param, ff_mlp_plan_t* plan_out);

/* The same with an explicit arithmetic (FF_PREC_*); FF_ERR_UNSUPPORTED if no instantiation of that family
 * covers the shape / mode / activation.  ff_mlp_plan_act(...) is ff_mlp_plan_prec(..., FF_PREC_F32, ...). */
int ff_mlp_plan_prec(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int mode,
                     int activation, const float* act_param, int precision, ff_mlp_plan_t* plan_out);

/* Floats (4-byte units) in the packed weight buffer of a plan. */
size_t ff_mlp_wpack_floats(const ff_mlp_plan_t* plan);

/*
 * Repack nn.Linear weights (HOST pointers, row-major [out_features, in_features]) into
 * the MFMA operand order of the plan.  W[0] is the first layer with `in_features0`
 * columns, of which columns [x_col0, x_col0+dim) multiply the state and
 * [c_col0, c_col0+cond_dim) the conditional (reference column order: MLP =
 * [time-embedding | x | cond] diffusion.py:109-113; flows = [x | t | cond]
 * flow.py:112-115,583-586); its remaining columns and its bias are NOT packed -- the
 * caller folds them into c1_e.  W[1..n_hidden-1] are hidden layers, W[n_hidden] the output
 * layer.  b[0] is ignored (may be NULL).  `out` is a HOST buffer of
 * ff_mlp_wpack_floats(plan) floats.
 */
int ff_mlp_wpack(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b,
                 const int* hidden_widths, int in_features0, int x_col0, int c_col0,
                 float* out);

/*
 * Enqueue the fused integration on `hip_stream` (a hipStream_t; NULL = default stream).
 * Replaces, per mode and table (see the header comment and INTEGRATION.md):
 *   odeint(self, (z,), t, method, ...)                     diffusion.py:631-639   FF_MODE_STATE
 *   odeint(self, (x0, delta_logpx), t, method, ...)        diffusion.py:744-752   FF_MODE_HUTCH / FF_MODE_EXACT
 *   the Euler-Maruyama loop of sample_sde                  diffusion.py:543-562   FF_MODE_STATE + FF_ROW_NOISE rows
 *   odeint(self.dynamics, (xT[, cond]), t)                 flow.py:299-303, 792-796            FF_MODE_STATE
 *   odeint(self.dynamics_with_jacobian, (x[, cond], logJ)) flow.py:371-382, 869-881            FF_MODE_EXACT
 * Returns FF_OK once enqueued; an argument or shape error enqueues nothing (FF_ERR_HIP from the second of two launches,
 * below, leaves the first enqueued and the outputs undefined).
 * One call may enqueue TWO kernels: the rows left over after the full rounds of tiles the chip runs at once go to the
 * small-batch twin of the kernel when that is faster (same arithmetic, bitwise the same results; FF_TAIL_SPLIT=0 in the
 * environment keeps one kernel).  Batches below one round run on the twin alone where it wins (FF_COOP=0/1 pins that).
 */
int ff_mlp_ode_launch(const ff_mlp_plan_t* plan, const ff_ode_args* args, void* hip_stream);

/*
 * ff_mlp_ode_launch with the Hutchinson divergence of every probe on its own: the same launch (same kernels, same x_out
 * and dlogp_out, bit for bit) also stores
 *     dlogp_probe_out[b][k] = integral of p_k^T (a I + b J_net) p_k      probe k of row b, in the units of dlogp_out
 * for k < K = max(1, args->tangent_count); the row sums are dlogp_out up to the order of the additions.  From them a
 * caller gets the spread of the K single-probe estimates (scale by K if the probes carry 1/sqrt(K)) and so a standard
 * error of their mean.  `dlogp_probe_out` is DEVICE memory of batch * K floats; NULL makes this ff_mlp_ode_launch.
 * With the pointer set, refused before anything is enqueued:
 *     args->mode != FF_MODE_HUTCH                                           FF_ERR_BADARG
 *     K + 1 > plan->tile                                                    FF_ERR_BADARG (as for tangent_count)
 *     k1_in, kl1_in, dlogp_in, jac_out set or n_aux > 0                     FF_ERR_BADARG (an attempt launch carries the
 *                                                                           stage-0 divergence of a sample on one lane;
 *                                                                           per-probe state across attempts is not kept)
 *     a split-precision plan                                                FF_ERR_UNSUPPORTED
 *     a two-network (pair / row-select) plan                                FF_ERR_BADARG (no divergence modes there)
 */
int ff_mlp_ode_launch_probes(const ff_mlp_plan_t* plan, const ff_ode_args* args,
                             float* dlogp_probe_out /* [batch, K], K = max(1, args->tangent_count) */,
                             void* hip_stream);

/* ---- flow-map sensitivities: K tangents pushed through a fixed-grid solve ------------------------------------------------
 * The push-forward units carry up to plan.tile - 1 tangent columns per sample like the Hutchinson kernels, but let them take
 * the stage algebra of the value column: each integrates the variational equation  dv/ds = a_e v + b_e J_net(y, cond) (v, c)
 * with the table's own tableau, c its constant conditional part.  What leaves is the exact derivative of the DISCRETE solver
 * map,
 *     tangent_out[b][k][:] = d x_out[b] / d (x_in[b], cond[b]) . (v_k, c_k)
 * for K directions in one launch; with unit directions the whole Jacobian of the flow map.  x_out is bit for bit the x_out of
 * an FF_MODE_HUTCH launch with tangent_count = K on the same rows.  The affine maps act on tangents by their linear parts:
 * v / in_scale on the way in, * out_scale on the way out, no shift; the conditional part is taken as given.
 *
 * ff_mlp_push_plan: the smallest of the three compiled units that holds the network -- SiLU, fp32, hidden width <= 128
 * with dim <= 16, width <= 256 with dim <= 16 or dim <= 32; cond_dim <= 16 -- else FF_ERR_UNSUPPORTED.  Its kernel_id is
 * FF_PUSH_KERNEL_BASE + an index (kernel names mlp_push_...; not entries of ff_kernel_count).  The packed weights and the
 * evaluation rows are those of any fp32 plan of the shape: ff_mlp_wpack[_floats], ff_mlp_row_width, ff_plan_kernel_name,
 * ff_mlp_samples_per_workgroup accept the plan.  ff_mlp_ode_launch, ff_mlp_ode_launch_probes and ff_mlp_ode_adaptive refuse
 * it (FF_ERR_BADARG).
 *
 * ff_mlp_ode_launch_push(plan, args, cond_tangent, tangent_out, stream): args as for ff_mlp_ode_launch with
 *     args->mode == FF_MODE_HUTCH   tangents as given: K = max(1, args->tangent_count), state parts args->probe [batch, K, dim]
 *                                   (NULL = zero), conditional parts cond_tangent [batch, K, cond_dim] (NULL = zero)
 *     args->mode == FF_MODE_EXACT   unit tangents j = tangent_first .. tangent_first + K - 1 of the combined space
 *                                   [0, dim + cond_dim): j < dim the state unit vector e_j, j >= dim the conditional unit
 *                                   vector e_{j - dim}; K = tangent_count, 0 = all dim + cond_dim (which must then fit)
 * and tangent_out DEVICE memory of batch * K * dim floats.  dlogp_out is not written.  Refused before anything is enqueued:
 *     tangent_out NULL; K < 1 or K + 1 > plan->tile; mode FF_MODE_STATE                           FF_ERR_BADARG
 *     dlogp_out, k1_in, kl1_in, dlogp_in or jac_out set, n_aux > 0                                FF_ERR_BADARG
 *     `noise` set                                                                                 FF_ERR_BADARG
 *     a unit range that reaches past dim + cond_dim; cond_tangent with cond_dim == 0, or with
 *     unit tangents                                                                               FF_ERR_BADARG
 *     a plan that is not a push plan                                                              FF_ERR_BADARG
 *     a split-precision plan                                                                      FF_ERR_UNSUPPORTED
 * Noise rows have no tangent form (Euler-Maruyama is out of scope).  The table lives in DEVICE memory, so the launcher cannot
 * look for FF_ROW_NOISE flags before it enqueues: a push kernel that meets such a row leaves the noise out and ORs
 * FF_STATUS_NOISE_ROW into args->status -- the results are invalid.  (The Python front ends take fixed-grid ODE methods only,
 * whose tables hold no such row.) */
#define FF_PUSH_KERNEL_BASE 0x40000
int ff_push_kernel_count(void);
const char* ff_push_kernel_name(int index);
int ff_mlp_push_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision,
                     ff_mlp_plan_t* plan_out);
int ff_mlp_ode_launch_push(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cond_tangent /* [batch, K, cond_dim] or NULL */,
                           float* tangent_out /* [batch, K, dim] */, void* hip_stream);

/* ---- flow-map pull-backs: K cotangents through a fixed-grid adjoint solve --------------------------------------------------
 * The pull-back units (csrc/ff_mlp_pull.hpp) integrate the CONTINUOUS adjoint, as torchdiffeq's odeint_adjoint does, for the
 * inputs of a solve (no parameter gradients).  Run the ordinary state-only solve x -> x_out first; then ONE pull launch over a
 * table built on the REVERSED span (same method, same step; the ordinary row format) integrates the augmented state
 * [y | alpha_k | gamma_k], k < K, from [x_out, w_k, 0]:
 *     dy/dt = a_e y + b_e NET(y, c)      dalpha/dt = -(a_e alpha + b_e J_net^T alpha)      dgamma/dt = -b_e (dNET/dc)^T alpha
 * (the signs are the kernel's) and returns
 *     args->x_out          the retraced state (compare it with x: the retrace error)
 *     cot_x_out[b][k][:]   w_k^T d x_out[b] / d x[b]
 *     cot_cond_out[b][k][:] w_k^T d x_out[b] / d cond[b]                      (NULL: not wanted)
 * This is NOT the transpose of the discrete map ff_mlp_ode_launch_push differentiates: the two differ by the discretisation
 * error of the method, and y is retraced, not stored.  The affine maps are the launch's own (args->x_in = the forward solve's
 * x_out in ITS output units: in_shift / in_scale undo the forward solve's output map, out_scale / out_shift redo its input
 * map); cotangent_in is taken in the units of x_in (alpha = w * in_scale) and cot_x_out handed back in those of x_out
 * (alpha / out_scale); cot_cond_out is with respect to `cond` as given.
 *
 * An evaluation runs two networks: the forward network, whose value columns park act'(z) of every hidden layer in LDS, and
 * the transposed network W_out^T, W_L^T .. W_2^T, W_1^T (no biases) on the cotangent columns.  ff_mlp_pull_wpack packs both
 * (ff_mlp_pull_wpack_floats floats; arguments as ff_mlp_wpack).  A workgroup is ONE wavefront; its LDS holds
 * slots * (dregs + cregs) * 256 bytes of stage slots, slots = args->stage_slots (0 = FF_MAX_SLOTS; a row naming a slot
 * beyond them sets FF_STATUS_BAD_SLOT), and the stash, (tile / (1 + K)) * n_hidden * width * 4 bytes.  A 4 x 256 network
 * at K = 1 with the four slots of rk4 takes 40 KiB: four wavefronts per compute unit.
 *
 * ff_mlp_pull_plan: the smallest of the three compiled units that holds the network -- SiLU, fp32, hidden width <= 128 with
 * dim <= 16, width <= 256 with dim <= 16 or dim <= 32; cond_dim <= 16 -- whose K = 1 stash fits 160 KiB of LDS beside all
 * FF_MAX_SLOTS stage slots (18 hidden
 * layers at width 256 with dim <= 16, 17 with dim <= 32, 36 at width 128), else FF_ERR_UNSUPPORTED.  Its kernel_id is
 * FF_PULL_KERNEL_BASE + an index (kernel names mlp_pull_...; not entries of ff_kernel_count).  ff_mlp_row_width,
 * ff_plan_kernel_name and ff_mlp_samples_per_workgroup accept the plan; ff_mlp_wpack refuses it (FF_ERR_BADARG) and
 * ff_mlp_wpack_floats returns 0.
 *
 * ff_mlp_ode_launch_pull(plan, args, cotangent_in, cot_x_out, cot_cond_out, stream): args as for ff_mlp_ode_launch with
 * args->mode == FF_MODE_HUTCH and K = args->tangent_count; cotangent_in [batch, K, dim], cot_x_out [batch, K, dim] and
 * cot_cond_out [batch, K, cond_dim] DEVICE memory.  Refused before anything is enqueued:
 *     a plan that is not a pull plan (and a pull plan handed to ff_mlp_ode_launch, ff_mlp_ode_launch_probes,
 *     ff_mlp_ode_launch_push or ff_mlp_ode_adaptive)                                              FF_ERR_BADARG
 *     K < 1 or K > plan->tile - 1; a mode other than FF_MODE_HUTCH                                FF_ERR_BADARG
 *     cotangent_in or cot_x_out NULL; cot_cond_out with cond_dim == 0                             FF_ERR_BADARG
 *     noise, k1_in, kl1_in, dlogp_in, jac_out, dlogp_out or probe set, n_aux > 0                  FF_ERR_BADARG
 *     a depth whose stash does not fit the LDS at this K                                          FF_ERR_UNSUPPORTED
 * A table row with FF_ROW_NOISE has no adjoint form; the table is device memory, so the kernel leaves the noise out and ORs
 * FF_STATUS_NOISE_ROW into args->status -- the results are invalid. */
#define FF_PULL_KERNEL_BASE 0x50000
int ff_pull_kernel_count(void);
const char* ff_pull_kernel_name(int index);
int ff_mlp_pull_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, int activation, int precision,
                     ff_mlp_plan_t* plan_out);
size_t ff_mlp_pull_wpack_floats(const ff_mlp_plan_t* plan);
int ff_mlp_pull_wpack(const ff_mlp_plan_t* plan, const float* const* W, const float* const* b, const int* hidden_widths,
                      int in_features0, int x_col0, int c_col0, float* out);
int ff_mlp_ode_launch_pull(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cotangent_in /* [batch, K, dim] */,
                           float* cot_x_out /* [batch, K, dim] */, float* cot_cond_out /* [batch, K, cond_dim] or NULL */,
                           void* hip_stream);

/* ---- per-row J^T v products along a fixed-grid solve: what Hutch++ / XTrace consume instead of a recorded Jacobian --------
 * The products units (csrc/ff_mlp_vjp.hpp), one sibling per pull-back unit, run the pull-back evaluation body on an ordinary
 * FORWARD table: the value column integrates the state exactly as a state-only solve does (stage slots, the affine maps,
 * args->x_out), and at every evaluation row e the K seed columns of a sample write
 *     prod_out[e][b][k][:] = a_e seed + b_e J_net(y_e, c)^T seed  =  A(y_e) seed,    A = (d rhs / d y)^T at the stage state y_e
 * -- row e of ff_ode_args.jac_all applied to a vector, without the matrix.  seed = seed_in[b][k][:] on every row
 * (seed_row_stride == 0) or seed_in[e][b][k][:] (seed_row_stride == batch * K * dim).  Seeds and products are in the units
 * of the integrated state (after the input map); the state never depends on them.
 *
 * ff_mlp_ode_launch_vjp(plan, args, seed_in, seed_row_stride, prod_out, stream): `plan` is a PULL plan (ff_mlp_pull_plan)
 * and args->wpack its two packs (ff_mlp_pull_wpack); the launch runs the sibling of the plan's unit (ff_vjp_kernel_name
 * (plan->kernel_id - FF_PULL_KERNEL_BASE); FF_VJP_KERNEL_BASE + index names it, no plan carries that id).  args as for
 * ff_mlp_ode_launch with args->mode == FF_MODE_HUTCH and K = args->tangent_count; DEVICE memory.  A tile holds
 * tile / (1 + K) samples; LDS = stage_slots * dregs * 256 bytes of stage slots and the stash of ff_mlp_ode_launch_pull.
 * Refused before anything is enqueued:
 *     a plan that is not a pull plan; K < 1 or K > plan->tile - 1; a mode other than FF_MODE_HUTCH     FF_ERR_BADARG
 *     seed_in or prod_out NULL; a seed_row_stride other than 0 or batch * K * dim                      FF_ERR_BADARG
 *     noise, k1_in, kl1_in, dlogp_in, jac_out, dlogp_out or probe set, n_aux > 0                       FF_ERR_BADARG
 *     a depth whose stash does not fit the LDS at this K                                               FF_ERR_UNSUPPORTED
 * A table row with FF_ROW_NOISE has no product form: the kernel leaves the noise out and ORs FF_STATUS_NOISE_ROW into
 * args->status; FF_STATUS_BAD_SLOT and FF_STATUS_NAN (a NaN in the final state) as in ff_mlp_ode_launch_pull. */
#define FF_VJP_KERNEL_BASE 0x60000
int ff_vjp_kernel_count(void);
const char* ff_vjp_kernel_name(int index);
int ff_mlp_ode_launch_vjp(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* seed_in, int64_t seed_row_stride,
                          float* prod_out /* [n_evals, batch, K, dim] */, void* hip_stream);

/* ---- the exact discrete adjoint of a fixed-grid solve, from recorded stage states ----------------------------------------
 * ff_mlp_ode_launch_pull integrates the CONTINUOUS adjoint; it is not the transpose of the map the forward kernels apply.  The
 * two units of csrc/ff_mlp_dadj.hpp, one sibling of each per pull-back unit, compute that transpose.  The forward solve is a
 * program over the rows e = 0 .. n_evals - 1 of an ordinary table,
 *     y_e = x + sum_s cin_e[s] k[s];  r_e = a_e y_e + b_e NET(y_e, c);  k[slot_e] = r_e;  FF_ROW_STEP_END: x += sum_s cout_e[s] k[s]
 * and its transpose runs the SAME table from the last row to the first on adjoint slots; it needs y_e of every row.
 *
 * ff_mlp_ode_launch_record(plan, args, record_out, stream): `plan` is a PULL plan and args->wpack its two packs
 * (ff_mlp_pull_wpack); args as for a state-only ff_mlp_ode_launch (FF_MODE_STATE).  Integrates the state (stage slots, the
 * affine maps, args->x_out, args->status) on one wavefront per tile of plan->tile samples and stores, at every row,
 *     record_out[(e * batch + b) * dim + d] = y_e[d]           in the integrated state's units (after the input map)
 * ff_mlp_record_floats(batch, n_evals, dim) floats of DEVICE memory.  LDS = stage_slots * dregs * 256 bytes.
 *
 * ff_mlp_ode_launch_pull_discrete(plan, args, record_in, cotangent_in, cot_x_out, cot_cond_out, stream): args is the FORWARD
 * launch's -- same table, same cond, same affine maps -- with args->mode == FF_MODE_HUTCH and K = args->tangent_count;
 * args->x_in and args->x_out are ignored.  Cotangents are taken in the units of the forward x_out (times out_scale) and handed
 * back in the units of the forward x_in (over in_scale): cot_x_out[b][k] = w_k^T d x_out / d x_in of the discrete map, exactly,
 * cot_cond_out[b][k] = w_k^T d x_out / d cond.  A tile holds tile / (1 + K) samples; LDS = stage_slots * dregs * 256 bytes of
 * adjoint slots and the stash of ff_mlp_ode_launch_pull -- never more than that launch's.
 *
 * Both refuse, before anything is enqueued:
 *     a plan that is not a pull plan                                                                   FF_ERR_BADARG
 *     record: a mode other than FF_MODE_STATE; discrete: other than FF_MODE_HUTCH, K < 1, K > tile - 1 FF_ERR_BADARG
 *     record_out / record_in, cotangent_in or cot_x_out NULL; cot_cond_out with cond_dim == 0          FF_ERR_BADARG
 *     noise, k1_in, kl1_in, dlogp_in, jac_out, dlogp_out or probe set, n_aux > 0                       FF_ERR_BADARG
 *     a depth whose stash does not fit the LDS at this K                                               FF_ERR_UNSUPPORTED
 * The kernel ids FF_REC_KERNEL_BASE + index and FF_DADJ_KERNEL_BASE + index name the units (index = plan->kernel_id -
 * FF_PULL_KERNEL_BASE); no plan carries them.  FF_STATUS_BAD_SLOT: a row names a slot beyond args->stage_slots (it stores
 * nothing forward and contributes nothing backward).  FF_STATUS_NOISE_ROW: the table holds a noise row; the record launch
 * leaves the noise out, so the results belong to another map. */
#define FF_REC_KERNEL_BASE 0x70000
#define FF_DADJ_KERNEL_BASE 0x80000
int ff_rec_kernel_count(void);
const char* ff_rec_kernel_name(int index);
int ff_dadj_kernel_count(void);
const char* ff_dadj_kernel_name(int index);
size_t ff_mlp_record_floats(int64_t batch, int32_t n_evals, int32_t dim);
int ff_mlp_ode_launch_record(const ff_mlp_plan_t* plan, const ff_ode_args* args, float* record_out /* [n_evals, batch, dim] */,
                             void* hip_stream);
int ff_mlp_ode_launch_pull_discrete(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* record_in,
                                    const float* cotangent_in /* [batch, K, dim] */, float* cot_x_out /* [batch, K, dim] */,
                                    float* cot_cond_out /* [batch, K, cond_dim] or NULL */, void* hip_stream);

/* ---- the gradient of a fixed-grid Hutchinson log-density, from recorded stage states ---------------------------------------
 * With one probe eps per row the forward program above also integrates the divergence,
 *     kl[slot_e] = a_e eps.eps + b_e eps^T J_net(y_e, c) eps;   FF_ROW_STEP_END: lp += sum_s cout_e[s] kl[s]
 * and a log-density is  lp + log prior(x_out).  The unit of csrc/ff_mlp_lgrad.hpp, one sibling per pull-back unit, runs the
 * transposed row program of ff_mlp_ode_launch_pull_discrete with one scalar adjoint slot per stage slot for lp and the
 * second-order source  w grad (eps^T J_net eps)  in every row: reverse mode over the forward-mode tangent, exact for the discrete
 * sum at fixed probes.
 *
 * ff_mlp_ode_launch_logp_grad(plan, args, record_in, probe_in, dlogp_cotangent, cotangent_in, grad_x_out, grad_cond_out, stream):
 * `plan` is a PULL plan and args->wpack its two packs; args is the FORWARD launch's -- same table, same cond, same affine maps --
 * with args->mode == FF_MODE_HUTCH and args->tangent_count 0 or 1; args->x_in and args->x_out are ignored.
 *     record_in        [n_evals, batch, dim]       the record launch's output
 *     probe_in         [batch, dim]                the Hutchinson probe of each row (in the integrated state's units)
 *     dlogp_cotangent  [batch] or NULL (= 1)       per-row weight of the divergence integral: 1 / K for a probe average over K
 *                                                  rows, 1 for unit probes of an exact trace, 0 switches the second-order path off
 *     cotangent_in     [batch, dim]                cotangent of the final state (the prior's gradient), units of x_out
 *     grad_x_out       [batch, dim]                d (w lp + cotangent . x_out) / d x_in
 *     grad_cond_out    [batch, cond_dim] or NULL   the same with respect to cond
 * Two columns per row, tile / 2 rows per tile; LDS = stage_slots * dregs * 256 bytes of adjoint slots + 64 * n_hidden * width
 * bytes of stash (two words per hidden unit and row).
 *
 * It refuses, before anything is enqueued:
 *     a plan that is not a pull plan                                                                   FF_ERR_BADARG
 *     a mode other than FF_MODE_HUTCH, tangent_count > 1                                               FF_ERR_BADARG
 *     record_in, probe_in, cotangent_in or grad_x_out NULL; grad_cond_out with cond_dim == 0           FF_ERR_BADARG
 *     noise, k1_in, kl1_in, dlogp_in, jac_out, dlogp_out or probe set, n_aux > 0                       FF_ERR_BADARG
 *     a depth whose stash does not fit the LDS (above about 9 x 256, 19 x 128)                         FF_ERR_UNSUPPORTED
 * FF_LGRAD_KERNEL_BASE + index names the unit (index = plan->kernel_id - FF_PULL_KERNEL_BASE); no plan carries it.
 * FF_STATUS_BAD_SLOT and FF_STATUS_NOISE_ROW: as for ff_mlp_ode_launch_pull_discrete. */
#define FF_LGRAD_KERNEL_BASE 0x90000
int ff_lgrad_kernel_count(void);
const char* ff_lgrad_kernel_name(int index);
int ff_mlp_ode_launch_logp_grad(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* record_in,
                                const float* probe_in /* [batch, dim] */, const float* dlogp_cotangent /* [batch] or NULL */,
                                const float* cotangent_in /* [batch, dim] */, float* grad_x_out /* [batch, dim] */,
                                float* grad_cond_out /* [batch, cond_dim] or NULL */, void* hip_stream);

/* Which kernel(s) ff_mlp_ode_launch enqueues for `batch` samples of a plan in `mode` (`tangent_count`: as in ff_ode_args,
 * 0 = the mode's default; `jac_out` != 0: a launch with a Jacobian output, which is never split): the launcher's rule as a
 * query, so that callers, benchmarks and tests can name the kernel that ran without timing it.  Honours FF_COOP /
 * FF_TAIL_SPLIT in the environment like the launcher does.  Negative: FF_ERR_*.  Two-network (pair) plans follow the
 * same rule -- the 256- and 128-wide pair kernels have a twin, the 64-wide one answers FF_LAUNCH_ONE_WAVE always -- and
 * take FF_MODE_STATE without a Jacobian output only (anything else: FF_ERR_BADARG). */
#define FF_LAUNCH_ONE_WAVE          0   /* the one-wavefront-per-tile kernel                                         */
#define FF_LAUNCH_TWIN              1   /* its cooperative small-batch twin (or a wide catch-all): a tile per workgroup */
#define FF_LAUNCH_ONE_WAVE_AND_TWIN 2   /* full rounds on the first, the leftover rows on the twin (two launches)     */
int ff_mlp_launch_kind(const ff_mlp_plan_t* plan, int64_t batch, int32_t mode, int32_t tangent_count, int32_t jac_out);

/* Samples handled by one workgroup of a plan/mode (for sizing and roofline accounting). */
int ff_mlp_samples_per_workgroup(const ff_mlp_plan_t* plan, int mode);

/* hipError_t of the most recent failing launch on this thread (0 if none). */
int ff_last_hip_error(void);

/* ---- two-network plans: the symplectic flows (flowfusion_amd/symplectic.py) ----------------------------------------
 * Right-hand side  a_e y + b_e (NET_A(y, cond; c1A_e) + NET_B(y, cond; c1B_e))  with two networks of one shape over a
 * state of `dim` = 2D dimensions [q | p].  The reference's v = [mlp_q(p, cond, t), -mlp_p(q, cond, t)]
 * (symplectic.py:80-122) is packed by ff_mlp_pair_wpack: NET_A = mlp_q reading the p half and writing rows 0..D-1,
 * NET_B = mlp_p reading the q half and writing rows D..2D-1 with its output layer negated.  State-only (FF_MODE_STATE:
 * the field is divergence-free by construction), SiLU; small batches and the leftover rows of a longer launch run on a
 * cooperative twin as for the single-network kernels (bitwise the same results; FF_COOP / FF_TAIL_SPLIT).  A pair plan is an ff_mlp_plan_t whose kernel_id is
 * FF_PAIR_KERNEL_BASE + an index into the pair family; ff_mlp_ode_launch, ff_mlp_ode_adaptive, ff_plan_kernel_name,
 * ff_mlp_launch_kind and ff_mlp_samples_per_workgroup accept it.  Its evaluation rows carry FF_ROW_HDR header words,
 * then c1 of net A (plan.width words), then c1 of net B (plan.width words): ff_mlp_row_width(plan) = 2 * plan.width. */
#define FF_PAIR_KERNEL_BASE 0x10000
/* Number of compiled pair instantiations and the name of each (index 0 .. count - 1). */
int ff_pair_kernel_count(void);
const char* ff_pair_kernel_name(int index);
/* Choose the pair instantiation for a state of `dim` (even) dimensions, `cond_dim` conditional inputs and the
 * reference's `units` (hidden_widths of each network); FF_ERR_UNSUPPORTED if none holds it. */
int ff_mlp_pair_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);
/* Floats in the packed weights of a pair plan: two single-network packs back to back; 0 for any other plan. */
size_t ff_mlp_pair_wpack_floats(const ff_mlp_plan_t* plan);
/* Pack the two reference networks (HOST pointers, nn.Linear layout as in ff_mlp_wpack): Wq / bq = mlp_q_dynamics,
 * Wp / bp = mlp_p_dynamics, first layers of `in_features0` columns of which [x_col0, x_col0 + dim/2) multiply that
 * network's half of the state (p for mlp_q, q for mlp_p) and [c_col0, c_col0 + cond_dim) the conditional; the other
 * columns (the time features) and the first biases go into c1.  `out` holds ff_mlp_pair_wpack_floats(plan) floats. */
int ff_mlp_pair_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                      const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                      int x_col0, int c_col0, float* out);
/* Words of first-layer bias per evaluation row (an etab row is FF_ROW_HDR + this many floats): plan.width, or
 * 2 * plan.width for a pair plan (plan.width for a select plan).  -1 for NULL. */
int ff_mlp_row_width(const ff_mlp_plan_t* plan);

/* ---- row-select plans: one network per evaluation row (kick-drift-kick leapfrog of the symplectic flows) ------------
 * The two networks of a pair plan, same shapes, same packed weights (ff_mlp_pair_wpack[_floats] take either plan), but an
 * evaluation row runs ONE of them: net B if its flag word has FF_ROW_NET_B, net A otherwise.  The other half of the
 * network output is exact zero, so with a = 0 a row's right-hand side and its FF_ROW_STEP_END update move one half of the
 * state and leave the other bitwise untouched -- a shear.  A row carries only its own network's c1: the row stride is
 * FF_ROW_HDR + plan.width (ff_mlp_row_width = plan.width).  Rows may select the networks in any order.
 * ff_mlp_pair_select_plan has the envelope and the preference of ff_mlp_pair_plan; the plan's kernel_id is
 * FF_PAIR_SELECT_KERNEL_BASE + the same index (kernel names mlp_pairsel_...; the select kernels are not entries of
 * ff_kernel_count or ff_pair_kernel_count).  ff_plan_kernel_name, ff_mlp_row_width, ff_mlp_samples_per_workgroup,
 * ff_mlp_launch_kind and ff_mlp_ode_launch accept it; ff_mlp_ode_adaptive refuses it (FF_ERR_BADARG).
 * ff_mlp_ode_launch on a select plan: FF_MODE_STATE only; the affine maps, `gate`, `status` and noise rows (FF_ROW_NOISE,
 * from a buffer or in-kernel: the code is the pair kernel's) work as for a pair plan; `k1_in`, `n_aux` > 0 and `jac_out`
 * are refused with FF_ERR_BADARG.  The launcher's rule (twin for small batches and leftover tiles; FF_COOP /
 * FF_TAIL_SPLIT) is the one of the pair plans, with the pair instances' constants. */
#define FF_PAIR_SELECT_KERNEL_BASE 0x20000
int ff_mlp_pair_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);

/* ---- row-select pull-backs: the transpose of a leapfrog of the symplectic flows (csrc/ff_mlp_pullsel.hpp) ---------------
 * A leapfrog row is a shear: it moves one half of [q | p] by w f(other half, cond, t).  Its transpose,
 *     lambda_q = lambda_q',  lambda_p = lambda_p' + w J_f(p)^T lambda_q',  gamma += w (df/dcond)^T lambda_q',
 * needs only the half the row leaves alone, so the row program of ff_mlp_ode_launch_pull run on the table of the REVERSED grid
 * (solvers.plan_leapfrog(grid.flip(0)): bitwise the forward table's times and weights in reverse order) retraces the state
 * from the forward solve's x_out and computes the EXACT discrete adjoint of the forward leapfrog on the way -- nothing is
 * recorded.  One sibling per pull-back unit (kernel names mlp_pullsel_...), same tile, registers, ring and LDS formula; a row
 * runs the forward and the transposed network of mlp_p if its flag word has FF_ROW_NET_B, of mlp_q otherwise, and carries
 * only that network's c1 (row stride FF_ROW_HDR + plan.width; ff_mlp_row_width = plan.width).  Rows may select in any order.
 *
 * ff_mlp_pull_select_plan(dim, cond_dim, n_hidden, hidden_widths, plan_out): `dim` is the joint 2D and must be even
 * (FF_ERR_BADARG); the envelope, preference and depth ceilings are ff_mlp_pull_plan's for that dim -- SiLU, fp32, hidden width
 * <= 128 with dim <= 16, width <= 256 with dim <= 16 or dim <= 32; cond_dim <= 16 -- else FF_ERR_UNSUPPORTED.  The plan's
 * kernel_id is FF_PULL_SELECT_KERNEL_BASE + an index (not entries of ff_kernel_count or ff_pull_kernel_count).
 * ff_plan_kernel_name, ff_mlp_row_width and ff_mlp_samples_per_workgroup accept the plan; every other launch and packer
 * refuses it with FF_ERR_BADARG (ff_mlp_wpack_floats, ff_mlp_pair_wpack_floats and ff_mlp_pull_wpack_floats return 0).
 *
 * ff_mlp_pull_select_wpack takes the arguments of ff_mlp_pair_wpack and writes ff_mlp_pull_select_wpack_floats(plan) = 2 x
 * ff_mlp_pull_wpack_floats floats: [A_q | B_q | A_p | B_p], each half what ff_mlp_pull_wpack makes of that network embedded in
 * the joint state as ff_mlp_pair_wpack embeds it (mlp_q: columns on the p half, rows 0..D-1; mlp_p: columns on the q half, rows
 * D..2D-1, output weights and bias negated).
 *
 * ff_mlp_ode_launch_pull_select: the arguments, refusals, LDS bound and status bits of ff_mlp_ode_launch_pull; it refuses every
 * plan that is not a pull-select plan (FF_ERR_BADARG), as ff_mlp_ode_launch_pull refuses this one.  cot_cond_out accumulates
 * from both networks.  A leapfrog table names slot 0 only: args->stage_slots = 1 keeps one stage slot in LDS. */
#define FF_PULL_SELECT_KERNEL_BASE 0xA0000
int ff_pullsel_kernel_count(void);
const char* ff_pullsel_kernel_name(int index);
int ff_mlp_pull_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);
size_t ff_mlp_pull_select_wpack_floats(const ff_mlp_plan_t* plan);
int ff_mlp_pull_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                             const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                             int x_col0, int c_col0, float* out);
int ff_mlp_ode_launch_pull_select(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cotangent_in /* [batch, K, dim] */,
                                  float* cot_x_out /* [batch, K, dim] */, float* cot_cond_out /* [batch, K, cond_dim] or NULL */,
                                  void* hip_stream);

/* ---- row-select push-forwards: the derivative of a leapfrog of the symplectic flows (csrc/ff_mlp_pushsel.hpp) ------------
 * The forward-mode form of a leapfrog row (a shear of [q | p]) is
 *     dq' = dq + w (J_f(p) dp + df/dcond dcond),   dp' = dp          (or the kick, its mirror image),
 * which is the stage algebra of ff_mlp_ode_launch_push on a select row (a_e = 0): K tangent columns beside every value column
 * run through the row's network, and the select pack's structural zeros leave the other half of every tangent bitwise alone.
 * One launch over the rows of solvers.plan_leapfrog(grid) returns the state of ff_mlp_pair_select_plan's launch on the same
 * rows (bit for bit at hidden widths 128 and 256) and tangent_out = d x_out / d (x_in, cond) . tangent, the derivative of the
 * discrete map -- on the forward grid the sampler's, on the flipped grid the log-density direction's.  One sibling per
 * push-forward unit (kernel names mlp_pushsel_...), same tile, registers, occupancy and ring; a row runs mlp_p's pack if its
 * flag word has FF_ROW_NET_B, mlp_q's otherwise, and carries only that network's c1 (row stride FF_ROW_HDR + plan.width;
 * ff_mlp_row_width = plan.width).  Rows may select in any order.
 *
 * ff_mlp_push_select_plan(dim, cond_dim, n_hidden, hidden_widths, plan_out): `dim` is the joint 2D and must be even
 * (FF_ERR_BADARG); the envelope and preference are ff_mlp_push_plan's for that dim -- SiLU, fp32, hidden width <= 128 with
 * dim <= 16, width <= 256 with dim <= 16 or dim <= 32; cond_dim <= 16 -- else FF_ERR_UNSUPPORTED.  The plan's kernel_id is
 * FF_PUSH_SELECT_KERNEL_BASE + an index (not entries of ff_kernel_count or ff_push_kernel_count).  ff_plan_kernel_name,
 * ff_mlp_row_width and ff_mlp_samples_per_workgroup accept the plan; every other launch and packer refuses it with
 * FF_ERR_BADARG (ff_mlp_wpack_floats, ff_mlp_pair_wpack_floats and the pull packers' sizes return 0).
 *
 * ff_mlp_push_select_wpack takes the arguments of ff_mlp_pair_wpack and writes ff_mlp_push_select_wpack_floats(plan) floats:
 * two forward packs back to back, each what ff_mlp_wpack makes of that network embedded in the joint state as
 * ff_mlp_pair_wpack embeds it (mlp_q: columns on the p half, rows 0..D-1; mlp_p: columns on the q half, rows D..2D-1, output
 * weights and bias negated).
 *
 * ff_mlp_ode_launch_push_select: the arguments, modes (FF_MODE_HUTCH: tangents as given in args->probe [batch, K, dim] and
 * cond_tangent [batch, K, cond_dim], NULL = zero; FF_MODE_EXACT: the unit vectors tangent_first .. + tangent_count - 1 of
 * [0, dim + cond_dim)), refusals and status bits of ff_mlp_ode_launch_push; it refuses every plan that is not a push-select
 * plan (FF_ERR_BADARG), as ff_mlp_ode_launch_push refuses this one. */
#define FF_PUSH_SELECT_KERNEL_BASE 0xB0000
int ff_pushsel_kernel_count(void);
const char* ff_pushsel_kernel_name(int index);
int ff_mlp_push_select_plan(int dim, int cond_dim, int n_hidden, const int* hidden_widths, ff_mlp_plan_t* plan_out);
size_t ff_mlp_push_select_wpack_floats(const ff_mlp_plan_t* plan);
int ff_mlp_push_select_wpack(const ff_mlp_plan_t* plan, const float* const* Wq, const float* const* bq,
                             const float* const* Wp, const float* const* bp, const int* hidden_widths, int in_features0,
                             int x_col0, int c_col0, float* out);
int ff_mlp_ode_launch_push_select(const ff_mlp_plan_t* plan, const ff_ode_args* args, const float* cond_tangent /* [batch, K, cond_dim] or NULL */,
                                  float* tangent_out /* [batch, K, dim] */, void* hip_stream);

/* ---- streaming helpers beside the fused integrator (csrc/ff_aux.hip) --------------------------------- */

/* Noise index reserved for the prior draw of a sample in the counter-based stream (never used by the
 * Euler-Maruyama rows, which count from rng_noise_base upwards). */
#define FF_PRIOR_NOISE_INDEX 0xFFFFFFFFu
/* Noise index reserved for the Hutchinson probe of a sample: e = sign(z(seed, global row, this index, d)) replaces the
 * host draw `torch.sign(torch.randn(shape)).to(device)` (diffusion.py:701) when a log-density batch is sharded over GPUs
 * or the host draw should leave the critical path (host side: probe="philox"). */
#define FF_PROBE_NOISE_INDEX 0xFFFFFFFEu
/* Noise indices reserved for the Hutch++ / XTrace probes of a sample (diffusion.py:703-719: S, G, O drawn once per solve as
 * `torch.sign(torch.randn(n, B, D))`): probe c of the FIRST set (S, or O) is the sign of z(seed, global row,
 * FF_TRACE_PROBE_NOISE_BASE + c, d), probe c of the SECOND set (G) that of index FF_TRACE_PROBE_NOISE_BASE + 0x8000 + c
 * (host side: probe="philox" on a model with hutchpp=True / xtrace=True) -- the same probes whatever the sharding. */
#define FF_TRACE_PROBE_NOISE_BASE 0xFFFE0000u
/* Noise indices reserved for the K momentum draws of a data point in the marginal log-density of the symplectic flows
 * (ff_marginal_expand / ff_marginal_reduce below): momentum k of global row g is z(seed, g, FF_MOMENTUM_NOISE_BASE + k, d),
 * k < 4096 -- a range of its own below the trace probes', so a seed shared with the prior draw or a probe set gives
 * unrelated momenta. */
#define FF_MOMENTUM_NOISE_BASE 0xFFFD0000u
/* Noise indices reserved for probes 1 .. K-1 of a sample in a K-probe Hutchinson launch (ff_ode_args.tangent_count = K in
 * FF_MODE_HUTCH; ff_probe_fill below): probe k >= 1 of global row g is the sign of z(seed, g, FF_HUTCH_PROBE_NOISE_BASE + k,
 * d), k < 65536; probe 0 keeps FF_PROBE_NOISE_INDEX, so K = 1 is the single-probe stream.  A range of its own below the
 * momenta's. */
#define FF_HUTCH_PROBE_NOISE_BASE 0xFFFC0000u
#define FF_MAX_HUTCH_PROBES 65535

/*
 * out[r][d] = scale * z(seed, global row sample_offset + r, noise_index, d)  for r < batch, d < dim, with z the
 * standard normal of the in-kernel stream defined at ff_ode_args.rng_seed (Philox4x32-10 + Box-Muller).
 * Replaces the prior draw `self.sde.prior(dims).sample([batch])` of sample_sde (diffusion.py:532-536; the
 * priors are Normal(0, 1) :1093 and Normal(0, sigma_max) :1003, hence `scale`) when a batch is sharded over
 * GPUs: each rank fills only its rows and every world size starts from the same points.  `out` is a DEVICE
 * pointer to [batch, dim] contiguous fp32.  Enqueues on hip_stream.
 */
int ff_normal_fill(float* out, int64_t batch, int32_t dim, uint64_t seed, int64_t sample_offset,
                   uint32_t noise_index, float scale, void* hip_stream);

/*
 * The K Rademacher probes of a K-probe Hutchinson launch, in the layout ff_ode_args.probe takes ([batch, K, dim]):
 *   out[r][k][d] = z(seed, sample_offset + r, index_k, d) >= 0 ? scale : -scale,
 *   index_0 = FF_PROBE_NOISE_INDEX,  index_k = FF_HUTCH_PROBE_NOISE_BASE + k  (1 <= k < K <= FF_MAX_HUTCH_PROBES)
 * -- bit for bit `where(ff_normal_fill(.., index_k, 1.0f) >= 0, 1, -1) * scale` of the K fills, stacked: one write-only
 * pass instead of K fills, a stack, a comparison and a product.  Rows are keyed by the global row, so a shard's rows are
 * the rows of the whole.  scale = 1/sqrt(K) makes the launch's sum over probes their mean.  `out` is a DEVICE pointer;
 * enqueues on hip_stream.  ff_probe_fill_host: the same on host memory (libm's transcendentals: a sign may differ from
 * the device's only where |z| is within their 2e-6 of zero).  FF_ERR_BADARG: out NULL, batch < 0, K or dim out of range.
 */
int ff_probe_fill(float* out, int64_t batch, int32_t K, int32_t dim, uint64_t seed, int64_t sample_offset, float scale,
                  void* hip_stream);
int ff_probe_fill_host(float* out, int64_t batch, int32_t K, int32_t dim, uint64_t seed, int64_t sample_offset, float scale);

/*
 * out = x_coef * x + sum_s coef[s] * k[s]   over n contiguous fp32 elements (DEVICE pointers; x may be NULL,
 * k[s] is not read when coef[s] == 0 and x is not read when x_coef == 0: such an array may hold anything, NaN included,
 * and its alignment does not decide between the 16-byte and the scalar loop; out may alias x or a k[s]).
 * The stage-input, step-update, dense-output and error-estimate algebra of an explicit Runge-Kutta step for a
 * right-hand side evaluated OUTSIDE the library -- the reference accepts any `model=` module in ScoreModel
 * (diffusion.py:201,233-238) and hands the stepping to torchdiffeq (call sites diffusion.py:631-639, 744-752),
 * which spends one elementwise pass over the state per term; this is one pass per combination.
 */
typedef struct ff_combine_args {
    const float* x;
    const float* k[FF_MAX_SLOTS];
    float        coef[FF_MAX_SLOTS];
    float        x_coef;
    float*       out;
    int64_t      n;
} ff_combine_args;
int ff_stage_combine(const ff_combine_args* args, void* hip_stream);

/*
 * Scaled RMS norms of an adaptive step, in one launch:
 *     out[i] = sqrt( mean_k ( (num_i[k] - sub_i[k]) / (atol + rtol * max(|scale0_i[k]|, |scale1_i[k]|)) )^2 )   i < n_terms
 *     out[n_terms] = 1 if `check[0 .. n_check)` holds a NaN or an infinity, else 0
 * (`sub` and `scale1` may be NULL).  These are the norms torchdiffeq's adaptive solvers take of the tuple state behind
 * the reference's default `method="dopri5"` (call sites diffusion.py:631-639, 744-752; flow.py:299-303, 371-382):
 * `_compute_error_ratio` (num = error estimate, scale0 / scale1 = y0 / y1) and `_select_initial_step` (num = y or f or
 * f1 - f0, scale0 = y); one term per component of the tuple, the caller takes the maximum (the mixed norm).
 * Deterministic (no floating-point atomics).  All pointers are DEVICE pointers; `out` has n_terms + 1 floats;
 * `workspace` is ff_scaled_rms_workspace_bytes() bytes of device memory whose first 16 bytes are zero before the first
 * use (the kernel leaves them zero); one workspace per stream.
 */
#define FF_NORM_TERMS 3
typedef struct ff_norm_term {
    const float* num;
    const float* sub;
    const float* scale0;
    const float* scale1;
    int64_t      n;
} ff_norm_term;
size_t ff_scaled_rms_workspace_bytes(void);
int ff_scaled_rms(const ff_norm_term* terms, int32_t n_terms, float atol, float rtol, const float* check,
                  int64_t n_check, float* out, void* workspace, void* hip_stream);

/* ---- marginal log-density of a symplectic flow over K momentum draws (csrc/ff_marginal.hip, csrc/ff_marginal.h) ----
 *
 * SymplecticFlowModel.log_prob (flowfusion/symplectic.py:204-253) draws ONE momentum p0 per data point and returns
 * log N(z1) - log N(p0) - sum log scale, z1 the solution from [q0 | p0].  The flow preserves volume in the joint space,
 * so the data density is the marginal p(q0) = E_{p0 ~ N}[N(Phi(q0, p0)) / N(p0)] and the reference's value a one-draw
 * estimate of it.  These two kernels are the ends of the K-draw estimate, around any state-only solve of the B K rows:
 * data point r, momentum k is row r K + k (the K rows of a point are contiguous), 1 <= K <= 4096.
 *
 * ff_marginal_expand:   z0[r K + k][0 : D]   = (x[r] - shift) / scale      fp32 subtraction, correctly rounded division
 *                       z0[r K + k][D : 2 D] = z(seed, sample_offset + r, FF_MOMENTUM_NOISE_BASE + k, d)
 *                       cond_out[r K + k]    = cond[r]
 *   x [B][D]; shift, scale [D] or NULL (0 and 1); cond [B][C], already normalised, or NULL (C and cond_out are then
 *   ignored); z0 [B K][2 D]; cond_out [B K][C].  The momenta are bit for bit what ff_normal_fill writes for that noise
 *   index and global row.
 * ff_marginal_reduce:   lw_k       = -1/2 (sum_{2D} z1[r K + k]^2 - sum_D p0(r, k)^2) - (D / 2) log 2 pi
 *                       out_logp[r] = logsumexp_k lw_k - log K - log_det
 *                       out_ess[r]  = (sum_k w_k)^2 / sum_k w_k^2,   w_k = exp(lw_k - max_k lw_k)
 *   z1 [B K][2 D]; out_logp [B]; out_ess [B] or NULL; log_det = sum log scale.  p0 is regenerated from the stream (pass
 *   the seed and sample_offset of the expand), neither stored nor read back.  The sums and the log-sum-exp run in double
 *   and are rounded to fp32 once.  Non-finite input follows torch.logsumexp in float64: a NaN in any lw_k gives NaN,
 *   all -inf gives -inf (and an effective sample size of NaN: no draw has weight).
 * A data point's results do not depend on B, on its position in the batch or on the launch geometry, so a batch may be
 * processed in chunks (sample_offset + first point of the chunk) or sharded over ranks with bitwise the same results.
 * All pointers are DEVICE pointers; both enqueue on hip_stream; B == 0 is FF_OK without a launch.  The _host twins run
 * the same arithmetic (csrc/ff_marginal.h) on HOST pointers for tests without a GPU: their normals come through libm
 * and agree with the device's to rounding, not bit for bit; the two host functions are consistent with each other.
 */
int ff_marginal_expand(const float* x, const float* shift, const float* scale, const float* cond, int64_t B, int32_t D,
                       int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0, float* cond_out,
                       void* hip_stream);
int ff_marginal_reduce(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                       double log_det, float* out_logp, float* out_ess, void* hip_stream);
int ff_marginal_expand_host(const float* x, const float* shift, const float* scale, const float* cond, int64_t B,
                            int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* z0,
                            float* cond_out);
int ff_marginal_reduce_host(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                            double log_det, float* out_logp, float* out_ess);

/* ---- the gradient of the K-draw marginal log-density (csrc/ff_marginal.hip, csrc/ff_marginal.h) ---------------------
 *
 * With the momenta fixed (the counter-based stream), L[r] = logsumexp_k lw_k - log K - log_det of ff_marginal_reduce has
 * dL / d lw_k = wn_k, the normalised weight of draw k, and lw_k = log N(z1_k) - log N(p0_k) depends on x and the
 * conditional through z1_k alone: its gradient is the pull-back of the one cotangent -z1_k through the solve (whatever
 * computes it; the library's: ff_mlp_ode_launch_pull_select on the flipped leapfrog table), (g_q,k | g_p,k) for the joint
 * state and gamma_k for the normalised conditional.  Per data point r, in double:
 *     w_k = exp(lw_k - max_k lw),   W = sum_k w_k,   wn_k = w_k / W
 *     grad_x[r][d] = (sum_k w_k g_q,kd / W) / scale[d]
 *     grad_c[r][c] = (sum_k w_k gamma_kc / W) / cond_scale[c]
 * the exact gradient of L with respect to x and the raw conditional; g_p is not read (the momenta are constants of the
 * estimate).  The sums run over KEPT draws only, with the weights of the full W:
 * ff_marginal_weigh:  ff_marginal_reduce -- its lanes, units, log-sum-exp states and butterflies: out_logp and out_ess are
 *   its results bit for bit -- that also stores every row's lw_k in double (lw_out [B K]) and, once the point's merged
 *   state is in every lane, keep[r K + k] = (wn_k > 0 && wn_k >= min_weight) ? 1 : 0 with wn_k = exp(lw_k - m) / s1 in
 *   double: the rule of ff_observe_keep.  A lane re-reads only the lw_out entries it stored itself: one kernel, no fence.
 *   0 <= min_weight < 1; 0 keeps every draw of non-zero weight.  A skipped draw would have added wn_k g_k: the
 *   truncation is at most sum_skipped wn_k |g_k| <= K min_weight max |g|.  A degenerate point (a NaN among its lw, or all
 *   -inf: W = 0) keeps nothing.  z1 [B K][2 D]; out_logp [B]; out_ess [B] or NULL; lw_out [B K] double; keep [B K] int32.
 *   FF_ERR_BADARG: the cases of ff_marginal_reduce (z1 or out_logp NULL; B < 0; D < 1; K outside 1 .. 4096); lw_out or
 *   keep NULL; min_weight outside [0, 1).
 * ff_marginal_grad_reduce:  row_of [B K] int32 says where the pull-back of draw (r, k) lies: row row_of[r K + k] of
 *   gz_rows [n][2 D] and gc_rows [n][C], or < 0 for a draw that was not kept -- no row of it is read and it adds nothing (the
 *   order-preserving compaction of keep: cumsum(keep) - 1 where kept; every entry must be below n).  The q half of a gz row
 *   is read in place (row stride 2 D: no slice copy).  gc_rows may be NULL (C, cond_scale and grad_c are then ignored);
 *   scale [D] and cond_scale [C] may be NULL (1).  A lane group of lanes_per_point(K) lanes with contiguous segments of
 *   draws, as ff_observe_grad_reduce: the weights recomputed from the double lw, one block of four dimensions at a time
 *   accumulated over the lane's draws in index order and merged by the fixed butterfly, times the double 1 / W (one
 *   division per point), over scale[d] (cond_scale[c]) in double, rounded to fp32 once.  A degenerate point writes NaN to
 *   both gradients.  K = 1 with a finite lw: grad_x is the correctly rounded fp32 quotient g_q / scale (a division of two
 *   floats through double rounds once), grad_c likewise.  16-byte accesses on gz_rows (gc_rows) where they are 16-byte
 *   aligned and D % 4 == 0 (C % 4 == 0), a scalar body otherwise.
 *   FF_ERR_BADARG, before anything is enqueued: lw, row_of, gz_rows or grad_x NULL; B < 0; D < 1; K outside 1 .. 4096;
 *   gc_rows given with C < 1 or grad_c NULL.
 * A data point's results are fixed by (K, D) and its own data, not by B, its position or the launch: chunks (sample_offset
 * + first point of the chunk) and shards give bitwise the same.  DEVICE pointers, enqueued on hip_stream; B == 0 is FF_OK
 * without a launch.  The _host twins run the same header arithmetic on HOST pointers: ff_marginal_weigh_host with rows and
 * units in index order (lw agrees to double rounding; the normals through libm), ff_marginal_grad_reduce_host in the
 * device's own order of additions (given the same lw the two differ only where libm's exp and the device's differ in the
 * last bit of a double).
 */
int ff_marginal_weigh(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                      double log_det, double min_weight, float* out_logp, float* out_ess, double* lw_out, int32_t* keep,
                      void* hip_stream);
int ff_marginal_grad_reduce(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                            const float* scale, const float* cond_scale, int64_t B, int32_t D, int32_t C, int32_t K,
                            float* grad_x, float* grad_c, void* hip_stream);
int ff_marginal_weigh_host(const float* z1, int64_t B, int32_t D, int32_t K, uint64_t seed, int64_t sample_offset,
                           double log_det, double min_weight, float* out_logp, float* out_ess, double* lw_out,
                           int32_t* keep);
int ff_marginal_grad_reduce_host(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                                 const float* scale, const float* cond_scale, int64_t B, int32_t D, int32_t C, int32_t K,
                                 float* grad_x, float* grad_c);

/* ---- log-density of noisy observations over K noise draws (csrc/ff_observe.hip, csrc/ff_observe.h) ------------------
 *
 * Every log-density of the reference (ScoreModel.log_prob diffusion.py:756-815, ODEFlow.log_prob flow.py:386-438, the
 * PopulationModelDiffusion wrappers :1633, :1837) is that of an exact point.  An observation xhat = x + n with
 * n ~ N(0, diag(sigma^2)), sigma known per object and per dimension, has the convolved density
 *     p_obs(xhat | sigma) = E_{z ~ N(0, I)}[p(xhat - sigma z)]
 * These two kernels are the ends of its K-draw estimate, around ANY log-density evaluated on the B K rows between them:
 * data point r, draw k is row r K + k (the K rows of a point are contiguous), 1 <= K <= FF_MAX_OBS_DRAWS.
 *
 * ff_observe_expand:  y[r K + k][d]     = x[r][d] - noise_std[r std_row_stride + d] * z(seed, sample_offset + r, FF_OBS_NOISE_BASE + k, d)
 *                     cond_out[r K + k] = cond[r]
 *   x [B][D]; noise_std [D] (std_row_stride = 0: one vector for every row) or [B][D] (std_row_stride = D); cond [B][C] or
 *   NULL (C and cond_out are then ignored); y [B K][D]; cond_out [B K][C].  The product is rounded to fp32, then the
 *   difference is (no fused multiply-add), and z is bit for bit what ff_normal_fill writes for that noise index and global
 *   row: the result is bit for bit the torch composition `x - noise_std * z` of K such fills.  One pass, write-only
 *   beyond x, noise_std and cond; 16-byte accesses where x, noise_std, y are 16-byte aligned and D % 4 == 0 (cond,
 *   cond_out and C likewise, on their own), a scalar body with the same arithmetic in the same order otherwise.
 *   FF_ERR_BADARG: x, noise_std or y NULL; B < 0; D < 1; K outside 1 .. FF_MAX_OBS_DRAWS; std_row_stride neither 0 nor D;
 *   cond given with C < 1 or cond_out NULL.
 * ff_logmeanexp:      out[r]     = logsumexp_k lp[r K + k] - log K
 *                     out_ess[r] = (sum_k w_k)^2 / sum_k w_k^2,   w_k = exp(lp[r K + k] - max_k lp[r K + k])
 *   lp [B K]; out [B]; out_ess [B] or NULL.  The sums run in double and are rounded to fp32 once.  Non-finite input
 *   follows torch.logsumexp in float64, exactly as ff_marginal_reduce: a NaN in any lp gives NaN, all -inf gives -inf
 *   (and an effective sample size of NaN: no draw has weight), a +inf gives +inf.  At K = 1 out[r] is lp[r] bit for bit.
 *   FF_ERR_BADARG: lp or out NULL; B < 0; K outside 1 .. FF_MAX_OBS_DRAWS.
 * A data point's results do not depend on B, on its position in the batch or on the launch geometry, so a batch may be
 * processed in chunks (sample_offset + first point of the chunk) or sharded over ranks with bitwise the same results.
 * All pointers are DEVICE pointers; both enqueue on hip_stream; B == 0 is FF_OK without a launch.  The _host twins run
 * the same arithmetic (csrc/ff_observe.h) on HOST pointers for tests without a GPU: their normals come through libm and
 * agree with the device's to rounding, not bit for bit.
 */
/* Noise indices reserved for the K noise draws of an observation: draw k of global row g is
 * z(seed, g, FF_OBS_NOISE_BASE + k, d), k < 4096 -- a range of its own below FF_HUTCH_PROBE_NOISE_BASE, so a seed shared
 * with the Hutchinson probes of the expanded rows, a prior draw or a momentum gives unrelated noise. */
#define FF_OBS_NOISE_BASE 0xFFFB0000u
#define FF_MAX_OBS_DRAWS  4096
int ff_observe_expand(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond, int64_t B,
                      int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* y, float* cond_out,
                      void* hip_stream);
int ff_logmeanexp(const float* lp, int64_t B, int32_t K, float* out, float* out_ess, void* hip_stream);
int ff_observe_expand_host(const float* x, const float* noise_std, int32_t std_row_stride, const float* cond, int64_t B,
                           int32_t D, int32_t C, int32_t K, uint64_t seed, int64_t sample_offset, float* y,
                           float* cond_out);
int ff_logmeanexp_host(const float* lp, int64_t B, int32_t K, float* out, float* out_ess);

/* ---- posterior draws and moments from the K weighted particles of an observation (csrc/ff_observe.hip) -------------
 *
 * The K rows of a data point with weights w_k proportional to p(y_k) are a self-normalised importance sample of its
 * posterior p(x | xhat, sigma) ~ p(x) N(xhat; x, diag sigma^2).  ff_weighted_resample turns them into M multinomial
 * draws and the weighted mean and variance, per data point r, in double:
 *     w_k = exp((double)lp[r K + k] - max_k lp),   W = sum_k w_k
 *     index[r][m]     = the smallest k with sum_{j <= k} w_j > u_m W  (strict, u_m < 1: a row of weight 0 is never chosen)
 *     samples[r][m][] = y[r K + index[r][m]][], copied bit for bit
 *     mean[r][d]      = sum_k w_k y_kd / W
 *     var[r][d]       = sum_k w_k (y_kd - mean_d)^2 / W   (about the double mean, a second pass: never negative; the
 *                       weight-normalised form, no Bessel correction)
 *   y [B K][D] (the rows of ff_observe_expand, or any particles); lp [B K]; samples [B][M][D]; index [B][M]; mean, var
 *   [B][D].  Each of the four outputs may be NULL (samples and index are ignored when M == 0); mean and var are rounded to
 *   fp32 once (the double sums times the double 1 / W: one division per point).  A point is degenerate if any of its lp is NaN or +inf, or if W is 0 (all -inf): index = -1, NaN in
 *   samples, mean and var.  K = 1 with a finite lp: index 0, every sample and the mean are the row, var = 0.
 *   The uniforms of the resampling step: u_m of global row g is (word[m & 3] >> 8) * 2^-24 in [0, 1), word = the Philox4x32-10
 *   block of counter (g lo, g hi, FF_OBS_RESAMPLE_NOISE_INDEX, m >> 2) under the seed -- an index of its own below
 *   FF_OBS_NOISE_BASE, so a seed shared with the noise draws, probes, momenta or a prior gives unrelated uniforms.
 *   A data point's results are fixed by K and its own data (a group of lanes_per_point(K) lanes: contiguous segments of
 *   draws, a scan of the segment sums, the moments one block of four dimensions at a time), not by B, its position or
 *   the launch: chunks (sample_offset + first point of the chunk) and shards give bitwise the same.  16-byte accesses on
 *   y and samples where they are 16-byte aligned and D % 4 == 0, a scalar body otherwise.
 *   FF_ERR_BADARG, before anything is enqueued: y or lp NULL; B < 0; D < 1; K outside 1 .. FF_MAX_OBS_DRAWS; M outside
 *   0 .. FF_MAX_OBS_SAMPLES; all four outputs NULL.  B == 0 is FF_OK without a launch.  DEVICE pointers, enqueued on
 *   hip_stream; the _host twin runs the same header arithmetic on HOST pointers with the draws in index order (the same
 *   uniforms bit for bit; sums agree to double rounding).
 */
#define FF_OBS_RESAMPLE_NOISE_INDEX 0xFFFA0000u
#define FF_MAX_OBS_SAMPLES 4096
int ff_weighted_resample(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed,
                         int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var, void* hip_stream);
int ff_weighted_resample_host(const float* y, const float* lp, int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed,
                              int64_t sample_offset, float* samples, int32_t* index, float* mean, float* var);

/* ---- the gradient of the K-draw log-density of noisy observations (csrc/ff_observe.hip, csrc/ff_observe.h) ----------
 *
 * L[r] = logsumexp_k lp[r K + k] - log K (ff_logmeanexp) of the rows y_k = xhat - sigma z_k has dL / d lp_k = wn_k, the
 * normalised weight of draw k, so its gradients are weighted sums of the rows' own gradients g_k = grad_y lp_k, h_k =
 * grad_c lp_k (whatever computes them; the library's: ff_mlp_ode_launch_logp_grad), per data point r, in double:
 *     w_k = exp((double)lp[r K + k] - max_k lp),   W = sum_k w_k,   wn_k = w_k / W
 *     grad_x[r][d]         =  sum_k w_k g_kd / W
 *     grad_c[r][c]         =  sum_k w_k h_kc / W
 *     grad_noise_std[r][d] = -sum_k w_k z_kd g_kd / W,   z_kd = z(seed, sample_offset + r, FF_OBS_NOISE_BASE + k, d)
 * the exact gradient of L at fixed draws with respect to xhat, the conditional and sigma (per object and dimension,
 * whatever the layout of noise_std).  The sums run over KEPT draws only, with the weights of the full W:
 * ff_observe_keep:  keep[r K + k] = (wn_k > 0 && wn_k >= min_weight) ? 1 : 0, in double, W and the maximum from the
 *   running state and the butterfly of ff_logmeanexp.  0 <= min_weight < 1; 0 keeps every draw of non-zero weight.  A
 *   skipped draw would have added wn_k g_k: the truncation is at most sum_skipped wn_k |g_k| <= K min_weight max |g|.
 *   A degenerate point (a NaN or +inf among its lp, or W = 0: all -inf) keeps nothing.  lp [B K]; keep [B K] int32.
 *   FF_ERR_BADARG: lp or keep NULL; B < 0; K outside 1 .. FF_MAX_OBS_DRAWS; min_weight outside [0, 1).
 * ff_observe_grad_reduce:  row_of [B K] int32 says where the gradient row of draw (r, k) lies: row row_of[r K + k] of
 *   gx_rows [n][D] and gc_rows [n][C], or < 0 for a draw that was not kept -- no row of it is read and it adds nothing (the
 *   order-preserving compaction of keep: cumsum(keep) - 1 where kept; every entry must be below n).  gc_rows may be NULL
 *   (C and grad_c are then ignored), grad_noise_std may be NULL.  noise_std / std_row_stride are those of
 *   ff_observe_expand and are checked like them; the derivative of xhat - sigma z in sigma is -z at any sigma, so their
 *   values are not read.  A lane group of lanes_per_point(K) lanes with contiguous segments of draws, as
 *   ff_weighted_resample: the weights recomputed from lp, one block of four dimensions at a time accumulated over the
 *   lane's draws in index order and merged by the fixed butterfly, times the double 1 / W (one division per point),
 *   rounded to fp32 once.  A degenerate point writes NaN to its three gradients.  K = 1 with a finite lp: grad_x and
 *   grad_c are the row bit for bit, grad_noise_std is -z g rounded once.  16-byte accesses on gx_rows (gc_rows) where
 *   they are 16-byte aligned and D % 4 == 0 (C % 4 == 0), a scalar body otherwise.
 *   FF_ERR_BADARG, before anything is enqueued: lp, row_of, gx_rows, noise_std or grad_x NULL; B < 0; D < 1; K outside
 *   1 .. FF_MAX_OBS_DRAWS; std_row_stride neither 0 nor D; gc_rows given with C < 1 or grad_c NULL.
 * A data point's results are fixed by K and its own data, not by B, its position or the launch: chunks (sample_offset +
 * first point of the chunk) and shards give bitwise the same.  DEVICE pointers, enqueued on hip_stream; B == 0 is FF_OK
 * without a launch.  The _host twins run the same header arithmetic on HOST pointers with the draws in index order (sums
 * agree to double rounding; the normals through libm).
 */
int ff_observe_keep(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep, void* hip_stream);
int ff_observe_grad_reduce(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows,
                           const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K,
                           uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std,
                           void* hip_stream);
int ff_observe_keep_host(const float* lp, int64_t B, int32_t K, double min_weight, int32_t* keep);
int ff_observe_grad_reduce_host(const float* lp, const int32_t* row_of, const float* gx_rows, const float* gc_rows,
                                const float* noise_std, int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K,
                                uint64_t seed, int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std);

/* ---- marginal log-density of NOISY observations under a symplectic flow, and its gradient ----------------------------
 * (csrc/ff_marginal_observe.hip, csrc/ff_marginal_observe.h)
 *
 * An observation xhat = x + n, n ~ N(0, diag(sigma^2)), of a symplectic flow, whose own density is a marginal over the
 * momentum.  The flow preserves volume in [q | p], so with JOINT draws (z_k, p_k) per data point
 *     p_obs(xhat | sigma) = E_{z, p}[N(Phi(z0)) / N(p)] / prod scale,   z0 = [((xhat - sigma z) - shift) / scale | p]
 *     lw_k = log N(z1_k) - log N(p_k),   L[r] = logsumexp_k lw_k - log K - sum log scale
 * Both draws of (r, k) are keyed by the seed and the GLOBAL row g = sample_offset + r: the noise under the noise index
 * FF_OBS_NOISE_BASE + k, the momentum under FF_MOMENTUM_NOISE_BASE + k.  L[r] is what ff_marginal_reduce / ff_marginal_weigh
 * compute on such rows (they regenerate p_k under the same keys); these two kernels are the other two ends.
 * 1 <= K <= 4096 (FF_MAX_OBS_DRAWS and the momentum range alike).
 *
 * ff_marginal_observe_expand:  t = fl(noise_std[r std_row_stride + d] * z_kd),  y = fl(x[r][d] - t)      (no fused multiply-add)
 *                              z0[r K + k][0 : D]   = fl(fl(y - shift[d]) / scale[d])
 *                              z0[r K + k][D : 2 D] = z(seed, sample_offset + r, FF_MOMENTUM_NOISE_BASE + k, d)
 *                              cond_out[r K + k]    = cond[r]
 *   y is bit for bit ff_observe_expand's row, the q half ff_marginal_expand's formula applied to it, the p half and cond_out
 *   bit for bit ff_marginal_expand(x, K)'s; with noise_std = 0 the whole output is ff_marginal_expand(x, K)'s.  (The
 *   composition ff_observe_expand -> ff_marginal_expand(K = 1) keys every momentum by the EXPANDED row instead.)
 *   x [B][D]; noise_std [D] (std_row_stride = 0) or [B][D] (std_row_stride = D); shift, scale [D] or NULL; cond [B][C] or
 *   NULL (C and cond_out are then ignored); z0 [B K][2 D]; cond_out [B K][C].  One pass, write-only beyond x, noise_std and
 *   cond; 16-byte accesses where x, noise_std, z0 are 16-byte aligned and D % 4 == 0 (cond, cond_out and C likewise, on
 *   their own), a scalar body with the same arithmetic in the same order otherwise.
 *   FF_ERR_BADARG, before anything is enqueued: the cases of both parents -- x, noise_std or z0 NULL; B < 0; D < 1; K
 *   outside 1 .. 4096; std_row_stride neither 0 nor D; cond given with C < 1 or cond_out NULL.
 * ff_marginal_observe_grad_reduce:  ff_marginal_grad_reduce -- its lanes, segments, order of additions and butterfly: grad_x
 *   and grad_c are its results bit for bit on the same inputs -- that in the same pass forms
 *     grad_noise_std[r][d] = -(sum_kept w_k z_kd g_q,kd / W) / scale[d],   z_kd = z(seed, sample_offset + r, FF_OBS_NOISE_BASE + k, d)
 *   the gradient of L with respect to sigma, per object and dimension whatever the layout of noise_std (dq0 / d sigma =
 *   -z / scale at any sigma: the values of noise_std are not read, only checked as ff_observe_grad_reduce checks them).  z is
 *   regenerated from the stream; the product z g (exact) and the sums are in double, the result is rounded to fp32 once.  A
 *   skipped draw's row is never read.  grad_noise_std may be NULL; gc_rows may be NULL (C, cond_scale and grad_c are then
 *   ignored); scale and cond_scale may be NULL (1).  A degenerate point (a NaN among its lw, or all -inf) writes NaN to all
 *   three gradients.  K = 1 with a finite lw: grad_noise_std is -z g / scale rounded once.
 *   FF_ERR_BADARG, before anything is enqueued: lw, row_of, gz_rows, noise_std or grad_x NULL; B < 0; D < 1; K outside
 *   1 .. 4096; std_row_stride neither 0 nor D; gc_rows given with C < 1 or grad_c NULL.
 * A data point's results are fixed by (K, D) and its own data, not by B, its position or the launch: chunks (sample_offset
 * + first point of the chunk) and shards give bitwise the same.  DEVICE pointers, enqueued on hip_stream; B == 0 is FF_OK
 * without a launch.  The _host twins run the same header arithmetic on HOST pointers: the normals through libm (they agree
 * with the device's to rounding, not bit for bit), ff_marginal_observe_grad_reduce_host in the device's own order of
 * additions, as ff_marginal_grad_reduce_host.
 */
int ff_marginal_observe_expand(const float* x, const float* noise_std, int32_t std_row_stride, const float* shift,
                               const float* scale, const float* cond, int64_t B, int32_t D, int32_t C, int32_t K,
                               uint64_t seed, int64_t sample_offset, float* z0, float* cond_out, void* hip_stream);
int ff_marginal_observe_grad_reduce(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                                    const float* scale, const float* cond_scale, const float* noise_std,
                                    int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed,
                                    int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std,
                                    void* hip_stream);
int ff_marginal_observe_expand_host(const float* x, const float* noise_std, int32_t std_row_stride, const float* shift,
                                    const float* scale, const float* cond, int64_t B, int32_t D, int32_t C, int32_t K,
                                    uint64_t seed, int64_t sample_offset, float* z0, float* cond_out);
int ff_marginal_observe_grad_reduce_host(const double* lw, const int32_t* row_of, const float* gz_rows, const float* gc_rows,
                                         const float* scale, const float* cond_scale, const float* noise_std,
                                         int32_t std_row_stride, int64_t B, int32_t D, int32_t C, int32_t K, uint64_t seed,
                                         int64_t sample_offset, float* grad_x, float* grad_c, float* grad_noise_std);

/* ---- per-object posteriors from the K joint draws of the noisy marginal --------------------------------------------------
 * (csrc/ff_marginal_posterior.hip, csrc/ff_marginal_posterior.h)
 *
 * The joint draw (z_k, p_k) of data point r carries the weight w_k = N(z1_k) / N(p_k) = exp(lw_k): the flow preserves volume,
 * so w_k is an unbiased one-momentum estimate of p(xhat - sigma z_k), and the K candidates y_k = xhat - sigma z_k with these
 * weights are a pseudo-marginal, self-normalised importance sample of p(x | xhat, sigma) ~ p(x) N(xhat; x, diag sigma^2).
 * ff_marginal_observe_resample is ff_weighted_resample on them, with two differences: the log-weights are the DOUBLE lw of
 * ff_marginal_weigh, and there is no particle buffer -- every candidate is regenerated from the counter-based stream where
 * it is needed, as ff_marginal_observe_grad_reduce regenerates z.  Per data point r, in double:
 *     w_k = exp(lw[r K + k] - max_k lw)  (1 for the maximum itself),   W = sum_k w_k
 *     y_k[d]          = fl(x[r][d] - fl(noise_std[r std_row_stride + d] * z_kd)),
 *                       z_kd = z(seed, sample_offset + r, FF_OBS_NOISE_BASE + k, d): bit for bit ff_observe_expand's row
 *     index[r][m]     = the smallest k of positive weight with sum_{j <= k} w_j > u_m W  (strict; u_m of
 *                       ff_weighted_resample: FF_OBS_RESAMPLE_NOISE_INDEX, global row sample_offset + r)
 *     samples[r][m][] = y_index[r][m], regenerated, in the units of x
 *     mean[r][d]      = sum_k w_k y_kd / W
 *     var[r][d]       = sum_k w_k (y_kd - mean_d)^2 / W   (about the double mean, a second pass: never negative)
 *   x [B][D]; noise_std [D] (std_row_stride = 0) or [B][D] (std_row_stride = D); lw [B K] double; samples [B][M][D]; index
 *   [B][M]; mean, var [B][D].  Each of the four outputs may be NULL (samples and index are ignored when M == 0); mean and var
 *   are rounded to fp32 once (the double sums times the double 1 / W: one division per point).  The lanes, segments, scan,
 *   targets, fallback and order of additions are ff_weighted_resample's: given the same particles and weights (lw that fp32
 *   holds exactly, y = ff_observe_expand's rows) all four outputs are its results bit for bit.  A point is degenerate if any
 *   of its lw is NaN, or if none is above -inf: index = -1, NaN in samples, mean and var.  K = 1 with a finite lw: index 0,
 *   every sample and the mean are y_0, var = 0.  16-byte stores on samples where it is 16-byte aligned and D % 4 == 0 (x and
 *   noise_std are read likewise, on their own), a scalar body with the same arithmetic otherwise.
 *   FF_ERR_BADARG, before anything is enqueued: x, noise_std or lw NULL; B < 0; D < 1; K outside 1 .. 4096; M outside
 *   0 .. FF_MAX_OBS_SAMPLES; std_row_stride neither 0 nor D; all four outputs NULL.  B == 0 is FF_OK without a launch.
 * A data point's results are fixed by (K, D) and its own data, not by B, its position or the launch: chunks (sample_offset
 * + first point of the chunk) and shards give bitwise the same.  DEVICE pointers, enqueued on hip_stream; the _host twin runs
 * the same header arithmetic on HOST pointers with the draws in index order (the same uniforms bit for bit; the normals
 * through libm; sums agree to double rounding).
 */
int ff_marginal_observe_resample(const float* x, const float* noise_std, int32_t std_row_stride, const double* lw,
                                 int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed, int64_t sample_offset,
                                 float* samples, int32_t* index, float* mean, float* var, void* hip_stream);
int ff_marginal_observe_resample_host(const float* x, const float* noise_std, int32_t std_row_stride, const double* lw,
                                      int64_t B, int32_t D, int32_t K, int32_t M, uint64_t seed, int64_t sample_offset,
                                      float* samples, int32_t* index, float* mean, float* var);

/* ---- Hutch++ / XTrace divergence estimates from recorded Jacobians (csrc/ff_trace.hip, csrc/ff_trace_est.h) ----
 *
 * Replaces the two estimator branches of ScoreModel.forward, diffusion.py:336-400 (Hutch++) and :402-481 (XTrace), for
 * every right-hand-side evaluation of a launch at once: with ff_ode_args.jac_all = 1 a fused FF_MODE_EXACT launch leaves
 * A[e][b] = J^T of every evaluation row e and sample b; one launch of this kernel returns the estimates
 *     out[e][b] = hutchpp(A[e][b]; S[:, b], G[:, b])   or   xtrace(A[e][b]; O[:, b])
 * with the probes laid out as the reference stores them ([n_probes][batch][dim], entries +-1; drawn once per solve,
 * diffusion.py:703-719).  The QR behind both is LAPACK's Householder scheme, what `torch.linalg.qr` (:378, :441) runs on
 * the reference's CPU path.  All pointers are DEVICE pointers (HOST pointers for ff_trace_estimate_host).
 */
#define FF_TRACE_HUTCHPP 1
#define FF_TRACE_XTRACE  2
typedef struct ff_trace_args {
    int32_t kind;            /* FF_TRACE_*                                                                     */
    int32_t dim;             /* D                                                                               */
    int32_t n_rows;          /* evaluation rows recorded in `jac`                                               */
    int32_t r;               /* Hutch++: sketch probes S (`hpp_rank`, <= D); XTrace: probes O (`xt_vecs`, <= D)  */
    int32_t m;               /* Hutch++: residual probes G (`hpp_vecs`, >= 1); XTrace: unused                   */
    int32_t reserved;
    int64_t batch;
    const float* jac;        /* [n_rows][batch][D][D]: row j of a matrix is J^T e_j (ff_ode_args.jac_out)        */
    const float* probes0;    /* S or O: [r][batch][D]                                                           */
    const float* probes1;    /* G: [m][batch][D], or NULL (XTrace)                                              */
    float*       out;        /* [n_rows][batch]                                                                 */
    float*       workspace;  /* ff_trace_workspace_floats(kind, dim, r, n_rows * batch) floats                   */
    const int32_t* gate;     /* optional DEVICE word: 0 = the launch does nothing (see ff_ode_args.gate)         */
} ff_trace_args;
size_t ff_trace_workspace_floats(int32_t kind, int32_t dim, int32_t r, int64_t items);
int ff_trace_estimate(const ff_trace_args* args, void* hip_stream);
/* The same arithmetic on the HOST (tests without a GPU): HOST pointers; `workspace` holds
 * ff_trace_workspace_floats(kind, dim, r, 1) floats; `gate` is ignored. */
int ff_trace_estimate_host(const ff_trace_args* args);

/* ---- the same estimates from J^T v PRODUCTS (csrc/ff_trace_prod.hip, csrc/ff_trace_prod.h) -------------------------------
 *
 * The reference computes both estimators from 2r + m (Hutch++) or 2m (XTrace) reverse-mode products per right-hand side
 * (diffusion.py:356-398, :419-455).  With ff_mlp_ode_launch_vjp supplying the products A v = a v + b J_net^T v of every
 * evaluation row, an estimate takes two sweeps and two streaming launches, and no Jacobian is recorded:
 *     sweep 1           y[e][b][c][:]    = A(y_e) p_c                     p = S (Hutch++, r columns) or O (XTrace, r columns)
 *     ff_trace_basis    Q = thin_qr(y[e][b]) -- the QR of ff_trace_estimate -- and
 *                       basis[e][b] = [q_0 .. q_{r-1} | u_0 .. u_{m-1}],  u_g = g - Q (Q^T g)      Hutch++, K2 = r + m
 *                       basis[e][b] = [q_0 .. q_{r-1}],  rfac[e][b] = R                             XTrace,  K2 = r
 *     sweep 2           prod[e][b][c][:] = A(y_e) basis[e][b][c]
 *     ff_trace_combine  out[e][b] = the estimate of :381-400 from (Q, U, AQ, AU), or of :451-481 from (Q, R, O, AQ)
 * in the fp32 operation order of ff_trace_estimate with every product read instead of summed.  One work item per
 * (row, sample); plain global-memory kernels (an item moves K2 * D floats, not D * D).  All pointers are DEVICE pointers
 * (HOST pointers for the _host twins, tests without a GPU: `workspace` then holds one item's floats, `gate` is ignored).
 * FF_ERR_BADARG: a kind other than FF_TRACE_*, dim < 1, r < 1 or r > dim, Hutch++ with m < 1 or no probes1, XTrace without
 * rfac, a NULL probes0 / basis / workspace, ff_trace_basis without y, ff_trace_combine without prod or out. */
typedef struct ff_trace_prod_args {
    int32_t kind;            /* FF_TRACE_*                                                                     */
    int32_t dim;             /* D                                                                               */
    int32_t n_rows;          /* evaluation rows                                                                 */
    int32_t r;               /* Hutch++: sketch probes S (`hpp_rank`, <= D); XTrace: probes O (`xt_vecs`, <= D)  */
    int32_t m;               /* Hutch++: residual probes G (`hpp_vecs`, >= 1); XTrace: unused                   */
    int32_t reserved;
    int64_t batch;
    const float* probes0;    /* S or O: [r][batch][D]                                                           */
    const float* probes1;    /* G: [m][batch][D], or NULL (XTrace)                                              */
    const float* y;          /* [n_rows][batch][r][D]   sweep 1's products          (ff_trace_basis)            */
    float*       basis;      /* [n_rows][batch][K2][D]  written by ff_trace_basis, read by ff_trace_combine     */
    float*       rfac;       /* [n_rows][batch][r][r]   XTrace: R, likewise; Hutch++: NULL                      */
    const float* prod;       /* [n_rows][batch][K2][D]  sweep 2's products          (ff_trace_combine)          */
    float*       out;        /* [n_rows][batch]                                     (ff_trace_combine)          */
    float*       workspace;  /* ff_trace_prod_workspace_floats(kind, dim, r, n_rows * batch) floats              */
    const int32_t* gate;     /* optional DEVICE word: 0 = the launch does nothing (see ff_ode_args.gate)         */
} ff_trace_prod_args;
size_t ff_trace_prod_workspace_floats(int32_t kind, int32_t dim, int32_t r, int64_t items);
int ff_trace_basis(const ff_trace_prod_args* args, void* hip_stream);
int ff_trace_combine(const ff_trace_prod_args* args, void* hip_stream);
int ff_trace_basis_host(const ff_trace_prod_args* args);
int ff_trace_combine_host(const ff_trace_prod_args* args);

/* ---- adaptive embedded Runge-Kutta solves with the step control ON THE DEVICE (csrc/ff_adaptive.hip) ---------
 *
 * Replaces `odeint(func, state, t, method="dopri5" | "bosh3" | "fehlberg2" | "adaptive_heun", rtol=, atol=, options=)`
 * -- the reference's DEFAULT solver at every call site (diffusion.py:572,631-639; 649,744-752; 762; flow.py:299-303,
 * 313,371-382) -- including torchdiffeq's batch-global step control: `_select_initial_step`, `_compute_error_ratio`
 * (mixed norm over the tuple state), accept / reject, `_optimal_step_size`, min / max step clamps, the fourth-order dense
 * output at t[-1].  One attempted step is three launches enqueued back to back with NO host round trip:
 *     the fused attempt (ff_mlp_ode_launch semantics, gated by ff_adapt_state.active)
 *  -> norms + controller (one reduction launch; its last block decides, advances (t, dt) and writes the NEXT attempt's
 *     evaluation rows: stage times, the SDE schedule scalars a_e / b_e and the first-layer time part c1_e, computed in
 *     fp32 in the reference's operation order: diffusion.py:276-278,905,1131,1316; MLP.forward :109-113; flow.py:112-118)
 *  -> commit (an accepted step's (y1, f1, lp1, fl1) become the current state).
 * The host enqueues a chunk of attempts, then reads ff_adapt_state once; attempts behind the end of the solve are no-ops.
 */
#define FF_SCHED_FLOW   0   /* flows: a = 0, b = 1, c1 = w_t t + b1 (flow.py:112-118)                       */
#define FF_SCHED_VE     1   /* VESDE (diffusion.py:818-1003):    p = {sigma_min, sigma_max, T}               */
#define FF_SCHED_VP     2   /* VPSDE (diffusion.py:1006-1180):   p = {beta_min, beta_max, T}                 */
#define FF_SCHED_SUBVP  3   /* SUBVPSDE (diffusion.py:1183-1366): p = {beta_min, beta_max, T}                */
#define FF_SCHED_FOURIER 4  /* a = 0, b = 1, c1 = [sin | cos] Fourier features through w0t + b0 (symplectic.py:98-99);
                               a pair plan takes w0t / b0 stacked as [net A rows | pad | net B rows | pad], h_real = 2 width */

#define FF_ADAPT_OK            0
#define FF_ADAPT_ERR_UNDERFLOW 1   /* torchdiffeq: AssertionError "underflow in dt {dt}" (state.dt holds it)   */
#define FF_ADAPT_ERR_NONFINITE 2   /* torchdiffeq: "non-finite values in state `y`"                            */
#define FF_ADAPT_ERR_MAXSTEPS  3   /* torchdiffeq: "max_num_steps exceeded"                                     */

#define FF_ADAPT_MAX_PASSES    8   /* unit-tangent passes of one attempt (FF_MODE_EXACT with dim + 1 > tile)    */

/* Controller state: 128 bytes of DEVICE memory, written by the controller, read back by the host. */
typedef struct ff_adapt_state {
    double  t;           /* solver time reached: the end of the last accepted step (rk_state.t1)            */
    double  dt;          /* step of the next attempt (clamped to [min_step, max_step])                      */
    double  t_prev;      /* start of the last accepted step (rk_state.t0)                                   */
    double  dt_prev;     /* its length                                                                      */
    double  t_end;       /* where the solve stops (solver time: a decreasing span is solved negated)        */
    double  h0;          /* initial-step rule: the trial step                                               */
    double  d0;          /* ... the norm of the scaled state                                                */
    double  d1;          /* ... the norm of the scaled derivative                                           */
    int32_t active;      /* gate of the launches that follow: 1 = attempts run                              */
    int32_t commit;      /* 1 = the latest attempt was accepted and is not the last: commit adopts it       */
    int32_t done;        /* the solve reached t_end: the buffers hold the last accepted step                */
    int32_t error;       /* FF_ADAPT_ERR_*                                                                  */
    int32_t n_attempts;
    int32_t n_accepted;
    int32_t n_steps;     /* loop iterations (torchdiffeq counts them against max_num_steps)                 */
    int32_t reserved0;
    float   last_ratio;  /* error ratio of the latest attempt                                               */
    float   reserved1[7];
} ff_adapt_state;

/* The embedded pair, the tolerances and the time-dependent part of the right-hand side (HOST struct). */
typedef struct ff_adapt_config {
    int32_t n_stages;    /* stages including the first-same-as-last one, 2 .. FF_MAX_SLOTS                  */
    int32_t order;       /* order of the pair (torchdiffeq `order`): dopri5 5, bosh3 3, fehlberg2 / adaptive_heun 2 */
    float   alpha[FF_MAX_SLOTS - 1];        /* stage i + 1 sits at t0 + alpha[i] dt (exactly t1 when alpha[i] == 1) */
    float   beta[FF_MAX_SLOTS - 1][8];      /* ... on y0 + dt sum_j beta[i][j] k_j                           */
    float   c_sol[8];    /* y1 = y0 + dt sum_j c_sol[j] k_j                                                 */
    float   c_mid[8];    /* dense-output midpoint                                                           */
    float   c_err[8];    /* error estimate                                                                  */
    float   rtol, atol;
    double  min_step, max_step;             /* torchdiffeq options (0, +inf by default)                      */
    double  first_step;  /* option first_step; NaN = torchdiffeq's `_select_initial_step`                   */
    int32_t max_num_steps;
    int32_t sched;       /* FF_SCHED_*                                                                      */
    int32_t no_sigma;    /* ScoreModel(no_sigma=): the network output is NOT divided by sigma(t) (diffusion.py:268-272) */
    float   sign;        /* +1, or -1 for a decreasing span (solved in -t with the right-hand side negated)  */
    double  p[4];        /* schedule parameters (FF_SCHED_*)                                                */
    const float* emb_w;  /* DEVICE [n_emb]: Gaussian-Fourier frequencies W (MLP.W, diffusion.py:73-76); NULL for flows */
    int32_t n_emb;
    float   pi;          /* MLP.pi as the model holds it (fp32)                                             */
    const float* w0t;    /* DEVICE [h_real][n_tcols]: the first layer's time columns ([sin | cos] features, or the
                            single t column of a flow), row-major                                           */
    const float* b0;     /* DEVICE [h_real]: the first layer's bias                                         */
    int32_t h_real;      /* rows of the first layer (<= plan.width; c1 is zero-padded to the width)          */
    int32_t n_tcols;     /* 2 * n_emb, or 1 for flows                                                        */
} ff_adapt_config;

/* Work buffers (all DEVICE memory owned by the caller; [B] = batch, [B, D] = batch x dim floats). */
typedef struct ff_adapt_buffers {
    float* y;            /* [B, D] in: the initial state; during the solve: the current state               */
    float* f0;           /* [B, D] derivative at the current state (FSAL)                                   */
    float* lp;           /* [B]    integrated divergence (modes 1, 2; in: its initial value) or NULL        */
    float* fl0;          /* [B]    its derivative or NULL                                                   */
    float* aux[FF_MAX_AUX];      /* [B, D] each: proposal y1, last stage f1, dense-output midpoint, error estimate */
    float* aux_lp[FF_MAX_AUX];   /* [B] each, or NULL                                                       */
    float* aux_lp_pass;  /* [n_passes][FF_MAX_AUX][B] partial divergences when n_passes > 1, else NULL      */
    float* scratch_x;    /* [B, D]                                                                          */
    float* scratch_lp;   /* [B] or NULL                                                                     */
    float* etab;         /* [FF_MAX_SLOTS + 1][FF_ROW_HDR + plan.width] evaluation rows, written by the controller */
    float* out_y;        /* [B, D] the solution at t_end (dense output of the last step)                    */
    float* out_lp;       /* [B] or NULL                                                                     */
    ff_adapt_state* state;
    void*  norm_workspace;       /* ff_scaled_rms_workspace_bytes() bytes, first 16 zero                    */
    const float* norm_only[2];   /* components the reference carries in the solver state with a zero derivative (the raw */
    int64_t norm_only_n[2];      /* `conditional` of ConditionalODEFlow, flow.py:779-796): they enter d0 of the initial step */
    int32_t n_passes;            /* 1, or the unit-tangent passes of FF_MODE_EXACT                          */
    int32_t pass_first[FF_ADAPT_MAX_PASSES];
    int32_t pass_count[FF_ADAPT_MAX_PASSES];
    /* Step control over SEVERAL shards of one batch (one process per GPU).  torchdiffeq's norms are over the whole batch
     * it is handed (one step size for all samples), so when the batch is cut over ranks the sums of squares behind every
     * norm have to meet: the one exchange step of this path.  With `exchange` set each norm is taken in two launches --
     * reduce into exchange_sums (FF_EXCHANGE_DOUBLES doubles: FF_NORM_TERMS sums of squares, the count of non-finite
     * values, FF_NORM_TERMS element counts, one spare), then the controller -- and `exchange(exchange_user, hip_stream)`
     * is called on the HOST in between: it must ENQUEUE, ordered with hip_stream, an in-place sum of those doubles over
     * all ranks (an RCCL all-reduce) and return 0; every rank then takes the same decisions and attempts the same number
     * of steps.  NULL: the norms are over this call's batch. */
    double* exchange_sums;
    int (*exchange)(void* user, void* hip_stream);
    void* exchange_user;
    /* Divergence by a Hutch++ / XTrace ESTIMATE instead of the exact trace (ScoreModel(hutchpp=True) / (xtrace=True),
     * diffusion.py:336-481; FF_MODE_EXACT only).  The state never depends on the divergence, so an attempted step stays
     * the fused launch(es) of the exact trace -- now recording the Jacobian of every evaluation row into est_jac -- followed
     * by ONE ff_trace_estimate launch over all rows and one launch that combines the rows' estimates with the attempt's
     * tail coefficients into aux_lp[0..3] (proposal, last stage, midpoint, error estimate), the same linear combinations
     * the fused kernel takes of its own divergence slots.  est_kind = 0: the exact trace. */
    int32_t est_kind;            /* 0 or FF_TRACE_*                                                          */
    int32_t est_r, est_m;        /* ff_trace_args.r / .m                                                     */
    int32_t est_reserved;
    const float* est_probes0;    /* ff_trace_args.probes0 / probes1                                          */
    const float* est_probes1;
    float* est_jac;              /* [n_stages - 1][B][D][D]                                                  */
    float* est_div;              /* [n_stages - 1][B]                                                        */
    float* est_workspace;        /* ff_trace_workspace_floats(est_kind, D, est_r, (n_stages - 1) * B) floats  */
} ff_adapt_buffers;
#define FF_EXCHANGE_DOUBLES 8

#define FF_ADAPT_START   1   /* initialise the state, evaluate f(t0, y), choose the first step              */
#define FF_ADAPT_FINISH  2   /* evaluate the dense output at t_end into out_y / out_lp (a no-op until done)  */

/*
 * Enqueue on hip_stream: [FF_ADAPT_START:] the start-up launches, then `n_attempts` attempted steps, then
 * [FF_ADAPT_FINISH:] the dense output.  `base` supplies cond / probe / wpack / mode / batch (its state, table, aux and
 * adaptive fields are ignored).  t0 / t_end are solver times (already negated for a decreasing span) and only read with
 * FF_ADAPT_START.  Nothing is read back: the caller copies *buffers->state to the host when it wants to know (done,
 * error, counters) and calls again with what = 0 or FF_ADAPT_FINISH while `done` and `error` are both zero.
 */
int ff_mlp_ode_adaptive(const ff_mlp_plan_t* plan, const ff_ode_args* base, const ff_adapt_config* config,
                        const ff_adapt_buffers* buffers, double t0, double t_end, int32_t what, int32_t n_attempts,
                        void* hip_stream);

/* The controller's arithmetic on the HOST (tests without a GPU): one evaluation row for real time `t_real` -- a_e, b_e
 * (already multiplied by config->sign) and c1[config->h_real] -- with emb_w / w0t / b0 read as HOST pointers. */
int ff_adapt_host_row(const ff_adapt_config* config, float t_real, float* a_out, float* b_out, float* c1_out);
/* ... and one controller transition: `phase` 1 = after the initial-step norms d0 (norms[0]) and d1 (norms[1]), 2 = after
 * d2 (norms[0] = the unscaled norm), 3 = after an attempted step (norms[0] = error ratio, norms[1] != 0: non-finite y1),
 * 4 = first_step given.  Updates *state; returns 1 if an attempt must follow. */
int ff_adapt_host_transition(const ff_adapt_config* config, ff_adapt_state* state, int32_t phase, const float* norms);

#ifdef __cplusplus
}
#endif
#endif /* FLOWFUSION_AMD_H */
