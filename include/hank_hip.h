/*
 * hank_hip.h — C ABI of the MI355X-native household block (the sequence-space JVP hot path).
 *
 * The reference (vasudeva-ram/Julia-NewtonRaphsonHANK) has no FFI; its boundary for this path is a
 * set of Julia call signatures. Each entry point below names the reference interface it replaces;
 * the Julia `ccall` shims that keep those signatures are in INTEGRATION.md / julia/HankHIP.jl.
 *
 * Conventions (all of them the reference's own):
 *   - every array is fp64, column-major; policy / value / distribution matrices are n_a x n_e
 *     with wealth fastest (ForwardIteration.jl:6-10); G = n_a*n_e; P = T-1 transition periods.
 *   - Pi is the row-stochastic productivity transition, column-major: Pi[e + n_e*e2] = P(e -> e2)
 *     (GeneralStructures.jl:500-525; used as V'*Pi' backward, KrusellSmith.jl:59, and D*Pi forward,
 *     ForwardIteration.jl:280-284).
 *   - "xhh" are the per-period household inputs the value function reads from xVals; for the
 *     Krusell-Smith plugin that is (r_t, w_t) (KrusellSmith.jl:53-54): xhh[k + n_hh*t], n_hh = 2
 *     (3 for the one-asset HANK family: (r_t, w_t, tr_t)); hank_n_hh() tells.
 *   - tangent batches are Julia-natural: dxhh is (n_hh, P, N) column-major, dagg is (P, N).
 *   - the caller owns every host buffer; the library copies in/out and retains no pointer past a
 *     call; the context owns all device memory. A context is bound to ONE HIP device (hank_create:
 *     the current one; hank_create_on: the one named), is not thread-safe, and host-pointer calls are synchronous on return.
 *   - every function returns a status (0 = ok). Julia exceptions on this path become codes:
 *     hank_last_error() carries the message the shim turns back into error(...).
 *
 * There is NO CPU fallback: every entry point fails with HANK_ERR_NO_DEVICE when no gfx950 device
 * is usable.
 */
#ifndef HANK_HIP_H
#define HANK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hank_ctx hank_ctx;

enum {
    HANK_OK = 0,
    HANK_ERR_NO_DEVICE = 1,   /* no usable HIP device / HIP runtime error                          */
    HANK_ERR_BAD_ARG = 2,     /* shape / argument errors (error(...) in the Julia callers)         */
    HANK_ERR_KNOTS = 3,       /* Interpolations.jl: knot-vectors must be unique and sorted
                                 (KrusellSmith.jl:69-72; acknowledged at SteadyState.jl:129-131)   */
    HANK_ERR_DOMAIN = 4,      /* Julia DomainError: negative base under a non-integer power
                                 (KrusellSmith.jl:59, :80)                                         */
    HANK_ERR_NOT_READY = 5,   /* boundary / primal not set before a dependent call                 */
    HANK_ERR_NONMONOTONE = 6, /* savings policy not monotone in wealth (cannot happen when the
                                 knots check passes; guards the segmented Young push-forward)      */
    HANK_ERR_NOMEM = 7,
    HANK_ERR_SWEEP = 8,       /* a persistent sweep could not form its workgroup groups or a wait in it timed out (every wait
                                 is bounded in time: 20 ms, HANK_XWAIT_MS at hank_create; the message says how long it
                                 waited); host-pointer entries fall back to the per-period launches by themselves. The
                                 persistent sweeps assume the process has the GPU to itself          */
    HANK_ERR_LAUNCH = 9       /* a kernel launch / graph / copy was refused by the HIP runtime (the message names it)   */
};

/* value-function families resolved from the YAML `function:` name (KrusellSmith.yaml:86,
 * ModelParser.jl:338-342 / _lookup_fn :404-413). */
enum {
    HANK_VF_KRUSELL_SMITH = 0,  /* KrusellSmith.jl:43-83; household inputs (r_t, w_t)                                  */
    HANK_VF_ONE_ASSET_HANK = 1  /* the same EGM step with a lump-sum transfer: inputs (r_t, w_t, tr_t), cash on hand
                                   (1+r) a + w z_e + tr. NOT in the reference: parity unpinned     */
};

/* The model-side constants BackwardIteration/ForwardIteration read from `model::SequenceModel`
 * (GeneralStructures.jl:216-226): heterogeneity grids + params + compspec.T. */
typedef struct {
    int32_t n_a;         /* model.heterogeneity.wealth.n                                          */
    int32_t n_e;         /* model.heterogeneity.productivity.n                                    */
    int32_t T;           /* model.compspec.T ; P = T-1 periods are solved                         */
    int32_t value_fn_id; /* HANK_VF_*                                                             */
    const double *a_grid; /* [n_a] wealth grid, strictly increasing                                */
    const double *z_grid; /* [n_e] productivity grid                                               */
    const double *Pi;     /* [n_e*n_e] column-major row-stochastic                                 */
    double beta, gamma, borrow_cons; /* model.params.β, γ, borrow_cons (KrusellSmith.jl:52)        */
} hank_model;

/* ---- lifetime ------------------------------------------------------------------------------- */
int hank_create(const hank_model *model, hank_ctx **out);   /* on the calling thread's current HIP device */
/* The same on HIP device `device` (0 .. hipGetDeviceCount-1). The reference has no notion of a device: `JVP(func, primal,
 * tangent)` (GeneralStructures.jl:542-550) is linear in `tangent`, so the columns of a tangent batch (the Jacobian
 * columns of SteadyStateJacobian.jl:240-243, ForwardDiff's chunks) shard over one context per GPU of a node; every entry
 * point makes its context's device current for the call and restores the caller's, so ONE host thread can keep all of a
 * node's contexts busy through the *_dev entries ("one process, eight GPUs"). */
int hank_create_on(const hank_model *model, int32_t device, hank_ctx **out);
/* hank_gather_columns: a tangent batch sharded by columns over one context per GPU (hank_create_on), assembled in ONE GPU's memory
 * over xGMI — what a single-process host (the Julia reference is one) needs in place of the RCCL all-gather of the one-process-per-
 * GPU form; `JVP(func, primal, tangent)` (GeneralStructures.jl:542-550) is linear in `tangent`, so the columns of a batch are
 * independent. ctxs[0] receives. d_blocks[k]: device pointer on ctxs[k]'s device of its (P, N_k[k]) column-major block, as written
 * by hank_jvp_dev / hank_primal_jvp_dev on ctxs[k]; d_out: (P, sum N_k) column-major on ctxs[0]'s device, the blocks in order.
 * Asynchronous: every block is copied on its OWN context's stream behind the sweeps that produce it (hipMemcpyPeerAsync from the
 * source device, peer access enabled on first use; a plain device copy where both contexts share a device) and ctxs[0]'s stream
 * waits for all of them: hank_sync(ctxs[0]) — or work enqueued on its stream — sees the assembled matrix. */
int hank_gather_columns(hank_ctx *const *ctxs, int32_t n, const double *const *d_blocks, const int32_t *N_k, double *d_out);
int hank_destroy(hank_ctx *ctx);
const char *hank_last_error(const hank_ctx *ctx); /* never NULL; "" when the last call succeeded  */
int hank_n_hh(const hank_ctx *ctx);               /* household inputs per period (KS: 2)          */
int hank_device_available(void);                  /* 1 when the current HIP device is a usable gfx950, else 0 */

/* Use the caller's HIP stream (a hipStream_t) for everything this context enqueues; NULL restores
 * the context's own stream. */
int hank_set_stream(hank_ctx *ctx, void *hip_stream);
int hank_sync(hank_ctx *ctx);

/* ---- boundary conditions ---------------------------------------------------------------------
 * ss_end_value: terminal marginal value, `ss_end.value` (BackwardIteration.jl:85).
 * ss_init_D:    initial distribution,   `ss_initial.D`  (ForwardIteration.jl:293).             */
int hank_set_boundary(hank_ctx *ctx, const double *ss_end_value, const double *ss_init_D);

/* ---- the fused household block -----------------------------------------------------------------
 * hank_primal  ==  ForwardIteration(BackwardIteration(x, ...), ...) on Float64
 *                  (NewtonRaphson.jl:78-79 inside fullFunction, called at :91).
 *   xhh[n_hh*P] -> agg_out[P] (the aggregate of the single heterogeneous variable, KD for KS:
 *   dot(vec(policy_t), D_t) with the POST-transition D_t, ForwardIteration.jl:301-307).
 *   Also records the linearisation every later hank_jvp uses.
 * hank_jvp     ==  the partials of the same composition under Dual{Tag,Float64,N}, i.e. what
 *                  JVP(fullFunction, x, y) (GeneralStructures.jl:542-550; NewtonRaphson.jl:95)
 *                  pushes through the household block, for N tangent directions at once.
 *   dxhh (n_hh, P, N) -> dagg_out (P, N).                                                        */
int hank_primal(hank_ctx *ctx, const double *xhh, double *agg_out);
int hank_jvp(hank_ctx *ctx, const double *dxhh, int32_t N, double *dagg_out);

/* Same, with DEVICE pointers (inputs already resident in HBM); enqueued on the context's stream,
 * asynchronous: call hank_sync (or synchronise the stream) before reading the outputs.
 * hank_primal_dev reports device-side errors (knots/domain) at the next hank_check. Device pointers must belong to the
 * context's device (hank_create_on); they are not validated. */
int hank_primal_dev(hank_ctx *ctx, const double *d_xhh, double *d_agg_out);
int hank_jvp_dev(hank_ctx *ctx, const double *d_dxhh, int32_t N, double *d_dagg_out);
/* hank_check: sync + fetch the device error word of the last primal. A persistent sweep that could not run (HANK_ERR_SWEEP:
 * its groups did not form, a wait ran into its deadline) is reported here for the asynchronous entries — which cannot re-run
 * a call — ONCE: a context whose schedule was not forced (HANK_SCHEDULE) continues on the per-period launches, so the caller's
 * next call succeeds (hank_stats out[4] counts it). A model error reported here (knots, domain, a non-monotone policy) is an
 * error on the recorded primal: it leaves no tangent batch current, so hank_get_dpolicy_seq and the other readers answer
 * HANK_ERR_NOT_READY until the next primal, exactly as after the host-pointer entries. */
int hank_check(hank_ctx *ctx);

/* hank_primal_jvp == JVP(fullFunction, x, y) exactly as the reference evaluates it: the Dual pass
 * recomputes the primal (NewtonRaphson.jl:95; GeneralStructures.jl:546-547), so value and N partials
 * travel together. One call = hank_primal + hank_jvp, but both recurrences advance together: a batch of one pass
 * (N <= 32) as TWO persistent launches that carry value and partials in every workgroup group (k_xdual_back, k_xfwd<D, true>),
 * a batch of 33 to 79 directions as ONE chain of T launches per direction (the tangent sweep runs one period behind the primal
 * sweep inside the same launches), a batch of at least HANK_WIDE_MIN = 80 directions as the Float64 sweeps followed by the on-chip
 * wide sweeps (one workgroup per direction: hank_wide.h). Leaves the context exactly as hank_primal followed by hank_jvp would.
 * PRIMAL MEMO (host-pointer form only): y_Iteration calls JVP(fullFunction, x, y) about 21 times per Newton step at ONE x
 * (NewtonRaphson.jl:91-95). When `xhh` and the boundary are bit-identical to the ones whose linearisation is on record,
 * hank_primal_jvp runs the tangent sweeps alone (= hank_jvp) and returns the recorded value: results equal the un-memoised
 * call's bit for bit under one implementation (HANK_SCHEDULE=launch|xcd) and to the rounding of the aggregate sums (1e-13)
 * in the default schedule, where a recorded primal is served by the persistent tangent sweeps. HANK_PRIMAL_MEMO=0 (read at
 * hank_create) switches it off; hank_stats out[6] counts the skipped primal sweeps. The _dev form never skips work.        */
int hank_primal_jvp(hank_ctx *ctx, const double *xhh, const double *dxhh, int32_t N, double *agg_out,
                    double *dagg_out);
int hank_primal_jvp_dev(hank_ctx *ctx, const double *d_xhh, const double *d_dxhh, int32_t N,
                        double *d_agg_out, double *d_dagg_out);

/* BackwardIteration's return value (BackwardIteration.jl:115): the policy sequence of the last
 * hank_primal, P matrices of n_a x n_e -> out[P*G]; and its partials for the last hank_jvp,
 * out[(G, P, N)] column-major (seqs_data[j][t] as Matrix{Dual}). A new primal or a new boundary
 * makes the partials HANK_ERR_NOT_READY until the next hank_jvp, under every schedule. */
int hank_get_policy_seq(hank_ctx *ctx, double *out);
int hank_get_dpolicy_seq(hank_ctx *ctx, int32_t N, double *out);
/* The Young lottery of the last primal, as the record holds it (tests): per period and grid point the bracket lo[P*G], the weight
 * lw[P*G] and the inverse gap ig[P*G] (0 at either clamp), the packed records lq[P*G] of 16 bytes {double w; int32 lo; int32
 * flags} (flags bit 0: ig is zero) that the lottery in front of a persistent Dual pass writes for its forward sweep — valid after
 * hank_primal_jvp[_dev] on the persistent sweeps only — and the wealth grid's inverse gaps iga[n_a] (iga[l] = 1 / (a[l+1] - a[l]),
 * the last entry 0): ig == (flags & 1 ? 0 : iga[lo]). Null: not asked for. */
int hank_get_lottery_record(hank_ctx *ctx, int32_t *lo, double *lw, double *ig, void *lq, double *iga);
/* Its counterpart for the persistent forward sweeps (tests): the work units the recorded lottery was cut into. With S =
 * ceil(n_a / 63) members: src[P*S], per period and member (source members lo | hi << 8 | a column is clamped << 16 | member 0 records
 * row 0's full mass << 17 | units << 18), and units[P*S*64*2], per period, member and unit the pair {e | ja << 4 | cnt << 16,
 * ta | tb << 8 | nv << 16}; a member's slots behind its count hold nothing. HANK_ERR_NOT_READY unless a persistent sweep has run at
 * the recorded primal. Null: not asked for. */
int hank_get_forward_units(hank_ctx *ctx, int32_t *src, int32_t *units);
/* More than one heterogeneous variable. BackwardIteration keeps one policy sequence per heterogeneous variable
 * (`seqs_data[j][t] = result[varname]`, BackwardIteration.jl:99-112) and ForwardIteration aggregates every one of them with the
 * SAME D_t: `agg_data[j][t] = dot(vec(policy_seqs[varname][t]), D)` (ForwardIteration.jl:303-307). Every forward kernel of the
 * fused sweeps (k_dist_step, k_tan_fwd / k_fused_fwd, k_xfwd, k_wide_fwd) therefore reduces TWO dot products per period with the
 * D_t / dD_t it holds: the policy-weighted one (hank_primal / hank_jvp's output) and the grid-weighted one, sum_pt a(pt) D_t(pt).
 * Any policy that is affine in (a, z_e, 1, a') with coefficients that depend on the period's inputs aggregates as the same
 * affine combination of them; the budget residual c = (1+r_t) a + w_t z_e + tr_t - a' (the c_grid of KrusellSmith.jl:79) is the
 * one built in:
 *   hank_get_het_outputs(ctx, n_het, dxhh, N, agg_out, dagg_out): output 0 = the policy variable of the endogenous dimension
 *   (KD / A: what hank_primal and hank_jvp return), output 1 = consumption, output 2 = Value = (1+r_t) c^-gamma (the
 *   value_current of KrusellSmith.jl:80), output 3 (one-asset HANK only) = UCE = z_e c^-gamma; n_het (1..3 Krusell-Smith,
 *   1..4 one-asset HANK) says how many the model's `heterogeneous:` section reaches, and may not exceed the count declared
 *   with hank_set_het_outputs (HANK_ERR_NOT_READY). Outputs 2 and 3 are not affine in the policy: they are reduced from the
 *   same post-transition D_t and the distribution tangent of the last tangent sweep's policy partials (csrc/hank_hetx.h),
 *   in buffers the context keeps (P·G·(2·(n_het-2) + N) doubles and less, grown to the widest request, freed by hank_destroy). agg_out (P, n_het) column-major of the last primal sweep; dagg_out (P, n_het, N)
 *   column-major of the last tangent sweep — whichever kernel family ran it — whose input `dxhh` (n_hh, P, N) is passed
 *   again (the partials of r_t, w_t, tr_t enter consumption directly). dagg_out NULL or N = 0: values only.
 *   hank_get_grid_aggregates: the raw second reduction, agg2_out[P] = sum a D_t and dagg2_out (P, N) = sum a dD_t, for a host
 *   that assembles other affine outputs itself.
 * The _dev forms take device pointers and are ordered on the context's stream.                                              */
int hank_get_het_outputs(hank_ctx *ctx, int32_t n_het, const double *dxhh, int32_t N, double *agg_out, double *dagg_out);
int hank_get_het_outputs_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, int32_t N, double *d_agg_out, double *d_dagg_out);
/* hank_set_het_outputs: how many of the family's heterogeneous outputs the caller will ask hank_get_het_outputs for
 * (BackwardIteration.jl:99-112 keeps one sequence per key listed under `heterogeneous:`, ForwardIteration.jl:303-307 dots each
 * with the same D_t). 1..3 for Krusell-Smith (KD, C, Value), 1..4 for the one-asset HANK (A, C, Value, UCE); default 2. The
 * sweeps are the same for every count; a change of the count drops the primal memo of hank_primal_jvp (a host shim that
 * serves several callers on one context only ever raises it: BackwardIteration.py ensure_het_outputs).                     */
int hank_set_het_outputs(hank_ctx *ctx, int32_t n_het);

/* ---- group outputs: who moves ----------------------------------------------------------------------
 * ForwardIteration aggregates every heterogeneous variable with the same post-transition D_t (ForwardIteration.jl:303-307).
 * A group output dots a WEIGHTED one with it: K groups (K <= HANK_GROUP_MAX), group k a weight vector W_k[G] indexed like D
 * (pt = e n_a + ia, the column-major vec of the (n_a, n_e) matrix; any real values, fixed over time) and a base b_k:
 *     Y^k_t  = sum W_k f D_t,   f = 1 (HANK_GROUP_MASS), a'_t (HANK_GROUP_POLICY), c_t = (1+r_t) a + w_t z_e + tr_t - a'_t (HANK_GROUP_CONS)
 *     dY^k_t = sum W_k f dD_t + sigma_b sum W_k D_t da'_t + [CONS] (dr_t sum W_k D_t a + dw_t sum W_k D_t z_e + dtr_t sum W_k D_t)
 * with sigma = 0, +1, -1. With W = 1, POLICY is output 0 of hank_get_het_outputs, CONS output 1, MASS is 1 with a zero tangent.
 * The caller supplies data, not formulas: the bottom half of the wealth distribution, the borrowing limit, a productivity state. */
enum {
    HANK_GROUP_MASS = 0,
    HANK_GROUP_POLICY = 1,
    HANK_GROUP_CONS = 2
};
#define HANK_GROUP_MAX 32
/* hank_set_group_outputs (ForwardIteration.jl:303-307): copies W (host, (G, K) column-major) and base[K] into buffers the context
 * owns; K = 0 clears them. The record, the current tangent batch, the primal memo and the hank_set_het_outputs count stay
 * untouched. K outside 0..HANK_GROUP_MAX, a base outside 0..2, or a null pointer with K > 0: HANK_ERR_BAD_ARG. A context made by
 * hank_clone starts without groups. */
int hank_set_group_outputs(hank_ctx *ctx, int32_t K, const double *W, const int32_t *base);
/* hank_get_group_outputs (ForwardIteration.jl:303-307): the rules of hank_get_het_outputs. agg_out (P, K) column-major from the last
 * primal; dagg_out (P, K, N) column-major from the current tangent batch of width N, whichever kernel family ran it, whose input
 * dxhh (n_hh, P, N) is passed again. dagg_out NULL or N = 0: values only. HANK_ERR_NOT_READY before any groups are set, before a
 * primal, when no batch of that width is current, and when the current batch carries boundary seeds (the recurrence after the
 * sweeps assumes dD_0 = 0, as for Value and UCE). Every sum is taken in a fixed order: the same inputs give the same bits. The
 * _dev form takes device pointers and is asynchronous on the context's stream; its direction-dependent buffers
 * (P·G·N doubles and less) live in the context and grow to the widest request. */
int hank_get_group_outputs(hank_ctx *ctx, const double *dxhh, int32_t N, double *agg_out, double *dagg_out);
int hank_get_group_outputs_dev(hank_ctx *ctx, const double *d_dxhh, int32_t N, double *d_agg_out, double *d_dagg_out);
int hank_get_grid_aggregates(hank_ctx *ctx, double *agg2_out, int32_t N, double *dagg2_out);
int hank_get_grid_aggregates_dev(hank_ctx *ctx, double *d_agg2_out, int32_t N, double *d_dagg2_out);
/* The distribution path D_1..D_P of the last hank_primal -> out[P*G] (ForwardIteration.jl:297-300). */
int hank_get_dist_seq(hank_ctx *ctx, double *out);

/* ---- granular steps (step-level parity with the reference's functions) -------------------------
 * hank_backward_step[_dual]  ==  model.value_fn(value_next, xVals, model) for the KS plugin
 *   `ValueFunction` (KrusellSmith.jl:43-83): -> (Value, KD). The _dual form carries N partials:
 *   dvalue_next/dvalue_out/dpolicy_out are (G, N) column-major, dxhh_t is (n_hh, N).
 * hank_forward_step[_dual]   ==  transition_step(policy, D_prev, Λ_exog, dim, n_exog)
 *   (ForwardIteration.jl:95-99, Young lottery :37-78) followed by dot(vec(policy), D_new)
 *   (:305-307). Any policy is accepted here (no monotonicity requirement).                       */
int hank_backward_step(hank_ctx *ctx, const double *value_next, const double *xhh_t,
                       double *value_out, double *policy_out);
int hank_backward_step_dual(hank_ctx *ctx, const double *value_next, const double *dvalue_next,
                            const double *xhh_t, const double *dxhh_t, int32_t N,
                            double *value_out, double *dvalue_out, double *policy_out,
                            double *dpolicy_out);
int hank_forward_step(hank_ctx *ctx, const double *policy, const double *D_prev, double *D_out,
                      double *agg_out);
int hank_forward_step_dual(hank_ctx *ctx, const double *policy, const double *dpolicy,
                           const double *D_prev, const double *dD_prev, int32_t N, double *D_out,
                           double *dD_out, double *agg_out, double *dagg_out);

/* ---- steady state ---------------------------------------------------------
 * hank_vfi == the inner fixed point of get_xVals (SteadyState.jl:132-141): value <- model.value_fn(value, xVals, model).Value
 * until max|value_new - value| < tol — checked after EVERY step, like the reference — or max_iter steps (:134 caps at
 * 10 000). The loop is device-resident. Where the grid fits the XCD-local schedule it is ONE persistent launch (k_xvfi:
 * the EGM step of the persistent Float64 sweep with constant prices; every member of the group compares its rows
 * against tol in Float64 and the group barrier carries the vote, so all members stop in the same step: 4.5 us per step
 * at 2000x11); otherwise the EGM step kernels of hank_backward_step iterate on HBM and a stop flag comes back per chunk
 * of steps (23 us per step). Same stopping rule, same step count, same value (tests/test_gpu_steady_state.py).
 * value_io[G]: in = the starting value (ones in the reference, :132), out = the
 * converged value; policy_out[G] = the policy of the step that produced it; *iters_out = steps taken,
 * *supnorm_out = the last max|difference|. The price Newton and invariant_dist stay on the host. */
int hank_vfi(hank_ctx *ctx, const double *xhh_t, double tol, int32_t max_iter, double *value_io, double *policy_out,
             int32_t *iters_out, double *supnorm_out);

/* hank_stationary_dist: the stationary distribution of the steady state by the power method on the device — D <- Lambda D with
 * the forward step of the hot path (Young lottery of `policy`[G] + exogenous transition), until two iterates
 * `check_every` steps apart differ by less than `tol` (max norm) or `max_iter` steps. This is the iteration the host's
 * invariant_dist uses for chains too large for the reference's direct solve (ForwardIteration.jl:436-442); same fixed
 * point. Where the grid fits the XCD-local schedule the whole iteration is ONE persistent launch (k_xstat: 3.0 us per
 * iteration at 2000x11, the verdict of every check rides on the group barrier), otherwise one launch per iteration and a
 * stop flag per chunk of checks (*iters_out then counts the iterations enqueued when the host saw the flag).
 * D_io[G]: in = start (any positive vector), out = the last iterate (NOT normalised). */
int hank_stationary_dist(hank_ctx *ctx, const double *policy, double *D_io, double tol, int32_t max_iter, int32_t check_every,
                         int32_t *iters_out);

/* hank_fake_news: the household block's sequence-space Jacobian AT THE STEADY STATE from its Toeplitz structure — what
 * getSteadyStateJacobian assembles from n_endog backward JVPs seeded at the last period (JBI, SteadyStateJacobian.jl:240-243),
 * the pullbacks through ForwardIteration (JFI, :249-253), `helper[t,s] = JFI[:, t-slice] * JBI[s-slice, :]` (:300-305) and
 * the recursion J̅[s,t] = J̅[s-1,t-1] + helper (:363-371). Here: ONE backward tangent sweep of n_hh directions (unit shock to
 * household input k in the last period: the policy response at every lag), one single-period forward push of all P*n_hh lagged
 * responses (the lottery impulse), P-1 steps of the transposed forward step (the expectation vectors), one product.
 * Requires hank_primal (host-pointer form) at the constant steady-state path with the steady state as both boundaries; anything
 * else is refused with HANK_ERR_NOT_READY (a path that varies over time, a device-pointer primal, or a recorded policy whose
 * first and last period differ by more than 1e-6 of its scale).
 *   F_out  (P, P, n_hh) column-major: F[u, j, k] = effect on the aggregate, u periods after the policy moved, of the policy
 *          response with j periods to go before a unit shock to input k (the reference's helper; "fake news" matrix)
 *   Dv_out (P, n_hh): Dv[j, k] = the direct term, (policy response at lag j) . D_ss
 * d agg_t / d xhh_{k,s} = J_k[t, s] with J_k[t, s] = J_k[t-1, s-1] + F[t, s, k], J_k[0, s] = Dv[s, k] + F[0, s, k],
 * J_k[t, 0] = F[t, 0, k] for t > 0 (0-based; hank_amd.SteadyStateJacobian.household_jacobian does the recursion). */
int hank_fake_news(hank_ctx *ctx, double *F_out, double *Dv_out);

/* hank_fake_news_het: the same Toeplitz form for the first n_het heterogeneous outputs of hank_get_het_outputs (0 the policy
 * variable KD / A, 1 consumption, 2 Value, 3 UCE for the one-asset HANK): n_het is 1..3 for Krusell-Smith, 1..4 for the
 * one-asset HANK, else HANK_ERR_BAD_ARG. Every output is Y^o_t = sum f_o D_t with the same post-transition D_t
 * (ForwardIteration.jl:303-307), so the policy responses Y_j and the lottery impulses iota_j are shared; per output only the
 * expectation vectors E^o_0 = f_o,ss, E^o_{u+1} = T' E^o_u and the direct term differ:
 *   F_out  (P, P, n_hh, n_het) column-major: F[u, j, k, o] = E^o_u . iota_{j,k}
 *   Dv_out (P, n_hh, n_het):     Dv[j, k, o] = sum D_ss (d f_o / d a') Y_{j,k} + [j == 0] d_{o,k}, d_{o,k} the same-period
 *          effect of input k on output o at the steady state (0 for o = 0; sum D (a, z_e, 1) for consumption; the Sa + Sr, Sz,
 *          S1 of hank_get_het_outputs for Value and UCE)
 * Output 0 equals hank_fake_news's F and Dv bit for bit; each output's J follows from the same recursion. The multi-output
 * J̅ has no counterpart in the reference (its slicing assumes one heterogeneous variable, SteadyStateJacobian.jl:295-303).
 * Same precondition and HANK_ERR_NOT_READY cases as hank_fake_news; independent of hank_set_het_outputs, which it leaves
 * unchanged. */
int hank_fake_news_het(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out);

/* hank_fake_news_group: the same Toeplitz form for the K group outputs of hank_set_group_outputs (ForwardIteration.jl:303-307 dots
 * every output with the same D_t, so the policy responses and the lottery impulses are shared once more):
 *   E^k_0 = W_k f_ss,  F_out (P, P, n_hh, K): F[u, j, i, k] = E^k_u . iota_{j,i}
 *   Dv_out (P, n_hh, K): Dv[j, i, k] = sigma_b sum W_k D_ss Y_{j,i} + [j == 0] d_{k,i}, d_{k,.} = sum W_k D_ss (a, z_e, 1) for
 *          HANK_GROUP_CONS and 0 for the other bases
 * The groups are served eight at a time, so the expectation vectors never take more than 8·P·G doubles. hank_fake_news's
 * precondition and refusals; HANK_ERR_NOT_READY without groups. Each group's J follows from the same recursion. */
int hank_fake_news_group(hank_ctx *ctx, double *F_out, double *Dv_out);

/* ---- the transposed household block: xhh_bar = J(x)' agg_bar -------------------------------------
 * hank_vjp == the reverse rules of the same composition at the recorded primal: the pullback of ForwardIteration
 * (ForwardIteration.jl:339-420, built on the reverse rule of transition_step, :131-192) followed by the transpose of the
 * partials of BackwardIteration (BackwardIteration.jl:46-116; the reference differentiates it forward only, so this half has
 * no counterpart there). It is the exact transpose of what hank_jvp / hank_get_het_outputs compute, for M cotangent columns
 * at once: one launch per period and sweep (csrc/hank_adjoint.h), no atomics — the same record and cotangents give the same
 * bits.
 *   agg_bar (P, n_het, M) column-major: cotangents of the aggregates of output 0 (the policy variable, KD / A) and, with
 *   n_het = 2, of output 1 (consumption) — the shape of hank_get_het_outputs's dagg_out. Outputs 2 and 3 (Value, UCE) are
 *   not affine in the policy: n_het > 2 is refused here with HANK_ERR_BAD_ARG — hank_vjp_het below carries their cotangents.
 *   xhh_bar (n_hh, P, M) column-major: cotangents of the household inputs — the shape of dxhh.
 * Needs a valid record (HANK_ERR_NOT_READY before the first primal, after a new boundary, after a persistent sweep that did
 * not run), written by any kernel family; touches neither the record, nor the current tangent batch (hank_get_dpolicy_seq,
 * hank_get_het_outputs keep serving it), nor the primal memo. The _dev form takes device pointers, is asynchronous on the
 * context's stream and never waits on the host; the host form copies in, runs, copies out and synchronises. */
int hank_vjp(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar);
int hank_vjp_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar);
/* The same product with cotangents on EVERY heterogeneous output: agg_bar (P, n_het, M) with n_het up to the family's count (3 for
 * Krusell-Smith: Value; 4 for the one-asset HANK: Value, UCE — the outputs of hank_get_het_outputs, which the reference dots with
 * the same D_t, ForwardIteration.jl:303-307). Y^o_t = sum f_o,t D_t is not affine in the policy for o >= 2; its cotangent enters
 * the reverse of the distribution sweep as a weight f_o,t on the distribution, a direct term -f_c,o,t D_t on the policy, and
 * (Sa + Sr, Sz, S1)_o,t on the inputs, from f, f_c and the sums hank_get_het_outputs uses, recorded once per primal.
 *   n_het above the family's count: HANK_ERR_BAD_ARG; above what hank_set_het_outputs declared: HANK_ERR_NOT_READY (the rule of
 *   hank_get_het_outputs); n_het <= 2: hank_vjp's own path, the same bits.
 * Everything else as hank_vjp: the record it needs, what it leaves alone, the workspace per batch width (shared with hank_vjp),
 * hank_get_policy_cotangent_seq and hank_last_vjp_timings, the _dev form. */
int hank_vjp_het(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar);
int hank_vjp_het_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar);
/* The cotangent of the policy sequence of the last hank_vjp[_het], out[(G, P, M)] column-major like hank_get_dpolicy_seq: the
 * reference's `Δpolicy_seqs` (ForwardIteration.jl:412-416) for the policy variable when n_het = 1. With n_het = 2 it is the
 * TOTAL cotangent of the savings policy: consumption's dependence on it (-agg_bar[t, 1, m] D_t) is folded in. A new primal or
 * a new boundary makes it HANK_ERR_NOT_READY until the next hank_vjp (never the cotangents of an older primal). */
int hank_get_policy_cotangent_seq(hank_ctx *ctx, int32_t M, double *out);

/* ---- tangents and cotangents on the boundary ------------------------------------------------------
 * The household block is a map (x, V_P, D_0) -> aggregates; the entries above differentiate it in x alone and hold the boundary
 * of hank_set_boundary constant. These two carry the terminal marginal value `ss_end.value` (BackwardIteration.jl:85) and the
 * initial distribution `ss_initial.D` (ForwardIteration.jl:293) as well: what a gradient with respect to a parameter that moves
 * the ending steady state, a sensitivity to the initial wealth distribution, or the seam between two time segments of a long
 * horizon needs in place of 2 G finite-difference primal sweeps. Outputs 0 and 1 (the policy variable, consumption) only.
 *
 * hank_jvp_boundary == the partials of ForwardIteration(BackwardIteration(x, ...)) under Duals seeded in xVals AND in
 * ss_end.value (BackwardIteration.jl:85) AND in ss_initial.D (ForwardIteration.jl:293), N directions at once:
 *   dxhh (n_hh, P, N) as in hank_jvp; dvalue_end, dD_init (G, N) column-major, pt = e n_a + a (the convention of
 *   hank_get_dpolicy_seq); any of the three may be NULL, meaning zeros; all three NULL is HANK_ERR_BAD_ARG.
 *   dagg_out (P, N) as in hank_jvp.
 * It always runs on the per-period launches, whatever HANK_SCHEDULE says and whichever kernel family wrote the record, and does
 * not change the context's schedule; hank_last_timings reports it in the tangent slots. It needs a valid record
 * (HANK_ERR_NOT_READY otherwise) and makes its batch the current one: hank_get_dpolicy_seq and hank_get_grid_aggregates serve it
 * as any other, hank_get_het_outputs with n_het <= 2 — consumption then includes the seed's productivity marginal,
 * w_t sum_e z_e m_t[e] + tr_t sum_e m_t[e] with m_{-1}[e] = sum_a dD_0[a, e], m_t = m_{t-1} Pi. With n_het > 2 and tangents it
 * answers HANK_ERR_NOT_READY at such a batch (Value and UCE under boundary seeds are not implemented); a later hank_jvp makes
 * them servable again. With zero seeds the results are hank_jvp's under HANK_SCHEDULE=launch bit for bit. */
int hank_jvp_boundary(hank_ctx *ctx, const double *dxhh, const double *dvalue_end, const double *dD_init, int32_t N, double *dagg_out);
int hank_jvp_boundary_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dvalue_end, const double *d_dD_init, int32_t N, double *d_dagg_out);
/* hank_vjp_boundary == hank_vjp (n_het = 1 or 2, its arguments and its refusals) with the two cotangents its sweeps hold and
 * drop — the reverse rules of ForwardIteration.jl:339-420 and :131-192 carried through to ss_initial.D (ForwardIteration.jl:293),
 * and the transpose of the backward loop carried through to ss_end.value (BackwardIteration.jl:85):
 *   value_end_bar, D_init_bar (G, M) column-major like dvalue_end / dD_init; either may be NULL (not wanted).
 *   xhh_bar equals hank_vjp's bit for bit. The exact transpose of hank_jvp_boundary with hank_get_het_outputs(n_het <= 2).
 * Everything else as hank_vjp: the record it needs, what it leaves alone (the tangent batch stays current),
 * hank_get_policy_cotangent_seq, hank_last_vjp_timings (the exports are timed with Sweep B), the _dev form. */
int hank_vjp_boundary(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar);
int hank_vjp_boundary_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar, double *d_D_init_bar);

/* ---- every output's tangent in one pair of sweeps, boundary seeds included -------------------------
 * hank_jvp_het == hank_jvp_boundary followed by hank_get_het_outputs, for EVERY declared output and from one pair of sweeps: the
 * partials of all keys of the plugin's NamedTuple (KrusellSmith.jl:80; dotted with the same D_t, ForwardIteration.jl:303-307)
 * under Duals seeded in xVals, ss_end.value (BackwardIteration.jl:85) and ss_initial.D (ForwardIteration.jl:293).
 *   dxhh, dvalue_end, dD_init as in hank_jvp_boundary: any may be NULL (zeros), all three NULL is HANK_ERR_BAD_ARG.
 *   dagg_out (P, n_het, N) column-major, as hank_get_het_outputs' dagg_out.
 *   n_het follows hank_vjp_het's rule: above the family's count HANK_ERR_BAD_ARG, above the declared count HANK_ERR_NOT_READY.
 * For outputs 2 and 3 (Value, UCE) the forward launches carry n_het - 2 extra reductions, sum f_o,t dD_t - sum f_c,o,t D_t da'_t,
 * over the dD_t the sweep itself holds: no second recurrence, and a dD_0 seed is simply there. n_het <= 2 launches the graphs of
 * hank_jvp / hank_jvp_boundary: the same bits as those under HANK_SCHEDULE=launch. With n_het > 2, outputs 0 and 1, the policy
 * partials and the grid aggregates are those of the n_het = 2 call bit for bit.
 * It always runs on the per-period launches and leaves the context's schedule alone; a record written by any family serves it.
 * Launches (hank_last_timings, tangent slots): backward P + 2, forward P + 3; with a seed pointer P + 4 and P + 5; one more
 * forward launch when n_het > 2. Its batch becomes the current one, named as hank_jvp (both seed pointers NULL) or as
 * hank_jvp_boundary (a seed pointer given) names it: hank_get_dpolicy_seq, hank_get_grid_aggregates and hank_get_het_outputs
 * behave as after those calls (hank_get_het_outputs keeps refusing n_het > 2 at a batch with seeds).
 * The _dev form takes device pointers and stays asynchronous on the context's stream. */
int hank_jvp_het(hank_ctx *ctx, int32_t n_het, const double *dxhh, const double *dvalue_end, const double *dD_init, int32_t N, double *dagg_out);
int hank_jvp_het_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, const double *d_dvalue_end, const double *d_dD_init, int32_t N, double *d_dagg_out);
/* hank_vjp_het_boundary == hank_vjp_boundary with hank_vjp_het's rule for n_het: cotangents on every declared output (Value and
 * UCE enter the reverse of the distribution sweep, ForwardIteration.jl:339-420, as in hank_vjp_het) carried through to
 * ss_end.value (BackwardIteration.jl:85) and ss_initial.D (ForwardIteration.jl:293). The exact transpose of hank_jvp_het.
 *   xhh_bar equals hank_vjp_het's bit for bit; value_end_bar, D_init_bar (G, M) column-major, either may be NULL (not wanted,
 *   left unwritten). Everything else as hank_vjp_boundary. */
int hank_vjp_het_boundary(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar);
int hank_vjp_het_boundary_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar, double *d_D_init_bar);
/* hank_vjp_group == the exact transpose of hank_get_group_outputs' tangent map: cotangents on the K group outputs of
 * hank_set_group_outputs through the transposed sweeps at the recorded primal, whichever kernel family recorded it. Group k is the
 * weighted dot of ForwardIteration.jl:303-307, so it enters the reverse of the distribution sweep (ForwardIteration.jl:339-420, on
 * the reverse rule of transition_step, :131-192) as an output with f = W_k f_b and f_c = -sigma_b W_k, formed inside the kernel:
 * nothing per grid point is stored. CONS groups also reach the inputs directly: xhh_bar_{i,t} += sum_k g[t,k] S[t][k][i].
 *   grp_bar (P, K, M) column-major, the shape of hank_get_group_outputs' dagg_out; required.
 *   agg_bar (P, n_het, M) column-major or NULL: cotangents on outputs 0 and 1 (hank_vjp's) in the same product. With agg_bar
 *   n_het is 1 or 2 (cotangents on Value / UCE come from hank_vjp_het and add linearly); with NULL n_het must be 0.
 *   xhh_bar (n_hh, P, M); value_end_bar, D_init_bar (G, M) column-major, either may be NULL (not wanted, left unwritten): the
 *   cotangents of ss_end.value (BackwardIteration.jl:85) and ss_initial.D (ForwardIteration.jl:293), as in hank_vjp_boundary.
 * HANK_ERR_BAD_ARG: a null grp_bar or xhh_bar, M < 1, an n_het that does not fit agg_bar, more LDS than the device has.
 * HANK_ERR_NOT_READY: no groups set, before a primal, after a new boundary, after a persistent sweep that did not run.
 * Leaves the record, the current tangent batch, the primal memo, the declared count and the schedule alone; shares hank_vjp's
 * workspace per width (a later hank_vjp / hank_vjp_het returns the bits it returned before). hank_get_policy_cotangent_seq serves
 * its total policy cotangent, hank_last_vjp_timings its two sweeps. No atomics, fixed-order sums: the same record, groups and
 * cotangents give the same bits. A new hank_set_group_outputs is honoured by the next call. The _dev form takes device pointers
 * and is asynchronous on the context's stream; extra workspace P * HANK_GROUP_MAX * M doubles, twice, per width. */
int hank_vjp_group(hank_ctx *ctx, int32_t n_het, const double *agg_bar, const double *grp_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar);
int hank_vjp_group_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, const double *d_grp_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar,
                       double *d_D_init_bar);

/* ---- a path of the discount factor: beta_t --------------------------------------------------------------
 * The household's own primitives are constants of a context; the one users move most is the discount factor — the demand /
 * preference shock of the HANK literature. beta enters the EGM step once, cm = (beta E_t[V_{t+1}])^(-1/gamma)
 * (KrusellSmith.jl:59-62), inside the backward loop (BackwardIteration.jl:90-113). A PATH has no counterpart in the reference,
 * which takes beta from the model's parameters (`model.params.β`) in every period.
 * DATING: beta_t is the factor in period t's Euler equation, u'(c_t) = beta_t E_t[V_{t+1}], t = 0 .. P-1; beta_{P-1} multiplies
 * the expectation of the terminal V_T (`ss_end.value`, BackwardIteration.jl:85).
 *
 * hank_set_discount_path (KrusellSmith.jl:59-62; BackwardIteration.jl:90-113; no counterpart in the reference: beta comes from
 * the model's parameters there): beta_t [P] on the host; NULL returns the context to the constant hank_model.beta (with no path
 * set that changes nothing). A non-finite or non-positive entry is HANK_ERR_BAD_ARG and nothing changes: the path in force and the
 * record stay valid. Setting or clearing a path invalidates what a new boundary invalidates — the record, the current tangent
 * batch, the policy cotangent, the primal memo (an x recorded under another path is not recognised).
 * WHILE A PATH IS SET hank_primal[_dev], hank_primal_jvp[_dev] and hank_jvp[_dev] run on the per-period launches whatever
 * HANK_SCHEDULE says (the persistent, wide and HANK_XSPEC kernels hold beta as a constant and are left as they are), without
 * changing the context's schedule policy and without counting a fallback — hank_jvp_boundary's precedent; hank_last_timings and
 * hank_info report the launch family, hank_stats out[0] does not grow. hank_vjp*, hank_jvp_boundary, hank_jvp_het,
 * hank_get_het_outputs and hank_get_group_outputs read the record and work at it unchanged. The entries that are defined at ONE
 * beta answer HANK_ERR_NOT_READY: hank_primal_batch[_dev], hank_ss_batch, hank_vfi, hank_ss_jvp[_dev], hank_ss_vjp[_dev] and
 * every hank_fake_news*. The step entries hank_backward_step[_dual] keep using hank_model.beta. */
int hank_set_discount_path(hank_ctx *ctx, const double *beta_t);
/* hank_jvp_shock == the partials of the block under Duals seeded in xVals AND in beta_t (KrusellSmith.jl:59-62 under Duals, inside
 * the loop of BackwardIteration.jl:90-113; a path has no counterpart in the reference, which takes beta from the model's
 * parameters), N directions at once:
 *   dxhh (n_hh, P, N) as in hank_jvp, or NULL (zeros); dbeta (P, N) column-major, or NULL (zeros); both NULL is HANK_ERR_BAD_ARG.
 *   dagg_out (P, N) as in hank_jvp.
 * d s_t / d beta_t = rho_t (-1/gamma) cm_t / beta_t at every knot, cm_t rebuilt from the recorded s_t: a rank-one seed of the knots'
 * tangent in EVERY period, applied by a seed kernel behind each launch of the backward tangent sweep (2 P + 3 launches; the forward
 * sweep is hank_jvp's). Works with or without a path (beta_t = hank_model.beta then). Always the per-period launches, the schedule
 * left alone; needs a valid record (HANK_ERR_NOT_READY). Its batch becomes the current one, named as hank_jvp names it:
 * hank_get_dpolicy_seq, hank_get_grid_aggregates, hank_get_het_outputs (every declared output) and hank_get_group_outputs serve
 * it. beta has NO direct term in any output: the caller passes the same dxhh (or zeros) to those getters. With dbeta zero or NULL
 * dagg_out and hank_get_dpolicy_seq equal hank_jvp's under HANK_SCHEDULE=launch bit for bit. */
int hank_jvp_shock(hank_ctx *ctx, const double *dxhh, const double *dbeta, int32_t N, double *dagg_out);
int hank_jvp_shock_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dbeta, int32_t N, double *d_dagg_out);
/* hank_vjp_shock == hank_vjp_het (its n_het rule, its refusals, its workspace, what it leaves alone) plus the cotangent of the
 * path (the transpose of KrusellSmith.jl:59-62's beta inside the loop of BackwardIteration.jl:90-113; no counterpart in the
 * reference, which differentiates forward only and takes beta from the model's parameters):
 *   beta_bar (P, M) column-major, required: beta_bar_t[m] = sum_{e,i} (d s_t / d beta_t)[e,i] sbar_t[e,i,m], sbar_t the knots'
 *   cotangent of Sweep B at period t — per-block partials behind every period's launch (the row blocks hank_vjp uses at this width),
 *   then one fixed-order sum over the blocks: no atomics, the same inputs give the same bits. P + 2 launches more in Sweep B.
 *   xhh_bar equals hank_vjp_het's bit for bit. The exact transpose of hank_jvp_shock followed by hank_get_het_outputs. */
int hank_vjp_shock(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *beta_bar);
int hank_vjp_shock_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_beta_bar);
/* hank_fake_news_shock: the Toeplitz column block of every heterogeneous output with respect to beta at the steady state
 * (KrusellSmith.jl:59-62; BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 — a beta path has no
 * counterpart in the reference, which takes beta from the model's parameters). hank_fake_news_het's preconditions, refusals,
 * definitions and recursion with the input fixed to beta; no path may be set. The policy responses come from ONE backward tangent
 * sweep seeded with d beta_{P-1} = 1; the lottery impulses, expectation vectors and products are shared code.
 *   F_out (P, P, n_het): F[u, j, o] = E^o_u . iota_j;  Dv_out (P, n_het): Dv[j, o] = sum D_ss (d f_o / d a') Y_j — the direct
 *   term d_{o,beta} is zero for every output. J_o[t, s] = J_o[t-1, s-1] + F[t, s, o], J_o[0, s] = Dv[s, o] + F[0, s, o]. */
int hank_fake_news_shock(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out);

/* ---- a path of income by productivity state: y_t[e] -------------------------------------------------------
 * Every income term of the budget is common to the productivity states; y_t[e] is an additive one that is not:
 *     c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e],    t = 0 .. P-1, e = 0 .. n_e-1
 * (KrusellSmith.jl:59-62 and :66-80 inside the loop of BackwardIteration.jl:90-113; no counterpart in the reference, whose income
 * process is a constant of the model). Targeted transfers, redistribution between states, unequal incidence of earnings and a path
 * of the productivities z_t[e] (y_t[e] = w_t (z_t[e] - z_e)) are all this primitive. y_t[e] enters wherever tr_t enters, per column:
 * the X half of period t (the knots s_t) and the Y half of period t (consumption, the marginal value), and consumption's aggregate
 * directly, C_t += sum_e y_t[e] m_t[e] with m_t[e] = sum_a D_t[e,a] the column masses of the post-transition distribution.
 *
 * hank_set_income_path: y (n_e, P) column-major on the host, y[e + n_e t]; NULL clears it (with no path set that changes nothing).
 * A non-finite entry is HANK_ERR_BAD_ARG and nothing changes. Setting or clearing a path invalidates what a new boundary
 * invalidates — the record, the current tangent batch, the policy cotangent, the primal memo. A path of zeros gives the bits of no
 * path. The income path and the discount-factor path exclude each other: each setter answers HANK_ERR_NOT_READY while the other's
 * path is set.
 * WHILE A PATH IS SET hank_primal[_dev], hank_primal_jvp[_dev] and hank_jvp[_dev] run on the per-period launches whatever
 * HANK_SCHEDULE says, as under a discount-factor path: the schedule policy is left alone, no fallback is counted, hank_info and
 * hank_last_timings report the launch family. hank_vjp (n_het <= 2), hank_get_policy_seq, hank_get_dist_seq,
 * hank_get_grid_aggregates and the group outputs on the mass and policy bases read the record and stay correct;
 * hank_get_het_outputs[_dev] with n_het <= 2 adds the direct term to consumption's level. The entries that rebuild consumption from
 * the inputs or are defined at one income process answer HANK_ERR_NOT_READY: hank_get_het_outputs with n_het > 2,
 * hank_get_group_outputs with a HANK_GROUP_CONS group, hank_jvp_het, hank_vjp_het*, hank_vjp_group, hank_jvp_boundary,
 * hank_vjp_boundary, hank_primal_batch, hank_ss_batch, hank_vfi, hank_ss_jvp, hank_ss_vjp and every hank_fake_news*. The step entries
 * hank_backward_step[_dual] ignore the path. */
int hank_set_income_path(hank_ctx *ctx, const double *y);
/* hank_jvp_income == the partials of the block under Duals seeded in xVals AND in y_t[e] (KrusellSmith.jl:59-62, :66-80 under
 * Duals, inside the loop of BackwardIteration.jl:90-113; no counterpart in the reference), N directions at once:
 *   dxhh (n_hh, P, N) as in hank_jvp, or NULL (zeros); dy (n_e, P, N) column-major, or NULL (zeros); both NULL is HANK_ERR_BAD_ARG.
 *   dagg_out (P, N) as in hank_jvp.
 * The seed, behind each launch of the backward tangent sweep: ds_t[e,i,n] += kc_t[e,i] sum_e2 Pi[e,e2] v_{t+1}[e2,i] dy_{t+1}[e2,n]
 * - rho_t dy_t[e,n] (2 P + 3 launches; the forward sweep is hank_jvp's). Works with or without a path; always the per-period
 * launches; needs a valid record (HANK_ERR_NOT_READY). Its batch becomes the current one, named as hank_jvp names it:
 * hank_get_dpolicy_seq, hank_get_grid_aggregates, hank_get_group_outputs and hank_get_het_outputs[_income] serve it. A batch seeded
 * with a dy carries it: hank_get_het_outputs (n_het <= 2) adds consumption's direct term from the batch's own dy, and the readers that
 * rebuild c from the inputs — hank_get_het_outputs with n_het > 2, hank_get_group_outputs with a HANK_GROUP_CONS group — answer
 * HANK_ERR_NOT_READY for its tangents until hank_jvp runs again. With dy zero or NULL dagg_out and hank_get_dpolicy_seq equal
 * hank_jvp's under HANK_SCHEDULE=launch bit for bit; with dy NULL the batch is hank_jvp's in every respect. */
int hank_jvp_income(hank_ctx *ctx, const double *dxhh, const double *dy, int32_t N, double *dagg_out);
int hank_jvp_income_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dy, int32_t N, double *d_dagg_out);
/* hank_get_het_outputs_income == hank_get_het_outputs for n_het <= 2 (KrusellSmith.jl:80: consumption is the budget residual;
 * ForwardIteration.jl:303-307: the weighted dot) with the direct term of the income directions: dy (n_e, P, N) column-major as
 * hank_jvp_income took it, or NULL (the dy the current batch carries, if any): consumption's tangent gains sum_e dy_t[e,n] m_t[e].
 * Output 0 has no direct term. */
int hank_get_het_outputs_income(hank_ctx *ctx, int32_t n_het, const double *dxhh, const double *dy, int32_t N, double *agg_out, double *dagg_out);
int hank_get_het_outputs_income_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, const double *d_dy, int32_t N, double *d_agg_out, double *d_dagg_out);
/* hank_vjp_income == hank_vjp (n_het 1 or 2, its refusals, its workspace, what it leaves alone) plus the cotangent of the path
 * (the transpose of KrusellSmith.jl:59-62, :66-80 inside the loop of BackwardIteration.jl:90-113; no counterpart in the reference,
 * which differentiates forward only):
 *   y_bar (n_e, P, M) column-major, required: y_bar_t[e,m] = sum_i (v_t[e,i] mu_t[e,i,m] - rho_t sbar_t[e,i,m]) + m_t[e] Cbar_t[m],
 *   sbar_t the knots' cotangent and mu_t the value's cotangent of Sweep B at period t, Cbar_t consumption's cotangent — per-block
 *   partials beside every period's launch, then one fixed-order sum over the blocks: no atomics, the same inputs give the same
 *   bits. P + 2 launches more in Sweep B. xhh_bar equals hank_vjp's bit for bit. The exact transpose of hank_jvp_income followed by
 *   hank_get_het_outputs_income. */
int hank_vjp_income(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *y_bar);
int hank_vjp_income_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_y_bar);
/* hank_fake_news_income: the Toeplitz column blocks of outputs 0 .. n_het-1 (n_het <= 2) with respect to y[e] at the steady state
 * (KrusellSmith.jl:59-62, :66-80; BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 — no counterpart in
 * the reference). hank_fake_news_het's preconditions and recursion with the input fixed to y[e]; no path may be set. The policy
 * responses come from n_e backward tangent directions seeded with d y_{P-1}[e] = 1; the rest is shared code.
 *   F_out (P, P, n_e, n_het), Dv_out (P, n_e, n_het); consumption's Dv carries the direct term m_ss[e] at lag 0, output 0 none. */
int hank_fake_news_income(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out);

/* A path of the borrowing limit (the credit crunch) is declared in a header of its own, include/hank_hip_borrow.h, which includes
 * this one: the entries of this header stay what every binding of it counts on. */

/* ---- derivatives through the steady state ------------------------------------------------------------
 * Two of the block's three inputs are steady-state objects: V_T is the fixed point of the EGM step at the steady-state prices
 * (the inner loop of get_xVals, SteadyState.jl:132-141) and D_0 the stationary distribution of the lottery that step induces
 * (invariant_dist). The reference's price Newton differentiates both: find_ss calls ForwardDiff.jacobian(F, p)
 * (SteadyState.jl:195) through a VFI carried on Duals (SteadyState.jl:132-141) and through invariant_dist's implicit-function
 * tangent (ForwardIteration.jl:446-530: (I - Lambda) dD = dLambda D, 1'dD = 0). These two entries serve that surface, forward
 * and transposed, from four fixed-point loops around ONE period of the launch family's sweep kernels (csrc/hank_ssdiff.h).
 *
 * Precondition (hank_fake_news's): the recorded primal is hank_primal (host-pointer form) at a constant path with the steady
 * state as both boundaries; anything else — no primal, a path that varies over time, a device-pointer primal, a new boundary, a
 * record whose first and last policy differ by more than 1e-6 of its scale — is HANK_ERR_NOT_READY. A record written by any
 * kernel family serves. WHICH PERIOD IS READ: the distribution side and both transposed loops read period 0 of the record
 * (D_ss = the boundary's initial distribution D_0, the lottery of the first policy, D_1 as the post-transition weights of the
 * aggregates); the value loop reads the interpolation brackets of period 1 and the knots and prices of period 0 (one period of
 * the backward tangent sweep spans two records). At a stationary record every period holds the same steady state. For that
 * reason a context of ONE period (T = 2) is refused by both entries before anything is launched: HANK_ERR_BAD_ARG, "needs a
 * record of at least two periods (T >= 3)". hank_fake_news[_het] reads period 0 alone and serves T = 2 (one lag).
 *
 * hank_ss_jvp == the partials ForwardDiff carries through the VFI (SteadyState.jl:132-141) and through invariant_dist
 * (ForwardIteration.jl:446-530) inside find_ss's Jacobian (SteadyState.jl:195), N directions at once:
 *   dxhh (n_hh, N) column-major: directions in the household prices.
 *   1. dV <- B_V dV + B_x dx from dV = 0, until max|dV_new - dV| <= tol max|dV_new| in every column;
 *   2. da' = P_V dV + P_x dx, the policy output of the converged step;
 *   3. dD <- Lambda dD + (dLambda/da' da') D from dD = 0, same stopping rule, centred (dD -= D_ss 1'dD) at every check;
 *   4. dagg_out (n_het, N): dY_o = sum f_o dD - sum f_c,o D da' + d_o . dx for the outputs of hank_get_het_outputs.
 *   dvalue_out, dpolicy_out, dD_out (G, N) column-major, pt = e n_a + a: each may be NULL (not wanted).
 * hank_ss_vjp == the transpose of that map (reverse mode through the steady state: what carries hank_vjp_het_boundary's
 * value_end_bar / D_init_bar back to the prices that determine V_ss and D_ss; the reference differentiates find_ss forward only,
 * SteadyState.jl:195, :132-141, ForwardIteration.jl:446-530), M columns at once:
 *   agg_bar (n_het, M), value_bar (G, M) on V_ss, D_bar (G, M) on D_ss: each may be NULL (zero); all three NULL is
 *   HANK_ERR_BAD_ARG. xhh_bar (n_hh, M) column-major. <agg_bar, dagg> + <value_bar, dV> + <D_bar, dD> = <xhh_bar, dx>.
 * n_het follows hank_vjp_het's rule (above the family's count HANK_ERR_BAD_ARG, above the declared count HANK_ERR_NOT_READY).
 * Not converging is not an error (as in hank_vfi): HANK_OK with iters_out[k] == max_iter and the last increment ratio in
 * resid_out[k]; k = 0 the value (nu) loop, k = 1 the distribution (lambda) loop. The loops are device-resident: the stop word
 * comes back once per chunk of 64 steps. Both calls leave alone the record's sweeps, the current tangent batch, the current
 * cotangent batch, the primal memo and the schedule; their workspaces live for the call. Like the other readers of a record they
 * may first complete it with what its writer left to be built on demand — the per-target segment records and the per-source
 * {w, ig D} records (hank_info out[7] counts that build), Sweep B's bracket segments, the extra outputs' f, f_c and sums — none of
 * which changes what any other entry computes. No atomics: the same record and inputs give the same bits. The _dev forms take
 * device pointers on the context's stream and synchronise with the host for the precondition's look at the recorded policy, for
 * the stop words, and once at the end (the workspaces go with the call). */
int hank_ss_jvp(hank_ctx *ctx, int32_t n_het, const double *dxhh, int32_t N, double tol, int32_t max_iter, double *dvalue_out, double *dpolicy_out,
                double *dD_out, double *dagg_out, int32_t iters_out[2], double resid_out[2]);
int hank_ss_jvp_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, int32_t N, double tol, int32_t max_iter, double *d_dvalue_out, double *d_dpolicy_out,
                    double *d_dD_out, double *d_dagg_out, int32_t iters_out[2], double resid_out[2]);
int hank_ss_vjp(hank_ctx *ctx, int32_t n_het, const double *agg_bar, const double *value_bar, const double *D_bar, int32_t M, double tol, int32_t max_iter,
                double *xhh_bar, int32_t iters_out[2], double resid_out[2]);
int hank_ss_vjp_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, const double *d_value_bar, const double *d_D_bar, int32_t M, double tol,
                    int32_t max_iter, double *d_xhh_bar, int32_t iters_out[2], double resid_out[2]);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------
 * Device time, in milliseconds, of the sweeps of the most recent hank_primal[_dev]/hank_jvp[_dev],
 * from HIP events recorded on the context's stream around each sweep:
 *   out[0] primal backward, out[1] primal forward, out[2] tangent backward, out[3] tangent forward,
 *   out[4] dual-sweep backward, out[5] dual-sweep forward (hank_primal_jvp); -1 where not applicable.
 * launches[k] = kernel launches inside sweep k. Valid after hank_sync. */
int hank_last_timings(hank_ctx *ctx, double out_ms[6], int32_t launches[6]);
/* The same for the two sweeps of the most recent hank_vjp[_dev]: out[0] Sweep A (the reverse of the distribution sweep,
 * ForwardIteration.jl:339-420), out[1] Sweep B (the reverse of the EGM sweep, with the reduction of xhh_bar); -1 before the
 * first hank_vjp. Valid after hank_sync. */
int hank_last_vjp_timings(hank_ctx *ctx, double out_ms[2], int32_t launches[2]);

/* Time, in milliseconds, of the two loops of the most recent hank_ss_jvp[_dev] / hank_ss_vjp[_dev], from HIP events recorded on
 * the context's stream before a loop's first step and behind the synchronisation that fetched its last stop word (the host's
 * round trip per chunk of steps is inside): out[0] the value (nu) loop, out[1] the distribution
 * (lambda) loop, in the order of iters_out; -1 before the first call. */
int hank_last_ss_timings(hank_ctx *ctx, double out_ms[2]);

/* ---- the household block at K input paths: one chain of launches --------------------------------------------------------------
 * hank_primal_batch  ==  the household block inside fullFunction (NewtonRaphson.jl:77-83) at K points x_1 .. x_K at once — what a
 *   step rule for Newton needs (the reference's alphaUpdate is a stub, NewtonRaphson.jl:117-120, and the outer loop :27-46 takes the full
 *   step unconditionally), and what nonlinear responses to a family of shocks and central differences need. Scenario k is the primal
 *   sweep at x_k: K independent paths share the launches of one (gridDim.y = scenario).
 *   xhh (n_hh, P, K) -> agg_out (P, n_het, K): outputs 0 .. n_het-1 of hank_get_het_outputs (n_het up to the count declared with
 *   hank_set_het_outputs: more is HANK_ERR_NOT_READY); policy_out (G, P, K) or NULL: every scenario's policy sequence.
 *   Needs a boundary (else HANK_ERR_NOT_READY); 1 <= K <= 64 (else HANK_ERR_BAD_ARG); the host-pointer form refuses a scenario
 *   with 1 + r <= 0 (HANK_ERR_DOMAIN) before anything runs. Output 0 and the policies hold the bits the per-period launches give
 *   for that path alone (HANK_SCHEDULE=launch), whatever K is and wherever the scenario sits in the batch.
 *   The call leaves the context's recorded primal, its tangent and cotangent batches, the memo and the counters of hank_stats
 *   exactly as they were: it works on K records of its own, grown to the widest K asked for and freed by hank_destroy.
 *   Verdict, per scenario: status_out[k] (K codes, or NULL) is scenario k's status (HANK_OK, HANK_ERR_KNOTS, HANK_ERR_DOMAIN,
 *   HANK_ERR_NONMONOTONE). The call returns HANK_OK when every scenario is; otherwise the code of the lowest failing k, and the
 *   message names k (from 0, as status_out counts), the period and the point. The outputs of the healthy scenarios are valid
 *   either way. The device-pointer form is asynchronous: its verdict arrives at the next hank_check, once, and touches neither
 *   the record nor the batches.
 * hank_last_batch_timings: HIP-event times (ms) of the last batch's backward and forward chains; -1 for none. */
int hank_primal_batch(hank_ctx *ctx, int32_t n_het, const double *xhh, int32_t K, double *agg_out, double *policy_out, int32_t *status_out);
int hank_primal_batch_dev(hank_ctx *ctx, int32_t n_het, const double *d_xhh, int32_t K, double *d_agg_out, double *d_policy_out);
int hank_last_batch_timings(hank_ctx *ctx, double out_ms[2]);

/* ---- the steady state's household side at K price vectors: one chain of launches ----------------------------------------------
 * hank_ss_batch  ==  the inner fixed point of get_xVals (SteadyState.jl:132-141) followed by invariant_dist's fixed point
 *   (ForwardIteration.jl:436-442, as the power method of hank_stationary_dist) and the aggregation of the heterogeneous keys, at K
 *   constant household price vectors at once — the forward-difference columns and the step-halving trials of the price Newton
 *   (SteadyState.jl:195), the two sides of a central difference, an asset-supply curve. Scenario k is hank_vfi at xhh[:, k] on the
 *   per-step launches, then hank_stationary_dist on its policy: K independent fixed points share the launches of one
 *   (gridDim.y = scenario), each with its own stop words; a scenario that has converged freezes while the others go on.
 *   xhh (n_hh, K) column-major. value_io (G, K): in = scenario k's starting value, out = its converged value; policy_out (G, K) =
 *   the policy of the step that produced it. D_io (G, K) or NULL (value iteration only; agg_out must then be NULL, else
 *   HANK_ERR_BAD_ARG): in = scenario k's start (positive, as the caller normalised it), out = the iterate at which its rule first
 *   held — exactly iters_out[2k+1] applications of Lambda(policy_k) to the start, NOT normalised. agg_out (n_het, K) or NULL:
 *   Y_o = sum f_o D_k / sum D_k, f_o the outputs of hank_get_het_outputs (n_het above the family's count is HANK_ERR_BAD_ARG, above
 *   the count declared with hank_set_het_outputs HANK_ERR_NOT_READY), by a block reduction in a fixed order: the same inputs give
 *   the same bits. iters_out [K][2]: value steps, distribution iterations applied (a multiple of check_every, or dist_max_iter);
 *   supnorm_out [K]: the last max|value_new - value|. Running into a cap is not an error (hank_vfi's rule): the scenario goes on
 *   with what it has and iters_out tells.
 *   The value, policy, step count and sup-norm of scenario k hold the bits of hank_vfi under HANK_SCHEDULE=launch, and D_io those of
 *   hank_stationary_dist there with max_iter = iters_out[2k+1], whatever K is and wherever the scenario sits in the batch.
 *   1 <= K <= 64, caps and check_every >= 1 (else HANK_ERR_BAD_ARG); a scenario with 1 + r <= 0 is HANK_ERR_DOMAIN before anything
 *   runs. Verdict, per scenario, as in hank_primal_batch: status_out[k] (K codes, or NULL) is HANK_OK, HANK_ERR_KNOTS,
 *   HANK_ERR_DOMAIN or HANK_ERR_NONMONOTONE; a failing scenario stops at its next check and skips the later stages (its outputs
 *   are unspecified); the call returns the code of the lowest failing k and the message names k (from 0), K and the step. The
 *   healthy scenarios' outputs are valid either way.
 *   The call needs no boundary, always runs on the launches, and leaves the recorded primal, both current batches, the memo, the
 *   schedule and the counters of hank_stats as they were, except out[5], which grows by the sum of the value steps. Its
 *   workspaces live for the call. There is no _dev form: the loops need the host once per chunk of steps.
 * hank_last_ss_batch_timings: HIP-event times (ms) of the last batch's value loops and distribution loops, the host's round trip
 *   per chunk inside; -1 before the first call (out[1]: and after a call without D_io). */
int hank_ss_batch(hank_ctx *ctx, int32_t n_het, const double *xhh, int32_t K, double vfi_tol, int32_t vfi_max_iter, double dist_tol,
                  int32_t dist_max_iter, int32_t check_every, double *value_io, double *policy_out, double *D_io, double *agg_out,
                  int32_t *iters_out, double *supnorm_out, int32_t *status_out);
int hank_last_ss_batch_timings(hank_ctx *ctx, double out_ms[2]);

/* Counters of this context (tests and scripts): out[0] sweep kernels launched by the persistent schedule, out[1] tangent
 * workspaces allocated (a change of batch width N re-uses a cached workspace: a small most-recently-used cache, 3 deep),
 * out[2] hipGraphs captured (per-period schedule), out[3] schedule in use (1 = XCD-local persistent sweeps, 0 = one
 * launch per period), out[4] times this context fell back from 1 to 0, out[5] device-resident value-function iterations
 * run by hank_vfi and hank_ss_batch (summed over its scenarios), out[6] primal sweeps the memo of hank_primal_jvp skipped, out[7] primal sweeps run (hank_primal[_dev],
 * hank_primal_jvp[_dev]). */
int hank_stats(hank_ctx *ctx, int64_t out[8]);

/* Which implementation served the last tangent sweep and how the context chooses (bench.py and the tests name the kernel family
 * they measured; the reference has one implementation, ForwardDiff's Dual pass, GeneralStructures.jl:542-550): out[0] the family of
 * the last tangent sweep (0 = one launch per period, 1 = XCD-local persistent sweeps, 2 = on-chip wide sweeps: one workgroup per
 * direction, the loop-carried state in registers), out[1] the wide sweeps' mode (0 off, 1 auto: batches of at least out[2]
 * directions, 2 every batch: HANK_SCHEDULE=wide), out[2] that threshold (HANK_WIDE_MIN at hank_create), out[3] 1 when the grid fits
 * the wide sweeps, out[4] the widest batch the persistent tangent sweeps take at a recorded primal, out[5] 1 when the tangent sweeps
 * rebuild kc and v instead of reading them (record diet), out[6] bytes of the linearisation record, out[7] times the per-source
 * records {w, ig D} were built on demand (a persistent Dual pass does not write them: the first tangent sweep or hank_fake_news
 * at its record builds them, once per record). */
int hank_info(hank_ctx *ctx, int64_t out[8]);

/* Which instances of the Dual pass's two persistent sweeps were enqueued last (tests and scripts). beta, gamma, the grids and Pi
 * are constructor arguments and fixed for a context's life (the reference closes over them in the same way: KrusellSmith.jl:59-80
 * reads them from the model's parameters in every period), so the backward sweep has instances compiled for the number of
 * productivity states and for gamma = 2 with the record diet on; they return the generic instance's bits. out[0], out[1]: NE (0 =
 * read at run time, else 4, 7 or 11) and CRRA (0 = generic powers, 1 = gamma = 2) of the last k_xdual_back; out[2], out[3]: the
 * same for the last k_xfwd<D, true> (always 0, 0: the forward sweep has no such instance); -1 before the first Dual pass.
 * HANK_XSPEC (read at hank_create): unset = the CRRA half alone (the NE half measured no gain of its own: DESIGN.md section 4),
 * 1 = both halves, ne | crra = one of them, 0 = the generic instances. */
int hank_sweep_instance(hank_ctx *ctx, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* HANK_HIP_H */
