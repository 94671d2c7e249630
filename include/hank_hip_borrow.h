/* hank_hip_borrow.h — the C ABI of a path of the borrowing limit in the household block (libhank_hip.so; csrc/hank_borrow.h,
 * DESIGN.md section 3m). An extension of include/hank_hip.h, which it includes: the same library, the same context, the same status
 * codes and layouts. (KrusellSmith.jl:52, :66-80; BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371.) */
#ifndef HANK_HIP_BORROW_H
#define HANK_HIP_BORROW_H

#include "hank_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a path of the borrowing limit: amin_t ----------------------------------------------------------------
 * The credit crunch (deleveraging shock) of the HANK literature: the limit tightens and relaxes over time and the constrained
 * households are forced to save. The limit enters the Y half once, a'_t = max(g_t, amin_t), g_t the interpolated or
 * flat-extrapolated policy (KrusellSmith.jl:66-76, inside the loop of BackwardIteration.jl:90-113). A PATH has no counterpart in
 * the reference, which reads `borrow_cons` from the model's parameters in every period (KrusellSmith.jl:52, :76).
 * DATING: amin_t is the limit in period t's choice, t = 0 .. P-1.
 * A point is CONSTRAINED in period t exactly where max took the limit under the DiffRules rule, (amin_t > g) | (signbit(amin_t) <
 * signbit(g)); a tie g == amin_t is not constrained, the partial stays with g. The derivative has two effects in period t, both on
 * the constrained set C_t: da'_t += d amin_t, and dc_t -= d amin_t, hence dV_t += -v_t d amin_t. C_t is rebuilt from the record.
 * KINK CONVENTIONS (the Dual rules' own): (i) with amin_t <= a_grid[0] the limit never binds through max — the grid's flat
 * extrapolation binds instead — and EVERY PARTIAL IN amin_t IS AN EXACT ZERO: a user who wants a response must carry grid points
 * below the limit. (ii) With amin_t exactly on a grid point a_grid[k], k > 0, the lottery's bracket is the left one
 * (searchsortedfirst) and the derivative is the left derivative.
 *
 * hank_set_borrow_path: amin_t [P] on the host; NULL returns the context to the constant hank_model.borrow_cons (with no path set
 * that changes nothing). A non-finite entry, or one above a_grid[n_a-1], is HANK_ERR_BAD_ARG and nothing changes. A path equal to
 * hank_model.borrow_cons in every period gives the bits of no path. Setting or clearing a path invalidates what a new boundary
 * invalidates. One path is in force at a time: this setter answers HANK_ERR_NOT_READY while a discount-factor or an income path is
 * set, and theirs do while this one is; hank_jvp_shock, hank_vjp_shock, hank_jvp_income and hank_vjp_income (and their _dev forms)
 * answer HANK_ERR_NOT_READY under a borrowing-limit path too. Mind convention (i): a path that stays at or below a_grid[0] moves nothing.
 * WHILE A PATH IS SET hank_primal[_dev], hank_primal_jvp[_dev] and hank_jvp[_dev] run on the per-period launches whatever
 * HANK_SCHEDULE says, as under a discount-factor path: the schedule policy is left alone, no fallback is counted. The readers of
 * the record see the limit only through the recorded policy and its zero partials and work unchanged: every hank_vjp*,
 * hank_jvp_boundary, hank_jvp_het, hank_get_het_outputs at every n_het, hank_get_group_outputs on all three bases, hank_vjp_group.
 * The entries defined at ONE limit answer HANK_ERR_NOT_READY: hank_primal_batch[_dev], hank_ss_batch, hank_vfi, hank_ss_jvp[_dev],
 * hank_ss_vjp[_dev] and every hank_fake_news*. The step entries hank_backward_step[_dual] keep using hank_model.borrow_cons. */
int hank_set_borrow_path(hank_ctx *ctx, const double *amin_t);
/* hank_jvp_borrow == the partials of the block under Duals seeded in xVals AND in amin_t (KrusellSmith.jl:76-80 under Duals, inside
 * the loop of BackwardIteration.jl:90-113; a path has no counterpart in the reference), N directions at once:
 *   dxhh (n_hh, P, N) as in hank_jvp, or NULL (zeros); damin (P, N) column-major, or NULL (zeros); both NULL is HANK_ERR_BAD_ARG.
 *   dagg_out (P, N) as in hank_jvp.
 * The seed, behind the launch of the backward tangent sweep that wrote period t's policy partials: dpol_t[e,a,n] += damin_t[n] on C_t
 * and ds_{t-1}[e,i,n] += kc_{t-1}[e,i] sum_e2 Pi[e,e2] (-v_t[e2,i] 1[(e2,i) in C_t]) damin_t[n] (at t = 0 only da'_0 moves); 2 P + 3
 * launches, the forward sweep is hank_jvp's. Works with or without a path (amin_t = hank_model.borrow_cons then), at a record
 * written by any kernel family; refused (HANK_ERR_NOT_READY) while a path of another kind is set. Always the per-period launches;
 * needs a valid record. Its batch becomes the current one, named as hank_jvp names it: hank_get_dpolicy_seq,
 * hank_get_grid_aggregates, hank_get_het_outputs (every declared output) and hank_get_group_outputs serve it. amin has NO direct term
 * in any output: the caller passes the same dxhh (or zeros) to those getters. With damin zero or NULL dagg_out and
 * hank_get_dpolicy_seq equal hank_jvp's under HANK_SCHEDULE=launch bit for bit. */
int hank_jvp_borrow(hank_ctx *ctx, const double *dxhh, const double *damin, int32_t N, double *dagg_out);
int hank_jvp_borrow_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_damin, int32_t N, double *d_dagg_out);
/* hank_vjp_borrow == hank_vjp_het (its n_het rule, its refusals, its workspace, what it leaves alone) plus the cotangent of the
 * path (the transpose of KrusellSmith.jl:76-80's limit inside the loop of BackwardIteration.jl:90-113; no counterpart in the
 * reference, which differentiates forward only):
 *   amin_bar (P, M) column-major, required: amin_bar_t[m] = sum_{(e,a) in C_t} (pbar_t[e,a,m] - v_t[e,a] mu_t[e,a,m]), pbar_t the
 *   total policy cotangent and mu_t the value's cotangent of Sweep B at period t — per-block partials beside every period's launch
 *   (the row blocks hank_vjp uses at this width), then one fixed-order sum over the blocks: no atomics, the same inputs give the
 *   same bits. P + 2 launches more in Sweep B. xhh_bar equals hank_vjp_het's bit for bit. The exact transpose of hank_jvp_borrow
 *   followed by hank_get_het_outputs. */
int hank_vjp_borrow(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *amin_bar);
int hank_vjp_borrow_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_amin_bar);
/* hank_fake_news_borrow: the Toeplitz column block of every heterogeneous output with respect to the limit at the steady state
 * (KrusellSmith.jl:76-80; BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 — no counterpart in the
 * reference). hank_fake_news_het's preconditions and recursion with the input fixed to the limit; no path may be set. The policy
 * responses come from ONE backward tangent sweep seeded with d amin_{P-1} = 1; the rest is shared code.
 *   F_out (P, P, n_het), Dv_out (P, n_het): the direct term is zero for every output; Dv[0, o] carries the constrained set's
 *   da' = 1 through sum D_ss (d f_o / d a') Y_0. Under convention (i) a steady state whose limit is a_grid[0] gives zeros. */
int hank_fake_news_borrow(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out);

#ifdef __cplusplus
}
#endif
#endif /* HANK_HIP_BORROW_H */
