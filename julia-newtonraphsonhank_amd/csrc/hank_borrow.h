// hank_borrow.h — a PATH of the borrowing limit, amin_t, in the household block: the primal sweep at a path, the tangent seed of
// d amin_t in the backward tangent sweep and its transpose in Sweep B (hank_set_borrow_path, hank_jvp_borrow, hank_vjp_borrow,
// hank_fake_news_borrow — include/hank_hip_borrow.h).
//
// The limit enters the Y half once (egm_Y_finish, hank_kernels.h; KrusellSmith.jl:76): a'_t = max(g_t, amin_t), g_t the interpolated
// or flat-extrapolated policy of KrusellSmith.jl:66-76. The reference reads borrow_cons from the model's parameters in every period
// (KrusellSmith.jl:52, :76), so a path has no counterpart there. DATING: amin_t is the limit in period t's choice, t = 0 .. P-1.
//
//   primal     the Y half of period t runs with a period-local copy of Consts whose bc is amin_t: egm_step_body is called unchanged
//              (k_shk_egm_step's method). The X half does not read bc: the last period's k_egm_X is the model's own launch.
//   the set    C_t, the points where the primal's max took the limit under the DiffRules rule egm_Y_finish implements,
//              (amin_t > g) | (signbit(amin_t) < signbit(g)); a tie g == amin_t is not in it. It is REBUILT FROM THE RECORD
//              (brw_constrained, the one statement of the rule), so the entries work at a record written by any kernel family.
//   tangent    on C_t: da'_t += damin_t, dc_t -= damin_t, hence dV_t += -v_t damin_t. The launch of k_tan_back that wrote dpol_t
//              also produced the knots' tangent of period t-1 from dV_t, so behind it
//                  dpol_t[e,a,n]    += damin_t[n]                                                          on C_t
//                  ds_{t-1}[e,i,n]  += kc_{t-1}[e,i] sum_{e2} Pi[e,e2] (-v_t[e2,i] 1[(e2,i) in C_t]) damin_t[n]
//              (at t = 0 there is no ds_{-1}: only da'_0 moves). k_tan_back itself is launched unchanged. amin has no direct term
//              in any output: every output's response comes through da' and dD.
//   transpose  amin_bar_t[m] = sum_{(e,a) in C_t} (pbar_t[e,a,m] - v_t[e,a] mu_t[e,a,m]): pbar_t the total policy cotangent, mu_t
//              the cotangent of dV_t that Sweep B carries into period t (mu_0 = 0) — what k_shk_bbar and k_inc_ybar read, without
//              the gather of sbar. Per block partials, then k_reduce_parts: no atomics, every sum in a fixed order.
//
// KINK CONVENTIONS (the Dual rules' own):
//   (i)  with amin_t <= a[0] the limit never binds through max — the grid's flat extrapolation binds instead — and every partial in
//        amin_t is an exact zero. A user who wants a response carries grid points below the limit.
//   (ii) with amin_t exactly on a grid point a[k], k > 0, the lottery's bracket is the left one (searchsortedfirst): the derivative
//        is the left derivative. Nothing here decides that: the forward tangent kernels read the recorded bracket.
// Nothing is added to the record.
#pragma once
#include "hank_kernels.h"

namespace hank {

// ---- the constrained set, from the record --------------------------------------------------------------------------------------
// convention (i): no point of a period with amin_t <= a[0] is constrained (a cheap way out for a whole launch; brw_constrained
// answers the same point by point)
__device__ __forceinline__ bool brw_never_binds(const Consts &c, double am) { return !(am > c.a[0]); }
// what the rule reads at a point of period t, so that a caller can issue every point's loads before it uses the first
struct BrwPt { double A, B, pol; };
__device__ __forceinline__ BrwPt brw_load(const Record &R, size_t off) { return BrwPt{R.A[off], R.B[off], R.pol[off]}; }
// (e, i) in C_t: max zeroed both partials and left the limit as the policy — and it was max, not the grid's flat extrapolation
// meeting a limit that sits on the grid's end: a tie, whose partial stays with g. The bottom tie (x < s_t[0,e] with a[0] == amin_t)
// belongs to a period brw_never_binds has already answered; the top tie (x > s_t[n_a-1,e] with a[n_a-1] == amin_t) is left here.
// top: amin_t == a[n_a-1], which the caller asks ONCE per thread (brw_top); the last knot is read only in such a period.
__device__ __forceinline__ bool brw_top(const Consts &c, double am) { return am == c.a[c.n_a - 1]; }
__device__ __forceinline__ bool brw_constrained(const Consts &c, const Record &R, int t, int e, int i, double am, bool top, const BrwPt &p) {
    if (!(p.A == 0.0 && p.B == 0.0 && p.pol == am)) return false;
    if (top && c.a[i] > R.s[(size_t)t * c.G + (size_t)e * c.n_a + (c.n_a - 1)]) return false;
    return true;
}

// ---- primal: k_egm_step with bc taken from the path ------------------------------------------------------------------------------
// Y of period t with amin_t, then X of period t-1 (no bc in it). block, grid and dynamic LDS of k_egm_step.
__global__ void k_brw_egm_step(Consts c, Record R, const double *xhh, const double *__restrict__ amin, int t, int *err) {
    extern __shared__ double sh[];
    Consts cb = c;
    cb.bc = amin[t];
    egm_step_body(cb, R, xhh, t, err, blockIdx.x, sh);
}

// ---- tangent ---------------------------------------------------------------------------------------------------------------------
constexpr int BRW_NE = 16;      // the context's bound on n_e (hank_create)
// The seed of period t, behind the launch of k_tan_back that wrote dpol_t [e][n_a][N] and the knots' tangent ds_{t-1} [e][n_a][N]
// (dsp; null at t = 0). One thread per (row, direction), direction fastest; it holds the n_e columns of its row. da: damin_t [N].
// lds: Pi and da are staged in dynamic LDS (n_e n_e + N doubles; the host says whether they fit), read from global memory otherwise.
// A zero seed adds nothing — not even +0 to a -0 — so zero directions leave hank_jvp's bits. grid ceil(n_a N / 256).
__global__ void __launch_bounds__(256) k_brw_seed_back(Consts c, Record R, const double *__restrict__ amin, int t, const double *__restrict__ da,
                                                       size_t N, int lds, double *__restrict__ dpol_t, double *__restrict__ dsp) {
    extern __shared__ double brw_sh[];
    const int ne = c.n_e;
    const double am = amin[t];
    if (brw_never_binds(c, am)) return;      // (the whole launch)
    const double *Pi = c.Pi, *d0 = da;
    if (lds) {
        double *Psh = brw_sh, *s0 = brw_sh + ne * ne;
        for (int k = threadIdx.x; k < ne * ne; k += 256) Psh[k] = c.Pi[k];
        for (size_t k = threadIdx.x; k < N; k += 256) s0[k] = da[k];
        __syncthreads();
        Pi = Psh; d0 = s0;
    }
    const size_t cnt = (size_t)c.n_a * N, j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int i = (int)(j / N);
    const double d = d0[j - (size_t)i * N];
    if (d == 0.0) return;
    // every column's loads first, in registers (the loops are unrolled to the bound on n_e), as k_inc_seed_back does
    BrwPt p[BRW_NE];
    double vv[BRW_NE], kcv[BRW_NE], dsv[BRW_NE], dpv[BRW_NE];
#pragma unroll
    for (int e = 0; e < BRW_NE; e++) {
        const size_t pt = (size_t)e * c.n_a + i, off = (size_t)t * c.G + pt;
        p[e] = e < ne ? brw_load(R, off) : BrwPt{1.0, 1.0, 0.0};
        vv[e] = e < ne ? R.v[off] : 0.0;
        dpv[e] = e < ne ? dpol_t[(size_t)e * cnt + j] : 0.0;
        kcv[e] = (dsp && e < ne) ? R.kc[off - c.G] : 0.0;
        dsv[e] = (dsp && e < ne) ? dsp[(size_t)e * cnt + j] : 0.0;
    }
    const bool top = brw_top(c, am);
    double q[BRW_NE];      // -v_t[e2,i] 1[(e2,i) in C_t] damin_t[n]
#pragma unroll
    for (int e = 0; e < BRW_NE; e++) {
        q[e] = 0.0;
        if (e < ne && brw_constrained(c, R, t, e, i, am, top, p[e])) {
            q[e] = -vv[e] * d;
            dpol_t[(size_t)e * cnt + j] = dpv[e] + d;
        }
    }
    if (!dsp) return;
#pragma unroll
    for (int e = 0; e < BRW_NE; e++) {
        if (e < ne) {
            double acc = 0.0;
#pragma unroll
            for (int e2 = 0; e2 < BRW_NE; e2++)
                if (e2 < ne) acc += Pi[e + ne * e2] * q[e2];
            const double add = kcv[e] * acc;
            if (add != 0.0) dsp[(size_t)e * cnt + j] = dsv[e] + add;
        }
    }
}

// ---- transpose -------------------------------------------------------------------------------------------------------------------
// amin_bar_t's per-block partials at period t of Sweep B (beside k_adj_egm's launch of that period: it reads the same mu_t = muIn and
// pbar_t and writes neither). A block owns the rows [i0, i0 + RO) of every column — RO the row count hank_vjp's blocks own at this
// width (AdjGeom::R) — and MC (a power of two <= 64) cotangent columns, column fastest across the lanes; the BRW_BT / MC slots of a
// column stride over the block's (e, i) items, e outer, and are combined through LDS in two steps of a fixed order, as k_shk_bbar's
// are. No gather: an item reads its own point. first: t = 0, mu_0 = 0. part [nb][M] of period t. grid (nb, ceil(M / MC)), block BRW_BT.
constexpr int BRW_BT = 1024;
__global__ void __launch_bounds__(BRW_BT) k_brw_abar(Consts c, Record R, const double *__restrict__ amin, int RO, int MC, int t, int first,
                                                  const double *__restrict__ muIn, const double *__restrict__ pbar, int M, double *__restrict__ part) {
    __shared__ double red[BRW_BT];
    const int n = c.n_a, ne = c.n_e;
    const int ml = threadIdx.x & (MC - 1), slot = threadIdx.x / MC, nslot = BRW_BT / MC;
    const int m = blockIdx.y * MC + ml, i0 = blockIdx.x * RO;
    const int rows = max(min(RO, n - i0), 0);
    const double am = amin[t];
    const bool top = brw_top(c, am);
    double acc = 0.0;
    if (m < M && !brw_never_binds(c, am)) {
        for (int it = slot; it < ne * rows; it += nslot) {
            const int e = it / rows, i = i0 + (it - e * rows);
            const size_t pt = (size_t)e * n + i, off = (size_t)t * c.G + pt;
            const BrwPt p = brw_load(R, off);
            double g = pbar[off * M + m];
            if (!first) g -= R.v[off] * muIn[pt * M + m];
            if (brw_constrained(c, R, t, e, i, am, top, p)) acc += g;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    const int n1 = min(nslot, 32);
    double v = 0.0;
    if (slot < n1)
        for (int k = slot; k < nslot; k += 32) v += red[k * MC + ml];
    __syncthreads();
    if (slot < n1) red[slot * MC + ml] = v;
    __syncthreads();
    if (slot == 0 && m < M) {
        double tot = 0.0;
        for (int k = 0; k < n1; k++) tot += red[k * MC + ml];
        part[(size_t)blockIdx.x * M + m] = tot;
    }
}

}  // namespace hank
