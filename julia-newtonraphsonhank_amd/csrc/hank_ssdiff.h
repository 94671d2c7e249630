// hank_ssdiff.h — derivatives THROUGH the steady state (hank_ss_jvp / hank_ss_vjp).
//
// The household block is a map (x, V_T, D_0) -> aggregates, and at a steady state two of its three inputs are fixed points of the
// prices themselves: V = B(V, x) (the inner loop of get_xVals, SteadyState.jl:132-141) and D = Lambda(a'(V, x)) D, 1'D = 1
// (invariant_dist, whose implicit-function tangent is ForwardIteration.jl:446-530: (I - Lambda) dD = dLambda D, 1'dD = 0). The
// reference differentiates both with ForwardDiff inside the price Newton (SteadyState.jl:195). Here the same derivatives come from
// four fixed-point loops around ONE period of the launch family's sweep kernels at a stationary record (the record of hank_primal
// at the constant steady-state path, the precondition of hank_fake_news):
//
//   JVP   dV  <- B_V dV + B_x dx                  k_ss_back: tan_back_body (k_tan_back's body), Y half of period 1, X half of period 0
//         dD  <- Lambda dD + (dLambda da') D      k_ss_fwd:  tan_fwd_body (k_tan_fwd / k_tan_fwd_hx's body) at period 0
//   VJP   e   <- Lambda' (e - (D'e) 1), lam += e  k_ss_lam:  adj_dist_body (k_adj_dist's body) at period 0, no output cotangent inside
//         nu  <- B_V' nu + (P_V' pbar + Vbar)     k_ss_nu:   adj_egm_body (k_adj_egm's body) at period 0, with a constant source
//
// The constant sources of the two JVP loops are the step bodies' own (the input tangents and the policy tangent are fed again every
// step). What the loops add lives in each step's epilogue, not in a second pass over the state: the per-column increment norm and
// scale as per-block partials (maxima: no order to fix), the lam accumulation, the nu source, and for dD the column sums. A one-block
// check kernel reduces the partials in block order, centres dD (dD -= D 1'dD: rounding drifts along the null direction of I - Lambda)
// and sets the stop word; once it is set, every later launch of the chunk leaves at once, so the state stays frozen (the manner of
// k_vfi_check) and the host reads the word once per chunk of steps.
//
// Layout and lanes are the launch family's: state [e][a][N], direction fastest, VT = double2 (two adjacent columns per lane) for an
// even width. No atomics: the same record and inputs give the same bits.
//
// These kernels are compiled in a translation unit of their own (hank_ssdiff.hip): they instantiate the sweep kernels' device bodies
// a second time, and inside one translation unit that changes how the compiler treats the bodies in the sweep kernels themselves
// (their register counts moved). Everything the two units share — structs, helpers, the bodies — is hank_device.h's, one definition
// in namespace hank; hank_hip.hip sees the launchers of hank_ssdiff_launch.h only.
#pragma once
#include "hank_device.h"
#include "hank_ssdiff_launch.h"

namespace hank {


__device__ __forceinline__ double ss_abs(double v) { return fabs(v); }
__device__ __forceinline__ double2 ss_abs(double2 v) { return make_double2(fabs(v.x), fabs(v.y)); }
__device__ __forceinline__ double ss_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double2 ss_max(double2 a, double2 b) { return make_double2(fmax(a.x, b.x), fmax(a.y, b.y)); }
// the value this thread has just stored with st_wt (a write-through store): read where that store went
__device__ __forceinline__ double ss_ld(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ double2 ss_ld(const double2 *p) { return make_double2(ss_ld(&p->x), ss_ld(&p->y)); }
template <typename VT>
__device__ __forceinline__ VT ss_rows_max(VT v, int NC) {      // over the lanes of a wave that share the column lane nl
    for (int off = 32; off >= NC; off >>= 1) v = ss_max(v, vshfl_xor(v, off));
    return v;
}

// (n_hh, N) column-major -> dxr[2][N], dxw[2][N], dxt[2][N]: the same input tangents at both periods the backward body reads
__global__ void k_ss_in(const double *__restrict__ dxhh, int n_hh, int N, double *__restrict__ dxr, double *__restrict__ dxw, double *__restrict__ dxt) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * N) return;
    const int n = idx >= N ? idx - N : idx;
    const double *x = dxhh + (size_t)n_hh * n;
    dxr[idx] = x[0];
    dxw[idx] = x[1];
    dxt[idx] = n_hh > 2 ? x[2] : 0.0;
}

// ---- JVP, value loop: one step dV <- B_V dV + B_x dx ----------------------------------------------------------------------------
// tan_back_body with t = 1: the Y half reads the knots' tangent ds (the loop's ping-pong state) and the brackets of period 1 and
// leaves da' (dpol, row 1 of a [2][G][N] buffer) and dV (in its LDS tile); the X half mixes dV into the next ds with the record of
// period 0. Epilogue: dV leaves the tile for its own [e][a][N] buffer next to the comparison with the last step's.
// parts [block][2][N]: max |dV_new - dV|, max |dV_new|.
template <int RG, typename VT>
__global__ void __launch_bounds__(1024)
k_ss_back(Consts c, Record R, const double *__restrict__ xhh, const VT *__restrict__ dxr, const VT *__restrict__ dxw, const VT *__restrict__ dxt,
          TanGeom g, const VT *__restrict__ dsIn, VT *__restrict__ dsOut, VT *__restrict__ dpol, VT *__restrict__ dV, VT *__restrict__ parts,
          const SsCtl *__restrict__ ctl) {
    __shared__ VT dVsh[RG < 2 ? 2 : RG][16 * 64];
    __shared__ double Pish[256];
    if (ctl->stop) return;
    tan_back_body<RG, VT>(c, R, xhh, dxr, dxw, dxt, g, 1, 0, dsIn, dsOut, dpol, blockIdx.x, blockIdx.y, dVsh, Pish);
    const int nbr_b = (g.nbx + RG - 1) / RG;
    const int bidx = ((int)blockIdx.x < nbr_b) ? xcd_contiguous(blockIdx.x, nbr_b) : (int)blockIdx.x;
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC, RB = 64 >> g.lgNC;
    const int n = blockIdx.y * g.NC + nl;
    const size_t N = g.N;
    VT inc, sc;
    vzero(inc); vzero(sc);
#pragma unroll
    for (int q = 0; q < RG; q++) {
        const int a = (bidx * RG + q) * RB + rl;
        if (a < c.n_a && n < g.N) {
            const VT nv = dVsh[q][e * 64 + lane];
            VT *p = &dV[((size_t)e * c.n_a + a) * N + n];
            inc = ss_max(inc, ss_abs(vsub(nv, *p)));
            sc = ss_max(sc, ss_abs(nv));
            *p = nv;
        }
    }
    inc = ss_rows_max(inc, g.NC); sc = ss_rows_max(sc, g.NC);
    lds_barrier();      // every wave has left the mixing: the tiles are free
    dVsh[0][e * 64 + lane] = inc;
    dVsh[1][e * 64 + lane] = sc;
    lds_barrier();
    if (e == 0 && rl == 0 && n < g.N) {
        for (int k = 1; k < c.n_e; k++) { inc = ss_max(inc, dVsh[0][k * 64 + lane]); sc = ss_max(sc, dVsh[1][k * 64 + lane]); }
        parts[((size_t)bidx * 2) * N + n] = inc;
        parts[((size_t)bidx * 2 + 1) * N + n] = sc;
    }
}

// ---- JVP, distribution loop: one step dD <- Lambda dD + (dLambda da') D -------------------------------------------------------------
// tan_fwd_body at period 0 with the converged da' fed every step: its lottery-weight term IS the source s = (dLambda/da' da') D
// (the impulse of k_fn_impulse), and its reductions at the last step are dY's (the direct policy terms and the NX extra outputs
// included). Epilogue: the thread reads back the rows it stored. parts [block][3][N]: max |dD_new - dD| and max |dD_new| over the
// rows 1 .. n_a-1, and the sum of every stored row (virtual rows included). Row 0 is a sum of parts (the real row and KV virtual
// rows): the check kernel compares it whole.
template <int RG, typename VT, bool SS, int NX>
__global__ void __launch_bounds__(1024)
k_ss_fwd(Consts c, Record R, TanGeom g, const VT *__restrict__ dDin, VT *__restrict__ dDout, const VT *__restrict__ dpol, VT *__restrict__ aggpart,
         TanHx<VT, NX> hx, VT *__restrict__ parts, const SsCtl *__restrict__ ctl) {
    __shared__ VT sh[RG > NX ? RG : NX][16 * 64];
    __shared__ VT red[16 * 64], red2[16 * 64];
    __shared__ double Pish[256];
    if (ctl->stop) return;
    tan_fwd_body<RG, VT, SS, NX>(c, R, g, 0, dDin, dDout, dpol, aggpart, blockIdx.x, blockIdx.y, gridDim.x, sh, Pish, red, red2, hx);
    const int nbr = (g.nbx + RG - 1) / RG;
    const int bidx = (g.N * (int)(sizeof(VT) / 8) <= HANK_XCDMAP_FWD_MAXN && (int)blockIdx.x < nbr) ? xcd_contiguous(blockIdx.x, nbr) : (int)blockIdx.x;
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC, RB = 64 >> g.lgNC;
    const int n = blockIdx.y * g.NC + nl;
    const size_t N = g.N;
    const int na = c.n_a, nav = c.n_a + KV;
    const bool nok = n < g.N;
    VT inc, sc, sum;
    vzero(inc); vzero(sc); vzero(sum);
#pragma unroll
    for (int q = 0; q < RG; q++) {
        const int r = bidx >= nbr ? na + (bidx - nbr) : (bidx * RG + q) * RB + rl;
        const bool valid = bidx >= nbr ? (q == 0 && nok && rl == 0) : (r < na && nok);
        if (valid) {
            const size_t idx = ((size_t)e * nav + r) * N + n;
            const VT nv = ss_ld(&dDout[idx]);
            sum = vadd(sum, nv);
            if (r > 0 && r < na) {
                inc = ss_max(inc, ss_abs(vsub(nv, dDin[idx])));
                sc = ss_max(sc, ss_abs(nv));
            }
        }
    }
    inc = ss_rows_max(inc, g.NC); sc = ss_rows_max(sc, g.NC);
    for (int off = 32; off >= g.NC; off >>= 1) sum = vadd(sum, vshfl_xor(sum, off));
    lds_barrier();      // wave 0 has read the body's partials: red, red2 and the sh tiles are free
    red[e * 64 + lane] = inc;
    red2[e * 64 + lane] = sc;
    sh[0][e * 64 + lane] = sum;
    lds_barrier();
    if (e == 0 && rl == 0 && nok) {
        for (int k = 1; k < c.n_e; k++) {
            inc = ss_max(inc, red[k * 64 + lane]); sc = ss_max(sc, red2[k * 64 + lane]); sum = vadd(sum, sh[0][k * 64 + lane]);
        }
        parts[((size_t)bidx * 3) * N + n] = inc;
        parts[((size_t)bidx * 3 + 1) * N + n] = sc;
        parts[((size_t)bidx * 3 + 2) * N + n] = sum;
    }
}

// ---- the check kernels: ONE block ---------------------------------------------------------------------------------------------------
// every column n: inc_n = max_b parts[b][0][n], sc_n = max_b parts[b][1][n]; converged when inc_n <= tol sc_n in EVERY column.
// ctl: one more step taken, the worst ratio inc_n / sc_n, the stop word. A launch behind the stop word does nothing.
__device__ inline void ss_verdict(double worst, int bad, SsCtl *ctl) {
    __shared__ double wsh[16];
    __shared__ int bsh[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    for (int off = 32; off > 0; off >>= 1) { worst = fmax(worst, __shfl_xor(worst, off, 64)); bad |= __shfl_xor(bad, off, 64); }
    if (lane == 0) { wsh[wv] = worst; bsh[wv] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < nw; k++) { worst = fmax(worst, wsh[k]); bad |= bsh[k]; }
        ctl->iters = ctl->iters + 1;
        ctl->resid = worst;
        if (!bad) ctl->stop = 1;
    }
}
__device__ __forceinline__ double ss_ratio(double inc, double sc) { return sc > 0.0 ? inc / sc : (inc > 0.0 ? INFINITY : 0.0); }

// sum_out (K = 3 only, else null): sum_out[n] = sum_b parts[b][2][n] in block order (the lambda loop's centring constant D_ss'e).
__global__ void __launch_bounds__(256) k_ss_check(const double *__restrict__ parts, int nb, int K, int N, double tol, SsCtl *ctl, double *__restrict__ sum_out) {
    if (ctl->stop) return;
    double worst = 0.0;
    int bad = 0;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double inc = 0.0, sc = 0.0;
        for (int b = 0; b < nb; b++) { inc = fmax(inc, parts[((size_t)b * K) * N + n]); sc = fmax(sc, parts[((size_t)b * K + 1) * N + n]); }
        if (sum_out) {
            double sm = 0.0;
            for (int b = 0; b < nb; b++) sm += parts[((size_t)b * K + 2) * N + n];
            sum_out[n] = sm;
        }
        if (!(inc <= tol * sc)) bad = 1;
        worst = fmax(worst, ss_ratio(inc, sc));
    }
    ss_verdict(worst, bad, ctl);
}

// the distribution loop's check: the same verdict with row 0 compared whole (real row + virtual rows, new against old), then the
// centring dD_new -= D_ss (1'dD_new) of every real row (D_ss: the boundary's initial distribution, R.Dseq of period 0), so the next
// step — or the caller — starts from a tangent that sums to zero. sig [N]: the column sums before the centring (scratch).
__global__ void __launch_bounds__(1024) k_ss_check_dist(Consts c, const double *__restrict__ Dss, const double *__restrict__ parts, int nb, int N, double tol,
                                                        double *__restrict__ dDnew, const double *__restrict__ dDold, double *__restrict__ sig, SsCtl *ctl) {
    if (ctl->stop) return;
    const int na = c.n_a, nav = c.n_a + KV;
    double worst = 0.0;
    int bad = 0;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double inc = 0.0, sc = 0.0, s = 0.0;
        for (int b = 0; b < nb; b++) {
            inc = fmax(inc, parts[((size_t)b * 3) * N + n]); sc = fmax(sc, parts[((size_t)b * 3 + 1) * N + n]); s += parts[((size_t)b * 3 + 2) * N + n];
        }
        for (int e = 0; e < c.n_e; e++) {
            double v1 = dDnew[((size_t)e * nav) * N + n], v0 = dDold[((size_t)e * nav) * N + n];
            for (int k = 0; k < KV; k++) { v1 += dDnew[((size_t)e * nav + na + k) * N + n]; v0 += dDold[((size_t)e * nav + na + k) * N + n]; }
            inc = fmax(inc, fabs(v1 - v0)); sc = fmax(sc, fabs(v1));
        }
        sig[n] = s;
        if (!(inc <= tol * sc)) bad = 1;
        worst = fmax(worst, ss_ratio(inc, sc));
    }
    __syncthreads();
    const size_t total = (size_t)c.G * N;
    for (size_t idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const size_t pt = idx / N;
        const int n = (int)(idx - pt * N), e = (int)(pt / na), a = (int)(pt - (size_t)e * na);
        dDnew[((size_t)e * nav + a) * N + n] -= Dss[pt] * sig[n];
    }
    ss_verdict(worst, bad, ctl);
}

// dY (n_het, N) column-major from the last step's per-block partials, blocks summed in order, plus the inputs' direct terms — the
// arithmetic of k_het_outputs at period 0: aggpart [block][2][N] (policy-weighted, grid-weighted), hxparts [block][NX][N].
__global__ void k_ss_jvp_out(int P, int n_hh, int n_het, int N, int nbf, const double *__restrict__ xhh, const double *__restrict__ dxhh,
                             const double *__restrict__ agg, const double *__restrict__ zd, const double *__restrict__ hxS,
                             const double *__restrict__ aggpart, const double *__restrict__ hxparts, double *__restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int NX = n_het > 2 ? n_het - 2 : 0;
    double dKD = 0.0, dAD = 0.0;
    for (int b = 0; b < nbf; b++) { dKD += aggpart[((size_t)b * 2) * N + n]; dAD += aggpart[((size_t)b * 2 + 1) * N + n]; }
    const double r = xhh[0], AD = agg[P], ZD = zd[0], MD = zd[P];
    const double *dx = dxhh + (size_t)n_hh * n;
    const double dtr = n_hh > 2 ? dx[2] : 0.0;
    out[(size_t)n_het * n] = dKD;
    if (n_het > 1) out[(size_t)n_het * n + 1] = out_dcons(r, dx[0], dx[1], dtr, AD, ZD, MD, dAD, dKD);
    for (int jx = 0; jx < NX; jx++) {
        double T = 0.0;
        for (int b = 0; b < nbf; b++) T += hxparts[((size_t)b * NX + jx) * N + n];
        out[(size_t)n_het * n + 2 + jx] = out_dhx(T, dx[0], dx[1], dtr, hxS + (size_t)jx * HX_NS);      // (the sums of period 0)
    }
}

// the distribution tangent [e][n_a + KV][N] -> (G, N) column-major, row 0 = the real row + its virtual rows
__global__ void k_ss_dist_out(const double *__restrict__ dD, int n_a, int n_e, int N, double *__restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, G = (size_t)n_a * n_e;
    if (idx >= G * N) return;
    const size_t n = idx / G, pt = idx - n * G;
    const int e = (int)(pt / n_a), a = (int)(pt - (size_t)e * n_a), nav = n_a + KV;
    double v = dD[((size_t)e * nav + a) * N + n];
    if (a == 0)
        for (int k = 0; k < KV; k++) v += dD[((size_t)e * nav + n_a + k) * N + n];
    out[idx] = v;
}

// ---- VJP ----------------------------------------------------------------------------------------------------------------------------
// agg_bar (n_het, M) column-major (or null) -> yb [4][M]: rows 0, 1 the policy variable's and consumption's cotangents, rows 2, 3
// the extra outputs'; absent rows are zero
__global__ void k_ss_y_in(const double *__restrict__ agg_bar, int n_het, int M, double *__restrict__ yb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * M) return;
    const int o = idx / M, m = idx - o * M;
    yb[idx] = (agg_bar && o < n_het) ? agg_bar[o + (size_t)n_het * m] : 0.0;
}

// g = sum_o ybar_o f_o + Dbar, centred: g -= (D_ss' g) 1 (the dropped constant meets 1's = 0 and contributes nothing). One block per
// column m; e0 and lam [G][M] both start as g. Fixed-order sums.
__global__ void __launch_bounds__(256) k_ss_cot_in(Consts c, Record R, const double *__restrict__ xhh, int NX, const double *__restrict__ yb,
                                                   const double *__restrict__ Dbar, const double *__restrict__ hxf, size_t PG, int M,
                                                   double *__restrict__ e0, double *__restrict__ lam) {
    __shared__ double red[16];
    __shared__ double tot_sh;
    const int m = blockIdx.x, G = c.G;
    const double r = xhh[0], w = xhh[1], tr = hh_tr(c, xhh, 0);
    const double y0 = yb[m], y1 = yb[M + m];
    double acc = 0.0;
    for (int pt = threadIdx.x; pt < G; pt += blockDim.x) {
        const int e = pt / c.n_a, ia = pt - e * c.n_a;
        const double pol = R.pol[pt], cons = ((1.0 + r) * c.a[ia] + (w * c.z[e] + tr)) - pol;
        double gv = pol * y0 + cons * y1;
        for (int o = 0; o < NX; o++) gv += hxf[o * PG + pt] * yb[(size_t)(2 + o) * M + m];
        if (Dbar) gv += Dbar[pt + (size_t)G * m];
        e0[(size_t)pt * M + m] = gv;
        acc += R.Dseq[pt] * gv;
    }
    const double tot = block_sum(acc, red, blockDim.x);
    if (threadIdx.x == 0) tot_sh = tot;
    __syncthreads();
    const double cen = tot_sh;
    for (int pt = threadIdx.x; pt < G; pt += blockDim.x) {
        const double gv = e0[(size_t)pt * M + m] - cen;
        e0[(size_t)pt * M + m] = gv;
        lam[(size_t)pt * M + m] = gv;
    }
}

// per-block maxima of two lane values (and, K = 3, the sum of a third) over the rows of a wave and the waves of a block, in a
// fixed order -> parts [block][K][MV]
template <typename VT, int K>
__device__ __forceinline__ void ss_adj_norms(VT inc, VT sc, VT sum, const AdjGeom &g, int ne, int e, int nl, int rl, int m, VT *__restrict__ parts) {
    __shared__ VT nred[K][16 * 16];
    inc = ss_rows_max(inc, g.NC); sc = ss_rows_max(sc, g.NC);
    if (K > 2) sum = adj_rows_sum(sum, g.NC);
    if (rl == 0) {
        nred[0][e * g.NC + nl] = inc; nred[1][e * g.NC + nl] = sc;
        if (K > 2) nred[K - 1][e * g.NC + nl] = sum;
    }
    __syncthreads();
    if (e == 0 && rl == 0 && m < g.MV) {
        for (int k = 1; k < ne; k++) {
            inc = ss_max(inc, nred[0][k * g.NC + nl]); sc = ss_max(sc, nred[1][k * g.NC + nl]);
            if (K > 2) sum = vadd(sum, nred[K - 1][k * g.NC + nl]);
        }
        parts[((size_t)blockIdx.x * K) * g.MV + m] = inc;
        parts[((size_t)blockIdx.x * K + 1) * g.MV + m] = sc;
        if (K > 2) parts[((size_t)blockIdx.x * K + 2) * g.MV + m] = sum;
    }
}

// One step e <- Lambda' e with lam += e (PB = false), or the policy cotangent from the converged lam (PB = true):
// adj_dist_body at period 0 with eIn in the tile — a block owns the target rows [r0, r1) and serves the sources the recorded lottery
// sends to them plus its share of the clamped prefix; every source row is written by exactly one block.
//   PB = false: eOut[j] = (1-w_j) U[lo_j] + w_j U[lo_j+1] - cen (U[0] - cen for a clamped source); lam[j] += eOut[j];
//               cen [MV]: D_ss'eIn of the last check — Lambda'(e - c 1) = Lambda'e - c 1, so the centring of the input is taken on
//               the output: a D_ss that is stationary only to the accuracy of the caller's steady state leaves a constant in e that
//               Lambda' never damps, and re-centring every step removes it (lam is defined up to a constant: only differences
//               of U enter pbar);
//               parts [block][3][MV]: max |eOut|, max |lam|, sum D_ss[j] eOut[j]
//   PB = true:  the tile holds lam (the TOTAL cotangent of D: g is its first term), and
//               pbar[j] = D_1[j] (yb0 - yb1 - sum_o f_c,o[j] ybx_o) + ig_j D_0[j] (U[lo_j+1] - U[lo_j])      (Sweep A's pbar line)
// dynamic LDS: VT tile[n_e][R + 2][NC] (slot R + 1 = row 0), double Pish[n_e * n_e]
template <typename VT, bool PB>
__global__ void __launch_bounds__(1024)
k_ss_lam(Consts c, Record R, AdjGeom g, const VT *__restrict__ eIn, VT *__restrict__ eOut, VT *__restrict__ lam, VT *__restrict__ parts,
         const SsCtl *__restrict__ ctl, const VT *__restrict__ cen, const VT *__restrict__ yb, int NX, const double *__restrict__ hxfc, size_t PG, VT *__restrict__ pbar) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
    if (!PB && ctl->stop) return;
    const AdjLane L = adj_lane(g);
    const int n = c.n_a, m = L.m;
    const size_t MV = g.MV, colb = (size_t)L.e * n;      // (period 0, column e) of the record
    const double *Dprev = R.Dseq + colb, *Dnext = R.Dseq + colb + c.G;
    const auto load = [&](int row) __attribute__((always_inline)) { return eIn[(colb + row) * MV + m]; };
    if constexpr (PB) {
        VT yd, yx[2];
        const auto begin = [&]() __attribute__((always_inline)) {
            vzero(yx[0]); vzero(yx[1]);
            yd = vsub(yb[m], yb[MV + m]);
#pragma unroll
            for (int o = 0; o < 2; o++)
                if (o < NX) yx[o] = yb[(size_t)(2 + o) * MV + m];
        };
        adj_dist_body<VT>(c, R, g, L, 0, adj_sh, load, begin, [&](int j, VT u0, VT u1, bool clamped) __attribute__((always_inline)) {
            VT ye = yd;
#pragma unroll
            for (int o = 0; o < 2; o++)
                if (o < NX) ye = vsub(ye, vmul(hxfc[o * PG + colb + j], yx[o]));
            pbar[(colb + j) * MV + m] = clamped ? vmul(Dnext[j], ye) : vadd(vmul(Dnext[j], ye), vmul(R.ig[colb + j] * Dprev[j], vsub(u1, u0)));
        });
    } else {
        VT inc, sc, dsum, cm;
        vzero(inc); vzero(sc); vzero(dsum);
        const auto begin = [&]() __attribute__((always_inline)) { cm = cen[m]; };
        adj_dist_body<VT>(c, R, g, L, 0, adj_sh, load, begin, [&](int j, VT u0, VT u1, bool clamped) __attribute__((always_inline)) {
            const size_t idx = (colb + j) * MV + m;
            double wj = 0.0;
            if (!clamped) wj = R.lw[colb + j];
            const VT v = vsub(clamped ? u0 : vadd(vmul(1.0 - wj, u0), vmul(wj, u1)), cm);
            const VT l = vadd(lam[idx], v);
            eOut[idx] = v;
            lam[idx] = l;
            inc = ss_max(inc, ss_abs(v)); sc = ss_max(sc, ss_abs(l)); dsum = vadd(dsum, vmul(Dprev[j], v));
        });
        ss_adj_norms<VT, 3>(inc, sc, dsum, g, c.n_e, L.e, L.nl, L.rl, m, parts);
    }
}

// One step nu <- B_V' nu + (P_V' pbar + Vbar): adj_egm_body at period 0 (neither first nor last) with the caller's
// cotangent of V_ss added to every new nu — nu is the TOTAL cotangent of dV, so gbar = pbar - v nu and the inputs' sums read it whole.
// partS, partM [block][3][MV]: sum sbar (s, z_e, 1) and sum nu (u + v a, v z_e, v) of the step, BOTH at the step's input nu: their
// reduction is xbar = P_x' (pbar - v nu) + M' nu = P_x' pbar + B_x' nu (Sweep B's, taken once). The two nu terms nearly cancel (the
// policy is an optimum), so a partM at nu_new next to a partS at nu leaves P_x' v (nu_new - nu) uncancelled: as large as the whole
// remaining tail of the loop, it doubled xbar's distance from the limit. parts [block][2][MV]: max |nu_new - nu|, max |nu_new|.
// dynamic LDS: VT tile[n_e][R][NC], double Pish[n_e * n_e], VT red[n_e][6][NC]
template <typename VT>
__global__ void __launch_bounds__(1024)
k_ss_nu(Consts c, Record R, AdjGeom g, const int *__restrict__ sb, const VT *__restrict__ nuIn, VT *__restrict__ nuOut, const VT *__restrict__ pbar,
        const VT *__restrict__ vbar, VT *__restrict__ partS, VT *__restrict__ partM, VT *__restrict__ parts, const SsCtl *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
    if (ctl->stop) return;
    const AdjLane L = adj_lane(g);
    const size_t MV = g.MV, colb = (size_t)L.e * c.n_a;
    VT inc, sc;
    vzero(inc); vzero(sc);
    adj_egm_body<VT>(c, R, g, L, 0, 0, true, true, sb, nuIn, pbar, adj_sh, partS, partM, [&](int i, VT mn) __attribute__((always_inline)) {
        const size_t idx = (colb + i) * MV + L.m;
        if (vbar) mn = vadd(mn, vbar[idx]);
        const VT old = nuIn[idx];
        inc = ss_max(inc, ss_abs(vsub(mn, old)));
        sc = ss_max(sc, ss_abs(mn));
        nuOut[idx] = mn;
        return old;      // (the sums weigh the nu sbar has read: see above)
    });
    ss_adj_norms<VT, 2>(inc, sc, inc, g, c.n_e, L.e, L.nl, L.rl, L.m, parts);
}

// xhh_bar (n_hh, M) column-major: the blocks' partials in block order (k_adj_out at one period), then the outputs' direct terms
// sum_o ybar_o d_o: consumption's (sum a D, sum z_e D, sum D) and the extra outputs' (Sa + Sr, Sz, S1) of period 0
__global__ void k_ss_xbar(int P, int n_hh, int M, int nb, int NX, const double *__restrict__ xhh, const double *__restrict__ partS,
                          const double *__restrict__ partM, const double *__restrict__ yb, const double *__restrict__ agg, const double *__restrict__ zd,
                          const double *__restrict__ hxS, double *__restrict__ xhh_bar) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    double s[3] = {0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nb; b++)
        for (int q = 0; q < 3; q++) { s[q] += partS[((size_t)b * 3 + q) * M + m]; mu[q] += partM[((size_t)b * 3 + q) * M + m]; }
    const double rho = 1.0 / (1.0 + xhh[0]), y1 = yb[M + m];
    double o[3] = {xbar_cons(mu[0], rho, s[0], y1, agg[P]), xbar_cons(mu[1], rho, s[1], y1, zd[0]), xbar_cons(mu[2], rho, s[2], y1, zd[P])};
    for (int jx = 0; jx < NX; jx++) xbar_hx(yb[(size_t)(2 + jx) * M + m], hxS + (size_t)jx * HX_NS, n_hh, o);
    double *out = xhh_bar + (size_t)n_hh * m;
    out[0] = o[0]; out[1] = o[1];
    if (n_hh > 2) out[2] = o[2];
}

}  // namespace hank
