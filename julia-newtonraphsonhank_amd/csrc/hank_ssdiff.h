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
//   VJP   e   <- Lambda' (e - (D'e) 1), lam += e  k_ss_lam:  the step of k_adj_dist at period 0, no output cotangent inside
//         nu  <- B_V' nu + (P_V' pbar + Vbar)     k_ss_nu:   the step of k_adj_egm at period 0, with a constant source
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
// the value this thread has just stored with st_mode (a write-through store): read where that store went
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
    if (n_het > 1) out[(size_t)n_het * n + 1] = (dx[0] * AD + dx[1] * ZD + dtr * MD + (1.0 + r) * dAD) - dKD;
    for (int jx = 0; jx < NX; jx++) {
        double T = 0.0;
        for (int b = 0; b < nbf; b++) T += hxparts[((size_t)b * NX + jx) * N + n];
        const double *S = hxS + (size_t)jx * HX_NS;      // period 0: Y, Sa, Sz, S1, Sr
        out[(size_t)n_het * n + 2 + jx] = T + dx[0] * (S[1] + S[4]) + dx[1] * S[2] + dtr * S[3];
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

// One step e <- Lambda' e with lam += e (PB = false), or the policy cotangent from the converged lam (PB = true): the arithmetic of
// k_adj_dist at period 0 — a block owns the target rows [r0, r1), mixes them with Pi through the LDS tile (U) and serves the sources
// the recorded lottery sends to them plus its share of the clamped prefix; every source row is written by exactly one block.
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
    const int NS = g.R + 2, n = c.n_a, ne = c.n_e;
    VT *tile = reinterpret_cast<VT *>(adj_sh);
    double *Pish = adj_sh + (size_t)ne * NS * g.NC * (sizeof(VT) / sizeof(double));
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC, RB = 64 >> g.lgNC;
    const int m = blockIdx.y * g.NC + nl;
    const bool mok = m < g.MV;
    const size_t MV = g.MV;
    const int r0 = blockIdx.x * g.R, r1 = min(r0 + g.R, n);
    for (int k = threadIdx.x; k < ne * ne; k += 64 * ne) Pish[k] = c.Pi[k];
    const size_t colb = (size_t)e * n;      // (period 0, column e) of the record
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB;
        if (slot < NS) {
            const int row = slot == g.R + 1 ? 0 : r0 + slot;
            VT v;
            vzero(v);
            if (mok && row <= r1 && row < n) v = eIn[((size_t)e * n + row) * MV + m];
            tile[((size_t)e * NS + slot) * g.NC + nl] = v;
        }
    }
    __syncthreads();
    VT U[ADJ_KS];
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB;
        vzero(U[k]);
        if (slot < NS)
            for (int e2 = 0; e2 < ne; e2++) U[k] = vadd(U[k], vmul(Pish[e + ne * e2], tile[((size_t)e2 * NS + slot) * g.NC + nl]));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB;
        if (slot < NS) tile[((size_t)e * NS + slot) * g.NC + nl] = U[k];
    }
    __syncthreads();
    VT inc, sc, dsum;
    vzero(inc); vzero(sc); vzero(dsum);
    if (mok) {
        VT cm;
        vzero(cm);
        if (!PB) cm = cen[m];
        const VT *Ue = tile + (size_t)e * NS * g.NC + nl;
        const double *Dprev = R.Dseq + colb, *Dnext = R.Dseq + colb + c.G;
        VT yd, yx[2];
        vzero(yd); vzero(yx[0]); vzero(yx[1]);
        if (PB) {
            yd = vsub(yb[m], yb[MV + m]);
#pragma unroll
            for (int o = 0; o < 2; o++)
                if (o < NX) yx[o] = yb[(size_t)(2 + o) * MV + m];
        }
        const int *st = R.start + (size_t)e * (n + 1);
        const int j0 = min(max(st[r0], 0), n), j1 = min(max(st[r1], 0), n);
        for (int j = j0 + rl; j < j1; j += RB) {
            const int sl = min(max(R.lo[colb + j] - r0, 0), g.R - 1);
            const VT u0 = Ue[(size_t)sl * g.NC], u1 = Ue[(size_t)(sl + 1) * g.NC];
            const size_t idx = (colb + j) * MV + m;
            if (PB) {
                const double gD = R.ig[colb + j] * Dprev[j], Dn = Dnext[j];
                VT ye = yd;
#pragma unroll
                for (int o = 0; o < 2; o++)
                    if (o < NX) ye = vsub(ye, vmul(hxfc[o * PG + colb + j], yx[o]));
                pbar[idx] = vadd(vmul(Dn, ye), vmul(gD, vsub(u1, u0)));
            } else {
                const double wj = R.lw[colb + j];
                const VT v = vsub(vadd(vmul(1.0 - wj, u0), vmul(wj, u1)), cm);
                const VT l = vadd(lam[idx], v);
                eOut[idx] = v;
                lam[idx] = l;
                inc = ss_max(inc, ss_abs(v)); sc = ss_max(sc, ss_abs(l)); dsum = vadd(dsum, vmul(Dprev[j], v));
            }
        }
        const int clo = min(max(R.clo[e], 0), n);
        const int c0 = (int)(((long long)clo * blockIdx.x) / gridDim.x), c1 = (int)(((long long)clo * (blockIdx.x + 1)) / gridDim.x);
        const VT U0 = Ue[(size_t)(g.R + 1) * g.NC];
        for (int j = c0 + rl; j < c1; j += RB) {
            const size_t idx = (colb + j) * MV + m;
            if (PB) {
                VT ye = yd;
#pragma unroll
                for (int o = 0; o < 2; o++)
                    if (o < NX) ye = vsub(ye, vmul(hxfc[o * PG + colb + j], yx[o]));
                pbar[idx] = vmul(Dnext[j], ye);
            } else {
                const VT v = vsub(U0, cm);
                const VT l = vadd(lam[idx], v);
                eOut[idx] = v;
                lam[idx] = l;
                inc = ss_max(inc, ss_abs(v)); sc = ss_max(sc, ss_abs(l)); dsum = vadd(dsum, vmul(Dprev[j], v));
            }
        }
    }
    if (!PB) ss_adj_norms<VT, 3>(inc, sc, dsum, g, ne, e, nl, rl, m, parts);
}

// One step nu <- B_V' nu + (P_V' pbar + Vbar): the arithmetic of k_adj_egm at period 0 (neither first nor last) with the caller's
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
    const int n = c.n_a, ne = c.n_e;
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC, RB = 64 >> g.lgNC, NS = g.R;
    VT *tile = reinterpret_cast<VT *>(adj_sh);
    double *Pish = adj_sh + (size_t)ne * NS * g.NC * (sizeof(VT) / sizeof(double));
    VT *red = reinterpret_cast<VT *>(Pish + ((ne * ne + 1) & ~1));
    const int m = blockIdx.y * g.NC + nl;
    const bool mok = m < g.MV;
    const size_t MV = g.MV;
    const int i0 = blockIdx.x * g.R;
    for (int k = threadIdx.x; k < ne * ne; k += 64 * ne) Pish[k] = c.Pi[k];
    const size_t colb = (size_t)e * n;
    const int *sbc = sb + (size_t)e * (n + 1);
    const double ze = c.z[e];
    VT sum[6], inc, sc;
#pragma unroll
    for (int q = 0; q < 6; q++) vzero(sum[q]);
    vzero(inc); vzero(sc);
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB, i = i0 + slot;
        VT sbar;
        vzero(sbar);
        if (mok && slot < g.R && i < n) {
            const int b1 = min(max(sbc[i], 0), n), b0 = i > 0 ? min(max(sbc[i - 1], 0), b1) : b1, b2 = min(max(sbc[i + 1], b1), n);
            const VT *pb = pbar + colb * MV + m, *mu = nuIn + colb * MV + m;
            for (int a = b0; a < b2; a += 2) {
                const bool two = a + 1 < b2;
                const int a1 = two ? a + 1 : a;
                const double w0 = a < b1 ? R.B[colb + a] : R.A[colb + a], w1 = a1 < b1 ? R.B[colb + a1] : R.A[colb + a1];
                const double v0 = R.v[colb + a], v1 = R.v[colb + a1];
                const VT g0 = vsub(pb[(size_t)a * MV], vmul(v0, mu[(size_t)a * MV])), g1 = vsub(pb[(size_t)a1 * MV], vmul(v1, mu[(size_t)a1 * MV]));
                sbar = vadd(sbar, vmul(w0, g0));
                if (two) sbar = vadd(sbar, vmul(w1, g1));
            }
            sum[0] = vadd(sum[0], vmul(R.s[colb + i], sbar));
            sum[1] = vadd(sum[1], vmul(ze, sbar));
            sum[2] = vadd(sum[2], sbar);
            sbar = vmul(R.kc[colb + i], sbar);
        }
        if (slot < g.R) tile[((size_t)e * NS + slot) * g.NC + nl] = sbar;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB, i = i0 + slot;
        if (mok && slot < g.R && i < n) {
            VT mn;
            vzero(mn);
            for (int e1 = 0; e1 < ne; e1++) mn = vadd(mn, vmul(Pish[e1 + ne * e], tile[((size_t)e1 * NS + slot) * g.NC + nl]));
            const size_t idx = (colb + i) * MV + m;
            if (vbar) mn = vadd(mn, vbar[idx]);
            const VT old = nuIn[idx];
            inc = ss_max(inc, ss_abs(vsub(mn, old)));
            sc = ss_max(sc, ss_abs(mn));
            nuOut[idx] = mn;
            const double u1 = R.u[colb + i], v1 = R.v[colb + i];
            sum[3] = vadd(sum[3], vmul(u1 + v1 * c.a[i], old));      // (the nu sbar has read: see above)
            sum[4] = vadd(sum[4], vmul(v1 * ze, old));
            sum[5] = vadd(sum[5], vmul(v1, old));
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const VT v = adj_rows_sum(sum[q], g.NC);
        if (rl == 0) red[((size_t)e * 6 + q) * g.NC + nl] = v;
    }
    __syncthreads();
    for (int q = e; q < 6; q += ne) {
        VT v;
        vzero(v);
        for (int e1 = rl; e1 < ne; e1 += RB) v = vadd(v, red[((size_t)e1 * 6 + q) * g.NC + nl]);
        v = adj_rows_sum(v, g.NC);
        if (rl == 0 && mok) {
            if (q < 3) partS[(((size_t)blockIdx.x) * 3 + q) * MV + m] = v;
            else partM[(((size_t)blockIdx.x) * 3 + (q - 3)) * MV + m] = v;
        }
    }
    ss_adj_norms<VT, 2>(inc, sc, inc, g, ne, e, nl, rl, m, parts);
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
    double o[3] = {(mu[0] - rho * s[0]) + y1 * agg[P], (mu[1] - rho * s[1]) + y1 * zd[0], (mu[2] - rho * s[2]) + y1 * zd[P]};
    for (int jx = 0; jx < NX; jx++) {
        const double y = yb[(size_t)(2 + jx) * M + m];
        const double *S = hxS + (size_t)jx * HX_NS;
        o[0] += y * (S[1] + S[4]); o[1] += y * S[2]; o[2] += y * S[3];
    }
    double *out = xhh_bar + (size_t)n_hh * m;
    out[0] = o[0]; out[1] = o[1];
    if (n_hh > 2) out[2] = o[2];
}

}  // namespace hank
