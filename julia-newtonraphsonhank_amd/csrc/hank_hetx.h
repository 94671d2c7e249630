// Heterogeneous outputs that are NOT affine in the policy: Value = (1+r) c^-gamma (KrusellSmith.jl:80, the value_current of
// the reference's own ValueFunction) and UCE = z_e c^-gamma, c = (1+r) a + w z_e + tr - a' the budget residual (the c_grid of
// KrusellSmith.jl:79). The reference dots every key of the plugin's NamedTuple with the same post-transition D_t
// (BackwardIteration.jl:99-112, ForwardIteration.jl:303-307):
//     Y_t  = sum f_t D_t
//     dY_t = sum f_t dD_t - sum f_c,t D_t da'_t  +  dr_t (Sa_t + Sr_t) + dw_t Sz_t + dtr_t S1_t
//     Sa_t = sum D_t f_c a, Sz_t = sum D_t f_c z_e, S1_t = sum D_t f_c, Sr_t = sum D_t df/dr|_c   (f_c = df/dc = -gamma f / c)
// The last four do not depend on the direction (k_hx_record, one block per period and output: once per primal record, for the
// tangent side here and the transposed sweeps of hank_adjoint.h alike — ensure_hx_record, hank_hip.hip). The first two need the
// distribution tangent dD_t of every direction: k_hx_mid / k_hx_mix re-run the forward tangent recurrence (ForwardIteration.jl:
// 37-99 under the Dual) from the policy partials the last tangent sweep left (any family, exported to one layout) and the
// lottery record of the primal, as a deterministic gather over the source segments of each target row (no atomics: the same
// inputs give the same bits). Everything runs after the sweeps, so the sweep kernels themselves are untouched.
#pragma once
#include "hank_kernels.h"

namespace hank {

constexpr int HX_ROWS = 256;

// f and its partials at one grid point for output j (2: Value, 3: UCE)
__device__ inline void hx_f(int j, double gamma, double r, double z, double cons, double &f, double &fc, double &fr) {
    const double u = pow(cons, -gamma);
    f = j == 2 ? (1.0 + r) * u : z * u;
    fr = j == 2 ? u : 0.0;
    fc = -gamma * f / cons;
}

// grid (P, NX): f and f_c of every point (rec [jx][t][pt], 2 arrays) and the direction-independent sums (S [t][jx][HX_NS]). Its one
// caller passes the family's count of extra outputs; the readers index S with that count as the stride, whatever they ask for.
__global__ void __launch_bounds__(256) k_hx_record(Consts c, Record R, const double *__restrict__ xhh, int NX,
                                                   double *__restrict__ fr_out, double *__restrict__ fc_out, double *__restrict__ S) {
    __shared__ double red[16];
    const int t = blockIdx.x, jx = blockIdx.y, j = 2 + jx;
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = c.n_hh > 2 ? xhh[c.n_hh * t + 2] : 0.0;
    const size_t base = (size_t)t * c.G, rb = ((size_t)jx * c.P + t) * c.G;
    double acc[HX_NS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int pt = threadIdx.x; pt < c.G; pt += blockDim.x) {
        const int e = pt / c.n_a, ia = pt - e * c.n_a;
        const double a = c.a[ia], z = c.z[e];
        const double cons = (1.0 + r) * a + w * z + tr - R.pol[base + pt];
        double f, fc, fr;
        hx_f(j, c.gamma, r, z, cons, f, fc, fr);
        fr_out[rb + pt] = f;
        fc_out[rb + pt] = fc;
        const double D = R.Dseq[base + c.G + pt];     // post-transition D_t
        acc[0] += f * D; acc[1] += fc * D * a; acc[2] += fc * D * z; acc[3] += fc * D; acc[4] += fr * D;
    }
    for (int k = 0; k < HX_NS; k++) {
        const double tot = block_sum(acc[k], red, blockDim.x);
        if (threadIdx.x == 0) S[((size_t)t * NX + jx) * HX_NS + k] = tot;
    }
}

// period t, lottery half: mid[n][pt] = the tangent of the pre-mixing distribution. grid (ceil(G / HX_ROWS), N).
// dpc: the policy partials [n][t][pt]; dDp: dD_{t-1} [n][pt] (ignored at t = 0: D_0 is the fixed initial distribution).
__global__ void __launch_bounds__(HX_ROWS) k_hx_mid(Consts c, Record R, int t, const double *__restrict__ dpc,
                                                    const double *__restrict__ dDp, double *__restrict__ mid) {
    const int pt = blockIdx.x * HX_ROWS + threadIdx.x, n = blockIdx.y;
    if (pt >= c.G) return;
    const int na = c.n_a, e = pt / na, r = pt - e * na;
    const size_t base = (size_t)t * c.G + (size_t)e * na;
    const double *lw = R.lw + base, *ig = R.ig + base, *Dp = R.Dseq + base;
    const double *dp = dpc + ((size_t)n * c.P + t) * c.G + (size_t)e * na;
    const double *dd = dDp + (size_t)n * c.G + (size_t)e * na;
    const bool first = t == 0;
    const int *st = R.start + ((size_t)t * c.n_e + e) * (na + 1);
    const int st1 = st[r], st2 = st[r + 1], st0 = r > 0 ? st[r - 1] : st1;
    double acc = 0.0;
    for (int k = st0; k < st1; k++) acc += (first ? 0.0 : lw[k] * dd[k]) + dp[k] * ig[k] * Dp[k];
    for (int k = st1; k < st2; k++) acc += (first ? 0.0 : (1.0 - lw[k]) * dd[k]) - dp[k] * ig[k] * Dp[k];
    if (r == 0 && !first) {      // the mass point at the first grid point (ig = 0 there: no policy partial)
        const int clo = R.clo[(size_t)t * c.n_e + e];
        for (int k = 0; k < clo; k++) acc += dd[k];
    }
    mid[(size_t)n * c.G + pt] = acc;
}

// period t, mixing half and the in-period reductions: dD_t[n][e2][r] = sum_e mid[n][e][r] Pi[e][e2], and per output
// sum f dD_t - f_c D_t da'_t over the block's rows -> parts [n][t][block][jx]. grid (nbr = ceil(n_a / HX_ROWS), N).
__global__ void __launch_bounds__(HX_ROWS) k_hx_mix(Consts c, Record R, int t, int NX, const double *__restrict__ dpc,
                                                    const double *__restrict__ mid, const double *__restrict__ f,
                                                    const double *__restrict__ fc, double *__restrict__ dD, double *__restrict__ parts) {
    __shared__ double red[16];
    const int r = blockIdx.x * HX_ROWS + threadIdx.x, n = blockIdx.y, na = c.n_a;
    double acc[2] = {0.0, 0.0};
    if (r < na) {
        const double *m = mid + (size_t)n * c.G;
        const double *dp = dpc + ((size_t)n * c.P + t) * c.G;
        const double *D = R.Dseq + (size_t)(t + 1) * c.G;
        for (int e2 = 0; e2 < c.n_e; e2++) {
            double s = 0.0;
            for (int e = 0; e < c.n_e; e++) s += m[(size_t)e * na + r] * c.Pi[e + c.n_e * e2];
            const size_t pt = (size_t)e2 * na + r;
            dD[(size_t)n * c.G + pt] = s;
            for (int jx = 0; jx < NX; jx++) {
                const size_t q = ((size_t)jx * c.P + t) * c.G + pt;
                acc[jx] += f[q] * s - fc[q] * D[pt] * dp[pt];
            }
        }
    }
    for (int jx = 0; jx < NX; jx++) {
        const double tot = block_sum(acc[jx], red, HX_ROWS);
        if (threadIdx.x == 0) parts[(((size_t)n * c.P + t) * gridDim.x + blockIdx.x) * NX + jx] = tot;
    }
}

// parts [n][t][nbr][jx] -> T [n][t][jx], blocks summed in order
__global__ void k_hx_reduce(const double *__restrict__ parts, int nbr, int NX, size_t count, double *__restrict__ T) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count) return;
    const size_t nt = idx / NX, jx = idx - nt * NX;
    double s = 0.0;
    for (int b = 0; b < nbr; b++) s += parts[(nt * nbr + b) * NX + jx];
    T[idx] = s;
}

// ---- n_het heterogeneous outputs ---------------------------------------------------------------------------------------------
// ForwardIteration aggregates EVERY heterogeneous variable with the same D_t: agg_j[t] = dot(vec(policy_j[t]), D_t)
// (ForwardIteration.jl:303-307; BackwardIteration.jl:99-112 keeps one policy sequence per variable). Output 0 is the policy variable
// of the endogenous dimension (the savings a', KD / A). Output 1 is consumption, the budget residual c = (1+r_t) a + w_t z_e + tr_t
// - a' (KrusellSmith.jl:80): its aggregate is affine in what the sweeps already reduce (out_cons, out_dcons: hank_device.h; ZD_t,
// MD_t carry no partials: see hank_set_boundary; under a dD_0 seed of hank_jvp_boundary they do, and k_bnd_cons adds them behind
// this kernel). Outputs 2, 3 (Value, UCE) are the sums above (out_dhx).
// agg (P, 2) and dagg (P, 2 N) as the sweeps leave them -> out_agg (P, n_het), out_dagg (P, n_het, N) column-major. hxS: the
// record's sums [t][SX][HX_NS] (SX: the outputs the record holds); hxT: the call's in-period sums [n][t][NX].
__global__ void k_het_outputs(int P, int n_hh, int n_het, int SX, int N, const double *__restrict__ xhh, const double *__restrict__ dxhh,
                              const double *__restrict__ agg, const double *__restrict__ dagg, const double *__restrict__ zd,
                              const double *__restrict__ hxS, const double *__restrict__ hxT,
                              double *__restrict__ out_agg, double *__restrict__ out_dagg) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)P * (N + 1)) return;
    const int t = (int)(idx % P), n = (int)(idx / P) - 1;
    const int NX = n_het > 2 ? n_het - 2 : 0;
    const double r = xhh[n_hh * t], w = xhh[n_hh * t + 1], tr = n_hh > 2 ? xhh[n_hh * t + 2] : 0.0;
    const double KD = agg[t], AD = agg[P + t], ZD = zd[t], MD = zd[P + t];
    if (n < 0) {
        if (!out_agg) return;
        out_agg[t] = KD;
        if (n_het > 1) out_agg[P + t] = out_cons(r, w, tr, AD, ZD, MD, KD);
        for (int jx = 0; jx < NX; jx++) out_agg[(size_t)(2 + jx) * P + t] = hxS[((size_t)t * SX + jx) * HX_NS];
        return;
    }
    if (!out_dagg) return;
    const double dKD = dagg[(size_t)n * P + t], dAD = dagg[((size_t)N + n) * P + t];
    const double *dx = dxhh + ((size_t)n * P + t) * n_hh;
    const double dtr = n_hh > 2 ? dx[2] : 0.0;
    out_dagg[((size_t)n * n_het) * P + t] = dKD;
    if (n_het > 1) out_dagg[((size_t)n * n_het + 1) * P + t] = out_dcons(r, dx[0], dx[1], dtr, AD, ZD, MD, dAD, dKD);
    for (int jx = 0; jx < NX; jx++)
        out_dagg[((size_t)n * n_het + 2 + jx) * P + t] = out_dhx(hxT[((size_t)n * P + t) * NX + jx], dx[0], dx[1], dtr, hxS + ((size_t)t * SX + jx) * HX_NS);
}

}  // namespace hank
