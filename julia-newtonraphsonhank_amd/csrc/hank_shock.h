// hank_shock.h — a PATH of the discount factor, beta_t, in the household block: the primal sweep at a path, the tangent seed of
// d beta_t in the backward tangent sweep and its transpose in Sweep B (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock,
// hank_fake_news_shock).
//
// beta enters the EGM step once (egm_X_point, hank_kernels.h; KrusellSmith.jl:59-62): cm = (beta E)^ex, ex = -1/gamma, with
// E = E_t[V_{t+1}]. DATING: beta_t is the factor in period t's Euler equation, u'(c_t) = beta_t E_t[V_{t+1}], t = 0 .. P-1, so
// beta_{P-1} multiplies the expectation of the terminal V_P. It belongs to the X half of period t (the knots s_t).
//
//   primal     the X half of period t' runs with a period-local copy of Consts whose beta is beta_{t'}: egm_X / egm_step_body are
//              called unchanged, so the textbook kc and diet_kc both stay consistent with the s that is recorded
//   tangent    d s_t / d beta_t = rho_t ex cm_t / beta_t =: kb_t[e,i], cm rebuilt from the recorded s as diet_kc does,
//              cm = (s opr + wz_tr) - xa. The seed is a rank-one update of the knots' tangent of EVERY period,
//              ds_t[e,i,n] += kb_t[e,i] dbeta_t[n], right after the launch of k_tan_back that produced ds_t (the boundary's
//              k_bnd_seed_back does this once, at t = P-1). k_tan_back itself is launched unchanged.
//   transpose  beta_bar_t[m] = sum_{e,i} kb_t[e,i] sbar_t[e,i,m], sbar_t the knots' cotangent of Sweep B at period t, gathered from
//              the same pbar_t, mu_t and bracket segments as k_adj_egm (and k_bnd_vend) gather it, in the same row order. Per block
//              partials, then k_reduce_parts: no atomics, every sum in a fixed order.
// Nothing is added to the record: kb comes from s and the period's inputs.
#pragma once
#include "hank_kernels.h"

namespace hank {

// kb = d s / d beta at one point, from the recorded knot s (rho = 1/(1+r), opr = 1 + r, wz_tr = w z_e + tr, xa = the grid point)
__device__ __forceinline__ double shk_kb(const Consts &c, double beta_t, double s, double rho, double opr, double wz_tr, double xa) {
    const double cm = (s * opr + wz_tr) - xa;
    return rho * ((-1.0 / c.gamma) * (cm / beta_t));
}

// ---- primal: k_egm_X and k_egm_step with beta taken from the path ---------------------------------------------------------------
// block, grid and dynamic LDS of k_egm_X; t: the period whose X half this is
__global__ void k_shk_egm_X(Consts c, const double *__restrict__ beta, const double *Vin, const double *xt, double *s_out, double *kc_out, int *err, int t) {
    extern __shared__ double sh[];
    Consts cb = c;
    cb.beta = beta[t];
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = blockIdx.x * RBP + row;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += blockDim.x) Pish[k] = c.Pi[k];
    if (a < c.n_a) Vsh[e * RBP + row] = Vin[e * c.n_a + a];
    __syncthreads();
    if (a < c.n_a) egm_X(cb, Vsh, Pish, row, a, e, xt[0], xt[1], c.n_hh > 2 ? xt[2] : 0.0, &s_out[e * c.n_a + a], &kc_out[e * c.n_a + a], err, t);
}
// Y of period t (no beta in it), then X of period t' = t-1 with beta_{t-1}
__global__ void k_shk_egm_step(Consts c, Record R, const double *xhh, const double *__restrict__ beta, int t, int *err) {
    extern __shared__ double sh[];
    Consts cb = c;
    cb.beta = beta[t > 0 ? t - 1 : 0];
    egm_step_body(cb, R, xhh, t, err, blockIdx.x, sh);
}

// ---- tangent ---------------------------------------------------------------------------------------------------------------------
// dbeta (P, N) column-major -> [P][N]
__global__ void k_shk_in(const double *__restrict__ dbeta, int P, int N, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int t = idx / N, n = idx - t * N;
    out[idx] = dbeta[(size_t)t + (size_t)P * n];
}

// The seed of period t, behind the launch of k_tan_back that produced the knots' tangent ds_t [e][n_a][N]. One thread per
// (row, direction), direction fastest; it walks the n_e columns of its row. db: dbeta_t [N]. grid ceil(n_a N / 256).
__global__ void __launch_bounds__(256) k_shk_seed_back(Consts c, Record R, const double *__restrict__ xhh, const double *__restrict__ beta, int t,
                                                       const double *__restrict__ db, size_t N, double *__restrict__ ds) {
    const size_t cnt = (size_t)c.n_a * N, j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int i = (int)(j / N);
    const double d = db[j - (size_t)i * N];
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t), rho = 1.0 / (1.0 + r), bt = beta[t], xa = c.a[i];
    const double *s = R.s + (size_t)t * c.G;
    for (int e = 0; e < c.n_e; e++) {
        const double kb = shk_kb(c, bt, s[(size_t)e * c.n_a + i], rho, 1.0 + r, w * c.z[e] + tr, xa);
        ds[(size_t)e * cnt + j] += kb * d;
    }
}

// ---- transpose -------------------------------------------------------------------------------------------------------------------
// beta_bar_t's per-block partials at period t of Sweep B (behind, or in front of, k_adj_egm's launch of that period: it reads the
// same mu_t = muIn and pbar_t and writes neither). A block owns the KNOT rows [i0, i0 + RO) of every column — RO the row count
// hank_vjp's blocks own at this width (AdjGeom::R) — and MC (a power of two <= 64) cotangent columns, column fastest across the
// lanes; the SHK_BT / MC slots of a column stride over the block's (e, i) items, e outer — 1024 threads, so that a slot gathers two or
// three knots, not eleven: the gather is a chain of dependent loads — and are combined through LDS in two steps of a fixed order
// (slot s < 32 sums the slots s, s + 32, ..; the column's first slot sums those). first: t = 0, mu_0 = 0. part [nb][M] of period t.
// grid (nb, ceil(M / MC)), block SHK_BT.
constexpr int SHK_BT = 1024;
__global__ void __launch_bounds__(SHK_BT) k_shk_bbar(Consts c, Record R, const double *__restrict__ xhh, const double *__restrict__ beta, int RO, int MC, int t,
                                                  int first, const int *__restrict__ sb, const double *__restrict__ muIn, const double *__restrict__ pbar,
                                                  int M, double *__restrict__ part) {
    __shared__ double red[SHK_BT];
    const int n = c.n_a, ne = c.n_e;
    const int ml = threadIdx.x & (MC - 1), slot = threadIdx.x / MC, nslot = SHK_BT / MC;
    const int m = blockIdx.y * MC + ml, i0 = blockIdx.x * RO;
    const int rows = min(RO, n - i0);
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t), rho = 1.0 / (1.0 + r), bt = beta[t];
    double acc = 0.0;
    if (m < M) {
        for (int it = slot; it < ne * rows; it += nslot) {
            const int e = it / rows, i = i0 + (it - e * rows);
            const size_t colb = (size_t)t * c.G + (size_t)e * n;
            const int *sbc = sb + ((size_t)t * ne + e) * (n + 1);
            const int b1 = min(max(sbc[i], 0), n), b0 = i > 0 ? min(max(sbc[i - 1], 0), b1) : b1, b2 = min(max(sbc[i + 1], b1), n);
            double sbar = 0.0;
            for (int a = b0; a < b2; a++) {
                double g = pbar[(colb + a) * M + m];
                if (!first) g -= R.v[colb + a] * muIn[((size_t)e * n + a) * M + m];
                sbar += (a < b1 ? R.B[colb + a] : R.A[colb + a]) * g;
            }
            acc += shk_kb(c, bt, R.s[colb + i], rho, 1.0 + r, w * c.z[e] + tr, c.a[i]) * sbar;
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
