// hank_income.h — an additive income PATH by productivity state, y_t[e], in the household block: the primal sweep at a path, the
// tangent seed of d y_t[e] in the backward tangent sweep, its transpose in Sweep B and the direct term in consumption
// (hank_set_income_path, hank_jvp_income, hank_vjp_income, hank_fake_news_income, hank_get_het_outputs_income).
//
// The budget gains one term per column (KrusellSmith.jl:59-62, :66-80): c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e], t = 0 .. P-1.
// y_t[e] enters wherever tr_t enters, per column: the X half of period t (the knots s_t and, under the record diet, the kc rebuilt
// from them) and the Y half of period t (the consumption cg behind u, v and the value).
//
//   primal     a thread of the primal kernels knows its column e: it hands tr_t + y_t[e] to the unchanged egm_X / egm_Y where they
//              take tr_t, so s, kc (textbook and diet_kc), u, v (textbook and diet_v) stay consistent with each other. With y = 0 the
//              sum is tr_t itself: the bits of no path.
//   tangent    the launch family's tangent kernels read kc, s, u, v from the record, so only the seed is new. With dV_t[e2] gaining
//              v_t[e2] dy_t[e2] (k_tan_Y) and ds_t[e] gaining -rho_t dy_t[e] (k_tan_X), the knots' tangent of period t, as the launch
//              of k_tan_back that produced it left it, gains
//                  ds_t[e,i,n] += kc_t[e,i] sum_{e2} Pi[e,e2] v_{t+1}[e2,i] dy_{t+1}[e2,n]  -  rho_t dy_t[e,n]
//              (the first term is absent at t = P-1: the terminal value is fixed). k_tan_back itself is launched unchanged.
//   transpose  y_bar_t[e,m] = sum_i (v_t[e,i] mu_t[e,i,m] - rho_t sbar_t[e,i,m]) + m_t[e] yb1_t[m]: sbar_t the knots' cotangent of
//              Sweep B at period t, gathered as k_shk_bbar gathers it; mu_t the cotangent of dV_t that Sweep B carries into period t
//              (mu_0 = 0); m_t[e] = sum_a D_t[e,a] the column masses of the post-transition distribution, which weigh the direct
//              term of consumption, C_t += sum_e y_t[e] m_t[e]. Per block partials, then k_reduce_parts: no atomics, a fixed order.
// Nothing is added to the record; the column masses are one small reduction per primal, kept in the context.
#pragma once
#include "hank_kernels.h"

namespace hank {

constexpr int INC_NE = 16;      // the context's bound on n_e (hank_create)

// ---- primal: k_egm_X and k_egm_step with tr_t + y_t[e] in tr_t's place ------------------------------------------------------------
// y [P][n_e] (the caller's (n_e, P) column-major as it is). block, grid and dynamic LDS of k_egm_X; t: the period whose X half this is
__global__ void k_inc_egm_X(Consts c, const double *__restrict__ y, const double *Vin, const double *xt, double *s_out, double *kc_out, int *err, int t) {
    extern __shared__ double sh[];
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = blockIdx.x * RBP + row;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += blockDim.x) Pish[k] = c.Pi[k];
    if (a < c.n_a) Vsh[e * RBP + row] = Vin[e * c.n_a + a];
    __syncthreads();
    if (a < c.n_a)
        egm_X(c, Vsh, Pish, row, a, e, xt[0], xt[1], (c.n_hh > 2 ? xt[2] : 0.0) + y[(size_t)t * c.n_e + e], &s_out[e * c.n_a + a], &kc_out[e * c.n_a + a], err, t);
}
// egm_step_body (hank_kernels.h) with the path: Y of period t with y_t[e], then X of period t-1 with y_{t-1}[e]
__device__ inline void inc_step_body(const Consts &c, const Record &R, const double *xhh, const double *__restrict__ y, int t, int *err, int bid, double *sh) {
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int nthr = RBP * c.n_e;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = bid * RBP + row;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += nthr) Pish[k] = c.Pi[k];
    const size_t base = (size_t)t * c.G;
    if (a < c.n_a) {
        const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t) + y[(size_t)t * c.n_e + e];
        const int guess = (t + 1 < c.P) ? R.ib[base + c.G + (size_t)e * c.n_a + a] : -1;
        const YOut o = egm_Y(c, R.s + base + (size_t)e * c.n_a, a, e, r, w, tr, err, t, guess);
        const size_t off = base + (size_t)e * c.n_a + a;
        R.pol[off] = o.g; R.ib[off] = o.ib; R.A[off] = o.A;
        R.B[off] = o.B; R.u[off] = o.u; R.v[off] = o.v;
        Vsh[e * RBP + row] = o.V;
    }
    lds_barrier();
    if (t > 0 && a < c.n_a) {
        const double r1 = xhh[c.n_hh * (t - 1)], w1 = xhh[c.n_hh * (t - 1) + 1], tr1 = hh_tr(c, xhh, t - 1) + y[(size_t)(t - 1) * c.n_e + e];
        const size_t off1 = base - c.G + (size_t)e * c.n_a + a;
        egm_X(c, Vsh, Pish, row, a, e, r1, w1, tr1, &R.s[off1], &R.kc[off1], err, t - 1);
    }
}
__global__ void k_inc_egm_step(Consts c, Record R, const double *xhh, const double *__restrict__ y, int t, int *err) {
    extern __shared__ double sh[];
    inc_step_body(c, R, xhh, y, t, err, blockIdx.x, sh);
}

// ---- the column masses m_t[e] = sum_a D_t[e,a] of the post-transition distribution (R.Dseq's row t + 1) --------------------------
// one block of 256 per (e, t), a fixed order (block_sum): the same record gives the same bits. m [P][n_e]. grid (n_e, P).
__global__ void __launch_bounds__(256) k_inc_mass(Consts c, Record R, double *__restrict__ m) {
    __shared__ double red[16];
    const int e = blockIdx.x, t = blockIdx.y;
    const double *D = R.Dseq + (size_t)(t + 1) * c.G + (size_t)e * c.n_a;
    double s = 0.0;
    for (int a = threadIdx.x; a < c.n_a; a += 256) s += D[a];
    const double tot = block_sum(s, red, 256);
    if (threadIdx.x == 0) m[(size_t)t * c.n_e + e] = tot;
}

// ---- tangent ---------------------------------------------------------------------------------------------------------------------
// dy (n_e, P, N) column-major -> [P][n_e][N]
__global__ void k_inc_in(const double *__restrict__ dy, int ne, int P, int N, double *__restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)P * ne * N) return;
    const size_t te = idx / N, n = idx - te * N, t = te / ne, e = te - t * ne;
    out[idx] = dy[e + (size_t)ne * (t + (size_t)P * n)];
}

// The seed of period t, behind the launch of k_tan_back that produced the knots' tangent ds_t [e][n_a][N]. One thread per (row,
// direction), direction fastest; it walks the n_e columns of its row. dyt: dy_t [n_e][N]; dyn: dy_{t+1} [n_e][N], or null at t = P-1.
// lds: Pi and the two dy slices are staged in dynamic LDS (n_e n_e + 2 n_e N doubles; the host says whether they fit), read from
// global memory otherwise. A zero seed adds nothing — not even +0 to a -0 — so zero directions leave hank_jvp's bits.
// grid ceil(n_a N / 256).
__global__ void __launch_bounds__(256) k_inc_seed_back(Consts c, Record R, const double *__restrict__ xhh, int t, const double *__restrict__ dyt,
                                                       const double *__restrict__ dyn, size_t N, int lds, double *__restrict__ ds) {
    extern __shared__ double inc_sh[];
    const int ne = c.n_e;
    const size_t eN = (size_t)ne * N;
    const double *Pi = c.Pi, *d0 = dyt, *d1 = dyn;
    if (lds) {
        double *Psh = inc_sh, *s0 = inc_sh + ne * ne, *s1 = s0 + eN;
        for (int k = threadIdx.x; k < ne * ne; k += 256) Psh[k] = c.Pi[k];
        for (size_t k = threadIdx.x; k < eN; k += 256) { s0[k] = dyt[k]; if (dyn) s1[k] = dyn[k]; }
        __syncthreads();
        Pi = Psh; d0 = s0; d1 = s1;
    }
    const size_t cnt = (size_t)c.n_a * N, j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int i = (int)(j / N);
    const size_t n = j - (size_t)i * N;
    const double rho = 1.0 / (1.0 + xhh[c.n_hh * t]);
    // every column's loads first, in registers (the loops are unrolled to the bound on n_e): walking the columns with a load, a wait
    // and a store each is a chain of n_e round trips (measured: 20 us a period at 2000x11, N = 32)
    double q[INC_NE], kcv[INC_NE], dsv[INC_NE];      // q: v_{t+1}[e2,i] dy_{t+1}[e2,n]
#pragma unroll
    for (int e = 0; e < INC_NE; e++) {
        q[e] = (dyn && e < ne) ? R.v[(size_t)(t + 1) * c.G + (size_t)e * c.n_a + i] * d1[(size_t)e * N + n] : 0.0;
        kcv[e] = e < ne ? R.kc[(size_t)t * c.G + (size_t)e * c.n_a + i] : 0.0;
        dsv[e] = e < ne ? ds[(size_t)e * cnt + j] : 0.0;
    }
#pragma unroll
    for (int e = 0; e < INC_NE; e++) {
        if (e < ne) {
            double acc = 0.0;
#pragma unroll
            for (int e2 = 0; e2 < INC_NE; e2++)
                if (e2 < ne) acc += Pi[e + ne * e2] * q[e2];
            const double add = kcv[e] * acc - rho * d0[(size_t)e * N + n];
            if (add != 0.0) ds[(size_t)e * cnt + j] = dsv[e] + add;
        }
    }
}

// ---- the direct term of consumption ---------------------------------------------------------------------------------------------
// behind k_het_outputs (n_het = 2): out_agg (P, 2) gains sum_e y_t[e] m_t[e] in its consumption column, out_dagg (P, 2, N) gains
// sum_e dy_t[e,n] m_t[e], e ascending. y [P][n_e] or null (no path: nothing to add to the level); dy (n_e, P, N) column-major or null.
// One thread per (t, n), n = -1 the level. Either output may be null.
__global__ void k_inc_cons(int P, int ne, int N, const double *__restrict__ y, const double *__restrict__ dy, const double *__restrict__ m,
                           double *__restrict__ out_agg, double *__restrict__ out_dagg) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)P * (N + 1)) return;
    const int t = (int)(idx % P), n = (int)(idx / P) - 1;
    const double *mt = m + (size_t)t * ne;
    double s = 0.0;
    if (n < 0) {
        if (!out_agg || !y) return;
        for (int e = 0; e < ne; e++) s += y[(size_t)t * ne + e] * mt[e];
        out_agg[P + t] += s;
        return;
    }
    if (!out_dagg || !dy) return;
    for (int e = 0; e < ne; e++) s += dy[e + (size_t)ne * (t + (size_t)P * n)] * mt[e];
    out_dagg[((size_t)n * 2 + 1) * P + t] += s;
}

// ---- transpose -------------------------------------------------------------------------------------------------------------------
// y_bar_t's per-block partials at period t of Sweep B (beside k_adj_egm's launch of that period: it reads the same mu_t = muIn and
// pbar_t and writes neither). A block owns the rows [i0, i0 + RO) of every column — RO the row count hank_vjp's blocks own at this
// width (AdjGeom::R) — and MC (a power of two <= INC_MC) cotangent columns, column fastest across the lanes. The INC_BT / MC slots of
// a cotangent column stride over the block's (e, i) items, e outer, as k_shk_bbar's do, so the work is even whatever n_e is; an item
// gathers sbar_t[e,i] as k_shk_bbar does and leaves v_t[e,i] mu_t[e,i] - rho_t sbar_t[e,i] in its own LDS cell. Column e's first
// slot then sums that column's cells in row order. first: t = 0, mu_0 = 0.
// part [nb][n_e][M] of period t. grid (nb, ceil(M / MC)), block INC_BT, dynamic LDS n_e RO MC doubles (inc_ybar_lds).
constexpr int INC_BT = 1024, INC_MC = 32;
__host__ __device__ inline size_t inc_ybar_lds(const Consts &c, int RO, int MC) { return sizeof(double) * (size_t)c.n_e * RO * MC; }
__global__ void __launch_bounds__(INC_BT) k_inc_ybar(Consts c, Record R, const double *__restrict__ xhh, int RO, int MC, int t, int first,
                                                  const int *__restrict__ sb, const double *__restrict__ muIn, const double *__restrict__ pbar, int M,
                                                  double *__restrict__ part) {
    extern __shared__ double inc_cell[];      // [e][RO][MC]
    const int n = c.n_a, ne = c.n_e;
    const int ml = threadIdx.x & (MC - 1), slot = threadIdx.x / MC, nslot = INC_BT / MC;
    const int m = blockIdx.y * MC + ml, i0 = blockIdx.x * RO;
    const int rows = max(min(RO, n - i0), 0);
    const double rho = 1.0 / (1.0 + xhh[c.n_hh * t]);
    for (int it = slot; it < ne * rows; it += nslot) {
        const int e = it / rows, ii = it - e * rows, i = i0 + ii;
        double val = 0.0;
        if (m < M) {
            const size_t colb = (size_t)t * c.G + (size_t)e * n;
            const int *sbc = sb + ((size_t)t * ne + e) * (n + 1);
            const int b1 = min(max(sbc[i], 0), n), b0 = i > 0 ? min(max(sbc[i - 1], 0), b1) : b1, b2 = min(max(sbc[i + 1], b1), n);
            double sbar = 0.0, vmu = 0.0;
            if (!first) vmu = R.v[colb + i] * muIn[((size_t)e * n + i) * M + m];
            for (int a = b0; a < b2; a++) {
                double g = pbar[(colb + a) * M + m];
                if (!first) g -= R.v[colb + a] * muIn[((size_t)e * n + a) * M + m];
                sbar += (a < b1 ? R.B[colb + a] : R.A[colb + a]) * g;
            }
            val = vmu - rho * sbar;
        }
        inc_cell[((size_t)e * RO + ii) * MC + ml] = val;
    }
    __syncthreads();
    if (slot < ne && m < M) {      // (nslot >= 32 >= n_e)
        double tot = 0.0;
        for (int ii = 0; ii < rows; ii++) tot += inc_cell[((size_t)slot * RO + ii) * MC + ml];
        part[((size_t)blockIdx.x * ne + slot) * M + m] = tot;
    }
}
// y_bar (n_e, P, M) column-major from the reduced sums rm [P][n_e][M] (k_reduce_parts over the blocks), the column masses m [P][n_e]
// and consumption's cotangent yb1 [P][M] (zeros when it carries none). One thread per (t, e, m).
__global__ void k_inc_ybar_out(int P, int ne, int M, const double *__restrict__ rm, const double *__restrict__ m, const double *__restrict__ yb1,
                               double *__restrict__ y_bar) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)P * ne * M) return;
    const size_t te = idx / M, mm = idx - te * M, t = te / ne, e = te - t * ne;
    y_bar[e + (size_t)ne * (t + (size_t)P * mm)] = rm[idx] + m[te] * yb1[t * M + mm];
}

}  // namespace hank
