// hank_adjoint.h — the TRANSPOSED sweeps of the household block: x̄ = J(x)ᵀ ȳ at the recorded primal (hank_vjp).
//
// The tangent map is the one k_tan_back / k_tan_fwd compute (hank_kernels.h). Its transpose runs the two
// recurrences in the opposite directions of time, for M cotangent columns at once:
//
//   Sweep A, t = P-1 .. 0 — the reverse of the distribution sweep (the reference's ForwardIteration_pullback,
//   ForwardIteration.jl:339-420, built on the reverse rule of transition_step, :131-192). State lam = cotangent of D_t:
//       lam     += yb0_t pol_t + yb1_t c_t                         c_t = (1+r_t) a + w_t z_e + tr_t - pol_t
//       U[r,e]   = sum_e2 Pi[e,e2] lam[r,e2]
//       pbar_t[j,e] = (yb0_t - yb1_t) D_t[j,e] + ig_j D_{t-1}[j,e] (U[lo_j+1,e] - U[lo_j,e])
//       lam[j,e] = (1-w_j) U[lo_j,e] + w_j U[lo_j+1,e]
//   Sweep B, t = 0 .. P-1 — the reverse of the EGM sweep (no counterpart in the reference: it differentiates
//   BackwardIteration forward only). State mu = cotangent of dV_t, mu_0 = 0, mu_P dropped (the terminal value is fixed):
//       gbar     = pbar_t - v_t mu
//       sbar[e,i] = sum_{a: ib[e,a] = i} A gbar[e,a] + sum_{a: ib[e,a] = i-1} B gbar[e,a]
//       mu[i,e2] = sum_e Pi[e,e2] kc_t[e,i] sbar[e,i]
//       xbar_{r,t} = sum mu (u_t + v_t a) - rho_t sum sbar s_t + yb1_t sum a D_t      (w: v_t z_e, z_e, sum z_e D_t; tr: v_t, 1, sum D_t)
//
// One launch per period and sweep, replayed from two hipGraphs per batch width. Layout as the tangent kernels': the state is
// [e][a][M] and pbar [P][G][M], cotangent index fastest; VT = double2 (two adjacent columns per lane, every state / pbar access
// 16 bytes) for an even M, double otherwise. Block = one wave per productivity column, lanes = (column pair fastest, row).
// No atomics: every sum has a fixed order, so the same record and cotangents give the same bits.
//
// Outputs 2, 3 (Value, UCE: hank_hetx.h) are not affine in the policy: Y^o_t = sum f_o,t D_t. Their cotangents (hank_vjp_het)
// enter Sweep A in two places, NX = 1 or 2 of them at a time, from the record k_hx_record writes once per primal (the context's
// HxRecord, the one hank_get_het_outputs reads: ensure_hx_record, hank_hip.hip):
//       lam        += sum_o ybx_o,t f_o,t                          (next to yb0 pol + yb1 c, before the Pi mix)
//       pbar_t[j,e] -= sum_o ybx_o,t f_c,o,t[j,e] D_t[j,e]         (next to (yb0 - yb1) D_t)
// and the household inputs' cotangents directly (k_adj_hx_out, after Sweep B): xbar_r += ybx_o,t (Sa + Sr), xbar_w += ybx_o,t Sz,
// xbar_tr += ybx_o,t S1. Sweep B is the same: pbar carries everything it reads.
// NOTE: k_ss_lam and k_ss_nu (hank_ssdiff.h) restate the tile mix, the bracket gather and the six block sums of k_adj_dist and k_adj_egm: a
// shared inline function for any one of them changes these kernels' instructions (profiles/ssdiff_unit.txt), so a change here is made there too.
#pragma once
#include "hank_hetx.h"
#include "hank_kernels.h"

namespace hank {

// (AdjGeom: hank_geom.h; ADJ_KS, adj_rows_sum, AdjHx: hank_device.h)

// agg_bar (P, n_het, M) column-major -> yb0[P][M], yb1[P][M] (zeros when consumption carries no cotangent)
__global__ void k_adj_in(const double *__restrict__ agg_bar, int P, int n_het, int M, double *__restrict__ yb0, double *__restrict__ yb1) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * M) return;
    const int t = idx / M, m = idx - t * M;
    const double *y = agg_bar + (size_t)t + (size_t)P * n_het * m;
    yb0[idx] = y[0];
    yb1[idx] = n_het > 1 ? y[P] : 0.0;
}

// agg_bar (P, n_het, M) column-major, outputs 2 .. n_het-1 -> ybx[P][NX][M], NX = n_het - 2
__global__ void k_adj_in_hx(const double *__restrict__ agg_bar, int P, int n_het, int M, double *__restrict__ ybx) {
    const int NX = n_het - 2, idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * NX * M) return;
    const int t = idx / (NX * M), jx = (idx - t * NX * M) / M, m = idx - (t * NX + jx) * M;
    ybx[idx] = agg_bar[(size_t)t + (size_t)P * ((2 + jx) + (size_t)n_het * m)];
}

// Segment starts of the interpolation brackets, once per record: sb[col][i] = first row a of column col = (t, e) with
// ib[a] >= i, taken over the rows [zlo, zhi) that carry a weight at all (A != 0 or B != 0) — the constrained prefix and the
// flat top of a column (hundreds of rows with ib = 0 / n_a - 2 and A = B = 0) belong to no segment, so Sweep B never walks
// them. ib is non-decreasing in a (sorted knots, increasing grid): the rows with ib = i are [sb[i], sb[i+1]). Every entry
// lies in [0, n_a] whatever the record holds. One block per column; dynamic LDS: (n_a + 1) ints.
__global__ void __launch_bounds__(256) k_adj_seg(Consts c, Record R, int ncols, int *__restrict__ sb) {
    extern __shared__ int shb[];
    __shared__ int redlo[4], redhi[4];
    const int col = blockIdx.x, n = c.n_a;
    if (col >= ncols) return;
    const size_t base = (size_t)col * n;
    int lo = n, hi = 0;
    for (int a = threadIdx.x; a < n; a += blockDim.x)
        if (R.A[base + a] != 0.0 || R.B[base + a] != 0.0) { lo = min(lo, a); hi = max(hi, a + 1); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo = min(lo, __shfl_xor(lo, off, 64)); hi = max(hi, __shfl_xor(hi, off, 64)); }
    if ((threadIdx.x & 63) == 0) { redlo[threadIdx.x >> 6] = lo; redhi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    int zlo = min(min(redlo[0], redlo[1]), min(redlo[2], redlo[3])), zhi = max(max(redhi[0], redhi[1]), max(redhi[2], redhi[3]));
    if (zlo >= zhi) zlo = zhi = 0;
    for (int r = threadIdx.x; r <= n; r += blockDim.x) shb[r] = zhi;
    __syncthreads();
    for (int a = zlo + threadIdx.x; a < zhi; a += blockDim.x) {
        const int prev = a > zlo ? min(max(R.ib[base + a - 1], -1), n - 1) : -1, cur = min(max(R.ib[base + a], -1), n - 1);
        for (int r = prev + 1; r <= cur; r++) shb[r] = a;
    }
    __syncthreads();
    int *out = sb + (size_t)col * (n + 1);
    for (int r = threadIdx.x; r <= n; r += blockDim.x) out[r] = shb[r];
}

// ---- Sweep A, one period -------------------------------------------------------------------------------------------------
// A block owns the TARGET rows [r0, r1) of the lottery, all columns: it loads lam rows r0 .. r1 (one halo row) and row 0 once,
// adds the period's output cotangents, mixes them with Pi through the LDS tile (U), and then serves, per column, the SOURCES
// [start[r0], start[r1]) that the recorded lottery sends to its rows — the transpose of the source-stationary forward kernel —
// plus its share of the clamped prefix [0, clo) (sources that all read U[0] and whose policy cotangent has no lottery part:
// shared out evenly over the row blocks). Every source row is written by exactly one block.
// NX extra outputs (hx: nothing for NX = 0): a lane also reads f_o at its target rows, f_c,o at its source rows and ybx_o,t.
// dynamic LDS: VT tile[n_e][R + 2][NC] (slot R + 1 = row 0), double Pish[n_e * n_e]
template <typename VT, int NX>
__global__ void __launch_bounds__(1024)
k_adj_dist(Consts c, Record R, const double *__restrict__ xhh, AdjGeom g, int t, int first, const VT *__restrict__ yb0,
           const VT *__restrict__ yb1, const VT *__restrict__ lamIn, VT *__restrict__ lamOut, VT *__restrict__ pbar, AdjHx<VT, NX> hx) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
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
    VT y0, y1;
    vzero(y0); vzero(y1);
    if (mok) { y0 = yb0[(size_t)t * MV + m]; y1 = yb1[(size_t)t * MV + m]; }
    [[maybe_unused]] VT yx[NX > 0 ? NX : 1];
    [[maybe_unused]] const size_t PG = (size_t)c.P * c.G;
    if constexpr (NX > 0) {
#pragma unroll
        for (int o = 0; o < NX; o++) {
            vzero(yx[o]);
            if (mok) yx[o] = hx.ybx[((size_t)t * NX + o) * MV + m];
        }
    }
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t), ze = c.z[e];
    const size_t colb = (size_t)t * c.G + (size_t)e * n;      // (t, e) column of the record
    // 1. lam + yb0 pol + yb1 c of the block's rows, own column
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB;
        if (slot < NS) {
            const int row = slot == g.R + 1 ? 0 : r0 + slot;
            VT v;
            vzero(v);
            if (mok && row <= r1 && row < n) {
                const double pol = R.pol[colb + row], cons = ((1.0 + r) * c.a[row] + (w * ze + tr)) - pol;
                if (!first) v = lamIn[((size_t)e * n + row) * MV + m];
                v = vadd(v, vadd(vmul(pol, y0), vmul(cons, y1)));
                if constexpr (NX > 0) {
#pragma unroll
                    for (int o = 0; o < NX; o++) v = vadd(v, vmul(hx.f[o * PG + colb + row], yx[o]));
                }
            }
            tile[((size_t)e * NS + slot) * g.NC + nl] = v;
        }
    }
    __syncthreads();
    // 2. U[row, e] = sum_e2 Pi[e, e2] lam[row, e2], back into the tile
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
    if (!mok) return;
    const VT *Ue = tile + (size_t)e * NS * g.NC + nl;
    const VT yd = vsub(y0, y1);
    const double *Dprev = R.Dseq + colb, *Dnext = R.Dseq + colb + c.G;
    VT *lo_out = lamOut + ((size_t)e * n) * MV + m, *pb_out = pbar + colb * MV + m;
    // 3. the sources of the block's target rows
    const int *st = R.start + ((size_t)t * ne + e) * (n + 1);
    const int j0 = min(max(st[r0], 0), n), j1 = min(max(st[r1], 0), n);
    for (int j = j0 + rl; j < j1; j += RB) {
        const int sl = min(max(R.lo[colb + j] - r0, 0), g.R - 1);
        const double wj = R.lw[colb + j], gD = R.ig[colb + j] * Dprev[j], Dn = Dnext[j];
        const VT u0 = Ue[(size_t)sl * g.NC], u1 = Ue[(size_t)(sl + 1) * g.NC];
        st_mode<HANK_ST_STATE>(&lo_out[(size_t)j * MV], vadd(vmul(1.0 - wj, u0), vmul(wj, u1)));
        VT ye = yd;      // the policy's direct weight in the outputs, per unit of D_t: yb0 - yb1 - sum_o f_c,o ybx_o
        if constexpr (NX > 0) {
#pragma unroll
            for (int o = 0; o < NX; o++) ye = vsub(ye, vmul(hx.fc[o * PG + colb + j], yx[o]));
        }
        st_mode<HANK_ST_DPOL>(&pb_out[(size_t)j * MV], vadd(vmul(Dn, ye), vmul(gD, vsub(u1, u0))));
    }
    // 4. the block's share of the clamped prefix
    const int clo = min(max(R.clo[(size_t)t * ne + e], 0), n);
    const int c0 = (int)(((long long)clo * blockIdx.x) / gridDim.x), c1 = (int)(((long long)clo * (blockIdx.x + 1)) / gridDim.x);
    const VT U0 = Ue[(size_t)(g.R + 1) * g.NC];
    for (int j = c0 + rl; j < c1; j += RB) {
        st_mode<HANK_ST_STATE>(&lo_out[(size_t)j * MV], U0);
        VT ye = yd;
        if constexpr (NX > 0) {
#pragma unroll
            for (int o = 0; o < NX; o++) ye = vsub(ye, vmul(hx.fc[o * PG + colb + j], yx[o]));
        }
        st_mode<HANK_ST_DPOL>(&pb_out[(size_t)j * MV], vmul(Dnext[j], ye));
    }
}

// ---- Sweep B, one period -------------------------------------------------------------------------------------------------
// A block owns the KNOT rows [i0, i0 + R), all columns. Knot i of column e gathers gbar = pbar_t - v_t mu over the two
// contiguous row segments that bracket on it ([sb[i], sb[i+1]) with weight A, [sb[i-1], sb[i]) with weight B: k_adj_seg), the
// n_e x n_e mixing of kc_t sbar goes through the LDS tile, and the block writes mu_{t+1} for its rows. A row of mu / pbar is
// read by the (at most two) knots of its bracket. The household inputs' cotangents leave as per-block partials, summed in a
// fixed order by k_adj_out: partS[t][block][3][M] = sum sbar (s_t, z_e, 1), partM[t+1][block][3][M] = sum mu_{t+1} (u + v a, v z_e, v).
// dynamic LDS: VT tile[n_e][R][NC], double Pish[n_e * n_e], VT red[n_e][6][NC]
template <typename VT>
__global__ void __launch_bounds__(1024)
k_adj_egm(Consts c, Record R, AdjGeom g, int t, int first, int last, const int *__restrict__ sb, const VT *__restrict__ muIn,
          VT *__restrict__ muOut, const VT *__restrict__ pbar, VT *__restrict__ partS, VT *__restrict__ partM) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
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
    const size_t colb = (size_t)t * c.G + (size_t)e * n;
    const int *sbc = sb + ((size_t)t * ne + e) * (n + 1);
    const double ze = c.z[e];
    VT sum[6];
#pragma unroll
    for (int q = 0; q < 6; q++) vzero(sum[q]);
    // 1. sbar of the block's knots, own column; kc sbar into the tile
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB, i = i0 + slot;
        VT sbar;
        vzero(sbar);
        if (mok && slot < g.R && i < n) {
            const int b1 = min(max(sbc[i], 0), n), b0 = i > 0 ? min(max(sbc[i - 1], 0), b1) : b1, b2 = min(max(sbc[i + 1], b1), n);
            const VT *pb = pbar + colb * MV + m, *mu = muIn + ((size_t)e * n) * MV + m;
            for (int a = b0; a < b2; a += 2) {      // two rows per trip, their loads in flight together; summed in row order
                const bool two = a + 1 < b2;
                const int a1 = two ? a + 1 : a;
                const double w0 = a < b1 ? R.B[colb + a] : R.A[colb + a], w1 = a1 < b1 ? R.B[colb + a1] : R.A[colb + a1];
                VT g0 = pb[(size_t)a * MV], g1 = pb[(size_t)a1 * MV];
                if (!first) {
                    const double v0 = R.v[colb + a], v1 = R.v[colb + a1];
                    const VT m0 = mu[(size_t)a * MV], m1 = mu[(size_t)a1 * MV];
                    g0 = vsub(g0, vmul(v0, m0));
                    g1 = vsub(g1, vmul(v1, m1));
                }
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
    // 2. mu_{t+1}[i, e2] = sum_e Pi[e, e2] kc_t[e, i] sbar[e, i] for the wave's column e2 = e
    if (!last) {
        const size_t coln = colb + c.G;
#pragma unroll
        for (int k = 0; k < ADJ_KS; k++) {
            const int slot = rl + k * RB, i = i0 + slot;
            if (mok && slot < g.R && i < n) {
                VT mn;
                vzero(mn);
                for (int e1 = 0; e1 < ne; e1++) mn = vadd(mn, vmul(Pish[e1 + ne * e], tile[((size_t)e1 * NS + slot) * g.NC + nl]));
                st_mode<HANK_ST_STATE>(&muOut[((size_t)e * n + i) * MV + m], mn);
                const double u1 = R.u[coln + i], v1 = R.v[coln + i];
                sum[3] = vadd(sum[3], vmul(u1 + v1 * c.a[i], mn));
                sum[4] = vadd(sum[4], vmul(v1 * ze, mn));
                sum[5] = vadd(sum[5], vmul(v1, mn));
            }
        }
    }
    // 3. the block's partial sums: rows of a wave, then — sum q in wave q mod n_e — the waves, RB at a time, in a fixed order
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
            if (q < 3) partS[(((size_t)t * gridDim.x + blockIdx.x) * 3 + q) * MV + m] = v;
            else if (!last) partM[(((size_t)(t + 1) * gridDim.x + blockIdx.x) * 3 + (q - 3)) * MV + m] = v;
        }
    }
}

// xhh_bar (n_hh, P, M) column-major from the blocks' partials, in block order (the manner of k_reduce_parts: the same record
// and cotangents give the same bits), plus consumption's direct dependence on the inputs: yb1_t (sum a D_t, sum z_e D_t, sum D_t)
// = yb1_t (agg2[t], zd[t], zd[P + t]) — the sums k_het_outputs uses. One thread per (t, column).
__global__ void k_adj_out(int P, int n_hh, int M, int nb, const double *__restrict__ xhh, const double *__restrict__ partS,
                          const double *__restrict__ partM, const double *__restrict__ yb1, const double *__restrict__ agg2,
                          const double *__restrict__ zd, double *__restrict__ xhh_bar) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * M) return;
    const int t = idx / M, m = idx - t * M;
    double s[3] = {0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nb; b++) {
        const size_t o = (((size_t)t * nb + b) * 3) * M + m;
        for (int q = 0; q < 3; q++) s[q] += partS[o + (size_t)q * M];
        if (t > 0)
            for (int q = 0; q < 3; q++) mu[q] += partM[o + (size_t)q * M];
    }
    const double rho = 1.0 / (1.0 + xhh[n_hh * t]), y1 = yb1[idx];
    double *out = xhh_bar + (size_t)n_hh * ((size_t)t + (size_t)P * m);
    out[0] = (mu[0] - rho * s[0]) + y1 * agg2[t];
    out[1] = (mu[1] - rho * s[1]) + y1 * zd[t];
    if (n_hh > 2) out[2] = (mu[2] - rho * s[2]) + y1 * zd[P + t];
}

// The extra outputs' direct dependence on the inputs, added to xhh_bar after k_adj_out, in output order:
// ybx_o,t (Sa + Sr, Sz, S1) of k_hx_record's sums S [t][SX][HX_NS] (SX: the outputs the record holds). One thread per (t, column).
__global__ void k_adj_hx_out(int P, int n_hh, int M, int NX, int SX, const double *__restrict__ ybx, const double *__restrict__ S,
                             double *__restrict__ xhh_bar) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * M) return;
    const int t = idx / M, m = idx - t * M;
    double *out = xhh_bar + (size_t)n_hh * ((size_t)t + (size_t)P * m);
    for (int o = 0; o < NX; o++) {
        const double y = ybx[((size_t)t * NX + o) * M + m];
        const double *s = S + ((size_t)t * SX + o) * HX_NS;      // Y, Sa, Sz, S1, Sr
        out[0] += y * (s[1] + s[4]);
        out[1] += y * s[2];
        if (n_hh > 2) out[2] += y * s[3];
    }
}

}  // namespace hank
