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
//
// Group outputs (hank_groups.h) are extra outputs in the same sense, K <= 32 of them, with f = W_k f_b and f_c = -sigma_b W_k formed in
// the kernel instead of read from a record (hank_vjp_group: k_adj_dist_grp, k_adj_in_grp, k_adj_grp_out below).
#pragma once
#include "hank_hetx.h"
#include "hank_kernels.h"
#include "hank_groups.h"

namespace hank {

// (AdjGeom: hank_geom.h; ADJ_KS, AdjLane, AdjHx, adj_dist_body, adj_egm_body, xbar_cons, xbar_hx: hank_device.h)

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

// ---- Sweep A, one period: adj_dist_body (hank_device.h) --------------------------------------------------------------------------
// A tile row is loaded with lam + yb0 pol + yb1 c (+ sum_o f_o ybx_o) of period t; source row j leaves lamOut[j] and pbar_t[j].
// NX extra outputs (hx: nothing for NX = 0): a lane also reads f_o at its target rows, f_c,o at its source rows and ybx_o,t.
// dynamic LDS: VT tile[n_e][R + 2][NC] (slot R + 1 = row 0), double Pish[n_e * n_e]
template <typename VT, int NX>
__global__ void __launch_bounds__(1024)
k_adj_dist(Consts c, Record R, const double *__restrict__ xhh, AdjGeom g, int t, int first, const VT *__restrict__ yb0,
           const VT *__restrict__ yb1, const VT *__restrict__ lamIn, VT *__restrict__ lamOut, VT *__restrict__ pbar, AdjHx<VT, NX> hx) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
    const AdjLane L = adj_lane(g);
    const int n = c.n_a, e = L.e, m = L.m;
    const size_t MV = g.MV;
    VT y0, y1;
    vzero(y0); vzero(y1);
    if (L.mok) { y0 = yb0[(size_t)t * MV + m]; y1 = yb1[(size_t)t * MV + m]; }
    [[maybe_unused]] VT yx[NX > 0 ? NX : 1];
    [[maybe_unused]] const size_t PG = (size_t)c.P * c.G;
    if constexpr (NX > 0) {
#pragma unroll
        for (int o = 0; o < NX; o++) {
            vzero(yx[o]);
            if (L.mok) yx[o] = hx.ybx[((size_t)t * NX + o) * MV + m];
        }
    }
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t), ze = c.z[e];
    const size_t colb = (size_t)t * c.G + (size_t)e * n;      // (t, e) column of the record
    VT yd;
    const double *Dprev = R.Dseq + colb, *Dnext = R.Dseq + colb + c.G;
    VT *lo_out = lamOut + ((size_t)e * n) * MV + m, *pb_out = pbar + colb * MV + m;
    adj_dist_body<VT>(c, R, g, L, t, adj_sh,
        [&](int row) __attribute__((always_inline)) {
            const double pol = R.pol[colb + row], cons = ((1.0 + r) * c.a[row] + (w * ze + tr)) - pol;
            VT v;
            vzero(v);
            if (!first) v = lamIn[((size_t)e * n + row) * MV + m];
            v = vadd(v, vadd(vmul(pol, y0), vmul(cons, y1)));
            if constexpr (NX > 0) {
#pragma unroll
                for (int o = 0; o < NX; o++) v = vadd(v, vmul(hx.f[o * PG + colb + row], yx[o]));
            }
            return v;
        },
        [&]() __attribute__((always_inline)) { yd = vsub(y0, y1); },
        [&](int j, VT u0, VT u1, bool clamped) __attribute__((always_inline)) {
            double wj = 0.0, gD = 0.0;
            if (!clamped) { wj = R.lw[colb + j]; gD = R.ig[colb + j] * Dprev[j]; }
            const double Dn = Dnext[j];
            st_wt(&lo_out[(size_t)j * MV], clamped ? u0 : vadd(vmul(1.0 - wj, u0), vmul(wj, u1)));
            VT ye = yd;      // the policy's direct weight in the outputs, per unit of D_t: yb0 - yb1 - sum_o f_c,o ybx_o
            if constexpr (NX > 0) {
#pragma unroll
                for (int o = 0; o < NX; o++) ye = vsub(ye, vmul(hx.fc[o * PG + colb + j], yx[o]));
            }
            // (a clamped source's policy cotangent has no lottery part)
            st_wt(&pb_out[(size_t)j * MV], clamped ? vmul(Dn, ye) : vadd(vmul(Dn, ye), vmul(gD, vsub(u1, u0))));
        });
}

// ---- Sweep A with cotangents on the group outputs (hank_vjp_group; hank_groups.h) ----------------------------------------------------
// Group k is an extra output with f = W_k f_b and f_c = -sigma_b W_k; neither is stored. With g[t,k,m] the groups' cotangents and
//       q0 = sum_{k: MASS} W_k g_k,   q1 = sum_{k: POLICY} W_k g_k,   q2 = sum_{k: CONS} W_k g_k        (point-wise, per column m)
// a tile row is loaded with lam + (yb0 + q1) pol + (yb1 + q2) c + q0 and source row j leaves pbar_t[j] = D_t[j] ((yb0 - yb1) + (q1 - q2)[j])
// + the lottery part. The lane forms them at its own rows in run-time loops over the K groups, in group order, from W_k[e n_a + row] in
// global memory (lanes that differ only in m ask for the same address) and g[t,k,m]. `codes`: the bases, two bits each (grp_codes) —
// uniform, so the selection is scalar and there is no branch on it. At a tile row the three q collapse into one sum,
// T = sum_k (W_k f_b) g_k with f_b = 1, pol or c of that row (f_o = W_k f_b itself), for the lane's three rows in one loop; these
// take g from global memory next to their W loads (no barrier in front of the first load). A source row needs q1 - q2 =
// sum_k sigma_b W_k g_k and reads g from LDS, staged once per block (visible behind adj_dist_body's barriers). g is never held in registers.
// k_adj_dist's lane geometry, tile and order of sums; no atomics: the same record, groups and cotangents give the same bits.
// dynamic LDS: k_adj_dist's (Pish rounded up to an even count), then VT gsh[K][NC]
__host__ __device__ inline size_t adj_grp_lds_off(int n_e, const AdjGeom &g, int V) {      // in doubles
    return (size_t)n_e * (g.R + 2) * g.NC * V + (((size_t)n_e * n_e + 1) & ~(size_t)1);
}
template <typename VT>
__global__ void __launch_bounds__(1024)
k_adj_dist_grp(Consts c, Record R, const double *__restrict__ xhh, AdjGeom g, int t, int first, const VT *__restrict__ yb0,
               const VT *__restrict__ yb1, const VT *__restrict__ lamIn, VT *__restrict__ lamOut, VT *__restrict__ pbar, int K,
               unsigned long long codes, const double *__restrict__ W, const VT *__restrict__ gb) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
    const AdjLane L = adj_lane(g);
    const int n = c.n_a, e = L.e, m = L.m;
    const size_t MV = g.MV, G = c.G;
    VT *gsh = reinterpret_cast<VT *>(adj_sh + adj_grp_lds_off(c.n_e, g, (int)(sizeof(VT) / sizeof(double))));
    for (int i = threadIdx.x; i < K * g.NC; i += 64 * c.n_e) {      // g[t, k, the block's columns]; zeros past the last column
        const int k = i >> g.lgNC, mm = blockIdx.y * g.NC + (i & (g.NC - 1));
        VT v;
        vzero(v);
        if (mm < g.MV) v = gb[((size_t)t * K + k) * MV + mm];
        gsh[i] = v;
    }
    // (no barrier here: the tile rows' sum below takes g straight from global memory, next to its W loads, and the source rows read
    // gsh behind adj_dist_body's own barriers)
    // groups per trip of the two K loops (their W loads are in flight together); scalar lanes at 4 and 8 spill four registers to scratch
    constexpr int ROW_UNROLL = sizeof(VT) == sizeof(double2) ? 4 : 2, SRC_UNROLL = sizeof(VT) == sizeof(double2) ? 8 : 4;
    const VT *gl = gsh + L.nl;
    const VT *gg = gb + (size_t)t * K * MV + (L.mok ? m : 0);
    VT y0, y1;
    vzero(y0); vzero(y1);
    if (L.mok) { y0 = yb0[(size_t)t * MV + m]; y1 = yb1[(size_t)t * MV + m]; }
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t), ze = c.z[e];
    const size_t colb = (size_t)t * c.G + (size_t)e * n;      // (t, e) column of the record
    const double *We = W + (size_t)e * n;                     // W_k[e n_a + row] = We[k G + row]
    // The groups' weight on the distribution at the lane's tile rows, T = sum_k (W_k f_b) g_k = q1 pol + q2 c + q0, for its ADJ_KS
    // slots in ONE loop over k: the slots' W loads of several k are in flight together (a loop per slot waits for each in turn).
    // rw: the slot's row as adj_dist_body maps it, or -1 where the body loads nothing.
    int rw[ADJ_KS];
    double fp[ADJ_KS], fq[ADJ_KS];
    VT T[ADJ_KS];
    {
        const int r0 = blockIdx.x * g.R, r1 = min(r0 + g.R, n);
#pragma unroll
        for (int s = 0; s < ADJ_KS; s++) {
            const int slot = L.rl + s * L.RB, row = slot == g.R + 1 ? 0 : r0 + slot;
            rw[s] = (L.mok && slot < g.R + 2 && row <= r1 && row < n) ? row : -1;
            fp[s] = rw[s] >= 0 ? R.pol[colb + rw[s]] : 0.0;
            fq[s] = rw[s] >= 0 ? ((1.0 + r) * c.a[rw[s]] + (w * ze + tr)) - fp[s] : 0.0;
            vzero(T[s]);
        }
#pragma unroll ROW_UNROLL
        for (int k = 0; k < K; k++) {
            const int b = (int)(codes >> (2 * k)) & 3;
            const double c0 = b == 0 ? 1.0 : 0.0, c1 = b == 1 ? 1.0 : 0.0, c2 = b == 2 ? 1.0 : 0.0;      // (uniform; f_b = c0 + c1 pol + c2 c, exactly)
            const VT gk = gg[(size_t)k * MV];
#pragma unroll
            for (int s = 0; s < ADJ_KS; s++) {
                const double wk = We[(size_t)k * G + max(rw[s], 0)];      // (a slot without a row reads row 0 and is not used)
                T[s] = vadd(T[s], vmul(wk * ((c1 * fp[s] + c2 * fq[s]) + c0), gk));
            }
        }
    }
    const int rw0 = rw[0], rw1 = rw[1];
    VT yd;
    const double *Dprev = R.Dseq + colb, *Dnext = R.Dseq + colb + c.G;
    VT *lo_out = lamOut + ((size_t)e * n) * MV + m, *pb_out = pbar + colb * MV + m;
    adj_dist_body<VT>(c, R, g, L, t, adj_sh,
        [&](int row) __attribute__((always_inline)) {
            const double pol = R.pol[colb + row], cons = ((1.0 + r) * c.a[row] + (w * ze + tr)) - pol;
            VT v;
            vzero(v);
            if (!first) v = lamIn[((size_t)e * n + row) * MV + m];
            v = vadd(v, vadd(vmul(pol, y0), vmul(cons, y1)));
            // the row's T, picked with 0 / 1 factors (a select between the three objects compiles to an indexed load from scratch memory)
            const double m0 = row == rw0 ? 1.0 : 0.0, m1 = (row != rw0 && row == rw1) ? 1.0 : 0.0, m2 = (1.0 - m0) - m1;
            return vadd(v, vadd(vadd(vmul(m0, T[0]), vmul(m1, T[1])), vmul(m2, T[2])));
        },
        [&]() __attribute__((always_inline)) { yd = vsub(y0, y1); },
        [&](int j, VT u0, VT u1, bool clamped) __attribute__((always_inline)) {
            double wj = 0.0, gD = 0.0;
            if (!clamped) { wj = R.lw[colb + j]; gD = R.ig[colb + j] * Dprev[j]; }
            const double Dn = Dnext[j];
            st_wt(&lo_out[(size_t)j * MV], clamped ? u0 : vadd(vmul(1.0 - wj, u0), vmul(wj, u1)));
            VT dq;      // the policy's direct weight in the outputs, per unit of D_t: (yb0 - yb1) + (q1 - q2), q1 - q2 = sum_k sigma_b W_k g_k
            vzero(dq);
            const double *Wp = We + j;
#pragma unroll SRC_UNROLL
            for (int k = 0; k < K; k++) {      // (no branch on the base: the W loads of SRC_UNROLL groups are in flight together)
                const int b = (int)(codes >> (2 * k)) & 3;
                const double sg = b == 1 ? 1.0 : (b == 2 ? -1.0 : 0.0);
                dq = vadd(dq, vmul(sg * Wp[(size_t)k * G], gl[(size_t)k * g.NC]));
            }
            const VT ye = vadd(yd, dq);
            st_wt(&pb_out[(size_t)j * MV], clamped ? vmul(Dn, ye) : vadd(vmul(Dn, ye), vmul(gD, vsub(u1, u0))));
        });
}

// grp_bar (P, K, M) column-major -> gb [P][K][M] (as VT: [P][K][MV]), the counterpart of k_adj_in_hx
__global__ void k_adj_in_grp(const double *__restrict__ grp_bar, int P, int K, int M, double *__restrict__ gb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * K * M) return;
    const int t = idx / (K * M), k = (idx - t * K * M) / M, m = idx - (t * K + k) * M;
    gb[idx] = grp_bar[(size_t)t + (size_t)P * (k + (size_t)K * m)];
}

// The group outputs' direct dependence on the inputs, added to xhh_bar after k_adj_out, in group order: g[t,k,m] S[t][k][.] of
// k_grp_record's CONS sums over (a, z_e, 1) -> (r, w, tr); S is zero for the other bases. One thread per (t, column).
__global__ void k_adj_grp_out(int P, int n_hh, int M, int K, const double *__restrict__ gb, const double *__restrict__ S, double *__restrict__ xhh_bar) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * M) return;
    const int t = idx / M, m = idx - t * M;
    double *out = xhh_bar + (size_t)n_hh * ((size_t)t + (size_t)P * m);
    for (int k = 0; k < K; k++) {
        const double y = gb[((size_t)t * K + k) * M + m], *s = S + ((size_t)t * K + k) * GRP_NS;
        out[0] += y * s[0];
        out[1] += y * s[1];
        if (n_hh > 2) out[2] += y * s[2];
    }
}

// ---- Sweep B, one period: adj_egm_body (hank_device.h) ---------------------------------------------------------------------------
// gbar = pbar_t - v_t mu (mu_0 = 0: first), and the mixed rows are mu_{t+1} (dropped when last: the terminal value is fixed), which
// the inputs' sums weigh at period t + 1. The partials are summed in a fixed order by k_adj_out:
// partS[t][block][3][M] = sum sbar (s_t, z_e, 1), partM[t+1][block][3][M] = sum mu_{t+1} (u + v a, v z_e, v).
// dynamic LDS: VT tile[n_e][R][NC], double Pish[n_e * n_e], VT red[n_e][6][NC]
template <typename VT>
__global__ void __launch_bounds__(1024)
k_adj_egm(Consts c, Record R, AdjGeom g, int t, int first, int last, const int *__restrict__ sb, const VT *__restrict__ muIn,
          VT *__restrict__ muOut, const VT *__restrict__ pbar, VT *__restrict__ partS, VT *__restrict__ partM) {
    extern __shared__ __attribute__((aligned(16))) double adj_sh[];
    const AdjLane L = adj_lane(g);
    const size_t MV = g.MV, per = (size_t)gridDim.x * 3 * MV;      // a period of partS / partM
    adj_egm_body<VT>(c, R, g, L, t, t + 1, !first, !last, sb, muIn, pbar, adj_sh, partS + (size_t)t * per, partM + (size_t)(t + 1) * per,
        [&](int i, VT mn) __attribute__((always_inline)) {
            st_wt(&muOut[((size_t)L.e * c.n_a + i) * MV + L.m], mn);
            return mn;
        });
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
    out[0] = xbar_cons(mu[0], rho, s[0], y1, agg2[t]);
    out[1] = xbar_cons(mu[1], rho, s[1], y1, zd[t]);
    if (n_hh > 2) out[2] = xbar_cons(mu[2], rho, s[2], y1, zd[P + t]);
}

// The extra outputs' direct dependence on the inputs, added to xhh_bar after k_adj_out, in output order:
// ybx_o,t (Sa + Sr, Sz, S1) of k_hx_record's sums S [t][SX][HX_NS] (SX: the outputs the record holds). One thread per (t, column).
__global__ void k_adj_hx_out(int P, int n_hh, int M, int NX, int SX, const double *__restrict__ ybx, const double *__restrict__ S,
                             double *__restrict__ xhh_bar) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * M) return;
    const int t = idx / M, m = idx - t * M;
    double *out = xhh_bar + (size_t)n_hh * ((size_t)t + (size_t)P * m);
    for (int o = 0; o < NX; o++) xbar_hx(ybx[((size_t)t * NX + o) * M + m], S + ((size_t)t * SX + o) * HX_NS, n_hh, out);
}

}  // namespace hank
