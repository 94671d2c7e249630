// hank_groups.h — group outputs: aggregates of caller-supplied weight arrays over the grid, their tangents and their Toeplitz
// Jacobian. The reference dots every heterogeneous variable with the same post-transition D_t (ForwardIteration.jl:303-307);
// group k dots W_k f_b with it, W_k[G] a fixed weight vector indexed like D (pt = e n_a + ia) and f_b one of three bases the
// record already holds (HANK_GROUP_MASS: 1, HANK_GROUP_POLICY: a'_t, HANK_GROUP_CONS: c_t = (1+r_t) a + w_t z_e + tr_t - a'_t):
//     Y^k_t  = sum W_k f_t D_t
//     dY^k_t = sum W_k f_t dD_t + sigma_b sum W_k D_t da'_t + [b = CONS] (dr_t sum W_k D_t a + dw_t sum W_k D_t z_e + dtr_t sum W_k D_t)
//     sigma_MASS = 0, sigma_POLICY = +1, sigma_CONS = -1
// The levels and the three CONS sums do not depend on the direction (k_grp_record: once per recorded primal and set of groups).
// The first two tangent terms need dD_t of every direction: the recurrence of hank_hetx.h after the sweeps (k_hx_mid as it is,
// then k_grp_mix: k_hx_mix's mixing with Pi and K reductions per period and direction; k_hx_reduce sums the blocks in order).
// W f is formed on the fly: no per-period f arrays. No atomics, fixed-order sums: the same inputs give the same bits.
#pragma once
#include "hank_kernels.h"
#include "hank_hetx.h"

namespace hank {

constexpr int GRP_MAX = 32;      // HANK_GROUP_MAX
constexpr int GRP_NS = 3;        // the CONS sums per period and group
constexpr int GRP_ROWS = 64;     // k_grp_mix: wealth rows per block (one wave per direction)
constexpr int GRP_LANES = 4;     // k_grp_mix: directions per block
constexpr int GRP_FN_CHUNK = 8;  // hank_fake_news_group: groups per pass over the expectation workspace

// f of base b at one point, and the sign of its policy partial
__device__ __forceinline__ double grp_f(int b, double pol, double cons) { return b == 0 ? 1.0 : (b == 1 ? pol : cons); }
__device__ __forceinline__ double grp_sigma(int b) { return b == 0 ? 0.0 : (b == 1 ? 1.0 : -1.0); }

// grid (P, K), one block per period and group: Y [t][k] = sum W_k f D_t and, for CONS, S [t][k][3] = sum W_k D_t (a, z_e, 1)
// (zeros for the other bases). W (G, K) column-major.
__global__ void __launch_bounds__(256) k_grp_record(Consts c, Record R, const double *__restrict__ xhh, int K, const double *__restrict__ W,
                                                    const int *__restrict__ base, double *__restrict__ Y, double *__restrict__ S) {
    __shared__ double red[16];
    const int t = blockIdx.x, k = blockIdx.y, b = base[k];
    const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = c.n_hh > 2 ? xhh[c.n_hh * t + 2] : 0.0;
    const size_t pb = (size_t)t * c.G;
    const double *Wk = W + (size_t)k * c.G;
    double acc[1 + GRP_NS] = {0.0, 0.0, 0.0, 0.0};
    for (int pt = threadIdx.x; pt < c.G; pt += blockDim.x) {
        const int e = pt / c.n_a, ia = pt - e * c.n_a;
        const double a = c.a[ia], z = c.z[e], pol = R.pol[pb + pt];
        const double cons = (1.0 + r) * a + w * z + tr - pol;
        const double WD = Wk[pt] * R.Dseq[pb + c.G + pt];     // post-transition D_t
        acc[0] += grp_f(b, pol, cons) * WD;
        if (b == 2) { acc[1] += WD * a; acc[2] += WD * z; acc[3] += WD; }
    }
    for (int j = 0; j <= GRP_NS; j++) {
        const double tot = block_sum(acc[j], red, blockDim.x);
        if (threadIdx.x == 0) {
            if (j == 0) Y[(size_t)t * K + k] = tot;
            else S[((size_t)t * K + k) * GRP_NS + j - 1] = tot;
        }
    }
}

// the K bases (0..2) packed two bits each: what k_grp_mix takes
inline unsigned long long grp_codes(const int *base, int K) {
    unsigned long long codes = 0;
    for (int k = 0; k < K; k++) codes |= (unsigned long long)(base[k] & 3) << (2 * k);
    return codes;
}

// a wave's sum in lane 0, fixed order
__device__ __forceinline__ double grp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// period t, mixing half (k_hx_mix's) and the K in-period reductions: dD_t[n][e2][r] = sum_e mid[n][e][r] Pi[e][e2], and per group
// sum W_k (f dD_t + sigma D_t da'_t) over the block's rows -> parts [n][t][block][k]. A block is GRP_ROWS rows x GRP_LANES
// directions, one wave per direction: each wave issues its own loads of W, pol and D_t, and the four waves of a block ask for the
// same addresses, so they share them through the CU's vector L1 where they hit (not measured with counters); across the
// ceil(N / GRP_LANES) block columns W is still read once per column. KC >= K accumulators sit in registers; `codes` packs the K
// bases, two bits each (grp_codes). KC = 16 and 32 spill 64 and 196 scalar registers to vector lanes (no scratch memory).
// grid (ceil(n_a / GRP_ROWS), ceil(N / GRP_LANES)), GRP_ROWS * GRP_LANES threads.
template <int KC>
__global__ void __launch_bounds__(GRP_ROWS * GRP_LANES) k_grp_mix(Consts c, Record R, int t, int N, int K, const double *__restrict__ xhh,
                                                                  const double *__restrict__ W, unsigned long long codes,
                                                                  const double *__restrict__ dpc, const double *__restrict__ mid,
                                                                  double *__restrict__ dD, double *__restrict__ parts) {
    const int lane = threadIdx.x & (GRP_ROWS - 1), n = blockIdx.y * GRP_LANES + threadIdx.x / GRP_ROWS;
    if (n >= N) return;      // (a whole wave: no block-wide barrier below)
    const int r = blockIdx.x * GRP_ROWS + lane, na = c.n_a;
    double acc[KC];
#pragma unroll
    for (int k = 0; k < KC; k++) acc[k] = 0.0;
    if (r < na) {
        const double rt = xhh[c.n_hh * t], wt = xhh[c.n_hh * t + 1], tr = c.n_hh > 2 ? xhh[c.n_hh * t + 2] : 0.0;
        const double *m = mid + (size_t)n * c.G;
        const double *dp = dpc + ((size_t)n * c.P + t) * c.G;
        const double *D = R.Dseq + (size_t)(t + 1) * c.G;
        const double *pol = R.pol + (size_t)t * c.G;
        const double cash = (1.0 + rt) * c.a[r] + tr;
        for (int e2 = 0; e2 < c.n_e; e2++) {
            double s = 0.0;
            for (int e = 0; e < c.n_e; e++) s += m[(size_t)e * na + r] * c.Pi[e + c.n_e * e2];
            const size_t pt = (size_t)e2 * na + r;
            dD[(size_t)n * c.G + pt] = s;
            const double p = pol[pt], cons = cash + wt * c.z[e2] - p, Ddp = D[pt] * dp[pt];
            const double v1 = p * s + Ddp, v2 = cons * s - Ddp;      // f dD_t + sigma D_t da'_t of POLICY and of CONS (MASS: s)
            const double *Wp = W + pt;
#pragma unroll
            for (int k = 0; k < KC; k++) {
                const int b = (int)(codes >> (2 * k)) & 3;
                if (k < K) acc[k] += Wp[(size_t)k * c.G] * (b == 0 ? s : (b == 1 ? v1 : v2));
            }
        }
    }
    double *out = parts + (((size_t)n * c.P + t) * gridDim.x + blockIdx.x) * K;
#pragma unroll
    for (int k = 0; k < KC; k++) {
        if (k < K) {      // (uniform)
            const double tot = grp_wave_sum(acc[k]);
            if (lane == 0) out[k] = tot;
        }
    }
}

// the assembly: (P, K) levels and (P, K, N) tangents, column-major, from the record's Y [t][k], S [t][k][3] and the call's in-period
// sums T [n][t][k]; the input terms of CONS are written here (S is zero for the other bases). Either output may be null.
__global__ void k_grp_outputs(int P, int n_hh, int K, int N, const double *__restrict__ dxhh, const double *__restrict__ Y,
                              const double *__restrict__ S, const double *__restrict__ T, double *__restrict__ out_agg,
                              double *__restrict__ out_dagg) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)P * K * (N + 1)) return;
    const int t = (int)(idx % P), k = (int)((idx / P) % K), n = (int)(idx / ((size_t)P * K)) - 1;
    if (n < 0) {
        if (out_agg) out_agg[(size_t)k * P + t] = Y[(size_t)t * K + k];
        return;
    }
    if (!out_dagg) return;
    const double *dx = dxhh + ((size_t)n * P + t) * n_hh, *s = S + ((size_t)t * K + k) * GRP_NS;
    const double dtr = n_hh > 2 ? dx[2] : 0.0;
    out_dagg[((size_t)n * K + k) * P + t] = T[((size_t)n * P + t) * K + k] + (dx[0] * s[0] + dx[1] * s[1] + dtr * s[2]);
}

// hank_fake_news_group's record, one block per group of the chunk k0 .. k0 + gridDim.x, at the stationary record (period 0):
// E0 [o][pt] = W_k f_ss (row o of E, `ostride` apart), Wd [o][pt] = sigma_b W_k D_ss, dsum [o][i] = d_{k,i} (CONS:
// sum W_k D (a, z_e, 1); else 0). The counterpart of k_fn_het_record; fixed-order block reductions.
__global__ void __launch_bounds__(256) k_grp_fn_record(Consts c, Record R, const double *__restrict__ xhh, int k0, const double *__restrict__ W,
                                                       const int *__restrict__ base, size_t ostride, double *__restrict__ E0,
                                                       double *__restrict__ Wd, double *__restrict__ dsum) {
    __shared__ double red[16];
    const int o = blockIdx.x, k = k0 + o, b = base[k], G = c.G;
    const double r = xhh[0], w = xhh[1], tr = c.n_hh > 2 ? xhh[2] : 0.0;
    const double *Wk = W + (size_t)k * G;
    const double sg = grp_sigma(b);
    double acc[GRP_NS] = {0.0, 0.0, 0.0};
    for (int pt = threadIdx.x; pt < G; pt += blockDim.x) {
        const int e = pt / c.n_a, ia = pt - e * c.n_a;
        const double a = c.a[ia], z = c.z[e], pol = R.pol[pt];
        const double cons = (1.0 + r) * a + w * z + tr - pol;
        const double WD = Wk[pt] * R.Dseq[G + pt];
        E0[(size_t)o * ostride + pt] = Wk[pt] * grp_f(b, pol, cons);
        Wd[(size_t)o * G + pt] = sg * WD;
        if (b == 2) { acc[0] += WD * a; acc[1] += WD * z; acc[2] += WD; }
    }
    double tot[GRP_NS];
    for (int j = 0; j < GRP_NS; j++) tot[j] = block_sum(acc[j], red, blockDim.x);
    if (threadIdx.x == 0) {
        double *d = dsum + (size_t)o * c.n_hh;
        d[0] = tot[0];
        d[1] = tot[1];
        if (c.n_hh > 2) d[2] = tot[2];
    }
}

}  // namespace hank
