// hank_boundary.h — tangents and cotangents on the BOUNDARY of the household block: the terminal marginal value V_P
// (`ss_end.value`, BackwardIteration.jl:85) and the initial distribution D_0 (`ss_initial.D`, ForwardIteration.jl:293), which
// every other product of the library holds constant (hank_jvp_boundary, hank_vjp_boundary).
//
// The tangent map is linear, so the boundary enters the launch family's recurrences (k_tan_back / k_tan_fwd, hank_kernels.h) as
// two SEEDS of their loop-carried states, and leaves the transposed recurrences (k_adj_dist / k_adj_egm, hank_adjoint.h) as two
// EXPORTS of theirs. The sweep kernels themselves are launched unchanged:
//
//   backward seed   ds_{P-1}[e,i] += kc_{P-1}[e,i] sum_e2 Pi[e,e2] dV_P[i,e2]      after k_tan_back(first = 1), which produced the
//                                                                                   knots' tangent of period P-1 from dV_P = 0
//   forward seed    dD state [e][n_a + KV][N] := dD_0 in the real rows, zero in the KV virtual rows        in place of k_zero_f64
//   marginal path   m_{-1}[e] = sum_a dD_0[a,e],  m_t = m_{t-1} Pi;  zm[t] = sum_e z_e m_t[e],  om[t] = sum_e m_t[e]  (as m_{-1} . Pi^{t+1} z, 1)
//                   consumption's aggregate gains  w_t zm[t] + tr_t om[t]  (k_het_outputs assumes both sums vanish: they do when
//                   dD_0 = 0, see hank_set_boundary)
//   D_0 cotangent   Sweep A's state after its last launch (t = 0), exported before Sweep B reuses the buffer
//   V_P cotangent   mu_P[i,e2] = sum_e Pi[e,e2] kc_{P-1}[e,i] sbar_{P-1}[e,i]: the mu that Sweep B's last launch (last = 1) does
//                   not form, from the same pbar_{P-1}, mu_{P-1} and bracket segments, summed in the same order
//
// The caller's boundary arrays are (G, N) column-major, pt = e n_a + a (the convention of hank_get_dpolicy_seq); the states are
// [e][row][N], direction fastest. No atomics: every sum has a fixed order, so the same inputs give the same bits.
#pragma once
#include "hank_kernels.h"

namespace hank {

constexpr int BND_T = 32;      // tile edge of the two layout kernels; block = (BND_T, 8)

// (G, N) column-major -> state [e][rows][N], rows >= n_a: the rows past n_a (the forward state's virtual rows) are zeroed.
// grid (ceil(n_a / 32), ceil(N / 32), n_e): both sides move 256-byte pieces through a 32 x 32 LDS tile.
__global__ void __launch_bounds__(256) k_bnd_in(const double *__restrict__ in, int n_a, int n_e, int rows, int N, double *__restrict__ out) {
    __shared__ double tile[BND_T][BND_T + 1];
    const int e = blockIdx.z, a0 = blockIdx.x * BND_T, n0 = blockIdx.y * BND_T, tx = threadIdx.x, ty = threadIdx.y;
    const size_t G = (size_t)n_a * n_e;
    for (int k = ty; k < BND_T; k += 8) {
        const int a = a0 + tx, n = n0 + k;
        if (a < n_a && n < N) tile[k][tx] = in[(size_t)e * n_a + a + G * n];
    }
    __syncthreads();
    const int n = n0 + tx;
    if (n >= N) return;
    for (int k = ty; k < BND_T; k += 8) {
        const int a = a0 + k;
        if (a < n_a) out[((size_t)e * rows + a) * N + n] = tile[tx][k];
    }
    if (blockIdx.x == 0)
        for (int a = n_a + ty; a < rows; a += 8) out[((size_t)e * rows + a) * N + n] = 0.0;
}

// state [e][n_a][M] -> (G, M) column-major; the same grid and tile
__global__ void __launch_bounds__(256) k_bnd_out(const double *__restrict__ in, int n_a, int n_e, int M, double *__restrict__ out) {
    __shared__ double tile[BND_T][BND_T + 1];
    const int e = blockIdx.z, a0 = blockIdx.x * BND_T, m0 = blockIdx.y * BND_T, tx = threadIdx.x, ty = threadIdx.y;
    const size_t G = (size_t)n_a * n_e;
    for (int k = ty; k < BND_T; k += 8) {
        const int a = a0 + k, m = m0 + tx;
        if (a < n_a && m < M) tile[k][tx] = in[((size_t)e * n_a + a) * M + m];
    }
    __syncthreads();
    const int a = a0 + tx;
    if (a >= n_a) return;
    for (int k = ty; k < BND_T; k += 8) {
        const int m = m0 + k;
        if (m < M) out[(size_t)e * n_a + a + G * m] = tile[tx][k];
    }
}

// The backward seed. dV: the terminal value's tangent as a state [e2][n_a][N]; ds: the knots' tangent of period P-1 as
// k_tan_back(first = 1) left it; kc: the record's kc of period P-1 [e][n_a]. One thread per (row, direction); its n_e values of
// dV sit in its own column of the LDS tile (no other thread reads them: no barrier), the contraction is tan_back_body's
// dE[e] = sum_e2 Pi[e,e2] dV[e2], e2 ascending. grid ceil(n_a N / 256).
__global__ void __launch_bounds__(256) k_bnd_seed_back(Consts c, const double *__restrict__ kc, const double *__restrict__ dV, size_t N,
                                                       double *__restrict__ ds) {
    __shared__ double v[16 * 256];
    const size_t cnt = (size_t)c.n_a * N, j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int i = (int)(j / N);
    for (int e2 = 0; e2 < c.n_e; e2++) v[e2 * 256 + threadIdx.x] = dV[(size_t)e2 * cnt + j];
    for (int e = 0; e < c.n_e; e++) {
        double dE = 0.0;
        for (int e2 = 0; e2 < c.n_e; e2++) dE += c.Pi[e + c.n_e * e2] * v[e2 * 256 + threadIdx.x];
        ds[(size_t)e * cnt + j] += kc[(size_t)e * c.n_a + i] * dE;
    }
}

// m_{-1}[n][e] = sum_a dD_0[a, e, n] from the caller's (G, N) column-major seed: one block per (e, n), the rows strided over the
// threads and combined by block_sum (fixed order). grid (n_e, N).
__global__ void __launch_bounds__(256) k_bnd_marginal(const double *__restrict__ dD0, int n_a, int n_e, double *__restrict__ m0) {
    __shared__ double red[16];
    const int e = blockIdx.x, n = blockIdx.y;
    const double *col = dD0 + (size_t)e * n_a + (size_t)n_a * n_e * n;
    double s = 0.0;
    for (int a = threadIdx.x; a < n_a; a += 256) s += col[a];
    const double tot = block_sum(s, red, 256);
    if (threadIdx.x == 0) m0[(size_t)n * n_e + e] = tot;
}

// The productivity marginal of dD_t along the path is m_t = m_{t-1} Pi (post-transition, like D_t: the recursion hank_set_boundary
// runs for D_t's), so what consumption needs is zm[t] = sum_e z_e m_t[e] = m_{-1} . (Pi^{t+1} z) and om[t] = sum_e m_t[e] =
// m_{-1} . (Pi^{t+1} 1). The two vector paths Q = {Pi^{t+1} z, Pi^{t+1} 1} [2][P][n_e] belong to the model (the host makes them once per
// context: ensure_bnd_q), which leaves n_e products per (t, direction) here and no recurrence over the periods on the device:
// zm[t][n], zm[P + t][n]; e ascending. One thread per (t, direction).
__global__ void k_bnd_mpath(int P, int n_e, int N, const double *__restrict__ m0, const double *__restrict__ Q, double *__restrict__ zm) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int t = idx / N, n = idx - t * N;
    const double *m = m0 + (size_t)n * n_e, *qz = Q + (size_t)t * n_e, *q1 = Q + ((size_t)P + t) * n_e;
    double z = 0.0, one = 0.0;
    for (int e = 0; e < n_e; e++) { z += m[e] * qz[e]; one += m[e] * q1[e]; }
    zm[idx] = z;
    zm[(size_t)P * N + idx] = one;
}

// consumption's aggregate under a dD_0 seed: out_dagg (P, n_het, N) column-major as k_het_outputs wrote it, output 1
// += w_t zm[t] + tr_t om[t]. One thread per (t, direction).
__global__ void k_bnd_cons(int P, int n_hh, int n_het, int N, const double *__restrict__ xhh, const double *__restrict__ zm,
                           double *__restrict__ out_dagg) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int t = idx / N, n = idx - t * N;
    const double w = xhh[n_hh * t + 1], tr = n_hh > 2 ? xhh[n_hh * t + 2] : 0.0;
    out_dagg[((size_t)n * n_het + 1) * P + t] += w * zm[(size_t)t * N + n] + tr * zm[((size_t)P + t) * N + n];
}

// The cotangent of the terminal value: mu_P as a state [e2][n_a][M], from Sweep B's inputs of its last period t = P-1 (pbar_t,
// mu_t = muIn, the bracket segment starts sb of k_adj_seg). One thread per (knot row i, column m): column e's sbar gathers
// gbar = pbar_t - v_t mu_t over the rows that bracket on knot i — [sb[i-1], sb[i]) with weight B, [sb[i], sb[i+1]) with weight A,
// in row order, every index clamped as in k_adj_egm — and kc_t sbar waits in the thread's own column of the LDS tile (no
// barrier) for the contraction mu_P[i,e2] = sum_e Pi[e,e2] kc_t[e,i] sbar[e,i], e ascending. first: P = 1, mu_t = 0.
// grid ceil(n_a M / 256).
__global__ void __launch_bounds__(256) k_bnd_vend(Consts c, Record R, int t, int first, const int *__restrict__ sb, const double *__restrict__ muIn,
                                                  const double *__restrict__ pbar, size_t M, double *__restrict__ muOut) {
    __shared__ double ks[16 * 256];
    const int n = c.n_a, ne = c.n_e;
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (size_t)n * M) return;
    const int i = (int)(j / M);
    const size_t m = j - (size_t)i * M;
    for (int e = 0; e < ne; e++) {
        const size_t colb = (size_t)t * c.G + (size_t)e * n;
        const int *sbc = sb + ((size_t)t * ne + e) * (n + 1);
        const int b1 = min(max(sbc[i], 0), n), b0 = i > 0 ? min(max(sbc[i - 1], 0), b1) : b1, b2 = min(max(sbc[i + 1], b1), n);
        double sbar = 0.0;
        for (int a = b0; a < b2; a++) {
            double g = pbar[(colb + a) * M + m];
            if (!first) g -= R.v[colb + a] * muIn[((size_t)e * n + a) * M + m];
            sbar += (a < b1 ? R.B[colb + a] : R.A[colb + a]) * g;
        }
        ks[e * 256 + threadIdx.x] = R.kc[colb + i] * sbar;
    }
    for (int e2 = 0; e2 < ne; e2++) {
        double mu = 0.0;
        for (int e = 0; e < ne; e++) mu += c.Pi[e + ne * e2] * ks[e * 256 + threadIdx.x];
        muOut[((size_t)e2 * n + i) * M + m] = mu;
    }
}

}  // namespace hank
