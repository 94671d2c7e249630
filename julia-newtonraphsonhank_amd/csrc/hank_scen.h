// hank_scen.h — the scenario batch of hank_primal_batch: K independent input paths x_k through ONE chain of launches, with
// gridDim.y = K. Scenario k is the launch family's hank_primal at x_k: the kernels here call the same bodies (egm_X, egm_step_body,
// lottery_body, dist_step_body — the only places the household problem is written) on scenario k's
// record, scenario k's inputs and scenario k's error word, so its policy and its aggregate hold the bits of k_egm_X / k_egm_step /
// k_lottery / k_dist_step.
//
// The scenario index is blockIdx.y, uniform over the workgroup: a scenario's bases are the arguments' plus k times a stride, scalar
// arithmetic on kernel arguments, nothing per lane. The K records are carved alike from one slab, so ONE byte stride moves every
// array of the record from scenario 0 to scenario k (scen_record). A scenario record has no `seg` and no `lwg` (null): no reader of
// either runs here — k_scen_lottery writes no segment records (write_seg = 0) and k_scen_dist_step hands dist_step_body explicit
// D_{t-1} / D_t rows, the form that writes no {w, ig D} records.
#pragma once
#include "hank_kernels.h"
#include "hank_hetx.h"

namespace hank {

struct ScenArgs {
    Record R0;             // scenario 0's record
    size_t stride;         // bytes from a scenario's record to the next one's (a multiple of 256)
    const double *xhh;     // (n_hh, P, K) column-major: scenario k's inputs at xhh + n_hh P k
    int *err;              // [K][4]: one error word per scenario
};

__device__ __forceinline__ Record scen_record(const Record &R0, size_t off) {
    Record R = R0;
    R.s = (double *)((char *)R0.s + off); R.kc = (double *)((char *)R0.kc + off); R.A = (double *)((char *)R0.A + off);
    R.B = (double *)((char *)R0.B + off); R.u = (double *)((char *)R0.u + off); R.v = (double *)((char *)R0.v + off);
    R.pol = (double *)((char *)R0.pol + off); R.lw = (double *)((char *)R0.lw + off); R.ig = (double *)((char *)R0.ig + off);
    R.Dseq = (double *)((char *)R0.Dseq + off); R.ib = (int *)((char *)R0.ib + off); R.lo = (int *)((char *)R0.lo + off);
    R.start = (int *)((char *)R0.start + off); R.clo = (int *)((char *)R0.clo + off);
    return R;      // (seg, lwg: null in every scenario)
}
__device__ __forceinline__ const double *scen_xhh(const Consts &c, const ScenArgs &a, int k) { return a.xhh + (size_t)c.n_hh * c.P * k; }

// grid (nbp, K), block RBP n_e, LDS primal_lds: k_egm_X of period t from the terminal value every scenario shares
__global__ void k_scen_egm_X(Consts c, const double *Vin, ScenArgs a, int t) {
    extern __shared__ double sh[];
    const int k = blockIdx.y;
    const Record R = scen_record(a.R0, a.stride * k);
    const double *xt = scen_xhh(c, a, k) + c.n_hh * t;
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int ia = blockIdx.x * RBP + row;
    for (int q = threadIdx.x; q < c.n_e * c.n_e; q += blockDim.x) Pish[q] = c.Pi[q];
    if (ia < c.n_a) Vsh[e * RBP + row] = Vin[e * c.n_a + ia];
    __syncthreads();
    const size_t off = (size_t)t * c.G + (size_t)e * c.n_a + ia;
    if (ia < c.n_a) egm_X(c, Vsh, Pish, row, ia, e, xt[0], xt[1], c.n_hh > 2 ? xt[2] : 0.0, &R.s[off], &R.kc[off], a.err + 4 * k, t);
}

// grid (nbp, K), block RBP n_e, LDS primal_lds: k_egm_step of period t
__global__ void k_scen_egm_step(Consts c, ScenArgs a, int t) {
    extern __shared__ double sh[];
    const int k = blockIdx.y;
    egm_step_body(c, scen_record(a.R0, a.stride * k), scen_xhh(c, a, k), t, a.err + 4 * k, blockIdx.x, sh);
}

// grid (P n_e, K), block 256, LDS 2 n_a + 2 ints: k_lottery's body with write_seg = 0 and use_ib = 1
__global__ void k_scen_lottery(Consts c, ScenArgs a, int ncols) {
    extern __shared__ int shlo[];
    __shared__ int sh_clo;
    const int col = blockIdx.x, k = blockIdx.y;
    if (col >= ncols) return;
    lottery_body(c, scen_record(a.R0, a.stride * k), col, a.err + 4 * k, 0, 1, shlo, &sh_clo);
}

// grid (nbp, K), block RBP n_e, LDS primal_lds: k_dist_step of period t with aggpart [k][t][block][2]. D0: the initial distribution
// every scenario shares (period 0 reads it; later periods read the scenario's own rows). NX > 0: behind the step, one block sum per
// declared non-affine output jx (Value, UCE: hank_hetx.h), sum f_o(c) D_t over the block's points with c the budget residual from
// the scenario's recorded policy, the grids and the period's inputs -> hxpart [k][t][block][NX]. None of that runs for NX = 0.
__global__ void k_scen_dist_step(Consts c, ScenArgs a, const double *D0, int t, double *aggpart, int NX, double *hxpart) {
    extern __shared__ double sh[];
    const int k = blockIdx.y, nb = gridDim.x, n = c.n_a;
    const Record R = scen_record(a.R0, a.stride * k);
    double *Dt = R.Dseq + (size_t)(t + 1) * c.G;
    dist_step_body(c, R, t, aggpart + (size_t)k * c.P * nb * 2, blockIdx.x, nb, sh, t == 0 ? D0 : R.Dseq + (size_t)t * c.G, Dt);
    if (NX <= 0) return;
    double *red = sh + c.n_e * RBP + c.n_e * c.n_e;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP, r = blockIdx.x * RBP + row;
    const double *x = scen_xhh(c, a, k) + c.n_hh * t;
    const double rt = x[0], w = x[1], tr = c.n_hh > 2 ? x[2] : 0.0;
    double acc[2] = {0.0, 0.0};
    if (r < n) {
        const size_t pt = (size_t)e * n + r;
        const double D = Dt[pt];      // (this thread's own store of dist_step_body)
        const double av = c.a[r], z = c.z[e];
        const double cons = (1.0 + rt) * av + w * z + tr - R.pol[(size_t)t * c.G + pt];
        for (int jx = 0; jx < NX; jx++) {
            double f, fc, fr;
            hx_f(2 + jx, c.gamma, rt, z, cons, f, fc, fr);
            acc[jx] = f * D;
        }
    }
    for (int jx = 0; jx < NX; jx++) {
        const double tot = block_sum(acc[jx], red, RBP * c.n_e);
        if (threadIdx.x == 0) hxpart[(((size_t)k * c.P + t) * nb + blockIdx.x) * NX + jx] = tot;
    }
}

// outputs 0 .. n_het-1 of every scenario, (P, n_het, K) column-major, the value half of k_het_outputs (out_cons):
// agg [k][t][2] and hx [k][t][NX] as k_reduce_parts leaves them over K P rows; zd does not depend on the scenario
__global__ void k_scen_outputs(int P, int n_hh, int n_het, int K, const double *__restrict__ xhh, const double *__restrict__ agg,
                               const double *__restrict__ zd, const double *__restrict__ hx, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * K) return;
    const int t = idx % P, k = idx / P;
    const int NX = n_het > 2 ? n_het - 2 : 0;
    const double *x = xhh + (size_t)n_hh * ((size_t)P * k + t);
    const double r = x[0], w = x[1], tr = n_hh > 2 ? x[2] : 0.0;
    const double KD = agg[(size_t)idx * 2], AD = agg[(size_t)idx * 2 + 1], ZD = zd[t], MD = zd[P + t];
    double *o = out + (size_t)k * n_het * P + t;
    o[0] = KD;
    if (n_het > 1) o[P] = out_cons(r, w, tr, AD, ZD, MD, KD);
    for (int jx = 0; jx < NX; jx++) o[(size_t)(2 + jx) * P] = hx[(size_t)idx * NX + jx];
}

}  // namespace hank
