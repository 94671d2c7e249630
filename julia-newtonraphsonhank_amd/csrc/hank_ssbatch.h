// hank_ssbatch.h — the scenario batch of hank_ss_batch: the steady state's household side (SteadyState.jl:132-141, then
// ForwardIteration.jl:436-442) at K constant price vectors through ONE chain of launches, with gridDim.y = K. Scenario k's value loop
// is hank_vfi's launch branch at x_k and its power method is hank_stationary_dist's: the kernels here call the same bodies (egm_X,
// egm_Y, supnorm_block, lottery_body, dist_step_body, hx_f — the only places the household problem is written) on scenario k's
// buffers, scenario k's prices and scenario k's error word, so its value, policy, step count and distribution hold the bits of
// k_egm_X / k_egm_Y / k_vfi_check / k_lottery / k_dist_iter.
//
// The scenario index is blockIdx.y (blockIdx.x in the one-block-per-scenario kernels), uniform over the workgroup. The K workspaces
// are carved alike from one slab, so ONE byte stride moves every array from scenario 0 to scenario k (ssb_at), as scen_record does.
// What differs from hank_scen.h is that the scenarios do not finish together: each owns a stop word per loop, in a 64-byte line of its
// own (K row blocks poll it, one block writes it), and a stopped scenario's workgroups return at once while the others go on. The
// launches are issued in lockstep, so the ping-pong parity of a step is the launch's; a scenario that stopped after n steps keeps its
// state in buffer n & 1.
#pragma once
#include "hank_kernels.h"
#include "hank_hetx.h"

namespace hank {

// a loop's stop word of one scenario: stop 0 running, 1 its rule held, 2 its error word was set (the verdict is the host's);
// n = value steps, or distribution iterations applied; norm = the last max|difference|
struct alignas(64) SsbCtl { int stop, n; double norm; };
constexpr int SSB_FAILED = 2;

struct SsbArgs {
    double *V[2], *sK, *kc, *A, *B, *u, *v;      // scenario 0's value double buffer and one-period EGM record
    int *ib;
    Record R0;                                   // scenario 0's one-period lottery record: pol, lw, ig, lo, start, clo (the rest null)
    double *D[2], *Dchk, *aggp;                  // scenario 0's distribution double buffer, last checked iterate, dist_step_body's block sums
    size_t stride;                               // bytes from a scenario's workspace to the next one's (a multiple of 256)
    const double *xhh;                           // (n_hh, K) column-major
    int *err;                                    // [K][4]: one error word per scenario
    SsbCtl *vctl, *dctl;                         // [K] each: the value loop's and the power method's stop words
};

template <typename T> __device__ __forceinline__ T *ssb_at(T *p, size_t off) { return (T *)((char *)p + off); }
__device__ __forceinline__ Record ssb_record(const Record &R0, size_t off) {
    Record R = R0;
    R.pol = ssb_at(R0.pol, off); R.lw = ssb_at(R0.lw, off); R.ig = ssb_at(R0.ig, off);
    R.lo = ssb_at(R0.lo, off); R.start = ssb_at(R0.start, off); R.clo = ssb_at(R0.clo, off);
    return R;
}

// grid (nbp, K), block RBP n_e, LDS primal_lds: k_egm_X of value step `cur` (it reads V[cur])
__global__ void k_ssb_egm_X(Consts c, SsbArgs a, int cur) {
    extern __shared__ double sh[];
    const int k = blockIdx.y;
    if (a.vctl[k].stop) return;
    const size_t o = a.stride * k;
    const double *Vin = ssb_at(a.V[cur], o), *xt = a.xhh + (size_t)c.n_hh * k;
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int ia = blockIdx.x * RBP + row;
    for (int q = threadIdx.x; q < c.n_e * c.n_e; q += blockDim.x) Pish[q] = c.Pi[q];
    if (ia < c.n_a) Vsh[e * RBP + row] = Vin[e * c.n_a + ia];
    __syncthreads();
    if (ia < c.n_a)
        egm_X(c, Vsh, Pish, row, ia, e, xt[0], xt[1], c.n_hh > 2 ? xt[2] : 0.0, &ssb_at(a.sK, o)[e * c.n_a + ia], &ssb_at(a.kc, o)[e * c.n_a + ia], a.err + 4 * k, 0);
}

// grid (nbp, K), block RBP n_e: k_egm_Y of value step `cur` (it writes V[cur ^ 1])
__global__ void k_ssb_egm_Y(Consts c, SsbArgs a, int cur) {
    const int k = blockIdx.y;
    if (a.vctl[k].stop) return;
    const size_t o = a.stride * k;
    const double *xt = a.xhh + (size_t)c.n_hh * k;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int ia = blockIdx.x * RBP + row;
    if (ia >= c.n_a) return;
    const YOut y = egm_Y(c, ssb_at(a.sK, o) + e * c.n_a, ia, e, xt[0], xt[1], c.n_hh > 2 ? xt[2] : 0.0, a.err + 4 * k, 0, -1);
    const int off = e * c.n_a + ia;
    ssb_at(a.R0.pol, o)[off] = y.g; ssb_at(a.ib, o)[off] = y.ib; ssb_at(a.A, o)[off] = y.A; ssb_at(a.B, o)[off] = y.B;
    ssb_at(a.u, o)[off] = y.u; ssb_at(a.v, o)[off] = y.v;
    ssb_at(a.V[cur ^ 1], o)[off] = y.V;
}

// grid (K), block 1024: k_vfi_check of value step `cur` for every scenario still running; a scenario whose error word is set
// stops here with SSB_FAILED (n names the step that raised it)
__global__ void k_ssb_vfi_check(SsbArgs a, int G, int cur, double tol) {
    __shared__ double red[16];
    const int k = blockIdx.x;
    SsbCtl *ctl = a.vctl + k;
    if (ctl->stop) return;
    const size_t o = a.stride * k;
    const double m = supnorm_block(ssb_at(a.V[cur ^ 1], o), ssb_at(a.V[cur], o), G, red);
    if (threadIdx.x == 0) {
        ctl->n += 1;
        ctl->norm = m;
        if (a.err[4 * k]) ctl->stop = SSB_FAILED;
        else if (m < tol) ctl->stop = 1;
    }
}

// grid (n_e, K), block 256, LDS 2 n_a + 2 ints: k_lottery on scenario k's policy as hank_stationary_dist calls it (the bisection:
// use_ib = 0); no segment records (write_seg = 0: dist_step_body reads `start`). A scenario whose value loop failed is skipped.
__global__ void k_ssb_lottery(Consts c, SsbArgs a) {
    extern __shared__ int shlo[];
    __shared__ int sh_clo;
    const int k = blockIdx.y;
    if (a.vctl[k].stop == SSB_FAILED) return;
    lottery_body(c, ssb_record(a.R0, a.stride * k), blockIdx.x, a.err + 4 * k, 0, 0, shlo, &sh_clo);
}

// grid (ceil(K / 64)), block 64: the power method's stop words. A scenario whose error word is set by now (the value loop, the
// lottery: a policy that is not monotone leaves segment offsets nobody may follow) never starts.
__global__ void k_ssb_dist_init(SsbArgs a, int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    a.dctl[k].stop = a.err[4 * k] ? SSB_FAILED : 0;
    a.dctl[k].n = 0;
    a.dctl[k].norm = 0.0;
}

// grid (nbp, K), block RBP n_e, LDS primal_lds: k_dist_iter, iteration `cur` (D[cur] -> D[cur ^ 1])
__global__ void k_ssb_dist_iter(Consts c, SsbArgs a, int cur) {
    extern __shared__ double sh[];
    const int k = blockIdx.y;
    if (a.dctl[k].stop) return;
    const size_t o = a.stride * k;
    dist_step_body(c, ssb_record(a.R0, o), 0, ssb_at(a.aggp, o), blockIdx.x, gridDim.x, sh, ssb_at(a.D[cur], o), ssb_at(a.D[cur ^ 1], o));
}

// grid (K), block 1024: the power method's check behind `n` more iterations, the newest iterate in D[cur]: max|D - Dchk| < tol stops
// the scenario with D[cur] as its result (exactly ctl->n applications); otherwise D[cur] becomes the last checked iterate
__global__ void k_ssb_dist_check(SsbArgs a, int G, int cur, int n, double tol) {
    __shared__ double red[16];
    __shared__ int go;
    const int k = blockIdx.x;
    SsbCtl *ctl = a.dctl + k;
    if (ctl->stop) return;
    const size_t o = a.stride * k;
    const double *Dn = ssb_at(a.D[cur], o);
    double *Dc = ssb_at(a.Dchk, o);
    const double m = supnorm_block(Dn, Dc, G, red);
    if (threadIdx.x == 0) {
        ctl->n += n;
        ctl->norm = m;
        go = !(m < tol);
        if (!go) ctl->stop = 1;
    }
    __syncthreads();
    if (go)
        for (int i = threadIdx.x; i < G; i += blockDim.x) Dc[i] = Dn[i];
}

// grid (n_het, K), block 1024: Y_o = sum f_o D / sum D over scenario k's points, f_o of hank_get_het_outputs (0 the policy, 1
// consumption, 2 Value, 3 UCE: hx_f). Every thread sums its points in index order, block_sum combines the threads in a fixed order,
// no atomics: the same inputs give the same bits. A failed scenario is skipped.
__global__ void __launch_bounds__(1024) k_ssb_outputs(Consts c, SsbArgs a, int n_het, double *__restrict__ out) {
    __shared__ double red[16];
    const int o_ = blockIdx.x, k = blockIdx.y;
    const SsbCtl *ctl = a.dctl + k;
    if (ctl->stop == SSB_FAILED) return;
    const size_t o = a.stride * k;
    const double *D = ssb_at(a.D[ctl->n & 1], o), *pol = ssb_at(a.R0.pol, o), *xt = a.xhh + (size_t)c.n_hh * k;
    const double r = xt[0], w = xt[1], tr = c.n_hh > 2 ? xt[2] : 0.0;
    double num = 0.0, den = 0.0;
    for (int pt = threadIdx.x; pt < c.G; pt += blockDim.x) {
        const int e = pt / c.n_a, ia = pt - e * c.n_a;
        const double d = D[pt], ap = pol[pt];
        double f = ap;
        if (o_ >= 1) {
            const double cons = (1.0 + r) * c.a[ia] + w * c.z[e] + tr - ap;
            f = cons;
            if (o_ >= 2) { double fc, fr; hx_f(o_, c.gamma, r, c.z[e], cons, f, fc, fr); }
        }
        num += f * d;
        den += d;
    }
    const double tn = block_sum(num, red, blockDim.x);
    const double td = block_sum(den, red, blockDim.x);
    if (threadIdx.x == 0) out[(size_t)k * n_het + o_] = tn / td;
}

// grid (ceil(G / 256), K), block 256: every scenario's results side by side — value from V[steps & 1], the policy, D from
// D[iterations & 1] (Dexp null: no distribution was asked for) — (G, K) column-major each
__global__ void k_ssb_export(SsbArgs a, int G, double *__restrict__ Vexp, double *__restrict__ Pexp, double *__restrict__ Dexp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= G) return;
    const size_t o = a.stride * k, q = (size_t)k * G + i;
    Vexp[q] = ssb_at(a.V[a.vctl[k].n & 1], o)[i];
    Pexp[q] = ssb_at(a.R0.pol, o)[i];
    if (Dexp) Dexp[q] = ssb_at(a.D[a.dctl[k].n & 1], o)[i];
}

}  // namespace hank
