// hank_device.h — what a kernel of the household block is built from: the argument structs, the constants, the lane helpers and the
// bodies that more than one kernel is a wrapper of, in either translation unit (hank_hip.hip's sweeps, hank_ssdiff.hip's fixed-point
// steps): tan_back_body, tan_fwd_body, lottery_body, adj_dist_body, adj_egm_body and the outputs' arithmetic (out_*, xbar_*).
// It defines no __global__ function and no __device__ variable, so any number of units may include it. hank_kernels.h,
// hank_hetx.h, hank_adjoint.h and hank_boundary.h include it and hold the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hank_geom.h"

// dev knobs of the Dual pass's forward sweep (A-B builds; with both at 0 every kernel is the one before them):
//   HANK_XFWD_LQ           one 16-byte load of a source's packed lottery record {w, lo, flags} instead of lo, lw and ig
//                          (k_lottery_lq writes it, k_xfwd<D, true, MAXT, true> reads it; ig comes from a table of the grid's inverse gaps in LDS)
//   HANK_XFWD_EARLY_BATCH  the next period's unit batch is issued in front of the period's second barrier, not behind it
//                          (measured and lost, +0.18 ms per step: off)
#ifndef HANK_XFWD_LQ
#define HANK_XFWD_LQ 1
#endif
#ifndef HANK_XFWD_EARLY_BATCH
#define HANK_XFWD_EARLY_BATCH 0
#endif
// dev knobs of the forward sweeps' source walk (the cost of ds_add_f64 by its lanes' addresses: scripts/ubench/lds_add_bench.hip,
// DESIGN.md section 4; with both at 0 every kernel is the one before them):
//   HANK_XFWD_TILE_SOA     k_xfwd<D, true, MAXT, true>'s tile is slot-major, [column][slot][lane] (hank_xlds.h): adds into consecutive
//                          target rows hit consecutive banks. Same sums in the same order: the outputs' bits do not move
//                          (measured and kept, -0.075 ms per step: on)
//   HANK_XFWD_FLAT_TR      a flat work unit (more than XFLAT_NUM / XFLAT_DEN sources per target row) deals its sources four apart
//                          inside each 16-lane group, in EVERY k_xfwd (same-address lanes of a group are added one after the other)
//                          (measured and lost, +0.03 ms per step alone and beside the slot-major tile: off)
#ifndef HANK_XFWD_TILE_SOA
#define HANK_XFWD_TILE_SOA 1
#endif
#ifndef HANK_XFWD_FLAT_TR
#define HANK_XFWD_FLAT_TR 0
#endif

namespace hank {

// a work unit is FLAT at more than 3/2 sources per target row: from there on some 16-lane group holds a run of two sources on one row,
// 20 cycles per ds_add_f64 in the slot-major tile against 16 for sources dealt four apart (32 and 44 against 16 and 11 at three and four)
constexpr int XFLAT_NUM = 3, XFLAT_DEN = 2;

struct Consts {
    int n_a, n_e, G, P;
    int n_hh;   // household inputs per period: 2 = (r, w) Krusell-Smith; 3 = (r, w, tr) one-asset HANK (lump-sum transfer)
    int diet;   // the tangent sweeps rebuild kc from s and v from u instead of reading them (CRRA with gamma = 1 or 2: see diet_kc)
    double beta, gamma, bc;
    const double *a, *z, *Pi;  // device
};

struct Record {
    double *s, *kc, *A, *B, *u, *v, *pol, *lw, *ig, *Dseq;
    int *ib, *lo, *start, *clo;
    int4 *seg;      // per target row: {start[r-1], start[r], start[r+1], -} — ONE read instead of three
    double2 *lwg;   // per source row: {lottery weight w, weight-tangent factor ig * D_{t-1}} — ONE 16-byte read per source in the forward tangent kernel
};

// ---- block reductions (64-wide wavefronts) ------------------------------------------------
__device__ inline double wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
// sum over the first `nthreads` threads of the block (the others must have left the kernel);
// result valid in thread 0; red must hold >= 16 doubles
__device__ inline double block_sum(double x, double *red, int nthreads) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nw = (nthreads + 63) >> 6;
    x = wave_sum(x);
    __syncthreads();
    if (lane == 0) red[wv] = x;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < nw; k++) r += red[k];
    return r;
}

// Workgroup barrier for LDS hand-offs: waits for this wave's LDS operations only. __syncthreads() carries a fence that
// also drains vmcnt — every write-through (sc1) store issued before it would have to reach memory before the barrier
// opens, although nothing behind these barriers reads global memory another thread of the block wrote.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// how the big streaming stores (policy partials, tangent state) leave the CU: sc1 write-through. The record's stores are plain.
__device__ __forceinline__ void st_wt(double *p, double x) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// acc += sum_{k=k0}^{n-1} P[k*ps] * V[k*vs], added in index order. The n_e-long mixing sums sit on every launch's
// critical path; as a plain loop each LDS read waits for the one before (n_e round trips of ~100 clocks: the launch
// floor is 4.1 us at n_e = 4 and 6.2 us at n_e = 11). Reads are issued four columns at a time, the order of the
// additions is unchanged.
__device__ __forceinline__ double mix_mul(double p, double v) { return p * v; }
__device__ __forceinline__ double2 mix_mul(double p, double2 v) { return make_double2(p * v.x, p * v.y); }
__device__ __forceinline__ double mix_add(double a, double b) { return a + b; }
__device__ __forceinline__ double2 mix_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
template <typename T>
__device__ __forceinline__ T mix_sum(T acc, const T *V, int vs, const double *P, int ps, int k0, int n) {
    int k = k0;
    for (; k + 3 < n; k += 4) {
        const T v0 = V[k * vs], v1 = V[(k + 1) * vs], v2 = V[(k + 2) * vs], v3 = V[(k + 3) * vs];
        const double p0 = P[k * ps], p1 = P[(k + 1) * ps], p2 = P[(k + 2) * ps], p3 = P[(k + 3) * ps];
        acc = mix_add(acc, mix_mul(p0, v0));
        acc = mix_add(acc, mix_mul(p1, v1));
        acc = mix_add(acc, mix_mul(p2, v2));
        acc = mix_add(acc, mix_mul(p3, v3));
    }
    if (k + 1 < n) {
        const T v0 = V[k * vs], v1 = V[(k + 1) * vs];
        const double p0 = P[k * ps], p1 = P[(k + 1) * ps];
        acc = mix_add(acc, mix_mul(p0, v0));
        acc = mix_add(acc, mix_mul(p1, v1));
        k += 2;
    }
    if (k < n) acc = mix_add(acc, mix_mul(P[k * ps], V[k * vs]));
    return acc;
}

// household inputs of period t: xhh[n_hh*t + k]; the lump-sum transfer is 0 for families without one
__device__ __forceinline__ double hh_tr(const Consts &c, const double *xhh, int t) { return c.n_hh > 2 ? xhh[c.n_hh * t + 2] : 0.0; }

// KV virtual rows per column (rows n_a .. n_a+KV-1 of the dD state) hold partial sums of the
// mass-point row 0 — see k_tan_fwd.

constexpr int KV = 16;

// one backward period: Y-tangent of period t (bracket gather -> dpol_t, dV_t), then X-tangent of
// period t-1 (mix over e -> knot tangents ds_{t-1}). `first`: dV_{t+1} = 0 for the last period
// (terminal value has zero partials, BackwardIteration.jl:85) => only the X half, from zeros.
// ds ping-pongs between two [e][a][N] buffers that live in L2 / Infinity Cache.
// RG = row groups per wave: a wave walks RG groups of RB = 64/NC rows with all their loads in
// flight together (the host picks RG per batch width: tan_rg in hank_hip.hip).
// Tangent lanes are templated on VT = double (one direction per lane) or double2 (two adjacent directions per
// lane: every state / dpol access is a 16-byte one, half the vector-memory instructions per byte; the memory
// layout [..][N] is the same, N even). g.N / g.NC count VT elements.
__device__ __forceinline__ void vzero(double &v) { v = 0.0; }
__device__ __forceinline__ void vzero(double2 &v) { v.x = 0.0; v.y = 0.0; }
__device__ __forceinline__ double vshfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ double2 vshfl_xor(double2 v, int m) { return make_double2(__shfl_xor(v.x, m, 64), __shfl_xor(v.y, m, 64)); }
__device__ __forceinline__ void st_wt(double2 *p, double2 v) {
    // one 16-byte write-through store (there is no 16-byte atomic store to spell it with); the trailing
    // s_nop keeps the compiler's next instruction off the data registers until the store has read them
    typedef double d2_t __attribute__((ext_vector_type(2)));
    d2_t d = {v.x, v.y};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(d) : "memory");
}
__device__ __forceinline__ void lds_add(double *p, double v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add(double2 *p, double2 v) { lds_add(&p->x, v.x); lds_add(&p->y, v.y); }
__device__ __forceinline__ double2 vmul(double a, double2 v) { return make_double2(a * v.x, a * v.y); }
__device__ __forceinline__ double vmul(double a, double v) { return a * v; }
__device__ __forceinline__ double2 vadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ double2 vsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double vsub(double a, double b) { return a - b; }

// XCD-aware block order. The dispatcher deals workgroups to the 8 XCDs round-robin (block p lands on XCD p mod 8), each XCD
// has its own L2, and neighbouring row blocks gather from overlapping rows: with the natural order every XCD touches every
// part of the state and a line is fetched by up to 8 L2s. Here the blocks that share an XCD own CONTIGUOUS row ranges
// (XCD x: logical blocks [start_x, start_x + count_x)), so a state line is fetched once, twice at the 7 seams. A
// bijection on [0, nb): nothing depends on where a block really runs.
// Measured at 2000x11: backward sweep -3 % at N=32, -8 % at N=64 and 128, -3 % at N=256; forward sweep -3 % at N=16, nothing
// at N=32 and +8..12 % (slower) from N=64 on, where one row block's data is many lines already and the natural order
// spreads the XCDs' requests better over the memory channels: the forward sweep keeps the natural order there.
#ifndef HANK_XCDMAP_FWD_MAXN
#define HANK_XCDMAP_FWD_MAXN 32
#endif
__device__ __forceinline__ int xcd_contiguous(int p, int nb) {
    const int x = p & 7, k = p >> 3, q = nb >> 3, rem = nb & 7;
    return x * q + (x < rem ? x : rem) + k;
}

template <int RG, typename VT>
__device__ inline void tan_back_body(const Consts &c, const Record &R, const double *__restrict__ xhh, const VT *__restrict__ dxr,
           const VT *__restrict__ dxw, const VT *__restrict__ dxt, const TanGeom &g, int t, int first, const VT *__restrict__ dsIn,
           VT *__restrict__ dsOut, VT *__restrict__ dpol, int bidx_phys, int bidy, VT (*dVsh)[16 * 64], double *Pish) {
    const int nbr_b = (g.nbx + RG - 1) / RG;
    const int bidx = (bidx_phys < nbr_b) ? xcd_contiguous(bidx_phys, nbr_b) : bidx_phys;
    const int nthr = 64 * c.n_e;
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (the column in a scalar register: its bases become scalar)
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC;
    const int RB = 64 >> g.lgNC;
    const int n = bidy * g.NC + nl;
    const size_t N = g.N;
    const int tx = first ? t : t - 1;   // period whose knots are produced
    const int txc = tx < 0 ? 0 : tx;
    int a[RG], bi[RG];
    bool valid[RG];
    double cA[RG], cB[RG], cu[RG], cv[RG], ck[RG], cs[RG], xa[RG];
#pragma unroll
    for (int q = 0; q < RG; q++) {
        a[q] = (bidx * RG + q) * RB + rl;
        valid[q] = (a[q] < c.n_a) && (n < g.N);
    }
    if (RG * RB <= 64) {
        // The record coefficients depend on the wealth row only: a wave touches RG*RB <= 64 distinct rows,
        // so ONE lane-sparse load per array (lane L fetches row L) plus cross-lane broadcasts replaces RG
        // full-width loads per array — the vector memory path is the scarce unit here (a full 64-lane
        // 8-byte load occupies it for >= 8 clocks however few distinct addresses it has).
        const int qa = lane / RB, ra = lane - qa * RB;
        const int al = (bidx * RG + qa) * RB + ra;
        int l_i = 0;
        double l_A = 0, l_B = 0, l_u = 0, l_v = 0, l_k = 0, l_s = 0, l_x = 0;
        if (lane < RG * RB && al < c.n_a) {
            const size_t pt = (size_t)e * c.n_a + al;
            const size_t off = (size_t)t * c.G + pt, off1 = (size_t)txc * c.G + pt;
            l_i = R.ib[off]; l_A = R.A[off]; l_B = R.B[off]; l_u = R.u[off]; l_v = R.v[off];
            l_k = R.kc[off1]; l_s = R.s[off1]; l_x = c.a[al];
        }
#pragma unroll
        for (int q = 0; q < RG; q++) {
            const int src = q * RB + rl;
            bi[q] = __shfl(l_i, src, 64); cA[q] = __shfl(l_A, src, 64); cB[q] = __shfl(l_B, src, 64);
            cu[q] = __shfl(l_u, src, 64); cv[q] = __shfl(l_v, src, 64); ck[q] = __shfl(l_k, src, 64);
            cs[q] = __shfl(l_s, src, 64); xa[q] = __shfl(l_x, src, 64);
        }
    } else {
#pragma unroll
        for (int q = 0; q < RG; q++) {
            bi[q] = 0; cA[q] = cB[q] = cu[q] = cv[q] = ck[q] = cs[q] = xa[q] = 0.0;
            if (valid[q]) {
                const size_t pt = (size_t)e * c.n_a + a[q];
                const size_t off = (size_t)t * c.G + pt, off1 = (size_t)txc * c.G + pt;
                bi[q] = R.ib[off]; cA[q] = R.A[off]; cB[q] = R.B[off]; cu[q] = R.u[off]; cv[q] = R.v[off];
                ck[q] = R.kc[off1]; cs[q] = R.s[off1]; xa[q] = c.a[a[q]];
            }
        }
    }
    const bool nok = n < g.N;
    VT dr, dw, dr1, dw1, dtr, dtr1;     // dtr: tangent of the lump-sum transfer (families with n_hh = 3)
    vzero(dr); vzero(dw); vzero(dr1); vzero(dw1); vzero(dtr); vzero(dtr1);
    if (nok) {
        dr = dxr[(size_t)t * N + n]; dw = dxw[(size_t)t * N + n];
        dr1 = dxr[(size_t)txc * N + n]; dw1 = dxw[(size_t)txc * N + n];
        if (c.n_hh > 2) { dtr = dxt[(size_t)t * N + n]; dtr1 = dxt[(size_t)txc * N + n]; }
    }
    const double ze = c.z[e], rho1 = 1.0 / (1.0 + xhh[c.n_hh * txc]);

    VT d0[RG], d1[RG];
#pragma unroll
    for (int q = 0; q < RG; q++) {
        vzero(d0[q]); vzero(d1[q]);
        if (valid[q] && !first) {
            const VT *col = dsIn + ((size_t)e * c.n_a) * N + n;
            d0[q] = col[(size_t)bi[q] * N]; d1[q] = col[(size_t)(bi[q] + 1) * N];
        }
    }
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += nthr) Pish[k] = c.Pi[k];
#pragma unroll
    for (int q = 0; q < RG; q++) {
        VT dV;
        vzero(dV);
        if (valid[q] && !first) {
            const VT dg = vadd(vmul(cA[q], d0[q]), vmul(cB[q], d1[q]));
            st_wt(&dpol[((size_t)t * c.G + (size_t)e * c.n_a + a[q]) * N + n], dg);
            dV = vadd(vmul(cu[q], dr), vmul(cv[q], vsub(vadd(vmul(xa[q], dr), vadd(vmul(ze, dw), dtr)), dg)));
        }
        dVsh[q][e * 64 + lane] = dV;
    }
    lds_barrier();
    if (tx < 0) return;
#pragma unroll
    for (int q = 0; q < RG; q++) {
        if (valid[q]) {
            const VT dE = mix_sum(vmul(Pish[e], dVsh[q][lane]), &dVsh[q][lane], 64, Pish + e, c.n_e, 1, c.n_e);
            st_wt(&dsOut[((size_t)e * c.n_a + a[q]) * N + n],
                                   vsub(vmul(ck[q], dE), vmul(rho1, vadd(vadd(vmul(ze, dw1), dtr1), vmul(cs[q], dr1)))));
        }
    }
}

// one forward period: segment gather of the lottery tangent (ForwardIteration.jl:37-99 under
// Dual), mix over e, aggregate dagg_t = sum(dpol_t * D_t + pol_t * dD_t) with the POST-transition
// D_t (:301-307). dD state: [e][n_a + KV][N].
//   blocks [0, nbx):      regular target rows; sources j >= clo only.
//   blocks [nbx, nbx+KV): the mass point. Block p sums its share of the clamped prefix [0, clo_e)
//     of every column (weight one, no weight tangent) plus, when row 0 itself is clamped, its share
//     of last period's virtual rows; after the mix the result is stored as VIRTUAL ROW n_a+p: row
//     0's tangent is (real row 0) + sum_p (virtual row p). Everything downstream is linear, so the
//     parts are never combined: a virtual row is a source with row 0's lottery (no own policy
//     tangent), and its aggregate term uses pol[0, e].
// NX extra reductions (hx: nothing for NX = 0, today's kernel): the in-period sums of the outputs that are not affine in the policy
// (hank_hetx.h), T_o,t = sum f_o,t dD_t - sum f_c,o,t D_t da'_t — the reduction made for the policy variable with other per-point
// weights: f_o,t at the target rows next to pol, f_c,o,t at the source rows next to D_t. hx.parts: [t][block][NX][N], the blocks
// summed in order by k_reduce_hx. The block reduction of the extra slots reuses the `sh` tiles (free after the mixing) behind one
// more barrier, so sh has max(RG, NX) tiles there.
template <typename VT, int NX>
struct TanHx { const double *f, *fc; VT *parts; };      // f, f_c [jx][P][G] (k_hx_record)
template <typename VT>
struct TanHx<VT, 0> {};
template <int RG, typename VT, bool SS, int NX = 0>
__device__ inline void tan_fwd_body(const Consts &c, const Record &R, const TanGeom &g, int t, const VT *__restrict__ dDin, VT *__restrict__ dDout,
          const VT *__restrict__ dpol, VT *__restrict__ aggpart, int bidx_phys, int bidy, int nbx_total, VT (*sh)[16 * 64], double *Pish, VT *red, VT *red2,
          TanHx<VT, NX> hx = TanHx<VT, NX>()) {
    const int nbr_f = (g.nbx + RG - 1) / RG;            // regular blocks; the mass-point blocks behind them keep their place
    const int bidx = (g.N * (int)(sizeof(VT) / 8) <= HANK_XCDMAP_FWD_MAXN && bidx_phys < nbr_f) ? xcd_contiguous(bidx_phys, nbr_f) : bidx_phys;
    const int nthr = 64 * c.n_e;
    const int lane = threadIdx.x & 63, e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (the column in a scalar register: its bases become scalar)
    const int nl = lane & (g.NC - 1), rl = lane >> g.lgNC;
    const int RB = 64 >> g.lgNC;
    const int n = bidy * g.NC + nl;
    const size_t N = g.N;
    const int na = c.n_a, nav = c.n_a + KV;
    const size_t base = (size_t)t * c.G, cb = base + (size_t)e * na;
    const double *Dnew = R.Dseq + base + c.G + (size_t)e * na;
    const VT *dDc = dDin + ((size_t)e * nav) * N + n;
    const VT *dpc = dpol + cb * N + n;
    const int clo = R.clo[(size_t)t * c.n_e + e];
    const int nbr = (g.nbx + RG - 1) / RG;            // regular blocks
    const bool virt_block = bidx >= nbr;
    const bool nok = n < g.N;
    int r[RG];
    bool valid[RG];
    VT acc[RG];
    double cp[RG];
    VT pagg;              // sum of dpol_j * D_t[j] over the sources this thread owns
    vzero(pagg);
    [[maybe_unused]] VT paggx[NX > 0 ? NX : 1];        // minus the same sources' f_c,o,t[j] * D_t[j] * dpol_j, per extra output
    [[maybe_unused]] double cfx[RG][NX > 0 ? NX : 1];  // f_o,t at the thread's target rows (a virtual row carries row 0's, as it carries pol of row 0)
    [[maybe_unused]] const size_t PG = (size_t)c.P * c.G;
    if constexpr (NX > 0) {
#pragma unroll
        for (int o = 0; o < NX; o++) vzero(paggx[o]);
    }
    bool in_lds = false;   // the gathered tile already sits in sh (source-stationary path)
    if (SS && !virt_block) {
        // SOURCE-STATIONARY form: the block owns the RG*RB target rows [r0, r0+rows); column e's wave walks the
        // contiguous source range that feeds them, RB source rows per instruction, and adds each source's two lottery
        // parts into the LDS tile of its target rows (ds_add_f64; a wave only touches its own column's tile).
        // Every source row is loaded once per block (the gather form loads it for both of its target rows, 35 %
        // more fabric reads at N=32) with half the vector-memory instructions per row.
        const int rows = RG * RB, r0 = bidx * rows, lgRB = 6 - g.lgNC;
#pragma unroll
        for (int q = 0; q < RG; q++) {
            r[q] = r0 + q * RB + rl;
            valid[q] = (r[q] < na) && nok;
            vzero(acc[q]);
            cp[q] = valid[q] ? R.pol[cb + r[q]] : 0.0;
            if constexpr (NX > 0) {
#pragma unroll
                for (int o = 0; o < NX; o++) cfx[q][o] = valid[q] ? hx.f[o * PG + cb + r[q]] : 0.0;
            }
            sh[q][e * 64 + lane] = acc[q];
        }
        const int *st = R.start + ((size_t)t * c.n_e + e) * (na + 1);
        const int rend = min(r0 + rows, na);
        const int jlo = st[r0 > 0 ? r0 - 1 : 0], jhi = st[rend];
        for (int jb = jlo; jb < jhi; jb += 2 * RB) {
            // two chunks per trip, all their loads first
            int l[2];
            double2 wg[2];
            double dn[2];
            VT dd[2], dp[2];
            [[maybe_unused]] double fx[2][NX > 0 ? NX : 1];
            bool ok[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int j = jb + u * RB + rl;
                ok[u] = (j < jhi) && nok;
                l[u] = 0; wg[u] = make_double2(0.0, 0.0); dn[u] = 0.0; vzero(dd[u]); vzero(dp[u]);
                if (ok[u]) {
                    l[u] = R.lo[cb + j];
                    wg[u] = R.lwg[cb + j];
                    dn[u] = Dnew[j];
                    dd[u] = dDc[(size_t)j * N];
                    dp[u] = dpc[(size_t)j * N];
                    if constexpr (NX > 0) {
#pragma unroll
                        for (int o = 0; o < NX; o++) fx[u][o] = hx.fc[o * PG + cb + j];
                    }
                    if (j == 0)   // (then clo == 0) row 0 not clamped: its virtual rows follow row 0's interior lottery
                        for (int k = 0; k < KV; k++) dd[u] = vadd(dd[u], dDc[(size_t)(na + k) * N]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (ok[u]) {
                    const VT gt = vmul(wg[u].y, dp[u]);
                    const int tl = l[u] - r0, th = tl + 1;
                    if (tl >= 0 && tl < rows)
                        lds_add(&sh[tl >> lgRB][e * 64 + ((tl & (RB - 1)) << g.lgNC) + nl], vsub(vmul(1.0 - wg[u].x, dd[u]), gt));
                    if (th >= 0 && th < rows) {   // the source's FIRST-segment target: its aggregate term is taken here, once
                        lds_add(&sh[th >> lgRB][e * 64 + ((th & (RB - 1)) << g.lgNC) + nl], vadd(vmul(wg[u].x, dd[u]), gt));
                        pagg = vadd(pagg, vmul(dn[u], dp[u]));
                        if constexpr (NX > 0) {
#pragma unroll
                            for (int o = 0; o < NX; o++) paggx[o] = vsub(paggx[o], vmul(fx[u][o] * dn[u], dp[u]));
                        }
                    }
                }
            }
        }
        in_lds = true;
    } else if (!SS && !virt_block) {
        int s0[RG], s1[RG], s2[RG];
#pragma unroll
        for (int q = 0; q < RG; q++) {
            r[q] = (bidx * RG + q) * RB + rl;
            valid[q] = (r[q] < na) && nok;
            s0[q] = s1[q] = s2[q] = 0; cp[q] = 0.0;
            if (valid[q]) {
                const int4 sg = R.seg[cb + r[q]];
                s0[q] = sg.x; s1[q] = sg.y; s2[q] = sg.z;
                cp[q] = R.pol[cb + r[q]];
            }
            if constexpr (NX > 0) {
#pragma unroll
                for (int o = 0; o < NX; o++) cfx[q][o] = valid[q] ? hx.f[o * PG + cb + r[q]] : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < RG; q++) {
            VT s;
            vzero(s);
            if (valid[q]) {
                if (RG == 1 && g.lgNC >= 4) {
                // every unclamped source sits in exactly one FIRST segment [s0, s1): its aggregate term
                // dpol_j * D_t[j] is taken there, so dpol is not read a third time by its own row.
                // Small batches (one row group per wave): the first FS sources are loaded under lane predicates
                // with no wait between them — a counted loop serialises one memory round trip per source
                // (forward sweep 3.68 -> 3.40 ms at N=32; it costs 25 % at N=128 with two row groups per wave,
                // and 14 % at N=16 where a wave spans 8 rows).
                {
                    constexpr int FS = 2;
                    VT pd[FS], pp[FS];
                    double pn[FS];
                    double2 pw[FS];
                    [[maybe_unused]] double pfx[FS][NX > 0 ? NX : 1];
#pragma unroll
                    for (int k = 0; k < FS; k++) {
                        const int j = s0[q] + k;
                        vzero(pd[k]); vzero(pp[k]); pn[k] = 0.0; pw[k] = make_double2(0.0, 0.0);
                        if (j < s2[q]) {
                            pp[k] = dpc[(size_t)j * N];
                            pw[k] = R.lwg[cb + j];
                            pd[k] = dDc[(size_t)j * N];
                            if (j < s1[q]) {
                                pn[k] = Dnew[j];
                                if constexpr (NX > 0) {
#pragma unroll
                                    for (int o = 0; o < NX; o++) pfx[k][o] = hx.fc[o * PG + cb + j];
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < FS; k++) {
                        const int j = s0[q] + k;
                        if (j < s1[q]) {
                            s = vadd(s, vadd(vmul(pw[k].x, pd[k]), vmul(pw[k].y, pp[k])));
                            pagg = vadd(pagg, vmul(pn[k], pp[k]));
                            if constexpr (NX > 0) {
#pragma unroll
                                for (int o = 0; o < NX; o++) paggx[o] = vsub(paggx[o], vmul(pfx[k][o] * pn[k], pp[k]));
                            }
                        } else if (j < s2[q]) {
                            s = vadd(s, vsub(vmul(1.0 - pw[k].x, pd[k]), vmul(pw[k].y, pp[k])));
                        }
                    }
                    for (int j = s0[q] + FS; j < s2[q]; j++) {
                        const VT dpj = dpc[(size_t)j * N];
                        const double2 wg = R.lwg[cb + j];
                        if (j < s1[q]) {
                            s = vadd(s, vadd(vmul(wg.x, dDc[(size_t)j * N]), vmul(wg.y, dpj)));
                            pagg = vadd(pagg, vmul(Dnew[j], dpj));
                            if constexpr (NX > 0) {
#pragma unroll
                                for (int o = 0; o < NX; o++) paggx[o] = vsub(paggx[o], vmul(hx.fc[o * PG + cb + j] * Dnew[j], dpj));
                            }
                        } else {
                            s = vadd(s, vsub(vmul(1.0 - wg.x, dDc[(size_t)j * N]), vmul(wg.y, dpj)));
                        }
                    }
                }
                } else {
                    for (int j = s0[q]; j < s1[q]; j++) {
                        // every unclamped source sits in exactly one FIRST segment: its aggregate term
                        // dpol_j * D_t[j] is taken here, so dpol is not read a third time by its own row
                        const VT dpj = dpc[(size_t)j * N];
                        const double2 wg = R.lwg[cb + j];
                        s = vadd(s, vadd(vmul(wg.x, dDc[(size_t)j * N]), vmul(wg.y, dpj)));
                        pagg = vadd(pagg, vmul(Dnew[j], dpj));
                        if constexpr (NX > 0) {
#pragma unroll
                            for (int o = 0; o < NX; o++) paggx[o] = vsub(paggx[o], vmul(hx.fc[o * PG + cb + j] * Dnew[j], dpj));
                        }
                    }
                    for (int j = s1[q]; j < s2[q]; j++) {
                        const double2 wg = R.lwg[cb + j];
                        s = vadd(s, vsub(vmul(1.0 - wg.x, dDc[(size_t)j * N]), vmul(wg.y, dpc[(size_t)j * N])));
                    }
                }
                // row 0 not clamped: its virtual rows follow row 0's (interior) lottery
                if (clo == 0 && s2[q] > 0 && (s0[q] == 0 || s1[q] == 0)) {
                    const double w0 = (s0[q] == 0 && s1[q] > 0) ? R.lw[cb] : 1.0 - R.lw[cb];
                    VT v;
                    vzero(v);
                    for (int k = 0; k < KV; k++) v = vadd(v, dDc[(size_t)(na + k) * N]);
                    s = vadd(s, vmul(w0, v));
                }
            }
            acc[q] = s;
        }
    } else {
        const int p = bidx - nbr;
#pragma unroll
        for (int q = 0; q < RG; q++) { r[q] = na + p; valid[q] = (q == 0) && nok && (rl == 0); vzero(acc[q]); cp[q] = 0.0; }
        cp[0] = R.pol[cb];       // a virtual row carries row 0's policy and no policy tangent of its own
        if constexpr (NX > 0) {
#pragma unroll
            for (int q = 0; q < RG; q++)
#pragma unroll
                for (int o = 0; o < NX; o++) cfx[q][o] = q == 0 ? hx.f[o * PG + cb] : 0.0;
        }
        VT s;
        vzero(s);
        if (nok && clo > 0) {
            const int M = clo + KV;                         // clamped sources, then the virtual rows
            const int lo = (int)(((long long)M * p) / KV), hi = (int)(((long long)M * (p + 1)) / KV);
            for (int i = lo + rl; i < hi; i += RB) {
                s = vadd(s, dDc[(size_t)(i < clo ? i : na + (i - clo)) * N]);
                if (i < clo) pagg = vadd(pagg, vmul(Dnew[i], dpc[(size_t)i * N]));   // clamped sources: policy partial is 0 except on a knot tie
                if constexpr (NX > 0) {
                    if (i < clo) {
#pragma unroll
                        for (int o = 0; o < NX; o++) paggx[o] = vsub(paggx[o], vmul(hx.fc[o * PG + cb + i] * Dnew[i], dpc[(size_t)i * N]));
                    }
                }
            }
        }
        for (int off = 32; off >= g.NC; off >>= 1) { s = vadd(s, vshfl_xor(s, off)); pagg = vadd(pagg, vshfl_xor(pagg, off)); }
        if (rl != 0) vzero(pagg);
        if constexpr (NX > 0) {
#pragma unroll
            for (int o = 0; o < NX; o++) {
                for (int off = 32; off >= g.NC; off >>= 1) paggx[o] = vadd(paggx[o], vshfl_xor(paggx[o], off));
                if (rl != 0) vzero(paggx[o]);
            }
        }
        acc[0] = s;
    }
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += nthr) Pish[k] = c.Pi[k];
    if (!in_lds) {
#pragma unroll
        for (int q = 0; q < RG; q++) sh[q][e * 64 + lane] = acc[q];
    }
    lds_barrier();
    VT part, part2;       // the policy-weighted aggregate's partial and the wealth-grid-weighted one's (see dist_step_body)
    vzero(part); vzero(part2);
    [[maybe_unused]] VT partx[NX > 0 ? NX : 1];
    if constexpr (NX > 0) {
#pragma unroll
        for (int o = 0; o < NX; o++) vzero(partx[o]);
    }
#pragma unroll
    for (int q = 0; q < RG; q++) {
        if (valid[q]) {
            // dD_t[r,e] = sum_k dD_mid[r,k] * Pi[k,e]
            const VT dDn = mix_sum(vmul(Pish[c.n_e * e], sh[q][lane]), &sh[q][lane], 64, Pish + c.n_e * e, 1, 1, c.n_e);
            st_wt(&dDout[((size_t)e * nav + r[q]) * N + n], dDn);
            part = vadd(part, vmul(cp[q], dDn));
            part2 = vadd(part2, vmul(c.a[r[q] < na ? r[q] : 0], dDn));       // (a virtual row is a part of row 0)
            if constexpr (NX > 0) {
#pragma unroll
                for (int o = 0; o < NX; o++) partx[o] = vadd(partx[o], vmul(cfx[q][o], dDn));
            }
        }
    }
    part = vadd(part, pagg);
    // aggregate of this block: the columns' partials meet in `red` (its own LDS array: no barrier is needed before
    // writing it), ONE barrier, then wave 0 sums over columns and over the RB row lanes of each tangent
    red[e * 64 + lane] = part;
    red2[e * 64 + lane] = part2;
    lds_barrier();
    if constexpr (NX > 0) {
        // every wave has left the mixing (it wrote `red` behind it): the sh tiles are free, one per extra slot
#pragma unroll
        for (int o = 0; o < NX; o++) sh[o][e * 64 + lane] = vadd(partx[o], paggx[o]);
        lds_barrier();
        if (e == 0) {
#pragma unroll
            for (int o = 0; o < NX; o++) {
                VT s = sh[o][lane];
                for (int k = 1; k < c.n_e; k++) s = vadd(s, sh[o][k * 64 + lane]);
                for (int off = 32; off >= g.NC; off >>= 1) s = vadd(s, vshfl_xor(s, off));
                if (rl == 0 && nok) hx.parts[(((size_t)t * nbx_total + bidx) * NX + o) * N + n] = s;      // [t][block][NX][N]
            }
        }
    }
    if (e == 0) {
        VT s = red[lane], s2 = red2[lane];
        for (int k = 1; k < c.n_e; k++) { s = vadd(s, red[k * 64 + lane]); s2 = vadd(s2, red2[k * 64 + lane]); }
        for (int off = 32; off >= g.NC; off >>= 1) { s = vadd(s, vshfl_xor(s, off)); s2 = vadd(s2, vshfl_xor(s2, off)); }
        if (rl == 0 && nok) {       // aggpart: [t][block][2 N]: the first aggregate's N partials, then the second's
            aggpart[((size_t)t * nbx_total + bidx) * 2 * N + n] = s;
            aggpart[((size_t)t * nbx_total + bidx) * 2 * N + N + n] = s2;
        }
    }
}

// ---- pieces of the extra outputs (hank_hetx.h), the transposed sweeps (hank_adjoint.h) and the steady-state loops (hank_ssdiff.h) ----
constexpr int HX_NS = 5;    // per period and extra output: Y, Sa, Sz, S1, Sr

constexpr int ADJ_KS = 3;      // row slots a lane may own in a block's tile

// sum over the lanes of a wave that share the column pair nl (the rows rl of the wave), fixed order
template <typename VT>
__device__ __forceinline__ VT adj_rows_sum(VT v, int NC) {
    for (int off = 32; off >= NC; off >>= 1) v = vadd(v, vshfl_xor(v, off));
    return v;
}

template <typename VT, int NX>
struct AdjHx { const double *f, *fc; const VT *ybx; };      // f, f_c [jx][P][G] and their stride P G (k_hx_record); ybx [P][NX][MV]
template <typename VT>
struct AdjHx<VT, 0> {};

struct SsCtl { int stop, iters; double resid; };      // a loop's stop word, the steps it took, the last increment ratio

// ---- the device's error word -----------------------------------------------------------------------------------------------------
enum { ERR_KNOTS = 3, ERR_DOMAIN = 4, ERR_NONMONO = 6 };

__device__ inline void set_err(int *err, int code, int t, int e, int j) {
    if (atomicCAS(&err[0], 0, code) == 0) {
        err[1] = t;
        err[2] = e;
        err[3] = j;
    }
}

// ---- Young lottery of one column col = (t, e) of the record R (ForwardIteration.jl:37-78): the body of k_lottery and of the
// scenario batch's k_scen_lottery --------------------------------------------------------------------------------------------------
// one block per column; builds lo / lw / ig and the segment offsets that turn the 2-nnz-per-column
// scatter into a deterministic gather (the policy is monotone in wealth):
//   clo      = number of sources clamped at the FIRST grid point (policy <= grid[1], :54-58): a
//              prefix [0, clo) of the column, all mass to row 0 with weight one and no weight
//              tangent — the borrowing-constraint mass point, summed separately (it is long);
//   start[r] = max(clo, first source j with lo_j >= r): target row r receives w_j from the sources
//              in [start[r-1], start[r]) and 1-w_j from those in [start[r], start[r+1]).
// shlo: the block's dynamic LDS, 2 n_a + 2 ints; sh_clo: one more LDS word
// lq (k_lottery for the persistent Dual pass; everybody else: null): the same lo and w once more as ONE 16-byte record per source,
// {w, lo, flags}, flags bit 0: ig is zero (either clamp) — ig is otherwise 1 / (a[lo+1] - a[lo]), a table of n_a entries (k_iga_build)
// LEAN (k_xdual_front, in front of the one-pass persistent Dual pass; everybody else: false): only what that pass reads is written —
// lq and clo; lo, lw, ig, start and seg are left to k_lottery when a reader comes (ensure_lottery). shlo / shst are built as always.
template <bool LEAN = false>
__device__ __forceinline__ void lottery_body(const Consts &c, const Record &R, int col, int *err, int write_seg, int use_ib, int *shlo, int *sh_clo, int4 *lq = nullptr) {
    const int t = col / c.n_e, e = col % c.n_e;
    const size_t base = (size_t)col * c.n_a;  // == t*G + e*n_a
    const int n = c.n_a;
    if (threadIdx.x == 0) *sh_clo = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const double p = R.pol[base + j];
        int lo = -1, hi = n;  // grid[lo] < p <= grid[hi]  (searchsortedfirst, :52)
        if (use_ib) {
            // the policy is the interpolation's convex combination of grid[ib] and grid[ib + 1] (egm_Y): its lottery bracket is the
            // interpolation's unless it sits on a grid point or was moved by the borrowing constraint — a probe of that bracket and
            // of the one below replaces the 11 dependent loads of the bisection (which still decides whatever the probe does not)
            const int g0 = min(max(R.ib[base + j], 0), n - 2);
            const double a0 = c.a[g0], a1 = c.a[g0 + 1];
            if (a0 < p && p <= a1) { lo = g0; hi = g0 + 1; }
            else if (g0 > 0 && p <= a0 && c.a[g0 - 1] < p) { lo = g0 - 1; hi = g0; }
        }
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (c.a[mid] < p) lo = mid; else hi = mid;
        }
        int l;
        double w, ig;
        if (hi == 0) {            // m == 1: all mass on the first point (:54-58)
            l = 0; w = 0.0; ig = 0.0;
            atomicMax(sh_clo, j + 1);
        } else if (hi >= n) {     // m > n_a: all mass on the last point (:59-63)
            l = n - 2; w = 1.0; ig = 0.0;
        } else {                  // interior (:64-73)
            l = hi - 1;
            const double gap = c.a[hi] - c.a[l];
            w = (p - c.a[l]) / gap;
            ig = 1.0 / gap;
        }
        if constexpr (!LEAN) { R.lo[base + j] = l; R.lw[base + j] = w; R.ig[base + j] = ig; }
        if (lq) lq[base + j] = make_int4(__double2loint(w), __double2hiint(w), l, (hi == 0 || hi >= n) ? 1 : 0);
        shlo[j] = (hi == 0) ? -1 : l;   // clamped-low sources sort before every interior bracket
    }
    __syncthreads();
    const int clo = *sh_clo;
    if (threadIdx.x == 0) R.clo[col] = clo;
    int *st = R.start + (size_t)col * (n + 1);
    int *shst = shlo + n;          // segment offsets staged in LDS (second half of the dynamic LDS)
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int prev = j ? shlo[j - 1] : -1, cur = shlo[j];
        if (cur < prev) set_err(err, ERR_NONMONO, t, e, j);
        for (int r = (prev < 0 ? 0 : prev + 1); r <= cur; r++) shst[r] = j;   // j >= clo whenever cur >= 0
        if (j == n - 1)
            for (int r = (cur < 0 ? 0 : cur + 1); r <= n; r++) shst[r] = n;
    }
    __syncthreads();
    if constexpr (LEAN) return;
    for (int r = threadIdx.x; r <= n; r += blockDim.x) st[r] = shst[r];
    // per target row: its three segment bounds in one 16-byte record — what the launch family's gather reads (and k_xstat, and
    // k_fn_impulse); a third of this kernel's bytes, and the persistent Dual pass reads none of them: written there on demand
    // (write_seg = 0, then k_seg_build before the first reader)
    if (write_seg)
        for (int r = threadIdx.x; r < n; r += blockDim.x)
            R.seg[base + r] = make_int4(r > 0 ? shst[r - 1] : shst[r], shst[r], shst[r + 1], 0);
}

// lottery_body's bracket search for ONE record entry, for a caller that needs only "is this source clamped at the first grid point"
// (k_xdual_front: row 0 of the columns of the period before). The same statements as in lottery_body above, which keeps its own
// copy: calling this one there reordered an instruction of k_lottery, and every existing kernel stays what it was.
// -> hi with grid[hi - 1] < p <= grid[hi]; hi == 0: clamped at the first grid point, hi >= n_a: at the last
__device__ __forceinline__ int lottery_hi(const Consts &c, const Record &R, size_t idx, double p, int use_ib) {
    const int n = c.n_a;
    int lo = -1, hi = n;
    if (use_ib) {
        const int g0 = min(max(R.ib[idx], 0), n - 2);
        const double a0 = c.a[g0], a1 = c.a[g0 + 1];
        if (a0 < p && p <= a1) { lo = g0; hi = g0 + 1; }
        else if (g0 > 0 && p <= a0 && c.a[g0 - 1] < p) { lo = g0 - 1; hi = g0; }
    }
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (c.a[mid] < p) lo = mid; else hi = mid;
    }
    return hi;
}

// ---- the transposed steps: one body each for the sweep kernel (hank_adjoint.h) and the steady-state loop's (hank_ssdiff.h) --------
// A thread of the transposed kernels: block = one wave per productivity column e, lanes = (column lane nl fastest, row rl), RB rows
// per wave instruction; m: the lane's cotangent column (pair), mok: it exists.
struct AdjLane { int e, nl, rl, RB, m; bool mok; };
__device__ __forceinline__ AdjLane adj_lane(const AdjGeom &g) {
    AdjLane L;
    const int lane = threadIdx.x & 63;
    L.e = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    L.nl = lane & (g.NC - 1); L.rl = lane >> g.lgNC; L.RB = 64 >> g.lgNC;
    L.m = blockIdx.y * g.NC + L.nl;
    L.mok = L.m < g.MV;
    return L;
}

// One step of Sweep A at the record of period t. A block owns the TARGET rows [r0, r1) of the lottery, all columns: it loads the
// rows r0 .. r1 (one halo row) and row 0 once — load(row): what a tile row holds before the mix —, mixes them with Pi through the LDS
// tile (U), and then serves, per column, the SOURCES [start[r0], start[r1]) that the recorded lottery sends to its rows — the
// transpose of the source-stationary forward kernel — plus its share of the clamped prefix [0, clo) (sources that all read U[0]:
// shared out evenly over the row blocks). Every source row j meets exactly one block, once: src(j, u0, u1, clamped) with
// u0 = U[lo_j], u1 = U[lo_j + 1] of the lane's column (both U[0] for a clamped source). begin(): once per lane with a column, behind
// the mix — where a caller loads what only src reads, so that it does not occupy registers next to U.
// adj_sh, dynamic LDS: VT tile[n_e][R + 2][NC] (slot R + 1 = row 0), double Pish[n_e * n_e]
template <typename VT, typename Load, typename Begin, typename Src>
__device__ __forceinline__ void adj_dist_body(const Consts &c, const Record &R, const AdjGeom &g, const AdjLane &L, int t, double *adj_sh, Load load,
                                              Begin begin, Src src) {
    const int NS = g.R + 2, n = c.n_a, ne = c.n_e;
    VT *tile = reinterpret_cast<VT *>(adj_sh);
    double *Pish = adj_sh + (size_t)ne * NS * g.NC * (sizeof(VT) / sizeof(double));
    const int e = L.e, nl = L.nl, rl = L.rl, RB = L.RB;
    const int r0 = blockIdx.x * g.R, r1 = min(r0 + g.R, n);
    for (int k = threadIdx.x; k < ne * ne; k += 64 * ne) Pish[k] = c.Pi[k];
    // 1. the block's rows, own column
#pragma unroll
    for (int k = 0; k < ADJ_KS; k++) {
        const int slot = rl + k * RB;
        if (slot < NS) {
            const int row = slot == g.R + 1 ? 0 : r0 + slot;
            VT v;
            vzero(v);
            if (L.mok && row <= r1 && row < n) v = load(row);
            tile[((size_t)e * NS + slot) * g.NC + nl] = v;
        }
    }
    __syncthreads();
    // 2. U[row, e] = sum_e2 Pi[e, e2] tile[row, e2], back into the tile
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
    if (!L.mok) return;
    begin();
    const VT *Ue = tile + (size_t)e * NS * g.NC + nl;
    const size_t colb = (size_t)t * c.G + (size_t)e * n;      // (t, e) column of the record
    // 3. the sources of the block's target rows
    const int *st = R.start + ((size_t)t * ne + e) * (n + 1);
    const int j0 = min(max(st[r0], 0), n), j1 = min(max(st[r1], 0), n);
    for (int j = j0 + rl; j < j1; j += RB) {
        const int sl = min(max(R.lo[colb + j] - r0, 0), g.R - 1);
        src(j, Ue[(size_t)sl * g.NC], Ue[(size_t)(sl + 1) * g.NC], false);
    }
    // 4. the block's share of the clamped prefix
    const int clo = min(max(R.clo[(size_t)t * ne + e], 0), n);
    const int c0 = (int)(((long long)clo * blockIdx.x) / gridDim.x), c1 = (int)(((long long)clo * (blockIdx.x + 1)) / gridDim.x);
    const VT U0 = Ue[(size_t)(g.R + 1) * g.NC];
    for (int j = c0 + rl; j < c1; j += RB) src(j, U0, U0, true);
}

// One step of Sweep B at the record of period t. A block owns the KNOT rows [i0, i0 + R), all columns. Knot i of column e gathers
// gbar = pbar - v mu (sub; pbar alone without it) over the two contiguous row segments that bracket on it ([sb[i], sb[i+1]) with
// weight A, [sb[i-1], sb[i]) with weight B: k_adj_seg); the n_e x n_e mixing of kc sbar goes through the LDS tile; mix: every mixed
// row mn = sum_e Pi[e, e2] kc[e, i] sbar[e, i] goes to row(i, mn), which stores the new state and returns the state the inputs'
// sums weigh with (u + v a, v z_e, v) of period tm. The household inputs' cotangents leave as per-block partials, every sum in a
// fixed order: partS[block][3][MV] = sum sbar (s, z_e, 1), partM[block][3][MV] (written when mix) the sums of what row returned.
// adj_sh, dynamic LDS: VT tile[n_e][R][NC], double Pish[n_e * n_e], VT red[n_e][6][NC]
template <typename VT, typename Row>
__device__ __forceinline__ void adj_egm_body(const Consts &c, const Record &R, const AdjGeom &g, const AdjLane &L, int t, int tm, bool sub, bool mix,
                                             const int *__restrict__ sb, const VT *__restrict__ muIn, const VT *__restrict__ pbar, double *adj_sh,
                                             VT *__restrict__ partS, VT *__restrict__ partM, Row row) {
    const int n = c.n_a, ne = c.n_e, NS = g.R;
    const int e = L.e, nl = L.nl, rl = L.rl, RB = L.RB, m = L.m;
    const bool mok = L.mok;
    VT *tile = reinterpret_cast<VT *>(adj_sh);
    double *Pish = adj_sh + (size_t)ne * NS * g.NC * (sizeof(VT) / sizeof(double));
    VT *red = reinterpret_cast<VT *>(Pish + ((ne * ne + 1) & ~1));
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
                if (sub) {
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
    // 2. the mixed rows of the wave's column e2 = e
    if (mix) {
        const size_t colm = (size_t)tm * c.G + (size_t)e * n;
#pragma unroll
        for (int k = 0; k < ADJ_KS; k++) {
            const int slot = rl + k * RB, i = i0 + slot;
            if (mok && slot < g.R && i < n) {
                VT mn;
                vzero(mn);
                for (int e1 = 0; e1 < ne; e1++) mn = vadd(mn, vmul(Pish[e1 + ne * e], tile[((size_t)e1 * NS + slot) * g.NC + nl]));
                const VT ms = row(i, mn);
                const double u1 = R.u[colm + i], v1 = R.v[colm + i];
                sum[3] = vadd(sum[3], vmul(u1 + v1 * c.a[i], ms));
                sum[4] = vadd(sum[4], vmul(v1 * ze, ms));
                sum[5] = vadd(sum[5], vmul(v1, ms));
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
            if (q < 3) partS[((size_t)blockIdx.x * 3 + q) * MV + m] = v;
            else if (mix) partM[((size_t)blockIdx.x * 3 + (q - 3)) * MV + m] = v;
        }
    }
}

// ---- the outputs' arithmetic: consumption's affine identity and the extra outputs' direct terms, forward and transposed -----------
//     C_t  = (1+r_t) AD_t + w_t ZD_t + tr_t MD_t - KD_t,      AD_t = sum a D_t, ZD_t = sum z_e D_t, MD_t = sum D_t
//     dC_t = dr_t AD_t + dw_t ZD_t + dtr_t MD_t + (1+r_t) dAD_t - dKD_t
//     dY^o_t = T_o,t + dr_t (Sa + Sr) + dw_t Sz + dtr_t S1      (S: k_hx_record's Y, Sa, Sz, S1, Sr)
__device__ __forceinline__ double out_cons(double r, double w, double tr, double AD, double ZD, double MD, double KD) {
    return ((1.0 + r) * AD + w * ZD + tr * MD) - KD;
}
__device__ __forceinline__ double out_dcons(double r, double dr, double dw, double dtr, double AD, double ZD, double MD, double dAD, double dKD) {
    return (dr * AD + dw * ZD + dtr * MD + (1.0 + r) * dAD) - dKD;
}
__device__ __forceinline__ double out_dhx(double T, double dr, double dw, double dtr, const double *S) {
    return T + dr * (S[1] + S[4]) + dw * S[2] + dtr * S[3];
}
// transposed: input q's cotangent from Sweep B's sums and consumption's direct term (d: sum a D, sum z_e D or sum D), and an extra
// output's direct terms added to o = (xbar_r, xbar_w, xbar_tr)
__device__ __forceinline__ double xbar_cons(double mu, double rho, double s, double y1, double d) { return (mu - rho * s) + y1 * d; }
__device__ __forceinline__ void xbar_hx(double y, const double *S, int n_hh, double *o) {
    o[0] += y * (S[1] + S[4]);
    o[1] += y * S[2];
    if (n_hh > 2) o[2] += y * S[3];
}

}  // namespace hank
