// hank_kernels.h — CDNA4 (gfx950) kernels of the household block. fp64 throughout, no MFMA:
// the path is interpolation / 2-nnz SpMV / reductions (HBM-bound), the only contraction is the
// n_e x n_e productivity mixing.
//
// Data layout in HBM (per context, P = T-1 periods, G = n_a*n_e, wealth fastest):
//   primal record  [P][n_e][n_a] : s (EGM knots), kc (d s/d E), ib/A/B (bracket + tangent weights),
//                                  u, v (marginal-value coefficients), pol (savings policy),
//                                  lo/lw/ig (Young lottery), start (segment offsets), Dseq[P+1]
//   tangent state  [n_e][n_a][N] : tangent index FASTEST (the AoS layout of Dual{T,V,N}): one grid
//                                  point's N partials are one contiguous row, so the bracket gather
//                                  and the lottery segment sums move whole coalesced rows.
//   dpol           [P][n_e][n_a][N] : the policy-partials sequence BackwardIteration materialises
//                                  (BackwardIteration.jl:88, :110-112); written once by the
//                                  backward sweep, read once by the forward sweep = the
//                                  algorithmic HBM traffic of a JVP batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hank_device.h"      // Consts, Record, the lane helpers, tan_back_body, tan_fwd_body

namespace hank {

constexpr int RBP = 32;        // rows (wealth points) per block in the primal kernels

// (ERR_KNOTS, ERR_DOMAIN, ERR_NONMONO, set_err: hank_device.h)

// CRRA (here and in pow_crra, diet_kc, diet_v, egm_Y, egm_Y_finish): 0 = gamma and the record diet are what the context holds,
// decided where they are used; 1 = an instance compiled for gamma = 2 with the record diet on (hank_xspec.h chooses it): the
// caller passes the exponents as the literals -0.5 and -2, and each of these functions IS the arm the generic one takes there —
// the same expressions in the same order, so the same bits.
template <int CRRA = 0>
__device__ inline bool pow_domain_error(double v, double y) {
    if constexpr (CRRA == 1) return (v < 0.0) && (y == -0.5);       // (-2 is an integer: no error; -0.5 is none)
    else return (v < 0.0) && (y != floor(y));
}

// Reciprocal and reciprocal square root of the primal EGM step: the hardware estimate (v_rcp_f64 / v_rsq_f64) and two Newton
// steps, without the div_scale / div_fmas / div_fixup wrapper of an IEEE division (~18 instructions) or the scaling of an IEEE
// square root. The operands — a marginal value, a consumption level, the distance of two sorted knots — are positive, finite and
// far from the denormal range wherever the step does not report ERR_KNOTS / ERR_DOMAIN anyway (zero or negative arguments give
// inf / NaN as the IEEE forms do); the results are within an ulp or two of the correctly rounded ones (oracle tolerance: 1e-10).
// A row of the Dual pass's backward half does four divisions and two roots: ~110 of its ~500 instructions per wave and period,
// on the critical path of a SIMD's three waves (the staircase at the tile barrier). EVERY primal
// kernel takes its quotients and roots from here (egm_X / egm_Y / diet_v are shared), so k_egm_step, k_xprimal_back, k_xdual_back
// and k_xvfi still agree with each other bit for bit.
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = __builtin_fma(y * 0.5, __builtin_fma(-(x * y), y, 1.0), y);
    y = __builtin_fma(y * 0.5, __builtin_fma(-(x * y), y, 1.0), y);
    return y;
}
__device__ __forceinline__ double fast_sqrt(double x) {     // x rsqrt(x), one correction of the product
    const double y = fast_rsqrt(x), g = x * y;
    return __builtin_fma(y * 0.5, __builtin_fma(-g, g, x), g);
}

// x^y with the exponents CRRA utility produces most often taken through a reciprocal / reciprocal square root
// (gamma = 2: y = -1/2 and y = -2; gamma = 1: y = -1) — a generic fp64 pow is a few
// hundred VALU instructions on the primal sweep's critical path. Same value as pow() to an ulp or two.
template <int CRRA = 0>
__device__ inline double pow_crra(double x, double y) {
    if constexpr (CRRA == 1) return y == -0.5 ? fast_rsqrt(x) : fast_rcp(x * x);
    if (y == -0.5) return fast_rsqrt(x);
    if (y == -2.0) return fast_rcp(x * x);
    if (y == -1.0) return fast_rcp(x);
    return pow(x, y);
}

// buffer accesses: ONE scalar descriptor for the whole record, a 32-bit lane offset (the row pair: shared by every array), a scalar
// offset (array, period and column)
typedef unsigned int wv2u __attribute__((ext_vector_type(2)));
typedef unsigned int wv4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wide_rsrc(const void *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ wv2u wide_ld2i(__amdgpu_buffer_rsrc_t rs, int vo, int so) { return __builtin_amdgcn_raw_buffer_load_b64(rs, vo, so, 0); }
template <int AUX>
__device__ __forceinline__ void wide_ld2d(__amdgpu_buffer_rsrc_t rs, int vo, int so, double &a, double &b) {    // two adjacent doubles: one 16-byte load
    const wv4u q = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, AUX);
    a = __hiloint2double((int)q.y, (int)q.x); b = __hiloint2double((int)q.w, (int)q.z);
}
__device__ __forceinline__ wv4u wide_ld128(__amdgpu_buffer_rsrc_t rs, int vo, int so) { return __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0); }
__device__ __forceinline__ void wide_st2d_nt(double a, double b, __amdgpu_buffer_rsrc_t rs, int vo, int so) {
    wv4u q;
    q.x = (unsigned)__double2loint(a); q.y = (unsigned)__double2hiint(a); q.z = (unsigned)__double2loint(b); q.w = (unsigned)__double2hiint(b);
    __builtin_amdgcn_raw_buffer_store_b128(q, rs, vo, so, 2);
}
__device__ __forceinline__ void wide_st64_nt(double v, __amdgpu_buffer_rsrc_t rs, int vo, int so) {
    wv2u q;
    q.x = (unsigned)__double2loint(v); q.y = (unsigned)__double2hiint(v);
    __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, so, 2);
}

// the same with the cache mode as a parameter, for the persistent sweeps' descriptor path (hank_xsweep.h). AUX: 0 plain, 2 nontemporal,
// 16 sc1 (bypasses the CU's L1: served by the XCD's L2). The descriptor's size is the allocation's, but that is NO safety net: the
// hardware's range check sees the lane offset and the immediate only, and the sweeps put array, period and column into the scalar
// offset, which it does not see. A wrong scalar offset reads and writes wherever it points; what keeps the offsets right is
// x_addr_fits (hank_xaddr.h) and the tests against the launches.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
template <int AUX>
__device__ __forceinline__ double buf_ld64(__amdgpu_buffer_rsrc_t rs, int vo, int so) {
    const wv2u q = __builtin_amdgcn_raw_buffer_load_b64(rs, vo, so, AUX);
    return __hiloint2double((int)q.y, (int)q.x);
}
template <int AUX>
__device__ __forceinline__ int buf_ld32(__amdgpu_buffer_rsrc_t rs, int vo, int so) { return (int)__builtin_amdgcn_raw_buffer_load_b32(rs, vo, so, AUX); }
template <int AUX>
__device__ __forceinline__ void buf_st64(double v, __amdgpu_buffer_rsrc_t rs, int vo, int so) {
    wv2u q;
    q.x = (unsigned)__double2loint(v); q.y = (unsigned)__double2hiint(v);
    __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, so, AUX);
}
template <int AUX>
__device__ __forceinline__ void buf_st32(int v, __amdgpu_buffer_rsrc_t rs, int vo, int so) { __builtin_amdgcn_raw_buffer_store_b32((unsigned)v, rs, vo, so, AUX); }
template <int AUX>
__device__ __forceinline__ void buf_st2d(double a, double b, __amdgpu_buffer_rsrc_t rs, int vo, int so) {
    wv4u q;
    q.x = (unsigned)__double2loint(a); q.y = (unsigned)__double2hiint(a); q.z = (unsigned)__double2loint(b); q.w = (unsigned)__double2hiint(b);
    __builtin_amdgcn_raw_buffer_store_b128(q, rs, vo, so, AUX);
}

// RECORD DIET. Two of the seven coefficients a backward tangent step reads per point are functions of their neighbours in the
// record: s = rho ((cm - (w z_e + tr)) + a) gives back cm, and kc = rho beta (-1/gamma) cm^(1 + gamma); u = cg^(-gamma) gives back
// cg, and v = (1 + r)(-gamma) u / cg. With gamma = 1 or 2 the powers are products and one square root: 16 of the 52 bytes per
// point and period are not read (by each of the 8 groups of a persistent sweep). Other gammas keep reading kc and v (a pow per
// point, period and group costs more than the 16 bytes). Both implementations use these two functions, so their policy partials
// stay bit-identical: the PRIMAL sweeps record kc and v as these two functions give them, the launch-path tangent kernels (whose
// lane-sparse coefficient loads are off their critical path: rebuilding cost them 1-3 %) read the record, the persistent
// tangent sweeps (8 groups re-read the record) rebuild: the same bits either way. Against the textbook expressions the values
// move by rounding (cm is rebuilt through a cancellation: 1e-13).
template <int CRRA = 0>
__device__ __forceinline__ double diet_kc(const Consts &c, double s, double rho, double opr, double wz_tr, double xa) {
    const double cm = (s * opr + wz_tr) - xa;
    const double k = rho * (c.beta * (CRRA == 1 ? -0.5 : -1.0 / c.gamma));
    return (CRRA == 1 || c.gamma == 2.0) ? k * (cm * cm * cm) : k * (cm * cm);
}
template <int CRRA = 0>
__device__ __forceinline__ double diet_v(const Consts &c, double u, double opr) {
    return (CRRA == 1 || c.gamma == 2.0) ? opr * (-2.0 * (u * fast_sqrt(u))) : opr * (-(u * u));
}

// ---- EGM step, split in the two halves that fuse across the period boundary ------------------
// X half (KrusellSmith.jl:59-62): from V_{t+1} (all e2 of this row, in LDS) to the endogenous
// knot s_t[a,e] and kc = d s / d E  (= rho * d c / d E).
// The half at ONE point, from the mixed expectation E = sum_k Pi[e, k] V_{t+1}[a, k]: every primal kernel — the launches through
// egm_X below, the persistent sweeps (k_xprimal_back, k_xvfi, k_xdual_back: hank_xsweep.h) behind their own mixing — takes s and kc
// from here, so they agree bit for bit. rho = 1/(1+r), opr = 1 + r, wz_tr = w z_e + tr, xa = the grid point a.
struct XPoint { double s1, kc; };
template <int CRRA = 0>
__device__ __forceinline__ XPoint egm_X_point(const Consts &c, double E, const double *x4, double ze, double xa, int *err, int t, int e, int a) {
    const double bE = E * c.beta;
    const double ex = CRRA == 1 ? -0.5 : -1.0 / c.gamma;
    if (pow_domain_error<CRRA>(bE, ex)) set_err(err, ERR_DOMAIN, t, e, a);
    const double cm = pow_crra<CRRA>(bE, ex);
    const double rho = x4[3];
    const double s1 = rho * ((cm - (x4[1] * ze + x4[2])) + xa);
    // d cmat/dE = beta*ex*(bE)^(ex-1)  (Dual^Real, ForwardDiff dual.jl:563-572); under the record diet the recorded value IS the
    // one the persistent tangent sweeps rebuild from s (diet_kc): whoever reads it and whoever rebuilds it hold the same bits
    const double kc = (CRRA == 1 || c.diet) ? diet_kc<CRRA>(c, s1, rho, 1.0 + x4[0], x4[1] * ze + x4[2], xa) : rho * (c.beta * ex * (cm / bE));
    return {s1, kc};
}
__device__ inline void egm_X(const Consts &c, const double *Vsh, const double *Pish, int row, int a,
                             int e, double r, double w, double tr, double *s_out, double *kc_out, int *err,
                             int t) {
    const double E = mix_sum(Vsh[row] * Pish[e], Vsh + row, RBP, Pish + e, c.n_e, 1, c.n_e);
    const double x4[4] = {r, w, tr, 1.0 / (1.0 + r)};
    const XPoint p = egm_X_point(c, E, x4, c.z[e], c.a[a], err, t, e, a);
    *s_out = p.s1; *kc_out = p.kc;
}

// Y half (KrusellSmith.jl:66-80): interpolate the policy on the exogenous grid point a from the
// knots of column e (sc = s_t[:,e]), apply the borrowing constraint, form the marginal value.
// Interpolations.jl Gridded(Linear()) + Flat(): bracket = last knot <= x, flat outside.
struct YOut {
    double g, A, B, u, v, V;
    int ib;
};
// `guess` (>= 0): the bracket of the same point one period later — brackets move by a few knots per
// period, so a probe there plus a short gallop replaces the 11 dependent loads of a cold bisection.
// `sc` is anything indexable that returns the knot s_t[i, e] (a plain pointer; the XCD-local sweep passes a
// loader that reads the L2-resident state with L1-bypassing loads) — the arithmetic is the same for both.
//
// The half is SPLIT AT THE BRACKET. In front of "the bracket is i with knots si, sj" there are two ways to get there:
//   * the search (probe, gallops, bisection) below, which every loader can serve;
//   * a loader that already holds the knots of the usual cases in registers names the bracket itself, in straight-line code
//     (YFrontOf<KNOTS>::value, `sc.front()`: XKnots, hank_xsweep.h), and leaves to the search only the lanes it could not
//     resolve — behind a wave-uniform branch, so a wave whose brackets moved by a knot at most never enters it.
// Behind the bracket there is ONE tail for both: the interpolation or a flat outcome, then egm_Y_finish. A bracket is unique,
// so the way it was found does not change a bit of the result. With a plain pointer the `FRONT` conditions are compile-time
// constants and the function is the search followed by the tail, as it always was.
enum { Y_INSIDE = 0, Y_BELOW = 1, Y_ABOVE = 2 };      // where the point lies among the knots (flat extrapolation outside)
struct YFront {
    int where, i;         // Y_*; the bracket of a point inside the knots (meaningless in a `slow` lane)
    double si, sj;        // the bracket's knots
    bool slow;            // an interior point whose bracket is none of the candidates: the search decides
    bool bad;             // Interpolations' check_gridded fails at this row
};
template <typename KNOTS> struct YFrontOf { static constexpr bool value = false; };
// a loader that brings the column's productivity z_e in a register (`sc.column_z()`), whether or not it has a front
template <typename KNOTS> struct YColumnZOf { static constexpr bool value = false; };
constexpr int Y_WAIT_VMCNT0 = 0x0F70;     // s_waitcnt immediate on gfx9: vmcnt(0), expcnt and lgkmcnt left at their maxima (7, 15)

// the tail's second piece: the borrowing constraint on the interpolated (or flat) policy, consumption, marginal value.
// ZREG: the column's productivity z_e comes in a register (`ze`: YColumnZOf<KNOTS>, see XKnots) instead of from c.z[e]
template <bool ZREG, int CRRA = 0>
__device__ __forceinline__ YOut egm_Y_finish(const Consts &c, int a, int e, double r, double w, double tr, int *err, int t,
                                             double x, double g, double A, double B, int i, double ze) {
    YOut o;
    // max(g, borrow_cons), DiffRules rule: partial passes unless (bc > g) | signbit(bc) < signbit(g)
    const double bc = c.bc;
    if ((bc > g) || ((int)signbit(bc) < (int)signbit(g))) {
        A = 0.0;
        B = 0.0;
    }
    g = (g > bc) ? g : ((bc > g) ? bc : (signbit(g) ? bc : g));
    const double opr = 1.0 + r;
    const double cg = (opr * x + (w * (ZREG ? ze : c.z[e]) + tr)) - g;
    const double mg = CRRA == 1 ? -2.0 : -c.gamma;
    if (pow_domain_error<CRRA>(cg, mg)) set_err(err, ERR_DOMAIN, t, e, a);
    const double u = pow_crra<CRRA>(cg, mg);
    o.g = g;
    o.A = A;
    o.B = B;
    o.ib = i;
    o.u = u;
    o.v = (CRRA == 1 || c.diet) ? diet_v<CRRA>(c, u, opr) : opr * ((-c.gamma) * (u / cg));
    o.V = opr * u;
    return o;
}

template <int CRRA = 0, typename KNOTS>
__device__ inline YOut egm_Y(const Consts &c, const KNOTS sc, int a, int e, double r, double w, double tr,
                             int *err, int t, int guess) {
    constexpr bool FRONT = YFrontOf<KNOTS>::value;
    const int n = c.n_a;
    const double x = c.a[a];
    double s0, sN, si, sj;
    int where, i;
    bool slow, slow_wave;                   // (this lane / some lane of this wave) goes through the search
    if constexpr (FRONT) {
        const YFront f = sc.front(x, guess);
        where = f.where; i = f.i; si = f.si; sj = f.sj;
        slow = f.slow;
        slow_wave = __any(f.slow || f.bad) != 0;
        if (slow_wave) {
            if (f.bad) set_err(err, ERR_KNOTS, t, e, a);
        }
    } else {
        const double sa = sc[a];
        // Interpolations' check_gridded: knots must be sorted and unique (values)
        if (a > 0 ? !(sa > sc[a - 1]) : !(sa == sa)) set_err(err, ERR_KNOTS, t, e, a);
        s0 = sc[0]; sN = sc[n - 1];
    }
    double g, A = 0.0, B = 0.0;
    if (FRONT ? where == Y_BELOW : x < s0) {
        g = c.a[0];
        i = 0;
    } else if (FRONT ? where == Y_ABOVE : x > sN) {
        g = c.a[n - 1];
        i = n - 2;
    } else {
        if (FRONT ? slow_wave : true) {
            if (FRONT ? slow : true) {
                int lo = -1, hi = n;  // sc[lo] <= x < sc[hi]
                bool have = false;    // vlo/vhi hold sc[lo], sc[hi] (bracket found by the first probe)
                double vlo = 0.0, vhi = 0.0;
                if (guess >= 0) {
                    // probe the guessed bracket AND its two neighbours in one round trip (four independent loads): a bracket
                    // that moved by one knot — the common miss — needs no second trip
                    const int p = guess < n - 1 ? guess : n - 2;
                    const int pm = p > 0 ? p - 1 : 0, pp = p + 2 < n ? p + 2 : n - 1;
                    const double sm = sc[pm], sp = sc[p], sp1 = sc[p + 1], sp2 = sc[pp];
                    if (sp <= x && x < sp1) {
                        lo = p; hi = p + 1; have = true; vlo = sp; vhi = sp1;   // the usual case
                    } else if (p + 2 < n && sp1 <= x && x < sp2) {
                        lo = p + 1; hi = p + 2; have = true; vlo = sp1; vhi = sp2;
                    } else if (p > 0 && sm <= x && x < sp) {
                        lo = p - 1; hi = p; have = true; vlo = sm; vhi = sp;
                    } else if (sp1 <= x) {          // gallop up
                        lo = p + 1;
                        for (int step = 1;; step <<= 1) {
                            const int q = lo + step;
                            if (q >= n) break;
                            if (sc[q] <= x) lo = q; else { hi = q; break; }
                        }
                    } else {                         // gallop down
                        hi = p;
                        for (int step = 1;; step <<= 1) {
                            const int q = hi - step;
                            if (q < 0) break;
                            if (sc[q] <= x) { lo = q; break; } else hi = q;
                        }
                    }
                }
                while (hi - lo > 1) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (sc[mid] <= x) lo = mid; else hi = mid;
                }
                i = lo < 0 ? 0 : (lo > n - 2 ? n - 2 : lo);
                si = have ? vlo : sc[i];
                sj = have ? vhi : sc[i + 1];
                // Without this explicit wait the compiler puts an s_waitcnt vmcnt(0) at the join BEHIND the search, where the waves
                // that skipped it arrive too and then wait for their partials' rows, which nothing in the tail needs (checked in the ISA
                // of k_xdual_back: with it, the vmcnt(0) sits inside this arm and the skipping waves keep their counted waits).
                if constexpr (FRONT) __builtin_amdgcn_s_waitcnt(Y_WAIT_VMCNT0);
            }
        }
        // ---- the tail: the bracket is i with knots si <= x < sj
        const double h = sj - si, rh = fast_rcp(h);      // (one reciprocal serves both quotients)
        const double f = (x - si) * rh;
        const double ai = c.a[i], aj = c.a[i + 1];
        g = (1.0 - f) * ai + f * aj;
        const double sl = (aj - ai) * rh;
        A = -sl * (1.0 - f);
        B = -sl * f;
    }
    if constexpr (YColumnZOf<KNOTS>::value) return egm_Y_finish<true, CRRA>(c, a, e, r, w, tr, err, t, x, g, A, B, i, sc.column_z());
    else return egm_Y_finish<false, CRRA>(c, a, e, r, w, tr, err, t, x, g, A, B, i, 0.0);
}

// block = RBP rows x n_e columns; thread (row, e) with row fastest. dynamic LDS:
// Vsh[n_e*RBP] + Pish[n_e*n_e]
// `stop` (may be null): the device-resident value-function iteration freezes its state once it has converged
__global__ void k_egm_X(Consts c, const double *Vin, const double *xt, double *s_out,
                        double *kc_out, int *err, int t, const int *stop) {
    extern __shared__ double sh[];
    if (stop && *stop) return;
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = blockIdx.x * RBP + row;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += blockDim.x) Pish[k] = c.Pi[k];
    if (a < c.n_a) Vsh[e * RBP + row] = Vin[e * c.n_a + a];
    __syncthreads();
    if (a < c.n_a) egm_X(c, Vsh, Pish, row, a, e, xt[0], xt[1], c.n_hh > 2 ? xt[2] : 0.0, &s_out[e * c.n_a + a], &kc_out[e * c.n_a + a], err, t);
}

// Y only (granular step): record slot pointers are for ONE period
__global__ void k_egm_Y(Consts c, const double *s, double r, double w, double tr, double *pol, int *ib,
                        double *A, double *B, double *u, double *v, double *Vout, int *err, int t, const int *stop) {
    if (stop && *stop) return;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = blockIdx.x * RBP + row;
    if (a >= c.n_a) return;
    const YOut o = egm_Y(c, s + e * c.n_a, a, e, r, w, tr, err, t, -1);
    const int off = e * c.n_a + a;
    pol[off] = o.g; ib[off] = o.ib; A[off] = o.A; B[off] = o.B; u[off] = o.u; v[off] = o.v;
    Vout[off] = o.V;
}

// fused sweep step: Y of period t, then X of period t-1 (value never leaves the CU).
// Body shared by k_egm_step and the dual-sweep kernel k_fused_back; runs on the first RBP*n_e
// threads of block `bid`; sh = Vsh[n_e*RBP] + Pish[n_e*n_e].
__device__ inline void egm_step_body(const Consts &c, const Record &R, const double *xhh, int t, int *err, int bid, double *sh) {
    double *Vsh = sh, *Pish = sh + c.n_e * RBP;
    const int nthr = RBP * c.n_e;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int a = bid * RBP + row;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += nthr) Pish[k] = c.Pi[k];
    const size_t base = (size_t)t * c.G;
    if (a < c.n_a) {
        const double r = xhh[c.n_hh * t], w = xhh[c.n_hh * t + 1], tr = hh_tr(c, xhh, t);
        const int guess = (t + 1 < c.P) ? R.ib[base + c.G + (size_t)e * c.n_a + a] : -1;
        const YOut o = egm_Y(c, R.s + base + (size_t)e * c.n_a, a, e, r, w, tr, err, t, guess);
        const size_t off = base + (size_t)e * c.n_a + a;
        R.pol[off] = o.g; R.ib[off] = o.ib; R.A[off] = o.A;
        R.B[off] = o.B; R.u[off] = o.u; R.v[off] = o.v;
        Vsh[e * RBP + row] = o.V;
    }
    lds_barrier();
    if (t > 0 && a < c.n_a) {
        const double r1 = xhh[c.n_hh * (t - 1)], w1 = xhh[c.n_hh * (t - 1) + 1], tr1 = hh_tr(c, xhh, t - 1);
        const size_t off1 = base - c.G + (size_t)e * c.n_a + a;
        egm_X(c, Vsh, Pish, row, a, e, r1, w1, tr1, &R.s[off1], &R.kc[off1], err, t - 1);
    }
}
__global__ void k_egm_step(Consts c, Record R, const double *xhh, int t, int *err) {
    extern __shared__ double sh[];
    egm_step_body(c, R, xhh, t, err, blockIdx.x, sh);
}

// ---- Young lottery for every (period, column) at once: lottery_body (hank_device.h), one block per column -------------------
// dynamic LDS: 2 n_a + 2 ints
__global__ void k_lottery(Consts c, Record R, int ncols, int *err, int write_seg, int use_ib) {
    extern __shared__ int shlo[];
    __shared__ int sh_clo;
    const int col = blockIdx.x;
    if (col >= ncols) return;
    lottery_body(c, R, col, err, write_seg, use_ib, shlo, &sh_clo);
}
#if HANK_XFWD_LQ
// k_lottery in front of a persistent Dual pass: with the packed per-source records lq [ncols][n_a] its forward sweep reads (see
// lottery_body). A kernel of its own: k_lottery's arguments, and with them its code, stay what every other caller has
__global__ void k_lottery_lq(Consts c, Record R, int ncols, int *err, int write_seg, int use_ib, int4 *lq) {
    extern __shared__ int shlo[];
    __shared__ int sh_clo;
    const int col = blockIdx.x;
    if (col >= ncols) return;
    lottery_body(c, R, col, err, write_seg, use_ib, shlo, &sh_clo, lq);
}
// the inverse gaps of the wealth grid, once per context: iga[l] = 1 / (a[l+1] - a[l]) — the expression lottery_body's ig is made
// with, so that the table's entry IS the record's ig of an interior source with bracket l — and 0 behind the last bracket
__global__ void k_iga_build(Consts c, double *iga) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < c.n_a) iga[l] = l + 1 < c.n_a ? 1.0 / (c.a[l + 1] - c.a[l]) : 0.0;
}
#endif
// the same records from the segment offsets k_lottery left (one block per column)
__global__ void k_seg_build(Consts c, Record R, int ncols) {
    const int col = blockIdx.x, n = c.n_a;
    if (col >= ncols) return;
    const int *st = R.start + (size_t)col * (n + 1);
    const size_t base = (size_t)col * n;
    for (int r = threadIdx.x; r < n; r += blockDim.x)
        R.seg[base + r] = make_int4(r > 0 ? st[r - 1] : st[r], st[r], st[r + 1], 0);
}

// ---- distribution push-forward, one period (ForwardIteration.jl:95-99, :297-308) -------------
// block = RBP rows x n_e, thread (row, e) with row fastest (a 32-lane half-wave per column);
// dynamic LDS: Dsh[n_e*RBP] + Pish[n_e*n_e] + red[16]
// body shared by k_dist_step and k_fused_fwd; first RBP*n_e threads of block `bid` of `nblocks`
// Din / Dout (may be null): explicit D_{t-1} and D_t buffers instead of the record's Dseq rows — the stationary-distribution
// iteration of the steady state reuses this step with one period's lottery and two ping-pong buffers
__device__ inline void dist_step_body(const Consts &c, const Record &R, int t, double *aggpart, int bid, int nblocks, double *sh,
                                      const double *Din = nullptr, double *Dout = nullptr) {
    double *Dsh = sh, *Pish = sh + c.n_e * RBP, *red = Pish + c.n_e * c.n_e;
    const int nthr = RBP * c.n_e;
    const int row = threadIdx.x % RBP, e = threadIdx.x / RBP;
    const int r = bid * RBP + row;
    const int n = c.n_a;
    for (int k = threadIdx.x; k < c.n_e * c.n_e; k += nthr) Pish[k] = c.Pi[k];
    const double *Dprev = Din ? Din : R.Dseq + (size_t)t * c.G;
    const size_t base = (size_t)t * c.G;
    const double *lw = R.lw + base + (size_t)e * n, *Dp = Dprev + (size_t)e * n;
    double acc = 0.0;
    if (r < n) {
        if (!Din) R.lwg[base + (size_t)e * n + r] = make_double2(lw[r], R.ig[base + (size_t)e * n + r] * Dp[r]);
        const int *st = R.start + ((size_t)t * c.n_e + e) * (n + 1);
        const int st1 = st[r], st2 = st[r + 1], st0 = r > 0 ? st[r - 1] : st1;
        for (int j = st0; j < st1; j++) acc += lw[j] * Dp[j];
        for (int j = st1; j < st2; j++) acc += (1.0 - lw[j]) * Dp[j];
    }
    if (bid == 0) {  // the mass point: sum_{j < clo} D_prev[j] -> row 0, by the column's 32 lanes
        const int clo = R.clo[(size_t)t * c.n_e + e];
        double part = 0.0;
        for (int j = row; j < clo; j += RBP) part += Dp[j];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        if (row == 0) acc += part;
    }
    if (r < n) Dsh[e * RBP + row] = acc;
    lds_barrier();
    // two aggregates of the POST-transition distribution (ForwardIteration.jl:301-307): the policy-weighted one (the heterogeneous
    // variable itself) and the wealth-GRID-weighted one, sum_pt a(pt) D_t(pt) — with it every heterogeneous output that is affine
    // in the policy, the state and the household inputs (consumption, cash on hand: BackwardIteration.jl:99-112 routes every key
    // of the plugin's NamedTuple) is assembled on the host. aggpart: [t][block][2]
    double part = 0.0, part2 = 0.0;
    if (r < n) {
        const int e2 = e;  // D_new[r,e2] = sum_e D_mid[r,e] * Pi[e,e2]
        double Dn = 0.0;
        Dn = mix_sum(Dn, Dsh + row, RBP, Pish + c.n_e * e2, 1, 0, c.n_e);
        (Dout ? Dout[(size_t)e2 * n + r] : R.Dseq[(size_t)(t + 1) * c.G + (size_t)e2 * n + r]) = Dn;
        part = R.pol[base + (size_t)e2 * n + r] * Dn;
        part2 = c.a[r] * Dn;
    }
    const double tot = block_sum(part, red, nthr);
    const double tot2 = block_sum(part2, red, nthr);
    if (threadIdx.x == 0) { aggpart[((size_t)t * nblocks + bid) * 2] = tot; aggpart[((size_t)t * nblocks + bid) * 2 + 1] = tot2; }
}
__global__ void k_dist_step(Consts c, Record R, int t, double *aggpart) {
    extern __shared__ double sh[];
    dist_step_body(c, R, t, aggpart, blockIdx.x, gridDim.x, sh);
}
// one application of the (fixed) transition of record period 0 to an explicit distribution: D_out = Lambda D_in
__global__ void k_dist_iter(Consts c, Record R, const double *Din, double *Dout, double *aggpart, const int *stop) {
    extern __shared__ double sh[];
    if (stop && *stop) return;
    dist_step_body(c, R, 0, aggpart, blockIdx.x, gridDim.x, sh, Din, Dout);
}

// supnorm_block: max|Vnew - Vold| over G points by one block of up to 1024 threads, valid in thread 0 (NaN when any difference is);
// the body of k_vfi_check and of the scenario batch's checks (hank_ssbatch.h). red: 16 doubles of LDS.
__device__ __forceinline__ double supnorm_block(const double *Vnew, const double *Vold, int G, double *red) {
    double m = 0.0;
    bool bad = false;
    for (int i = threadIdx.x; i < G; i += blockDim.x) {
        const double d = fabs(Vnew[i] - Vold[i]);
        if (!(d == d)) bad = true;
        m = d > m ? d : m;
    }
    if (bad) m = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(m, off, 64); m = (o > m || !(o == o)) ? o : m; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < (int)(blockDim.x >> 6); k++) m = (red[k] > m || !(red[k] == red[k])) ? red[k] : m;
    return m;
}
// one convergence check of the steady state's inner fixed point (SteadyState.jl:136-139: max|value_new - value| < tol,
// after EVERY step): one block; state = {stop, steps done}. A NaN norm never stops the loop, as in the reference.
__global__ void k_vfi_check(const double *Vnew, const double *Vold, int G, double tol, int *state, double *norm_out) {
    __shared__ double red[16];
    if (state[0]) return;
    const double m = supnorm_block(Vnew, Vold, G, red);
    if (threadIdx.x == 0) {
        state[1] += 1;
        *norm_out = m;
        if (m < tol) state[0] = 1;
    }
}

// zero fills as kernels (no memset nodes inside the captured graphs)
__global__ void k_zero_i32(int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}
__global__ void k_zero_f64(double *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.0;
}

// out[t*N + n] = sum_b parts[(t*nb + b)*N + n]; one block per (t, 64-wide tangent chunk), four
// groups of 64 lanes stride over the row blocks, fixed combination order: bitwise reproducible
__global__ void k_reduce_parts(const double *__restrict__ parts, int nb, int N, double *__restrict__ out) {
    __shared__ double red[256];
    const int t = blockIdx.x, nl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + nl;
    double s = 0.0;
    if (n < N) {
        const double *p = parts + (size_t)t * nb * N + n;
        int b = g;
        for (; b + 28 < nb; b += 32) {      // 8 independent loads in flight per lane
            const double v0 = p[(size_t)b * N], v1 = p[(size_t)(b + 4) * N], v2 = p[(size_t)(b + 8) * N], v3 = p[(size_t)(b + 12) * N];
            const double v4 = p[(size_t)(b + 16) * N], v5 = p[(size_t)(b + 20) * N], v6 = p[(size_t)(b + 24) * N], v7 = p[(size_t)(b + 28) * N];
            s += ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7));
        }
        for (; b < nb; b += 4) s += p[(size_t)b * N];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && n < N) out[(size_t)t * N + n] = (red[nl] + red[64 + nl]) + (red[128 + nl] + red[192 + nl]);
}

// ---- tangent sweeps ------------------------------------------------------------------------
// One wavefront per productivity column e: lane = (tangent nl fastest, wealth row rl), so a wave
// instruction moves RB = 64/NC adjacent rows x NC lanes' worth of tangents = one contiguous 512-byte
// (one direction per lane) or 1-KiB (two per lane) piece of the [e][a][N] state. The n_e x n_e mixing goes through a 64 x n_e LDS tile (conflict-free: the lane
// is the fastest LDS index). Block = 64*n_e threads.

// (n_hh, P, N) column-major  ->  dxr[P][N], dxw[P][N] (, dxt[P][N] when the family has a transfer input)
__global__ void k_tan_in(const double *__restrict__ dxhh, int n_hh, int P, int N, double *__restrict__ dxr, double *__restrict__ dxw,
                         double *__restrict__ dxt) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int t = idx / N, n = idx - t * N;
    const double *x = dxhh + (size_t)n_hh * ((size_t)t + (size_t)P * n);
    dxr[idx] = x[0];
    dxw[idx] = x[1];
    if (n_hh > 2) dxt[idx] = x[2];
}
// dagg[P][N] -> (P, N) column-major
__global__ void k_tan_out(const double *__restrict__ dagg, int P, int N, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int n = idx / P, t = idx - n * P;
    out[idx] = dagg[(size_t)t * N + n];
}

// one backward period: tan_back_body (hank_device.h)
template <int RG, typename VT>
__global__ void __launch_bounds__(1024)
k_tan_back(Consts c, Record R, const double *__restrict__ xhh, const VT *__restrict__ dxr,
           const VT *__restrict__ dxw, const VT *__restrict__ dxt, TanGeom g, int t, int first, const VT *__restrict__ dsIn,
           VT *__restrict__ dsOut, VT *__restrict__ dpol) {
    __shared__ VT dVsh[RG][16 * 64];
    __shared__ double Pish[256];
    tan_back_body<RG, VT>(c, R, xhh, dxr, dxw, dxt, g, t, first, dsIn, dsOut, dpol, blockIdx.x, blockIdx.y, dVsh, Pish);
}

// the dual-sweep backward launch: blocks [0, nbp) of grid row 0 run the PRIMAL EGM step of period tp,
// the others the tangent step of period tt = tp + 1 (whose record the previous launch wrote) — both
// recurrences advance in one chain of T launches instead of two.
template <int RG, typename VT>
__global__ void __launch_bounds__(1024)
k_fused_back(Consts c, Record R, const double *__restrict__ xhh, int *err, int tp, int nbp,
             const VT *__restrict__ dxr, const VT *__restrict__ dxw, const VT *__restrict__ dxt, TanGeom g, int tt, int first,
             const VT *__restrict__ dsIn, VT *__restrict__ dsOut, VT *__restrict__ dpol) {
    __shared__ VT dVsh[RG][16 * 64];
    __shared__ double Pish[256];
    if ((int)blockIdx.x < nbp) {
        if (blockIdx.y != 0 || tp < 0 || (int)threadIdx.x >= RBP * c.n_e) return;
        egm_step_body(c, R, xhh, tp, err, blockIdx.x, reinterpret_cast<double *>(&dVsh[0][0]));   // needs n_e*RBP + n_e^2 <= 768 doubles
        return;
    }
    if (tt < 0) return;
    tan_back_body<RG, VT>(c, R, xhh, dxr, dxw, dxt, g, tt, first, dsIn, dsOut, dpol, blockIdx.x - nbp, blockIdx.y, dVsh, Pish);
}

// one forward period: tan_fwd_body (hank_device.h)
template <int RG, typename VT, bool SS>
__global__ void __launch_bounds__(1024)
k_tan_fwd(Consts c, Record R, TanGeom g, int t, const VT *__restrict__ dDin, VT *__restrict__ dDout,
          const VT *__restrict__ dpol, VT *__restrict__ aggpart) {
    __shared__ VT sh[RG][16 * 64];
    __shared__ VT red[16 * 64], red2[16 * 64];
    __shared__ double Pish[256];
    tan_fwd_body<RG, VT, SS>(c, R, g, t, dDin, dDout, dpol, aggpart, blockIdx.x, blockIdx.y, gridDim.x, sh, Pish, red, red2);
}

// the forward tangent launch with NX = 1, 2 extra reductions (hank_jvp_het): k_tan_fwd keeps its name and its arguments, so the
// NX = 0 launch is the kernel it was
template <int RG, typename VT, bool SS, int NX>
__global__ void __launch_bounds__(1024)
k_tan_fwd_hx(Consts c, Record R, TanGeom g, int t, const VT *__restrict__ dDin, VT *__restrict__ dDout,
             const VT *__restrict__ dpol, VT *__restrict__ aggpart, TanHx<VT, NX> hx) {
    __shared__ VT sh[RG > NX ? RG : NX][16 * 64];
    __shared__ VT red[16 * 64], red2[16 * 64];
    __shared__ double Pish[256];
    tan_fwd_body<RG, VT, SS, NX>(c, R, g, t, dDin, dDout, dpol, aggpart, blockIdx.x, blockIdx.y, gridDim.x, sh, Pish, red, red2, hx);
}
// T[n][t][jx] = sum_b parts[((t nb + b) NX + jx) N + n] (the layout k_het_outputs reads as hxT); one block per (t, 64-wide chunk
// of the NX N columns), in the manner of k_reduce_parts: four groups of lanes stride over the blocks in order, then the groups combine
__global__ void k_reduce_hx(const double *__restrict__ parts, int nb, int NX, int N, int P, double *__restrict__ T) {
    __shared__ double red[256];
    const int t = blockIdx.x, nl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int col = blockIdx.y * 64 + nl, W = NX * N;
    double s = 0.0;
    if (col < W) {
        const double *p = parts + (size_t)t * nb * W + col;
        for (int b = g; b < nb; b += 4) s += p[(size_t)b * W];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && col < W) {
        const int jx = col / N, n = col - jx * N;
        T[((size_t)n * P + t) * NX + jx] = (red[nl] + red[64 + nl]) + (red[128 + nl] + red[192 + nl]);
    }
}

// the dual-sweep forward launch: blocks [0, nbp) of grid row 0 run the PRIMAL distribution step of
// period tp, the others the tangent step of period tt = tp - 1 (D_{tt+1} was written by the previous launch).
template <int RG, typename VT, bool SS>
__global__ void __launch_bounds__(1024)
k_fused_fwd(Consts c, Record R, int tp, int nbp, double *__restrict__ paggpart, TanGeom g, int tt,
            const VT *__restrict__ dDin, VT *__restrict__ dDout, const VT *__restrict__ dpol,
            VT *__restrict__ aggpart) {
    __shared__ VT sh[RG][16 * 64];
    __shared__ VT red[16 * 64], red2[16 * 64];
    __shared__ double Pish[256];
    if ((int)blockIdx.x < nbp) {
        if (blockIdx.y != 0 || tp < 0 || (int)threadIdx.x >= RBP * c.n_e) return;
        dist_step_body(c, R, tp, paggpart, blockIdx.x, nbp, reinterpret_cast<double *>(&sh[0][0]));
        return;
    }
    if (tt < 0) return;
    tan_fwd_body<RG, VT, SS>(c, R, g, tt, dDin, dDout, dpol, aggpart, blockIdx.x - nbp, blockIdx.y, gridDim.x - nbp, sh, Pish, red, red2);
}

// ---- granular tangent halves (hank_backward_step_dual) ---------------------------------------
// X-tangent alone: dV' (G,N col-major) -> ds[e][a][N]
__global__ void k_tan_X(Consts c, const double *kc, const double *s, double r, const double *dr,
                        const double *dw, const double *dtr, int N, const double *dVin_colmajor, double *dsOut) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= c.G * N) return;
    const int n = idx % N, pt = idx / N, e = pt / c.n_a, a = pt - e * c.n_a;
    double dE = 0.0;
    for (int e2 = 0; e2 < c.n_e; e2++) dE += dVin_colmajor[(size_t)n * c.G + (size_t)e2 * c.n_a + a] * c.Pi[e + c.n_e * e2];
    const double rho = 1.0 / (1.0 + r);
    dsOut[(size_t)pt * N + n] = kc[pt] * dE - rho * ((c.z[e] * dw[n] + (dtr ? dtr[n] : 0.0)) + s[pt] * dr[n]);
}
// Y-tangent alone: ds -> dpol, dV (both (G,N) col-major for the caller)
__global__ void k_tan_Y(Consts c, const int *ib, const double *A, const double *B, const double *u,
                        const double *v, const double *dr, const double *dw, const double *dtr, int N,
                        const double *ds, double *dpol_cm, double *dV_cm) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= c.G * N) return;
    const int n = idx % N, pt = idx / N, e = pt / c.n_a, a = pt - e * c.n_a;
    const int i = ib[pt];
    const double *col = ds + ((size_t)e * c.n_a) * N + n;
    const double dg = A[pt] * col[(size_t)i * N] + B[pt] * col[(size_t)(i + 1) * N];
    dpol_cm[(size_t)n * c.G + pt] = dg;
    dV_cm[(size_t)n * c.G + pt] = u[pt] * dr[n] + v[pt] * ((c.a[a] * dr[n] + (c.z[e] * dw[n] + (dtr ? dtr[n] : 0.0))) - dg);
}

// ---- granular forward step for ARBITRARY policies (atomic scatter; parity tests of a6/a7) -----
// Dmid [G*(1+N)]: slot 0 = value, slots 1..N = partials, layout [pt][1+N]
__global__ void k_scatter_general(Consts c, const double *policy, const double *dpolicy_cm,
                                  const double *Dprev, const double *dDprev_cm, int N, double *Dmid) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int W = 1 + N;
    if (idx >= c.G * W) return;
    const int k = idx % W, pt = idx / W, e = pt / c.n_a;
    const int n = c.n_a;
    const double p = policy[pt];
    int lo = -1, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (c.a[mid] < p) lo = mid; else hi = mid;
    }
    const double Dv = Dprev[pt];
    const double dD = k ? dDprev_cm[(size_t)(k - 1) * c.G + pt] : 0.0;
    const double val = k ? dD : Dv;  // the slot's "D"
    if (hi == 0) {
        atomicAdd(&Dmid[((size_t)e * n + 0) * W + k], val);
    } else if (hi >= n) {
        atomicAdd(&Dmid[((size_t)e * n + n - 1) * W + k], val);
    } else {
        const int l = hi - 1;
        const double gap = c.a[hi] - c.a[l];
        const double w = (p - c.a[l]) / gap;
        if (k == 0) {
            atomicAdd(&Dmid[((size_t)e * n + l) * W], (1.0 - w) * Dv);
            atomicAdd(&Dmid[((size_t)e * n + hi) * W], w * Dv);
        } else {
            const double dwt = dpolicy_cm[(size_t)(k - 1) * c.G + pt] / gap;
            atomicAdd(&Dmid[((size_t)e * n + l) * W + k], (1.0 - w) * dD - dwt * Dv);
            atomicAdd(&Dmid[((size_t)e * n + hi) * W + k], w * dD + dwt * Dv);
        }
    }
}
// mix over e + per-point aggregate terms; outputs col-major (G) and (G,N); aggterm[pt*(1+N)+k]
__global__ void k_mix_general(Consts c, const double *Dmid, const double *policy,
                              const double *dpolicy_cm, int N, double *Dout, double *dDout_cm,
                              double *aggterm) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int W = 1 + N;
    if (idx >= c.G * W) return;
    const int k = idx % W, pt = idx / W, e2 = pt / c.n_a, a = pt - e2 * c.n_a;
    double s = 0.0;
    for (int e = 0; e < c.n_e; e++) s += Dmid[((size_t)e * c.n_a + a) * W + k] * c.Pi[e + c.n_e * e2];
    if (k == 0) {
        Dout[pt] = s;
        aggterm[(size_t)pt * W] = policy[pt] * s;
    } else {
        dDout_cm[(size_t)(k - 1) * c.G + pt] = s;
        double Dn = 0.0;
        for (int e = 0; e < c.n_e; e++) Dn += Dmid[((size_t)e * c.n_a + a) * W] * c.Pi[e + c.n_e * e2];
        aggterm[(size_t)pt * W + k] = policy[pt] * s + dpolicy_cm[(size_t)(k - 1) * c.G + pt] * Dn;
    }
}
// out[k] = sum_pt aggterm[pt*W + k], one block per k (fixed order within the block tree)
__global__ void k_colsum(const double *aggterm, int G, int W, double *out) {
    __shared__ double red[16];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int pt = threadIdx.x; pt < G; pt += blockDim.x) s += aggterm[(size_t)pt * W + k];
    const double tot = block_sum(s, red, blockDim.x);
    if (threadIdx.x == 0) out[k] = tot;
}

// (G,P,N) col-major export of dpol[P][G][N]
__global__ void k_export_dpol(const double *dpol, int G, int P, int N, double *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)G * P * N;
    if (idx >= total) return;
    const size_t n = idx / ((size_t)G * P), rem = idx - n * (size_t)G * P, t = rem / G, pt = rem - t * G;
    out[idx] = dpol[(t * G + pt) * N + n];
}

}  // namespace hank
