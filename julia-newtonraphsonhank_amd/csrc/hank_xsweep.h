// hank_xsweep.h — the XCD-local persistent sweeps: ONE launch per sweep instead of one per period.
//
// The same recurrences as hank_kernels.h (BackwardIteration.jl:90-113, ForwardIteration.jl:297-308 and their partials
// under Dual{Tag,Float64,N}), behind the same entry points and on the same record, as six persistent kernels:
//   k_xprimal_back, k_xfwd<0, true>  : the Float64 recurrences (they record the linearisation),
//   k_xtan_back<D>, k_xfwd<D, false> : the N partials as linear recurrences at that record (the whole y-iteration keeps x
//                                      fixed, NewtonRaphson.jl:91-111; so does every pass of a wide batch),
//   k_xdual_back<D>, k_xfwd<D, true> : value AND partials in one chain of periods (the Dual pass, hank_primal_jvp),
//   k_xvfi, k_xstat                  : the steady state's two fixed points, one launch each, with a convergence vote.
// What they share is stated once: the LDS layouts (hank_xlds.h: the kernel's pointers and the host's launch size from ONE struct), admission
// and wave roles (xmember_join, xroles), the group barrier and the vote (xbar_*, xpoll, xvote), the staging (xstage_*) and egm_X_point.
//
// Mapping (MI355X: 8 XCDs x 32 CUs, one 4 MiB L2 per XCD, L2s not coherent with each other):
//   * a launch has one workgroup per CU; each workgroup reads the XCD it actually runs on (HW_REG_XCC_ID) and takes a
//     ticket there: the workgroups of one XCD form a GROUP. Nothing assumes a placement — a group that does not have
//     the members it needs reports XERR_PLACEMENT and the host falls back to the per-period launches.
//   * inside a group, workgroup c owns 63 wealth rows (all n_e productivity columns: wave = column, lane = row).
//   * tangent sweeps: group x owns the directions [x*D, (x+1)*D) of the pass (D = 1, 2 or 4; 8*D directions per pass);
//     Float64 sweeps: the group of XCD 0 runs them, the other workgroups leave at once.
//   * the loop-carried state (EGM knots s_t / their partials ds_t backward; D_t / dD_t forward) lives in a small
//     ping-pong buffer in the XCD's L2: written with plain stores (the line stays in that L2), read back — after ONE
//     group barrier per period — with sc1 loads, which bypass the reading CU's L1 and are served by that same L2. No
//     kernel boundary, no fence, no atomics in the loop.
//   * group barrier: every storing wave drains (vmcnt(0)), raw s_barrier, the member publishes the episode number in ITS
//     flag line with a plain store, one wave polls all members' lines with one sc1 load per trip, s_barrier. It comes in
//     two halves (arrive / wait) so that loads which do not depend on the other members fly while the group meets.
//     Every spin is bounded; on timeout a status word is set and every later wait falls through: the grid always drains.
//   * what a period reads that is uniform over the workgroup (r_t, w_t, rho_t, dr/dw/dtr of the group, the clamped prefix
//     lengths) is LDS-resident for the whole sweep: as a per-period global load each is a cold round trip on the
//     critical path.
//
// Layouts:  Float64 state   st_s [2][XG][G] (backward), st_D [2][XG][G + 64*n_e] (forward; the tail holds the virtual rows)
//           tangent state   D/2 PLANES of 16-byte pairs, [plane][2][XG][rows][2] (D = 1: [2][XG][rows]): a store instruction
//                           writes 16 contiguous bytes per lane, whole lines per wave (XRows). rows = G backward; forward
//                           [n_e][members][64]: a member's 63 rows + its virtual row (slot 63) are one line-aligned block
//           dpol            [P][groups][n_e][n_a][D] — a group's stream is contiguous: whole lines, one XCD each.
// What was measured on the way (a dual kernel carrying value and partials together, a run-ahead wave, atomic-counter
// barriers, ...) is in DESIGN.md section 4.
#pragma once
#include "hank_kernels.h"
#include "hank_xaddr.h"
#include "hank_xlds.h"
#include "hank_xunits.h"
#include <type_traits>

namespace hank {

constexpr int XG = 8;             // groups = XCDs
constexpr int XRW = 63;           // wealth rows per workgroup; lane 63 of every wave is the forward sweep's virtual row
enum { XERR_TIMEOUT = 1, XERR_PLACEMENT = 2 };
// Every wait is bounded in TIME: s_memrealtime counts at 100 MHz for the whole chip, a wait that has lasted longer than
// g_xwait_ticks (20 ms unless HANK_XWAIT_MS says otherwise at hank_create: four thousand periods' worth) marks the launch failed
// and every later wait falls through, so the grid always drains and the host learns how long the sweep had waited.
__device__ unsigned long long g_xwait_ticks = 2000000ull;
struct XDeadline {
    unsigned long long t0;
    __device__ __forceinline__ XDeadline() : t0(__builtin_amdgcn_s_memrealtime()) {}
    __device__ __forceinline__ bool expired(unsigned spins) const { return (spins & 63u) == 63u && __builtin_amdgcn_s_memrealtime() - t0 > g_xwait_ticks; }
    __device__ __forceinline__ unsigned waited_us() const { return (unsigned)((__builtin_amdgcn_s_memrealtime() - t0) / 100ull); }
};

struct XSync {                    // zeroed by a memset node before EVERY launch (66.9 KB, a multiple of 16)
    unsigned ticket[XG][32];      // [x][0]: workgroups that arrived on XCD x (one 128-B line each)
    unsigned total[32];           // [0]: workgroups that hold a ticket
    unsigned flag[XG][64][32];    // [x][c][0]: the last barrier episode member c of group x has reached — one 128-B line per
                                  // member: 32 writers and 32 pollers on ONE line queue at one L2 channel (1.0-1.15 us per
                                  // episode against 0.71, scripts/ubench/xbar_bench.hip)
    unsigned status[32];          // [0]: XERR_* (sticky), [1]: the XCD that raised it, [2]: microseconds the wait that timed out had lasted
    unsigned pad[32];
};

typedef unsigned int xv4u __attribute__((ext_vector_type(4)));

template <class T>      // a piece of a kernel's dynamic LDS at the byte offset its layout states (hank_xlds.h)
__device__ __forceinline__ T *xlds_at(double *xl, unsigned off) { return reinterpret_cast<T *>(reinterpret_cast<char *>(xl) + off); }

__device__ __forceinline__ double xld(const double *p) {      // 8-byte sc1 load: bypasses L1, served by the XCD's L2
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned xldu(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one row of D partials (8*D bytes, 8*D-aligned) with sc1 loads: 16-byte buffer loads where the row allows
// The state of D partials per row is kept as D/2 PLANES of 16-byte pairs ([plane][row][2]; D = 1: [row]): one store
// instruction then writes 16 contiguous bytes per lane, whole lines per wave. With [row][D] a D = 4 row took two store
// instructions that each wrote half of every 32-byte sector.
template <int D>
struct XRows {
    __amdgpu_buffer_rsrc_t rs;
    double *base;
    size_t plane;               // rows per plane = rows of the whole buffer
    __device__ __forceinline__ void init(double *p, size_t rows_total) {
        base = p; plane = rows_total;
        if (D >= 2) rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)(rows_total * 8 * D), 0x00020000);
    }
    // row index counts rows from `base` (ping-pong half and group are part of the row index)
    __device__ __forceinline__ void load(size_t row, double *v) const {
        if (D == 1) {
            v[0] = xld(base + row);
        } else {
#pragma unroll
            for (int k = 0; k < D / 2; k++) {
                const xv4u q = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((k * plane + row) * 16), 0, 16);   // aux 16 = sc1
                v[2 * k] = __hiloint2double((int)q.y, (int)q.x);
                v[2 * k + 1] = __hiloint2double((int)q.w, (int)q.z);
            }
        }
    }
    __device__ __forceinline__ double load_one(size_t row, int k) const {            // slot k of a row (sc1, 8 bytes)
        return D == 1 ? xld(base + row) : xld(base + ((size_t)(k / 2) * plane + row) * 2 + (k & 1));
    }
    // the descriptor path (k_xdual_back, k_xfwd<D, true>): the row index in two parts — the lane's (rv, 32-bit, often loop-invariant) and the wave's (rs_, scalar: ping-pong
    // half, group, column) — straight into the instruction's vector and scalar offsets. init_buf: a descriptor for D = 1 too
    static constexpr int RB = D == 1 ? 8 : 16;       // bytes of a row in one plane
    __device__ __forceinline__ void init_buf(double *p, int rows_total) {
        base = p; plane = (size_t)rows_total;
        rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, rows_total * 8 * D, 0x00020000);
    }
    __device__ __forceinline__ void load_vs(int rv, int rs_, double *v) const {     // sc1
        if (D == 1) {
            v[0] = buf_ld64<16>(rs, rv * RB, rs_ * RB);
        } else {
#pragma unroll
            for (int k = 0; k < D / 2; k++) {
                const xv4u q = __builtin_amdgcn_raw_buffer_load_b128(rs, rv * RB, (k * (int)plane + rs_) * RB, 16);
                v[2 * k] = __hiloint2double((int)q.y, (int)q.x);
                v[2 * k + 1] = __hiloint2double((int)q.w, (int)q.z);
            }
        }
    }
    __device__ __forceinline__ void store_vs(int rv, int rs_, const double *v) const {      // plain
        if (D == 1) {
            buf_st64<0>(v[0], rs, rv * RB, rs_ * RB);
        } else {
#pragma unroll
            for (int k = 0; k < D / 2; k++) buf_st2d<0>(v[2 * k], v[2 * k + 1], rs, rv * RB, (k * (int)plane + rs_) * RB);
        }
    }
    __device__ __forceinline__ void store(size_t row, const double *v) const {      // plain stores: the line stays in the XCD's L2
        if (D == 1) {
            base[row] = v[0];
        } else {
#pragma unroll
            for (int k = 0; k < D / 2; k++) reinterpret_cast<double2 *>(base)[k * plane + row] = make_double2(v[2 * k], v[2 * k + 1]);
        }
    }
};
// the policy partials are a pure stream: written once by the backward sweep, read once by the forward sweep. Stores are
// nontemporal (the lines are not kept for a reader that comes a whole sweep later: backward sweep 1.36 -> 1.28 ms at
// N = 32); loads stay plain — a row is one member's own row AND a source of its neighbours in the same period, and with
// nontemporal loads the forward sweep took 3.46 ms instead of 2.25 (profiles/r03_col_nt_stream.log). L2 is write-through
// either way: every stored byte reaches the fabric once (WRITE_SIZE = stream + state with both flavours).
typedef double xv2d __attribute__((ext_vector_type(2)));
template <int D>
__device__ __forceinline__ void xstore_row(double *p, const double *v) {
    if (D == 1) {
        __builtin_nontemporal_store(v[0], p);
    } else {
#pragma unroll
        for (int k = 0; k < D / 2; k++) { xv2d q; q.x = v[2 * k]; q.y = v[2 * k + 1]; __builtin_nontemporal_store(q, reinterpret_cast<xv2d *>(p) + k); }
    }
}
template <int D>
__device__ __forceinline__ void xstore_row_buf(__amdgpu_buffer_rsrc_t rs, int vo, int so, const double *v) {     // the same through a buffer descriptor
    if (D == 1) {
        buf_st64<2>(v[0], rs, vo, so);
    } else {
#pragma unroll
        for (int k = 0; k < D / 2; k++) buf_st2d<2>(v[2 * k], v[2 * k + 1], rs, vo + 16 * k, so);
    }
}
template <int D>
__device__ __forceinline__ void xload_row_buf(__amdgpu_buffer_rsrc_t rs, int vo, int so, double *v) {           // plain loads
    if (D == 1) {
        v[0] = buf_ld64<0>(rs, vo, so);
    } else {
#pragma unroll
        for (int k = 0; k < D / 2; k++) wide_ld2d<0>(rs, vo + 16 * k, so, v[2 * k], v[2 * k + 1]);
    }
}
template <int D>
__device__ __forceinline__ void xload_row_plain(const double *p, double *v) {  // read-only inputs (written by an earlier launch)
    if (D == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int k = 0; k < D / 2; k++) { const double2 q = reinterpret_cast<const double2 *>(p)[k]; v[2 * k] = q.x; v[2 * k + 1] = q.y; }
    }
}

// The descriptor path's sweep-long wave-uniform integers: one whose TESTS are made anew where they are used (one s_cmp / s_bitcmp on one
// scalar register). Left to itself the compiler hoists every test `k < ne`, `flags & bit` out of the period loop as a 64-bit lane
// mask of its own: more of them than there are scalar registers, so each costs two v_readlane per period.
__device__ __forceinline__ int xopaque(int v) { asm volatile("" : "+s"(v)); return v; }

struct XMember { int x, c, Sact; bool on; };       // the XCD, the member index in its group, the members that own rows; on: this workgroup is one of them
struct XRoles { int lane, wv, e; bool syncw, sync_duty; };

// dev build only (make stamp): s_memtime stamps of lane 0 / wave 0 of the first and last member of group 0, periods
// [XSTAMP_T0, XSTAMP_T0+8): where a period's time goes. Never compiled into the product library.
#ifdef HANK_XSTAMP
#ifndef HANK_XSTAMP_T0
#define HANK_XSTAMP_T0 100
#endif
#ifndef HANK_XSTAMP_STRIDE
#define HANK_XSTAMP_STRIDE 1       // > 1: every STRIDE-th period from T0 on is stamped (where in the sweep the time goes)
#endif
constexpr int XSTAMP_T0 = HANK_XSTAMP_T0, XSTAMP_NP = 8, XSTAMP_NS = 12, XSTAMP_ST = HANK_XSTAMP_STRIDE;
#define XSTAMP_ON(per) ((per) >= XSTAMP_T0 && (per) < XSTAMP_T0 + XSTAMP_NP * XSTAMP_ST && ((per) - XSTAMP_T0) % XSTAMP_ST == 0)
#define XSTAMP_SLOT(per) (((per) - XSTAMP_T0) / XSTAMP_ST)
__device__ unsigned long long g_xstamps[2][32][XSTAMP_NP][XSTAMP_NS];     // [sweep][member of group 0][period][stamp]
#define XSTAMP(sw, on, per, i)                                                                                   \
    do {                                                                                                         \
        if ((on) >= 0 && XSTAMP_ON(per) && threadIdx.x == 0)                 \
            g_xstamps[sw][on][XSTAMP_SLOT(per)][i] = __builtin_amdgcn_s_memrealtime();                              \
    } while (0)
// every wave's arrival at one chosen point of the period (lane 0 of each wave)
__device__ unsigned long long g_xwaves[2][32][XSTAMP_NP][16];
#define XSTAMPV(sw, on, per)                                                                                     \
    do {                                                                                                         \
        if ((on) >= 0 && XSTAMP_ON(per) && (threadIdx.x & 63) == 0)          \
            g_xwaves[sw][on][XSTAMP_SLOT(per)][threadIdx.x >> 6] = __builtin_amdgcn_s_memrealtime();             \
    } while (0)
// once per kernel (entry, prologue done, loop done): slot 0, stamps 9..11
#define XSTAMP1(sw, on, i) do { if ((on) >= 0 && threadIdx.x == 0) g_xstamps[sw][on][0][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define XSTAMP1(sw, on, i) do {} while (0)
#define XSTAMPV(sw, on, per) do {} while (0)
#define XSTAMP(sw, on, per, i) do {} while (0)
#endif

__device__ inline void xfail(XSync *sy, unsigned code, int x, unsigned waited_us = 0u) {
    if (__hip_atomic_exchange(&sy->status[0], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
        __hip_atomic_store(&sy->status[1], (unsigned)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sy->status[2], waited_us, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// dev knob HANK_XFAULT: the status word of a launch's sync block pre-set by the host
__global__ void k_xpoison(XSync *base, int count, unsigned code) {
    if ((int)threadIdx.x < count) { base[threadIdx.x].status[0] = code; base[threadIdx.x].status[1] = 0u; }
}

// Admission, the same for every persistent kernel: which XCD am I on, which member of its group am I, how many members does it
// have (known once EVERY workgroup of the launch holds a ticket: one launch-wide wait at the start of the sweep, none afterwards).
// A workgroup takes part (`on`) if the launch has not failed, its XCD is one of the `groups` that work (1: the Float64 sweeps, XCD 0
// only) and it is one of the Sact members that own rows; a group of fewer reports XERR_PLACEMENT (the whole group agrees on the count).
__device__ __forceinline__ XMember xmember_join(XSync *sy, int *ctl, int groups, int n_a) {
    if (threadIdx.x == 0) {
        int xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 7;
        if (xldu(&sy->status[0]) != 0u) {       // the launch is already marked failed (a sibling gave up; the dev knob): leave at once
            ctl[0] = xcc; ctl[1] = 0; ctl[2] = 0; ctl[3] = 0;
        } else {
            const unsigned c = __hip_atomic_fetch_add(&sy->ticket[xcc][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the ticket is taken before it is counted
            __hip_atomic_fetch_add(&sy->total[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int ok = 1;
            const XDeadline dl;
            for (unsigned spins = 0;; spins++) {
                if (xldu(&sy->total[0]) >= gridDim.x) break;
                if (dl.expired(spins) || ((spins & 255u) == 255u && xldu(&sy->status[0]) != 0u)) { xfail(sy, XERR_TIMEOUT, xcc, dl.waited_us()); ok = 0; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            ctl[0] = xcc; ctl[1] = (int)c; ctl[2] = (int)xldu(&sy->ticket[xcc][0]); ctl[3] = ok;
        }
    }
    __syncthreads();
    XMember m;
    m.x = __builtin_amdgcn_readfirstlane(ctl[0]); m.c = __builtin_amdgcn_readfirstlane(ctl[1]);
    const int S = __builtin_amdgcn_readfirstlane(ctl[2]), ok = __builtin_amdgcn_readfirstlane(ctl[3]);
    m.Sact = (n_a + XRW - 1) / XRW;
    m.on = false;
    if (!ok || m.x >= groups) return m;
    if (S < m.Sact) { if (threadIdx.x == 0) xfail(sy, XERR_PLACEMENT, m.x); return m; }
    m.on = m.c < m.Sact;
    return m;
}
// Wave roles of a member: wave e < n_e is column e (lane = row); a block with room for one more wave has a SYNC wave with no memory traffic
// of its own that runs the group barrier's polls (else wave 0 does: sync_duty). The wave index is a scalar register: column bases become scalar.
__device__ __forceinline__ XRoles xroles(int ne) {
    XRoles r;
    r.lane = threadIdx.x & 63; r.wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    r.syncw = r.wv >= ne;
    r.sync_duty = blockDim.x > 64 * ne ? r.syncw : r.wv == 0;
    r.e = r.syncw ? 0 : r.wv;
    return r;
}

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, NOT for its global loads and stores
// (__syncthreads() carries a fence that drains vmcnt: the dpol stores and the run-ahead touches would stall here)
__device__ __forceinline__ void xlds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The group barrier. No atomics (they execute at the memory side, a fabric round trip each): member c publishes the episode
// number in ITS flag line with a plain store — the line lives in the XCD's L2 like the state itself — and one wave of
// every member polls all members' lines with ONE sc1 load per trip.
// It comes in two halves, so that loads which do not depend on the other members (next period's record) can be
// issued BETWEEN them and fly while the group meets: arrive = every storing wave drains, the workgroup meets; wait = the
// SYNC wave (an extra wave with no memory traffic of its own where the block has room for one, else wave 0) publishes
// this member's episode and polls the group's flags, then the workgroup meets again.
__device__ __forceinline__ void xbar_arrive(bool drain) {
    if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    xlds_barrier();
}
// the wait half's two steps, each run by ONE wave: publish this member's episode; poll the flag lines of members lo..hi until every one
// has reached `need` (bounded: see XDeadline)
__device__ __forceinline__ void xpublish(XSync *sy, int x, int c, unsigned episode) {
    if ((threadIdx.x & 63) == 0) *reinterpret_cast<volatile unsigned *>(&sy->flag[x][c][0]) = episode;
}
__device__ __forceinline__ void xpoll(XSync *sy, int x, int lo, int hi, unsigned need) {
    const int lane = threadIdx.x & 63;
    const XDeadline dl;
    for (unsigned spins = 0;; spins++) {
        const unsigned f = (lane >= lo && lane <= hi) ? xldu(&sy->flag[x][lane][0]) : need;
        if (__all((int)(f - need) >= 0)) break;
        if (dl.expired(spins) || ((spins & 255u) == 255u && xldu(&sy->status[0]) != 0u)) {
            if (lane == 0) xfail(sy, XERR_TIMEOUT, x, dl.waited_us());
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
__device__ __forceinline__ void xbar_wait(XSync *sy, int x, int c, int members, unsigned episode, bool sync_wave) {
    if (sync_wave) { xpublish(sy, x, c, episode); xpoll(sy, x, 0, members - 1, episode); }
    xlds_barrier();
}
// The tangent sweeps split the barrier further. A member's period t needs the state rows of FEW other members (the
// brackets / lottery segments of its 63 rows: recorded by the primal, so the range of members is known in advance), and
// it may overwrite a state half only when EVERY member is done reading it. So: (1) before a period's gathers wait only
// for the source members' episode; (2) before the period's state stores — a whole gather-and-mix phase later — check that
// all members have published the previous episode; (3) publish after the stores have drained, and wait for nobody.
// Arrival skew up to the length of the first phase disappears from the critical path.

// knots of one column, read from the L2-resident state. Everything egm_Y is going to look at in the usual case — the
// row's own knot and its lower neighbour (sortedness check), the column's two end knots (flat extrapolation) and the
// four knots around the guessed bracket — is fetched in ONE batch of independent loads up front: behind the branches
// of the bracket search each of them would be a round trip of its own. Anything else (a gallop after a far move) is
// loaded on demand.
// BUF (k_xdual_back): the column is reached through a buffer descriptor over the whole knot state — a 32-bit lane
// offset (the knot's index) and a scalar offset (ping-pong half, group, column) instead of a 64-bit address per load.
template <bool BUF>
struct XKnotsT {
    const double *p;
    __amdgpu_buffer_rsrc_t rs;
    int so;                     // BUF: the column's byte offset in the state
    int a, n, i0, i1, i2, i3;
    double sa, sam1, s0, sN, w0, w1, w2, w3;
    double ze;                  // the column's productivity z_e, from the register the kernel keeps it in for the whole sweep
    __device__ __forceinline__ double ld(int i) const {
        if constexpr (BUF) return buf_ld64<16>(rs, i * 8, so);
        else return xld(p + i);
    }
    __device__ __forceinline__ void preload(const double *col, int a_, int n_, int guess, double ze_) { p = col; batch(a_, n_, guess, ze_); }
    __device__ __forceinline__ void preload(__amdgpu_buffer_rsrc_t rs_, int so_, int a_, int n_, int guess, double ze_) { rs = rs_; so = so_; batch(a_, n_, guess, ze_); }      // BUF
    __device__ __forceinline__ void batch(int a_, int n_, int guess, double ze_) {
        a = a_; n = n_; ze = ze_;
        sa = ld(a);
        sam1 = ld(a > 0 ? a - 1 : 0);
        s0 = ld(0);
        sN = ld(n - 1);
        i0 = i1 = i2 = i3 = -1;
        w0 = w1 = w2 = w3 = 0.0;
        if (guess >= 0) {
            const int q = guess < n - 1 ? guess : n - 2;
            i0 = q > 0 ? q - 1 : 0; i1 = q; i2 = q + 1; i3 = q + 2 < n ? q + 2 : n - 1;
            w0 = ld(i0); w1 = ld(i1); w2 = ld(i2); w3 = ld(i3);
        }
    }
    // The straight-line front of egm_Y (hank_kernels.h), on the preloaded registers alone — no operator[], no branch: the
    // sortedness check, the two flat outcomes (they take precedence over the probe), the guessed bracket p (clipped to n - 2
    // by preload) and its neighbours p + 1 (if p + 2 < n) and p - 1 (if p > 0) as predicates, tried in egm_Y's order, and
    // the chosen bracket by selects. Without a guess (i1 = -1, the first period) and when no candidate holds the lane is
    // `slow`: the search finds its bracket, with on-demand loads.
    __device__ __forceinline__ YFront front(double x, int guess) const {
        YFront f;
        f.bad = a > 0 ? !(sa > sam1) : !(sa == sa);
        const bool below = x < s0, above = !below & (x > sN);
        const int p = i1;
        const bool c0 = (w1 <= x) & (x < w2);
        const bool cp = !c0 & (p + 2 < n) & (w2 <= x) & (x < w3);
        const bool cm = !c0 & !cp & (p > 0) & (w0 <= x) & (x < w1);
        f.slow = !below & !above & ((guess < 0) | !(c0 | cp | cm));
        f.where = below ? Y_BELOW : (above ? Y_ABOVE : Y_INSIDE);
        f.i = c0 ? p : (cp ? p + 1 : p - 1);
        f.si = c0 ? w1 : (cp ? w2 : w0);
        f.sj = c0 ? w2 : (cp ? w3 : w1);
        return f;
    }
    // z_e for egm_Y's tail (YColumnZOf, independent of the front). Read as c.z[e] it is a global load in every period — the
    // compiler cannot keep it across the sweep's stores — with an s_waitcnt vmcnt(0) in front of the consumption that needs it.
    __device__ __forceinline__ double column_z() const { return ze; }
    __device__ __forceinline__ double operator[](int i) const {
        if (i == a) return sa;
        if (i == a - 1) return sam1;
        if (i == i1) return w1;
        if (i == i2) return w2;
        if (i == i0) return w0;
        if (i == i3) return w3;
        if (i == 0) return s0;
        if (i == n - 1) return sN;
        return ld(i);
    }
};
using XKnots = XKnotsT<false>;

template <bool BUF> struct YFrontOf<XKnotsT<BUF>> { static constexpr bool value = true; };
template <bool BUF> struct YColumnZOf<XKnotsT<BUF>> { static constexpr bool value = true; };

__device__ __forceinline__ double xwave_sum(double v) {            // butterfly: every lane ends with the same sum, fixed order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double xmax_nan(double a, double b) { return (b > a || !(b == b)) ? b : a; }      // a NaN wins and stays
__device__ __forceinline__ double xwave_max_nan(double v) {        // butterfly: every lane ends with the wave's max
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = xmax_nan(v, __shfl_xor(v, off, 64));
    return v;
}

// The convergence vote of the two fixed points (k_xvfi, k_xstat), run by the member's sync_duty wave in place of xbar_wait: the group
// barrier carries it. The member publishes {episode, my rows converged | error word seen << 1, my max} in ONE 16-byte store to ITS flag
// line (converged: the max over redsh[0..ne), its waves' maxima of this trip, is below tol, in Float64 like k_vfi_check; a NaN never
// converges, nor a trip without a comparison: !have) and reads everybody's, bounded like every wait: a timeout says stop. Every member
// reads every line, so all leave in the same trip: ctl[4] = all have converged, ctl[5] = stop anyway; WITH_MAX: redsh[15] = the group's max.
template <bool WITH_MAX>
__device__ __forceinline__ void xvote(XSync *sy, int x, int c, int members, unsigned episode, double *redsh, int ne, bool have, double tol, unsigned bad, int *ctl) {
    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t frs = __builtin_amdgcn_make_buffer_rsrc(&sy->flag[x][0][0], 0, 64 * 32 * 4, 0x00020000);     // the group's flag lines
    double m = 0.0;
    if (have) for (int k = 0; k < ne; k++) m = xmax_nan(m, redsh[k]);
    if (lane == 0) {
        const xv4u q = {episode, ((have && m < tol) ? 1u : 0u) | (bad << 1), WITH_MAX ? (unsigned)__double2loint(m) : 0u, WITH_MAX ? (unsigned)__double2hiint(m) : 0u};
        *reinterpret_cast<volatile xv4u *>(&sy->flag[x][c][0]) = q;
    }
    xv4u f = {episode, 1u, 0u, 0u};
    const XDeadline dl;
    for (unsigned spins = 0;; spins++) {
        if (lane < members) f = __builtin_amdgcn_raw_buffer_load_b128(frs, lane * 128, 0, 16);     // sc1: served by the XCD's L2
        if (__all((int)(f.x - episode) >= 0)) break;
        if (dl.expired(spins) || ((spins & 255u) == 255u && xldu(&sy->status[0]) != 0u)) {
            if (lane == 0) xfail(sy, XERR_TIMEOUT, x, dl.waited_us());
            f.y = 2u;                               // leave the loop: the host reads the status word
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    const bool allc = __all((f.y & 1u) != 0u) != 0, anyb = __any((f.y & 2u) != 0u) != 0;      // (every lane votes: not inside the lane-0 branch)
    if (lane == 0) { ctl[4] = (have && allc) ? 1 : 0; ctl[5] = anyb ? 1 : 0; }
    if constexpr (WITH_MAX) {
        const double fm = xwave_max_nan(__hiloint2double((int)f.w, (int)f.z));
        if (lane == 0) redsh[15] = fm;
    }
}

// sum over the 64 lanes with DPP moves (no LDS traffic), fixed order; the result is valid in lane 63 ONLY
template <int CTRL, int RM, int BM>
__device__ __forceinline__ double xdpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, RM, BM, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, RM, BM, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double xwave_reduce63(double v) {
    double s = v + xdpp<0x111, 0xf, 0xf>(v);     // row_shr:1
    s = s + xdpp<0x112, 0xf, 0xf>(v);            // row_shr:2
    s = s + xdpp<0x113, 0xf, 0xf>(v);            // row_shr:3
    s = s + xdpp<0x114, 0xf, 0xe>(s);            // row_shr:4, banks 1..3
    s = s + xdpp<0x118, 0xf, 0xc>(s);            // row_shr:8, banks 2..3
    s = s + xdpp<0x142, 0xa, 0xf>(s);            // row_bcast:15 into rows 1 and 3
    s = s + xdpp<0x143, 0xc, 0xf>(s);            // row_bcast:31 into rows 2 and 3
    return s;
}

// The LDS tile of the n_e-wide mixing: [column k][lane][slot], slot 0 = the value, 1..D = the partials, padded to an
// even count SL so that a lane's slots are one run of 16-byte pieces (ds_read/write_b128; lane stride 8*SL bytes is
// conflict-free for SL = 2, 4, 6). One pass over k serves the value and every partial.
template <int SL>
__device__ __forceinline__ void xtile_store(double *t, const double *v) {      // v holds SL values
    if (SL == 1) { t[0] = v[0]; return; }
#pragma unroll
    for (int q = 0; q < SL / 2; q++) reinterpret_cast<double2 *>(t)[q] = make_double2(v[2 * q], v[2 * q + 1]);
}
template <int SL, int NS>
__device__ __forceinline__ void xtile_store_n(double *t, const double *v) {    // v holds NS <= SL values; the padding slots stay unwritten
    if (SL == 1) { t[0] = v[0]; return; }
#pragma unroll
    for (int q = 0; q < NS / 2; q++) reinterpret_cast<double2 *>(t)[q] = make_double2(v[2 * q], v[2 * q + 1]);
    if (NS & 1) t[NS - 1] = v[NS - 1];
}
// out[s] = sum_k P[k*ps] * tile[k][lane][s], k ascending, first term unrounded-added (same order as mix_sum)
// FMA: the forward sweeps (round 5) fuse the multiply-adds — a rounding away from the launches' sums, half the instructions of the
// mixing (the library is built with -ffp-contract=off: a sum written p * v + acc is two instructions)
template <int SL, int NS, bool FMA = false>
__device__ __forceinline__ void xtile_mix(const double *tl, const double *P, int ps, int ne, double *out) {
    const int ks = 64 * SL;
    auto rd = [&](int k, double *v) {                   // column k's slots of this lane
        if (SL == 1) v[0] = tl[(size_t)k * ks];
        else {
#pragma unroll
            for (int q = 0; q < (NS + 1) / 2; q++) { const double2 d = reinterpret_cast<const double2 *>(tl + (size_t)k * ks)[q]; v[2 * q] = d.x; v[2 * q + 1] = d.y; }
        }
    };
    auto acc = [&](double p, const double *v) {
#pragma unroll
        for (int q = 0; q < NS; q++) out[q] = FMA ? __builtin_fma(p, v[q], out[q]) : out[q] + p * v[q];
    };
    // the first column by itself: with `k == 0 ? p * v : fma(p, v, out)` in the loop the compiler keeps the test in every trip — a
    // product and two selects per slot and column next to the multiply-add. The operands and their order are the same.
    {
        double v[SL];
        rd(0, v);
        const double p = P[0];
#pragma unroll
        for (int q = 0; q < NS; q++) out[q] = p * v[q];
    }
    int k = 1;
    // U columns per trip: every read of the trip is in flight before its first multiply-add (left to itself the scheduler does that
    // at `unroll 4`; at 5 it reuses the registers and waits for the LDS three times a trip), then single columns
    constexpr int U = 5;                                // (n_e = 11 is two whole trips, no single-column trip left over)
    for (; k + U <= ne; k += U) {
        double v[U][SL], p[U];
#pragma unroll
        for (int u = 0; u < U; u++) { rd(k + u, v[u]); p[u] = P[(k + u) * ps]; }
        __builtin_amdgcn_sched_barrier(0);              // (nothing moves across: the reads stay in front)
#pragma unroll
        for (int u = 0; u < U; u++) acc(p[u], v[u]);
    }
#pragma unroll 1
    for (; k < ne; k++) {
        double v[SL];
        rd(k, v);
        acc(P[k * ps], v);
    }
}

// the same with the column of Pi held in registers (16 unrolled steps, the ones beyond n_e predicated off): no LDS read for
// the coefficient, and every tile read of the pass can be in flight at once
// BRK (the descriptor path; the caller passes xopaque(ne)): the pass ends at the first k >= ne — one scalar compare per step on one
// register, where the sixteen hoisted predicates `k < ne` are sixteen spilled lane masks (two v_readlane each, every period)
// NK: the coefficients held (16; a kernel instance compiled for its n_e holds exactly n_e and passes ne = NK as a literal with
// BRK off: NK straight-line steps, no predicate and no compare)
template <int SL, int NS, bool FMA = false, bool BRK = false, int NK = 16>
__device__ __forceinline__ void xtile_mix_reg(const double *tl, const double (&pr)[NK], int ne, double *out) {
    const int ks = 64 * SL;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        if (BRK && k > 0 && k >= ne) break;
        if (BRK || k < ne) {
            double v[SL];
            if (SL == 1) v[0] = tl[(size_t)k * ks];
            else {
#pragma unroll
                for (int q = 0; q < (NS + 1) / 2; q++) { const double2 d = reinterpret_cast<const double2 *>(tl + (size_t)k * ks)[q]; v[2 * q] = d.x; v[2 * q + 1] = d.y; }
            }
#pragma unroll
            for (int q = 0; q < NS; q++) out[q] = k == 0 ? pr[k] * v[q] : (FMA ? __builtin_fma(pr[k], v[q], out[q]) : out[q] + pr[k] * v[q]);
        }
    }
}

// ---- the SLOT-MAJOR tile of k_xfwd<D, true, MAXT, true> (HANK_XFWD_TILE_SOA; hank_xlds.h: xtile_soa): [column k][slot][lane] in
// doubles. The source walk's ds_add_f64 into consecutive target rows then hit consecutive banks (8.4 cycles per wave-instruction
// against 16 at the 48-byte row stride of [lane][SL = 6]: scripts/ubench/lds_add_bench.hip), and a lane's slot is read by one
// conflict-free ds_read_b64. The functions beside xtile_store, xtile_store_n, xtile_mix and xtile_mix_reg, which every other kernel
// keeps; t and tl point at this lane's entry of column 0's (the store: of the lane's own column's) slot 0.
// (a volatile read in the LDS address space: ONE ds_read_b64 each — paired into ds_read2st64_b64 the reads take four times the LDS
// cycles, and volatile through a generic pointer is a flat load, which the counted vector-memory batch must not see)
typedef const volatile __attribute__((address_space(3))) double xlds_cvdouble;
__device__ __forceinline__ double xtile_soa_ld(const double *p) { return *(xlds_cvdouble *)p; }
template <int NS>
__device__ __forceinline__ void xtile_soa_store(double *t, const double *v) {      // v holds NS values
#pragma unroll
    for (int q = 0; q < NS; q++) t[q * XTILE_SOA_SLOT] = v[q];
}
// xtile_mix's sums, operand by operand: k ascending, the first column by itself, U columns' reads in front of their multiply-adds
template <int NS, bool FMA = false>
__device__ __forceinline__ void xtile_soa_mix(const double *tl, const double *P, int ps, int ne, double *out) {
    constexpr int ks = XTILE_SOA_SLOT * NS;
    auto rd = [&](int k, double *v) {
#pragma unroll
        for (int q = 0; q < NS; q++) v[q] = xtile_soa_ld(tl + (size_t)k * ks + q * XTILE_SOA_SLOT);
    };
    auto acc = [&](double p, const double *v) {
#pragma unroll
        for (int q = 0; q < NS; q++) out[q] = FMA ? __builtin_fma(p, v[q], out[q]) : out[q] + p * v[q];
    };
    {
        double v[NS];
        rd(0, v);
        const double p = P[0];
#pragma unroll
        for (int q = 0; q < NS; q++) out[q] = p * v[q];
    }
    int k = 1;
    constexpr int U = 5;
    for (; k + U <= ne; k += U) {
        double v[U][NS], p[U];
#pragma unroll
        for (int u = 0; u < U; u++) { rd(k + u, v[u]); p[u] = P[(k + u) * ps]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; u++) acc(p[u], v[u]);
    }
#pragma unroll 1
    for (; k < ne; k++) {
        double v[NS];
        rd(k, v);
        acc(P[k * ps], v);
    }
}
// xtile_mix_reg's sums, operand by operand
template <int NS, bool FMA = false, bool BRK = false, int NK = 16>
__device__ __forceinline__ void xtile_soa_mix_reg(const double *tl, const double (&pr)[NK], int ne, double *out) {
    constexpr int ks = XTILE_SOA_SLOT * NS;
#pragma unroll
    for (int k = 0; k < NK; k++) {
        if (BRK && k > 0 && k >= ne) break;
        if (BRK || k < ne) {
            double v[NS];
#pragma unroll
            for (int q = 0; q < NS; q++) v[q] = tl[(size_t)k * ks + q * XTILE_SOA_SLOT];
#pragma unroll
            for (int q = 0; q < NS; q++) out[q] = k == 0 ? pr[k] * v[q] : (FMA ? __builtin_fma(pr[k], v[q], out[q]) : out[q] + pr[k] * v[q]);
        }
    }
}

// Per-period inputs that are uniform over the workgroup, staged in LDS once for the whole sweep (as a per-period global load each is a
// cold round trip on the critical path). xsh[P][4]: r_t, w_t, tr_t, rho_t = 1/(1+r_t)
__device__ __forceinline__ void xstage_prices(double *xsh, const Consts &c, const double *xhh, const double *rho, int P) {
    for (int k = threadIdx.x; k < P; k += blockDim.x) {
        xsh[4 * k] = xhh[c.n_hh * k]; xsh[4 * k + 1] = xhh[c.n_hh * k + 1]; xsh[4 * k + 2] = hh_tr(c, xhh, k); xsh[4 * k + 3] = rho[k];
    }
}
// dxsh[P][3][D]: dr, dw, dtr of the D directions group x owns, out of the pass's N (columns n0.. of [P][Ntot]); a direction beyond N is zero
template <int D>
__device__ __forceinline__ void xstage_dx(double *dxsh, const Consts &c, const double *dxr, const double *dxw, const double *dxt, int Ntot, int n0, int N, int x, int P) {
    for (int k = threadIdx.x; k < P * D; k += blockDim.x) {
        const int t_ = k / D, d_ = k - t_ * D;
        const bool on = x * D + d_ < N;
        const size_t ix = (size_t)t_ * Ntot + n0 + x * D + d_;
        dxsh[(t_ * 3 + 0) * D + d_] = on ? dxr[ix] : 0.0;
        dxsh[(t_ * 3 + 1) * D + d_] = on ? dxw[ix] : 0.0;
        dxsh[(t_ * 3 + 2) * D + d_] = (on && c.n_hh > 2) ? dxt[ix] : 0.0;
    }
}

// ================================ the Float64 sweeps ==========================================
// One group (the XCD with id 0) runs them; the workgroups that landed elsewhere leave at once. They write the policy
// sequence, the distribution path and the linearisation record the tangent sweeps — of either implementation — read.
// The descriptor path: where the record's arrays start in its ONE allocation (bytes): an access is descriptor + 32-bit lane offset +
// scalar offset (array + period) instead of a 64-bit base per array — more bases than a wave has scalar registers
struct XRecOff {
    const char *rec;
    unsigned bytes;
    unsigned pol, ib, A, B, u, v, s, kc, lo, lw, ig, Dseq;
    unsigned lq;                // the packed per-source records {w, lo, flags} (k_lottery_lq), 16-byte aligned. It takes the struct's tail pad:
};                              // the arguments of every kernel that holds an XRecOff keep their places
static_assert(sizeof(XRecOff) == 64, "XRecOff: a field more moves the arguments behind it in k_xdual_back and k_xfwd");
// (x_addr_fits, the host's question whether 32-bit offsets reach every stream of a launch, is plain C++ of its own: hank_xaddr.h)

struct XBackArgs {
    Consts c;
    const double *ss_value;     // [G] terminal marginal value (BackwardIteration.jl:85)
    const double *xhh;          // [n_hh*P]
    const double *rho;          // [P] 1/(1+r_t)
    XSync *sy;
    double *st_s;               // [2][XG][G] knots (see top)
    int *err;                   // device error word of the context (knots / domain)
    Record R;                   // pol; s, kc, ib, A, B, u, v: the linearisation
};

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_xprimal_back(XBackArgs A) {
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_primal_back (hank_xlds.h), which also sizes the launch
    const Consts &c = A.c;
    const int ne = c.n_e, na = c.n_a, P = c.P, G = c.G;
    const XLdsPrimalBack L = xlds_primal_back(ne, na, P);
    double *Vsh = xlds_at<double>(xl, L.Vsh), *Pish = xlds_at<double>(xl, L.Pish), *ash = xlds_at<double>(xl, L.ash), *xsh = xlds_at<double>(xl, L.xsh);
    int *ctl = xlds_at<int>(xl, L.ctl);
    const XMember mb = xmember_join(A.sy, ctl, 1, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int a = cW * XRW + lane;
    const bool own = !syncw && lane < XRW && a < na;
    const size_t pt = (size_t)e * na + (own ? a : 0);
    for (int k = threadIdx.x; k < ne * ne; k += blockDim.x) Pish[k] = c.Pi[k];
    for (int k = threadIdx.x; k < na; k += blockDim.x) ash[k] = c.a[k];
    xstage_prices(xsh, c, A.xhh, A.rho, P);
    Consts cl = c;                                      // what egm_Y sees: the same model, grid served from LDS
    cl.a = ash;
    const double ze = c.z[e], xa = c.a[own ? a : 0];
    const size_t hs = (size_t)XG * G;                   // the other half of the ping-pong state
    double *const sS = A.st_s;
    if (!syncw) Vsh[e * 64 + lane] = own ? A.ss_value[pt] : 0.0;      // terminal value (BackwardIteration.jl:85)
    __syncthreads();
    int guess = -1;
    unsigned episode = 0;
    // sequence: X(P-1) | Y(P-1) X(P-2) | ... | Y(1) X(0) | Y(0), one group barrier after every X
    for (int i = 0; i <= P; i++) {
        if (i > 0) {
            // ---- Y half of period t (KrusellSmith.jl:66-80): bracket search in the L2-resident knots -> policy, marginal value -> LDS
            const int t = P - i, cur = (i - 1) & 1;
            double V = 0.0;
            if (own) {
                XKnots kn;
                kn.preload(sS + (size_t)cur * hs + (size_t)e * na, a, na, guess, ze);
                const YOut o = egm_Y(cl, kn, a, e, xsh[4 * t], xsh[4 * t + 1], xsh[4 * t + 2], A.err, t, guess);
                guess = o.ib;
                V = o.V;
                const size_t ro = (size_t)t * G + pt;
                A.R.pol[ro] = o.g; A.R.ib[ro] = o.ib; A.R.A[ro] = o.A; A.R.B[ro] = o.B; A.R.u[ro] = o.u; A.R.v[ro] = o.v;
            }
            if (!syncw) Vsh[e * 64 + lane] = V;
            xlds_barrier();
        }
        if (i < P) {
            // ---- X half of period tx from V_{tx+1} in LDS (KrusellSmith.jl:59-62): the knots s_tx -> state[i & 1]
            const int tx = P - 1 - i;
            if (own) {
                double E;
                xtile_mix<1, 1>(Vsh + lane, Pish + e, ne, ne, &E);
                const XPoint p = egm_X_point(c, E, xsh + 4 * tx, ze, xa, A.err, tx, e, a);      // rho = 1/(1+r_tx) once per period (k_xrho), not once per thread
                sS[(size_t)(i & 1) * hs + pt] = p.s1;
                A.R.s[(size_t)tx * G + pt] = p.s1; A.R.kc[(size_t)tx * G + pt] = p.kc;
            }
            episode++;
            xbar_arrive(!syncw);
            xbar_wait(A.sy, x, cW, Sact, episode, sync_duty);
        }
    }
}
static inline size_t x_lds_primal_back(const Consts &c) { return xlds_primal_back(c.n_e, c.n_a, c.P).bytes; }

// ---- the steady state's inner fixed point as ONE launch (hank_vfi; SteadyState.jl:132-141) ----------------------------
// value <- value_fn(value, xVals).Value until max|value' - value| < tol, on the group of XCD 0 exactly like k_xprimal_back
// (constant prices, nothing recorded). The group barrier carries the vote (xvote: max < tol over all rows <=> every member's max < tol).
struct XVfiArgs {
    Consts c;
    const double *V0;           // [G] start value
    double r, w, tr;
    double tol;
    int max_iter;
    XSync *sy;
    double *st_s;               // [2][XG][G] knots
    int *err;
    double *Vout, *pol;         // [G] the converged value and its policy
    int *iters;                 // [0] steps taken, [1] 1 = converged
    double *supnorm;            // max|value' - value| of the last step
};

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_xvfi(XVfiArgs A) {
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_vfi (hank_xlds.h), which also sizes the launch
    const Consts &c = A.c;
    const int ne = c.n_e, na = c.n_a, G = c.G;
    const XLdsVfi L = xlds_vfi(ne, na);
    double *Vsh = xlds_at<double>(xl, L.Vsh), *Pish = xlds_at<double>(xl, L.Pish), *ash = xlds_at<double>(xl, L.ash), *redsh = xlds_at<double>(xl, L.redsh);
    int *ctl = xlds_at<int>(xl, L.ctl);                 // [4] group placement, [4..5] the vote's outcome
    const XMember mb = xmember_join(A.sy, ctl, 1, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, wv = rl.wv, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int a = cW * XRW + lane;
    const bool own = !syncw && lane < XRW && a < na;
    const size_t pt = (size_t)e * na + (own ? a : 0);
    for (int k = threadIdx.x; k < ne * ne; k += blockDim.x) Pish[k] = c.Pi[k];
    for (int k = threadIdx.x; k < na; k += blockDim.x) ash[k] = c.a[k];
    Consts cl = c;
    cl.a = ash;
    const double ze = c.z[e], xa = c.a[own ? a : 0];
    const double x4[4] = {A.r, A.w, A.tr, 1.0 / (1.0 + A.r)};      // the prices and rho (same expression as egm_X / k_xrho)
    const size_t hs = (size_t)XG * G;
    double *const sS = A.st_s;
    double Vprev = own ? A.V0[pt] : 0.0, V = Vprev, pol = 0.0;
    if (!syncw) Vsh[e * 64 + lane] = Vprev;
    __syncthreads();
    int guess = -1, steps = 0, conv = 0;
    double gmax = 0.0;
    unsigned episode = 0;
    // sequence: X(V_0) | Y -> V_1, vote, X(V_1) | Y -> V_2, vote, X(V_2) | ...: step k is complete after the Y half of trip k
    for (int i = 0; i <= A.max_iter; i++) {
        double dmax = 0.0;
        if (i > 0) {
            const int cur = (i - 1) & 1;
            if (own) {
                XKnots kn;
                kn.preload(sS + (size_t)cur * hs + (size_t)e * na, a, na, guess, ze);
                const YOut o = egm_Y(cl, kn, a, e, A.r, A.w, A.tr, A.err, 0, guess);
                guess = o.ib;
                V = o.V; pol = o.g;
                dmax = fabs(V - Vprev);
                Vprev = V;
            }
            if (!syncw) Vsh[e * 64 + lane] = V;
            dmax = xwave_max_nan(dmax);
            if (lane == 0) redsh[wv] = syncw ? 0.0 : dmax;
            xlds_barrier();
        }
        // ---- X half from the value in LDS (it is discarded if the vote below ends the iteration)
        if (own) {
            double E;
            xtile_mix<1, 1>(Vsh + lane, Pish + e, ne, ne, &E);
            sS[(size_t)(i & 1) * hs + pt] = egm_X_point(c, E, x4, ze, xa, A.err, 0, e, a).s1;      // (kc is not needed)
        }
        episode++;
        xbar_arrive(!syncw);
        if (sync_duty) xvote<true>(A.sy, x, cW, Sact, episode, redsh, ne, i > 0, A.tol, xldu(reinterpret_cast<const unsigned *>(A.err)) != 0u ? 1u : 0u, ctl);
        xlds_barrier();
        if (i > 0) { steps = i; gmax = redsh[15]; }
        conv = ctl[4];
        const int stop = conv | ctl[5];
        xlds_barrier();                                     // (ctl / redsh are rewritten in the next trip)
        if (i > 0 && stop) break;
    }
    if (own) { A.Vout[pt] = V; A.pol[pt] = pol; }
    if (cW == 0 && threadIdx.x == 0) { A.iters[0] = steps; A.iters[1] = conv; *A.supnorm = gmax; }
}
static inline size_t x_lds_vfi(const Consts &c) { return xlds_vfi(c.n_e, c.n_a).bytes; }

// ================================ tangent-only sweeps at a recorded primal ===================================
// The dual sweeps above cost what the Float64 recurrence costs — and every group repeats it (bracket search, two
// roots and four divisions per point and period: ~10x the work of one partial). At a FIXED x (the whole y-iteration,
// NewtonRaphson.jl:91-111; every pass of a wide batch) the primal sweep runs ONCE (the D = 0 instances above, which
// also record the linearisation) and the partials run as pure linear recurrences: these two kernels. Same groups, same
// state exchange through the XCD's L2, same barrier; per point and period a few FMAs per direction.

// ---- the stationary distribution as ONE launch (hank_stationary_dist) ------------------------------------------------
// D <- Lambda(policy) D on the group of XCD 0 exactly like k_xprimal_fwd with ONE period's lottery record (k_lottery on the
// steady-state policy: seg, lw, clo), nothing recorded. Every `check_every` iterations each member compares its rows with
// its copy of the iterate `check_every` steps earlier (registers); the verdict rides on the group barrier as in k_xvfi.
// A member's virtual row is one of up to `members` parts of row 0: its part must move by less than tol / members, so that
// the rule is at least as strict as comparing the folded row (|sum| <= sum of |parts|).
struct XStatArgs {
    Consts c;
    Record R;                   // seg, lw, clo of the ONE lottery (period 0 of a private record)
    const double *D0;           // [G] start
    double tol;
    int max_iter, check_every;
    XSync *sy;
    double *st_D;               // [2][XG][G + 64*n_e]
    double *Dout;               // [G] the last iterate, the virtual mass folded into row 0 of its column
    int *iters;                 // [0] iterations run, [1] 1 = converged
};

template <int MAXT>
__global__ void __launch_bounds__(MAXT) k_xstat(XStatArgs A) {
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_stat (hank_xlds.h), which also sizes the launch
    const Consts &c = A.c;
    const Record &R = A.R;
    const int ne = c.n_e, na = c.n_a, G = c.G;
    const int GV = G + 64 * ne;
    const XLdsStat L = xlds_stat(ne);
    double *tile = xlds_at<double>(xl, L.tile), *redsh = xlds_at<double>(xl, L.redsh);
    int *ctl = xlds_at<int>(xl, L.ctl);                 // [4] placement, [4..5] the vote's outcome
    const XMember mb = xmember_join(A.sy, ctl, 1, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, wv = rl.wv, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int r0 = cW * XRW, r = r0 + lane;
    const bool own = !syncw && lane < XRW && r < na;
    const bool virt = !syncw && lane == 63;
    const size_t pt = (size_t)e * na + (own ? r : 0);
    const size_t slot = own ? pt : (size_t)G + (size_t)e * 64 + cW;
    double pr[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pr[k] = k < ne ? c.Pi[ne * e + k] : 0.0;
    const size_t hs = (size_t)XG * GV;
    double *const sP = A.st_D;
    double Dcur = own ? A.D0[pt] : 0.0;
    if (own || virt) sP[slot] = Dcur;
    double Dchk = Dcur;                                 // this lane's entry of the iterate check_every steps back
    // the lottery does not change: this lane's segments (as a target) and the clamped prefix of its column
    int sg0 = 0, sg1 = 0, sg2 = 0;
    if (own) { const int4 q = R.seg[pt]; sg0 = q.x; sg1 = q.y; sg2 = q.z; }
    const int clo = syncw ? 0 : min(max(R.clo[e], 0), na);
    bool anyclo = false;
    for (int k = 0; k < ne; k++) anyclo = anyclo || R.clo[k] > 0;
    const int s0 = max(sg0, 0), s2 = min(sg2, na);
    const bool need_vD = anyclo && clo == 0 && __any(own && (sg0 <= 0 && s2 > 0));
    unsigned episode = 1;
    xbar_arrive(!syncw);
    xbar_wait(A.sy, x, cW, Sact, episode, sync_duty);
    int cur = 0, it = 0, conv = 0;
    bool vnz = false;                                   // the virtual rows hold mass from the first iteration on (if any column is clamped)
    for (it = 1; it <= A.max_iter; it++) {
        const size_t hb = (size_t)cur * hs;
        double accD = 0.0;
        if (!syncw) {
            const double *Dp = sP + hb + (size_t)e * na;
            double cD = 0.0;
            if (own && r < clo) cD = xld(Dp + r);
            if (virt && clo > 0 && vnz) cD = xld(sP + hb + slot);
            double vD = 0.0;
            if (vnz && need_vD) {
                if (lane < Sact) vD = xld(sP + hb + (size_t)G + (size_t)e * 64 + lane);
                vD = xwave_sum(vD);
            }
            if (own) {
                for (int j0 = s0; j0 < s2; j0 += 4) {
                    double wj[4], Dj[4];
                    bool on[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int j = j0 + u;
                        on[u] = j < s2;
                        wj[u] = 0.0; Dj[u] = 0.0;
                        if (on[u]) { wj[u] = R.lw[(size_t)e * na + j]; Dj[u] = xld(Dp + j); }
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int j = j0 + u;
                        if (!on[u]) continue;
                        if (j == 0) Dj[u] += vD;
                        accD += (j < sg1 ? wj[u] : 1.0 - wj[u]) * Dj[u];
                    }
                }
            }
            if (clo > r0) cD = xwave_reduce63(cD);
            if (virt) accD = cD;
            tile[e * 64 + lane] = accD;
        }
        xlds_barrier();
        vnz = anyclo;
        const int nxt = cur ^ 1;
        const bool chk = (it % A.check_every) == 0 || it == A.max_iter;
        double dmax = 0.0;
        if (!syncw) {
            double Dn;
            xtile_mix_reg<1, 1>(tile + lane, pr, ne, &Dn);
            if (own || virt) sP[(size_t)nxt * hs + slot] = Dn;
            Dcur = Dn;
            if (chk) {
                if (own) dmax = fabs(Dn - Dchk);
                else if (virt) dmax = fabs(Dn - Dchk) * (double)Sact;      // one of up to Sact parts of row 0 (see top)
                Dchk = Dn;
                dmax = xwave_max_nan(dmax);
            }
        }
        if (chk && lane == 0) redsh[wv] = syncw ? 0.0 : dmax;
        cur = nxt;
        episode++;
        xbar_arrive(!syncw);
        if (sync_duty) xvote<false>(A.sy, x, cW, Sact, episode, redsh, ne, chk, A.tol, 0u, ctl);
        xlds_barrier();
        conv = ctl[4];
        const int stop = conv | ctl[5];
        xlds_barrier();
        if (stop) break;
    }
    if (it > A.max_iter) it = A.max_iter;
    // the last iterate; row 0 of a column takes the mass kept on the members' virtual rows (member order fixed, like k_xfix_D)
    if (own) {
        double v = Dcur;
        if (r == 0) for (int m = 0; m < Sact; m++) v += xld(sP + (size_t)cur * hs + (size_t)G + (size_t)e * 64 + m);
        A.Dout[pt] = v;
    }
    if (cW == 0 && threadIdx.x == 0) { A.iters[0] = it; A.iters[1] = conv; }
}
static inline size_t x_lds_stat(const Consts &c) { return xlds_stat(c.n_e).bytes; }

struct XTanBackArgs {
    Consts c;
    Record R;                   // s, kc, ib, A, B, u, v of the recorded primal
    const double *rho;          // [P] 1/(1+r_t)
    const double *xhh;          // [n_hh*P] the household inputs of the recorded primal (record diet: see diet_kc)
    const double *dxr, *dxw, *dxt;
    int Ntot, n0, N;
    XSync *sy;
    double *st_ds;              // [2][XG][G][D]
    double *dpol;               // [P][groups][G][D]
    int groups;
    const int *src;             // [P][members] lo | hi << 8: the members whose rows period t's gathers of member c read (k_xsrc_back); null = all
    int stall;                  // dev knob HANK_XFAULT=stall: member 0 of group 0 stops publishing after three periods — a wait that really times out
};

template <int D, int MAXT>
__global__ void __launch_bounds__(MAXT) k_xtan_back(XTanBackArgs A) {
    constexpr int SL = XTileT<D>::SL;
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_tan_back (hank_xlds.h), which also sizes the launch
    const Consts &c = A.c;
    const Record &R = A.R;
    const int ne = c.n_e, na = c.n_a, P = c.P, G = c.G;
    const XLdsTanBack L = xlds_tan_back(ne, P, D);
    double *tile = xlds_at<double>(xl, L.tile), *rhosh = xlds_at<double>(xl, L.rhosh), *pxsh = xlds_at<double>(xl, L.pxsh), *dxsh = xlds_at<double>(xl, L.dxsh);
    int *srcsh = xlds_at<int>(xl, L.srcsh), *ctl = xlds_at<int>(xl, L.ctl);
    const XMember mb = xmember_join(A.sy, ctl, A.groups, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    for (int k = threadIdx.x; k < P; k += blockDim.x) { rhosh[k] = A.rho[k]; pxsh[3 * k] = 1.0 + A.xhh[c.n_hh * k]; pxsh[3 * k + 1] = A.xhh[c.n_hh * k + 1]; pxsh[3 * k + 2] = hh_tr(c, A.xhh, k); }
    for (int k = threadIdx.x; k < P; k += blockDim.x) srcsh[k] = A.src ? A.src[(size_t)k * Sact + cW] : ((Sact - 1) << 8);
    xstage_dx<D>(dxsh, c, A.dxr, A.dxw, A.dxt, A.Ntot, A.n0, A.N, x, P);
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int r0 = cW * XRW, a = r0 + lane;
    const bool own = !syncw && lane < XRW && a < na;
    const size_t pt = (size_t)e * na + (own ? a : 0);
    const double ze = c.z[e], xa = c.a[own ? a : 0];
    const size_t hs = (size_t)XG * G;
    XRows<D> rows;
    rows.init(A.st_ds, 2 * hs);
    const size_t gx = (size_t)x * G;                    // this group's rows within a half
    double *const myt = tile + ((size_t)e * 64 + lane) * SL;
    {
        double z[D];
#pragma unroll
        for (int k = 0; k < D; k++) z[k] = 0.0;
        if (!syncw) xtile_store_n<SL, D>(myt, z);       // dV_T = 0 (BackwardIteration.jl:85)
    }
    __syncthreads();
    double pr[16];                                      // Pi[e, k]: this wave's coefficients of the mixing
#pragma unroll
    for (int k = 0; k < 16; k++) pr[k] = k < ne ? c.Pi[e + ne * k] : 0.0;
    // the record of the period each half is about to use, fetched one trip ahead: the loads are issued between the two
    // halves of the group barrier and land while the group meets
    int ibY = 0;
    double cA = 0.0, cB = 0.0, cu = 0.0, cv = 0.0, ck = 0.0, cs = 0.0;
    if (own) { cs = R.s[(size_t)(P - 1) * G + pt]; if (!c.diet) ck = R.kc[(size_t)(P - 1) * G + pt]; }
    // ... and, since round 5, TWO trips ahead: these are cold lines of the record (2-3 us from HBM under this load) and a trip is
    // ~4 us, but the loads used to be issued behind the publish and needed right behind the next poll — a flag round (~1 us) later.
    // A second register set (n_*) is loaded a whole trip before it is needed and handed over at the end of the trip.
    int n_ib = 0;
    double n_A = 0.0, n_B = 0.0, n_u = 0.0, n_v = 0.0, n_k = 0.0, n_s = 0.0;
    auto load_next = [&](int ty) {                      // the record of Y(ty) and X(ty - 1); ty < 0: nothing left to load
        if (own && ty >= 0) {
            const size_t ro = (size_t)ty * G + pt;
            n_ib = R.ib[ro]; n_A = R.A[ro]; n_B = R.B[ro]; n_u = R.u[ro];
            if (!c.diet) n_v = R.v[ro];
            if (ty > 0) { n_s = R.s[ro - G]; if (!c.diet) n_k = R.kc[ro - G]; }
        }
    };
    // (narrow kernels only: single tangent 1.96 -> 1.90 ms, N = 16 2.40 -> 2.35; at D = 4 the second set costs 26 registers and the
    // trip — longer there — already covers most of the latency: 3.24 -> 3.28 ms, so D = 4 keeps the one-trip form)
    constexpr bool DEEP = D <= 2;
    if constexpr (DEEP) load_next(P - 1);               // what trip 1 uses
    // sequence: X(P-1) | Y(P-1) X(P-2) | ... | Y(1) X(0) | Y(0); member c publishes episode i+1 when the stores of trip i have drained
    const int son = (x == 0 && cW < 32) ? cW : -1;     // dev stamps (make stamp)
    (void)son;
    for (int i = 0; i <= P; i++) {
        XSTAMP(0, son, i, 0);
        if (i > 0) {
            // ---- Y-tangent of period t: dg = A ds[ib] + B ds[ib+1]; dV = u dr + v ((a dr + z dw + dtr) - dg)
            const int t = P - i, cur = (i - 1) & 1;
            if (sync_duty) xpoll(A.sy, x, srcsh[t] & 255, srcsh[t] >> 8, (unsigned)i);    // the members this period gathers from have published trip i-1
            xlds_barrier();
            XSTAMP(0, son, i, 1);
            double dV[D];
#pragma unroll
            for (int k = 0; k < D; k++) dV[k] = 0.0;
            if (own) {
                double d0[D], d1[D], dg[D];
#pragma unroll
                for (int k = 0; k < D; k++) d0[k] = d1[k] = 0.0;
                if (cA != 0.0 || cB != 0.0) {
                    const size_t rb = (size_t)cur * hs + gx + (size_t)e * na;
                    rows.load(rb + ibY, d0);
                    rows.load(rb + ibY + 1, d1);
                }
                const double cvt = c.diet ? diet_v(c, cu, pxsh[3 * t]) : cv;
#pragma unroll
                for (int k = 0; k < D; k++) {
                    const double dr = dxsh[(t * 3 + 0) * D + k], dw = dxsh[(t * 3 + 1) * D + k], dtr = dxsh[(t * 3 + 2) * D + k];
                    dg[k] = cA * d0[k] + cB * d1[k];
                    dV[k] = cu * dr + cvt * ((xa * dr + (ze * dw + dtr)) - dg[k]);
                }
                xstore_row<D>(A.dpol + (((size_t)t * A.groups + x) * G + pt) * D, dg);
            }
            if (!syncw) xtile_store_n<SL, D>(myt, dV);
            XSTAMP(0, son, i, 2);
            XSTAMPV(0, son, i);
            if (sync_duty) xpoll(A.sy, x, 0, Sact - 1, (unsigned)i);      // EVERY member is done reading the half the X half overwrites
            xlds_barrier();
            XSTAMP(0, son, i, 3);
        }
        if (i < P) {
            // ---- X-tangent of period tx: ds = kc dE - rho ((z dw + dtr) + s dr)
            const int tx = P - 1 - i;
            if (own) {
                const double rho = rhosh[tx];
                const double ckt = c.diet ? diet_kc(c, cs, rho, pxsh[3 * tx], pxsh[3 * tx + 1] * ze + pxsh[3 * tx + 2], xa) : ck;
                double mx[D], ds[D];
                xtile_mix_reg<SL, D>(tile + (size_t)lane * SL, pr, ne, mx);
#pragma unroll
                for (int k = 0; k < D; k++) {
                    const double dr1 = dxsh[(tx * 3 + 0) * D + k], dw1 = dxsh[(tx * 3 + 1) * D + k], dt1 = dxsh[(tx * 3 + 2) * D + k];
                    ds[k] = ckt * mx[k] - rho * ((ze * dw1 + dt1) + cs * dr1);
                }
                rows.store((size_t)(i & 1) * hs + gx + pt, ds);
            }
            XSTAMP(0, son, i, 4);
            xbar_arrive(!syncw);                                         // this member's stores have reached L2
            XSTAMP(0, son, i, 5);
            if (sync_duty && !(A.stall && x == 0 && cW == 0 && i > 2)) xpublish(A.sy, x, cW, (unsigned)(i + 1));
            // the record the next trip needs (Y of period tx, X of period tx - 1) was requested a trip ago: hand it over, and request
            // the one after (in flight through the whole next trip)
            if constexpr (DEEP) {
                ibY = n_ib; cA = n_A; cB = n_B; cu = n_u; cv = n_v;
                if (tx > 0) { cs = n_s; ck = n_k; }
                load_next(tx - 1);
            } else if (own) {      // in flight while the others arrive
                const size_t ro = (size_t)tx * G + pt;
                ibY = R.ib[ro]; cA = R.A[ro]; cB = R.B[ro]; cu = R.u[ro];
                if (!c.diet) cv = R.v[ro];
                if (tx > 0) { cs = R.s[ro - G]; if (!c.diet) ck = R.kc[ro - G]; }
            }
        }
    }
}
static inline size_t x_lds_tan_back(const Consts &c, int D) { return xlds_tan_back(c.n_e, c.P, D).bytes; }

// ---- the backward half of a Dual pass (hank_primal_jvp) as ONE launch: value AND D partials in every group -----------
// Every group repeats the Float64 EGM step (bit for bit the same in all of them: same expressions, same order) and carries
// its own D partials through it. What that buys over k_xprimal_back followed by k_xtan_back: one chain of P periods instead
// of two, and the tangent half never reads the record — the bracket and the coefficients of a row are the registers of the
// lane that has just computed them. What it costs: the EGM step's arithmetic in all eight groups at once (it is parallel,
// not serial: every XCD would otherwise idle behind XCD 0) and the partials' gather behind the bracket search instead of
// behind a prefetched bracket. The record and the policy for every later hank_jvp at this primal are written once, the arrays shared out over the groups (all hold the same numbers). The value
// rides as one more slot of the partials' LDS tile (slot D), so one pass over the columns mixes all of them.
struct XDualBackArgs {
    XBackArgs p;                // the Float64 sweep's arguments (st_s: [2][XG][G], a slice per group here)
    const double *dxr, *dxw, *dxt;
    int Ntot, n0, N;
    double *st_ds;              // [2][XG][G][D]
    double *dpol;               // [P][groups][G][D]
    int groups;
    XRecOff ro;                 // the record's allocation and its arrays' offsets in it ...
    unsigned dpol_bytes;        // ... and this launch's dpol in bytes (x_addr_fits has checked that 32-bit offsets reach everything)
};

// NE, CRRA: instances compiled for the model's constants (hank_xspec.h: x_spec chooses, x_launch_dual_back dispatches). NE > 0 is
// the number of productivity states as a literal — the mixing is NE straight-line steps on NE coefficients; CRRA = 1 is gamma = 2
// with the record diet on — the powers are a reciprocal square root and a reciprocal of a square with no test of the exponent
// (hank_kernels.h). Both take the arms the generic instance (0, 0) takes at those constants: the same bits.
template <int D, int MAXT, int NE = 0, int CRRA = 0>
__global__ void __launch_bounds__(MAXT) k_xdual_back(XDualBackArgs B) {
    constexpr int NSL = D + 1, SL = XSlots<NSL>::SL, IV = D;
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_dual_back (hank_xlds.h), which also sizes the launch
    const XBackArgs &A = B.p;
    const Consts &c = A.c;
    const int ne = NE > 0 ? NE : c.n_e, na = c.n_a, P = c.P, G = c.G;
    const XLdsDualBack L = xlds_dual_back(ne, na, P, D);
    double *tile = xlds_at<double>(xl, L.tile), *ash = xlds_at<double>(xl, L.ash), *xsh = xlds_at<double>(xl, L.xsh), *dxsh = xlds_at<double>(xl, L.dxsh);
    int *ctl = xlds_at<int>(xl, L.ctl);
#ifdef HANK_XSTAMP
    const unsigned long long t_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const XMember mb = xmember_join(A.sy, ctl, B.groups, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    const int son = (x == 0 && cW < 32) ? cW : -1;     // dev stamps (make stamp)
    (void)son;
#ifdef HANK_XSTAMP
    if (son >= 0 && threadIdx.x == 0) g_xstamps[0][son][0][8] = t_entry;
#endif
    XSTAMP1(0, son, 9);
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int a = cW * XRW + lane;
    const bool own = !syncw && lane < XRW && a < na;
    // every group holds the same Float64 numbers: group x writes the record arrays j with j % groups == x (pol, ib, A, B, u, v, s, kc)
    const int ng = B.groups;
    const bool rc0 = 0 % ng == x, rc1 = 1 % ng == x, rc2 = 2 % ng == x, rc3 = 3 % ng == x, rc4 = 4 % ng == x, rc5 = 5 % ng == x, rc6 = 6 % ng == x, rc7 = 7 % ng == x;
    const size_t pt = (size_t)e * na + (own ? a : 0);
    for (int k = threadIdx.x; k < na; k += blockDim.x) ash[k] = c.a[k];
    xstage_prices(xsh, c, A.xhh, A.rho, P);
    xstage_dx<D>(dxsh, c, B.dxr, B.dxw, B.dxt, B.Ntot, B.n0, B.N, x, P);
    Consts cl = c;
    cl.a = ash;
    const double ze = c.z[e], xa = c.a[own ? a : 0];
    const size_t hs = (size_t)XG * G;
    double *const sS = A.st_s;
    XRows<D> rows;
    rows.init_buf(B.st_ds, 2 * XG * G);
    // Every stream goes through a buffer descriptor (see XRecOff): four descriptors (record, dpol, knots, partials) instead of a
    // dozen 64-bit bases; this lane's row as ONE loop-invariant
    // element index (every array's lane offset is that times the element size); the writer flags as one mask in one scalar register
    const __amdgpu_buffer_rsrc_t rrec = buf_rsrc(B.ro.rec, B.ro.bytes), rdp = buf_rsrc(B.dpol, B.dpol_bytes), rkn = buf_rsrc(sS, (unsigned)(2 * hs * 8));
    const int ipt = (int)pt, igx = x * G, ihs = XG * G;
    const int rcm0 = __builtin_amdgcn_readfirstlane((rc0 ? 1 : 0) | (rc1 ? 2 : 0) | (rc2 ? 4 : 0) | (rc3 ? 8 : 0) | (rc4 ? 16 : 0) | (rc5 ? 32 : 0) | (rc6 ? 64 : 0) | (rc7 ? 128 : 0));
    double *const myt = tile + ((size_t)e * 64 + lane) * SL;
    if (!syncw) {
        double z[NSL];
#pragma unroll
        for (int k = 0; k < D; k++) z[k] = 0.0;         // dV_T = 0, V_T = the terminal marginal value (BackwardIteration.jl:85)
        z[IV] = own ? A.ss_value[pt] : 0.0;
        xtile_store_n<SL, NSL>(myt, z);
    }
    __syncthreads();
    constexpr int NK = NE > 0 ? NE : 16;
    double pr[NK];                                      // Pi[e, k]: this wave's coefficients of the mixing, in registers (1.94 -> 1.87 ms at
#pragma unroll                                          // N=32 against LDS reads; the kernel sits at 168 VGPRs = 3 waves per SIMD)
    for (int k = 0; k < NK; k++) pr[k] = k < ne ? c.Pi[e + ne * k] : 0.0;
    int guess = -1;
    unsigned episode = 0;
    XSTAMP1(0, son, 10);
    // sequence: X(P-1) | Y(P-1) X(P-2) | ... | Y(1) X(0) | Y(0), one group barrier after every X (as k_xprimal_back)
    for (int i = 0; i <= P; i++) {
        XSTAMP(0, son, i, 0);
        if (i > 0) {
            const int t = P - i, cur = (i - 1) & 1;
            double tv[NSL];
#pragma unroll
            for (int k = 0; k < NSL; k++) tv[k] = 0.0;
            if (own) {
                XKnotsT<true> kn;
                const int icb = cur * ihs + igx + e * na;          // this column in the state half being read (elements; wave-uniform)
                kn.preload(rkn, icb * 8, a, na, guess, ze);
                // the partials' rows at the bracket of the period before, in the same batch of loads as the knots: the bracket
                // rarely moves by more than a knot per period, and behind the search every gather is a round trip of its own
                const int q = guess < 0 ? 0 : (guess < na - 1 ? guess : na - 2);
                double w0[D], w1[D];
                rows.load_vs(q, icb, w0); rows.load_vs(q + 1, icb, w1);
                const YOut o = egm_Y<CRRA>(cl, kn, a, e, xsh[4 * t], xsh[4 * t + 1], xsh[4 * t + 2], A.err, t, guess);
                guess = o.ib;
                tv[IV] = o.V;
                XSTAMP(0, son, i, 1);
                // Y-tangent (k_xtan_back's expressions; the coefficients are this lane's own)
                double d0[D], d1[D], dg[D];
#pragma unroll
                for (int k = 0; k < D; k++) d0[k] = d1[k] = 0.0;
                if (o.A != 0.0 || o.B != 0.0) {
                    if (o.ib == q) {
#pragma unroll
                        for (int k = 0; k < D; k++) { d0[k] = w0[k]; d1[k] = w1[k]; }
                    } else if (o.ib == q + 1) {
#pragma unroll
                        for (int k = 0; k < D; k++) d0[k] = w1[k];
                        rows.load_vs(o.ib + 1, icb, d1);
                    } else if (o.ib == q - 1) {
#pragma unroll
                        for (int k = 0; k < D; k++) d1[k] = w0[k];
                        rows.load_vs(o.ib, icb, d0);
                    } else {
                        rows.load_vs(o.ib, icb, d0); rows.load_vs(o.ib + 1, icb, d1);
                    }
                }
#pragma unroll
                for (int k = 0; k < D; k++) {
                    const double dr = dxsh[(t * 3 + 0) * D + k], dw = dxsh[(t * 3 + 1) * D + k], dtr = dxsh[(t * 3 + 2) * D + k];
                    dg[k] = o.A * d0[k] + o.B * d1[k];
                    tv[k] = o.u * dr + o.v * ((xa * dr + (ze * dw + dtr)) - dg[k]);
                }
                xstore_row_buf<D>(rdp, ipt * (8 * D), (int)((unsigned)((t * B.groups + x) * G) * (unsigned)(8 * D)), dg);
                const int tg = t * G, rcm = xopaque(rcm0);
                if (rcm & 1) buf_st64<0>(o.g, rrec, ipt * 8, (int)(B.ro.pol + (unsigned)tg * 8u));
                if (rcm & 2) buf_st32<0>(o.ib, rrec, ipt * 4, (int)(B.ro.ib + (unsigned)tg * 4u));
                if (rcm & 4) buf_st64<0>(o.A, rrec, ipt * 8, (int)(B.ro.A + (unsigned)tg * 8u));
                if (rcm & 8) buf_st64<0>(o.B, rrec, ipt * 8, (int)(B.ro.B + (unsigned)tg * 8u));
                if (rcm & 16) buf_st64<0>(o.u, rrec, ipt * 8, (int)(B.ro.u + (unsigned)tg * 8u));
                if (rcm & 32) buf_st64<0>(o.v, rrec, ipt * 8, (int)(B.ro.v + (unsigned)tg * 8u));
            }
            if (!syncw) xtile_store_n<SL, NSL>(myt, tv);
            XSTAMP(0, son, i, 2);
            XSTAMPV(0, son, i);
            xlds_barrier();
            XSTAMP(0, son, i, 3);
        }
        if (i < P) {
            const int tx = P - 1 - i;
            if (own) {
                double mx[NSL];
                // (next to the generic powers' arms, 11 columns of D = 4 partials as straight-line code spill 37 VGPRs: that one instance
                // keeps the step-by-step form on its 11 coefficients)
                constexpr bool STEPS = CRRA == 0 && NE * ((NSL + 1) / 2) > 24;
                if constexpr (NE > 0 && STEPS) xtile_mix_reg<SL, NSL, false, true, NK>(tile + (size_t)lane * SL, pr, xopaque(NE), mx);
                else if constexpr (NE > 0) xtile_mix_reg<SL, NSL, false, false, NK>(tile + (size_t)lane * SL, pr, NE, mx);
                else xtile_mix_reg<SL, NSL, false, true>(tile + (size_t)lane * SL, pr, xopaque(ne), mx);
                const XPoint p = egm_X_point<CRRA>(c, mx[IV], xsh + 4 * tx, ze, xa, A.err, tx, e, a);
                const double s1 = p.s1, kc = p.kc, rho = xsh[4 * tx + 3];
                double ds[D];
#pragma unroll
                for (int k = 0; k < D; k++) {
                    const double dr1 = dxsh[(tx * 3 + 0) * D + k], dw1 = dxsh[(tx * 3 + 1) * D + k], dt1 = dxsh[(tx * 3 + 2) * D + k];
                    ds[k] = kc * mx[k] - rho * ((ze * dw1 + dt1) + s1 * dr1);
                }
                const int ihb = (i & 1) * ihs + igx, rcm = xopaque(rcm0);
                buf_st64<0>(s1, rkn, ipt * 8, ihb * 8);
                rows.store_vs(ipt, ihb, ds);
                if (rcm & 64) buf_st64<0>(s1, rrec, ipt * 8, (int)(B.ro.s + (unsigned)(tx * G) * 8u));
                if (rcm & 128) buf_st64<0>(kc, rrec, ipt * 8, (int)(B.ro.kc + (unsigned)(tx * G) * 8u));
            }
            episode++;
            XSTAMP(0, son, i, 4);
            xbar_arrive(!syncw);
            XSTAMP(0, son, i, 5);
            xbar_wait(A.sy, x, cW, Sact, episode, sync_duty);
        }
    }
    XSTAMP1(0, son, 11);
}
static inline size_t x_lds_dual_back(const Consts &c, int D) { return xlds_dual_back(c.n_e, c.n_a, c.P, D).bytes; }

// ================================ forward sweeps, source-stationary (round 4) ========================================
// ONE kernel for the three forward recurrences (ForwardIteration.jl:297-308 and its partials):
//   k_xfwd<0, true>  the Float64 distribution sweep: group 0 only, writes D_1..D_P, {w, ig D} and the aggregate
//   k_xfwd<D, false> D partials per group at a recorded primal
//   k_xfwd<D, true>  value AND D partials per group (the forward half of the Dual pass, hank_primal_jvp): every group carries
//                    D_t itself — one more slot of the same linear step, no pow, no search — and group 0 writes D_t. The
//                    per-source record {w, ig D} is NOT written here: nothing of a Dual pass reads it, and it is a pure function
//                    of what the pass leaves behind (k_xlwg_build, before the first tangent sweep at this record)
// A member's period in the target-stationary form of rounds 2-3 was a gather loop per target row: 2-8 sources on one row,
// three at a time, each trip a dependent L2 round trip, every source row fetched by both of its targets, and the workgroup
// waited for its slowest wave. Here the SOURCES are walked: 64 source rows per instruction, each source's two lottery parts
// added into the LDS tile of its target rows (ds_add_f64). The walk is cut into WORK UNITS in advance (k_xunits_fwd, once per
// recorded lottery): a unit is a run of <= 64 consecutive sources of one column that feeds a run of consecutive target rows
// of the member; a source on the seam between two units is walked by both, each adding only the part that lands in its own
// target run — so every tile entry is written by exactly one unit, by one wave, in program order: the sum is reproducible
// bit for bit whichever wave a unit is dealt to. Units are dealt round-robin to the member's waves, two per wave in straight-
// line code (both in flight together; the rare member with more units loops): the wave of a column whose policy is flat — up
// to 216 sources on 63 targets at 2000x11 — no longer holds the whole group back (stamps, DESIGN.md section 4: 3.2 us behind).
// The mass kept on the members' virtual rows travels as extra lanes of the unit that walks source row 0 of an open column
// (same lottery record, the members' virtual rows as state rows): no special sums. The mass point itself needs no load at
// all: a member's clamped rows and its virtual row are its own rows of the previous period — its own registers.
constexpr int XUCAP = 64;       // work units per member and period (k_xunits_fwd reports an overflow; the host then uses the launches)
struct XSweepFwdArgs {
    Consts c;
    Record R;                   // pol, lo, lw, ig (k_lottery); !VAL: lwg, Dseq of the recorded primal; VAL: group 0 writes Dseq (and, D = 0, lwg)
    XSync *sy;
    double *st;                 // [2][XG][n_e*members*64][SP] the ping-pong state
    const double *D0;           // VAL: [G] initial distribution (ForwardIteration.jl:293)
    const double *dpol;         // D > 0: [P][groups][G][D]
    int groups;
    double *Dvirt;              // VAL: [P][n_e][64] the mass kept on the virtual rows (k_xfix_D)
    double *aggpart;            // VAL: [P][members][2]
    double *daggpart;           // D > 0: [P][members][2*XG*D]
    const int *src;             // [P][members] lo | hi << 8 | (some column clamped) << 16 | (member 0 records row 0's full mass) << 17 | units << 18
    const int *overflow;        // k_xunits_fwd's flag: a member's walk did not fit XUCAP units — nothing is computed from a truncated list
    const int2 *units;          // [P][members][XUCAP] {e | ja << 4 | cnt << 16, ta | tb << 8 | nv << 16}
    int all_members;            // dev knob: every period waits for every member
    XRecOff ro;                 // VAL, D > 0: the record's allocation and its arrays' offsets in it ...
    unsigned dpol_bytes;        // ... and this launch's dpol in bytes (x_addr_fits has checked that 32-bit offsets reach everything). The work units
                                // keep their POINTER and take a 32-bit scalar index: a unit's address is wave-uniform, a third buffer resource only added spills
    unsigned iga;               // LQ: the grid's inverse gaps [n_a] in the record's allocation (bytes; k_iga_build). In the struct's tail pad, like XRecOff::lq
};

// LQ (VAL and D > 0 only; HANK_XFWD_LQ): a source's lo, w and "ig is zero" come as ONE 16-byte load of the packed record, ig itself
// from the grid's inverse gaps in LDS (xlds_fwd_lq) — two vector-memory instructions per unit less on the one path the mix phase
// queues on. Without the knob the kernel has no fourth parameter: its instances are, name and code, what they were.
#if HANK_XFWD_LQ
template <int D, bool VAL, int MAXT, bool LQ = false>
#else
template <int D, bool VAL, int MAXT>
#endif
__global__ void __launch_bounds__(MAXT) k_xfwd(XSweepFwdArgs A) {
#pragma clang fp contract(fast)                         // (round 5) fused multiply-adds in this kernel (the mixing: xtile_mix<.., true>)
#if !HANK_XFWD_LQ
    constexpr bool LQ = false;
#endif
    constexpr int NSL = D + (VAL ? 1 : 0);              // live slots: the D partials, then the value
    constexpr int SP = XSlots<NSL>::SP, SL = XSlots<NSL>::SL;
    constexpr int IV = D;                               // the value's slot
    constexpr int DD = D > 0 ? D : 1;
    constexpr bool PIREG = NSL < 4;                     // the mixing's coefficients in registers
    constexpr bool XB = VAL && D > 0;                   // the Dual pass: streams through buffer descriptors (see XRecOff)
    constexpr bool EARLYB = XB && HANK_XFWD_EARLY_BATCH != 0;       // ... and issues the unit batch in front of the second barrier
    static_assert(!LQ || XB, "the packed record is read through the record's descriptor");
    // SOA (HANK_XFWD_TILE_SOA): this instance's tile is slot-major, [column][slot][lane] (xtile_soa_at, hank_xlds.h); every other
    // instance keeps [column][lane][SL]. The strides, in doubles, of a target row, a slot and a column of the tile:
    // (without the knob the text is the parent's, token by token: the register allocation of several instances follows it)
#if HANK_XFWD_TILE_SOA
    constexpr bool SOA = LQ;
    constexpr int TCS = SOA ? XTILE_SOA_SLOT * NSL : 64 * SL;
    static_assert(NSL <= SL, "the slot-major tile lies inside the tile piece");
#define XT_COL(c) (SOA ? tile + (size_t)(c) * (XTILE_SOA_SLOT * NSL) : tile + (size_t)(c) * 64 * SL)
#define XT_ROW(p, r) (SOA ? (p) + (size_t)(r) : (p) + (size_t)(r) * SL)
#define XT_SLOT(p, k) (SOA ? (p) + (k) * XTILE_SOA_SLOT : (p) + (k))
#else
#define XT_COL(c) (tile + (size_t)(c) * 64 * SL)
#define XT_ROW(p, r) ((p) + (size_t)(r) * SL)
#define XT_SLOT(p, k) ((p) + (k))
#endif
    extern __shared__ __attribute__((aligned(16))) double xl[];      // laid out by xlds_fwd (hank_xlds.h), which also sizes the launch
    const Consts &c = A.c;
    const Record &R = A.R;
    const int ne = c.n_e, na = c.n_a, P = c.P, G = c.G;
    const XLdsFwd L = xlds_fwd(ne, P, D, VAL);
    double *tile = xlds_at<double>(xl, L.tile), *Pish = xlds_at<double>(xl, L.Pish), *aggsh = xlds_at<double>(xl, L.aggsh);      // [ne][64][SL]; [ne*ne] (read when !PIREG); [ne][64][NAP]:
    // (round 5) the aggregate's terms of a period, per lane: the column waves leave them here and the SYNC wave — idle between its
    // polls — sums them over the columns and the lanes one period later. As eleven waves' own reductions they were 105 of the 562
    // VALU instructions a wave issues per period, three waves deep on a SIMD.
    // Two aggregates per slot (see dist_step_body): the policy-weighted one and the wealth-grid-weighted one. ONE buffer is enough:
    // the sync wave reads it between the period's first barrier and its own all-member poll, which stands in front of the barrier
    // the column waves must pass before they write the next period's terms.
    constexpr int NAP = 2 * NSL;                        // terms per lane: NSL of the first aggregate, NSL of the second
    int *closh = xlds_at<int>(xl, L.closh), *srcsh = xlds_at<int>(xl, L.srcsh), *ctl = xlds_at<int>(xl, L.ctl);      // [P][ne] the clamped-prefix lengths, [P]
    double *igash = nullptr;                            // LQ: [na] the grid's inverse gaps, between srcsh and ctl (xlds_fwd_lq: the other pieces are xlds_fwd's)
    if constexpr (LQ) { const XLdsFwdLq Q = xlds_fwd_lq(ne, na, P, D); igash = xlds_at<double>(xl, Q.iga); ctl = xlds_at<int>(xl, Q.ctl); }
    (void)igash;
    if (*A.overflow) return;                            // (every workgroup of the launch reads the same word: written by a kernel that ran before it)
    const XMember mb = xmember_join(A.sy, ctl, A.groups, na);
    if (!mb.on) return;
    const int x = mb.x, cW = mb.c, Sact = mb.Sact;
    // every group carries the same D_t: group 0 writes D_t, the virtual rows' mass and the aggregate. The Float64 sweep (D = 0,
    // one group) also writes the per-source record {w, ig D_{t-1}} — whose row 0 needs every member's virtual row, i.e. member 0
    // waits for everybody; the Dual pass (D >= 1) leaves that record to k_xlwg_build: its two own-row loads were dead in seven
    // groups of eight, and the all-member wait of its row 0 sat in the period's latency chain
    constexpr bool RECL = VAL && D == 0;
    const bool recD = VAL && x == 0, recL = RECL && x == 1 % A.groups;       // (one group: group 0)
    for (int k = threadIdx.x; k < ne * ne; k += blockDim.x) Pish[k] = c.Pi[k];
    for (int k = threadIdx.x; k < P * ne; k += blockDim.x) closh[k] = R.clo[k];
    if constexpr (LQ) { for (int k = threadIdx.x; k < na; k += blockDim.x) igash[k] = reinterpret_cast<const double *>(A.ro.rec + A.iga)[k]; }
    for (int k = threadIdx.x; k < P; k += blockDim.x) {
        int w = A.src[(size_t)k * Sact + cW];
        if (A.all_members || (recL && ((w >> 17) & 1))) w = (w & ~0xffff) | ((Sact - 1) << 8);
        srcsh[k] = w;
    }
    const XRoles rl = xroles(ne);
    const int lane = rl.lane, wv = rl.wv, e = rl.e; const bool syncw = rl.syncw, sync_duty = rl.sync_duty;
    const int r0 = cW * XRW, r = r0 + lane;
    const bool own = !syncw && lane < XRW && r < na;
    const bool virt = !syncw && lane == 63;             // this wave's virtual row: part of the mass point (row 0) kept by this member
    const bool live = own || virt;
    const size_t pt = (size_t)e * na + (own ? r : 0);
    const double xar = c.a[own ? r : 0];                // this row's grid point (a virtual row is a part of row 0)
    // state layout [e][member][64][SP]: a member's 63 rows and its virtual row (slot 63) are ONE line-aligned block
    const size_t GM = (size_t)ne * Sact * 64;
    const size_t gx = (size_t)x * GM;
    const size_t slot = gx + ((size_t)e * Sact + cW) * 64 + lane;
    const size_t hs = (size_t)XG * GM;
    double pr[16];                                      // Pi[k, e] as this wave's mixing uses it
#pragma unroll
    for (int k = 0; k < 16; k++) pr[k] = (PIREG && k < ne) ? c.Pi[ne * e + k] : 0.0;
    XRows<SP> rows;
    // (XB: sizes and offsets in 32-bit integers from scalar sources. The 64-bit product GM above is computed by the vector unit, and a
    // descriptor or a scalar offset derived from it sits in vector registers: every state access then runs inside a loop that reads
    // the descriptor back lane by lane)
    const int iGM = ne * Sact * 64;
    if constexpr (XB) rows.init_buf(A.st, 2 * XG * iGM); else rows.init(A.st, 2 * hs);
    // XB: three descriptors (record, dpol, state) instead of a 64-bit base per array; the work units keep their pointer (see unit_ld). A lane's offset is an element index
    // times the element size — this row's (ipt, loop-invariant) or a unit's source row (once per unit) — and the array, the period
    // and the column go into the instruction's scalar offset
    __amdgpu_buffer_rsrc_t rrec, rdp;
    if constexpr (XB) { rrec = buf_rsrc(A.ro.rec, A.ro.bytes); rdp = buf_rsrc(A.dpol, A.dpol_bytes); }
    const int ipt = e * na + (own ? r : 0), igx = x * iGM, ihs = XG * iGM, islot = (e * Sact + cW) * 64;
#if HANK_XFWD_TILE_SOA
    double *const myt = SOA ? tile + (size_t)e * TCS + lane : tile + ((size_t)e * 64 + lane) * SL;      // this lane's entry of its column (SOA: its slot 0)
#else
    double *const myt = tile + ((size_t)e * 64 + lane) * SL;
#endif
    double mxp[NSL];                                    // this lane's row of the previous period (the state it stored)
#pragma unroll
    for (int k = 0; k < NSL; k++) mxp[k] = 0.0;
    if constexpr (VAL) { if (own) mxp[IV] = A.D0[pt]; }
    {
        double sv[SP];
#pragma unroll
        for (int k = 0; k < SP; k++) sv[k] = k < NSL ? mxp[k] : 0.0;
        if constexpr (XB) { if (live) rows.store_vs(lane, igx + islot, sv); }
        else if (live) rows.store(slot, sv);                 // D_0; it carries no partials
    }
    // this lane's own-row record of the period about to be processed (what the aggregate and the record need). At a recorded
    // primal the term dpol_t D_t of the aggregate is taken where the policy partials are loaded anyway — at the SOURCE rows —
    // and a row's own partials only count where the row is clamped (not walked as a source: its partial is zero except on a
    // knot tie). Branch-free on purpose: these loads are part of the counted batch behind the period's stores (see XFWD_NLD).
    double polr = 0.0, Dr = 0.0, lwr = 0.0, igr = 0.0, dpr[DD];
#pragma unroll
    for (int k = 0; k < DD; k++) dpr[k] = 0.0;
    auto prefetch = [&](int t) {
        if constexpr (XB) {
            polr = buf_ld64<0>(rrec, ipt * 8, (int)(A.ro.pol + (unsigned)(t * G) * 8u));
            xload_row_buf<DD>(rdp, ipt * (8 * D), (int)((unsigned)((t * A.groups + x) * G) * (unsigned)(8 * D)), dpr);
            return;
        }
        const size_t ro = (size_t)t * G + (size_t)e * na + (own ? r : 0);       // (a virtual row carries row 0's policy and partials)
        polr = R.pol[ro];
        if constexpr (D > 0) xload_row_plain<DD>(A.dpol + ((size_t)t * A.groups + x) * (size_t)G * D + ((size_t)e * na + (own ? r : 0)) * D, dpr);
        if constexpr (RECL) { lwr = R.lw[ro]; igr = R.ig[ro]; }
        else if constexpr (!VAL && D > 0) Dr = R.Dseq[ro + G];      // D_t[r] (row 0 includes what the primal kept on its virtual rows)
    };
    // ---- the two work units of this wave, register sets 0 and 1: per lane a source's lottery record {lo, w, ig D_{t-1} | ig},
    // its policy partials and (at a recorded primal) D_t of its row; then its state row
    int2 ud[2];                                         // the units' descriptors (wave-uniform)
    int qlo[2];
    double qw[2], qg[2], qdn[2], qdp[2][DD], dd[2][SP];
    bool qon[2], qvl[2];
    // qrow (the descriptor path): a unit's state row within its column, set by load_rec — a period before the
    // state is read, in the mixing phase's shadow — so that nothing but scalar setup stands between the barrier behind the source
    // poll and the state loads. A lane that is off reads row 0 of the unit's column (in range; process_* gate on qon / doL / doH)
    int qrow[2] = {0, 0};
    int qfl[2] = {1, 1};                                // LQ: the packed record's flags (bit 0: ig is zero — the source is clamped at either end of the grid)
    (void)qfl;
    const int2 *const ubase = A.units + (size_t)cW * XUCAP;       // (the pointer path; XB: unit_ld)
    auto unit_ld = [&](int tu, int u) -> int2 {         // XB: a descriptor's address is wave-uniform — a scalar base and a 32-bit scalar index, no lane arithmetic
        return A.units[(unsigned)((tu * Sact + cW) * XUCAP + u)];
    };
    auto unit_desc = [&](int t, int u) -> int2 {        // unit u of this member in period t (u wave-uniform): broadcast load -> scalar registers
        int2 q;
        if constexpr (XB) q = unit_ld(t, u); else q = ubase[(size_t)t * Sact * XUCAP + u];
        return make_int2(__builtin_amdgcn_readfirstlane(q.x), __builtin_amdgcn_readfirstlane(q.y));
    };
    // (branch-free: every lane loads — a lane beyond the unit's sources the unit's last row, an empty unit row 0 of column 0 — and
    // qon / qvl say what counts)
    // FLAT_TR (HANK_XFWD_FLAT_TR): a FLAT unit — more than XFLAT_NUM / XFLAT_DEN sources per row of its target run [ta, tb), asked of the
    // descriptor in scalar code — deals a trip's 64 sources four apart inside each 16-lane group: lane g * 16 + j walks source 4 j + g.
    // ds_add_f64 is served in 16-lane groups and lanes of a group on ONE address are added one after the other (12 cycles per wave-
    // instruction and extra lane: scripts/ubench/lds_add_bench.hip); consecutive sources of a flat unit share their target rows, sources
    // four apart mostly do not. Every kernel that walks the units takes the same map (this lambda): the lanes' order at a tile entry is
    // the order of its terms, and the value's bits are the same whichever k_xfwd carries it.
#if HANK_XFWD_FLAT_TR
    const int ltr = (lane & 15) * 4 + (lane >> 4);
    auto unit_flat = [&](int2 d) -> bool {              // (wave-uniform; an empty unit is not flat)
        const int cnt = (d.x >> 16) & 0xfff, ta = d.y & 0xff, tb = (d.y >> 8) & 0xff;
        return XFLAT_DEN * cnt > XFLAT_NUM * (tb - ta);
    };
    auto unit_lane = [&](int2 d) -> int { return unit_flat(d) ? ltr : lane; };      // this lane's source within a trip of unit d
#define XUNIT_LANE(d) unit_lane(d)
#else
#define XUNIT_LANE(d) lane
#endif
    auto load_rec = [&](auto U, int t, int2 d, int i0) {
        constexpr int u = decltype(U)::value;
        const int ue = d.x & 15, ja = (d.x >> 4) & 0xfff, cnt = (d.x >> 16) & 0xfff, nv = (d.y >> 16) & 0xff;
        const int i = i0 + XUNIT_LANE(d);
        const bool real = i < cnt;
        qvl[u] = !real && i < cnt + nv;                 // a member's virtual row riding on source row 0's record
        qon[u] = real || qvl[u];
        const size_t cb = (size_t)t * G + (size_t)ue * na;      // (the pointer path's column base; XB: icb. It stays in front of j: swapped, every k_xfwd gets another register allocation)
        const int j = real ? ja + i : (qvl[u] ? 0 : min(ja + max(cnt - 1, 0), na - 1));
        if constexpr (XB) {
            const int icb = t * G + ue * na;            // the unit's column in period t (elements; wave-uniform)
            qrow[u] = qvl[u] ? (i - cnt) * 64 + 63 : (real ? (j / XRW) * 64 + j % XRW : 0);
            if constexpr (LQ) {                         // {w, lo, flags} in one instruction; qg[u]: set_g, where the wave is idle and the record has landed
                const xv4u q = __builtin_amdgcn_raw_buffer_load_b128(rrec, j * 16, (int)(A.ro.lq + (unsigned)icb * 16u), 0);
                qw[u] = __hiloint2double((int)q.y, (int)q.x); qlo[u] = (int)q.z; qfl[u] = (int)q.w;
            } else {
                qlo[u] = buf_ld32<0>(rrec, j * 4, (int)(A.ro.lo + (unsigned)icb * 4u));
                qw[u] = buf_ld64<0>(rrec, j * 8, (int)(A.ro.lw + (unsigned)icb * 8u));
                qg[u] = buf_ld64<0>(rrec, j * 8, (int)(A.ro.ig + (unsigned)icb * 8u));
            }
            xload_row_buf<DD>(rdp, j * (8 * D), (int)((unsigned)((t * A.groups + x) * G + ue * na) * (unsigned)(8 * D)), qdp[u]);
            return;
        }
        qlo[u] = R.lo[cb + j];
        if constexpr (VAL) qw[u] = R.lw[cb + j];        // (D = 0: ig only weights the policy partials)
        else { const double2 wg = R.lwg[cb + j]; qw[u] = wg.x; qg[u] = wg.y; if constexpr (D > 0) qdn[u] = R.Dseq[cb + G + j]; }
        if constexpr (D > 0) xload_row_plain<DD>(A.dpol + (((size_t)t * A.groups + x) * G + (size_t)ue * na + j) * D, qdp[u]);
    };
    auto load_state = [&](auto U, size_t hb, int hc, int2 d, int i0) {       // hc: the state half being read (hb = hc * hs)
        constexpr int u = decltype(U)::value;
        const int ue = d.x & 15, ja = (d.x >> 4) & 0xfff, cnt = (d.x >> 16) & 0xfff;
#pragma unroll
        for (int k = 0; k < SP; k++) dd[u][k] = 0.0;
        const int i = i0 + XUNIT_LANE(d), j = ja + i;    // (load_rec's source)
        if constexpr (XB) {
            rows.load_vs(qrow[u], hc * ihs + igx + ue * Sact * 64, dd[u]);        // unconditional: the compiler counts the loads in flight
            return;
        }
        const size_t row = qvl[u] ? ((size_t)ue * Sact + (i - cnt)) * 64 + 63 : ((size_t)ue * Sact + j / XRW) * 64 + j % XRW;
        if (qon[u]) rows.load(hb + gx + row, dd[u]);
    };
    // LQ: a unit's ig from the table — the record's own bits: k_iga_build's expression is lottery_body's, and a clamped source's
    // ig is +0. The bracket is one the lottery wrote, lo <= na - 2 (the index is held in the table all the same)
    auto set_g = [&](auto U) {
        constexpr int u = decltype(U)::value;
        if constexpr (LQ) { const double g = igash[min((unsigned)qlo[u], (unsigned)(na - 1))]; qg[u] = (qfl[u] & 1) ? 0.0 : g; }
    };
    const std::integral_constant<int, 0> I0;
    const std::integral_constant<int, 1> I1;
    int2 udn[2];                                        // the descriptors of the period after next, on their way (loaded a period ahead: cold lines)
    bool udv[2] = {false, false};                       // ... and whether this wave has such a unit at all
    udn[0] = udn[1] = make_int2(0, 0);
    auto request_units = [&](int t) {                   // this wave's two units of period t (branch-free: an index that exists is loaded anyway)
        const int tc = min(t, P - 1);
        int nu = (srcsh[tc] >> 18) & 0xff;
        nu = t < P ? nu : 0;
        udv[0] = wv < nu; udv[1] = wv + ne < nu;
        if constexpr (XB) { udn[0] = unit_ld(tc, udv[0] ? wv : 0); udn[1] = unit_ld(tc, udv[1] ? wv + ne : 0); }
        else {
            udn[0] = ubase[(size_t)tc * Sact * XUCAP + (udv[0] ? wv : 0)];
            udn[1] = ubase[(size_t)tc * Sact * XUCAP + (udv[1] ? wv + ne : 0)];
        }
    };
    auto take_units = [&]() {
        ud[0] = udv[0] ? make_int2(__builtin_amdgcn_readfirstlane(udn[0].x), __builtin_amdgcn_readfirstlane(udn[0].y)) : make_int2(0, 0);
        ud[1] = udv[1] ? make_int2(__builtin_amdgcn_readfirstlane(udn[1].x), __builtin_amdgcn_readfirstlane(udn[1].y)) : make_int2(0, 0);
    };
    // The loads of the NEXT period — its two units' records, the own-row record, the descriptors of the period after — are cold
    // lines of the record (2.4 us from HBM under this load) and vector-memory waits are in order. Round 5 splits them in two:
    //  * the UNIT batch (the two units' records, the descriptors of the period after) is issued BEFORE the mixing, as soon as the
    //    tile is complete: the stamps of round 4's single batch showed where its time went — not in latency but in ISSUE: twelve
    //    waves x 17 loads through one CU's vector-memory path took 2.4 us, every member's flag waited for the slowest wave's last
    //    load to be accepted, and the mixing (2 us of LDS and arithmetic that needs no memory path) sat in front of it, idle on
    //    that path. Issued here they are accepted while the waves mix, and have landed when the period's stores are drained;
    //  * the OWN-ROW batch (policy, policy partials, and — D = 0 — lottery weights of this lane's row: their registers are in use until the
    //    aggregate) stays behind the period's last store as a batch of exactly XFWD_NLD instructions, every one unconditional, and
    //    the drain waits with vmcnt(XFWD_NLD): everything older — the stores, and the unit batch — has completed, the own-row batch
    //    stays in flight through the publish, the next poll and the next state loads (tests/test_isa_hazards.py counts the
    //    instructions between the two markers in the ISA against the immediate).
    constexpr int DPI = D == 0 ? 0 : (D <= 2 ? 1 : D / 2);                 // load instructions per row of policy partials
    constexpr int XFWD_NLD = 1 + DPI + (RECL ? 2 : ((!VAL && D > 0) ? 1 : 0));    // policy, its partials; lw and ig (the record's writer), or D_t (at a recorded primal)
    auto next_units_loads = [&](int t) {                // t: the period being processed (ud holds the NEXT period's units by now)
        const int t1 = min(t + 1, P - 1);
        load_rec(I0, t1, ud[0], 0);
        load_rec(I1, t1, ud[1], 0);
        request_units(t + 2);
    };
    xbar_arrive(!syncw);                                // the initial state has reached L2: episode 1
    if (sync_duty) xpublish(A.sy, x, cW, 1u);
    ud[0] = ud[1] = make_int2(0, 0);
    if (!syncw) { request_units(0); take_units(); load_rec(I0, 0, ud[0], 0); load_rec(I1, 0, ud[1], 0); prefetch(0); request_units(1); }
    int cur = 0;
    bool vnz = false;                                   // the virtual rows may hold mass: some column was clamped last period
    const int son = (x == 0 && cW < 32) ? cW : -1;     // dev stamps (make stamp)
    (void)son;
    // the aggregate of period tp from the lanes' terms (sync wave; fixed order: columns ascending, then the lanes' DPP tree)
    auto reduce_agg = [&](int tp) {
        const double *ap = aggsh + (size_t)lane * NAP;
        double sk[NAP];
#pragma unroll
        for (int k = 0; k < NAP; k++) sk[k] = 0.0;
        for (int k2 = 0; k2 < ne; k2++) {
            double v[NAP];
            if (NAP == 1) v[0] = ap[(size_t)k2 * 64 * NAP];
            else {
#pragma unroll
                for (int q = 0; q < NAP / 2; q++) { const double2 d = reinterpret_cast<const double2 *>(ap + (size_t)k2 * 64 * NAP)[q]; v[2 * q] = d.x; v[2 * q + 1] = d.y; }
            }
#pragma unroll
            for (int k = 0; k < NAP; k++) sk[k] += v[k];
        }
        const size_t pb = (size_t)tp * Sact + cW;
#pragma unroll
        for (int k = 0; k < D; k++) {       // daggpart: [P][members][2 W], W = XG * D: the first aggregate's partials, then the second's
            const double pd = xwave_reduce63(sk[k]), pd2 = xwave_reduce63(sk[NSL + k]);
            if (lane == 63) { A.daggpart[pb * (size_t)(2 * XG * D) + x * D + k] = pd; A.daggpart[pb * (size_t)(2 * XG * D) + XG * D + x * D + k] = pd2; }
        }
        if constexpr (VAL) {
            if (recD) {
                const double pD = xwave_reduce63(sk[IV]), pD2 = xwave_reduce63(sk[NSL + IV]);
                if (lane == 63) { A.aggpart[2 * pb] = pD; A.aggpart[2 * pb + 1] = pD2; }
            }
        }
    };
    for (int t = 0; t < P; t++) {
        XSTAMP(1, son, t, 0);
        const size_t base = (size_t)t * G + (size_t)e * na;
        const size_t hb = (size_t)cur * hs;
        const int sw = srcsh[t];
        int clo = 0;
        if (!syncw) {
            clo = min(max(closh[t * ne + e], 0), na);
            double z[SL];
#pragma unroll
            for (int k = 0; k < SL; k++) z[k] = 0.0;
#if HANK_XFWD_TILE_SOA
            if constexpr (SOA) xtile_soa_store<NSL>(myt, z); else
#endif
            xtile_store<SL>(myt, z);                    // (every wave is past the previous period's mixing: xbar_arrive)
            set_g(I0);                                 // (LQ) the units' records have landed — the drain waited for them — and the wave has
            set_g(I1);                                  // nothing to do until the source poll is through: not between the state loads and process()
        }
        if (sync_duty) xpoll(A.sy, x, sw & 255, (sw >> 8) & 255, (unsigned)(t + 1));   // this period's source members have published period t-1
        xlds_barrier();
        XSTAMP(1, son, t, 1);
        if (sync_duty && t > 0) reduce_agg(t - 1);      // (the sync wave has nothing else to do until the gathers are done)
        double pagg[DD];
#pragma unroll
        for (int k = 0; k < DD; k++) pagg[k] = 0.0;
        double v0 = 0.0;                                // the record's row 0: the mass on every member's virtual row of this column
        if (!syncw) {
            const bool need0 = recL && r0 == 0 && vnz && clo == 0;      // (wave-uniform)
            if constexpr (RECL) {
                if (need0 && lane < Sact) v0 = rows.load_one(hb + gx + ((size_t)e * Sact + lane) * 64 + 63, IV);
            }
            load_state(I0, hb, cur, ud[0], 0);
            load_state(I1, hb, cur, ud[1], 0);
            // Young lottery of a source (ForwardIteration.jl:59-73): (1-w) to row lo, w to row lo+1; the weight's partial is
            // dpol / gap (zero where clamped), times D_{t-1} of the row. Only the parts that land in the unit's own target run
            // [ta, tb) are added (the other part of a seam source belongs to the neighbouring unit).
            // PRE-COMBINE (round 5). The sources of a unit are consecutive lanes and their brackets rise with them: where the policy moves
            // one grid row per source row — most of the grid — the upper part of lane i-1 and the lower part of lane i land on the SAME
            // tile row. Lane i then adds both in one ds_add_f64 (the neighbour's part arrives by a wave_shr:1 DPP move) and lane i-1
            // skips its own: half the LDS atomics of the walk (20 per wave and period at D = 4 with the value; a timing build without
            // them put their cost at 0.33 ms of the sweep). Still one unit = one wave in program order: reproducible bit for bit; where a
            // row receives exactly these two terms the sum is the same (0 + L) + H = 0 + (L + H).
            auto process_pc = [&](auto U, int2 d) {
                constexpr int u = decltype(U)::value;
                const int ta = d.y & 0xff, tb = (d.y >> 8) & 0xff;
                double *const colt = XT_COL(d.x & 15);
                const double w = qw[u], w1 = 1.0 - w;
                double gD = qg[u], Dv = 0.0;
                if constexpr (VAL) { Dv = dd[u][IV]; gD = qg[u] * Dv; }
                else { if (qvl[u]) gD = 0.0; }          // (a virtual row's mass is part of the recorded ig * D of row 0)
                const int tl = qlo[u] - r0, th = tl + 1;
                const bool doL = qon[u] && tl >= ta && tl < tb, doH = qon[u] && th >= ta && th < tb;
                const int thp = __builtin_amdgcn_update_dpp(-2, doH ? th : -2, 0x138, 0xf, 0xf, false);        // lane i-1's upper target (wave_shr:1; lane 0: none)
#if HANK_XFWD_FLAT_TR
                const bool take = doL && thp == tl && !unit_flat(d);      // (a transposed unit's DPP neighbours are not its source neighbours)
#else
                const bool take = doL && thp == tl;
#endif
                const bool given = __builtin_amdgcn_update_dpp(0, take ? 1 : 0, 0x130, 0xf, 0xf, false) != 0;   // lane i+1 adds my upper part with its lower one (wave_shl:1)
                double *const tpl = XT_ROW(colt, doL ? tl : 0), *const tph = XT_ROW(colt, doH ? th : 0);
#pragma unroll
                for (int k = 0; k < D; k++) {
                    const double hk = w * dd[u][k] + gD * qdp[u][k];
                    const double hp = xdpp<0x138, 0xf, 0xf>(hk);
                    const double lk = w1 * dd[u][k] - gD * qdp[u][k];
                    if (doL) lds_add(XT_SLOT(tpl, k), take ? lk + hp : lk);
                    if (doH && !given) lds_add(XT_SLOT(tph, k), hk);
                }
                if constexpr (VAL) {                    // (the VALUE keeps one add per part: D_t — the record — is the same bits whichever kernel carries it)
                    if (doL) lds_add(XT_SLOT(tpl, IV), w1 * Dv);
                    if (doH) lds_add(XT_SLOT(tph, IV), w * Dv);
                }
                if constexpr (!VAL) {
                    if (doL && !qvl[u]) {               // (every unclamped source has exactly one lower target: its aggregate term is taken here, once)
#pragma unroll
                        for (int k = 0; k < D; k++) pagg[k] += qdp[u][k] * qdn[u];
                    }
                }
            };
            auto process_1 = [&](auto U, int2 d) {
                constexpr int u = decltype(U)::value;
                if (!qon[u]) return;
                const int ta = d.y & 0xff, tb = (d.y >> 8) & 0xff;
                double *const colt = XT_COL(d.x & 15);
                const double w = qw[u], w1 = 1.0 - w;
                double gD = qg[u], Dv = 0.0;
                if constexpr (VAL) { Dv = dd[u][IV]; gD = qg[u] * Dv; }
                else { if (qvl[u]) gD = 0.0; }          // (a virtual row's mass is part of the recorded ig * D of row 0)
                const int tl = qlo[u] - r0, th = tl + 1;
                if (tl >= ta && tl < tb) {              // (every unclamped source has exactly one lower target: its aggregate term is taken here, once)
                    double *tp = XT_ROW(colt, tl);
#pragma unroll
                    for (int k = 0; k < D; k++) lds_add(XT_SLOT(tp, k), w1 * dd[u][k] - gD * qdp[u][k]);
                    if constexpr (VAL) lds_add(XT_SLOT(tp, IV), w1 * Dv);
                    if constexpr (!VAL) {
                        if (!qvl[u]) {
#pragma unroll
                            for (int k = 0; k < D; k++) pagg[k] += qdp[u][k] * qdn[u];
                        }
                    }
                }
                if (th >= ta && th < tb) {
                    double *tp = XT_ROW(colt, th);
#pragma unroll
                    for (int k = 0; k < D; k++) lds_add(XT_SLOT(tp, k), w * dd[u][k] + gD * qdp[u][k]);
                    if constexpr (VAL) lds_add(XT_SLOT(tp, IV), w * Dv);
                }
            };
            // (narrow kernels — one or two slots per tile row — keep one add per part: at D = 1 the exchange costs more than the
            // one atomic it saves, single-tangent JVP 1.98 -> 2.06 ms)
            constexpr bool PRECOMB = NSL >= 3;
            auto process = [&](auto U, int2 d) { if constexpr (PRECOMB) process_pc(U, d); else process_1(U, d); };
            process(I0, ud[0]);
            process(I1, ud[1]);
            // (rare) a unit wider than a wave — more than 64 sources on ONE target row — and units beyond the member's 2 n_e slots
            const int nu = (sw >> 18) & 0xff;
            for (int u2 = wv; u2 < nu; u2 += ne) {
                const int2 d = u2 < 2 * ne ? ud[u2 >= ne ? 1 : 0] : unit_desc(t, u2);
                const int tot = ((d.x >> 16) & 0xfff) + ((d.y >> 16) & 0xff);
                for (int i0 = u2 < 2 * ne ? 64 : 0; i0 < tot; i0 += 64) {
                    load_rec(I0, t, d, i0);
                    load_state(I0, hb, cur, d, i0);
                    set_g(I0);                          // (behind the state loads' issue: the record, loaded first, lands first)
                    process(I0, d);
                }
            }
            if constexpr (RECL) { if (need0) v0 = xwave_sum(v0); }
            take_units();                               // the next period's descriptors (requested a period ago; this wave's loads have all landed here)
            // (dev knob HANK_XFWD_EARLY_BATCH, off) the unit batch HERE, where its registers are free — process() and the rare units are through —
            // instead of behind the barrier below; still older than the own-row batch, vmcnt(XFWD_NLD) drains it. Measured: 0.18 ms per step
            // SLOWER — the path is not idle in front of that barrier, and the period's stores then queue behind the batch
            if constexpr (EARLYB) next_units_loads(t);
            XSTAMP(1, son, t, 2);
            // the mass point: sources clamped at the first grid point (:54-58) go to row 0 with weight one and no weight
            // partial. Each member sums ITS clamped rows into its virtual row (never combined: everything downstream is
            // linear); while row 0 itself is clamped the old virtual row is carried along.
            double cT[NSL];
#pragma unroll
            for (int k = 0; k < NSL; k++) cT[k] = ((own && r < clo) || (virt && clo > 0 && vnz)) ? mxp[k] : 0.0;
            if (clo > r0) {
#pragma unroll
                for (int k = 0; k < NSL; k++) cT[k] = xwave_reduce63(cT[k]);
            }
#if HANK_XFWD_TILE_SOA
            if constexpr (SOA) { if (virt) xtile_soa_store<NSL>(myt, cT); } else
#endif
            if (virt) xtile_store_n<SL, NSL>(myt, cT);
        }
        XSTAMP(1, son, t, 3);
        XSTAMPV(1, son, t);
        if (sync_duty) xpoll(A.sy, x, 0, Sact - 1, (unsigned)(t + 1));      // EVERY member is done reading the half about to be overwritten
        xlds_barrier();
        XSTAMP(1, son, t, 4);
        vnz = ((sw >> 16) & 1) != 0;
        const int nxt = cur ^ 1;
        if (!syncw) {
            if constexpr (!EARLYB) next_units_loads(t); // accepted by the memory path while the waves mix (see above)
            // exogenous transition: D_t[., e] = sum_k D_mid[., k] Pi[k, e] (ForwardIteration.jl:95-99), value and partials in one pass
            double mx[NSL];
#if HANK_XFWD_TILE_SOA
            if constexpr (SOA) {
                if (PIREG) xtile_soa_mix_reg<NSL, true>(tile + lane, pr, ne, mx);
                else xtile_soa_mix<NSL, true>(tile + lane, Pish + ne * e, 1, ne, mx);
            } else
#endif
            if (PIREG) xtile_mix_reg<SL, NSL, true>(tile + (size_t)lane * SL, pr, ne, mx);
            else xtile_mix<SL, NSL, true>(tile + (size_t)lane * SL, Pish + ne * e, 1, ne, mx);
            if (live) {
                double sv[SP];
#pragma unroll
                for (int k = 0; k < SP; k++) sv[k] = k < NSL ? mx[k] : 0.0;
                if constexpr (XB) rows.store_vs(lane, nxt * ihs + igx + islot, sv);
                else rows.store((size_t)nxt * hs + slot, sv);
            }
            double at[NAP];
#pragma unroll
            for (int k = 0; k < NAP; k++) at[k] = 0.0;
            if constexpr (RECL) {
                if (recL && own) {
                    // what the tangent sweeps read per SOURCE: {w, ig * D_{t-1}} (k_lottery's w and ig); k_xlwg_build repeats this
                    // arithmetic operand by operand
                    double Dfull = mxp[IV];
                    if (r == 0 && clo == 0) Dfull += v0;
                    R.lwg[base + r] = make_double2(lwr, igr * Dfull);
                }
            }
            if constexpr (VAL) {
                if (recD) {
                    if (own) {
                        if constexpr (XB) buf_st64<0>(mx[IV], rrec, ipt * 8, (int)(A.ro.Dseq + (unsigned)((t + 1) * G) * 8u));
                        else R.Dseq[(size_t)(t + 1) * G + pt] = mx[IV];
                    } else if (virt) A.Dvirt[((size_t)t * ne + e) * 64 + cW] = mx[IV];
                    // aggregate on the POST-transition distribution (ForwardIteration.jl:301-307); a virtual row carries row 0's policy
                    at[IV] = live ? polr * mx[IV] : 0.0;
                    at[NSL + IV] = live ? xar * mx[IV] : 0.0;
                }
            }
            // aggregate partials: pol_t dD_t + dpol_t D_t. Value carried: a row's own policy partials meet its new D_t here (a
            // virtual row carries row 0's policy and row 0's partials). At a recorded primal: the second term was taken at the
            // source rows (pagg), clamped rows add theirs here, and a virtual row's share of D_t[0] is in the recorded D_t[0].
#pragma unroll
            for (int k = 0; k < D; k++) {
                double term = live ? polr * mx[k] : 0.0;
                if constexpr (VAL) term = live ? (polr * mx[k] + dpr[k] * mx[IV]) : 0.0;
                else term = (term + pagg[k]) + ((own && r < clo) ? dpr[k] * Dr : 0.0);
                at[k] = term;
                at[NSL + k] = live ? xar * mx[k] : 0.0;      // the grid-weighted aggregate's partial: sum a dD_t
            }
            xtile_store<NAP>(aggsh + ((size_t)e * 64 + lane) * NAP, at);      // summed by the sync wave in the next period (reduce_agg)
#pragma unroll
            for (int k = 0; k < NSL; k++) mxp[k] = mx[k];
        }
        cur = nxt;
        XSTAMP(1, son, t, 5);
        if (!syncw) {
            asm volatile("; XFWD_BATCH_BEGIN" ::: "memory");
            prefetch(min(t + 1, P - 1));                // (t: the period that has just been stored)
            XSTAMP(1, son, t, 7);
            asm volatile("; XFWD_BATCH_END\n\ts_waitcnt vmcnt(%0)" ::"n"(XFWD_NLD) : "memory");       // this member's stores have reached L2 ...
            XSTAMP(1, son, t, 8);
        }
        xlds_barrier();
        if (sync_duty) xpublish(A.sy, x, cW, (unsigned)(t + 2));                                       // ... episode t+2
        XSTAMP(1, son, t, 6);
    }
    if (sync_duty) reduce_agg(P - 1);                   // (every wave wrote its terms before the last barrier)
}
#undef XUNIT_LANE
#undef XT_COL
#undef XT_ROW
#undef XT_SLOT
static inline size_t x_lds_fwd(const Consts &c, int D, bool val) { return xlds_fwd(c.n_e, c.P, D, val).bytes; }
static inline size_t x_lds_fwd_lq(const Consts &c, int D) { return xlds_fwd_lq(c.n_e, c.n_a, c.P, D).bytes; }      // k_xfwd<D, true, ., true>: where it does not fit the device, the launcher takes k_xfwd<D, true>

// the forward sweeps' work units from the lottery record (see k_xfwd), one block per (period, member): thread e cuts column
// e's walk over the sources of the member's target rows into units — a run [ta, tb) of target rows (relative to the member's
// first row) and the <= 64 consecutive sources [ja, ja + cnt) whose brackets touch it; the unit that walks source row 0 of an
// open column while the virtual rows hold mass gets `nv` = members extra lanes (see k_xfwd). Units are numbered column by
// column; unit u goes to wave u mod n_e. Per (period, member) also: the members its sources belong to (lo | hi << 8), whether
// some column is clamped in the period (<< 16: the virtual rows hold mass in the next one), whether member 0 needs every
// member's virtual row for the record of row 0 (<< 17), and the unit count (<< 18).
__global__ void k_xunits_fwd(Consts c, Record R, int Sact, int *src, int2 *units, int *overflow, int ucap) {
    __shared__ int2 su[16][XUCAP];
    __shared__ int scnt[16], slo, shi, sany0;
    __shared__ int sst[16][XRW + 3];                    // start[r0-1 .. r0+nrows] of every column: the walk below is serial per column,
    const int t = blockIdx.x, m = blockIdx.y, ne = c.n_e, na = c.n_a;      // and as dependent global loads it was 86 us per record
    const int r0 = m * XRW, nrows = min(XRW, na - r0);
    __shared__ int sclo[16], sclop[16], soff[17];       // clamped prefixes of this period and of the one before, unit offsets per column
    if (threadIdx.x == 0) { slo = m; shi = m; sany0 = 0; }
    if ((int)threadIdx.x < ne) {
        sclo[threadIdx.x] = R.clo[(size_t)t * ne + threadIdx.x];
        sclop[threadIdx.x] = t > 0 ? R.clo[(size_t)(t - 1) * ne + threadIdx.x] : 0;
    }
    for (int k = threadIdx.x; k < ne * (XRW + 3); k += blockDim.x) {
        const int e = k / (XRW + 3), q = k - e * (XRW + 3);
        sst[e][q] = min(max(R.start[((size_t)t * ne + e) * (na + 1) + min(max(r0 - 1 + q, 0), na)], 0), na);
    }
    __syncthreads();
    bool vnz = false;
    for (int e = 0; e < ne; e++) vnz = vnz || sclop[e] > 0;
    // One wave per column (the block's waves take the columns in turn). The greedy walk "extend the unit while it has <= 64 lanes"
    // is 63 dependent steps as a loop; the end of the unit that STARTS at target row ta is a monotone search, so lane ta finds it
    // by bisection (nxt), all 63 at once, and lane 0 then follows the chain nxt[0], nxt[nxt[0]], ... — a handful of hops.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    for (int e = wave; e < ne; e += nwaves) {
        const int clo = sclo[e];
        auto S = [&](int rr) { return sst[e][min(max(rr - (r0 - 1), 0), XRW + 2)]; };     // (clamped at the fill: a record that is not a lottery must not turn into a long walk or an out-of-range row)
        // lanes of a unit that starts at `a` and ends before target row `b`: its sources, and every member's virtual row when it walks source 0
        auto lanes_of = [&](int a, int b, int *ja_out, bool *has0_out) {
            const int ja = S(r0 + a - 1 < 0 ? 0 : r0 + a - 1);
            const bool has0 = ja == 0 && clo <= 0 && vnz;        // (then source row 0 is the unit's first lane, if it has any)
            const int cnt = max(S(r0 + b) - ja, 0);
            *ja_out = ja; *has0_out = has0;
            return cnt;
        };
        int nxt = nrows;
        if (lane < nrows) {
            int ja; bool has0;
            (void)lanes_of(lane, lane + 1, &ja, &has0);
            auto fits = [&](int b) { const int c2 = max(S(r0 + b) - ja, 0); return c2 + ((has0 && c2 > 0) ? Sact : 0) <= 64; };
            int lo = lane + 1, hi = nrows;               // the unit ends at the largest b in [lane + 1, nrows] with every step up to it fitting
            if (lo < hi && fits(lo + 1)) {               // (the count is monotone in b: a bisection)
                if (fits(hi)) lo = hi;
                else {
                    lo = lo + 1;
                    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (fits(mid)) lo = mid; else hi = mid; }
                }
            }
            nxt = lo;
        }
        int n = 0, ta = 0;
        while (ta < nrows && n < XUCAP) {               // (wave-uniform: every lane follows the same chain)
            const int tb = __shfl(nxt, ta, 64);
            int ja; bool has0;
            const int cnt = lanes_of(ta, tb, &ja, &has0);
            const int nv = (has0 && cnt > 0) ? Sact : 0;
            if (cnt > 0) {
                if (lane == 0) {
                    su[e][n] = make_int2(e | (ja << 4) | (cnt << 16), ta | (tb << 8) | (nv << 16));
                    atomicMin(&slo, ja / XRW); atomicMax(&shi, (ja + cnt - 1) / XRW);
                    if (nv) sany0 = 1;
                }
                n++;
            }
            ta = tb;
        }
        if (lane == 0) {
            if (ta < nrows) atomicExch(overflow, 1);
            scnt[e] = n;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0;
        for (int e = 0; e < ne; e++) { soff[e] = off; off += scnt[e]; }
        soff[ne] = off;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < min(soff[ne], XUCAP); k += blockDim.x) {      // units numbered column by column
        int e = 0;
        while (e + 1 < ne && soff[e + 1] <= k) e++;
        units[((size_t)t * Sact + m) * XUCAP + k] = su[e][k - soff[e]];
    }
    if (threadIdx.x == 0) {
        int tot = soff[ne], anyclo = 0, anyopen = 0;
        for (int e = 0; e < ne; e++) {
            if (sclo[e] > 0) anyclo = 1; else anyopen = 1;
        }
        if (tot > ucap) { atomicExch(overflow, 1); tot = min(tot, XUCAP); }      // (ucap = XUCAP but for the dev knob HANK_XUCAP)
        int ml = min(slo, m), mh = max(shi, m);
        if (sany0) { ml = 0; mh = Sact - 1; }           // the units with virtual lanes read every member's virtual row
        const int allv = (m == 0 && vnz && anyopen) ? 1 : 0;
        src[(size_t)t * Sact + m] = ml | (mh << 8) | (anyclo << 16) | (allv << 17) | (tot << 18);
    }
}

// ---- the front of the one-pass persistent Dual pass (between k_xdual_back and k_xfwd<D, true, ., true>): two launches that stand for
// k_lottery_lq and k_xunits_fwd and write only what that pass reads --------------------------------------------------------------
// k_xdual_front, one block per column (t, e) like k_lottery. Lottery: lottery_body's lean arm — lq and clo; lo, lw, ig, start and
// seg stay unwritten (the host marks the record: ensure_lottery runs k_lottery before the first reader). Cut: with the column's
// start table still in LDS (shst), a thread per member cuts the column's walk into that member's units (xu_cut,
// hank_xunits.h: the end of each unit by bisection, then the chain is followed) and stages them per
// (t, member, column): su [P][Sact][n_e][XU_ROWS] the units, sm [P][Sact][n_e] {count, source members lo, hi, a unit has virtual lanes}.
// A column has at most XU_ROWS units of a member, so the staging never truncates: what overflows is a member's TOTAL, in k_xunits_pack.
// vnz — the virtual rows hold mass in period t: some column of t - 1 is clamped — is the one thing a column needs from other columns:
// row 0 of every column of pol[t - 1] under lottery_body's own test (a clamped prefix, where the policy is monotone, starts at row 0;
// where it is not, the error word is set and the call fails).
// poison (tests only: HANK_XDUAL_FRONT_POISON): the arrays left unwritten are filled with values no reader can take for a lottery —
// lw, ig NaN; lo, start 0 (in range) — so that a reader that skipped ensure_lottery fails a parity test instead of reading the last record.
// dynamic LDS: 2 n_a + 2 ints (lottery_body's)
static_assert(XU_ROWS == XRW && XU_LANES == 64, "hank_xunits.h cuts for this sweep geometry");
__global__ void __launch_bounds__(512) k_xdual_front(Consts c, Record R, int ncols, int *err, int4 *lq, int Sact, int2 *su, int4 *sm, int poison) {
    extern __shared__ int shlo[];
    __shared__ int sh_clo, sh_vnz;
    const int col = blockIdx.x;
    if (col >= ncols) return;
    const int ne = c.n_e, n = c.n_a;
    const int t = col / ne, e = col - t * ne;
    bool v = false;
    if (t > 0 && (int)threadIdx.x < ne) {
        const size_t i0 = (size_t)(t - 1) * c.G + (size_t)threadIdx.x * n;
        v = lottery_hi(c, R, i0, R.pol[i0], 1) == 0;
    }
    if (threadIdx.x == 0) sh_vnz = 0;
    lottery_body<true>(c, R, col, err, 0, 1, shlo, &sh_clo, lq);      // (its barriers order sh_vnz's reset, and shst is complete behind it)
    if (v) atomicOr(&sh_vnz, 1);
    if (poison) {
        const size_t base = (size_t)col * n;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        for (int j = threadIdx.x; j < n; j += blockDim.x) { R.lo[base + j] = 0; R.lw[base + j] = qnan; R.ig[base + j] = qnan; }
        for (int r = threadIdx.x; r <= n; r += blockDim.x) R.start[(size_t)col * (n + 1) + r] = 0;
    }
    __syncthreads();
    const int *shst = shlo + n;
    const int clo = sh_clo;
    const bool vnz = sh_vnz != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    auto S = [&](int r) { return min(max(shst[min(max(r, 0), n)], 0), n); };
    // a thread per member, the members dealt round the block's waves (Sact / waves lanes of each: the walks of a wave's lanes run in
    // lockstep and take as long as the longest, so few share a wave): the serial form of the cut, every read from LDS
    for (int m = wave + nwaves * lane; m < Sact; m += nwaves * 64) {
        const int r0 = m * XRW, nrows = min(XRW, n - r0);
        const size_t slot = ((size_t)t * Sact + m) * ne + e;
        int2 *out = su + slot * XU_ROWS;
        const XuCut q = xu_cut(S, [&](int ta) { return xu_next(S, clo, vnz, Sact, r0, nrows, ta); }, [&](int k, int x, int y) { out[k] = make_int2(x, y); },
                               clo, vnz, r0, nrows, Sact, e, m, XU_ROWS);
        sm[slot] = make_int4(q.n, q.mlo, q.mhi, q.anyv);
    }
}
// k_xunits_pack, one wave per (period, member): the prefix over the columns' staged counts, the units copied to units[t][m][k]
// numbered column by column, the src word — bit for bit k_xunits_fwd's — and the overflow flag. A launch of its own behind
// k_xdual_front: a "last block of the period finishes" counter inside that launch would be a hand-off between XCDs within one launch.
__global__ void __launch_bounds__(256) k_xunits_pack(Consts c, Record R, int Sact, const int2 *su, const int4 *sm, int *src, int2 *units, int *overflow, int ucap) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= c.P * Sact) return;                         // (wave-uniform)
    const int ne = c.n_e, t = w / Sact, m = w - t * Sact;
    int4 q = make_int4(0, m, m, 0);
    int clo = 0, clop = 0;
    if (lane < ne) {
        q = sm[(size_t)w * ne + lane];
        clo = R.clo[(size_t)t * ne + lane];
        clop = t > 0 ? R.clo[(size_t)(t - 1) * ne + lane] : 0;
    }
    const int cnt = min(max(q.x, 0), XU_ROWS);
    int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) { const int up = __shfl_up(inc, off, 64); if (lane >= off) inc += up; }
    const int excl = inc - cnt;
    int tot = __shfl(inc, 63, 64);
    int mycol = -1, myoff = 0;
    for (int e = 0; e < ne; e++) {
        const int oe = __shfl(excl, e, 64), ce = __shfl(cnt, e, 64);
        if (lane >= oe && lane < oe + ce) { mycol = e; myoff = lane - oe; }
    }
    if (mycol >= 0 && lane < XUCAP) units[(size_t)w * XUCAP + lane] = su[((size_t)w * ne + mycol) * XU_ROWS + myoff];
    int ml = min(q.y, m), mh = max(q.z, m);
    for (int off = 32; off > 0; off >>= 1) { ml = min(ml, __shfl_xor(ml, off, 64)); mh = max(mh, __shfl_xor(mh, off, 64)); }
    const bool sany0 = __ballot(lane < ne && q.w != 0) != 0, anyclo = __ballot(lane < ne && clo > 0) != 0;
    const bool anyopen = __ballot(lane < ne && clo <= 0) != 0, vnz = __ballot(clop > 0) != 0;
    if (lane == 0) {
        if (tot > ucap) { atomicExch(overflow, 1); tot = min(tot, XUCAP); }      // (ucap = XUCAP but for the dev knob HANK_XUCAP)
        ml = min(max(ml, 0), Sact - 1); mh = min(max(mh, 0), Sact - 1);
        if (sany0) { ml = 0; mh = Sact - 1; }           // the units with virtual lanes read every member's virtual row
        const int allv = (m == 0 && vnz && anyopen) ? 1 : 0;
        src[w] = ml | (mh << 8) | ((anyclo ? 1 : 0) << 16) | (allv << 17) | (tot << 18);
    }
}

// which members does member c gather from in period t? (lo | hi << 8), from the recorded primal; one block per (t, c)
__global__ void k_xsrc_back(Consts c, Record R, int Sact, int *src) {
    __shared__ int smin[256], smax[256];
    const int t = blockIdx.x, m = blockIdx.y;
    const int r0 = m * XRW, rows = min(XRW, c.n_a - r0);
    int lo = 1 << 30, hi = -1;
    for (int k = threadIdx.x; k < rows * c.n_e; k += blockDim.x) {
        const int e = k / rows, a = r0 + (k - e * rows);
        const size_t ro = (size_t)t * c.G + (size_t)e * c.n_a + a;
        if (R.A[ro] != 0.0 || R.B[ro] != 0.0) { const int ib = R.ib[ro]; lo = min(lo, ib); hi = max(hi, ib + 1); }
    }
    smin[threadIdx.x] = lo; smax[threadIdx.x] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)blockDim.x; k++) { lo = min(lo, smin[k]); hi = max(hi, smax[k]); }
        int ml = m, mh = m;
        if (hi >= 0) { ml = min(m, max(lo, 0) / XRW); mh = max(m, min(hi, c.n_a - 1) / XRW); }
        src[(size_t)t * Sact + m] = ml | (mh << 8);
    }
}
// rho_t = 1/(1+r_t) for every period (the X half's discounting; same expression as egm_X)
__global__ void k_xrho(const double *xhh, int n_hh, int P, double *rho) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P) rho[t] = 1.0 / (1.0 + xhh[n_hh * t]);
}

// row 0 of every column of D_1..D_P: add the virtual mass the forward sweep kept apart (member order fixed). D0own keeps what
// member 0 itself held on that row (k_xlwg_build's operand)
__global__ void k_xfix_D(Consts c, double *Dseq, const double *Dvirt, int Sact, double *D0own) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= c.P * c.n_e) return;
    const int t = idx / c.n_e, e = idx - t * c.n_e;
    double s = Dseq[(size_t)(t + 1) * c.G + (size_t)e * c.n_a];
    D0own[idx] = s;
    for (int m = 0; m < Sact; m++) s += Dvirt[(size_t)idx * 64 + m];
    Dseq[(size_t)(t + 1) * c.G + (size_t)e * c.n_a] = s;
}

// The per-source record {w, ig D_{t-1}} of every period, for the tangent sweeps at a primal that a Dual pass recorded (its forward
// half does not write it: see k_xfwd). One block per (period, column); 24 bytes read and 16 written per point. Operand by
// operand what the Float64 sweep's writer does (k_xfwd<0, true>), so that the record has the same bits whoever made it: a row's
// D_{t-1} as its member stored it, and for row 0 of an open column while the virtual rows hold mass (some column was clamped the
// period before) member 0's own part PLUS the butterfly sum of the members' virtual rows in lane order (xwave_sum) — not the
// completed row 0 of Dseq, which k_xfix_D sums member by member.
__global__ void __launch_bounds__(256) k_xlwg_build(Consts c, Record R, const double *__restrict__ Dvirt, const double *__restrict__ D0own, int Sact) {
    const int col = blockIdx.x, ne = c.n_e, n = c.n_a;
    if (col >= c.P * ne) return;
    const int t = col / ne, e = col - t * ne, lane = threadIdx.x & 63;
    const size_t base = (size_t)col * n;                // == t * G + e * n_a
    bool vnz = false;
    if (t > 0)
        for (int k = 0; k < ne; k++) vnz = vnz || R.clo[(size_t)(t - 1) * ne + k] > 0;
    const int clo = min(max(R.clo[col], 0), n);
    double v0 = 0.0;
    if (threadIdx.x < 64 && vnz && clo == 0) {          // (block-uniform but for the wave: wave 0 owns row 0)
        if (lane < Sact) v0 = Dvirt[((size_t)(t - 1) * ne + e) * 64 + lane];
        v0 = xwave_sum(v0);
    }
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        double Dfull = (r == 0 && t > 0) ? D0own[(size_t)(t - 1) * ne + e] : R.Dseq[base + r];
        if (r == 0 && clo == 0) Dfull += v0;
        R.lwg[base + r] = make_double2(R.lw[base + r], R.ig[base + r] * Dfull);
    }
}

// dagg of one pass [P][XG*D] -> columns [n0, n0+N) of the caller's (P, Ntot) column-major block
__global__ void k_xout(const double *__restrict__ dagg, int P, int W, int src0, int n0, int N, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * N) return;
    const int n = idx / P, t = idx - n * P;
    out[(size_t)(n0 + n) * P + t] = dagg[(size_t)t * W + src0 + n];
}

// ---- the persistent Dual pass's small work in TWO launches (round 5) ---------------------------------------------------------
// A one-pass Dual pass used to be wrapped in fifteen launches and copies of a few microseconds each (two input copies, two
// memsets of the sync blocks, k_zero_i32, k_xrho, k_tan_in in front; k_reduce_parts, k_tan_out, k_xfix_D, k_reduce_parts, two
// k_xout and two output copies behind): dependent launches on one stream cost ~3-5 us apiece, 0.07 ms of a 4.35 ms step.
// k_xdual_prologue: inputs in (the caller's device buffers are read where they lie; the context keeps its copies), rho_t, the
// per-direction input partials [P][N], the four sync blocks and the error word zeroed.
__global__ void k_xdual_prologue(const double *__restrict__ xhh_src, double *__restrict__ xhh_dst, const double *__restrict__ dx_src, double *__restrict__ dx_dst,
                                 int n_hh, int P, int N, double *__restrict__ rho, double *__restrict__ dxr, double *__restrict__ dxw, double *__restrict__ dxt,
                                 xv4u *__restrict__ sync, size_t sync_q, int *__restrict__ err) {
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < sync_q; i += step) { xv4u z; z.x = z.y = z.z = z.w = 0u; sync[i] = z; }
    if (i0 < 4) err[i0] = 0;
    for (size_t t = i0; t < (size_t)P; t += step) {
        rho[t] = 1.0 / (1.0 + xhh_src[(size_t)n_hh * t]);                   // (k_xrho's expression)
        if (xhh_dst != xhh_src)
            for (int k = 0; k < n_hh; k++) xhh_dst[(size_t)n_hh * t + k] = xhh_src[(size_t)n_hh * t + k];
    }
    for (size_t idx = i0; idx < (size_t)P * N; idx += step) {              // (k_tan_in)
        const size_t t = idx / N, n = idx - t * N;
        const size_t o = (size_t)n_hh * (t + (size_t)P * n);
        const double a = dx_src[o], b = dx_src[o + 1], c2 = n_hh > 2 ? dx_src[o + 2] : 0.0;
        dxr[idx] = a; dxw[idx] = b;
        if (n_hh > 2) dxt[idx] = c2;
        if (dx_dst != dx_src) { dx_dst[o] = a; dx_dst[o + 1] = b; if (n_hh > 2) dx_dst[o + 2] = c2; }
    }
}
// the sum k_reduce_parts takes over nb row blocks, in its order (four strided groups of eight, then the groups)
__device__ __forceinline__ double xreduce_parts_at(const double *__restrict__ parts, int nb, int N, int t, int n) {
    const double *p = parts + (size_t)t * nb * N + n;
    double sg[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        double s = 0.0;
        int b = g;
        for (; b + 28 < nb; b += 32) {
            const double v0 = p[(size_t)b * N], v1 = p[(size_t)(b + 4) * N], v2 = p[(size_t)(b + 8) * N], v3 = p[(size_t)(b + 12) * N];
            const double v4 = p[(size_t)(b + 16) * N], v5 = p[(size_t)(b + 20) * N], v6 = p[(size_t)(b + 24) * N], v7 = p[(size_t)(b + 28) * N];
            s += ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7));
        }
        for (; b < nb; b += 4) s += p[(size_t)b * N];
        sg[g] = s;
    }
    return (sg[0] + sg[1]) + (sg[2] + sg[3]);
}
// k_xdual_epilogue: both aggregates of the value and of the pass's partials summed over the members (k_reduce_parts' order), laid
// out as the entry points return them (k_tan_out, k_xout) — into the context's buffers AND the caller's —, and row 0 of every D_t
// completed with the virtual rows' mass (k_xfix_D, which also keeps member 0's own part). One thread per (period, output).
__global__ void k_xdual_epilogue(Consts c, const double *__restrict__ aggpart, const double *__restrict__ daggpart, int Sact, int W, int n0, int N, int Ntot,
                                 double *__restrict__ agg_rm, double *__restrict__ agg_cm, double *__restrict__ dagg_pass, double *__restrict__ dagg_cm,
                                 double *__restrict__ Dseq, const double *__restrict__ Dvirt, double *__restrict__ D0own, double *__restrict__ out_agg, double *__restrict__ out_dagg) {
    const int P = c.P, per = 2 * W + 2 + c.n_e;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * per) return;
    const int t = idx / per, j = idx - t * per;
    if (j < 2 * W) {
        const double v = xreduce_parts_at(daggpart, Sact, 2 * W, t, j);
        dagg_pass[(size_t)t * 2 * W + j] = v;
        const int half = j >= W, n = j - half * W;
        if (n < N) {
            dagg_cm[(size_t)half * P * Ntot + (size_t)(n0 + n) * P + t] = v;
            if (!half && out_dagg) out_dagg[(size_t)(n0 + n) * P + t] = v;
        }
    } else if (j < 2 * W + 2) {
        const int k = j - 2 * W;
        const double v = xreduce_parts_at(aggpart, Sact, 2, t, k);
        agg_rm[(size_t)t * 2 + k] = v;
        agg_cm[(size_t)k * P + t] = v;
        if (k == 0 && out_agg) out_agg[t] = v;
    } else {
        const int e = j - 2 * W - 2;
        const size_t q = (size_t)t * c.n_e + e, o = (size_t)(t + 1) * c.G + (size_t)e * c.n_a;
        double sD = Dseq[o];
        D0own[q] = sD;
        for (int m = 0; m < Sact; m++) sD += Dvirt[q * 64 + m];
        Dseq[o] = sD;
    }
}

// (G,P,N) col-major export of one pass's dpol [P][groups][G][D] into columns [n0, n0+N)
__global__ void k_xexport_dpol(const double *dpol, int G, int P, int groups, int D, int n0, int N, double *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)G * P * N;
    if (idx >= total) return;
    const size_t n = idx / ((size_t)G * P), rem = idx - n * (size_t)G * P, t = rem / G, pt = rem - t * G;
    const int x = (int)n / D, k = (int)n - x * D;
    out[((size_t)(n0 + n) * P + t) * G + pt] = dpol[(((size_t)t * groups + x) * G + pt) * D + k];
}

}  // namespace hank
