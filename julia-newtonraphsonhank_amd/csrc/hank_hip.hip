// hank_hip.hip — context, hipGraph-captured sweeps and the C ABI (include/hank_hip.h) of the
// MI355X household block. Both sweeps are strict recurrences in t (value_t needs value_{t+1},
// D_t needs D_{t-1}); every period is one kernel whose X half of period t-1 is fused behind the
// Y half of period t, so the loop-carried state only crosses a launch boundary once per period,
// and the 2(T-1) dependent launches are replayed from hipGraphs (no host launch cost).
#include "hank_kernels.h"
#include "hank_xsweep.h"
#include "hank_xspec.h"
#include "hank_jacobian.h"
#include "hank_wide.h"
#include "hank_hetx.h"
#include "hank_groups.h"
#include "hank_scen.h"
#include "hank_ssbatch.h"
#include "hank_adjoint.h"
#include "hank_boundary.h"
#include "hank_shock.h"
#include "hank_income.h"
#include "hank_borrow.h"
#include "hank_ssdiff_launch.h"
#include "../../include/hank_hip.h"
#include "../../include/hank_hip_borrow.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <list>
#include <mutex>
#include <new>
#include <vector>

using namespace hank;

// Who owns device memory and graph handles: ONE move-only owner type. An Owner holds a handle or nothing, releases it in its
// destructor and before it takes another, and converts to the handle where one is read (kernel arguments, copies, launches).
// DevBuf<T> is the owner of one device allocation, GraphExec the owner of one instantiated graph; every other pointer to device
// memory in this file is a view into one of them.
struct FreeDevice { void operator()(void *p) const { (void)hipFree(p); } };
struct FreeGraphExec { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); } };
template <typename H, typename Release>
struct Owner {
    Owner() = default;
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    Owner(Owner &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owner &operator=(Owner &&o) noexcept { if (this != &o) { reset(o.h); o.h = nullptr; } return *this; }
    ~Owner() { reset(); }
    void reset(H next = nullptr) { if (h) Release()(h); h = next; }
    H get() const { return h; }
    operator H() const { return h; }
protected:
    H h = nullptr;
};
using GraphExec = Owner<hipGraphExec_t, FreeGraphExec>;
template <typename T>
struct DevBuf : Owner<T *, FreeDevice> {
    // count elements (8 bytes for none: every buffer has an address); what the buffer held before is released first
    hipError_t alloc(size_t count) {
        this->reset();
        return hipMalloc((void **)&this->h, count * sizeof(T) > 0 ? count * sizeof(T) : 8);
    }
};
// a slab is carved into 256-byte aligned pieces: the offset of the next piece of `bytes`
static size_t carve(size_t &off, size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }

// Lane geometry of the tangent kernels, chosen per batch width N (measured, MI355X, 2000x11, T=300):
//  - lane width: an even batch runs TWO adjacent directions per lane (double2): every state / dpol access is
//    16 bytes, half the vector-memory instructions per byte (N=32: 4650 -> 5380 JVPs/s; N=256: 8130 -> 10940);
//  - wealth-row groups per wave: backward 2 (4 from 256 directions on) — its gathers are independent, more
//    groups = more bytes in flight per wave; forward 2 for 16-lane groups (N = 18..32, which run the
//    source-stationary form of the forward kernel, see ensure_tanwork) and from N = 64 on, 1 otherwise.
static inline int tan_rg(int NV, int forward, int ss = 0) {   // NV = lanes' worth of directions
    const char *e = getenv(forward ? "HANK_RG_F" : "HANK_RG_B");   // dev knobs
    if (e) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) return v; }
    return forward ? ((NV >= 32 || ss) ? 2 : 1) : (NV >= 128 ? 4 : 2);
}
static inline int tan_lane_width(int N, int forward) {
    const char *e = getenv(forward ? "HANK_LANE_WIDTH_F" : "HANK_LANE_WIDTH_B");   // dev knobs
    const int want = e ? atoi(e) : 2;
    return (want == 2 && N % 2 == 0) ? 2 : 1;
}

// Which exogenous path the household block runs under: the discount factors beta_t (hank_shock.h), income by
// productivity state y_t[e] (hank_income.h) or the borrowing limit amin_t (hank_borrow.h). What differs between the kinds on the host is stated HERE, once; everything below indexes
// by kind. The context owns the path in force (hank_ctx::path, set_path); the kinds exclude each other.
enum PathKind { PATH_NONE, PATH_DISCOUNT, PATH_INCOME, PATH_BORROW };
constexpr int N_PATH_KINDS = 4;
struct hank_ctx;
typedef int (*VjpRule)(hank_ctx *, int, const void *, int, const void *);
static int vjp_args(hank_ctx *ctx, int n_het, const void *in, int M, const void *out);
static int vjp_het_args(hank_ctx *ctx, int n_het, const void *in, int M, const void *out);
struct PathTraits {
    const char *a_path;                     // the kind, as the messages name a path of it
    const char *set, *jvp, *vjp, *fn;       // its entries, as the messages name them (set: also the clearing hint, `set(ctx, NULL) clears it`)
    const char *dir, *bar;                  // its directions and its cotangent among their arguments
    const char *refusal;                    // what an entry that is not served at a path of this kind says of itself (refuses_at)
    unsigned excluded_under;                // the kinds (one bit each, 1u << kind) under whose path its jvp / vjp entries refuse (path_entry_excluded)
    VjpRule vjp_rule;                       // the argument rule of its vjp entry
};
static const PathTraits PATHS[N_PATH_KINDS] = {
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, nullptr},
    {"a discount-factor path", "hank_set_discount_path", "hank_jvp_shock", "hank_vjp_shock", "hank_fake_news_shock", "dbeta", "beta_bar",
     "is defined at one discount factor", 1u << PATH_BORROW, vjp_het_args},
    {"an income path", "hank_set_income_path", "hank_jvp_income", "hank_vjp_income", "hank_fake_news_income", "dy", "y_bar",
     "is not served at an income path", (1u << PATH_DISCOUNT) | (1u << PATH_BORROW), vjp_args},
    {"a borrowing-limit path", "hank_set_borrow_path", "hank_jvp_borrow", "hank_vjp_borrow", "hank_fake_news_borrow", "damin", "amin_bar",
     "is defined at one borrowing limit", (1u << PATH_DISCOUNT) | (1u << PATH_INCOME), vjp_het_args},
};
// values per period (beta_t, amin_t: 1; y_t[e]: n_e), and the value of every period without a path (the model's beta; zero; the model's limit)
static int path_width(const Consts &c, PathKind k) { return k == PATH_INCOME ? c.n_e : 1; }
static double path_neutral(const Consts &c, PathKind k) { return k == PATH_DISCOUNT ? c.beta : k == PATH_BORROW ? c.bc : 0.0; }

// a kind's share of a tangent workspace, allocated on its first use at this width (ensure_path_tan_graph): the caller's directions as they
// come — dbeta (P, N), dy (n_e, P, N), damin (P, N), column-major (staging) — the same as [P][N] / [P][n_e][N] (k_shk_in, k_inc_in), and the backward
// sweep with the seed of every period between its launches
struct PathSeed { DevBuf<double> in, dir; GraphExec g_tback; };

struct TanWork {
    int N = 0;
    TanGeom g{}, gf{};   // lane geometry of the backward / forward tangent kernels
    DevBuf<double> dxhh;      // (2,P,N) staging for the host-pointer entry
    DevBuf<double> dxr, dxw, dxt;   // [P][N] tangents of r, w (, lump-sum transfer)
    DevBuf<double> ds[2];
    DevBuf<double> dD[2];
    DevBuf<double> dpol;
    DevBuf<double> aggpart;
    DevBuf<double> dagg;      // [P][N]
    DevBuf<double> dagg_cm;   // (P,N) column-major
    int nbx = 0, nbxf = 0;
    GraphExec g_fback, g_ffwd;   // dual-sweep graphs (primal + tangents in one chain)
    // hank_jvp_boundary (hank_boundary.h), allocated on its first use at this width: the caller's seeds (G, N) column-major,
    // m_{-1} [N][n_e], {zm, om} [2][P][N]
    DevBuf<double> bnd_dV, bnd_dD, bnd_m0, bnd_zm;
    // hank_jvp_het, allocated on its first use at this width: the (P, n_het, N) result and, for n_het > 2,
    // the extra slots' partials [P][nbf][NX][N] and sums T [N][P][NX] (sized for the family's count)
    DevBuf<double> hx_parts, hx_T, het_out;
    int VB = 1, VF = 1, RGB = 1, RGF = 1;   // lane widths and row groups the graphs are captured with
    unsigned nbf = 0;
    // The tangent-only graphs, each captured on its first use at this width, named HERE and nowhere else: bnd — with the boundary's
    // seed kernels in them (hank_boundary.h); NX — the forward sweep with that many extra reductions (hank_jvp_het, n_het = 2 + NX)
    // The path kinds' seeds and backward graphs (hank_jvp_shock, hank_jvp_income, the two Toeplitz entries), by kind: each kind has its
    // OWN buffers and graph, so the kinds alternate at one width without touching each other's ([PATH_NONE] stays empty: tan_back)
    PathSeed seed[N_PATH_KINDS];
    GraphExec &tan_back(bool bnd) { return g_tback[bnd]; }
    GraphExec &tan_fwd(bool bnd, int NX) { return g_tfwd[bnd][NX]; }
private:
    GraphExec g_tback[2], g_tfwd[2][3];
};

// ---- XCD-local persistent sweeps (hank_xsweep.h): per-context workspace and per-batch-width tangent buffers ----
constexpr int XD_MAX = 4;           // directions per group and pass (D = 8 spills registers: wider batches run as passes)
constexpr int XPASS_MAX = 64;       // passes per call: N <= 8 * XD_MAX * XPASS_MAX = 2048 directions
struct XPass { int n0, N, D, groups; size_t dpol_off; };
struct XTan {                       // one per batch width N (kept in a small LRU: Jacobian assembly and Newton alternate widths)
    int N = 0;
    std::vector<XPass> passes;
    DevBuf<double> dxhh, dxr, dxw, dxt;   // staging + [P][N] input tangents
    DevBuf<double> dpol;            // per pass [P][groups][G][D]
    DevBuf<double> daggpart;        // [P][Sact*n_e][XG*XD_MAX] (reused by every pass)
    DevBuf<double> dagg_pass;       // [P][XG*XD_MAX]
    DevBuf<double> dagg_cm;         // (P, N) column-major
};
struct XWork {
    bool ready = false;
    int grid = 0, Sact = 0, maxt = 768, dmax = XD_MAX;
    DevBuf<XSync> sync;             // [2 * XPASS_MAX]: backward and forward sweep of every pass
    DevBuf<double> st_s, st_ds, st_D, st_dD;
    DevBuf<double> Dvirt, aggpart, rho;
    DevBuf<double> D0own;           // [P][n_e] row 0 of every D_t as member 0 held it, before the virtual rows' mass was added (k_xlwg_build)
    DevBuf<int> srcB, srcF;                   // [P][Sact] source-member ranges of the tangent sweeps at the recorded primal
    DevBuf<int2> unitsF;                      // [P][Sact][XUCAP] the forward sweeps' work units (k_xunits_fwd)
    DevBuf<int> unit_overflow;                // set by k_xunits_fwd when a member has more units than XUCAP
    int ucap = 64;                            // dev knob HANK_XUCAP (read once, at hank_create): a smaller budget, to exercise the overflow path
    bool rng_valid = false;                   // srcF / unitsF belong to the recorded lottery
    DevBuf<int2> stageU;                      // [P][Sact][n_e][XU_ROWS] k_xdual_front's staged units per (period, member, column), read by k_xunits_pack
    DevBuf<int4> stageM;                      // [P][Sact][n_e] their {count, source members lo, hi, has virtual lanes}
    bool front = true;                        // knob HANK_XDUAL_FRONT=0 (read once, at hank_create): the one-pass Dual pass keeps k_lottery_lq + k_xunits_fwd in front
    int front_poison = 0;                     // tests only, HANK_XDUAL_FRONT_POISON=1 (read once, at hank_create): the lean front fills what it leaves unwritten (k_xdual_front)
    bool packed = true;                       // dev knob HANK_XFWD_PACKED=0 (read once, at hank_create): the Dual pass's forward sweep reads the three-array record (k_xfwd<D, true>, the
                                              // [lane][SL] tile) — what tests/test_gpu_xfwd_walk.py holds the packed-record instance's slot-major tile against, byte for byte
    bool neigh = true;                        // dev knob HANK_XNEIGH=0 (read once, at hank_create): every period waits for every member
    bool syncwave = true;                     // dev knob HANK_XSYNCWAVE=0 (read once, at hank_create): wave 0 polls instead of an extra wave
    int lds_max = 65536;
    int fault_where = 7;
    int fault = 0;                            // dev knob HANK_XFAULT=placement: every persistent launch finds its status word set ("a
                                              // group is short of members") and leaves at once — exercises the fallback paths
    bool src_valid = false;
    std::list<XTan> tans;           // most recently used first
    int last_blocks = 0;            // sync blocks the last call used, from block 0 (x_status checks their status words)
    int xspec = XSPEC_CRRA;                   // dev knob HANK_XSPEC (read once, at hank_create): which halves of hank_xspec.h's choice are on
    int inst[4] = {-1, -1, -1, -1};           // {NE, CRRA} of the last k_xdual_back and of the last k_xfwd<D, true> enqueued (hank_sweep_instance; -1: none yet)
};

// ---- on-chip wide sweeps (hank_wide.h): tangent buffers per batch width ----
struct WTan {
    int N = 0;
    DevBuf<double> dxhh;            // (n_hh, P, N) the caller's input tangents (staging for the host-pointer entries)
    DevBuf<double> dpol;            // [P][N][G]
    DevBuf<double> dagg_cm;         // (P, N) column-major
};

// ---- transposed sweeps (hank_adjoint.h): hank_vjp's workspace per batch width M (its own: no TanWork's dpol is reused, so the
// current tangent batch stays current and its readers keep serving it) ----
// a kind's share of it: g_B is Sweep B — for a path kind with the path cotangent's partials behind every period's launch (k_shk_bbar,
// k_inc_ybar, k_brw_abar) and their reduction at the end, captured on its first use at this width with the buffers: the partials [P][nb][width][M],
// their sums [P][width][M] and the caller's layout (width, P, M) column-major (width: 1 for beta_bar, n_e for y_bar).
// [PATH_NONE]: hank_vjp's plain Sweep B, captured with Sweep A, and no buffers.
struct PathCot { DevBuf<double> part, rm, cm; GraphExec g_B; };
struct CotWork {
    int N = 0;                      // the batch width M (the cache's key)
    int V = 1;                      // cotangent columns per lane
    AdjGeom g{};
    DevBuf<double> ybar;            // (P, n_het, M) the caller's cotangents (staging for every entry; sized for the family's outputs)
    DevBuf<double> yb0, yb1;                    // [P][M] cotangents of the policy variable's aggregate and of consumption's
    DevBuf<double> ybx;             // [P][NX][M] cotangents of outputs 2 .. (hank_vjp_het), sized for the family's largest NX
    DevBuf<double> st[2];                       // [G][M] ping-pong state: lam in Sweep A, then mu in Sweep B
    DevBuf<double> pbar;            // [P][G][M] the policy cotangent sequence: written once by Sweep A, read once by Sweep B
    DevBuf<double> partS, partM;                // [P][nb][3][M] per-block partial sums of the inputs' cotangents
    DevBuf<double> xbar;            // (n_hh, P, M) column-major
    GraphExec g_A;
    PathCot path[N_PATH_KINDS];     // Sweep B by path kind, each kind with its own buffers: the kinds alternate at one width
    GraphExec g_AX[2];              // Sweep A with NX = 1, 2 extra outputs (hank_vjp_het), captured on first use; Sweep B is the same
    DevBuf<double> gin, gb;         // hank_vjp_group, allocated on its first use at this width: the caller's (P, K, M) cotangents on the group outputs
                                    // (staging) and the same as [P][K][M] (k_adj_in_grp), both at HANK_GROUP_MAX groups
    GraphExec g_AG;                 // Sweep A with the context's groups (k_adj_dist_grp), captured on first use and dropped with the set (GroupSet)
    DevBuf<double> bnd_vbar, bnd_dbar;          // (G, M) column-major the boundary's cotangents (hank_vjp_boundary), allocated on its first use at this width
};
// The current cotangent batch, with the same single owner as the tangent batch: cot_ran / cot_none write, the reader asks cot_current.
struct CotBatch {
    bool current = false;
    int M = 0;
    const void *ws = nullptr;       // view
    const double *pbar = nullptr;   // view
};

// f, f_c and the direction-independent sums of the outputs that are not affine in the policy (2 Value, 3 UCE: k_hx_record), always
// at the family's count SX (hx_count): f, fc [SX][P][G], S [P][SX][HX_NS]. They belong to the recorded primal: ensure_hx_record
// builds them for whoever asks first (hx_outputs, enqueue_vjp) and record_rewritten drops them. Allocated at first use and never
// again: the NX > 0 Sweep A graphs hold the addresses.
struct HxRecord { DevBuf<double> f, fc, S; bool valid = false; };

// The caller's group outputs (hank_set_group_outputs; hank_groups.h): K weight vectors W (G, K) and their bases, owned by the context,
// and their share of the record — the levels Y [P][K] and the CONS sums S [P][K][GRP_NS] (k_grp_record) — which belongs to the recorded
// primal AND to this set of groups: ensure_grp_record builds it for the first reader, record_rewritten and a new set drop it. slab:
// the direction-dependent buffers of hank_get_group_outputs, grown to the widest request.
// hank_vjp_group's Sweep A graphs (CotWork::g_AG, one per cached width) hold K, the bases and the addresses of W and of the cotangents:
// hank_set_group_outputs drops the group graph of EVERY cached width (after its stream synchronisation), so the next hank_vjp_group
// captures against the new set. Nothing else of a CotWork depends on the groups.
struct GroupSet {
    int K = 0;
    DevBuf<double> W, Y, S;
    DevBuf<int> base;
    unsigned long long codes = 0;      // the bases as k_grp_mix takes them (grp_codes)
    bool valid = false;
    DevBuf<char> slab;
    size_t bytes = 0;
};

// hank_primal_batch's workspace (hank_scen.h): K scenario records carved alike from ONE slab (R0 is scenario
// 0's, `stride` bytes to the next), the scenarios' inputs, partial sums, error words and outputs, and the two graphs of the last
// (K, n_het) that ran. Grown to the widest K asked for (build_scenwork into a local, moved in when complete: a failed allocation
// leaves the context's workspace as it was); freed with the context.
struct ScenWork {
    int K = 0;                         // scenarios the buffers hold
    int gK = 0, g_nhet = 0;            // what the graphs were captured for (gK = 0: none)
    Record R0{};                       // views into slab (seg, lwg: null — no reader of either runs on a scenario)
    size_t stride = 0;
    DevBuf<char> slab;
    DevBuf<double> xhh;                // (n_hh, P, K)
    DevBuf<double> aggpart, agg_rm;    // [k][t][block][2], [k][t][2]
    DevBuf<double> hxpart, hx_rm;      // [k][t][block][NX], [k][t][NX]
    DevBuf<double> out;                // (P, n_het, K)
    DevBuf<int> err;                   // [K][4]
    GraphExec g_back, g_fwd;
};

// The current tangent batch: at most ONE is current, and it belongs to the recorded primal. Written by batch_ran ("family F has
// just run a batch on workspace W") and batch_none ("nothing is current") only; the readers ask batch_current.
struct TanBatch {
    int family = 0;                 // which family ran the last tangent sweep (0 launches, 1 persistent, 2 wide): kept for hank_info when nothing is current
    bool current = false;
    int N = 0;
    const void *ws = nullptr;       // view: the cache entry that holds it (its eviction makes nothing current)
    const double *dagg_cm = nullptr, *dpol = nullptr;     // views: the family's (P, 2 N) tangents of the aggregates and its policy partials
    const std::vector<XPass> *passes = nullptr;           // persistent family: how dpol is laid out
    bool boundary = false;          // the batch carries boundary seeds (hank_jvp_boundary): its dD_0 is not zero, so only outputs 0 and 1 are served
    const double *bnd_zm = nullptr; // view: {zm, om} [2][P][N] of its dD_0 seed (k_bnd_mpath), or nullptr without one
    const double *inc_dy = nullptr; // view: the dy (n_e, P, N) column-major of a batch hank_jvp_income seeded with one, or nullptr: consumption's tangent has
                                    // a direct term in it, so the readers that rebuild c from the inputs refuse such a batch and hank_get_het_outputs adds the term
};

// The timed sweeps of hank_last_timings (the first six, in its slot order), hank_last_vjp_timings (the next two) and
// hank_last_ss_timings (the next two), hank_last_batch_timings (the next two) and hank_last_ss_batch_timings (the last two). A span is a
// begin event, an end event, a valid flag and the launch count of the run that ended it; the run functions reach them through these
// operations only. Recording a span's begin makes it invalid until its end is recorded. What each run function leaves behind
// (V valid, I invalid, . untouched) — the families do NOT agree, see DESIGN.md section 2a:
//                        PRIMAL_BACK PRIMAL_FWD TAN_BACK TAN_FWD DUAL_BACK DUAL_FWD VJP_A VJP_B SS_VALUE SS_DIST
//   run_primal                V          V         .        .        I        I       .     .      .       .
//   x_primal                  V          V         I        I        I        I       .     .      .       .
//   x_jvp                     .          .         V        V        I        I       .     .      .       .
//   x_dual_two                V          I         V        V        I        I       .     .      .       .
//   x_dual_fused              V          I         V*       V        I        I       .     .      .       .      (* brackets nothing: k_xdual_back is PRIMAL_BACK's)
//   w_run_tangent             .          .         V        V        I        I       .     .      .       .
//   run_jvp                   .          .         V        V        .        .       .     .      .       .
//   run_fused                 I          I         I        I        V        V       .     .      .       .
//   enqueue_vjp               .          .         .        .        .        .       V     V      .       .
//   ss_loop                   .          .         .        .        .        .       .     .      V       V      (the loop it was called for; I until that loop's end)
//   primal_batch              .          .         .        .        .        .       .     .      .       .      (its own two, SCEN_BACK and SCEN_FWD: V)
//   ss_batch                  .          .         .        .        .        .       .     .      .       .      (its own two, SSB_VALUE and SSB_DIST: V; SSB_DIST I without a distribution)
enum Span { PRIMAL_BACK, PRIMAL_FWD, TAN_BACK, TAN_FWD, DUAL_BACK, DUAL_FWD, VJP_A, VJP_B, SS_VALUE, SS_DIST, SCEN_BACK, SCEN_FWD, SSB_VALUE, SSB_DIST, N_SPANS };
struct Spans {
    struct One { hipEvent_t ev0 = nullptr, ev1 = nullptr, from = nullptr; bool valid = false; int launches = 0; } s[N_SPANS];      // from: the event the span began with (ev0, or the end of the span before it)
    hipError_t create() { hipError_t e = hipSuccess; for (One &o : s) { if (e == hipSuccess) e = hipEventCreate(&o.ev0); if (e == hipSuccess) e = hipEventCreate(&o.ev1); } return e; }
    void destroy() { for (One &o : s) { if (o.ev0) (void)hipEventDestroy(o.ev0); if (o.ev1) (void)hipEventDestroy(o.ev1); } }
    hipError_t begin(Span k, hipStream_t st) { s[k].valid = false; s[k].from = s[k].ev0; return hipEventRecord(s[k].ev0, st); }
    hipError_t end(Span k, hipStream_t st, int launches) { const hipError_t e = hipEventRecord(s[k].ev1, st); s[k].launches = launches; s[k].valid = e == hipSuccess; return e; }
    // ONE event ends span k and begins span next
    hipError_t end_begin(Span k, int launches, Span next, hipStream_t st) { s[next].valid = false; s[next].from = s[k].ev1; return end(k, st, launches); }
    void invalidate(std::initializer_list<Span> ks) { for (Span k : ks) s[k].valid = false; }
    void absent(Span k, int launches) { s[k].valid = false; s[k].launches = launches; }      // the sweep rode on another span's launch: no events
    // after a synchronisation: -1 ms for an invalid span; the launch count of the last run that ended it either way
    hipError_t read(Span k, double *ms, int32_t *launches) const {
        float f = -1.f;
        const hipError_t e = s[k].valid ? hipEventElapsedTime(&f, s[k].from, s[k].ev1) : hipSuccess;
        *ms = e == hipSuccess ? f : -1.0;
        if (launches) *launches = s[k].launches;
        return e;
    }
};
// the slots of hank_stats, named as hip.py names them (SCHEDULE is filled from the context's schedule when it is read)
enum Stat { SWEEP_LAUNCHES, TANGENT_WORKSPACES_ALLOCATED, GRAPHS_CAPTURED, SCHEDULE, FALLBACKS, VFI_ITERATIONS, PRIMAL_MEMO_HITS, PRIMAL_SWEEPS, N_STATS };

struct hank_ctx {
    int device = 0;
    Consts c{};                    // (c.a, c.z, c.Pi: views of d_a, d_z, d_Pi)
    Record R{};                    // views: every member points into rec_slab
    int T = 0;
    DevBuf<double> d_a, d_z, d_Pi;
    DevBuf<double> d_ss_value;
    double *d_ss_D = nullptr;      // view: aliases R.Dseq[0]
    DevBuf<double> d_xhh, d_agg, d_aggpart;     // d_agg: (P, 2) column-major — the policy-weighted aggregate, then the grid-weighted one
    DevBuf<double> d_agg_rm;        // [P][2] as the reduction leaves it
    DevBuf<double> d_zd;            // [2][P]: sum_e z_e m_t(e) and sum_e m_t(e), m_t = Pi' m_{t-1} the productivity marginal of D_t (hank_get_het_outputs)
    DevBuf<int> d_err;
    int nbp = 0;  // row blocks of the primal kernels
    bool boundary_set = false, primal_done = false;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // the primal forward sweep runs on a side stream, concurrently with the tangent backward sweep (both only
    // need the primal backward record); ev_side marks its completion, side_pending = the main stream has not
    // been made to wait for it yet
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_side = nullptr;
    bool side_pending = false;
    GraphExec g_pfwd;              // the primal forward sweep (every kind's: it does not know a path)
    // The exogenous paths, one ExoPath per kind: d — beta_t [P] / y_t[e] [P][n_e] — ALWAYS holds the values in
    // force, the kind's neutral value in every period while no path of it is set (the graphs hold its address); h is its host copy;
    // g_pback is the backward primal graph that reads it (capture_primal_back, captured at the first primal under a path of the kind).
    // exo[PATH_NONE] has no values: its g_pback is the model's own backward graph. `path` says which kind is in force — at most one:
    // set_path alone writes it, and it and the refusals next to it alone ask. A path in force keeps everything that (re)writes the
    // record on the per-period launches.
    // The income kind's alone: d_inc_m [P][n_e], the column masses of the recorded distributions (k_inc_mass) — the direct term of
    // y_t[e] in consumption — valid for the recorded primal or not (inc_m_valid, ensure_inc_mass; record_rewritten drops it).
    struct ExoPath { DevBuf<double> d; std::vector<double> h; GraphExec g_pback; } exo[N_PATH_KINDS];
    PathKind path = PATH_NONE;
    DevBuf<double> d_inc_m;
    bool inc_m_valid = false;
    Spans spans;                   // the timed sweeps (hank_last_timings, hank_last_vjp_timings, hank_last_ss_timings)
    std::list<TanWork> tws;        // per batch width, most recently used first (a small cache: Jacobian assembly and Newton alternate widths)
    // 0 = one launch per period for everything; 1 = XCD-local persistent sweeps for everything; 2 = auto (default where
    // the persistent sweeps are supported): each entry point takes the faster of the two for its shape — see sched_*
    int schedule = 2;
    bool forced_xcd = false;       // HANK_SCHEDULE=xcd at hank_create: no silent fallback to the launches
    TanBatch batch;                // the current tangent batch (hank_get_dpolicy_seq, hank_get_grid_aggregates, hank_get_het_outputs, hank_info)
    int xjvp_max = 64;             // auto: batches up to this width take the persistent tangent sweeps (measured crossover)
    XWork xw;
    struct { DevBuf<double> dpT, iota, E, Cp, F, Dv, W, dsum; int N = 0, n_het = 0; } fn;   // hank_fake_news[_het] workspace (E, Cp, F, Dv, W, dsum sized for n_het outputs)
    // on-chip wide sweeps: 0 = never, 1 = auto (batches of at least wide_min directions), 2 = every batch (HANK_SCHEDULE=wide: tests)
    int wide_mode = 0, wide_min = 80, num_cus = 256, wide_r = 2;     // wide_r: rows per thread of the wide kernels (2: 1024-thread workgroups, 4 waves per SIMD — since the L2 warming of round 5 the faster geometry for both sweeps, 5.16 / 6.80 ms against 5.30 / 7.10 at N=256; dev knob HANK_WIDE_R=2|4 at hank_create)
    size_t lds_max = 65536;
    DevBuf<char> rec_slab;         // the record's ONE allocation
    size_t rec_bytes = 0;
    int4 *rec_lq = nullptr;        // views into it (HANK_XFWD_LQ; null without): the packed per-source records [P][G] {w, lo, flags} that k_lottery_lq writes in front
    double *rec_iga = nullptr;     // of a persistent Dual pass, and the grid's inverse gaps [n_a] (k_iga_build, once: hank_create)
    DevBuf<int> d_ibw;             // the wide backward sweep's bracket record (k_wide_prep), valid for the recorded primal or not
    bool seg_valid = true;          // the record's per-target segment records match its lottery (k_lottery writes them except in the persistent Dual pass)
    bool lwg_valid = true;          // the record's per-source records {w, ig D} match it (every forward sweep of a primal writes them except the persistent Dual pass's)
    bool lot_valid = true;          // the record's lo, lw, ig and start match its policies (every lottery writes them except the lean front of the one-pass persistent Dual pass: ensure_lottery)
    long long lwg_builds = 0;       // times k_xlwg_build ran (hank_info)
    bool wprep_valid = false;
    std::list<WTan> wtans;         // most recently used first
    std::list<CotWork> cws;        // hank_vjp's workspaces, most recently used first
    CotBatch cot;                  // the current cotangent batch (hank_get_policy_cotangent_seq)
    DevBuf<int> d_adj_sb;          // [P][n_e][n_a + 1] Sweep B's bracket segment starts (k_adj_seg), valid for the recorded primal or not
    bool adj_seg_valid = false;
    DevBuf<double> d_bnd_q;        // [2][P][n_e]: Pi^{t+1} z and Pi^{t+1} 1 (hank_jvp_boundary: ensure_bnd_q), the model's; allocated once (the graphs hold its address)
    HxRecord hx;                   // the extra outputs' share of the record (ensure_hx_record), valid for the recorded primal or not
    GroupSet grp;                  // the group outputs and their share of the record (ensure_grp_record)
    ScenWork scen;                 // hank_primal_batch's workspace
    int scen_pending = 0;          // scenarios of a hank_primal_batch_dev whose verdict hank_check has not taken yet
    std::vector<double> h_Pi, h_z;  // host copies (the wide sweeps take the mixing matrix as a kernel argument)
    double a_top = 0.0;             // a_grid[n_a-1]: the bound on a borrowing-limit path's values (path_values_ok)
    long long stats[N_STATS] = {};   // see Stat and hank_stats
    // primal memo of the host-pointer hank_primal_jvp (NewtonRaphson.jl:91-95 calls JVP(fullFunction, x, y) ~21 times at one x):
    // the x whose linearisation is on record, as the host handed it in
    bool memo_on = true;                              // HANK_PRIMAL_MEMO=0 (read at hank_create) switches it off
    bool xdual_back = true;                           // dev knob HANK_XDUAL_BACK=0 (read at hank_create): a persistent Dual pass runs k_xprimal_back + k_xtan_back instead of k_xdual_back
    bool memo_valid = false;
    std::vector<double> memo_xhh;
    int n_het = 2;                                    // heterogeneous outputs the caller declared (hank_set_het_outputs; a change drops the memo)
    DevBuf<char> hx_slab;                             // the extra outputs' direction-dependent buffers (hx_outputs), grown to the largest request, freed with the context
    size_t hx_bytes = 0;
    bool stationary = false;                          // the recorded primal is the constant steady-state path with the steady state as both boundaries (hank_fake_news)
    std::vector<double> h_ss_value, h_ss_D;           // the boundary as the host handed it in (stationarity check)
    hipEvent_t ev_stream = nullptr;
    char errmsg[512] = {0};
};

static int fail(hank_ctx *ctx, int code, const char *fmt, ...);
// heterogeneous outputs of the context's value-function family: the policy variable, consumption, Value, and UCE where there are
// transfers; the last hx_count of them are not affine in the policy (hank_hetx.h)
static int het_max(const hank_ctx *ctx) { return ctx->c.n_hh > 2 ? 4 : 3; }
static int hx_count(const hank_ctx *ctx) { return het_max(ctx) - 2; }
static void batch_none(hank_ctx *ctx) { ctx->batch.current = false; ctx->batch.ws = nullptr; }
static void cot_none(hank_ctx *ctx) { ctx->cot = CotBatch(); }
static void cot_ran(hank_ctx *ctx, const void *ws, int M, const double *pbar) { ctx->cot = CotBatch{true, M, ws, pbar}; }
static void batch_ran(hank_ctx *ctx, int family, const void *ws, int N, const double *dagg_cm, const double *dpol, const std::vector<XPass> *passes = nullptr) {
    ctx->batch = TanBatch{family, true, N, ws, dagg_cm, dpol, passes};
}
// the same for a batch of hank_jvp_boundary (always the launch family): zm as TanBatch::bnd_zm
static void batch_ran_boundary(hank_ctx *ctx, const void *ws, int N, const double *dagg_cm, const double *dpol, const double *zm) {
    batch_ran(ctx, 0, ws, N, dagg_cm, dpol);
    ctx->batch.boundary = true;
    ctx->batch.bnd_zm = zm;
}
// the same for a batch of hank_jvp_income with income directions: dy as TanBatch::inc_dy, marking the batch batch_ran has just named.
// The income kind alone marks its batches: y_t[e] has a direct term in consumption, beta_t has none in any output
static void batch_ran_income(hank_ctx *ctx, const double *dy) { ctx->batch.inc_dy = dy; }
// every reader's question: is a batch of N directions current?
static int batch_current(hank_ctx *ctx, int N, const TanBatch **out) {
    if (!ctx->batch.current || ctx->batch.N != N) return fail(ctx, HANK_ERR_NOT_READY, "no tangent sweep with N=%d is current", N);
    *out = &ctx->batch;
    return HANK_OK;
}
// the record was rewritten (or is about to be, by work already enqueued): what was derived from the old one goes, and so does the
// batch. seg_written: the per-target segment records were written with it (k_lottery writes them except in the persistent Dual pass);
// lwg_written: so were the per-source records {w, ig D} (the forward sweep writes them except the persistent Dual pass's);
// lot_written: so were lo, lw, ig and start (every lottery but k_xdual_front's) — seg and lwg are made from them, so neither is valid without
static void record_rewritten(hank_ctx *ctx, bool seg_written, bool lwg_written, bool lot_written = true) {
    ctx->primal_done = true; ctx->seg_valid = seg_written && lot_written; ctx->lwg_valid = lwg_written && lot_written; ctx->lot_valid = lot_written;
    ctx->wprep_valid = false; ctx->xw.src_valid = false; ctx->xw.rng_valid = false; ctx->adj_seg_valid = false; ctx->hx.valid = false; ctx->grp.valid = false; ctx->inc_m_valid = false;
    batch_none(ctx);
    cot_none(ctx);
}
// the record is gone (a new boundary, a persistent sweep that did not run): the next tangent sweep needs a primal first
static void record_gone(hank_ctx *ctx) {
    record_rewritten(ctx, false, false);
    ctx->primal_done = false;
}
static hipError_t join_side(hank_ctx *ctx) {
    if (!ctx->side_pending) return hipSuccess;
    ctx->side_pending = false;
    return hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0);
}

static int fail(hank_ctx *ctx, int code, const char *fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->errmsg, sizeof(ctx->errmsg), fmt, ap);
        va_end(ap);
    }
    return code;
}

// every entry that takes a count of heterogeneous outputs: above the family's count is a bad argument; above the declared count
// (where the entry serves declared outputs only) the caller has to declare them first. rest_ok: the entry's other arguments, refused
// in the same check as the count
static int het_count_ok(hank_ctx *ctx, const char *who, int n_het, bool declared, bool rest_ok = true) {
    const int max_het = het_max(ctx);
    if (n_het < 1 || n_het > max_het || !rest_ok)
        return fail(ctx, HANK_ERR_BAD_ARG, "%s: bad argument: n_het must be 1..%d (the policy variable, consumption, Value%s), got %d", who, max_het, max_het > 3 ? ", UCE" : "", n_het);
    if (declared && n_het > ctx->n_het)
        return fail(ctx, HANK_ERR_NOT_READY, "%s: %d outputs asked for, %d declared: call hank_set_het_outputs first", who, n_het, ctx->n_het);
    return HANK_OK;
}

static int hip_status(hipError_t e) {
    if (e == hipErrorOutOfMemory) return HANK_ERR_NOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNotInitialized || e == hipErrorInsufficientDriver) return HANK_ERR_NO_DEVICE;
    return HANK_ERR_LAUNCH;
}
#define HIPC(ctx, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(ctx, hip_status(e_),                                                   \
                        "HIP error %d (%s) at %s:%d: %s", (int)e_, hipGetErrorString(e_),       \
                        __FILE__, __LINE__, #call);                                             \
    } while (0)

// a context belongs to ONE HIP device (hank_create: the current one; hank_create_on: the one named). Every entry point
// makes that device current for the duration of the call and restores the caller's, so one host thread can drive one
// context per GPU of a node (GeneralStructures.jl:542-550 has no notion of a device: the shim owns the placement).
struct DeviceGuard {
    int prev = -1;
    bool switched = false, ok = true;
    explicit DeviceGuard(const hank_ctx *ctx);
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
DeviceGuard::DeviceGuard(const hank_ctx *ctx) {
    if (!ctx) return;
    if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
    if (prev != ctx->device) { switched = hipSetDevice(ctx->device) == hipSuccess; ok = switched; }
}
// (a call must never run on the caller's device with another device's pointers: a failed switch fails the call)
#define ENTER(ctx)                                                                                                       \
    DeviceGuard dev_guard_(ctx);                                                                                         \
    if (!dev_guard_.ok) return fail(ctx, HANK_ERR_NO_DEVICE, "HIP device %d of this context could not be made current", (ctx) ? (ctx)->device : -1)

// the copy-outs of the sweeps' results on stream s: column `col` of d_agg (P, 2), and the N columns of aggregate `col` of a family's
// dagg_cm (P, 2 N) — both column-major; a null destination asks for nothing
static hipError_t copy_agg(hank_ctx *ctx, double *dst, hipMemcpyKind kind, hipStream_t s, int col = 0) {
    const size_t P = ctx->c.P;
    return dst ? hipMemcpyAsync(dst, ctx->d_agg + P * col, sizeof(double) * P, kind, s) : hipSuccess;
}
static hipError_t copy_dagg(hank_ctx *ctx, double *dst, const double *dagg_cm, int N, hipMemcpyKind kind, int col = 0) {
    const size_t PN = (size_t)ctx->c.P * N;
    return dst ? hipMemcpyAsync(dst, dagg_cm + PN * col, sizeof(double) * PN, kind, ctx->stream) : hipSuccess;
}

static size_t primal_lds(const Consts &c) { return sizeof(double) * ((size_t)c.n_e * RBP + (size_t)c.n_e * c.n_e + 16); }

// ---- graph construction -----------------------------------------------------------------------
static int end_capture(hank_ctx *ctx, GraphExec *out) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HIPC(ctx, hipStreamEndCapture(ctx->own_stream, &graph));
    HIPC(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    out->reset(exec);
    HIPC(ctx, hipGraphDestroy(graph));
    HIPC(ctx, hipGetLastError());
    ctx->stats[GRAPHS_CAPTURED]++;
    return HANK_OK;
}

// the error word starts a run of kernels clean, in stream order (the sweeps, the granular steps, the steady state's fixed points)
static void zero_err(hank_ctx *ctx, hipStream_t s) { hipLaunchKernelGGL(k_zero_i32, dim3(1), dim3(64), 0, s, ctx->d_err, 4); }

// The backward primal graph of one path kind, the chain written ONCE: the error word cleared, X of the last period from the terminal
// value, then P fused Y;X steps, then the lottery. Only the two EGM launches differ by kind: PATH_NONE the model's own; PATH_DISCOUNT
// (hank_shock.h) beta_t' from the kind's values in the X half of period t'; PATH_INCOME (hank_income.h) y_t[e] in both halves;
// PATH_BORROW (hank_borrow.h) amin_t in the Y half of period t.
static int capture_primal_back(hank_ctx *ctx, PathKind kind) {
    const Consts &c = ctx->c;
    const int P = c.P;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp);
    const size_t lds = primal_lds(c);
    const double *v = ctx->exo[kind].d.get(), *x_last = ctx->d_xhh + c.n_hh * (P - 1);
    double *s_last = ctx->R.s + (size_t)(P - 1) * c.G, *kc_last = ctx->R.kc + (size_t)(P - 1) * c.G;
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    zero_err(ctx, s);
    switch (kind) {
    case PATH_NONE: hipLaunchKernelGGL(k_egm_X, grd, blk, lds, s, c, ctx->d_ss_value, x_last, s_last, kc_last, ctx->d_err, P - 1, (const int *)nullptr); break;
    case PATH_DISCOUNT: hipLaunchKernelGGL(k_shk_egm_X, grd, blk, lds, s, c, v, ctx->d_ss_value, x_last, s_last, kc_last, ctx->d_err, P - 1); break;
    case PATH_INCOME: hipLaunchKernelGGL(k_inc_egm_X, grd, blk, lds, s, c, v, ctx->d_ss_value, x_last, s_last, kc_last, ctx->d_err, P - 1); break;
    case PATH_BORROW: hipLaunchKernelGGL(k_egm_X, grd, blk, lds, s, c, ctx->d_ss_value, x_last, s_last, kc_last, ctx->d_err, P - 1, (const int *)nullptr); break;      // (no bc in the X half)
    }
    for (int t = P - 1; t >= 0; t--)
        switch (kind) {
        case PATH_NONE: hipLaunchKernelGGL(k_egm_step, grd, blk, lds, s, c, ctx->R, ctx->d_xhh, t, ctx->d_err); break;
        case PATH_DISCOUNT: hipLaunchKernelGGL(k_shk_egm_step, grd, blk, lds, s, c, ctx->R, ctx->d_xhh, v, t, ctx->d_err); break;
        case PATH_INCOME: hipLaunchKernelGGL(k_inc_egm_step, grd, blk, lds, s, c, ctx->R, ctx->d_xhh, v, t, ctx->d_err); break;
        case PATH_BORROW: hipLaunchKernelGGL(k_brw_egm_step, grd, blk, lds, s, c, ctx->R, ctx->d_xhh, v, t, ctx->d_err); break;
        }
    hipLaunchKernelGGL(k_lottery, dim3(P * c.n_e), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s, c, ctx->R, P * c.n_e, ctx->d_err, 1, 1);
    return end_capture(ctx, &ctx->exo[kind].g_pback);
}
// the model's own pair: backward without a path, and the forward graph every kind shares
static int build_primal_graphs(hank_ctx *ctx) {
    const Consts &c = ctx->c;
    const int P = c.P;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp);
    const int rc = capture_primal_back(ctx, PATH_NONE);
    if (rc) return rc;
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int t = 0; t < P; t++)
        hipLaunchKernelGGL(k_dist_step, grd, blk, primal_lds(c), s, c, ctx->R, t, ctx->d_aggpart);
    hipLaunchKernelGGL(k_reduce_parts, dim3(P, 1), dim3(256), 0, s, ctx->d_aggpart, ctx->nbp, 2, ctx->d_agg_rm);
    hipLaunchKernelGGL(k_tan_out, dim3((2 * P + 255) / 256), dim3(256), 0, s, ctx->d_agg_rm, P, 2, ctx->d_agg);
    return end_capture(ctx, &ctx->g_pfwd);
}
// the graphs a primal on the launches needs under `kind`: a path kind's backward graph is captured the first time a primal runs under it
static int ensure_primal_graphs(hank_ctx *ctx, PathKind kind) {
    if (!ctx->exo[PATH_NONE].g_pback) { const int rc = build_primal_graphs(ctx); if (rc) return rc; }
    return ctx->exo[kind].g_pback ? (int)HANK_OK : capture_primal_back(ctx, kind);
}

// Captures the four tangent graphs for lane type VT (double: one direction per lane; double2: two).
// the row-group count is a template parameter of the kernels and a run-time choice here
#define LAUNCH_RG(RGV, KERNEL, VTYPE, ...)                                                      \
    do {                                                                                        \
        if ((RGV) == 4) hipLaunchKernelGGL((KERNEL<4, VTYPE>), __VA_ARGS__);                    \
        else if ((RGV) == 2) hipLaunchKernelGGL((KERNEL<2, VTYPE>), __VA_ARGS__);               \
        else hipLaunchKernelGGL((KERNEL<1, VTYPE>), __VA_ARGS__);                               \
    } while (0)

#define LAUNCH_RG_SS(RGV, SSV, KERNEL, VTYPE, ...)                                              \
    do {                                                                                        \
        if (SSV) {                                                                              \
            if ((RGV) == 4) hipLaunchKernelGGL((KERNEL<4, VTYPE, true>), __VA_ARGS__);          \
            else if ((RGV) == 2) hipLaunchKernelGGL((KERNEL<2, VTYPE, true>), __VA_ARGS__);     \
            else hipLaunchKernelGGL((KERNEL<1, VTYPE, true>), __VA_ARGS__);                     \
        } else {                                                                                \
            if ((RGV) == 4) hipLaunchKernelGGL((KERNEL<4, VTYPE, false>), __VA_ARGS__);         \
            else if ((RGV) == 2) hipLaunchKernelGGL((KERNEL<2, VTYPE, false>), __VA_ARGS__);    \
            else hipLaunchKernelGGL((KERNEL<1, VTYPE, false>), __VA_ARGS__);                    \
        }                                                                                       \
    } while (0)

// The launch family's graphs of one batch width, ONE capture per sweep, each on its first use (ensure_tan_graphs,
// ensure_dual_graphs). VT / VF: the lane type of the backward / forward kernels (double: one direction per lane; double2: two).
// the pair every forward tangent graph ends with: the partials' sums, then (P, 2 N) column-major
static void launch_tan_reduce(hank_ctx *ctx, TanWork &w, hipStream_t s) {
    const int P = ctx->c.P, N = w.N;
    hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)P, (2 * N + 63) / 64), dim3(256), 0, s, w.aggpart, (int)w.nbf, 2 * N, w.dagg);
    hipLaunchKernelGGL(k_tan_out, dim3((2 * P * N + 255) / 256), dim3(256), 0, s, w.dagg, P, 2 * N, w.dagg_cm);
}
// the grid of the boundary's layout kernels (k_bnd_in)
static dim3 bnd_grid(const Consts &c, int N) { return dim3((unsigned)((c.n_a + BND_T - 1) / BND_T), (unsigned)((N + BND_T - 1) / BND_T), (unsigned)c.n_e); }

// the backward tangent sweep; bnd: with the dV_P seed (hank_boundary.h: the same launches of the same kernel, the seed kernels between them)
// kind (never with bnd): a path kind's seed of EVERY period — d beta_t (hank_shock.h), d y_t[e] (hank_income.h) — behind the launch that produced
// that period's knots' tangent — P launches more, and the kind's layout kernel in front; w.seed[kind]'s buffers are allocated before this.
// d amin_t (hank_borrow.h) is seeded behind the launch that wrote dpol_t — the P launches of the loop — and touches dpol_t and ds_{t-1}.
static size_t brw_seed_lds(const Consts &c, int N) {      // k_brw_seed_back's staging, or 0 where it does not fit (it reads global memory then)
    const size_t b = sizeof(double) * ((size_t)c.n_e * c.n_e + (size_t)N);
    return b <= 48 * 1024 ? b : 0;
}
static size_t inc_seed_lds(const Consts &c, int N) {      // k_inc_seed_back's staging, or 0 where it does not fit (it reads global memory then)
    const size_t b = sizeof(double) * ((size_t)c.n_e * c.n_e + 2 * (size_t)c.n_e * N);
    return b <= 48 * 1024 ? b : 0;
}
template <typename VT>
static int capture_tan_back(hank_ctx *ctx, TanWork &w, bool bnd, PathKind kind = PATH_NONE) {
    const Consts &c = ctx->c;
    const size_t P = c.P;
    const int N = w.N, PN = (int)(P * N), RGB = w.RGB;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e);
    const unsigned ny = (w.g.N + w.g.NC - 1) / w.g.NC, nbt = (w.nbx + RGB - 1) / RGB;
    const VT *dxr = reinterpret_cast<const VT *>(w.dxr.get()), *dxw = reinterpret_cast<const VT *>(w.dxw.get()), *dxt = reinterpret_cast<const VT *>(w.dxt.get());
    VT *ds[2] = {reinterpret_cast<VT *>(w.ds[0].get()), reinterpret_cast<VT *>(w.ds[1].get())};
    VT *dpol = reinterpret_cast<VT *>(w.dpol.get());
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipLaunchKernelGGL(k_tan_in, dim3((PN + 255) / 256), dim3(256), 0, s, w.dxhh, c.n_hh, (int)P, N, w.dxr, w.dxw, w.dxt);
    PathSeed &ps = w.seed[kind];
    const bool seeded = kind != PATH_NONE;
    if (kind == PATH_DISCOUNT || kind == PATH_BORROW) hipLaunchKernelGGL(k_shk_in, dim3((PN + 255) / 256), dim3(256), 0, s, ps.in.get(), (int)P, N, ps.dir.get());
    if (kind == PATH_INCOME) hipLaunchKernelGGL(k_inc_in, dim3((unsigned)(((size_t)PN * c.n_e + 255) / 256)), dim3(256), 0, s, ps.in.get(), c.n_e, (int)P, N, ps.dir.get());
    const dim3 sgrd((unsigned)(((size_t)c.n_a * N + 255) / 256));
    const size_t ilds = inc_seed_lds(c, N), eN = (size_t)c.n_e * N, blds = brw_seed_lds(c, N);
    const bool brw = kind == PATH_BORROW;
    auto seed_brw = [&](int t, double *ds_prev) {      // behind the launch that wrote dpol_t and ds_{t-1} (null at t = 0)
        hipLaunchKernelGGL(k_brw_seed_back, sgrd, dim3(256), blds, s, c, ctx->R, ctx->exo[PATH_BORROW].d.get(), t, ps.dir.get() + (size_t)t * N, (size_t)N, blds ? 1 : 0,
                           w.dpol.get() + (size_t)t * c.G * N, ds_prev);
    };
    auto seed = [&](int t, double *ds_t) {      // ds_t: the knots' tangent of period t, as the launch before left it
        if (kind == PATH_INCOME)
            hipLaunchKernelGGL(k_inc_seed_back, sgrd, dim3(256), ilds, s, c, ctx->R, ctx->d_xhh.get(), t, ps.dir.get() + (size_t)t * eN,
                               t + 1 < (int)P ? ps.dir.get() + (size_t)(t + 1) * eN : (const double *)nullptr, (size_t)N, ilds ? 1 : 0, ds_t);
        else
            hipLaunchKernelGGL(k_shk_seed_back, sgrd, dim3(256), 0, s, c, ctx->R, ctx->d_xhh.get(), ctx->exo[PATH_DISCOUNT].d.get(), t, ps.dir.get() + (size_t)t * N, (size_t)N, ds_t);
    };
    LAUNCH_RG(RGB, k_tan_back, VT, dim3(nbt, ny), blk, 0, s, c, ctx->R, ctx->d_xhh, dxr, dxw, dxt, w.g, (int)P - 1, 1,
                       ds[1], ds[0], dpol);
    if (seeded && !brw) seed((int)P - 1, w.ds[0].get());
    if (bnd) {      // dV_P (BackwardIteration.jl:85) into the knots' tangent of period P-1; ds[1] is free until the next launch writes it
        hipLaunchKernelGGL(k_bnd_in, bnd_grid(c, N), dim3(BND_T, 8), 0, s, w.bnd_dV.get(), c.n_a, c.n_e, c.n_a, N, w.ds[1].get());
        hipLaunchKernelGGL(k_bnd_seed_back, dim3((unsigned)(((size_t)c.n_a * N + 255) / 256)), dim3(256), 0, s, c, ctx->R.kc + (P - 1) * c.G, w.ds[1].get(), (size_t)N, w.ds[0].get());
    }
    int cur = 0;
    for (int t = (int)P - 1; t >= 0; t--) {
        LAUNCH_RG(RGB, k_tan_back, VT, dim3(nbt, ny), blk, 0, s, c, ctx->R, ctx->d_xhh, dxr, dxw, dxt, w.g, t, 0,
                           ds[cur], ds[cur ^ 1], dpol);
        if (brw) seed_brw(t, t > 0 ? w.ds[cur ^ 1].get() : (double *)nullptr);
        else if (seeded && t > 0) seed(t - 1, w.ds[cur ^ 1].get());
        cur ^= 1;
    }
    return end_capture(ctx, seeded ? &ps.g_tback : &w.tan_back(bnd));
}

// the forward tangent sweep; bnd: with the dD_0 seed; NX > 0 (hank_jvp_het): k_tan_fwd_hx in k_tan_fwd's place and k_reduce_hx behind
// the reductions — instantiated for the geometries the defaults launch, the gather form with one row group and the source-stationary
// form with two; a dev knob that asks for another is refused.
// (the seeds' buffers and, for NX > 0, the record's f, f_c and the workspace's hx_parts, hx_T are allocated before this: the graph
// holds their addresses)
template <typename VF, int NX>
static int capture_tan_fwd(hank_ctx *ctx, TanWork &w, bool bnd) {
    const Consts &c = ctx->c;
    const size_t P = c.P, GV = (size_t)(c.n_a + KV) * c.n_e;
    const int N = w.N, PN = (int)(P * N);
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e);
    const unsigned nbf = w.nbf, nyf = (w.gf.N + w.gf.NC - 1) / w.gf.NC;
    VF *dD[2] = {reinterpret_cast<VF *>(w.dD[0].get()), reinterpret_cast<VF *>(w.dD[1].get())};
    VF *dpolf = reinterpret_cast<VF *>(w.dpol.get()), *aggpart = reinterpret_cast<VF *>(w.aggpart.get());
    const bool ss = w.gf.ss != 0;
    if (NX > 0 && !((w.RGF == 1 && !ss) || (w.RGF == 2 && ss)))
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_jvp_het: the forward kernel with extra outputs exists for the default geometries only (got %d row groups, %s form)",
                    w.RGF, ss ? "source-stationary" : "gather");
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    if (bnd) {      // dD_0 (ForwardIteration.jl:293) into the real rows of the state, zero virtual rows; its productivity marginal along the path
        hipLaunchKernelGGL(k_bnd_in, bnd_grid(c, N), dim3(BND_T, 8), 0, s, w.bnd_dD.get(), c.n_a, c.n_e, c.n_a + KV, N, w.dD[0].get());
        hipLaunchKernelGGL(k_bnd_marginal, dim3((unsigned)c.n_e, (unsigned)N), dim3(256), 0, s, w.bnd_dD.get(), c.n_a, c.n_e, w.bnd_m0.get());
        hipLaunchKernelGGL(k_bnd_mpath, dim3((unsigned)((PN + 255) / 256)), dim3(256), 0, s, (int)P, c.n_e, N, w.bnd_m0.get(), ctx->d_bnd_q.get(), w.bnd_zm.get());
    } else
        hipLaunchKernelGGL(k_zero_f64, dim3(512), dim3(256), 0, s, w.dD[0], GV * N);  // dD_0 = 0 (ForwardIteration.jl:293)
    int cur = 0;
    for (int t = 0; t < (int)P; t++) {
        if constexpr (NX == 0) {
            LAUNCH_RG_SS(w.RGF, ss, k_tan_fwd, VF, dim3(nbf, nyf), blk, 0, s, c, ctx->R, w.gf, t, dD[cur], dD[cur ^ 1], dpolf, aggpart);
        } else {
            const TanHx<VF, NX> hx{ctx->hx.f.get(), ctx->hx.fc.get(), reinterpret_cast<VF *>(w.hx_parts.get())};
            if (ss) hipLaunchKernelGGL((k_tan_fwd_hx<2, VF, true, NX>), dim3(nbf, nyf), blk, 0, s, c, ctx->R, w.gf, t, dD[cur], dD[cur ^ 1], dpolf, aggpart, hx);
            else hipLaunchKernelGGL((k_tan_fwd_hx<1, VF, false, NX>), dim3(nbf, nyf), blk, 0, s, c, ctx->R, w.gf, t, dD[cur], dD[cur ^ 1], dpolf, aggpart, hx);
        }
        cur ^= 1;
    }
    launch_tan_reduce(ctx, w, s);
    if (NX > 0) hipLaunchKernelGGL(k_reduce_hx, dim3((unsigned)P, (NX * N + 63) / 64), dim3(256), 0, s, w.hx_parts.get(), (int)nbf, NX, N, (int)P, w.hx_T.get());
    return end_capture(ctx, &w.tan_fwd(bnd, NX));
}

// The dual-sweep graphs (hank_primal_jvp): the primal recurrence and the tangent recurrence advance in the SAME chain of launches,
// the tangent one period behind (it reads the record the previous launch wrote): T launches per direction instead of 2(T-1).
template <typename VT, typename VF>
static int capture_dual_graphs(hank_ctx *ctx, TanWork &w) {
    const Consts &c = ctx->c;
    const size_t P = c.P, GV = (size_t)(c.n_a + KV) * c.n_e;
    const int N = w.N, PN = (int)(P * N), RGB = w.RGB, RGF = w.RGF;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e);
    const unsigned nbf = w.nbf, ny = (w.g.N + w.g.NC - 1) / w.g.NC, nyf = (w.gf.N + w.gf.NC - 1) / w.gf.NC;
    const VT *dxr = reinterpret_cast<const VT *>(w.dxr.get()), *dxw = reinterpret_cast<const VT *>(w.dxw.get()), *dxt = reinterpret_cast<const VT *>(w.dxt.get());
    VT *ds[2] = {reinterpret_cast<VT *>(w.ds[0].get()), reinterpret_cast<VT *>(w.ds[1].get())};
    VF *dD[2] = {reinterpret_cast<VF *>(w.dD[0].get()), reinterpret_cast<VF *>(w.dD[1].get())};
    VT *dpol = reinterpret_cast<VT *>(w.dpol.get());
    VF *dpolf = reinterpret_cast<VF *>(w.dpol.get()), *aggpart = reinterpret_cast<VF *>(w.aggpart.get());
    const unsigned nbt = (w.nbx + RGB - 1) / RGB;
    int cur = 0;
    const dim3 pblk(RBP * c.n_e), pgrd(ctx->nbp);
    const size_t lds = primal_lds(c);
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    zero_err(ctx, s);
    hipLaunchKernelGGL(k_tan_in, dim3((PN + 255) / 256), dim3(256), 0, s, w.dxhh, c.n_hh, (int)P, N, w.dxr, w.dxw, w.dxt);
    hipLaunchKernelGGL(k_egm_X, pgrd, pblk, lds, s, c, ctx->d_ss_value, ctx->d_xhh + c.n_hh * (P - 1),
                       ctx->R.s + (size_t)(P - 1) * c.G, ctx->R.kc + (size_t)(P - 1) * c.G, ctx->d_err, (int)P - 1, (const int *)nullptr);
    for (int k = 0; k <= (int)P; k++) {
        const int tp = k < (int)P ? (int)P - 1 - k : -1;
        if (k == 0) {
            LAUNCH_RG(RGB, k_fused_back, VT, dim3(ctx->nbp + nbt, ny), blk, 0, s, c, ctx->R, ctx->d_xhh, ctx->d_err, tp, ctx->nbp,
                               dxr, dxw, dxt, w.g, (int)P - 1, 1, ds[1], ds[0], dpol);
        } else {
            LAUNCH_RG(RGB, k_fused_back, VT, dim3(ctx->nbp + nbt, ny), blk, 0, s, c, ctx->R, ctx->d_xhh, ctx->d_err, tp, ctx->nbp,
                               dxr, dxw, dxt, w.g, (int)P - k, 0, ds[cur], ds[cur ^ 1], dpol);
            cur ^= 1;
        }
    }
    hipLaunchKernelGGL(k_lottery, dim3(P * c.n_e), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s, c, ctx->R, (int)P * c.n_e, ctx->d_err, 1, 1);
    const int rc = end_capture(ctx, &w.g_fback);
    if (rc) return rc;
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipLaunchKernelGGL(k_zero_f64, dim3(512), dim3(256), 0, s, w.dD[0], GV * N);
    cur = 0;
    for (int k = 0; k <= (int)P; k++) {
        const int tp = k < (int)P ? k : -1, tt = k - 1;
        LAUNCH_RG_SS(RGF, w.gf.ss, k_fused_fwd, VF, dim3(ctx->nbp + nbf, nyf), blk, 0, s, c, ctx->R, tp, ctx->nbp, ctx->d_aggpart, w.gf, tt,
                  dD[cur], dD[cur ^ 1], dpolf, aggpart);
        if (tt >= 0) cur ^= 1;
    }
    hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)P, 1), dim3(256), 0, s, ctx->d_aggpart, ctx->nbp, 2, ctx->d_agg_rm);
    hipLaunchKernelGGL(k_tan_out, dim3((unsigned)((2 * P + 255) / 256)), dim3(256), 0, s, ctx->d_agg_rm, (int)P, 2, ctx->d_agg);
    launch_tan_reduce(ctx, w, s);
    return end_capture(ctx, &w.g_ffwd);
}

// The workspaces of one family for a batch of N directions, from a small most-recently-used cache (Jacobian assembly at N = 256
// and the Newton inner loop at N = 1 alternate: neither re-allocates). On a miss `build` sizes and allocates the new entry
// (its N is set); an entry's members own its device memory and graphs, so dropping the entry releases them.
template <typename W, typename Build>
static int tan_cache_get(hank_ctx *ctx, std::list<W> &cache, int N, Build build, W **out) {
    for (auto it = cache.begin(); it != cache.end(); ++it)
        if (it->N == N) { cache.splice(cache.begin(), cache, it); *out = &cache.front(); return HANK_OK; }
    const char *ce = getenv("HANK_TAN_CACHE");
    const size_t keep = ce ? (size_t)atoi(ce) : 3;
    while (cache.size() >= (keep ? keep : 1)) {        // evict the least recently used — the async entries may still have its graphs or buffers in flight
        HIPC(ctx, join_side(ctx));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->batch.ws == &cache.back()) batch_none(ctx);
        if (ctx->cot.ws == &cache.back()) cot_none(ctx);
        cache.pop_back();
    }
    cache.emplace_front();
    W &w = cache.front();
    w.N = N;
    ctx->stats[TANGENT_WORKSPACES_ALLOCATED]++;
    // a failed allocation must not leave a half-built entry in the cache: a retry with this N would find it, return
    // HANK_OK and launch on null pointers
    const int rc = build(w);
    if (rc) { cache.pop_front(); (void)hipGetLastError(); return rc; }
    *out = &w;
    return HANK_OK;
}

static int build_tanwork(hank_ctx *ctx, TanWork &w) {
    const Consts &c = ctx->c;
    const size_t P = c.P, G = c.G;
    const int N = w.N;
    // an even batch can run two directions per lane (16-byte accesses): the [..][N] layout is the same, so
    // each sweep picks its own lane width
    const int VB = tan_lane_width(N, 0), VF = tan_lane_width(N, 1);
    w.g = tan_geom(c.n_a, N, VB); w.gf = tan_geom(c.n_a, N, VF);
    w.nbx = w.g.nbx; w.nbxf = w.gf.nbx;
    const size_t GV = (size_t)(c.n_a + KV) * c.n_e;   // dD state carries KV virtual rows per column
    // forward kernel form: source-stationary from 16-lane groups on (N >= 18: forward sweep 3.42 -> 3.05 ms at N=32 with 2 row
    // groups; round 4, with the column index in a scalar register: 4.58 -> 4.28 ms at N=64, 12.5 -> 11.6 ms at N=256,
    // profiles/r04_wide_knobs.log), target-stationary gather below
    const char *se = getenv("HANK_FWD_SS");   // dev knob
    w.gf.ss = se ? atoi(se) : (w.gf.NC >= 16 ? 1 : 0);
    const int RGB = tan_rg(w.g.N, 0), RGF = tan_rg(w.gf.N, 1, w.gf.ss);
    const unsigned nbf = (w.nbxf + RGF - 1) / RGF + KV;   // forward blocks: regular + mass-point
    w.VB = VB; w.VF = VF; w.RGB = RGB; w.RGF = RGF; w.nbf = nbf;
    HIPC(ctx, w.dxhh.alloc((size_t)c.n_hh * P * N));
    HIPC(ctx, w.dxr.alloc(P * N));
    HIPC(ctx, w.dxw.alloc(P * N));
    HIPC(ctx, w.dxt.alloc(P * N));
    for (int k = 0; k < 2; k++) {
        HIPC(ctx, w.ds[k].alloc(G * N));
        HIPC(ctx, w.dD[k].alloc(GV * N));
    }
    HIPC(ctx, w.dpol.alloc(P * G * N));
    HIPC(ctx, w.aggpart.alloc(2 * P * (size_t)nbf * N));      // both aggregates: [P][blocks][2 N]
    HIPC(ctx, w.dagg.alloc(2 * P * N));
    HIPC(ctx, w.dagg_cm.alloc(2 * P * N));                    // (P, 2 N) column-major: the policy-weighted aggregate's N columns, then the grid-weighted one's
    return HANK_OK;
}
static int ensure_tanwork(hank_ctx *ctx, int N, TanWork **out) {
    return tan_cache_get(ctx, ctx->tws, N, [ctx](TanWork &w) { return build_tanwork(ctx, w); }, out);
}

// The tangent-only graphs one entry launches, captured the first time it runs at this batch width: the backward sweep and the plain
// forward sweep as a pair (whatever NX asks: graphs_captured counts them so, and fake_news takes the backward one from the pair), then
// the forward sweep with NX extra reductions. Every buffer the graphs name is allocated before this (enqueue_tan_launch).
static int ensure_tan_graphs(hank_ctx *ctx, TanWork &w, bool bnd, int NX) {
    auto fwd = [&](int nx) {
        if (w.tan_fwd(bnd, nx)) return (int)HANK_OK;
        if (nx == 0) return w.VF == 2 ? capture_tan_fwd<double2, 0>(ctx, w, bnd) : capture_tan_fwd<double, 0>(ctx, w, bnd);
        if (nx == 1) return w.VF == 2 ? capture_tan_fwd<double2, 1>(ctx, w, bnd) : capture_tan_fwd<double, 1>(ctx, w, bnd);
        return w.VF == 2 ? capture_tan_fwd<double2, 2>(ctx, w, bnd) : capture_tan_fwd<double, 2>(ctx, w, bnd);
    };
    int rc = HANK_OK;
    if (!w.tan_back(bnd)) rc = w.VB == 2 ? capture_tan_back<double2>(ctx, w, bnd) : capture_tan_back<double>(ctx, w, bnd);
    if (!rc) rc = fwd(0);
    if (!rc && NX > 0) rc = fwd(NX);
    return rc;
}
// a path kind's backward graph — its jvp entry's and its Toeplitz entry's (the forward sweep is the plain one: it does not know where a
// seed came from) — and, before the capture, the kind's buffers at this width
static int ensure_path_tan_graph(hank_ctx *ctx, TanWork &w, PathKind kind) {
    PathSeed &ps = w.seed[kind];
    const size_t cnt = (size_t)ctx->c.P * path_width(ctx->c, kind) * w.N;
    if (!ps.dir) {
        HIPC(ctx, ps.in.alloc(cnt));
        HIPC(ctx, ps.dir.alloc(cnt));      // (last: a failed allocation is tried again by the next call)
    }
    if (ps.g_tback) return HANK_OK;
    return w.VB == 2 ? capture_tan_back<double2>(ctx, w, false, kind) : capture_tan_back<double>(ctx, w, false, kind);
}
static int ensure_dual_graphs(hank_ctx *ctx, TanWork &w) {
    if (w.g_fback) return HANK_OK;
    if (w.VB == 2) return w.VF == 2 ? capture_dual_graphs<double2, double2>(ctx, w) : capture_dual_graphs<double2, double>(ctx, w);
    return w.VF == 2 ? capture_dual_graphs<double, double2>(ctx, w) : capture_dual_graphs<double, double>(ctx, w);
}

// ---- the device's verdict on work already enqueued, and what the context does about it ------------------
// Three sources — the error word d_err, the persistent sweeps' status (x_status), the fallback decision — and one consequence: the
// caller says WHOSE work the verdict speaks about. THE_RECORD: the sweeps that (re)write the record (hank_primal*, hank_jvp,
// hank_check, fake_news, and what an earlier asynchronous sweep left pending when a call-scoped entry starts): an error goes through
// record_gone, so the batch, the cotangent batch and everything derived from the record go with it, as for a new boundary.
// THIS_CALL: the call's own kernels on its own buffers (the granular steps, hank_vfi, hank_stationary_dist): an error leaves the
// record and the batch exactly as they were.
enum Whose { THE_RECORD, THIS_CALL };
enum ErrIn { IN_SWEEP, IN_VFI, IN_POWER_METHOD };      // which kernels raised the word: a sweep over the periods, steps of the value iteration, the power method
static int x_status(hank_ctx *ctx, const char *what, const XSync *fetched = nullptr);
static int scen_pending_verdict(hank_ctx *ctx);
// the ONE host read of the error word: drain, copy {code, period, state, index}, clear it when set (reported once: the next call starts clean)
static int take_error_word(hank_ctx *ctx, int e[4]) {
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    HIPC(ctx, hipMemcpy(e, ctx->d_err, 4 * sizeof(int), hipMemcpyDeviceToHost));
    if (e[0] != 0) HIPC(ctx, hipMemsetAsync(ctx->d_err, 0, 4 * sizeof(int), ctx->stream));
    return HANK_OK;
}
// the word as a status code and message (step: the caller's count of the fixed-point step that raised it)
static int word_verdict(hank_ctx *ctx, Whose whose, const int e[4], ErrIn in, int step = 0) {
    int rc = HANK_OK;
    if (in == IN_VFI) {
        if (e[0] == ERR_KNOTS)
            rc = fail(ctx, HANK_ERR_KNOTS, "knot-vectors must be unique and sorted in increasing order (steady-state value iteration, step %d, "
                      "productivity state %d, wealth index %d)", step, e[2] + 1, e[3] + 1);
        else if (e[0] == ERR_DOMAIN)
            rc = fail(ctx, HANK_ERR_DOMAIN, "DomainError: negative base under a non-integer power (steady-state value iteration, step %d)", step);
    } else if (in == IN_POWER_METHOD) {
        if (e[0] == ERR_NONMONO) rc = fail(ctx, HANK_ERR_NONMONOTONE, "savings policy is not monotone in wealth (productivity state %d, wealth index %d)", e[2] + 1, e[3] + 1);
    } else if (e[0] == ERR_KNOTS)
        rc = fail(ctx, HANK_ERR_KNOTS,
                  "knot-vectors must be unique and sorted in increasing order (EGM implied state, "
                  "period %d, productivity state %d, wealth index %d)", e[1] + 1, e[2] + 1, e[3] + 1);
    else if (e[0] == ERR_DOMAIN)
        rc = fail(ctx, HANK_ERR_DOMAIN,
                  "DomainError: negative base under a non-integer power (period %d, productivity "
                  "state %d, wealth index %d)", e[1] + 1, e[2] + 1, e[3] + 1);
    else if (e[0] == ERR_NONMONO)
        rc = fail(ctx, HANK_ERR_NONMONOTONE,
                  "savings policy is not monotone in wealth (period %d, productivity state %d, "
                  "wealth index %d)", e[1] + 1, e[2] + 1, e[3] + 1);
    else if (e[0] != 0)
        rc = fail(ctx, HANK_ERR_BAD_ARG, "unknown device error %d (%d,%d,%d) d_err=%p", e[0], e[1], e[2], e[3], (void *)ctx->d_err.get());
    if (rc && whose == THE_RECORD) record_gone(ctx);
    return rc;
}
// the verdict on sweeps: a persistent sweep that did not run (its groups did not form, a wait timed out) leaves the record
// unwritten: what the kernels behind it then found in it (a "non-monotone policy", say) is not an error of the model — the sweep's
// status outranks the word
static int device_verdict(hank_ctx *ctx, Whose whose) {
    int e[4] = {0, 0, 0, 0};
    int rc = take_error_word(ctx, e);
    if (rc) return rc;
    if (ctx->schedule >= 1 && (rc = x_status(ctx, nullptr)) != HANK_OK) {
        if (whose == THE_RECORD) record_gone(ctx);
        return rc;
    }
    return word_verdict(ctx, whose, e, IN_SWEEP);
}

// a sweep could not form its groups (or timed out): this context continues on the per-period launches
static int to_launch_schedule(hank_ctx *ctx) {
    record_gone(ctx);
    if (!ctx->exo[PATH_NONE].g_pback) {     // (a context that has only run persistent sweeps has never captured them)
        const int rc = build_primal_graphs(ctx);
        if (rc != HANK_OK) return rc;       // the schedule is left as it was: the next call reports the sweep's failure again, not a null graph
    }
    ctx->schedule = 0;
    ctx->stats[FALLBACKS]++;
    return HANK_OK;
}
static bool x_fallback_allowed(const hank_ctx *ctx) { return !ctx->forced_xcd; }      // a schedule forced at hank_create fails loudly instead
// the ONE fallback decision on a verdict: anything but a sweep that could not run, or a forced schedule, is reported as it is.
// Otherwise the context moves to the launches (*moved: the work can be run again, they serve it now) and the return value is still
// the sweep's status with the sweep's message, kept here across the move — unless the launches' graphs cannot be built either: then
// THAT is what the caller has to see (the message names it), and the context stays unusable until a later call builds them
static int fallback_decision(hank_ctx *ctx, int verdict, bool *moved) {
    *moved = false;
    if (verdict != HANK_ERR_SWEEP || !x_fallback_allowed(ctx)) return verdict;
    char keep[sizeof(ctx->errmsg)];
    memcpy(keep, ctx->errmsg, sizeof(keep));
    const int rc = to_launch_schedule(ctx);
    if (rc != HANK_OK) return rc;
    memcpy(ctx->errmsg, keep, sizeof(keep));
    *moved = true;
    return verdict;
}
// after a host-pointer entry has enqueued its work: drain it and take the verdict on the record. *rerun: the context has moved to
// the launches, the caller runs its work again. (The device-pointer entries never re-run work: hank_check reports and moves the context.)
static int settle(hank_ctx *ctx, bool *rerun) {
    const int rc = fallback_decision(ctx, device_verdict(ctx, THE_RECORD), rerun);
    return *rerun ? HANK_OK : rc;
}
// a host-pointer entry: enqueue, settle, and when the context has moved to the launches enqueue again and take their verdict
template <typename Enqueue>
static int run_settled(hank_ctx *ctx, Enqueue enqueue) {
    bool rerun = false;
    int rc = enqueue();
    if (!rc) rc = settle(ctx, &rerun);
    if (rerun) rc = enqueue();
    return rerun && !rc ? device_verdict(ctx, THE_RECORD) : rc;
}

// ================================ XCD-local persistent sweeps: host side ==========================
// Two chip-filling launches must never share the chip half-resident (each would wait for workgroups the other's spinning
// workgroups keep out): every such launch of this process, from any context or stream, is ordered behind the previous one
// through one event per device, and the launches of ONE call are enqueued as one block.
static std::mutex g_xmutex;
static hipEvent_t g_xlast[64] = {};
static std::mutex g_xsection[64];
// XSection is the one owner of both: "this thread is enqueueing a block of chip-filling launches on device d". Opening it takes the
// device's section lock — a second host thread (another context on the same GPU: parallel.DeviceGroup) cannot wait for the event of
// the call BEFORE and then enqueue its sweeps beside this call's — and makes the context's stream wait for the device's event.
// Closing it records that event behind what was enqueued and releases the lock: the success path calls close(), so a HIP error
// reaches the caller; the destructor closes what an early return left open, silently, so the next chip-filling launch of the process
// is still ordered behind whatever was enqueued. There is no re-entrancy (a second section of the device inside one would wait for
// itself): whatever launches inside a section takes the open one by reference and gets the stream from it, and only the body that
// knows a call's extent opens one (ensure_lwg keeps taking the context: the launch family calls it too, outside any section; from
// a step it is called on the section's context). One call = one section = one block for x_primal, x_jvp, x_dual_two, x_dual_fused, w_run_tangent
// and x_fixed_point; a WIDE hank_primal_jvp[_dev] is hank_primal[_dev] and then hank_jvp[_dev]: two calls, two blocks.
struct XSection {
    hank_ctx *const ctx;
    explicit XSection(hank_ctx *c) : ctx(c), d(c->device & 63) {
        g_xsection[d].lock();
        std::lock_guard<std::mutex> lk(g_xmutex);
        err = g_xlast[d] ? hipStreamWaitEvent(ctx->stream, g_xlast[d], 0) : hipSuccess;
    }
    XSection(const XSection &) = delete;
    ~XSection() { (void)close(); }
    hipError_t opened() const { return err; }
    hipStream_t stream() const { return ctx->stream; }
    hipError_t close() {
        if (!open) return hipSuccess;
        open = false;
        hipError_t e = hipSuccess;
        {
            std::lock_guard<std::mutex> lk(g_xmutex);
            if (!g_xlast[d]) e = hipEventCreateWithFlags(&g_xlast[d], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(g_xlast[d], ctx->stream);
        }
        g_xsection[d].unlock();
        return e;
    }
private:
    const int d;
    bool open = true;
    hipError_t err = hipSuccess;
};

// the grid fits the XCD-local schedule: a 63-row slab per CU of an XCD, and the Float64 sweeps' LDS (which holds the
// per-period inputs of the WHOLE horizon) fits a workgroup
static size_t x_lds_float64(const Consts &c) { return std::max(x_lds_primal_back(c), x_lds_fwd(c, 0, true)); }
static bool x_supported(const hank_ctx *ctx, int cus, size_t lds_max) {
    const Consts &c = ctx->c;
    const int Sact = (c.n_a + XRW - 1) / XRW;
    return cus >= XG && Sact <= cus / XG && c.n_e <= 16 && x_lds_float64(c) <= lds_max;
}

static int x_setup(hank_ctx *ctx) {
    XWork &X = ctx->xw;
    if (X.ready) return HANK_OK;
    const Consts &c = ctx->c;
    hipDeviceProp_t prop;
    HIPC(ctx, hipGetDeviceProperties(&prop, ctx->device));
    X.grid = (prop.multiProcessorCount / XG) * XG;
    X.Sact = (c.n_a + XRW - 1) / XRW;
    // 64*n_e threads per workgroup (+ one run-ahead wave in the forward sweep); the register budget follows the bound
    X.maxt = 64 * (c.n_e + 1) <= 768 ? 768 : 1024;
    X.dmax = X.maxt == 768 ? XD_MAX : 2;
    const size_t G = c.G, GV = G + 64 * (size_t)c.n_e, P = c.P;
    HIPC(ctx, X.sync.alloc((size_t)2 + 2 * XPASS_MAX));
    HIPC(ctx, hipMemsetAsync(X.sync, 0, sizeof(XSync) * ((size_t)2 + 2 * XPASS_MAX), ctx->stream));      // x_status reads blocks 0, 1 also when the launches recorded the primal
    HIPC(ctx, X.st_s.alloc(2 * XG * G));
    HIPC(ctx, X.st_ds.alloc(2 * XG * G * X.dmax));
    const size_t GM = (size_t)c.n_e * X.Sact * 64;       // member-major state of the forward sweeps: [n_e][members][64]
    HIPC(ctx, X.st_D.alloc(2 * XG * std::max(GV, GM)));
    HIPC(ctx, X.st_dD.alloc(2 * XG * GM * xslots(X.dmax + 1).SP));      // D partials + the value, padded to pairs
    HIPC(ctx, X.Dvirt.alloc(P * c.n_e * 64));
    HIPC(ctx, X.D0own.alloc(P * c.n_e));
    HIPC(ctx, X.aggpart.alloc(2 * P * (size_t)X.Sact));       // [P][members][2]
    HIPC(ctx, X.rho.alloc(P));
    HIPC(ctx, X.srcB.alloc(P * X.Sact));
    HIPC(ctx, X.srcF.alloc(P * X.Sact));
    HIPC(ctx, X.unitsF.alloc(P * X.Sact * XUCAP));
    HIPC(ctx, X.unit_overflow.alloc(1));
    HIPC(ctx, hipMemsetAsync(X.unit_overflow, 0, sizeof(int), ctx->stream));
    if (X.front && ctx->rec_lq) {      // the staging of k_xdual_front
        HIPC(ctx, X.stageU.alloc(P * X.Sact * c.n_e * XU_ROWS));
        HIPC(ctx, X.stageM.alloc(P * X.Sact * c.n_e));
    }
    if (const char *ng = getenv("HANK_XNEIGH")) X.neigh = atoi(ng) != 0;
    if (const char *pk = getenv("HANK_XFWD_PACKED")) X.packed = atoi(pk) != 0;
    if (const char *uc = getenv("HANK_XUCAP")) X.ucap = std::min(XUCAP, std::max(1, atoi(uc)));
    {   // the bound on every wait inside a persistent sweep, in 100 MHz ticks (read once, here)
        double ms = 20.0;
        if (const char *wm = getenv("HANK_XWAIT_MS")) ms = atof(wm);
        const unsigned long long ticks = (unsigned long long)(std::max(ms, 0.01) * 1e5);
        HIPC(ctx, hipMemcpyToSymbol(HIP_SYMBOL(hank::g_xwait_ticks), &ticks, sizeof(ticks)));
    }
    if (const char *sv = getenv("HANK_XSYNCWAVE")) X.syncwave = atoi(sv) != 0;
    X.lds_max = (int)prop.sharedMemPerBlock;
    if (const char *xf = getenv("HANK_XFAULT")) {      // "placement" | "timeout", optionally ":primal" | ":tangent" | ":fixedpoint" (default: every persistent launch)
        X.fault = strncmp(xf, "placement", 9) == 0 ? XERR_PLACEMENT : (strncmp(xf, "timeout", 7) == 0 ? XERR_TIMEOUT : (strncmp(xf, "stall", 5) == 0 ? 3 : 0));
        const char *w = strchr(xf, ':');
        X.fault_where = !w ? 7 : (strcmp(w, ":primal") == 0 ? 1 : (strcmp(w, ":tangent") == 0 ? 2 : (strcmp(w, ":fixedpoint") == 0 ? 4 : 7)));
    }
    HIPC(ctx, hipMemsetAsync(X.Dvirt, 0, sizeof(double) * P * c.n_e * 64, ctx->stream));
    X.ready = true;
    return HANK_OK;
}

// the passes of a batch of w.N directions and their buffers
static int x_build_tan(hank_ctx *ctx, XTan &w) {
    XWork &X = ctx->xw;
    const Consts &c = ctx->c;
    const size_t P = c.P, G = c.G;
    const int N = w.N;
    size_t off = 0;
    for (int n0 = 0; n0 < N; n0 += XG * X.dmax) {
        XPass ps;
        ps.n0 = n0; ps.N = std::min(N - n0, XG * X.dmax);
        ps.D = 1; while (XG * ps.D < ps.N) ps.D *= 2;
        ps.groups = (ps.N + ps.D - 1) / ps.D;
        ps.dpol_off = off;
        off += P * ps.groups * G * ps.D;
        w.passes.push_back(ps);
    }
    if ((int)w.passes.size() > XPASS_MAX) return fail(ctx, HANK_ERR_BAD_ARG, "N=%d needs %d passes, at most %d per call", N, (int)w.passes.size(), XPASS_MAX);
    HIPC(ctx, w.dxhh.alloc((size_t)c.n_hh * P * N));
    HIPC(ctx, w.dxr.alloc(P * N)); HIPC(ctx, w.dxw.alloc(P * N)); HIPC(ctx, w.dxt.alloc(P * N));
    HIPC(ctx, w.dpol.alloc(off));
    const size_t W = (size_t)XG * X.dmax, nb = (size_t)X.Sact;
    HIPC(ctx, w.daggpart.alloc(2 * P * nb * W));              // both aggregates: [P][members][2 W]
    HIPC(ctx, hipMemsetAsync(w.daggpart, 0, sizeof(double) * 2 * P * nb * W, ctx->stream));
    HIPC(ctx, w.dagg_pass.alloc(2 * P * W));
    HIPC(ctx, w.dagg_cm.alloc(2 * P * N));                    // (P, 2 N) column-major
    return HANK_OK;
}
static int x_ensure_tan(hank_ctx *ctx, int N, XTan **out) {
    const int nmax = 8 * ctx->xw.dmax * XPASS_MAX;      // (a cached width has passed this check)
    if (N > nmax) return fail(ctx, HANK_ERR_BAD_ARG, "N=%d exceeds %d directions per call", N, nmax);
    return tan_cache_get(ctx, ctx->xw.tans, N, [ctx](XTan &w) { return x_build_tan(ctx, w); }, out);
}

// workgroup of the persistent kernels: 64 threads per productivity state + one wave that only runs the group barrier's poll,
// where the block has room (dev knob HANK_XSYNCWAVE=0: wave 0 polls)
static dim3 x_block(const XWork &X, const Consts &c) {
    const bool fits = 64 * (c.n_e + 1) <= X.maxt && X.syncwave;
    return dim3(fits ? 64 * (c.n_e + 1) : 64 * c.n_e);
}

// One launcher per persistent kernel: the whole chip (a workgroup per CU), the instance for X.maxt (and D, val), and the dynamic LDS
// of THAT instance from the size function under the kernel. k_xdual_back and every D = 4 instance exist for 768 threads only.
// (x_launch_vfi and x_launch_stat stand with their caller, x_fixed_point. The kernels are emitted into the code object in the order
// these launchers name them: moving one moves its kernels, and a disassembly diff against the previous build is no longer empty.
// Each takes the open section and launches on its stream: a persistent launch outside a section cannot be written.)
template <typename F>
static void x_by_maxt(const XWork &X, F launch) { if (X.maxt == 768) launch(std::integral_constant<int, 768>()); else launch(std::integral_constant<int, 1024>()); }
#define XL(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(X.grid), x_block(X, c), lds, sec.stream(), a)
static bool x_has_dual_back(const XWork &X) { return X.maxt == 768; }
// (the instances compiled for the model's constants, hank_xspec.h, are named behind the generic three: see above)
static void x_launch_dual_back(XSection &sec, XWork &X, const Consts &c, int D, const XDualBackArgs &a) {      // (X.inst: which instance went out)
    const size_t lds = x_lds_dual_back(c, D);
    if (!x_has_dual_back(X)) return;
    const XSpec sp = x_spec(X.xspec, c.n_e, c.gamma, c.diet);
    X.inst[0] = sp.ne; X.inst[1] = sp.crra;
    if (!sp.ne && !sp.crra) {
        if (D == 1) XL(k_xdual_back<1, 768>);
        else if (D == 2) XL(k_xdual_back<2, 768>);
        else XL(k_xdual_back<4, 768>);
        return;
    }
    auto by_d = [&](auto ne, auto crra) {
        constexpr int NE = decltype(ne)::value, CRRA = decltype(crra)::value;
        if (D == 1) XL(k_xdual_back<1, 768, NE, CRRA>);
        else if (D == 2) XL(k_xdual_back<2, 768, NE, CRRA>);
        else XL(k_xdual_back<4, 768, NE, CRRA>);
    };
    auto by_crra = [&](auto ne) {
        if (sp.crra) by_d(ne, std::integral_constant<int, 1>()); else if constexpr (decltype(ne)::value != 0) by_d(ne, std::integral_constant<int, 0>());
    };
    if (sp.ne == 4) by_crra(std::integral_constant<int, 4>());
    else if (sp.ne == 7) by_crra(std::integral_constant<int, 7>());
    else if (sp.ne == 11) by_crra(std::integral_constant<int, 11>());
    else by_crra(std::integral_constant<int, 0>());
}
// does the Dual pass's forward sweep take the packed-record instance k_xfwd<D, true, ., true>? (x_launch_fwd's rule, asked by x_dual_fused
// too: only that instance can run behind the lean front)
static bool x_fwd_serves_lq(const XWork &X, const Consts &c, int D) {
#if HANK_XFWD_LQ
    return X.packed && D > 0 && x_lds_fwd_lq(c, D) <= (size_t)X.lds_max;
#else
    return false;
#endif
}
// k_xfwd<D, VAL>: D = 0 (the Float64 sweep alone, VAL), 1, 2, 4
static void x_launch_fwd(XSection &sec, XWork &X, const Consts &c, int D, bool val, const XSweepFwdArgs &a) {
    if (val && D > 0) { X.inst[2] = 0; X.inst[3] = 0; }      // (k_xfwd has no instance of hank_xspec.h's: DESIGN.md section 4)
#if HANK_XFWD_LQ
    // the Dual pass (every caller has written the packed record in front, in this section: k_lottery_lq or k_xdual_front): the packed record where the table fits beside the carve
    if (val && x_fwd_serves_lq(X, c, D)) {
        const size_t lds = x_lds_fwd_lq(c, D);
        x_by_maxt(X, [&](auto mt) {
            constexpr int MT = decltype(mt)::value;
            if (D == 1) XL(k_xfwd<1, true, MT, true>);
            else if (D == 2) XL(k_xfwd<2, true, MT, true>);
            else if (D == 4) { if constexpr (MT == 768) XL(k_xfwd<4, true, MT, true>); }
        });
        return;
    }
#endif
    const size_t lds = x_lds_fwd(c, D, val || D == 0);
    x_by_maxt(X, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        if (D == 0) XL(k_xfwd<0, true, MT>);
        else if (D == 1) { if (val) XL(k_xfwd<1, true, MT>); else XL(k_xfwd<1, false, MT>); }
        else if (D == 2) { if (val) XL(k_xfwd<2, true, MT>); else XL(k_xfwd<2, false, MT>); }
        else if (D == 4) { if constexpr (MT == 768) { if (val) XL(k_xfwd<4, true, MT>); else XL(k_xfwd<4, false, MT>); } }
    });
}
static void x_launch_primal_back(XSection &sec, const XWork &X, const Consts &c, const XBackArgs &a) { const size_t lds = x_lds_primal_back(c); x_by_maxt(X, [&](auto mt) { XL(k_xprimal_back<decltype(mt)::value>); }); }
static void x_launch_tan_back(XSection &sec, const XWork &X, const Consts &c, int D, const XTanBackArgs &a) {
    const size_t lds = x_lds_tan_back(c, D);
    x_by_maxt(X, [&](auto mt) {
        constexpr int MT = decltype(mt)::value;
        if (D == 1) XL(k_xtan_back<1, MT>);
        else if (D == 2) XL(k_xtan_back<2, MT>);
        else if (D == 4) { if constexpr (MT == 768) XL(k_xtan_back<4, MT>); }
    });
}
// before a reader of R.lo, R.lw, R.ig or R.start: the lean front of the one-pass persistent Dual pass (k_xdual_front) wrote none of
// them — k_lottery on the recorded policies makes them, the same body and the same bits as every other lottery (it rewrites clo
// with the values it has). Every host path that lets a kernel read one of the four comes through here: DESIGN.md section 2a.
static int ensure_lottery(hank_ctx *ctx, hipStream_t s = nullptr) {
    if (ctx->lot_valid) return HANK_OK;
    const Consts &c = ctx->c;
    hipLaunchKernelGGL(k_lottery, dim3((unsigned)(c.P * c.n_e)), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s ? s : ctx->stream, c, ctx->R, c.P * c.n_e, ctx->d_err, 0, 1);
    HIPC(ctx, hipGetLastError());
    ctx->lot_valid = true;
    return HANK_OK;
}
// the forward sweeps' geometry at the recorded lottery (once per primal)
static void x_ensure_rng(XSection &sec) {
    hank_ctx *ctx = sec.ctx;
    XWork &X = ctx->xw;
    if (X.rng_valid) return;
    (void)ensure_lottery(ctx, sec.stream());      // (k_xunits_fwd reads R.start)
    hipLaunchKernelGGL(k_xunits_fwd, dim3((unsigned)ctx->c.P, (unsigned)X.Sact), dim3(256), 0, sec.stream(), ctx->c, ctx->R, X.Sact, X.srcF, X.unitsF, X.unit_overflow, X.ucap);
    X.rng_valid = true;
}

static int ensure_seg(hank_ctx *ctx) {       // before a reader of R.seg (launch-family forward tangent sweeps, hank_fake_news)
    if (ctx->seg_valid) return HANK_OK;
    { const int rc = ensure_lottery(ctx); if (rc) return rc; }
    hipLaunchKernelGGL(k_seg_build, dim3((unsigned)(ctx->c.P * ctx->c.n_e)), dim3(256), 0, ctx->stream, ctx->c, ctx->R, ctx->c.P * ctx->c.n_e);
    HIPC(ctx, hipGetLastError());
    ctx->seg_valid = true;
    return HANK_OK;
}
// before a reader of R.lwg (every forward tangent sweep at a recorded primal — persistent, launch family, wide — and
// hank_fake_news): a persistent Dual pass leaves the record to be made from what it wrote (lw, ig, D_t, the virtual rows' mass)
static int ensure_lwg(hank_ctx *ctx) {
    if (ctx->lwg_valid) return HANK_OK;
    { const int rc = ensure_lottery(ctx); if (rc) return rc; }
    const XWork &X = ctx->xw;
    hipLaunchKernelGGL(k_xlwg_build, dim3((unsigned)(ctx->c.P * ctx->c.n_e)), dim3(256), 0, ctx->stream, ctx->c, ctx->R, X.Dvirt, X.D0own, X.Sact);
    HIPC(ctx, hipGetLastError());
    ctx->lwg_valid = true;
    ctx->lwg_builds++;
    return HANK_OK;
}
// zero the sync blocks of the launches about to be enqueued (and, under the dev knob, pre-set their status words)
static int x_sync_reset(XSection &sec, XSync *base, int count, int where) {     // where: 1 primal sweeps, 2 tangent sweeps, 4 the steady state's fixed points
    hank_ctx *ctx = sec.ctx;
    HIPC(ctx, hipMemsetAsync(base, 0, sizeof(XSync) * (size_t)count, sec.stream()));
    if (ctx->xw.fault && ctx->xw.fault != 3 && (ctx->xw.fault_where & where)) hipLaunchKernelGGL(k_xpoison, dim3(1), dim3(64), 0, sec.stream(), base, count, (unsigned)ctx->xw.fault);
    return HANK_OK;
}

// ---- the steps of the persistent shapes ----------------------------------------------------------------------------------------
// Each takes the open section (and the batch it works on) and enqueues ONE thing, whole; none is told what another has done. The
// bodies that compose them (x_primal, x_jvp, x_dual_two, x_dual_fused: one per shape of call) hold the section and the bookkeeping.
// Sync blocks: 0, 1 the Float64 sweeps (backward, forward); 2 + 2p, 3 + 2p the backward and forward sweep of tangent pass p (a
// forward sweep that carries the value too is still pass 0's): x_status reads them in this order.
static void x_rho(XSection &sec) {
    hank_ctx *ctx = sec.ctx;
    hipLaunchKernelGGL(k_xrho, dim3((unsigned)((ctx->c.P + 255) / 256)), dim3(256), 0, sec.stream(), ctx->d_xhh, ctx->c.n_hh, ctx->c.P, ctx->xw.rho);
}
static void x_tan_in(XSection &sec, XTan *w) {
    const Consts &c = sec.ctx->c;
    hipLaunchKernelGGL(k_tan_in, dim3((unsigned)(((size_t)c.P * w->N + 255) / 256)), dim3(256), 0, sec.stream(), w->dxhh, c.n_hh, c.P, w->N, w->dxr, w->dxw, w->dxt);
}
// in front of the tangent sweeps at a recorded primal: their sync blocks, the inputs, and once per recorded primal which members
// each member's gathers read, period by period
static int x_tan_front(XSection &sec, XTan *w) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    const int rc = x_sync_reset(sec, X.sync + 2, 2 * (int)w->passes.size(), 2); if (rc) return rc;
    x_tan_in(sec, w);
    x_rho(sec);     // (the primal may have been recorded by the launches)
    if (!X.src_valid) {
        hipLaunchKernelGGL(k_xsrc_back, dim3((unsigned)ctx->c.P, X.Sact), dim3(256), 0, sec.stream(), ctx->c, ctx->R, X.Sact, X.srcB);
        X.src_valid = true;
    }
    return HANK_OK;
}
// The Dual-pass sweeps reach the record and dpol through buffer descriptors with 32-bit offsets, and the work units
// (on their pointer) with a 32-bit index (hank_xsweep.h: XRecOff, hank_xaddr.h: x_addr_fits). The
// record's offsets, and whether every stream of the widest Dual pass of this context fits (asked where the schedule is chosen:
// a context that does not fit keeps the per-period launches, as one whose LDS does not fit does)
static XRecOff x_rec_off(const hank_ctx *ctx) {
    const Record &R = ctx->R;
    const char *b = ctx->rec_slab;
    auto off = [&](const void *p) { return (unsigned)((const char *)p - b); };
    XRecOff o{};
    o.rec = b; o.bytes = (unsigned)ctx->rec_bytes;
    o.pol = off(R.pol); o.ib = off(R.ib); o.A = off(R.A); o.B = off(R.B); o.u = off(R.u); o.v = off(R.v); o.s = off(R.s); o.kc = off(R.kc);
    o.lo = off(R.lo); o.lw = off(R.lw); o.ig = off(R.ig); o.Dseq = off(R.Dseq);
    o.lq = ctx->rec_lq ? off(ctx->rec_lq) : 0u;
    return o;
}
static bool x_dual_addr_fits(const hank_ctx *ctx) {
    const Consts &c = ctx->c;
    return x_addr_fits(ctx->rec_bytes, (unsigned long long)c.P, XG, (unsigned long long)c.G, XD_MAX, (unsigned long long)((c.n_a + XRW - 1) / XRW), XUCAP);
}
// span PRIMAL_BACK: the Float64 backward sweep at the context's x (d_xhh) and boundary, on ONE XCD's workgroups; with a one-pass
// batch `dual` it carries the batch's partials too (k_xdual_back)
static int x_back(XSection &sec, XTan *dual = nullptr) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    const Consts &c = ctx->c;
    XBackArgs ab{};
    ab.c = c; ab.ss_value = ctx->d_ss_value; ab.xhh = ctx->d_xhh; ab.rho = X.rho; ab.sy = X.sync; ab.st_s = X.st_s;
    ab.err = ctx->d_err; ab.R = ctx->R;
    HIPC(ctx, ctx->spans.begin(PRIMAL_BACK, sec.stream()));
    if (dual) {
        const XPass &ps = dual->passes[0];
        XDualBackArgs db{};
        db.p = ab; db.dxr = dual->dxr; db.dxw = dual->dxw; db.dxt = dual->dxt; db.Ntot = dual->N; db.n0 = ps.n0; db.N = ps.N;
        db.st_ds = X.st_ds; db.dpol = dual->dpol + ps.dpol_off; db.groups = ps.groups;
        db.ro = x_rec_off(ctx); db.dpol_bytes = (unsigned)((size_t)c.P * ps.groups * c.G * ps.D * sizeof(double));
        x_launch_dual_back(sec, X, c, ps.D, db);
    } else x_launch_primal_back(sec, X, c, ab);
    HIPC(ctx, ctx->spans.end(PRIMAL_BACK, sec.stream(), 1));
    return HANK_OK;
}
// the Young lottery of the policies just written; seg: with the per-target segment records (the Dual pass whose forward sweep reads
// the lottery through its work units leaves them to be built when somebody asks: ensure_seg)
// lq: a persistent Dual pass follows — with the packed per-source records its forward sweep reads (k_lottery_lq)
static void x_lottery(XSection &sec, bool seg, bool lq = false) {
    hank_ctx *ctx = sec.ctx;
    const Consts &c = ctx->c;
#if HANK_XFWD_LQ
    if (lq) {
        hipLaunchKernelGGL(k_lottery_lq, dim3((unsigned)(c.P * c.n_e)), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), sec.stream(), c, ctx->R, c.P * c.n_e, ctx->d_err, seg ? 1 : 0, 1, ctx->rec_lq);
        return;
    }
#endif
    hipLaunchKernelGGL(k_lottery, dim3((unsigned)(c.P * c.n_e)), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), sec.stream(), c, ctx->R, c.P * c.n_e, ctx->d_err, seg ? 1 : 0, 1);
}
// the front of the one-pass Dual pass whose forward sweep reads the packed record: the lean lottery with the cut of every column in
// its launch (k_xdual_front), then the units packed member by member (k_xunits_pack) — what x_lottery(sec, false, true) and
// x_ensure_rng leave behind for that sweep, without lo, lw, ig and start (the caller marks the record: ensure_lottery)
static void x_front(XSection &sec) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    const Consts &c = ctx->c;
    hipLaunchKernelGGL(k_xdual_front, dim3((unsigned)(c.P * c.n_e)), dim3(512), sizeof(int) * (2 * (size_t)c.n_a + 2), sec.stream(), c, ctx->R, c.P * c.n_e, ctx->d_err, ctx->rec_lq,
                       X.Sact, X.stageU.get(), X.stageM.get(), X.front_poison);
    hipLaunchKernelGGL(k_xunits_pack, dim3((unsigned)((c.P * X.Sact + 3) / 4)), dim3(256), 0, sec.stream(), c, ctx->R, X.Sact, X.stageU.get(), X.stageM.get(), X.srcF.get(), X.unitsF.get(),
                       X.unit_overflow.get(), X.ucap);
}
// span TAN_BACK: the backward sweep of every pass of the batch, every XCD a group
static int x_tan_back(XSection &sec, XTan *w) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    const int np = (int)w->passes.size();
    XTanBackArgs ab{};
    ab.c = ctx->c; ab.R = ctx->R; ab.rho = X.rho; ab.xhh = ctx->d_xhh; ab.dxr = w->dxr; ab.dxw = w->dxw; ab.dxt = w->dxt; ab.Ntot = w->N; ab.st_ds = X.st_ds;
    ab.src = X.neigh ? X.srcB.get() : nullptr;
    ab.stall = X.fault == 3 ? 1 : 0;
    HIPC(ctx, ctx->spans.begin(TAN_BACK, sec.stream()));
    for (int p = 0; p < np; p++) {
        const XPass &ps = w->passes[p];
        ab.n0 = ps.n0; ab.N = ps.N; ab.groups = ps.groups; ab.sy = X.sync + 2 + 2 * p; ab.dpol = w->dpol + ps.dpol_off;
        x_launch_tan_back(sec, X, ctx->c, ps.D, ab);
    }
    HIPC(ctx, ctx->spans.end(TAN_BACK, sec.stream(), np));
    return HANK_OK;
}
// behind a forward sweep that carried the value: both aggregates summed over the members, and the virtual rows' mass folded into D_t
static void x_value_epilogue(XSection &sec) {
    hank_ctx *ctx = sec.ctx; const XWork &X = ctx->xw;
    const Consts &c = ctx->c;
    const size_t P = c.P;
    hipStream_t s = sec.stream();
    hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)P, 1), dim3(256), 0, s, X.aggpart, X.Sact, 2, ctx->d_agg_rm);
    hipLaunchKernelGGL(k_tan_out, dim3((unsigned)((2 * P + 255) / 256)), dim3(256), 0, s, ctx->d_agg_rm, (int)P, 2, ctx->d_agg);
    hipLaunchKernelGGL(k_xfix_D, dim3((unsigned)((P * c.n_e + 255) / 256)), dim3(256), 0, s, c, ctx->R.Dseq, X.Dvirt, X.Sact, X.D0own);
}
// the forward sweeps' arguments; val: the sweep carries the value, from D_0 on (the record's D_t, the virtual rows' mass, the aggregates' parts)
static XSweepFwdArgs x_fwd_args(const hank_ctx *ctx, bool val) {
    const XWork &X = ctx->xw;
    XSweepFwdArgs fa{};
    fa.c = ctx->c; fa.R = ctx->R; fa.src = X.srcF; fa.units = X.unitsF; fa.overflow = X.unit_overflow; fa.all_members = X.neigh ? 0 : 1;
    if (val) { fa.D0 = ctx->d_ss_D; fa.Dvirt = X.Dvirt; fa.aggpart = X.aggpart; }
    return fa;
}
// span PRIMAL_FWD: the Float64 distribution sweep alone (k_xfwd<0, true>), and its epilogue
static int x_fwd_value(XSection &sec) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    XSweepFwdArgs fa = x_fwd_args(ctx, true);
    fa.sy = X.sync + 1; fa.st = X.st_D; fa.groups = 1;
    HIPC(ctx, ctx->spans.begin(PRIMAL_FWD, sec.stream()));
    x_launch_fwd(sec, X, ctx->c, 0, true, fa);
    HIPC(ctx, ctx->spans.end(PRIMAL_FWD, sec.stream(), 1));
    x_value_epilogue(sec);
    return HANK_OK;
}
// the forward sweep of pass p of the batch (k_xfwd<D, val>); val: it is the Float64 distribution sweep of a Dual pass too. Without,
// it runs at the recorded primal and reads the per-source records, built here when a persistent Dual pass left them to be made
static int x_tan_fwd(XSection &sec, XTan *w, int p, bool val) {
    hank_ctx *ctx = sec.ctx; XWork &X = ctx->xw;
    const XPass &ps = w->passes[p];
    if (!val) { const int rc = ensure_lwg(ctx); if (rc) return rc; }
    XSweepFwdArgs fa = x_fwd_args(ctx, val);
    fa.sy = X.sync + 2 + 2 * p + 1; fa.st = X.st_dD; fa.daggpart = w->daggpart; fa.groups = ps.groups; fa.dpol = w->dpol + ps.dpol_off;
    fa.ro = x_rec_off(ctx); fa.dpol_bytes = (unsigned)((size_t)ctx->c.P * ps.groups * ctx->c.G * ps.D * sizeof(double));
    fa.iga = ctx->rec_iga ? (unsigned)((const char *)ctx->rec_iga - (const char *)ctx->rec_slab) : 0u;
    x_launch_fwd(sec, X, ctx->c, ps.D, val, fa);
    return HANK_OK;
}
// behind the forward sweep of pass p: its partials of both aggregates, summed over the members (one row of partials per member:
// the sync wave sums a member's columns) and written to their columns of dagg_cm
static void x_tan_reduce(XSection &sec, XTan *w, int p) {
    hank_ctx *ctx = sec.ctx;
    const size_t P = ctx->c.P;
    const XPass &ps = w->passes[p];
    const int W = XG * ps.D;
    hipStream_t s = sec.stream();
    hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)P, (2 * W + 63) / 64), dim3(256), 0, s, w->daggpart, ctx->xw.Sact, 2 * W, w->dagg_pass);
    hipLaunchKernelGGL(k_xout, dim3((unsigned)((P * ps.N + 255) / 256)), dim3(256), 0, s, w->dagg_pass, (int)P, 2 * W, 0, ps.n0, ps.N, w->dagg_cm);
    hipLaunchKernelGGL(k_xout, dim3((unsigned)((P * ps.N + 255) / 256)), dim3(256), 0, s, w->dagg_pass, (int)P, 2 * W, W, ps.n0, ps.N, w->dagg_cm + P * (size_t)w->N);
}
// passes `first`.. of the batch at the recorded primal, each with its reduction; TAN_FWD (begun by the body) ends behind the last sweep
static int x_tan_fwd_from(XSection &sec, XTan *w, int first) {
    hank_ctx *ctx = sec.ctx;
    const int np = (int)w->passes.size();
    for (int p = first; p < np; p++) {
        const int rc = x_tan_fwd(sec, w, p, false); if (rc) return rc;
        if (p == np - 1) HIPC(ctx, ctx->spans.end(TAN_FWD, sec.stream(), np));
        x_tan_reduce(sec, w, p);
    }
    return HANK_OK;
}
// behind the value-carrying forward sweep of a ONE-pass batch: the value epilogue, the reduction and the copies to the caller's
// buffers (null: not asked for) in one launch
static void x_dual_epilogue(XSection &sec, XTan *w, double *d_agg_out, double *d_dagg_out) {
    hank_ctx *ctx = sec.ctx; const XWork &X = ctx->xw;
    const Consts &c = ctx->c;
    const XPass &ps = w->passes[0];
    const int W = XG * ps.D, per = 2 * W + 2 + c.n_e;
    hipLaunchKernelGGL(k_xdual_epilogue, dim3((unsigned)(((size_t)c.P * per + 255) / 256)), dim3(256), 0, sec.stream(), c, X.aggpart, w->daggpart, X.Sact, W, ps.n0, ps.N, w->N,
                       ctx->d_agg_rm, ctx->d_agg, w->dagg_pass, w->dagg_cm, ctx->R.Dseq, X.Dvirt, X.D0own, d_agg_out, d_dagg_out);
}

// after a synchronisation: did every persistent launch of the last call form its groups and meet all its barriers? The ONE judge of
// the sync blocks. For the sweeps (what == nullptr) it reads them itself, behind the work units' overflow flag (the forward sweeps');
// for a steady-state fixed point, `what` is its name (its wording) and `fetched` its one block, which x_fixed_point copied in front
// of the synchronisation. What the answer does to the record is the caller's business (device_verdict)
static int x_status(hank_ctx *ctx, const char *what, const XSync *fetched) {
    XWork &X = ctx->xw;
    std::vector<XSync> own;
    if (!fetched) {
        if (!X.ready || X.last_blocks == 0) return HANK_OK;
        int uo = 0;
        HIPC(ctx, hipMemcpy(&uo, X.unit_overflow, sizeof(int), hipMemcpyDeviceToHost));
        if (uo) {
            HIPC(ctx, hipMemsetAsync(X.unit_overflow, 0, sizeof(int), ctx->stream));
            return fail(ctx, HANK_ERR_SWEEP, "persistent forward sweep: a member's walk over its sources needs more than %d work units (a savings policy this flat is served by the per-period launches)", XUCAP);
        }
        own.resize((size_t)X.last_blocks);
        HIPC(ctx, hipMemcpy(own.data(), X.sync, sizeof(XSync) * own.size(), hipMemcpyDeviceToHost));
    }
    const XSync *h = fetched ? fetched : own.data();
    for (size_t k = 0; k < (fetched ? 1 : own.size()); k++)
        if (h[k].status[0] != 0) {
            if (what) return fail(ctx, HANK_ERR_SWEEP, "persistent %s: %s on XCD %u", what, h[k].status[0] == XERR_PLACEMENT ? "the group is short of members" : "a wait timed out", h[k].status[1]);
            char waited[64] = "";
            if (h[k].status[0] == XERR_TIMEOUT) snprintf(waited, sizeof(waited), " after %.1f ms", h[k].status[2] / 1000.0);
            return fail(ctx, HANK_ERR_SWEEP, "persistent %s sweep %zu (0 = primal, then one per tangent pass): %s%s on XCD %u (workgroups per XCD: %u %u %u %u %u %u %u %u)",
                        (k & 1) ? "forward" : "backward", k / 2, h[k].status[0] == XERR_PLACEMENT ? "a group is short of members" : "a wait timed out", waited,
                        h[k].status[1], h[k].ticket[0][0], h[k].ticket[1][0], h[k].ticket[2][0], h[k].ticket[3][0], h[k].ticket[4][0],
                        h[k].ticket[5][0], h[k].ticket[6][0], h[k].ticket[7][0]);
        }
    return HANK_OK;
}

// ================================ on-chip wide sweeps (hank_wide.h): host side ====================
// value-function families share the kernels (n_hh and the record diet are run-time / template switches); the number of
// productivity states is a template parameter (the state of a grid row is a register array)
#define HANK_WIDE_NE_LIST(X) X(2) X(3) X(4) X(5) X(7) X(11)
static bool w_ne_instantiated(int ne) {
#define X(NEV) if (ne == NEV) return true;
    HANK_WIDE_NE_LIST(X)
#undef X
    return false;
}
// geometry of the wide kernels (hank_wide.h): rows per thread 4 (workgroups of <= 512 threads) or 2 (<= 1024); which columns of the
// state stay in registers follows from the register budget of each: all of them, except the forward kernel of the 2-row geometry
struct WGeom { int R, maxt, kreg_b, kreg_f; };
static WGeom w_geom(const hank_ctx *ctx) { return ctx->wide_r == 2 ? WGeom{2, 1024, 16, 7} : WGeom{4, 512, 16, 16}; }
static int w_threads(const hank_ctx *ctx) { const WGeom g = w_geom(ctx); return std::max(64, ((ctx->c.n_a + g.R - 1) / g.R + 63) / 64 * 64); }
static size_t w_lds(const hank_ctx *ctx) { const WGeom g = w_geom(ctx); return std::max(wide_lds_back(ctx->c, g.kreg_b), wide_lds_fwd(ctx->c, g.kreg_f)); }
static bool w_supported(const hank_ctx *ctx) {
    const Consts &c = ctx->c;
    return w_ne_instantiated(c.n_e) && c.n_a <= WIDE_CS && w_lds(ctx) <= ctx->lds_max &&
           ctx->rec_bytes < 0x7fffffffull && (size_t)c.G * sizeof(double) < 0x7fffffffull;
}
// auto: a workgroup (= a direction) per CU and round; a round costs what ~80 directions cost the per-period launches (measured at
// 2000x11, T=300, profiles/r05b_wide_crossover.log: 12.9 ms per round with the primal, 10.3 at a recorded primal, whatever its
// fill; the launches 13.1 ms at N = 80, 14.0 at 128 and 23.5 from 144 on), so the batch goes to the wide sweeps when its last round
// holds at least that many (before the L2 warming of k_wide_back a round cost 13.9 ms at a recorded primal and the crossover was 152).
// wide_min (HANK_WIDE_MIN) is that fill, in directions.
static bool use_wide(const hank_ctx *ctx, int N) {
    if (ctx->wide_mode == 2) return true;
    if (ctx->wide_mode != 1) return false;
    const int rounds = (N + ctx->num_cus - 1) / ctx->num_cus;
    return (long long)N * 256 >= (long long)rounds * ctx->wide_min * ctx->num_cus;      // (wide_min is quoted for a 256-CU chip)
}

template <int NE, int R, int MAXT, int KB, int KF>
static int w_launch_geom(XSection &sec, bool fwd, int N, const WideArgs &a) {
    hank_ctx *ctx = sec.ctx;
    const Consts &c = ctx->c;
    WMat<NE> M;
    for (int k = 0; k < NE; k++)
        for (int e = 0; e < NE; e++) M.m[k * NE + e] = fwd ? ctx->h_Pi[k + NE * e] : ctx->h_Pi[e + NE * k];
    for (int e = 0; e < NE; e++) M.z[e] = ctx->h_z[e];
    const dim3 grd((unsigned)N), blk((unsigned)w_threads(ctx));
    if (fwd) {
        const size_t lds = wide_lds_fwd(c, KF);
        HIPC(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wide_fwd<NE, R, MAXT, KF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_wide_fwd<NE, R, MAXT, KF>), grd, blk, lds, sec.stream(), a, M);
    } else {
        const size_t lds = wide_lds_back(c, KB);
        if (c.diet) {
            HIPC(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wide_back<NE, R, MAXT, true, KB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_wide_back<NE, R, MAXT, true, KB>), grd, blk, lds, sec.stream(), a, M);
        } else {
            HIPC(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wide_back<NE, R, MAXT, false, KB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_wide_back<NE, R, MAXT, false, KB>), grd, blk, lds, sec.stream(), a, M);
        }
    }
    return HANK_OK;
}
static int w_launch(XSection &sec, bool fwd, int N, const WideArgs &a) {
    hank_ctx *ctx = sec.ctx;
#define X(NEV) if (ctx->c.n_e == NEV) return ctx->wide_r == 2 ? w_launch_geom<NEV, 2, 1024, 16, 7>(sec, fwd, N, a) : w_launch_geom<NEV, 4, 512, 16, 16>(sec, fwd, N, a);
    HANK_WIDE_NE_LIST(X)
#undef X
    return fail(ctx, HANK_ERR_BAD_ARG, "on-chip wide sweeps: n_e=%d is not instantiated", ctx->c.n_e);
}

// (the staging buffer of the host-pointer entries is allocated when one of them first uses the width)
static int w_ensure_tan(hank_ctx *ctx, int N, bool staging, WTan **out) {
    const size_t P = ctx->c.P, G = ctx->c.G;
    const int rc = tan_cache_get(ctx, ctx->wtans, N, [=](WTan &w) -> int {
        HIPC(ctx, w.dpol.alloc(P * (size_t)N * G + 2));       // (+ 2: the last 16-byte load of an odd-sized grid reads 8 bytes past its row)
        HIPC(ctx, w.dagg_cm.alloc(2 * P * (size_t)N));            // (P, 2 N) column-major: both aggregates
        return HANK_OK;
    }, out);
    if (rc) return rc;
    if (staging && !(*out)->dxhh) HIPC(ctx, (*out)->dxhh.alloc((size_t)ctx->c.n_hh * P * N));
    return HANK_OK;
}

// the N partials at the recorded primal (either schedule may have recorded it): two launches, one workgroup per direction
static int w_run_tangent(hank_ctx *ctx, WTan *w, const double *d_dxhh) {
    const Consts &c = ctx->c;
    XSection sec(ctx);                      // (a persistent sweep of another context must not find the chip half full of these workgroups)
    HIPC(ctx, sec.opened());
    hipStream_t s = sec.stream();
    if (!ctx->d_ibw) HIPC(ctx, ctx->d_ibw.alloc((size_t)c.P * c.G + 4));      // (before the kernel arguments are filled in)
    WideArgs a{};
    a.c = c; a.R = ctx->R; a.xhh = ctx->d_xhh; a.dxhh = d_dxhh; a.Ntot = w->N; a.n0 = 0; a.dpol = w->dpol; a.dagg = w->dagg_cm;
    a.rec = ctx->rec_slab;
    auto off = [&](const void *p) { return (unsigned)((const char *)p - ctx->rec_slab); };
    const Record &R = ctx->R;
    a.o_s = off(R.s); a.o_kc = off(R.kc); a.o_u = off(R.u); a.o_v = off(R.v); a.ibw = ctx->d_ibw;
    a.nrank = std::max(1, std::min(ctx->num_cus / 8, w->N / 8));       // workgroups per XCD of the backward launch (hank_wide.h: L2 warming)
    a.o_lwg = off(R.lwg); a.o_start = off(R.start); a.o_D = off(R.Dseq); a.o_pol = off(R.pol);
    if (!ctx->wprep_valid) {                // once per recorded primal
        const size_t npt = (size_t)c.P * c.G;
        hipLaunchKernelGGL(k_wide_prep, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, s, R.ib, R.A, R.B, npt, ctx->d_ibw);
        ctx->wprep_valid = true;
    }
    HIPC(ctx, ctx->spans.begin(TAN_BACK, s));
    int rc = w_launch(sec, false, w->N, a);
    if (rc) return rc;
    HIPC(ctx, ctx->spans.end(TAN_BACK, s, 1));
    HIPC(ctx, join_side(ctx));              // the forward sweep reads D_t and the {w, ig D} record of the primal's forward sweep
    rc = ensure_lwg(ctx);
    if (rc) return rc;
    HIPC(ctx, ctx->spans.begin(TAN_FWD, s));
    rc = w_launch(sec, true, w->N, a);
    if (rc) return rc;
    HIPC(ctx, ctx->spans.end(TAN_FWD, s, 1));
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    ctx->spans.invalidate({DUAL_BACK, DUAL_FWD});
    batch_ran(ctx, 2, w, w->N, w->dagg_cm, w->dpol);
    ctx->stats[SWEEP_LAUNCHES] += 2;
    return HANK_OK;
}
static int w_jvp(hank_ctx *ctx, const double *dxhh, hipMemcpyKind kind, int N, double *d_dagg_out) {
    WTan *w = nullptr;
    const bool staging = kind != hipMemcpyDeviceToDevice;
    int rc = w_ensure_tan(ctx, N, staging, &w);
    if (rc) return rc;
    if (staging) HIPC(ctx, hipMemcpyAsync(w->dxhh, dxhh, sizeof(double) * ctx->c.n_hh * ctx->c.P * N, kind, ctx->stream));
    rc = w_run_tangent(ctx, w, staging ? w->dxhh.get() : dxhh);
    if (rc) return rc;
    HIPC(ctx, copy_dagg(ctx, d_dagg_out, w->dagg_cm, N, hipMemcpyDeviceToDevice));
    return HANK_OK;
}

// the policy partials of the current tangent batch, whichever family ran it, as [n][t][pt] (the (G, P, N) export layout)
static int export_dpol_dev(hank_ctx *ctx, const TanBatch &b, double *out) {
    const int G = ctx->c.G, P = ctx->c.P;
    const size_t total = (size_t)P * G * b.N;
    const dim3 grd((unsigned)((total + 255) / 256)), blk(256);
    if (b.family == 2) {
        hipLaunchKernelGGL(k_wide_export_dpol, grd, blk, 0, ctx->stream, b.dpol, G, P, b.N, out);
    } else if (b.family == 1) {
        for (const XPass &ps : *b.passes) {
            const size_t cnt = (size_t)P * G * ps.N;
            hipLaunchKernelGGL(k_xexport_dpol, dim3((unsigned)((cnt + 255) / 256)), blk, 0, ctx->stream, b.dpol + ps.dpol_off, G, P, ps.groups, ps.D, ps.n0, ps.N, out);
        }
    } else {
        hipLaunchKernelGGL(k_export_dpol, grd, blk, 0, ctx->stream, b.dpol, G, P, b.N, out);
    }
    HIPC(ctx, hipGetLastError());
    return HANK_OK;
}

// ================================ C ABI =========================================================
extern "C" {

const char *hank_last_error(const hank_ctx *ctx) { return ctx ? ctx->errmsg : "null context"; }
int hank_device_available(void) {
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || hipGetDevice(&dev) != hipSuccess) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}
int hank_n_hh(const hank_ctx *ctx) { return ctx ? ctx->c.n_hh : 0; }

int hank_create(const hank_model *m, hank_ctx **out) {
    int dev = 0;
    if (out) *out = nullptr;
    if (hipGetDevice(&dev) != hipSuccess) return HANK_ERR_NO_DEVICE;
    return hank_create_on(m, dev, out);
}

int hank_create_on(const hank_model *m, int32_t device, hank_ctx **out) {
    if (!m || !out) return HANK_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return HANK_ERR_NO_DEVICE;
    hank_ctx *ctx = new (std::nothrow) hank_ctx();
    if (!ctx) return HANK_ERR_NOMEM;
    *out = ctx;  // returned even on failure so the caller can read hank_last_error, then destroy
    if (device < 0 || device >= ndev) return fail(ctx, HANK_ERR_BAD_ARG, "device %d: the process sees %d HIP device(s)", device, ndev);
    ctx->device = device;
    ENTER(ctx);
    if (m->n_a < 2 || m->n_e < 1 || m->n_e > 16 || m->T < 2)
        return fail(ctx, HANK_ERR_BAD_ARG, "bad shape: n_a=%d (>=2), n_e=%d (1..16), T=%d (>=2)", m->n_a, m->n_e, m->T);
    if (m->value_fn_id != HANK_VF_KRUSELL_SMITH && m->value_fn_id != HANK_VF_ONE_ASSET_HANK)
        return fail(ctx, HANK_ERR_BAD_ARG, "unknown value function id %d", m->value_fn_id);
    if (!m->a_grid || !m->z_grid || !m->Pi) return fail(ctx, HANK_ERR_BAD_ARG, "null grid pointer");
    for (int i = 1; i < m->n_a; i++)
        if (!(m->a_grid[i] > m->a_grid[i - 1])) return fail(ctx, HANK_ERR_BAD_ARG, "wealth grid must be strictly increasing (index %d)", i + 1);
    hipDeviceProp_t prop;
    HIPC(ctx, hipGetDeviceProperties(&prop, ctx->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ctx, HANK_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", ctx->device, prop.gcnArchName);
    Consts &c = ctx->c;
    c.n_a = m->n_a; c.n_e = m->n_e; c.G = m->n_a * m->n_e; c.P = m->T - 1;
    c.beta = m->beta; c.gamma = m->gamma; c.bc = m->borrow_cons;
    c.n_hh = m->value_fn_id == HANK_VF_ONE_ASSET_HANK ? 3 : 2;
    {   // record diet (hank_kernels.h:diet_kc): the tangent sweeps rebuild kc and v where CRRA's powers are products and a root
        const char *rd = getenv("HANK_RECORD_DIET");      // dev knob (A-B): 0 = read kc and v from the record
        c.diet = ((c.gamma == 1.0 || c.gamma == 2.0) && !(rd && atoi(rd) == 0)) ? 1 : 0;
    }
    ctx->T = m->T;
    const size_t P = c.P, G = c.G;
    if ((2 * (size_t)c.n_a + 2) * sizeof(int) > 150 * 1024) return fail(ctx, HANK_ERR_BAD_ARG, "n_a=%d too large for the LDS-staged lottery", c.n_a);
    HIPC(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    HIPC(ctx, hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
    HIPC(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPC(ctx, hipEventCreate(&ctx->ev_side));
    HIPC(ctx, ctx->spans.create());
    HIPC(ctx, ctx->d_a.alloc(c.n_a));
    HIPC(ctx, ctx->d_z.alloc(c.n_e));
    HIPC(ctx, ctx->d_Pi.alloc((size_t)c.n_e * c.n_e));
    HIPC(ctx, hipMemcpy(ctx->d_a, m->a_grid, sizeof(double) * c.n_a, hipMemcpyHostToDevice));
    HIPC(ctx, hipMemcpy(ctx->d_z, m->z_grid, sizeof(double) * c.n_e, hipMemcpyHostToDevice));
    HIPC(ctx, hipMemcpy(ctx->d_Pi, m->Pi, sizeof(double) * c.n_e * c.n_e, hipMemcpyHostToDevice));
    c.a = ctx->d_a; c.z = ctx->d_z; c.Pi = ctx->d_Pi;      // views
    ctx->h_Pi.assign(m->Pi, m->Pi + (size_t)c.n_e * c.n_e);
    ctx->h_z.assign(m->z_grid, m->z_grid + c.n_e);
    ctx->a_top = m->a_grid[c.n_a - 1];
    ctx->lds_max = prop.sharedMemPerBlock;
    ctx->num_cus = std::max(1, prop.multiProcessorCount);
    Record &R = ctx->R;
    {   // the record is ONE allocation: the on-chip wide sweeps reach every array through one buffer descriptor (hank_wide.h)
        size_t off = 0;
        const size_t d8 = P * G * sizeof(double);
        const size_t o_s = carve(off, d8), o_kc = carve(off, d8), o_A = carve(off, d8), o_B = carve(off, d8), o_u = carve(off, d8), o_v = carve(off, d8),
                     o_pol = carve(off, d8), o_lw = carve(off, d8), o_ig = carve(off, d8), o_D = carve(off, (P + 1) * G * sizeof(double)),
                     o_ib = carve(off, P * G * sizeof(int)), o_lo = carve(off, P * G * sizeof(int)),
                     o_st = carve(off, P * (size_t)c.n_e * (c.n_a + 1) * sizeof(int)), o_clo = carve(off, P * (size_t)c.n_e * sizeof(int)),
                     o_lwg = carve(off, P * G * sizeof(double2)), o_seg = carve(off, P * G * sizeof(int4));
#if HANK_XFWD_LQ
        const size_t o_lq = carve(off, P * G * sizeof(int4)), o_iga = carve(off, (size_t)c.n_a * sizeof(double));      // (behind everything else: the other arrays keep their offsets)
#endif
        HIPC(ctx, ctx->rec_slab.alloc(off));
        ctx->rec_bytes = off;
        char *b = ctx->rec_slab;
        R.s = (double *)(b + o_s); R.kc = (double *)(b + o_kc); R.A = (double *)(b + o_A); R.B = (double *)(b + o_B);
        R.u = (double *)(b + o_u); R.v = (double *)(b + o_v); R.pol = (double *)(b + o_pol); R.lw = (double *)(b + o_lw);
        R.ig = (double *)(b + o_ig); R.Dseq = (double *)(b + o_D); R.ib = (int *)(b + o_ib); R.lo = (int *)(b + o_lo);
        R.start = (int *)(b + o_st); R.clo = (int *)(b + o_clo); R.lwg = (double2 *)(b + o_lwg); R.seg = (int4 *)(b + o_seg);
#if HANK_XFWD_LQ
        ctx->rec_lq = (int4 *)(b + o_lq); ctx->rec_iga = (double *)(b + o_iga);
        hipLaunchKernelGGL(k_iga_build, dim3((unsigned)((c.n_a + 255) / 256)), dim3(256), 0, ctx->stream, c, ctx->rec_iga);
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (whichever stream a sweep runs on later, the table is there)
#endif
    }
    HIPC(ctx, ctx->d_ss_value.alloc(G));
    ctx->d_ss_D = R.Dseq;      // view
    ctx->nbp = (c.n_a + RBP - 1) / RBP;
    HIPC(ctx, ctx->d_xhh.alloc((size_t)c.n_hh * P));
    for (PathKind k : {PATH_DISCOUNT, PATH_INCOME, PATH_BORROW}) {      // no path: the kind's neutral value in every period
        hank_ctx::ExoPath &e = ctx->exo[k];
        e.h.assign((size_t)P * path_width(c, k), path_neutral(c, k));
        HIPC(ctx, e.d.alloc(e.h.size()));
        HIPC(ctx, hipMemcpy(e.d, e.h.data(), sizeof(double) * e.h.size(), hipMemcpyHostToDevice));
    }
    HIPC(ctx, ctx->d_inc_m.alloc((size_t)P * c.n_e));
    HIPC(ctx, ctx->d_agg.alloc(2 * P));
    HIPC(ctx, ctx->d_agg_rm.alloc(2 * P));
    HIPC(ctx, ctx->d_zd.alloc(2 * P));
    HIPC(ctx, ctx->d_aggpart.alloc(2 * P * (size_t)ctx->nbp));
    HIPC(ctx, ctx->d_err.alloc(4));
    HIPC(ctx, hipMemsetAsync(ctx->d_err, 0, 4 * sizeof(int), ctx->stream));
    HIPC(ctx, hipEventCreateWithFlags(&ctx->ev_stream, hipEventDisableTiming));
    // schedule (measured on MI355X): "auto" wherever the grid fits one 63-row slab per CU of an XCD —
    // the Float64 sweeps alone (hank_primal) and narrow tangent batches at a recorded primal (hank_jvp, N <= 64) run as
    // XCD-local persistent sweeps, the dual pass (hank_primal_jvp) and wide batches as per-period launches; both
    // read and write the same record. HANK_SCHEDULE=launch|xcd forces one implementation for everything (A-B, tests).
    const char *se = getenv("HANK_SCHEDULE");
    ctx->schedule = x_supported(ctx, prop.multiProcessorCount, prop.sharedMemPerBlock) ? 2 : 0;
    if (se && strcmp(se, "launch") == 0) ctx->schedule = 0;
    if (se && strcmp(se, "xcd") == 0) {
        if (ctx->schedule == 0)
            return fail(ctx, HANK_ERR_BAD_ARG, "HANK_SCHEDULE=xcd: n_a=%d needs %d workgroups per XCD (the device has %d) and %zu bytes of LDS per workgroup (it has %zu)", c.n_a,
                        (c.n_a + XRW - 1) / XRW, prop.multiProcessorCount / XG, x_lds_float64(c), (size_t)prop.sharedMemPerBlock);
        ctx->schedule = 1;
        ctx->forced_xcd = true;
    }
    // on-chip wide sweeps (hank_wide.h): "auto" sends tangent batches of at least wide_min directions to them (measured crossover,
    // DESIGN.md section 4); a forced schedule (launch | xcd) keeps its one implementation; HANK_SCHEDULE=wide sends every batch (tests)
    if (const char *wr = getenv("HANK_WIDE_R")) ctx->wide_r = atoi(wr) == 4 ? 4 : 2;
    ctx->wide_mode = (w_supported(ctx) && !(se && (strcmp(se, "launch") == 0 || strcmp(se, "xcd") == 0))) ? 1 : 0;
    if (se && strcmp(se, "wide") == 0) {
        if (!w_supported(ctx))
            return fail(ctx, HANK_ERR_BAD_ARG, "HANK_SCHEDULE=wide: %dx%d, T=%d does not fit the on-chip wide sweeps (n_e instantiated: 2,3,4,5,7,11; n_a <= %d; %zu bytes of LDS per workgroup, the device has %zu)",
                        c.n_a, c.n_e, ctx->T, WIDE_CS, w_lds(ctx), ctx->lds_max);
        ctx->wide_mode = 2;
    }
    if (const char *wm = getenv("HANK_WIDE_MIN")) ctx->wide_min = std::max(1, atoi(wm));
    if (const char *xm = getenv("HANK_XJVP_MAX")) ctx->xjvp_max = atoi(xm);
    if (const char *pm = getenv("HANK_PRIMAL_MEMO")) ctx->memo_on = atoi(pm) != 0;
    if (const char *xd = getenv("HANK_XDUAL_BACK")) ctx->xdual_back = atoi(xd) != 0;
    ctx->xw.xspec = x_spec_mode(getenv("HANK_XSPEC"));
    if (const char *xf = getenv("HANK_XDUAL_FRONT")) ctx->xw.front = atoi(xf) != 0;
    if (const char *xp = getenv("HANK_XDUAL_FRONT_POISON")) ctx->xw.front_poison = atoi(xp) != 0 ? 1 : 0;
    int rc = HANK_OK;
    if (ctx->schedule == 0) rc = build_primal_graphs(ctx);
    else rc = x_setup(ctx);
    if (rc) return rc;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

int hank_destroy(hank_ctx *ctx) {
    if (!ctx) return HANK_OK;
    ENTER(ctx);
    if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    if (ctx->ev_stream) (void)hipEventDestroy(ctx->ev_stream);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_side) (void)hipEventDestroy(ctx->ev_side);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    ctx->spans.destroy();
    const hipStream_t own = ctx->own_stream;
    delete ctx;      // both streams are idle: the members release their device memory and graphs, in any order
    if (own) (void)hipStreamDestroy(own);      // (the own stream outlives them)
    return HANK_OK;
}

int hank_set_stream(hank_ctx *ctx, void *hip_stream) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (next != ctx->stream) {      // what is still queued on the old stream (and on the side stream) happens before the new one's work
        HIPC(ctx, join_side(ctx));
        HIPC(ctx, hipEventRecord(ctx->ev_stream, ctx->stream));
        HIPC(ctx, hipStreamWaitEvent(next, ctx->ev_stream, 0));
    }
    ctx->stream = next;
    return HANK_OK;
}

int hank_sync(hank_ctx *ctx) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

int hank_set_boundary(hank_ctx *ctx, const double *ss_end_value, const double *ss_init_D) {
    ENTER(ctx);
    if (!ctx || !ss_end_value || !ss_init_D) return fail(ctx, HANK_ERR_BAD_ARG, "null boundary pointer");
    const size_t G = ctx->c.G;
    // the same boundary again (the reference's closures pass ss_end / ss_initial on every call, NewtonRaphson.jl:78-79): nothing
    // to do, and the recorded primal stays valid
    if (ctx->boundary_set && ctx->h_ss_value.size() == G && ctx->h_ss_D.size() == G &&
        memcmp(ctx->h_ss_value.data(), ss_end_value, sizeof(double) * G) == 0 && memcmp(ctx->h_ss_D.data(), ss_init_D, sizeof(double) * G) == 0) {
        ctx->errmsg[0] = 0;
        return HANK_OK;
    }
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(ctx->d_ss_value, ss_end_value, sizeof(double) * G, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(ctx->d_ss_D, ss_init_D, sizeof(double) * G, hipMemcpyHostToDevice, ctx->stream));
    {   // the productivity marginal of D_t does not depend on the policies (the lottery moves mass within a column, the exogenous
        // step mixes the columns: ForwardIteration.jl:95-99): m_t = Pi' m_{t-1} from D_0's
        const int ne = ctx->c.n_e, na = ctx->c.n_a, P = ctx->c.P;
        std::vector<double> m(ne, 0.0), m2(ne), zd(2 * (size_t)P);
        for (int e = 0; e < ne; e++) for (int i = 0; i < na; i++) m[e] += ss_init_D[(size_t)e * na + i];
        for (int t = 0; t < P; t++) {
            for (int e2 = 0; e2 < ne; e2++) { double v = 0.0; for (int e = 0; e < ne; e++) v += ctx->h_Pi[e + (size_t)ne * e2] * m[e]; m2[e2] = v; }
            m.swap(m2);
            double z = 0.0, one = 0.0;
            for (int e = 0; e < ne; e++) { z += ctx->h_z[e] * m[e]; one += m[e]; }
            zd[t] = z; zd[(size_t)P + t] = one;
        }
        HIPC(ctx, hipMemcpyAsync(ctx->d_zd, zd.data(), sizeof(double) * 2 * P, hipMemcpyHostToDevice, ctx->stream));   // (synchronised below: zd may go)
    }
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->boundary_set = true;
    record_gone(ctx);
    ctx->memo_valid = false;
    ctx->stationary = false;
    ctx->h_ss_value.assign(ss_end_value, ss_end_value + G);
    ctx->h_ss_D.assign(ss_init_D, ss_init_D + G);
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

// ---- the path in force: its one writer and the refusals that ask about it ------------------------------------
// No other code tests which path is set; what else names a kind selects that kind's graph, buffer or kernel argument.
// a kind's validity rule for the caller's values, with its message
static int path_values_ok(hank_ctx *ctx, PathKind kind, const double *v) {
    const size_t ne = ctx->c.n_e, cnt = (size_t)ctx->c.P * path_width(ctx->c, kind);
    for (size_t k = 0; k < cnt; k++) {
        if (kind == PATH_DISCOUNT && (!(v[k] > 0.0) || !(v[k] <= 1.7976931348623157e308)))
            return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_discount_path: beta_t must be finite and positive (period %zu: %g); the path in force is unchanged", k + 1, v[k]);
        if (kind == PATH_INCOME && !(v[k] >= -1.7976931348623157e308 && v[k] <= 1.7976931348623157e308))
            return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_income_path: y must be finite (state %zu, period %zu: %g); the path in force is unchanged", k % ne + 1, k / ne + 1, v[k]);
        if (kind == PATH_BORROW && !(v[k] >= -1.7976931348623157e308 && v[k] <= ctx->a_top))
            return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_borrow_path: amin_t must be finite and at most a_grid[n_a-1] = %g (period %zu: %g); the path in force is unchanged", ctx->a_top,
                        k + 1, v[k]);
    }
    return HANK_OK;
}
// hank_set_discount_path (hank_shock.h; KrusellSmith.jl:59-62, BackwardIteration.jl:90-113): beta_t [P]; hank_set_income_path
// (hank_income.h; KrusellSmith.jl:59-62, :66-80 inside the same loop): y (n_e, P) column-major — on the host, or null for no path of the
// kind (its neutral value in every period). THE rule that the kinds exclude each other. What a new boundary invalidates goes: the
// record, both current batches, the memo.
static int set_path(hank_ctx *ctx, PathKind kind, const double *values) {
    ENTER(ctx);
    if (!ctx) return HANK_ERR_BAD_ARG;
    hank_ctx::ExoPath &e = ctx->exo[kind];
    if (!values && ctx->path != kind) { ctx->errmsg[0] = 0; return HANK_OK; }      // (no path to clear: nothing changes)
    if (ctx->path != PATH_NONE && ctx->path != kind)
        return fail(ctx, HANK_ERR_NOT_READY, "%s: %s is set and the two exclude each other (%s(ctx, NULL) clears it)", PATHS[kind].set, PATHS[ctx->path].a_path, PATHS[ctx->path].set);
    if (values) { const int vrc = path_values_ok(ctx, kind, values); if (vrc) return vrc; }
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (sweeps in flight read the values)
    if (values) e.h.assign(values, values + e.h.size());
    else e.h.assign(e.h.size(), path_neutral(ctx->c, kind));
    HIPC(ctx, hipMemcpyAsync(e.d, e.h.data(), sizeof(double) * e.h.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->path = values ? kind : PATH_NONE;
    record_gone(ctx);
    ctx->memo_valid = false;
    ctx->stationary = false;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}
int hank_set_discount_path(hank_ctx *ctx, const double *beta_t) { return set_path(ctx, PATH_DISCOUNT, beta_t); }
int hank_set_income_path(hank_ctx *ctx, const double *y) { return set_path(ctx, PATH_INCOME, y); }
// (hank_borrow.h; KrusellSmith.jl:52, :76 inside the same loop): amin_t [P]
int hank_set_borrow_path(hank_ctx *ctx, const double *amin_t) { return set_path(ctx, PATH_BORROW, amin_t); }
// a path of any kind: the sweeps run on the per-period launches
static bool path_on(const hank_ctx *ctx) { return ctx->path != PATH_NONE; }
// the income values in force as k_inc_cons takes them: null without an income path
static const double *income_in_force(const hank_ctx *ctx) { return ctx->path == PATH_INCOME ? ctx->exo[PATH_INCOME].d.get() : nullptr; }
// an entry that is not served while a path of `kind` is set
static int refuses_at(hank_ctx *ctx, PathKind kind, const char *name) {
    if (ctx && ctx->path == kind)
        return fail(ctx, HANK_ERR_NOT_READY, "%s %s: a path is set (%s(ctx, NULL) clears it)", name, PATHS[kind].refusal, PATHS[kind].set);
    return HANK_OK;
}
// the entries that rebuild consumption from the inputs (w z_e + tr) or carry seeds the income entries do not, while an income path is set
static int income_refuses(hank_ctx *ctx, const char *name) { return refuses_at(ctx, PATH_INCOME, name); }
// the entries that are defined at ONE beta and ONE income process (the scenario and steady-state entries, the Toeplitz Jacobians) while a path is set
static int path_refuses(hank_ctx *ctx, const char *name) {
    for (PathKind k : {PATH_DISCOUNT, PATH_INCOME, PATH_BORROW}) {
        const int rc = refuses_at(ctx, k, name);
        if (rc) return rc;
    }
    return HANK_OK;
}
// a kind's own jvp / vjp entry (`who`) while a kind that excludes it is set (PathTraits::excluded_under): hank_jvp_income under a discount-factor path,
// every kind's under a borrowing-limit path and the limit's under either of theirs — one path at a time
static int path_entry_excluded(hank_ctx *ctx, PathKind kind, const char *who) {
    const PathKind other = ctx->path;
    if (other != PATH_NONE && (PATHS[kind].excluded_under >> other & 1u)) return fail(ctx, HANK_ERR_NOT_READY, "%s: %s is set and the two exclude each other", who, PATHS[other].a_path);
    return HANK_OK;
}
// the column masses of the recorded distributions, for the first reader at this record (the main stream has joined the forward sweep)
static int ensure_inc_mass(hank_ctx *ctx) {
    if (ctx->inc_m_valid) return HANK_OK;
    hipLaunchKernelGGL(k_inc_mass, dim3((unsigned)ctx->c.n_e, (unsigned)ctx->c.P), dim3(256), 0, ctx->stream, ctx->c, ctx->R, ctx->d_inc_m.get());
    HIPC(ctx, hipGetLastError());
    ctx->inc_m_valid = true;
    return HANK_OK;
}

// which x the record belongs to: the host-pointer entries know it (and whether it is a constant path), the device-pointer
// entries do not
static void note_primal_x(hank_ctx *ctx, const double *xhh) {
    const size_t n = (size_t)ctx->c.n_hh * ctx->c.P, nh = ctx->c.n_hh;
    if (!xhh) { ctx->memo_valid = false; ctx->stationary = false; return; }
    ctx->memo_xhh.assign(xhh, xhh + n);
    ctx->memo_valid = true;
    bool constant = true;
    for (size_t k = nh; k < n && constant; k++) constant = xhh[k] == xhh[k - nh];
    ctx->stationary = constant;      // (hank_fake_news also compares the first and the last recorded policy on the device)
}

static int run_primal(hank_ctx *ctx, double *d_agg_out) {
    { const int grc = ensure_primal_graphs(ctx, ctx->path); if (grc) return grc; }      // (whatever the schedule: a path runs on the launches)
    HIPC(ctx, join_side(ctx));     // a previous forward sweep still reads the record this one overwrites
    HIPC(ctx, ctx->spans.begin(PRIMAL_BACK, ctx->stream));
    HIPC(ctx, hipGraphLaunch(ctx->exo[ctx->path].g_pback, ctx->stream));
    HIPC(ctx, ctx->spans.end(PRIMAL_BACK, ctx->stream, ctx->c.P + 2));
    // fork: the distribution sweep goes to the side stream; the main stream is free for the tangent
    // backward sweep and joins (join_side) before anything that needs D_t or the aggregates
    HIPC(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPC(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    HIPC(ctx, ctx->spans.begin(PRIMAL_FWD, ctx->side_stream));
    HIPC(ctx, hipGraphLaunch(ctx->g_pfwd, ctx->side_stream));
    HIPC(ctx, ctx->spans.end(PRIMAL_FWD, ctx->side_stream, ctx->c.P + 1));
    HIPC(ctx, copy_agg(ctx, d_agg_out, hipMemcpyDeviceToDevice, ctx->side_stream));
    HIPC(ctx, hipEventRecord(ctx->ev_side, ctx->side_stream));
    ctx->side_pending = true;
    ctx->spans.invalidate({DUAL_BACK, DUAL_FWD});
    record_rewritten(ctx, true, true);
    return HANK_OK;
}

// ---- xcd schedule: entry-point bodies --------------------------------------------------------------
// One body per shape of call. Each opens the call's ONE section, enqueues its steps top to bottom, closes the section and does
// its bookkeeping: what the record now holds, which spans are valid, the launch count, and the sync blocks x_status will read.
// P (hank_primal[_dev]): the Float64 recurrences at x — the policy sequence, the distribution path and the linearisation record
static int x_primal(hank_ctx *ctx, const double *xhh, hipMemcpyKind kind, double *d_agg_out) {
    int rc = x_setup(ctx); if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(ctx->d_xhh, xhh, sizeof(double) * ctx->c.n_hh * ctx->c.P, kind, ctx->stream));
    XSection sec(ctx);
    HIPC(ctx, sec.opened());
    rc = x_sync_reset(sec, ctx->xw.sync, 2, 1); if (rc) return rc;
    zero_err(ctx, sec.stream());
    x_rho(sec);
    rc = x_back(sec); if (rc) return rc;
    x_lottery(sec, true);
    record_rewritten(ctx, true, true);
    x_ensure_rng(sec);
    rc = x_fwd_value(sec); if (rc) return rc;
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    ctx->stats[SWEEP_LAUNCHES] += 2;
    ctx->xw.last_blocks = 2;
    ctx->spans.invalidate({TAN_BACK, TAN_FWD, DUAL_BACK, DUAL_FWD});
    HIPC(ctx, copy_agg(ctx, d_agg_out, hipMemcpyDeviceToDevice, ctx->stream));
    return HANK_OK;
}
// T (hank_jvp[_dev]): the N partials at the recorded primal — linear recurrences at that record, so a y-iteration pays the Float64
// sweeps once (NewtonRaphson.jl:91) and each JVP (:95) only these: two persistent launches per pass of up to 8*dmax directions
static int x_jvp(hank_ctx *ctx, const double *dxhh, hipMemcpyKind kind, int N, double *d_dagg_out) {
    int rc = x_setup(ctx); if (rc) return rc;
    XTan *w = nullptr;
    rc = x_ensure_tan(ctx, N, &w); if (rc) return rc;
    const int np = (int)w->passes.size();
    HIPC(ctx, hipMemcpyAsync(w->dxhh, dxhh, sizeof(double) * ctx->c.n_hh * ctx->c.P * N, kind, ctx->stream));
    XSection sec(ctx);
    HIPC(ctx, sec.opened());
    rc = x_tan_front(sec, w); if (rc) return rc;
    x_ensure_rng(sec);
    rc = x_tan_back(sec, w); if (rc) return rc;
    HIPC(ctx, ctx->spans.begin(TAN_FWD, sec.stream()));
    rc = x_tan_fwd_from(sec, w, 0); if (rc) return rc;
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    ctx->stats[SWEEP_LAUNCHES] += 2 * np;
    ctx->xw.last_blocks = 2 + 2 * np;
    ctx->spans.invalidate({DUAL_BACK, DUAL_FWD});
    batch_ran(ctx, 1, w, N, w->dagg_cm, w->dpol, &w->passes);
    HIPC(ctx, copy_dagg(ctx, d_dagg_out, w->dagg_cm, N, hipMemcpyDeviceToDevice));
    return HANK_OK;
}
// what a Dual pass leaves behind whichever sweeps carried it: the Float64 forward sweep rode on pass 0's (PRIMAL_FWD has no events
// of its own and keeps a sweep's count of one launch), and x_status reads the primal's sync blocks and every pass's
static void x_dual_ran(hank_ctx *ctx, XTan *w, int launches) {
    ctx->stats[SWEEP_LAUNCHES] += launches;
    ctx->xw.last_blocks = 2 + 2 * (int)w->passes.size();
    ctx->spans.absent(PRIMAL_FWD, 1);
    ctx->spans.invalidate({DUAL_BACK, DUAL_FWD});
    batch_ran(ctx, 1, w, w->N, w->dagg_cm, w->dpol, &w->passes);
}
// D2 (hank_primal_jvp[_dev] of several passes, or whose backward sweeps do not fuse): P's backward half, T's backward sweeps at the
// record it wrote, and the Float64 distribution sweep on the forward sweep of pass 0 (k_xfwd<D, true>): 1 + 2 np persistent launches
static int x_dual_two(hank_ctx *ctx, XTan *w, const double *xhh, const double *dxhh, hipMemcpyKind kind, double *d_agg_out, double *d_dagg_out) {
    const size_t nP = (size_t)ctx->c.n_hh * ctx->c.P;
    const int np = (int)w->passes.size();
    XSection sec(ctx);
    HIPC(ctx, sec.opened());
    HIPC(ctx, hipMemcpyAsync(w->dxhh, dxhh, sizeof(double) * nP * w->N, kind, sec.stream()));
    HIPC(ctx, hipMemcpyAsync(ctx->d_xhh, xhh, sizeof(double) * nP, kind, sec.stream()));
    int rc = x_sync_reset(sec, ctx->xw.sync, 2, 1); if (rc) return rc;
    zero_err(ctx, sec.stream());
    x_rho(sec);
    rc = x_back(sec); if (rc) return rc;
    x_lottery(sec, true, true);
    record_rewritten(ctx, true, false);       // (no forward sweep of a Dual pass writes the per-source records)
    x_ensure_rng(sec);
    rc = x_tan_front(sec, w);
    if (!rc) rc = x_tan_back(sec, w);
    if (rc) return rc;
    HIPC(ctx, ctx->spans.begin(TAN_FWD, sec.stream()));
    rc = x_tan_fwd(sec, w, 0, true); if (rc) return rc;
    if (np == 1) {
        HIPC(ctx, ctx->spans.end(TAN_FWD, sec.stream(), 1));
        x_dual_epilogue(sec, w, d_agg_out, d_dagg_out);
    } else {
        x_value_epilogue(sec);
        x_tan_reduce(sec, w, 0);
        rc = x_tan_fwd_from(sec, w, 1); if (rc) return rc;
    }
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    x_dual_ran(ctx, w, 1 + 2 * np);
    if (np > 1) {       // (k_xdual_epilogue has written the caller's buffers)
        HIPC(ctx, copy_agg(ctx, d_agg_out, hipMemcpyDeviceToDevice, ctx->stream));
        HIPC(ctx, copy_dagg(ctx, d_dagg_out, w->dagg_cm, w->N, hipMemcpyDeviceToDevice));
    }
    return HANK_OK;
}
// D1 (the one-pass hank_primal_jvp[_dev], N <= 8 groups x 4: what bench.py times): value and partials together in BOTH sweeps
// (k_xdual_back, k_xfwd<D, true>), two persistent launches. prologue: the inputs are device-resident and no fault is injected, so ONE
// launch in front of the sweeps (k_xdual_prologue) stands for the seven launches, copies and memsets of the separate front
static int x_dual_fused(hank_ctx *ctx, XTan *w, const double *xhh, const double *dxhh, hipMemcpyKind kind, bool prologue, double *d_agg_out, double *d_dagg_out) {
    XWork &X = ctx->xw;
    const size_t nP = (size_t)ctx->c.n_hh * ctx->c.P;
    XSection sec(ctx);        // (the sync blocks about to be zeroed may belong to a sweep still in flight on another stream)
    HIPC(ctx, sec.opened());
    if (prologue) {
        hipLaunchKernelGGL(k_xdual_prologue, dim3(64), dim3(256), 0, sec.stream(), xhh, ctx->d_xhh, dxhh, w->dxhh, ctx->c.n_hh, ctx->c.P, w->N, X.rho, w->dxr, w->dxw, w->dxt,
                           reinterpret_cast<xv4u *>(X.sync.get()), sizeof(XSync) * 4 / sizeof(xv4u), ctx->d_err);
    } else {
        HIPC(ctx, hipMemcpyAsync(w->dxhh, dxhh, sizeof(double) * nP * w->N, kind, sec.stream()));
        HIPC(ctx, hipMemcpyAsync(ctx->d_xhh, xhh, sizeof(double) * nP, kind, sec.stream()));
        int rc = x_sync_reset(sec, X.sync, 2, 1);
        if (!rc) rc = x_sync_reset(sec, X.sync + 2, 2, 2);
        if (rc) return rc;
        zero_err(ctx, sec.stream());
        x_rho(sec);
        x_tan_in(sec, w);
    }
    int rc = x_back(sec, w); if (rc) return rc;
    if (X.front && X.stageU && ctx->rec_lq && x_fwd_serves_lq(X, ctx->c, w->passes[0].D)) {
        // the lean front: k_xfwd<D, true, ., true> reads lq, clo, the grid's inverse gaps and the work units, and nothing else of the lottery
        x_front(sec);
        record_rewritten(ctx, false, false, false);
        X.rng_valid = true;
    } else {
        x_lottery(sec, false, true);
        record_rewritten(ctx, false, false);
        x_ensure_rng(sec);
    }
    HIPC(ctx, ctx->spans.begin(TAN_BACK, sec.stream()));      // (brackets nothing: k_xdual_back is PRIMAL_BACK's. The readers of
    HIPC(ctx, ctx->spans.end(TAN_BACK, sec.stream(), 1));      // hank_last_timings count on a valid slot of about 0 ms)
    HIPC(ctx, ctx->spans.begin(TAN_FWD, sec.stream()));
    rc = x_tan_fwd(sec, w, 0, true); if (rc) return rc;
    HIPC(ctx, ctx->spans.end(TAN_FWD, sec.stream(), 1));
    x_dual_epilogue(sec, w, d_agg_out, d_dagg_out);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    x_dual_ran(ctx, w, 2);
    return HANK_OK;
}
// hank_primal_jvp[_dev] on the persistent sweeps: which shape, decided once
static bool x_dual_back_fits(const hank_ctx *ctx, int D);
static int x_dual(hank_ctx *ctx, const double *xhh, const double *dxhh, hipMemcpyKind kind, int N, double *d_agg_out, double *d_dagg_out) {
    int rc = x_setup(ctx); if (rc) return rc;
    XTan *w = nullptr;
    rc = x_ensure_tan(ctx, N, &w); if (rc) return rc;
    if (w->passes.size() != 1 || !x_dual_back_fits(ctx, w->passes[0].D)) return x_dual_two(ctx, w, xhh, dxhh, kind, d_agg_out, d_dagg_out);
    return x_dual_fused(ctx, w, xhh, dxhh, kind, kind == hipMemcpyDeviceToDevice && !ctx->xw.fault, d_agg_out, d_dagg_out);      // (a fault-injection run, HANK_XFAULT, keeps the separate launches)
}
static bool use_x_primal(const hank_ctx *ctx) { return ctx->schedule >= 1; }
// the persistent tangent sweeps' LDS grows with the horizon too (the group's dr/dw/dtr of every period): a long horizon goes
// to the per-period launches, which take any T
static bool x_tan_fits(const hank_ctx *ctx, int N) {
    const XWork &X = ctx->xw;
    int D = 1;
    while (XG * D < N && D < X.dmax) D *= 2;
    return std::max(x_lds_tan_back(ctx->c, D), x_lds_fwd(ctx->c, D, true)) <= (size_t)X.lds_max;
}
static bool use_x_jvp(const hank_ctx *ctx, int N) { return (ctx->schedule == 1 || (ctx->schedule == 2 && N <= ctx->xjvp_max)) && x_tan_fits(ctx, N); }
// hank_primal_jvp on the persistent sweeps. Forced schedule: always. auto: a batch of ONE pass (N <= 8 groups x 4) runs value and
// partials together in both sweeps (k_xdual_back, k_xfwd<D, true>: 4.8 ms against 5.13 for the dual-sweep launches at 2000x11,
// T=300, N=32; 3.3 against 4.2 at N=1); wider batches would be two backward sweeps at the same record: the launches keep them
static bool x_dual_back_fits(const hank_ctx *ctx, int D) {
    const XWork &X = ctx->xw;
    return ctx->xdual_back && x_has_dual_back(X) && 64 * (ctx->c.n_e + 1) <= X.maxt && x_lds_dual_back(ctx->c, D) <= (size_t)X.lds_max;
}
static bool use_x_fused(const hank_ctx *ctx, int N) {
    if (ctx->schedule < 1 || !x_tan_fits(ctx, N) || !x_dual_addr_fits(ctx)) return false;
    if (ctx->schedule == 1) return true;
    return N <= XG * ctx->xw.dmax && x_dual_back_fits(ctx, ctx->xw.dmax);
}

static int check_rates(hank_ctx *ctx, const double *xhh) {      // the host-pointer entries see x before the device does
    for (int t = 0; t < ctx->c.P; t++)
        if (!(1.0 + xhh[ctx->c.n_hh * t] > 0.0)) return fail(ctx, HANK_ERR_DOMAIN, "1 + r must be positive (period %zu)", (size_t)t + 1);
    return HANK_OK;
}
// hank_primal[_dev]: x from the caller (kind: where it lives) and the Float64 sweeps of the context's schedule
static int enqueue_primal(hank_ctx *ctx, const double *xhh, hipMemcpyKind kind, double *d_agg_out) {
    if (!path_on(ctx) && use_x_primal(ctx)) return x_primal(ctx, xhh, kind, d_agg_out);      // (a path: the launches, the schedule left as it is)
    HIPC(ctx, hipMemcpyAsync(ctx->d_xhh, xhh, sizeof(double) * ctx->c.n_hh * ctx->c.P, kind, ctx->stream));
    return run_primal(ctx, d_agg_out);
}

int hank_primal_dev(hank_ctx *ctx, const double *d_xhh, double *d_agg_out) {
    ENTER(ctx);
    if (!ctx || !d_xhh) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    if (!ctx->boundary_set) return fail(ctx, HANK_ERR_NOT_READY, "hank_set_boundary must be called first");
    note_primal_x(ctx, nullptr);
    ctx->stats[PRIMAL_SWEEPS]++;
    return enqueue_primal(ctx, d_xhh, hipMemcpyDeviceToDevice, d_agg_out);
}

int hank_check(hank_ctx *ctx) {
    ENTER(ctx);
    if (!ctx) return HANK_ERR_BAD_ARG;
    // the asynchronous entries cannot re-run a call: the error is reported (once, and a model error leaves no tangent batch current),
    // and a context whose schedule was not forced continues on the per-period launches, so the caller's next call succeeds
    bool moved = false;
    const int rc = fallback_decision(ctx, device_verdict(ctx, THE_RECORD), &moved);
    return rc ? rc : scen_pending_verdict(ctx);      // (then what a hank_primal_batch_dev left: its own words, THIS_CALL)
}

int hank_primal(hank_ctx *ctx, const double *xhh, double *agg_out) {
    ENTER(ctx);
    if (!ctx || !xhh) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    if (!ctx->boundary_set) return fail(ctx, HANK_ERR_NOT_READY, "hank_set_boundary must be called first");
    { const int rrc = check_rates(ctx, xhh); if (rrc) return rrc; }
    note_primal_x(ctx, nullptr);
    const int rc = run_settled(ctx, [&] { return enqueue_primal(ctx, xhh, hipMemcpyHostToDevice, nullptr); });
    if (rc) return rc;
    if (agg_out) {
        HIPC(ctx, copy_agg(ctx, agg_out, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
    }
    note_primal_x(ctx, xhh);
    ctx->stats[PRIMAL_SWEEPS]++;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

// bnd: the graphs with the boundary's seeds (hank_jvp_boundary: w.bnd_dV and w.bnd_dD hold them); zm: whether a dD_0 seed is among them
// NX > 0 (hank_jvp_het): the forward graph with that many extra reductions, one launch more (k_reduce_hx)
// kind (hank_jvp_shock, hank_jvp_income; never with bnd): the kind's backward graph with its seeds, 2 P + 3 launches
static int run_jvp(hank_ctx *ctx, TanWork &w, bool bnd, bool zm, int NX, PathKind kind = PATH_NONE) {
    const bool seeded = kind != PATH_NONE;
    int grc = ensure_tan_graphs(ctx, w, bnd, NX);
    if (!grc && seeded) grc = ensure_path_tan_graph(ctx, w, kind);
    if (grc) return grc;
    HIPC(ctx, ctx->spans.begin(TAN_BACK, ctx->stream));
    HIPC(ctx, hipGraphLaunch(seeded ? w.seed[kind].g_tback : w.tan_back(bnd), ctx->stream));
    HIPC(ctx, ctx->spans.end(TAN_BACK, ctx->stream, seeded ? 2 * ctx->c.P + 3 : ctx->c.P + (bnd ? 4 : 2)));
    HIPC(ctx, join_side(ctx));      // the tangent forward sweep needs D_t
    { const int src = ensure_seg(ctx); if (src) return src; }
    { const int src = ensure_lwg(ctx); if (src) return src; }
    HIPC(ctx, ctx->spans.begin(TAN_FWD, ctx->stream));
    HIPC(ctx, hipGraphLaunch(w.tan_fwd(bnd, NX), ctx->stream));
    HIPC(ctx, ctx->spans.end(TAN_FWD, ctx->stream, ctx->c.P + (bnd ? 5 : 3) + (NX > 0 ? 1 : 0)));
    if (bnd) batch_ran_boundary(ctx, &w, w.N, w.dagg_cm, w.dpol, zm ? w.bnd_zm.get() : nullptr);
    else batch_ran(ctx, 0, &w, w.N, w.dagg_cm, w.dpol);
    return HANK_OK;
}

// One request to the launch family's tangent sweeps, whatever the context's schedule and whichever family wrote the record (any primal
// serves any tangent sweep: run_jvp's ensure_seg / ensure_lwg). hank_jvp, hank_jvp_boundary and hank_jvp_het are this with options.
struct TanReq {
    int n_het;                                     // 0: the raw aggregates (P, 2 N); >= 1: hank_jvp_het's (P, n_het, N), the entry's rule has checked the count
    const double *dxhh, *dvalue_end, *dD_init;     // the directions and the boundary's seeds, (.., N) column-major; null: zero
    hipMemcpyKind kind;                            // where they live
    bool seeded;                                   // run the graphs with the seed kernels: hank_jvp_boundary always (null seeds too),
                                                   // hank_jvp_het when a seed is given, hank_jvp never — NOT derived from the pointers
    PathKind path = PATH_NONE;                     // run the backward graph with this kind's seeds (hank_jvp_shock, hank_jvp_income always, null directions too)
    const double *dpath = nullptr;                 // the directions in the kind's values — dbeta (P, N), dy (n_e, P, N), column-major; null: zero
};
static int ensure_bnd_bufs(hank_ctx *ctx, TanWork &w);
static int ensure_hx_record(hank_ctx *ctx);
static int ensure_grp_record(hank_ctx *ctx);

// the one enqueue of a request: the workspace of this width, every buffer a graph names (before any capture: the graph holds their
// addresses), the inputs, the sweeps. batch_ran has named the batch when this returns HANK_OK; the copy-out is the entry's.
static int enqueue_tan_launch(hank_ctx *ctx, const TanReq &q, int N, TanWork **out) {
    const Consts &c = ctx->c;
    const size_t P = c.P, GN = (size_t)c.G * N;
    const int NX = q.n_het > 2 ? q.n_het - 2 : 0, SX = hx_count(ctx);
    TanWork *w = nullptr;
    int rc = ensure_tanwork(ctx, N, &w);
    if (rc) return rc;
    if (q.seeded && (rc = ensure_bnd_bufs(ctx, *w)) != HANK_OK) return rc;
    if (q.n_het > 0 && !w->het_out) HIPC(ctx, w->het_out.alloc(P * het_max(ctx) * N));
    if (NX > 0) {
        HIPC(ctx, join_side(ctx));      // the record's sums read D_t
        rc = ensure_hx_record(ctx);
        if (rc) return rc;
        if (!w->hx_T) {
            HIPC(ctx, w->hx_parts.alloc(P * (size_t)w->nbf * SX * N));
            HIPC(ctx, w->hx_T.alloc((size_t)N * P * SX));      // (last: a failed allocation is tried again by the next call)
        }
    }
    const struct { double *dst; const double *src; size_t count; } in[3] = {{w->dxhh, q.dxhh, c.n_hh * P * N}, {w->bnd_dV, q.dvalue_end, GN}, {w->bnd_dD, q.dD_init, GN}};
    for (int k = 0; k < (q.seeded ? 3 : 1); k++) {
        if (in[k].src) HIPC(ctx, hipMemcpyAsync(in[k].dst, in[k].src, sizeof(double) * in[k].count, q.kind, ctx->stream));
        else HIPC(ctx, hipMemsetAsync(in[k].dst, 0, sizeof(double) * in[k].count, ctx->stream));
    }
    if (q.path != PATH_NONE) {      // the path directions staged or zeroed (their buffers, and the kind's graph, before that)
        rc = ensure_path_tan_graph(ctx, *w, q.path);
        if (rc) return rc;
        const size_t bytes = sizeof(double) * P * path_width(c, q.path) * N;
        if (q.dpath) HIPC(ctx, hipMemcpyAsync(w->seed[q.path].in, q.dpath, bytes, q.kind, ctx->stream));
        else HIPC(ctx, hipMemsetAsync(w->seed[q.path].in, 0, bytes, ctx->stream));
    }
    rc = run_jvp(ctx, *w, q.seeded, q.dD_init != nullptr, NX, q.path);
    if (rc) return rc;
    if (q.path == PATH_INCOME && q.dpath) batch_ran_income(ctx, w->seed[PATH_INCOME].in);      // (a null dy is hank_jvp's batch; beta_t has no direct term to mark)
    *out = w;
    return HANK_OK;
}
// a request for the raw aggregates and its device copy-out (hank_jvp's launch-family branch, hank_jvp_boundary)
static int enqueue_tan_raw(hank_ctx *ctx, const TanReq &q, int N, double *d_dagg_out) {
    TanWork *w = nullptr;
    const int rc = enqueue_tan_launch(ctx, q, N, &w);
    if (rc) return rc;
    HIPC(ctx, copy_dagg(ctx, d_dagg_out, w->dagg_cm, N, hipMemcpyDeviceToDevice));
    return HANK_OK;
}
// the host forms' tail: the result to the caller, the stream drained, the call a success
static int tan_host_tail(hank_ctx *ctx, double *out, const double *d_src, size_t count) {
    HIPC(ctx, hipMemcpyAsync(out, d_src, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->errmsg[0] = 0;
    return HANK_OK;
}
// the rule of the entries that take seeds: the arguments, then (het) the count (hank_vjp_het's rule), then the record
static int tan_seed_args(hank_ctx *ctx, const char *who, bool het, const TanReq &q, int N, const void *out, bool need_out) {
    if (!ctx || (!q.dxhh && !q.dvalue_end && !q.dD_init) || (need_out && !out) || N < 1)
        return fail(ctx, HANK_ERR_BAD_ARG, "%s: bad argument (N=%d; at least one of dxhh, dvalue_end, dD_init must be given)", who, N);
    int rc = het ? het_count_ok(ctx, who, q.n_het, true) : HANK_OK;
    if (!rc) rc = income_refuses(ctx, who);
    if (rc) return rc;
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before %s", who);
    return HANK_OK;
}

// hank_jvp[_dev]: N directions from the caller (kind: where they live) through the tangent sweeps of the family that serves
// this width at the recorded primal; batch_ran has named the family and its buffers when this returns HANK_OK
static int enqueue_jvp(hank_ctx *ctx, const double *dxhh, hipMemcpyKind kind, int N, double *d_dagg_out) {
    // at a record written under a discount-factor path the persistent and the wide tangent sweeps would rebuild kc with the model's
    // beta (diet_kc): the launches read it from the record
    if (!path_on(ctx) && use_wide(ctx, N)) return w_jvp(ctx, dxhh, kind, N, d_dagg_out);
    if (!path_on(ctx) && use_x_jvp(ctx, N)) return x_jvp(ctx, dxhh, kind, N, d_dagg_out);
    return enqueue_tan_raw(ctx, TanReq{0, dxhh, nullptr, nullptr, kind, false}, N, d_dagg_out);
}

int hank_jvp_dev(hank_ctx *ctx, const double *d_dxhh, int32_t N, double *d_dagg_out) {
    ENTER(ctx);
    if (!ctx || !d_dxhh || N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument (N=%d)", N);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before hank_jvp");
    return enqueue_jvp(ctx, d_dxhh, hipMemcpyDeviceToDevice, N, d_dagg_out);
}

int hank_jvp(hank_ctx *ctx, const double *dxhh, int32_t N, double *dagg_out) {
    ENTER(ctx);
    if (!ctx || !dxhh || !dagg_out || N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument (N=%d)", N);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before hank_jvp");
    int rc = enqueue_jvp(ctx, dxhh, hipMemcpyHostToDevice, N, nullptr);
    if (rc) return rc;
    // the launches' tangent sweeps raise no device error: nothing to ask (and no synchronisation beyond the copy-out's); the
    // on-chip wide sweeps do, but have no cross-workgroup waits: nothing to fall back from
    if (ctx->batch.family == 2) rc = device_verdict(ctx, THE_RECORD);
    else if (ctx->batch.family == 1) {
        bool rerun = false;
        rc = settle(ctx, &rerun);
        if (rerun) {                             // this entry's extra step: re-record the primal at the current x with the launches
            rc = run_primal(ctx, nullptr);
            if (!rc) rc = device_verdict(ctx, THE_RECORD);
            if (!rc) rc = enqueue_jvp(ctx, dxhh, hipMemcpyHostToDevice, N, nullptr);
        }
    }
    if (rc) return rc;
    return tan_host_tail(ctx, dagg_out, ctx->batch.dagg_cm, (size_t)ctx->c.P * N);
}

// hank_jvp_boundary[_dev]: the request with the boundary's seeds, always on the seeded graphs. A null input is a zero seed. The
// schedule is left as it is.
// Pi^{t+1} z and Pi^{t+1} 1, t = 0 .. P-1, once per context (k_bnd_mpath dots the seed's productivity marginal with them)
static int ensure_bnd_q(hank_ctx *ctx) {
    if (ctx->d_bnd_q) return HANK_OK;
    const int ne = ctx->c.n_e, P = ctx->c.P;
    std::vector<double> Q(2 * (size_t)P * ne), q(ctx->h_z), o(ne, 1.0), q2(ne), o2(ne);
    for (int t = 0; t < P; t++) {
        for (int e = 0; e < ne; e++) {
            double a = 0.0, b = 0.0;
            for (int e2 = 0; e2 < ne; e2++) { a += ctx->h_Pi[e + (size_t)ne * e2] * q[e2]; b += ctx->h_Pi[e + (size_t)ne * e2] * o[e2]; }
            q2[e] = a; o2[e] = b;
        }
        q.swap(q2); o.swap(o2);
        for (int e = 0; e < ne; e++) { Q[(size_t)t * ne + e] = q[e]; Q[((size_t)P + t) * ne + e] = o[e]; }
    }
    DevBuf<double> buf;
    HIPC(ctx, buf.alloc(Q.size()));
    // on the context's stream, not the legacy one: a copy there would join every blocking stream of the process, and another
    // context of this GPU (parallel.DeviceGroup) may be capturing a graph on its own
    HIPC(ctx, hipMemcpyAsync(buf, Q.data(), sizeof(double) * Q.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (Q is this call's)
    ctx->d_bnd_q = std::move(buf);
    return HANK_OK;
}
// the seeds' buffers of a workspace and the model's Q, before the first capture with seeds at this width
static int ensure_bnd_bufs(hank_ctx *ctx, TanWork &w) {
    const size_t P = ctx->c.P, GN = (size_t)ctx->c.G * w.N;
    const int rc = ensure_bnd_q(ctx);
    if (rc) return rc;
    if (!w.bnd_zm) {
        HIPC(ctx, w.bnd_dV.alloc(GN));
        HIPC(ctx, w.bnd_dD.alloc(GN));
        HIPC(ctx, w.bnd_m0.alloc((size_t)w.N * ctx->c.n_e));
        HIPC(ctx, w.bnd_zm.alloc(2 * P * w.N));      // (last: a failed allocation is tried again by the next call)
    }
    return HANK_OK;
}
int hank_jvp_boundary_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dvalue_end, const double *d_dD_init, int32_t N, double *d_dagg_out) {
    ENTER(ctx);
    const TanReq q{0, d_dxhh, d_dvalue_end, d_dD_init, hipMemcpyDeviceToDevice, true};
    const int rc = tan_seed_args(ctx, "hank_jvp_boundary", false, q, N, d_dagg_out, false);
    return rc ? rc : enqueue_tan_raw(ctx, q, N, d_dagg_out);
}

int hank_jvp_boundary(hank_ctx *ctx, const double *dxhh, const double *dvalue_end, const double *dD_init, int32_t N, double *dagg_out) {
    ENTER(ctx);
    const TanReq q{0, dxhh, dvalue_end, dD_init, hipMemcpyHostToDevice, true};
    int rc = tan_seed_args(ctx, "hank_jvp_boundary", false, q, N, dagg_out, true);
    if (!rc) rc = enqueue_tan_raw(ctx, q, N, nullptr);
    if (rc) return rc;
    // (the launches' tangent sweeps raise no device error: nothing to ask, as in hank_jvp)
    return tan_host_tail(ctx, dagg_out, ctx->batch.dagg_cm, (size_t)ctx->c.P * N);
}

// hank_jvp_shock[_dev] (hank_shock.h), hank_jvp_income[_dev] (hank_income.h), hank_jvp_borrow[_dev] (hank_borrow.h): the request with the
// kind's seeds — d beta_t, d y_t[e], d amin_t —
// always on the launches' graphs with the seed kernels; a null input is a zero seed. Named as hank_jvp names its batch. The four
// entries' one body; the rule differs by kind in its messages and in path_entry_excluded alone.
static int jvp_path(hank_ctx *ctx, PathKind kind, const double *dxhh, const double *dpath, int N, double *out, bool dev) {
    ENTER(ctx);
    const PathTraits &pt = PATHS[kind];
    if (!ctx || (!dxhh && !dpath) || (!dev && !out) || N < 1)
        return fail(ctx, HANK_ERR_BAD_ARG, "%s: bad argument (N=%d; at least one of dxhh, %s must be given)", pt.jvp, N, pt.dir);
    int rc = path_entry_excluded(ctx, kind, pt.jvp);
    if (rc) return rc;
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before %s", pt.jvp);
    TanReq q{0, dxhh, nullptr, nullptr, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, false};
    q.path = kind;
    q.dpath = dpath;
    rc = enqueue_tan_raw(ctx, q, N, dev ? out : nullptr);
    if (rc || dev) return rc;
    return tan_host_tail(ctx, out, ctx->batch.dagg_cm, (size_t)ctx->c.P * N);
}
int hank_jvp_shock_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dbeta, int32_t N, double *d_dagg_out) { return jvp_path(ctx, PATH_DISCOUNT, d_dxhh, d_dbeta, N, d_dagg_out, true); }
int hank_jvp_shock(hank_ctx *ctx, const double *dxhh, const double *dbeta, int32_t N, double *dagg_out) { return jvp_path(ctx, PATH_DISCOUNT, dxhh, dbeta, N, dagg_out, false); }
int hank_jvp_income_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_dy, int32_t N, double *d_dagg_out) { return jvp_path(ctx, PATH_INCOME, d_dxhh, d_dy, N, d_dagg_out, true); }
int hank_jvp_income(hank_ctx *ctx, const double *dxhh, const double *dy, int32_t N, double *dagg_out) { return jvp_path(ctx, PATH_INCOME, dxhh, dy, N, dagg_out, false); }
int hank_jvp_borrow_dev(hank_ctx *ctx, const double *d_dxhh, const double *d_damin, int32_t N, double *d_dagg_out) { return jvp_path(ctx, PATH_BORROW, d_dxhh, d_damin, N, d_dagg_out, true); }
int hank_jvp_borrow(hank_ctx *ctx, const double *dxhh, const double *damin, int32_t N, double *dagg_out) { return jvp_path(ctx, PATH_BORROW, dxhh, damin, N, dagg_out, false); }

static int run_fused(hank_ctx *ctx, TanWork &w) {
    const int grc = ensure_dual_graphs(ctx, w);
    if (grc) return grc;
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, ctx->spans.begin(DUAL_BACK, ctx->stream));
    HIPC(ctx, hipGraphLaunch(w.g_fback, ctx->stream));
    HIPC(ctx, ctx->spans.end_begin(DUAL_BACK, ctx->c.P + 5, DUAL_FWD, ctx->stream));
    HIPC(ctx, hipGraphLaunch(w.g_ffwd, ctx->stream));
    HIPC(ctx, ctx->spans.end(DUAL_FWD, ctx->stream, ctx->c.P + 5));
    ctx->spans.invalidate({PRIMAL_BACK, PRIMAL_FWD, TAN_BACK, TAN_FWD});
    record_rewritten(ctx, true, true);
    batch_ran(ctx, 0, &w, w.N, w.dagg_cm, w.dpol);
    return HANK_OK;
}

// hank_primal_jvp[_dev] below the wide batches (those are hank_primal + hank_jvp of the same form): x and N directions from the
// caller (kind: where they live) through one Dual pass, on the persistent sweeps or the dual-sweep launches
static int enqueue_primal_jvp(hank_ctx *ctx, const double *xhh, const double *dxhh, hipMemcpyKind kind, int N, double *d_agg_out, double *d_dagg_out) {
    if (use_x_fused(ctx, N)) return x_dual(ctx, xhh, dxhh, kind, N, d_agg_out, d_dagg_out);
    TanWork *w = nullptr;
    int rc = ensure_tanwork(ctx, N, &w);
    if (rc) return rc;
    const size_t P = ctx->c.P;
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(ctx->d_xhh, xhh, sizeof(double) * ctx->c.n_hh * P, kind, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(w->dxhh, dxhh, sizeof(double) * ctx->c.n_hh * P * N, kind, ctx->stream));
    rc = run_fused(ctx, *w);
    if (rc) return rc;
    HIPC(ctx, copy_agg(ctx, d_agg_out, hipMemcpyDeviceToDevice, ctx->stream));
    HIPC(ctx, copy_dagg(ctx, d_dagg_out, w->dagg_cm, N, hipMemcpyDeviceToDevice));
    return HANK_OK;
}

int hank_primal_jvp_dev(hank_ctx *ctx, const double *d_xhh, const double *d_dxhh, int32_t N, double *d_agg_out,
                        double *d_dagg_out) {
    ENTER(ctx);
    if (!ctx || !d_xhh || !d_dxhh || N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument (N=%d)", N);
    if (!ctx->boundary_set) return fail(ctx, HANK_ERR_NOT_READY, "hank_set_boundary must be called first");
    if (use_wide(ctx, N) || path_on(ctx)) {           // a wide batch: the Float64 sweeps of the context's schedule, then the on-chip tangent sweeps; a path: both on the launches
        const int rc = hank_primal_dev(ctx, d_xhh, d_agg_out);
        return rc ? rc : hank_jvp_dev(ctx, d_dxhh, N, d_dagg_out);
    }
    note_primal_x(ctx, nullptr);      // (this entry never skips work: bench.py times it)
    ctx->stats[PRIMAL_SWEEPS]++;
    return enqueue_primal_jvp(ctx, d_xhh, d_dxhh, hipMemcpyDeviceToDevice, N, d_agg_out, d_dagg_out);
}

int hank_primal_jvp(hank_ctx *ctx, const double *xhh, const double *dxhh, int32_t N, double *agg_out, double *dagg_out) {
    ENTER(ctx);
    if (!ctx || !xhh || !dxhh || !dagg_out || N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument (N=%d)", N);
    if (!ctx->boundary_set) return fail(ctx, HANK_ERR_NOT_READY, "hank_set_boundary must be called first");
    const size_t P = ctx->c.P;
    int rc = check_rates(ctx, xhh);
    if (rc) return rc;
    // The reference calls JVP(fullFunction, x, y) about 21 times per Newton step at ONE x (NewtonRaphson.jl:91-95) and its Dual
    // pass recomputes the primal every time (GeneralStructures.jl:546-547). The linearisation of the x on record is still
    // valid when the same x comes in again: only the tangent sweeps run (what hank_jvp does), the value is the recorded one.
    if (ctx->memo_on && ctx->primal_done && ctx->memo_valid && ctx->memo_xhh.size() == (size_t)ctx->c.n_hh * P &&
        memcmp(ctx->memo_xhh.data(), xhh, sizeof(double) * ctx->c.n_hh * P) == 0) {
        ctx->stats[PRIMAL_MEMO_HITS]++;
        rc = hank_jvp(ctx, dxhh, N, dagg_out);
        if (rc) return rc;
        if (agg_out) {
            HIPC(ctx, join_side(ctx));
            HIPC(ctx, copy_agg(ctx, agg_out, hipMemcpyDeviceToHost, ctx->stream));
            HIPC(ctx, hipStreamSynchronize(ctx->stream));
        }
        return HANK_OK;
    }
    if (use_wide(ctx, N) || path_on(ctx)) {
        rc = hank_primal(ctx, xhh, agg_out);
        return rc ? rc : hank_jvp(ctx, dxhh, N, dagg_out);
    }
    note_primal_x(ctx, nullptr);
    rc = run_settled(ctx, [&] { return enqueue_primal_jvp(ctx, xhh, dxhh, hipMemcpyHostToDevice, N, nullptr, nullptr); });
    if (rc) return rc;      // (a verdict against the record has left no batch current: the partials of a primal that failed are nobody's)
    HIPC(ctx, copy_agg(ctx, agg_out, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, copy_dagg(ctx, dagg_out, ctx->batch.dagg_cm, N, hipMemcpyDeviceToHost));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    note_primal_x(ctx, xhh);
    ctx->stats[PRIMAL_SWEEPS]++;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

// the fake-news workspace for n_het outputs: allocated at the first call, grown (all of it, after the stream drains) when a
// call asks for more outputs than it holds
// Nw: the directions of the backward batch — the n_hh inputs, or the n_e income states of hank_fake_news_income; the workspace holds the
// widest and the most outputs asked for so far
static int ensure_fn(hank_ctx *ctx, int n_het, int Nw) {
    if (ctx->fn.n_het >= n_het && ctx->fn.N >= std::max(Nw, ctx->c.n_hh)) return HANK_OK;
    n_het = std::max(n_het, ctx->fn.n_het);
    Nw = std::max(std::max(Nw, ctx->fn.N), ctx->c.n_hh);      // (never below n_hh: k_fn_het_record and k_grp_fn_record write dsum [nh][n_hh] whatever the batch)
    const size_t P = ctx->c.P, G = ctx->c.G, NP = P * Nw, S = 16, nh = n_het;
    if (ctx->fn.dpT) HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->fn = {};
    auto alloc = [&]() -> int {
        HIPC(ctx, ctx->fn.dpT.alloc(G * NP)); HIPC(ctx, ctx->fn.iota.alloc(G * NP));
        HIPC(ctx, ctx->fn.E.alloc(nh * P * G)); HIPC(ctx, ctx->fn.Cp.alloc(S * nh * P * NP));
        HIPC(ctx, ctx->fn.F.alloc(nh * P * NP)); HIPC(ctx, ctx->fn.Dv.alloc(nh * NP));
        HIPC(ctx, ctx->fn.W.alloc(nh * G)); HIPC(ctx, ctx->fn.dsum.alloc(nh * Nw));
        return HANK_OK;
    };
    const int rc = alloc();
    if (rc) {
        ctx->fn = {};
        (void)hipGetLastError();
        return rc;
    }
    ctx->fn.n_het = n_het;
    ctx->fn.N = Nw;
    return HANK_OK;
}

// "Is the record stationary?" — the one check of every entry that reads the record as the steady state's linear operators
// (hank_fake_news[_het], hank_ss_jvp, hank_ss_vjp): the recorded primal is hank_primal (host-pointer form) at a constant path, and
// the policy of its first period equals the policy of its last (a constant path that is not the steady state of the boundary
// drifts; 1e-6 of the policy's scale is far above a converged value iteration's 1e-11). Synchronises the stream.
static int stationary_record(hank_ctx *ctx, const char *name) {
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before %s", name);
    if (!ctx->stationary)
        return fail(ctx, HANK_ERR_NOT_READY, "%s needs the recorded primal to be hank_primal at a CONSTANT path (the steady state; SteadyStateJacobian.jl:53-57): "
                    "the last primal was recorded at a path that varies over time, or through a device-pointer entry", name);
    const int P = ctx->c.P, G = ctx->c.G;
    hipStream_t s = ctx->stream;
    std::vector<double> p0((size_t)G), p1((size_t)G);
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(p0.data(), ctx->R.pol, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpyAsync(p1.data(), ctx->R.pol + (size_t)(P - 1) * G, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    double scale = 0.0, diff = 0.0;
    for (int k = 0; k < G; k++) { scale = std::max(scale, fabs(p1[k])); diff = std::max(diff, fabs(p0[k] - p1[k])); }
    if (!(diff <= 1e-6 * std::max(scale, 1e-300)))
        return fail(ctx, HANK_ERR_NOT_READY, "%s: the recorded primal is not stationary (policy of period 1 and of period %d differ by %.3g): "
                    "it needs hank_primal at the steady state with the steady state as both boundaries", name, P, diff);
    return HANK_OK;
}

// The household block's sequence-space Jacobian at a stationary primal from its Toeplitz structure (hank_jacobian.h):
// F (P, P, n_hh[, n_het]) and Dv (P, n_hh[, n_het]), column-major. Requires hank_primal at the constant steady-state path
// with the steady state as both boundaries (what getSteadyStateJacobian builds, SteadyStateJacobian.jl:53-57).
// n_het == 0: hank_fake_news (the policy variable's aggregate: E_0 = pol_ss, Dv weights D_ss); n_het >= 1: hank_fake_news_het
// (outputs 0 .. n_het-1 of hank_get_het_outputs; output 0 is the same arithmetic as n_het == 0, bit for bit); groups: hank_fake_news_group
// (the context's K group outputs: the same policy responses and impulses, the outputs served GRP_FN_CHUNK at a time so the expectation
// workspace never holds more — steps 3 and 4 run once per chunk, once in all for the other two entries).
// kind: the derivative with respect to a path kind's values, its directions in place of the n_hh inputs' —
// PATH_DISCOUNT (hank_fake_news_shock; with n_het >= 1): ONE direction, the backward sweep seeded with d beta_{P-1} = 1 (hank_shock.h),
// and no direct term: F (P, P, n_het), Dv (P, n_het);
// PATH_INCOME (hank_fake_news_income; with n_het = 1, 2): n_e directions, the backward sweep seeded with d y_{P-1}[e] = 1 in direction e
// (hank_income.h), and the direct term m_ss[e] of consumption at lag 0: F (P, P, n_e, n_het), Dv (P, n_e, n_het).
static int fake_news(hank_ctx *ctx, int n_het, bool groups, double *F_out, double *Dv_out, PathKind kind = PATH_NONE) {
    const bool inputs = kind == PATH_NONE;      // the directions are the n_hh inputs'
    const char *name = !inputs ? PATHS[kind].fn : groups ? "hank_fake_news_group" : n_het ? "hank_fake_news_het" : "hank_fake_news";
    { const int prc = path_refuses(ctx, name); if (prc) return prc; }
    { const int nrc = stationary_record(ctx, name); if (nrc) return nrc; }
    const Consts &c = ctx->c;
    // the input, described once: the batch width N; the direct term of its direction k in output o at lag 0 — dsum of the record kernels
    // (hd) for the inputs, the column mass m_ss[k] (hm) in consumption for y[k], none for beta; below, its seed and its backward graph
    const int P = c.P, G = c.G, N = inputs ? c.n_hh : path_width(c, kind), NP = P * N, S = 16, nout = groups ? ctx->grp.K : n_het ? n_het : 1;
    const bool direct_hd = inputs && (groups || n_het), direct_hm = kind == PATH_INCOME;
    const int cap = groups ? std::min(nout, GRP_FN_CHUNK) : nout;      // outputs per pass
    hipStream_t s = ctx->stream;
    { const int src = ensure_seg(ctx); if (src) return src; }
    { const int src = ensure_lwg(ctx); if (src) return src; }
    // 1. n_hh backward tangent sweeps (one batch) seeded at the last period: every lag of the policy response
    TanWork *wp = nullptr;
    int rc = ensure_tanwork(ctx, N, &wp);
    if (rc) return rc;
    TanWork &w = *wp;
    rc = ensure_tan_graphs(ctx, w, false, 0);
    if (!rc && !inputs) rc = ensure_path_tan_graph(ctx, w, kind);
    if (rc) return rc;
    const GraphExec &back = inputs ? w.tan_back(false) : w.seed[kind].g_tback;
    rc = ensure_fn(ctx, cap, N);
    if (rc) return rc;
    HIPC(ctx, join_side(ctx));      // D_1 and the {w, ig D} records come from the primal's forward sweep
    std::vector<double> hm(direct_hm ? N : 0);         // income: the steady state's column masses, the direct term of consumption
    switch (kind) {
    case PATH_INCOME: {      // no input moves; d y_{P-1}[e] = 1 in direction e, (n_e, P, n_e) column-major
        std::vector<double> seed((size_t)N * P * N, 0.0);
        for (int e = 0; e < N; e++) seed[(size_t)e + (size_t)N * ((size_t)(P - 1) + (size_t)P * e)] = 1.0;
        rc = ensure_inc_mass(ctx);
        if (rc) return rc;
        HIPC(ctx, hipMemsetAsync(w.dxhh, 0, sizeof(double) * c.n_hh * P * N, s));
        HIPC(ctx, hipMemcpyAsync(w.seed[kind].in, seed.data(), sizeof(double) * seed.size(), hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync(hm.data(), ctx->d_inc_m, sizeof(double) * N, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));      // (seed is this block's)
        break;
    }
    case PATH_BORROW:          // no input moves; d amin_{P-1} = 1, staged as d beta_{P-1} = 1 is
    case PATH_DISCOUNT: {      // no input moves; d beta_{P-1} = 1 (the batch is one direction wide: (P, 1) column-major is [P])
        static const double one = 1.0;
        HIPC(ctx, hipMemsetAsync(w.dxhh, 0, sizeof(double) * c.n_hh * P, s));
        HIPC(ctx, hipMemsetAsync(w.seed[kind].in, 0, sizeof(double) * P, s));
        HIPC(ctx, hipMemcpyAsync(w.seed[kind].in.get() + (P - 1), &one, sizeof(double), hipMemcpyHostToDevice, s));
        break;
    }
    case PATH_NONE: hipLaunchKernelGGL(k_fn_seed, dim3((unsigned)((N * P * N + 255) / 256)), dim3(256), 0, s, w.dxhh, N, P); break;
    }
    HIPC(ctx, hipGraphLaunch(back, s));
    batch_none(ctx);      // (w.dpol no longer belongs to a caller's batch)
    // 2. the lottery impulse of every lag and input at once
    hipLaunchKernelGGL(k_fn_transpose, dim3((unsigned)((G + 31) / 32), (unsigned)((P + 31) / 32), (unsigned)N), dim3(256), 0, s, w.dpol, P, G, N, ctx->fn.dpT);
    hipLaunchKernelGGL(k_fn_impulse, dim3((unsigned)c.n_a, (unsigned)((NP + 255) / 256)), dim3(256), 0, s, c, ctx->R, ctx->fn.dpT, NP, ctx->fn.iota);
    const size_t PG = (size_t)P * G;
    std::vector<double> hF((size_t)cap * P * NP), hD((size_t)cap * NP), hd((size_t)cap * N, 0.0);
    auto direct = [&](int o, int k) -> const double * {      // the direct term of direction k in output o of a pass, or none
        if (direct_hm) return o == 1 ? &hm[k] : nullptr;      // (y_t[e]'s is m_ss[e], in consumption; beta has none in any output)
        return direct_hd && (groups || o > 0) ? &hd[(size_t)k + (size_t)N * o] : nullptr;
    };
    for (int o0 = 0; o0 < nout; o0 += cap) {
        const int nh = std::min(cap, nout - o0);
        const int kchunk = ((G + S - 1) / S + 15) / 16 * 16, MP = nh * P;
        // 3. the expectation vectors E^o_u = (T')^u f_o,ss of every output (rows o*P + u of E) and the direct term's weights
        const double *Wd = ctx->R.Dseq + G;
        if (groups || n_het) {
            if (groups)
                hipLaunchKernelGGL(k_grp_fn_record, dim3((unsigned)nh), dim3(256), 0, s, c, ctx->R, ctx->d_xhh, o0, ctx->grp.W, ctx->grp.base, PG, ctx->fn.E, ctx->fn.W, ctx->fn.dsum);
            else
                hipLaunchKernelGGL(k_fn_het_record, dim3((unsigned)nh), dim3(256), 0, s, c, ctx->R, ctx->d_xhh, PG, ctx->fn.E, ctx->fn.W, ctx->fn.dsum);
            for (int u = 0; u + 1 < P; u++)
                hipLaunchKernelGGL(k_fn_expect_het, dim3((unsigned)((G + 255) / 256), (unsigned)nh), dim3(256), 0, s, c, ctx->R, ctx->fn.E, PG, u);
            Wd = ctx->fn.W;
        } else {
            HIPC(ctx, hipMemcpyAsync(ctx->fn.E, ctx->R.pol, sizeof(double) * G, hipMemcpyDeviceToDevice, s));
            for (int u = 0; u + 1 < P; u++)
                hipLaunchKernelGGL(k_fn_expect, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, c, ctx->R, ctx->fn.E + (size_t)u * G, ctx->fn.E + (size_t)(u + 1) * G);
        }
        // 4. F = E iota, Dv = W dpT (the K split depends on G only: every output's elements are summed in the same order)
        hipLaunchKernelGGL(k_fn_gemm, dim3((unsigned)((NP + 63) / 64), (unsigned)((MP + 63) / 64), (unsigned)S), dim3(256), 0, s, ctx->fn.E, ctx->fn.iota, ctx->fn.Cp, MP, NP, G, kchunk);
        hipLaunchKernelGGL(k_fn_reduce, dim3((unsigned)(((size_t)MP * NP + 255) / 256)), dim3(256), 0, s, ctx->fn.Cp, MP * NP, S, ctx->fn.F);
        hipLaunchKernelGGL(k_fn_gemm, dim3((unsigned)((NP + 63) / 64), (unsigned)((nh + 63) / 64), (unsigned)S), dim3(256), 0, s, Wd, ctx->fn.dpT, ctx->fn.Cp, nh, NP, G, kchunk);
        hipLaunchKernelGGL(k_fn_reduce, dim3((unsigned)((nh * NP + 255) / 256)), dim3(256), 0, s, ctx->fn.Cp, nh * NP, S, ctx->fn.Dv);
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(hF.data(), ctx->fn.F, sizeof(double) * MP * NP, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipMemcpyAsync(hD.data(), ctx->fn.Dv, sizeof(double) * nh * NP, hipMemcpyDeviceToHost, s));
        if (direct_hd) HIPC(ctx, hipMemcpyAsync(hd.data(), ctx->fn.dsum, sizeof(double) * nh * N, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));
        if (o0 == 0) {
            rc = device_verdict(ctx, THE_RECORD);
            if (rc) return rc;
        }
        // column n' = t*N + k of the device arrays is lag j = P-1-t of input k; the same-period effect d_{o,k} lands at lag 0
        // (output 0 of the het outputs has none; a group's is zero unless its base is consumption)
        for (int o = 0; o < nh; o++)
            for (int k = 0; k < N; k++) {
                const double *dk = direct(o, k);
                for (int t = 0; t < P; t++) {
                    const int j = P - 1 - t;
                    const size_t ko = (size_t)k + (size_t)N * (o0 + o);
                    const double dv = hD[(size_t)o * NP + (size_t)t * N + k];
                    Dv_out[j + (size_t)P * ko] = dk && j == 0 ? dv + *dk : dv;
                    for (int u = 0; u < P; u++) F_out[u + (size_t)P * (j + (size_t)P * ko)] = hF[((size_t)o * P + u) * NP + (size_t)t * N + k];
                }
            }
    }
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

int hank_fake_news(hank_ctx *ctx, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    return fake_news(ctx, 0, false, F_out, Dv_out);
}

// every heterogeneous output at once (hank_jacobian.h): F (P, P, n_hh, n_het), Dv (P, n_hh, n_het). Independent of the
// hank_set_het_outputs declaration, which it leaves as it is.
int hank_fake_news_het(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    const int rc = het_count_ok(ctx, "hank_fake_news_het", n_het, false);
    return rc ? rc : fake_news(ctx, n_het, false, F_out, Dv_out);
}

// (KrusellSmith.jl:59-62, BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 with the input fixed to beta)
int hank_fake_news_shock(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    const int rc = het_count_ok(ctx, "hank_fake_news_shock", n_het, false);
    return rc ? rc : fake_news(ctx, n_het, false, F_out, Dv_out, PATH_DISCOUNT);
}

// (KrusellSmith.jl:59-62, :66-80, BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 with the input fixed to y[e])
int hank_fake_news_income(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    const int rc = het_count_ok(ctx, "hank_fake_news_income", n_het, false, n_het <= 2);
    return rc ? rc : fake_news(ctx, n_het, false, F_out, Dv_out, PATH_INCOME);
}

// (KrusellSmith.jl:52, :76, BackwardIteration.jl:90-113; the recursion of SteadyStateJacobian.jl:363-371 with the input fixed to the limit)
int hank_fake_news_borrow(hank_ctx *ctx, int32_t n_het, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    const int rc = het_count_ok(ctx, "hank_fake_news_borrow", n_het, false);
    return rc ? rc : fake_news(ctx, n_het, false, F_out, Dv_out, PATH_BORROW);
}

#ifdef HANK_XSTAMP
int hank_debug_wstamps(hank_ctx *ctx, unsigned long long *out) {
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    HIPC(ctx, hipMemcpyFromSymbol(out, HIP_SYMBOL(hank::g_wstamps), sizeof(unsigned long long) * 2 * 4 * 64));
    return HANK_OK;
}
// dev build: the stamps of the last sweeps (see hank_xsweep.h)
int hank_debug_stamps(hank_ctx *ctx, unsigned long long *out) {
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    HIPC(ctx, hipMemcpyFromSymbol(out, HIP_SYMBOL(hank::g_xstamps), sizeof(unsigned long long) * 2 * 32 * XSTAMP_NP * XSTAMP_NS));
    HIPC(ctx, hipMemcpyFromSymbol(out + 2 * 32 * XSTAMP_NP * XSTAMP_NS, HIP_SYMBOL(hank::g_xwaves), sizeof(unsigned long long) * 2 * 32 * XSTAMP_NP * 16));
    return HANK_OK;
}
#endif

int hank_stats(hank_ctx *ctx, int64_t out[8]) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    for (int k = 0; k < N_STATS; k++) out[k] = k == SCHEDULE ? ctx->schedule : ctx->stats[k];
    return HANK_OK;
}

int hank_sweep_instance(hank_ctx *ctx, int32_t out[4]) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    for (int k = 0; k < 4; k++) out[k] = ctx->xw.inst[k];
    return HANK_OK;
}

int hank_gather_columns(hank_ctx *const *ctxs, int32_t n, const double *const *d_blocks, const int32_t *N_k, double *d_out) {
    if (!ctxs || n < 1 || !ctxs[0]) return HANK_ERR_BAD_ARG;
    hank_ctx *c0 = ctxs[0];
    if (!d_blocks || !N_k || !d_out) return fail(c0, HANK_ERR_BAD_ARG, "hank_gather_columns: null pointer");
    const size_t P = c0->c.P;
    size_t col = 0;
    for (int k = 0; k < n; k++) {
        hank_ctx *ck = ctxs[k];
        if (!ck || ck->c.P != c0->c.P || N_k[k] < 0 || (N_k[k] > 0 && !d_blocks[k])) return fail(c0, HANK_ERR_BAD_ARG, "hank_gather_columns: bad block %d", k);
        const size_t bytes = sizeof(double) * P * (size_t)N_k[k];
        double *dst = d_out + P * col;
        col += (size_t)N_k[k];
        if (bytes == 0) continue;
        ENTER(ck);                          // the copy is enqueued on the SOURCE context's stream, behind the sweeps that write the block
        if (ck->device == c0->device) {
            HIPC(c0, hipMemcpyAsync(dst, d_blocks[k], bytes, hipMemcpyDeviceToDevice, ck->stream));
        } else {
            const hipError_t pe = hipDeviceEnablePeerAccess(c0->device, 0);      // (from the source device: it writes into device 0's memory over xGMI)
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return fail(c0, HANK_ERR_NO_DEVICE, "no peer access from device %d to device %d (%s)", ck->device, c0->device, hipGetErrorString(pe)); }
            (void)hipGetLastError();
            HIPC(c0, hipMemcpyPeerAsync(dst, c0->device, d_blocks[k], ck->device, bytes, ck->stream));
        }
        if (ck != c0 && ck->stream != c0->stream) {
            HIPC(c0, hipEventRecord(ck->ev_stream, ck->stream));
            HIPC(c0, hipStreamWaitEvent(c0->stream, ck->ev_stream, 0));
        }
    }
    c0->errmsg[0] = 0;
    return HANK_OK;
}

int hank_info(hank_ctx *ctx, int64_t out[8]) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    out[0] = ctx->batch.family; out[1] = ctx->wide_mode; out[2] = ctx->wide_min; out[3] = w_supported(ctx) ? 1 : 0;
    out[4] = ctx->xjvp_max; out[5] = ctx->c.diet; out[6] = (int64_t)ctx->rec_bytes; out[7] = ctx->lwg_builds;
    return HANK_OK;
}

int hank_last_timings(hank_ctx *ctx, double *out_ms, int32_t *launches) {      // (six slots each: PRIMAL_BACK .. DUAL_FWD)
    if (!ctx || !out_ms) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = PRIMAL_BACK; k <= DUAL_FWD; k++) HIPC(ctx, ctx->spans.read((Span)k, &out_ms[k], launches ? &launches[k] : nullptr));
    return HANK_OK;
}

int hank_get_policy_seq(hank_ctx *ctx, double *out) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(out, ctx->R.pol, sizeof(double) * (size_t)ctx->c.P * ctx->c.G, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

int hank_get_lottery_record(hank_ctx *ctx, int32_t *lo, double *lw, double *ig, void *lq, double *iga) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
    if ((lq || iga) && !ctx->rec_lq) return fail(ctx, HANK_ERR_BAD_ARG, "hank_get_lottery_record: this build keeps no packed lottery record");
    HIPC(ctx, join_side(ctx));
    if (lo || lw || ig) { const int rc = ensure_lottery(ctx); if (rc) return rc; }
    const size_t n = (size_t)ctx->c.P * ctx->c.G;
    if (lo) HIPC(ctx, hipMemcpyAsync(lo, ctx->R.lo, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (lw) HIPC(ctx, hipMemcpyAsync(lw, ctx->R.lw, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (ig) HIPC(ctx, hipMemcpyAsync(ig, ctx->R.ig, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (lq) HIPC(ctx, hipMemcpyAsync(lq, ctx->rec_lq, sizeof(int4) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (iga) HIPC(ctx, hipMemcpyAsync(iga, ctx->rec_iga, sizeof(double) * (size_t)ctx->c.n_a, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

// the forward sweeps' work units of the recorded lottery as the persistent sweeps read them (tests): src [P][Sact], units
// [P][Sact][XUCAP][2]; the slots of a member behind its count (src >> 18) hold nothing
int hank_get_forward_units(hank_ctx *ctx, int32_t *src, int32_t *units) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    const XWork &X = ctx->xw;
    if (!ctx->primal_done || !X.ready || !X.rng_valid) return fail(ctx, HANK_ERR_NOT_READY, "hank_get_forward_units: no persistent sweep has cut the recorded lottery into work units");
    HIPC(ctx, join_side(ctx));
    const size_t n = (size_t)ctx->c.P * X.Sact;
    if (src) HIPC(ctx, hipMemcpyAsync(src, X.srcF, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (units) HIPC(ctx, hipMemcpyAsync(units, X.unitsF, sizeof(int2) * n * XUCAP, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

int hank_get_dist_seq(hank_ctx *ctx, double *out) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(out, ctx->R.Dseq + ctx->c.G, sizeof(double) * (size_t)ctx->c.P * ctx->c.G, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

// The grid-weighted aggregate AD_t = sum_pt a(pt) D_t(pt) of the last primal sweep and its N tangents dAD_t = sum a dD_t of the
// last tangent sweep (whichever family ran it): every forward kernel reduces it next to the policy-weighted one. dev != 0:
// the outputs are device pointers (copies ordered on the context's stream).
static int grid_aggregates(hank_ctx *ctx, double *agg2_out, int32_t N, double *dagg2_out, bool dev) {
    if (!ctx || (!agg2_out && !dagg2_out) || N < 0) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (agg2_out) {
        if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
        HIPC(ctx, join_side(ctx));
        HIPC(ctx, copy_agg(ctx, agg2_out, kind, ctx->stream, 1));
    }
    if (dagg2_out && N > 0) {
        const TanBatch *b = nullptr;
        const int rc = batch_current(ctx, N, &b);
        if (rc) return rc;
        HIPC(ctx, copy_dagg(ctx, dagg2_out, b->dagg_cm, N, kind, 1));
    }
    if (!dev) HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}
int hank_get_grid_aggregates(hank_ctx *ctx, double *agg2_out, int32_t N, double *dagg2_out) { return grid_aggregates(ctx, agg2_out, N, dagg2_out, false); }
int hank_get_grid_aggregates_dev(hank_ctx *ctx, double *d_agg2_out, int32_t N, double *d_dagg2_out) { return grid_aggregates(ctx, d_agg2_out, N, d_dagg2_out, true); }

int hank_get_dpolicy_seq(hank_ctx *ctx, int32_t N, double *out) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    const TanBatch *b = nullptr;
    int rc = batch_current(ctx, N, &b);
    if (rc) return rc;
    const size_t total = (size_t)ctx->c.P * ctx->c.G * N;
    DevBuf<double> tmp;      // (released on every way out: hipFree waits for the work that uses it)
    HIPC(ctx, tmp.alloc(total));
    rc = export_dpol_dev(ctx, *b, tmp);
    if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(out, tmp, sizeof(double) * total, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

}  // extern "C"

// ================================ transposed sweeps: hank_vjp (hank_adjoint.h) ==========================
// Lane geometry per batch width M: adj_geom (hank_geom.h).
static int build_cotwork(hank_ctx *ctx, CotWork &w) {
    const Consts &c = ctx->c;
    const size_t P = c.P, G = c.G, M = (size_t)w.N;
    w.V = adj_lane_width(w.N);
    w.g = adj_geom(c.n_a, w.N);
    const AdjGeom &g = w.g;
    HIPC(ctx, w.ybar.alloc(het_max(ctx) * P * M));
    HIPC(ctx, w.yb0.alloc(P * M));
    HIPC(ctx, w.yb1.alloc(P * M));
    HIPC(ctx, w.ybx.alloc(hx_count(ctx) * P * M));      // (the NX > 0 graphs hold its address)
    for (int k = 0; k < 2; k++) HIPC(ctx, w.st[k].alloc(G * M));
    HIPC(ctx, w.pbar.alloc(P * G * M));
    HIPC(ctx, w.partS.alloc(P * (size_t)g.nb * 3 * M));
    HIPC(ctx, w.partM.alloc(P * (size_t)g.nb * 3 * M));
    HIPC(ctx, w.xbar.alloc((size_t)c.n_hh * P * M));
    return HANK_OK;
}
static size_t adj_lds_dist(const Consts &c, const AdjGeom &g, int V) { return sizeof(double) * ((size_t)c.n_e * (g.R + 2) * g.NC * V + (size_t)c.n_e * c.n_e); }
// k_adj_dist_grp: k_adj_dist's tile and Pi, then the K groups' cotangents of the block's columns
static size_t adj_lds_dist_grp(const Consts &c, const AdjGeom &g, int V, int K) { return sizeof(double) * (adj_grp_lds_off(c.n_e, g, V) + (size_t)K * g.NC * V); }
static size_t adj_lds_egm(const Consts &c, const AdjGeom &g, int V) {
    return sizeof(double) * ((size_t)c.n_e * g.R * g.NC * V + (((size_t)c.n_e * c.n_e + 1) & ~(size_t)1) + (size_t)c.n_e * 6 * g.NC * V);
}

// Sweep A's graph of a width with NX extra outputs (P launches, t = P-1 .. 0): hx = the record and cotangents of those outputs
template <typename VT, int NX>
static int capture_cot_graph_a(hank_ctx *ctx, CotWork &w, AdjHx<VT, NX> hx, GraphExec *out) {
    const Consts &c = ctx->c;
    const int P = c.P;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e), grd((unsigned)w.g.nb, (unsigned)((w.g.MV + w.g.NC - 1) / w.g.NC));
    const size_t ldsA = adj_lds_dist(c, w.g, w.V);
    VT *st[2] = {reinterpret_cast<VT *>(w.st[0].get()), reinterpret_cast<VT *>(w.st[1].get())};
    VT *pbar = reinterpret_cast<VT *>(w.pbar.get());
    const VT *yb0 = reinterpret_cast<const VT *>(w.yb0.get()), *yb1 = reinterpret_cast<const VT *>(w.yb1.get());
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int cur = 0;
    for (int t = P - 1; t >= 0; t--) {
        hipLaunchKernelGGL((k_adj_dist<VT, NX>), grd, blk, ldsA, s, c, ctx->R, ctx->d_xhh, w.g, t, t == P - 1 ? 1 : 0, yb0, yb1, st[cur], st[cur ^ 1], pbar, hx);
        cur ^= 1;
    }
    return end_capture(ctx, out);
}
template <typename VT, int NX>
static int capture_cot_graph_ax(hank_ctx *ctx, CotWork &w) {
    const AdjHx<VT, NX> hx{ctx->hx.f.get(), ctx->hx.fc.get(), reinterpret_cast<const VT *>(w.ybx.get())};
    return capture_cot_graph_a<VT, NX>(ctx, w, hx, &w.g_AX[NX - 1]);
}

// Sweep A's graph of a width with the context's groups (k_adj_dist_grp): it holds K, the bases and the addresses of W and w.gb
template <typename VT>
static int capture_cot_graph_ag(hank_ctx *ctx, CotWork &w) {
    const Consts &c = ctx->c;
    const GroupSet &gs = ctx->grp;
    const int P = c.P;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e), grd((unsigned)w.g.nb, (unsigned)((w.g.MV + w.g.NC - 1) / w.g.NC));
    const size_t ldsA = adj_lds_dist_grp(c, w.g, w.V, gs.K);
    VT *st[2] = {reinterpret_cast<VT *>(w.st[0].get()), reinterpret_cast<VT *>(w.st[1].get())};
    VT *pbar = reinterpret_cast<VT *>(w.pbar.get());
    const VT *yb0 = reinterpret_cast<const VT *>(w.yb0.get()), *yb1 = reinterpret_cast<const VT *>(w.yb1.get());
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int cur = 0;
    for (int t = P - 1; t >= 0; t--) {
        hipLaunchKernelGGL((k_adj_dist_grp<VT>), grd, blk, ldsA, s, c, ctx->R, ctx->d_xhh, w.g, t, t == P - 1 ? 1 : 0, yb0, yb1, st[cur], st[cur ^ 1], pbar, gs.K, gs.codes,
                           gs.W.get(), reinterpret_cast<const VT *>(w.gb.get()));
        cur ^= 1;
    }
    return end_capture(ctx, &w.g_AG);
}

// the two graphs of a width, captured the first time hank_vjp runs at it: Sweep A (NX = 0) and Sweep B (P launches,
// t = 0 .. P-1, then the fixed-order reduction of the inputs' cotangents)
// kind: Sweep B with a path kind's cotangent — beta_bar_t (hank_vjp_shock; hank_shock.h: k_shk_bbar), y_bar_t (hank_vjp_income; hank_income.h:
// k_inc_ybar) — as partials behind every period's launch, while that period's mu_t is in the state the launch read, then their reduction
// and the caller's layout — the same launches of k_adj_egm and k_adj_out, P + 2 more, into w.path[kind].g_B. For y_bar the column masses
// (ensure_inc_mass) are current before the graph is launched.
static int shk_mc(int M) { int mc = 1; while (mc < M && mc < 64) mc <<= 1; return mc; }      // cotangent columns across k_shk_bbar's lanes
template <typename VT>
static int capture_cot_graph_b(hank_ctx *ctx, CotWork &w, PathKind kind) {
    const Consts &c = ctx->c;
    const int P = c.P, M = w.N, MC = shk_mc(M), IMC = std::min(MC, INC_MC);
    hipStream_t s = ctx->own_stream;
    const dim3 blk(64 * c.n_e), grd((unsigned)w.g.nb, (unsigned)((w.g.MV + w.g.NC - 1) / w.g.NC));
    const size_t ldsB = adj_lds_egm(c, w.g, w.V);
    VT *st[2] = {reinterpret_cast<VT *>(w.st[0].get()), reinterpret_cast<VT *>(w.st[1].get())};
    VT *pbar = reinterpret_cast<VT *>(w.pbar.get());
    PathCot &pc = w.path[kind];
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int cur = 0;
    for (int t = 0; t < P; t++) {
        hipLaunchKernelGGL((k_adj_egm<VT>), grd, blk, ldsB, s, c, ctx->R, w.g, t, t == 0 ? 1 : 0, t == P - 1 ? 1 : 0, ctx->d_adj_sb, st[cur], st[cur ^ 1], pbar,
                           reinterpret_cast<VT *>(w.partS.get()), reinterpret_cast<VT *>(w.partM.get()));
        if (kind == PATH_DISCOUNT)
            hipLaunchKernelGGL(k_shk_bbar, dim3((unsigned)w.g.nb, (unsigned)((M + MC - 1) / MC)), dim3(SHK_BT), 0, s, c, ctx->R, ctx->d_xhh.get(), ctx->exo[PATH_DISCOUNT].d.get(), w.g.R, MC, t,
                               t == 0 ? 1 : 0, ctx->d_adj_sb.get(), w.st[cur].get(), w.pbar.get(), M, pc.part.get() + (size_t)t * w.g.nb * M);
        if (kind == PATH_INCOME)
            hipLaunchKernelGGL(k_inc_ybar, dim3((unsigned)w.g.nb, (unsigned)((M + IMC - 1) / IMC)), dim3(INC_BT), inc_ybar_lds(c, w.g.R, IMC), s, c, ctx->R, ctx->d_xhh.get(),
                               w.g.R, IMC, t, t == 0 ? 1 : 0, ctx->d_adj_sb.get(), w.st[cur].get(), w.pbar.get(), M, pc.part.get() + (size_t)t * w.g.nb * c.n_e * M);
        if (kind == PATH_BORROW)
            hipLaunchKernelGGL(k_brw_abar, dim3((unsigned)w.g.nb, (unsigned)((M + MC - 1) / MC)), dim3(BRW_BT), 0, s, c, ctx->R, ctx->exo[PATH_BORROW].d.get(), w.g.R, MC, t,
                               t == 0 ? 1 : 0, w.st[cur].get(), w.pbar.get(), M, pc.part.get() + (size_t)t * w.g.nb * M);
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_adj_out, dim3((unsigned)((P * w.N + 255) / 256)), dim3(256), 0, s, P, c.n_hh, w.N, w.g.nb, ctx->d_xhh, w.partS, w.partM, w.yb1,
                       ctx->d_agg + P, ctx->d_zd, w.xbar);
    const int W = path_width(c, kind) * M;
    if (kind != PATH_NONE)
        hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)P, (unsigned)((W + 63) / 64)), dim3(256), 0, s, pc.part.get(), w.g.nb, W, pc.rm.get());
    if (kind == PATH_INCOME)
        hipLaunchKernelGGL(k_inc_ybar_out, dim3((unsigned)(((size_t)P * c.n_e * M + 255) / 256)), dim3(256), 0, s, P, c.n_e, M, pc.rm.get(),
                           ctx->d_inc_m.get(), w.yb1.get(), pc.cm.get());
    if (kind == PATH_DISCOUNT || kind == PATH_BORROW)      // [P][M] -> (P, M) column-major
        hipLaunchKernelGGL(k_tan_out, dim3((unsigned)((P * M + 255) / 256)), dim3(256), 0, s, pc.rm.get(), P, M, pc.cm.get());
    return end_capture(ctx, &pc.g_B);
}
template <typename VT>
static int capture_cot_graphs(hank_ctx *ctx, CotWork &w) {
    const int rc = capture_cot_graph_a<VT, 0>(ctx, w, AdjHx<VT, 0>{}, &w.g_A);
    return rc ? rc : capture_cot_graph_b<VT>(ctx, w, PATH_NONE);
}

// Sweep B's segment starts belong to the record (like seg_valid): built before the first hank_vjp at a record, by whichever family wrote it
static int ensure_adj_seg(hank_ctx *ctx) {
    const Consts &c = ctx->c;
    if (ctx->adj_seg_valid) return HANK_OK;
    { const int rc = ensure_lottery(ctx); if (rc) return rc; }
    hipLaunchKernelGGL(k_adj_seg, dim3((unsigned)(c.P * c.n_e)), dim3(256), sizeof(int) * ((size_t)c.n_a + 1), ctx->stream, c, ctx->R, c.P * c.n_e, ctx->d_adj_sb);
    HIPC(ctx, hipGetLastError());
    ctx->adj_seg_valid = true;
    return HANK_OK;
}

// the extra outputs' share belongs to the record in the same way: built before the first reader at a record (hx_outputs,
// enqueue_vjp: after join_side, the sums read D_t), whichever product asks first. The only launch of k_hx_record.
static int ensure_hx_record(hank_ctx *ctx) {
    const Consts &c = ctx->c;
    HxRecord &h = ctx->hx;
    if (h.valid) return HANK_OK;
    { const int rc = ensure_lottery(ctx); if (rc) return rc; }
    const size_t P = c.P, SX = hx_count(ctx);
    if (!h.S) {
        HIPC(ctx, h.f.alloc(SX * P * c.G));
        HIPC(ctx, h.fc.alloc(SX * P * c.G));
        HIPC(ctx, h.S.alloc(P * SX * HX_NS));
    }
    hipLaunchKernelGGL(k_hx_record, dim3((unsigned)P, (unsigned)SX), dim3(256), 0, ctx->stream, c, ctx->R, ctx->d_xhh, (int)SX, h.f.get(), h.fc.get(), h.S.get());
    HIPC(ctx, hipGetLastError());
    h.valid = true;
    return HANK_OK;
}

// hank_vjp[_dev], hank_vjp_het[_dev]: M cotangent columns from the caller (kind: where they live) through the transposed sweeps
// at the recorded primal, whichever family recorded it. Touches neither the record nor the tangent batch nor the primal memo.
// n_het > 2: Sweep A's graph with NX = n_het - 2 extra outputs, and their direct terms after Sweep B.
// One request to them, as TanReq is one to the tangent sweeps: an entry names the options it sets.
struct CotReq {
    int n_het;                        // the outputs agg_bar covers (the entry's rule has checked the count)
    const double *agg_bar;            // (P, n_het, M) column-major, where `kind` says; null (hank_vjp_group with n_het = 0): no cotangent on outputs 0 and 1
    hipMemcpyKind kind;
    int M;
    double *d_xhh_bar;                // a device pointer for the inputs' cotangents, or null: the entry copies them from the workspace
    // hank_vjp_boundary (device pointers, (G, M) column-major, either may be null): the cotangents of the terminal value and of the initial
    // distribution, exported from the sweeps' states (hank_boundary.h) — everything else is the same work
    double *d_vend_bar = nullptr, *d_D0_bar = nullptr;
    // hank_vjp_group ((P, K, M) column-major, where `kind` says): cotangents on the context's group outputs — Sweep A's graph with the
    // groups, and their direct terms after Sweep B
    const double *grp_bar = nullptr;
    PathKind path = PATH_NONE;        // hank_vjp_shock, hank_vjp_income: Sweep B from the kind's graph, which reduces the path's cotangent
    double *d_path_bar = nullptr;     // a device pointer for it — beta_bar (P, M), y_bar (n_e, P, M), column-major — or null: the entry copies it from the workspace
};
static int enqueue_vjp(hank_ctx *ctx, const CotReq &q, CotWork **out) {
    const Consts &c = ctx->c;
    const size_t P = c.P;
    const int n_het = q.n_het, M = q.M;
    const double *agg_bar = q.agg_bar, *grp_bar = q.grp_bar;
    double *d_vend_bar = q.d_vend_bar, *d_D0_bar = q.d_D0_bar;
    const hipMemcpyKind kind = q.kind;
    const int NX = n_het > 2 ? n_het - 2 : 0, K = grp_bar ? ctx->grp.K : 0;
    CotWork *w = nullptr;
    int rc = tan_cache_get(ctx, ctx->cws, M, [ctx](CotWork &cw) { return build_cotwork(ctx, cw); }, &w);
    if (rc) return rc;
    if (adj_lds_dist(c, w->g, w->V) > ctx->lds_max || adj_lds_egm(c, w->g, w->V) > ctx->lds_max)
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp: n_e=%d needs more LDS per workgroup than the device has", c.n_e);
    if (K > 0 && adj_lds_dist_grp(c, w->g, w->V, K) > ctx->lds_max)
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: n_e=%d with K=%d groups needs more LDS per workgroup than the device has", c.n_e, K);
    if (K > 0 && !w->gb) {
        HIPC(ctx, w->gin.alloc(P * GRP_MAX * M));
        HIPC(ctx, w->gb.alloc(P * GRP_MAX * M));      // (the group graph holds its address)
    }
    if (!w->g_A) {
        if (!ctx->d_adj_sb) HIPC(ctx, ctx->d_adj_sb.alloc(P * c.n_e * ((size_t)c.n_a + 1)));      // (the graphs hold its address)
        rc = w->V == 2 ? capture_cot_graphs<double2>(ctx, *w) : capture_cot_graphs<double>(ctx, *w);
        if (rc) return rc;
    }
    if (q.path == PATH_INCOME && inc_ybar_lds(c, w->g.R, std::min(shk_mc(M), INC_MC)) > ctx->lds_max)
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_income: n_e=%d needs more LDS per workgroup than the device has", c.n_e);
    PathCot &pc = w->path[q.path];      // ([PATH_NONE]: the plain Sweep B, captured above)
    const size_t PWM = P * path_width(c, q.path) * M;
    if (!pc.g_B) {
        if (!pc.cm) {
            HIPC(ctx, pc.part.alloc(PWM * w->g.nb));
            HIPC(ctx, pc.rm.alloc(PWM));
            HIPC(ctx, pc.cm.alloc(PWM));      // (last: a failed allocation is tried again by the next call)
        }
        rc = w->V == 2 ? capture_cot_graph_b<double2>(ctx, *w, q.path) : capture_cot_graph_b<double>(ctx, *w, q.path);
        if (rc) return rc;
    }
    hipStream_t s = ctx->stream;
    if (agg_bar) HIPC(ctx, hipMemcpyAsync(w->ybar, agg_bar, sizeof(double) * P * n_het * M, kind, s));
    if (K > 0) HIPC(ctx, hipMemcpyAsync(w->gin, grp_bar, sizeof(double) * P * K * M, kind, s));
    HIPC(ctx, join_side(ctx));      // D_t, the lottery and the grid aggregates come from the primal's forward sweep
    rc = ensure_adj_seg(ctx);
    if (!rc && q.path == PATH_INCOME) rc = ensure_inc_mass(ctx);
    if (rc) return rc;
    if (K > 0) {
        rc = ensure_grp_record(ctx);      // (before the capture, as below; the CONS sums read D_t)
        if (rc) return rc;
        if (!w->g_AG) {
            rc = w->V == 2 ? capture_cot_graph_ag<double2>(ctx, *w) : capture_cot_graph_ag<double>(ctx, *w);
            if (rc) return rc;
        }
    }
    if (NX > 0) {
        rc = ensure_hx_record(ctx);      // (before the capture: the graph holds the record's addresses)
        if (rc) return rc;
        if (!w->g_AX[NX - 1]) {
            if (NX == 1) rc = w->V == 2 ? capture_cot_graph_ax<double2, 1>(ctx, *w) : capture_cot_graph_ax<double, 1>(ctx, *w);
            else rc = w->V == 2 ? capture_cot_graph_ax<double2, 2>(ctx, *w) : capture_cot_graph_ax<double, 2>(ctx, *w);
            if (rc) return rc;
        }
    }
    if (agg_bar) hipLaunchKernelGGL(k_adj_in, dim3((unsigned)((P * M + 255) / 256)), dim3(256), 0, s, w->ybar, (int)P, n_het, M, w->yb0, w->yb1);
    else {
        HIPC(ctx, hipMemsetAsync(w->yb0, 0, sizeof(double) * P * M, s));
        HIPC(ctx, hipMemsetAsync(w->yb1, 0, sizeof(double) * P * M, s));
    }
    if (K > 0) hipLaunchKernelGGL(k_adj_in_grp, dim3((unsigned)((P * K * M + 255) / 256)), dim3(256), 0, s, w->gin.get(), (int)P, K, M, w->gb.get());
    if (NX > 0) hipLaunchKernelGGL(k_adj_in_hx, dim3((unsigned)((P * NX * M + 255) / 256)), dim3(256), 0, s, w->ybar, (int)P, n_het, M, w->ybx.get());
    HIPC(ctx, ctx->spans.begin(VJP_A, s));
    HIPC(ctx, hipGraphLaunch(K > 0 ? w->g_AG : (NX > 0 ? w->g_AX[NX - 1] : w->g_A), s));
    HIPC(ctx, ctx->spans.end_begin(VJP_A, (int)P, VJP_B, s));
    const dim3 tblk(BND_T, 8), tgrd((unsigned)((c.n_a + BND_T - 1) / BND_T), (unsigned)((M + BND_T - 1) / BND_T), (unsigned)c.n_e);      // the layout kernel
    // Sweep A's state after its last launch (t = 0) is the cotangent of D_0; Sweep B's first launches overwrite it
    if (d_D0_bar) hipLaunchKernelGGL(k_bnd_out, tgrd, tblk, 0, s, w->st[P & 1].get(), c.n_a, c.n_e, M, d_D0_bar);
    HIPC(ctx, hipGraphLaunch(pc.g_B, s));
    if (d_vend_bar) {      // Sweep B's last launch (t = P-1) read mu_{P-1} from st[(P-1) & 1] and wrote no state: mu_P goes where it would have
        hipLaunchKernelGGL(k_bnd_vend, dim3((unsigned)(((size_t)c.n_a * M + 255) / 256)), dim3(256), 0, s, c, ctx->R, (int)P - 1, P == 1 ? 1 : 0, ctx->d_adj_sb.get(),
                           w->st[(P - 1) & 1].get(), w->pbar.get(), (size_t)M, w->st[P & 1].get());
        hipLaunchKernelGGL(k_bnd_out, tgrd, tblk, 0, s, w->st[P & 1].get(), c.n_a, c.n_e, M, d_vend_bar);
    }
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, ctx->spans.end(VJP_B, s, (int)P + 1 + (d_D0_bar ? 1 : 0) + (d_vend_bar ? 2 : 0) + (q.path != PATH_NONE ? (int)P + 2 : 0)));
    if (q.d_path_bar) HIPC(ctx, hipMemcpyAsync(q.d_path_bar, pc.cm, sizeof(double) * PWM, hipMemcpyDeviceToDevice, s));
    if (NX > 0) {
        hipLaunchKernelGGL(k_adj_hx_out, dim3((unsigned)((P * M + 255) / 256)), dim3(256), 0, s, (int)P, c.n_hh, M, NX, hx_count(ctx), w->ybx.get(),
                           ctx->hx.S.get(), w->xbar.get());
        HIPC(ctx, hipGetLastError());
    }
    if (K > 0) {
        hipLaunchKernelGGL(k_adj_grp_out, dim3((unsigned)((P * M + 255) / 256)), dim3(256), 0, s, (int)P, c.n_hh, M, K, w->gb.get(), ctx->grp.S.get(), w->xbar.get());
        HIPC(ctx, hipGetLastError());
    }
    cot_ran(ctx, w, M, w->pbar);
    if (q.d_xhh_bar) HIPC(ctx, hipMemcpyAsync(q.d_xhh_bar, w->xbar, sizeof(double) * c.n_hh * P * M, hipMemcpyDeviceToDevice, s));
    *out = w;
    return HANK_OK;
}
static int vjp_args(hank_ctx *ctx, int n_het, const void *in, int M, const void *out) {
    if (!ctx || !in || !out || M < 1) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp: bad argument (M=%d)", M);
    if (n_het > 2 && n_het <= het_max(ctx))
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp: n_het=%d reaches Value / UCE, which are not affine in the policy: their cotangents are not implemented (n_het must be 1 or 2)", n_het);
    if (n_het < 1 || n_het > 2) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp: n_het must be 1 (the policy variable) or 2 (and consumption), got %d", n_het);
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before hank_vjp");
    return HANK_OK;
}

// hank_vjp_group's rules (grp_bar itself: the entries, below): agg_bar with n_het 1 or 2, or none with n_het 0; then the groups, then
// the record — hank_get_group_outputs' order
static int vjp_group_args(hank_ctx *ctx, int n_het, const void *in, int M, const void *out) {
    if (!ctx || !out || M < 1) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: bad argument (M=%d)", M);
    if (in && (n_het < 1 || n_het > 2))
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: with agg_bar n_het must be 1 (the policy variable) or 2 (and consumption), got %d; cotangents on Value / UCE "
                    "come from hank_vjp_het and add linearly", n_het);
    if (!in && n_het != 0) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: n_het=%d without agg_bar (n_het must be 0 then)", n_het);
    if (ctx->grp.K == 0) return fail(ctx, HANK_ERR_NOT_READY, "hank_vjp_group: no groups are set: call hank_set_group_outputs first");
    { const int irc = income_refuses(ctx, "hank_vjp_group"); if (irc) return irc; }
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before hank_vjp_group");
    return HANK_OK;
}

// hank_vjp_het's rules: the family's count, then the declared count (the rule of hank_get_het_outputs), then the record
static int vjp_het_args(hank_ctx *ctx, int n_het, const void *in, int M, const void *out) {
    if (!ctx || !in || !out || M < 1) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_het: bad argument (M=%d)", M);
    int rc = het_count_ok(ctx, "hank_vjp_het", n_het, true);
    if (!rc) rc = income_refuses(ctx, "hank_vjp_het");
    if (rc) return rc;
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "hank_primal must be called before hank_vjp_het");
    return HANK_OK;
}

// The eight entries' one body: args is the entry's rule (hank_vjp's, or hank_vjp_het's under which Value and UCE carry cotangents
// too); the _dev form leaves the copies to enqueue_vjp and stays asynchronous. value_end_bar, D_init_bar (the _boundary entries):
// the boundary's cotangents, either may be null (not wanted); the host form stages the wanted ones in the workspace of this width.
static int vjp_boundary(hank_ctx *ctx, int (*args)(hank_ctx *, int, const void *, int, const void *), int n_het, const double *agg_bar, int M, double *xhh_bar,
                        double *value_end_bar, double *D_init_bar, bool dev, const double *grp_bar = nullptr) {
    ENTER(ctx);
    int rc = args(ctx, n_het, agg_bar, M, xhh_bar);
    if (rc) return rc;
    CotWork *w = nullptr;
    CotReq q{n_het, agg_bar, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, M, dev ? xhh_bar : nullptr};
    q.grp_bar = grp_bar;
    if (dev) {
        q.d_vend_bar = value_end_bar;
        q.d_D0_bar = D_init_bar;
        return enqueue_vjp(ctx, q, &w);
    }
    const size_t GM = (size_t)ctx->c.G * M;
    if (value_end_bar || D_init_bar) {
        rc = tan_cache_get(ctx, ctx->cws, M, [ctx](CotWork &cw) { return build_cotwork(ctx, cw); }, &w);
        if (rc) return rc;
        if (!w->bnd_dbar) {
            HIPC(ctx, w->bnd_vbar.alloc(GM));
            HIPC(ctx, w->bnd_dbar.alloc(GM));
        }
    }
    if (value_end_bar) q.d_vend_bar = w->bnd_vbar.get();
    if (D_init_bar) q.d_D0_bar = w->bnd_dbar.get();
    rc = enqueue_vjp(ctx, q, &w);
    if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(xhh_bar, w->xbar, sizeof(double) * ctx->c.n_hh * ctx->c.P * M, hipMemcpyDeviceToHost, ctx->stream));
    if (value_end_bar) HIPC(ctx, hipMemcpyAsync(value_end_bar, w->bnd_vbar, sizeof(double) * GM, hipMemcpyDeviceToHost, ctx->stream));
    if (D_init_bar) HIPC(ctx, hipMemcpyAsync(D_init_bar, w->bnd_dbar, sizeof(double) * GM, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->errmsg[0] = 0;
    return HANK_OK;
}
static int vjp(hank_ctx *ctx, int (*args)(hank_ctx *, int, const void *, int, const void *), int n_het, const double *agg_bar, int M, double *xhh_bar, bool dev) {
    return vjp_boundary(ctx, args, n_het, agg_bar, M, xhh_bar, nullptr, nullptr, dev);
}

// hank_vjp_shock[_dev], hank_vjp_income[_dev]: the kind's rule (PathTraits::vjp_rule — hank_vjp_het's for beta_bar; hank_vjp's, n_het 1 or 2,
// for y_bar — then path_entry_excluded), the same work, Sweep B from the kind's graph with the path cotangent's reduction
static int vjp_path(hank_ctx *ctx, PathKind kind, int n_het, const double *agg_bar, int M, double *xhh_bar, double *path_bar, bool dev) {
    ENTER(ctx);
    const PathTraits &pt = PATHS[kind];
    if (ctx && !path_bar) return fail(ctx, HANK_ERR_BAD_ARG, "%s: %s is required", pt.vjp, pt.bar);
    int rc = pt.vjp_rule(ctx, n_het, agg_bar, M, xhh_bar);
    if (!rc) rc = path_entry_excluded(ctx, kind, pt.vjp);
    if (rc) return rc;
    CotWork *w = nullptr;
    CotReq q{n_het, agg_bar, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, M, dev ? xhh_bar : nullptr};
    q.path = kind;
    if (dev) q.d_path_bar = path_bar;
    rc = enqueue_vjp(ctx, q, &w);
    if (rc || dev) return rc;
    HIPC(ctx, hipMemcpyAsync(xhh_bar, w->xbar, sizeof(double) * ctx->c.n_hh * ctx->c.P * M, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipMemcpyAsync(path_bar, w->path[kind].cm, sizeof(double) * ctx->c.P * path_width(ctx->c, kind) * M, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

extern "C" {
// (KrusellSmith.jl:59-62, :66-80: where y enters; BackwardIteration.jl:90-113: the loop the transposed sweep reverses)
int hank_vjp_income(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *y_bar) { return vjp_path(ctx, PATH_INCOME, n_het, agg_bar, M, xhh_bar, y_bar, false); }
int hank_vjp_income_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_y_bar) { return vjp_path(ctx, PATH_INCOME, n_het, d_agg_bar, M, d_xhh_bar, d_y_bar, true); }
// (KrusellSmith.jl:59-62: where beta enters; BackwardIteration.jl:90-113: the loop the transposed sweep reverses)
int hank_vjp_shock(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *beta_bar) { return vjp_path(ctx, PATH_DISCOUNT, n_het, agg_bar, M, xhh_bar, beta_bar, false); }
int hank_vjp_shock_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_beta_bar) { return vjp_path(ctx, PATH_DISCOUNT, n_het, d_agg_bar, M, d_xhh_bar, d_beta_bar, true); }
// (KrusellSmith.jl:52, :76: where the limit enters; BackwardIteration.jl:90-113: the loop the transposed sweep reverses)
int hank_vjp_borrow(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *amin_bar) { return vjp_path(ctx, PATH_BORROW, n_het, agg_bar, M, xhh_bar, amin_bar, false); }
int hank_vjp_borrow_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_amin_bar) { return vjp_path(ctx, PATH_BORROW, n_het, d_agg_bar, M, d_xhh_bar, d_amin_bar, true); }
int hank_vjp_boundary_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar, double *d_D_init_bar) {
    { const int irc = income_refuses(ctx, "hank_vjp_boundary"); if (irc) return irc; }
    return vjp_boundary(ctx, vjp_args, n_het, d_agg_bar, M, d_xhh_bar, d_value_end_bar, d_D_init_bar, true);
}
// (KrusellSmith.jl:80: Value and UCE are keys of the plugin's NamedTuple; BackwardIteration.jl:85, ForwardIteration.jl:293: the boundary)
int hank_vjp_het_boundary_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar, double *d_D_init_bar) {
    return vjp_boundary(ctx, vjp_het_args, n_het, d_agg_bar, M, d_xhh_bar, d_value_end_bar, d_D_init_bar, true);
}
int hank_vjp_het_boundary(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar) {
    return vjp_boundary(ctx, vjp_het_args, n_het, agg_bar, M, xhh_bar, value_end_bar, D_init_bar, false);
}
int hank_vjp_boundary(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar) {
    { const int irc = income_refuses(ctx, "hank_vjp_boundary"); if (irc) return irc; }
    return vjp_boundary(ctx, vjp_args, n_het, agg_bar, M, xhh_bar, value_end_bar, D_init_bar, false);
}
// (ForwardIteration.jl:303-307: the weighted dot; :339-420 on :131-192: the reverse rules; BackwardIteration.jl:85, ForwardIteration.jl:293: the exports)
int hank_vjp_group(hank_ctx *ctx, int32_t n_het, const double *agg_bar, const double *grp_bar, int32_t M, double *xhh_bar, double *value_end_bar, double *D_init_bar) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    if (!grp_bar) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: grp_bar is required");
    return vjp_boundary(ctx, vjp_group_args, n_het, agg_bar, M, xhh_bar, value_end_bar, D_init_bar, false, grp_bar);
}
int hank_vjp_group_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, const double *d_grp_bar, int32_t M, double *d_xhh_bar, double *d_value_end_bar,
                       double *d_D_init_bar) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    if (!d_grp_bar) return fail(ctx, HANK_ERR_BAD_ARG, "hank_vjp_group: grp_bar is required");
    return vjp_boundary(ctx, vjp_group_args, n_het, d_agg_bar, M, d_xhh_bar, d_value_end_bar, d_D_init_bar, true, d_grp_bar);
}
int hank_vjp_het_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar) { return vjp(ctx, vjp_het_args, n_het, d_agg_bar, M, d_xhh_bar, true); }
int hank_vjp_het(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar) { return vjp(ctx, vjp_het_args, n_het, agg_bar, M, xhh_bar, false); }
int hank_vjp_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, int32_t M, double *d_xhh_bar) { return vjp(ctx, vjp_args, n_het, d_agg_bar, M, d_xhh_bar, true); }
int hank_vjp(hank_ctx *ctx, int32_t n_het, const double *agg_bar, int32_t M, double *xhh_bar) { return vjp(ctx, vjp_args, n_het, agg_bar, M, xhh_bar, false); }

int hank_get_policy_cotangent_seq(hank_ctx *ctx, int32_t M, double *out) {
    if (!ctx || !out) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!ctx->cot.current || ctx->cot.M != M) return fail(ctx, HANK_ERR_NOT_READY, "no hank_vjp with M=%d is current", M);
    const size_t G = ctx->c.G, P = ctx->c.P, total = P * G * (size_t)M;
    DevBuf<double> tmp;
    HIPC(ctx, tmp.alloc(total));
    hipLaunchKernelGGL(k_export_dpol, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, ctx->cot.pbar, (int)G, (int)P, M, tmp.get());
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipMemcpyAsync(out, tmp, sizeof(double) * total, hipMemcpyDeviceToHost, ctx->stream));
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    return HANK_OK;
}

int hank_last_vjp_timings(hank_ctx *ctx, double *out_ms, int32_t *launches) {      // (two slots each: VJP_A, VJP_B)
    if (!ctx || !out_ms) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; k++) HIPC(ctx, ctx->spans.read((Span)(VJP_A + k), &out_ms[k], launches ? &launches[k] : nullptr));
    return HANK_OK;
}
}  // extern "C"

// ---- granular steps ---------------------------------------------------------------------------
struct Scratch {  // a call's device buffers, of any element type: released on scope exit
    std::vector<DevBuf<char>> p;
    template <typename T> hipError_t alloc(T **out, size_t n) {
        p.emplace_back();
        const hipError_t e = p.back().alloc(n * sizeof(T));
        *out = reinterpret_cast<T *>(p.back().get());
        return e;
    }
};

static int granular_backward(hank_ctx *ctx, const double *value_next, const double *dvalue_next,
                             const double *xhh_t, const double *dxhh_t, int N, double *value_out,
                             double *dvalue_out, double *policy_out, double *dpolicy_out) {
    if (!ctx || !value_next || !xhh_t || !value_out || !policy_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    if (N > 0 && (!dvalue_next || !dxhh_t || !dvalue_out || !dpolicy_out)) return fail(ctx, HANK_ERR_BAD_ARG, "null tangent pointer");
    ENTER(ctx);
    { const int pend = device_verdict(ctx, THE_RECORD); if (pend) return pend; }      // an error a preceding async sweep left is reported, not overwritten: it is the record's
    const Consts &c = ctx->c;
    const size_t G = c.G;
    hipStream_t s = ctx->stream;
    Scratch sc;
    double *Vin, *xt, *sK, *kc, *A, *B, *u, *v, *pol, *Vout;
    int *ib;
    HIPC(ctx, sc.alloc(&Vin, G)); HIPC(ctx, sc.alloc(&xt, 3)); HIPC(ctx, sc.alloc(&sK, G)); HIPC(ctx, sc.alloc(&kc, G));
    HIPC(ctx, sc.alloc(&A, G)); HIPC(ctx, sc.alloc(&B, G)); HIPC(ctx, sc.alloc(&u, G)); HIPC(ctx, sc.alloc(&v, G));
    HIPC(ctx, sc.alloc(&pol, G)); HIPC(ctx, sc.alloc(&Vout, G)); HIPC(ctx, sc.alloc(&ib, G));
    if (!(1.0 + xhh_t[0] > 0.0)) return fail(ctx, HANK_ERR_DOMAIN, "1 + r must be positive");
    HIPC(ctx, hipMemcpyAsync(Vin, value_next, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(xt, xhh_t, sizeof(double) * c.n_hh, hipMemcpyHostToDevice, s));
    zero_err(ctx, s);
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp);
    hipLaunchKernelGGL(k_egm_X, grd, blk, primal_lds(c), s, c, Vin, xt, sK, kc, ctx->d_err, 0, (const int *)nullptr);
    hipLaunchKernelGGL(k_egm_Y, grd, blk, 0, s, c, sK, xhh_t[0], xhh_t[1], c.n_hh > 2 ? xhh_t[2] : 0.0, pol, ib, A, B, u, v, Vout, ctx->d_err, 0, (const int *)nullptr);
    HIPC(ctx, hipGetLastError());
    const int rc = device_verdict(ctx, THIS_CALL);      // the step's own error: the record and the batch stay as they were
    if (rc) return rc;
    HIPC(ctx, hipMemcpyAsync(value_out, Vout, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpyAsync(policy_out, pol, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    if (N > 0) {
        double *dVin, *dr, *dw, *dtr = nullptr, *ds, *dpol, *dV;
        HIPC(ctx, sc.alloc(&dVin, G * N)); HIPC(ctx, sc.alloc(&dr, N)); HIPC(ctx, sc.alloc(&dw, N));
        HIPC(ctx, sc.alloc(&ds, G * N)); HIPC(ctx, sc.alloc(&dpol, G * N)); HIPC(ctx, sc.alloc(&dV, G * N));
        std::vector<double> hr(N), hw(N), ht(N);
        for (int n = 0; n < N; n++) { hr[n] = dxhh_t[c.n_hh * n]; hw[n] = dxhh_t[c.n_hh * n + 1]; ht[n] = c.n_hh > 2 ? dxhh_t[c.n_hh * n + 2] : 0.0; }
        if (c.n_hh > 2) {
            HIPC(ctx, sc.alloc(&dtr, N));
            HIPC(ctx, hipMemcpyAsync(dtr, ht.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
        }
        HIPC(ctx, hipMemcpyAsync(dVin, dvalue_next, sizeof(double) * G * N, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync(dr, hr.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync(dw, hw.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
        const unsigned nb = (unsigned)((G * N + 255) / 256);
        hipLaunchKernelGGL(k_tan_X, dim3(nb), dim3(256), 0, s, c, kc, sK, xhh_t[0], dr, dw, dtr, N, dVin, ds);
        hipLaunchKernelGGL(k_tan_Y, dim3(nb), dim3(256), 0, s, c, ib, A, B, u, v, dr, dw, dtr, N, ds, dpol, dV);
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(dvalue_out, dV, sizeof(double) * G * N, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipMemcpyAsync(dpolicy_out, dpol, sizeof(double) * G * N, hipMemcpyDeviceToHost, s));
    }
    HIPC(ctx, hipStreamSynchronize(s));
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

// ---- n_het heterogeneous outputs (k_het_outputs and what it assembles: hank_hetx.h) --------------------------------------------
// outputs 2 .. n_het-1: for N > 0 the in-period sums of every direction (T) from one forward tangent recurrence over the exported
// policy partials (hank_hetx.h) and the record's f, f_c (ensure_hx_record, which also holds the direction-independent sums). The
// direction-dependent buffers live in the context (hx_slab: one allocation, grown when a wider batch asks, reused in stream
// order), so the _dev form stays asynchronous.
static int hx_outputs(hank_ctx *ctx, int NX, const TanBatch *b, double **T_out) {      // b: the current batch, or nullptr (no tangents asked for)
    const Consts &c = ctx->c;
    const int N = b ? b->N : 0;
    const size_t P = c.P, G = c.G;
    const int nbr = (c.n_a + HX_ROWS - 1) / HX_ROWS;
    int rc = ensure_hx_record(ctx);
    if (rc) return rc;
    *T_out = nullptr;
    if (N == 0) return HANK_OK;
    const size_t sz[5] = {P * G * N, G * N, G * N, (size_t)N * P * nbr * NX, (size_t)N * P * NX};
    size_t need = 0, off = 0;
    for (size_t k : sz) carve(need, sizeof(double) * k);
    if (need > ctx->hx_bytes) {
        if (ctx->hx_slab) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (the old slab is released by alloc)
        ctx->hx_bytes = 0;
        HIPC(ctx, ctx->hx_slab.alloc(need));
        ctx->hx_bytes = need;
    }
    double *buf[5];      // views
    for (int k = 0; k < 5; k++) buf[k] = reinterpret_cast<double *>(ctx->hx_slab + carve(off, sizeof(double) * sz[k]));
    double *dpc = buf[0], *mid = buf[1], *dD = buf[2], *parts = buf[3], *T = buf[4];
    rc = export_dpol_dev(ctx, *b, dpc);
    if (rc) return rc;
    const dim3 gmid((unsigned)((G + HX_ROWS - 1) / HX_ROWS), (unsigned)N), gmix((unsigned)nbr, (unsigned)N);
    for (size_t t = 0; t < P; t++) {
        hipLaunchKernelGGL(k_hx_mid, gmid, dim3(HX_ROWS), 0, ctx->stream, c, ctx->R, (int)t, dpc, dD, mid);
        hipLaunchKernelGGL(k_hx_mix, gmix, dim3(HX_ROWS), 0, ctx->stream, c, ctx->R, (int)t, NX, dpc, mid, ctx->hx.f.get(), ctx->hx.fc.get(), dD, parts);
    }
    const size_t cnt = (size_t)N * P * NX;
    hipLaunchKernelGGL(k_hx_reduce, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, parts, nbr, NX, cnt, T);
    HIPC(ctx, hipGetLastError());
    *T_out = T;
    return HANK_OK;
}

// (P, n_het) levels into d_a and (P, n_het, Nk) tangents into d_da (either may be null) from the aggregates, a batch's dagg_cm and the
// extra outputs' sums hxT: the one place that launches k_het_outputs, and k_bnd_cons behind it
static int assemble_het_outputs(hank_ctx *ctx, int n_het, int Nk, const double *d_dx, const double *dagg_cm, const double *hxT, const double *bnd_zm, double *d_a, double *d_da) {
    const size_t P = ctx->c.P;
    const int nh = ctx->c.n_hh;
    hipLaunchKernelGGL(k_het_outputs, dim3((unsigned)((P * ((size_t)Nk + 1) + 255) / 256)), dim3(256), 0, ctx->stream, (int)P, nh, n_het, hx_count(ctx), Nk, ctx->d_xhh,
                       d_dx, ctx->d_agg, dagg_cm, ctx->d_zd, ctx->hx.S.get(), hxT, d_a, d_da);
    // under a dD_0 seed the productivity marginal of dD_t does not vanish: consumption gains w_t zm_t + tr_t om_t (hank_boundary.h)
    if (d_da && n_het >= 2 && bnd_zm)
        hipLaunchKernelGGL(k_bnd_cons, dim3((unsigned)((P * Nk + 255) / 256)), dim3(256), 0, ctx->stream, (int)P, nh, n_het, Nk, ctx->d_xhh, bnd_zm, d_da);
    HIPC(ctx, hipGetLastError());
    return HANK_OK;
}

// income (hank_get_het_outputs_income; n_het <= 2): dy (n_e, P, N) column-major, the income directions of the batch hank_jvp_income made, or
// null — consumption's tangent gains sum_e dy_t[e,n] m_t[e]. Its level gains sum_e y_t[e] m_t[e] whenever a path is set, in either entry.
static int het_outputs(hank_ctx *ctx, int32_t n_het, const double *dxhh, int32_t N, double *agg_out, double *dagg_out, bool dev, const double *dy = nullptr,
                       PathKind entry = PATH_NONE) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    const char *who = entry == PATH_INCOME ? "hank_get_het_outputs_income" : "hank_get_het_outputs";
    int rc = het_count_ok(ctx, who, n_het, true, N >= 0 && (agg_out || dagg_out) && !(entry == PATH_INCOME && n_het > 2));      // (N >= 0, an output array)
    if (!rc && n_het > 2) rc = income_refuses(ctx, who);      // (Value and UCE rebuild c from the inputs)
    if (rc) return rc;
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
    const size_t P = ctx->c.P, nh = ctx->c.n_hh;
    const bool tan = dagg_out && N > 0;
    if (tan && !dxhh) return fail(ctx, HANK_ERR_BAD_ARG, "the tangent outputs need the dxhh of the last tangent sweep");
    const TanBatch *b = nullptr;
    if (tan) {
        rc = batch_current(ctx, N, &b);
        if (rc) return rc;
        if (b->inc_dy && n_het > 2)
            return fail(ctx, HANK_ERR_NOT_READY, "%s: the current tangent batch carries income directions (hank_jvp_income), under which only outputs 0 and 1 "
                        "have tangents (Value and UCE rebuild c from the inputs): n_het = %d is served again after hank_jvp", who, n_het);
        if (b->boundary && n_het > 2)
            return fail(ctx, HANK_ERR_NOT_READY, "hank_get_het_outputs: the current tangent batch carries boundary seeds (hank_jvp_boundary), under which only outputs 0 and 1 "
                        "have tangents (Value and UCE assume dD_0 = 0): n_het = %d is served again after hank_jvp", n_het);
    }
    HIPC(ctx, join_side(ctx));
    Scratch sc;
    const double *d_dx = dxhh;
    double *d_a = agg_out, *d_da = dagg_out;
    if (!dev) {
        double *tmp = nullptr;
        if (tan) {
            HIPC(ctx, sc.alloc(&tmp, nh * P * N));
            HIPC(ctx, hipMemcpyAsync(tmp, dxhh, sizeof(double) * nh * P * N, hipMemcpyHostToDevice, ctx->stream));
            d_dx = tmp;
            HIPC(ctx, sc.alloc(&d_da, P * n_het * N));
            if (dy) {
                HIPC(ctx, sc.alloc(&tmp, P * ctx->c.n_e * N));
                HIPC(ctx, hipMemcpyAsync(tmp, dy, sizeof(double) * P * ctx->c.n_e * N, hipMemcpyHostToDevice, ctx->stream));
                dy = tmp;
            }
        }
        if (agg_out) HIPC(ctx, sc.alloc(&d_a, P * n_het));
    }
    if (tan && !dy) dy = b->inc_dy;      // no dy from the caller: the batch's own (a device pointer; null for a batch without income directions)
    const int Nk = tan ? N : 0;
    double *hxT = nullptr;
    if (n_het > 2) {
        rc = hx_outputs(ctx, n_het - 2, b, &hxT);
        if (rc) return rc;
    }
    // (a batch with boundary seeds is served for n_het <= 2 only, above)
    rc = assemble_het_outputs(ctx, n_het, Nk, d_dx, b ? b->dagg_cm : nullptr, hxT, b ? b->bnd_zm : nullptr, d_a, tan ? d_da : nullptr);
    if (rc) return rc;
    const double *d_y = income_in_force(ctx);
    if (n_het == 2 && (d_y || (tan && dy))) {      // the direct term of y_t[e] in consumption (hank_income.h)
        rc = ensure_inc_mass(ctx);
        if (rc) return rc;
        hipLaunchKernelGGL(k_inc_cons, dim3((unsigned)((P * ((size_t)Nk + 1) + 255) / 256)), dim3(256), 0, ctx->stream, (int)P, ctx->c.n_e, Nk,
                           d_y, tan ? dy : (const double *)nullptr, ctx->d_inc_m.get(), d_a, tan ? d_da : nullptr);
        HIPC(ctx, hipGetLastError());
    }
    if (!dev) {
        if (agg_out) HIPC(ctx, hipMemcpyAsync(agg_out, d_a, sizeof(double) * P * n_het, hipMemcpyDeviceToHost, ctx->stream));
        if (tan) HIPC(ctx, hipMemcpyAsync(dagg_out, d_da, sizeof(double) * P * n_het * N, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HANK_OK;
}
extern "C" {
int hank_get_het_outputs(hank_ctx *ctx, int32_t n_het, const double *dxhh, int32_t N, double *agg_out, double *dagg_out) {
    return het_outputs(ctx, n_het, dxhh, N, agg_out, dagg_out, false);
}
int hank_get_het_outputs_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, int32_t N, double *d_agg_out, double *d_dagg_out) {
    return het_outputs(ctx, n_het, d_dxhh, N, d_agg_out, d_dagg_out, true);
}
// (KrusellSmith.jl:80: consumption is the budget residual, which gains y_t[e]; ForwardIteration.jl:303-307: the weighted dot)
int hank_get_het_outputs_income(hank_ctx *ctx, int32_t n_het, const double *dxhh, const double *dy, int32_t N, double *agg_out, double *dagg_out) {
    return het_outputs(ctx, n_het, dxhh, N, agg_out, dagg_out, false, dy, PATH_INCOME);
}
int hank_get_het_outputs_income_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, const double *d_dy, int32_t N, double *d_agg_out, double *d_dagg_out) {
    return het_outputs(ctx, n_het, d_dxhh, N, d_agg_out, d_dagg_out, true, d_dy, PATH_INCOME);
}
int hank_set_het_outputs(hank_ctx *ctx, int32_t n_het) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    const int rc = het_count_ok(ctx, "hank_set_het_outputs", n_het, false);
    if (rc) return rc;
    if (n_het != ctx->n_het) ctx->memo_valid = false;      // the next hank_primal_jvp records its primal afresh
    ctx->n_het = n_het;
    return HANK_OK;
}
}

// ---- group outputs (hank_groups.h) ---------------------------------------------------------------------------
// the groups' share of the record: built before the first reader at a record and a set of groups (group_outputs), after join_side
// (the sums read D_t). It reads the policies and D_t alone, so a call for the levels needs no lottery record. The only launch of
// k_grp_record.
static int ensure_grp_record(hank_ctx *ctx) {
    const Consts &c = ctx->c;
    GroupSet &g = ctx->grp;
    if (g.valid) return HANK_OK;
    hipLaunchKernelGGL(k_grp_record, dim3((unsigned)c.P, (unsigned)g.K), dim3(256), 0, ctx->stream, c, ctx->R, ctx->d_xhh, g.K, g.W.get(), g.base.get(), g.Y.get(), g.S.get());
    HIPC(ctx, hipGetLastError());
    g.valid = true;
    return HANK_OK;
}

static_assert(GRP_MAX == HANK_GROUP_MAX, "hank_groups.h and hank_hip.h disagree on the largest K");
template <int KC>
static void launch_grp_mix(hank_ctx *ctx, dim3 grid, int t, int N, const double *dpc, const double *mid, double *dD, double *parts) {
    const GroupSet &g = ctx->grp;
    hipLaunchKernelGGL(k_grp_mix<KC>, grid, dim3(GRP_ROWS * GRP_LANES), 0, ctx->stream, ctx->c, ctx->R, t, N, g.K, ctx->d_xhh, g.W.get(), g.codes, dpc, mid, dD, parts);
}

// the in-period sums T [n][t][k] of every direction of batch b: hx_outputs' recurrence (k_hx_mid as it is) with k_grp_mix's K
// reductions, in the groups' own slab (grown when a wider batch asks, reused in stream order: the _dev form stays asynchronous)
static int grp_tangent_sums(hank_ctx *ctx, const TanBatch &b, double **T_out) {
    const Consts &c = ctx->c;
    GroupSet &g = ctx->grp;
    const int N = b.N, K = g.K;
    const size_t P = c.P, G = c.G;
    const int nbr = (c.n_a + GRP_ROWS - 1) / GRP_ROWS;
    const size_t sz[5] = {P * G * N, G * N, G * N, (size_t)N * P * nbr * K, (size_t)N * P * K};
    size_t need = 0, off = 0;
    for (size_t k : sz) carve(need, sizeof(double) * k);
    if (need > g.bytes) {
        if (g.slab) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (the old slab is released by alloc)
        g.bytes = 0;
        HIPC(ctx, g.slab.alloc(need));
        g.bytes = need;
    }
    double *buf[5];      // views
    for (int k = 0; k < 5; k++) buf[k] = reinterpret_cast<double *>(g.slab + carve(off, sizeof(double) * sz[k]));
    double *dpc = buf[0], *mid = buf[1], *dD = buf[2], *parts = buf[3], *T = buf[4];
    int rc = ensure_lottery(ctx);      // (k_hx_mid reads lw, ig and start)
    if (rc) return rc;
    rc = export_dpol_dev(ctx, b, dpc);
    if (rc) return rc;
    const dim3 gmid((unsigned)((G + HX_ROWS - 1) / HX_ROWS), (unsigned)N), gmix((unsigned)nbr, (unsigned)((N + GRP_LANES - 1) / GRP_LANES));
    for (size_t t = 0; t < P; t++) {
        hipLaunchKernelGGL(k_hx_mid, gmid, dim3(HX_ROWS), 0, ctx->stream, c, ctx->R, (int)t, dpc, dD, mid);
        if (K <= 4) launch_grp_mix<4>(ctx, gmix, (int)t, N, dpc, mid, dD, parts);
        else if (K <= 8) launch_grp_mix<8>(ctx, gmix, (int)t, N, dpc, mid, dD, parts);
        else if (K <= 16) launch_grp_mix<16>(ctx, gmix, (int)t, N, dpc, mid, dD, parts);
        else launch_grp_mix<GRP_MAX>(ctx, gmix, (int)t, N, dpc, mid, dD, parts);
    }
    const size_t cnt = (size_t)N * P * K;
    hipLaunchKernelGGL(k_hx_reduce, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, parts, nbr, K, cnt, T);
    HIPC(ctx, hipGetLastError());
    *T_out = T;
    return HANK_OK;
}

// hank_get_group_outputs[_dev]: hank_get_het_outputs' rules, for the context's groups
static int group_outputs(hank_ctx *ctx, const double *dxhh, int32_t N, double *agg_out, double *dagg_out, bool dev) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (N < 0 || !(agg_out || dagg_out)) return fail(ctx, HANK_ERR_BAD_ARG, "hank_get_group_outputs: bad argument: N must be >= 0 and an output array given");
    const int K = ctx->grp.K;
    if (K == 0) return fail(ctx, HANK_ERR_NOT_READY, "hank_get_group_outputs: no groups are set: call hank_set_group_outputs first");
    for (int k = 0; k < K; k++)      // (a consumption group rebuilds c from the inputs)
        if (((ctx->grp.codes >> (2 * k)) & 3) == HANK_GROUP_CONS) {
            const int irc = income_refuses(ctx, "hank_get_group_outputs with a HANK_GROUP_CONS group");
            if (irc) return irc;
        }
    if (!ctx->primal_done) return fail(ctx, HANK_ERR_NOT_READY, "no primal sweep has been run");
    const size_t P = ctx->c.P, nh = ctx->c.n_hh;
    const bool tan = dagg_out && N > 0;
    if (tan && !dxhh) return fail(ctx, HANK_ERR_BAD_ARG, "the tangent outputs need the dxhh of the last tangent sweep");
    const TanBatch *b = nullptr;
    if (tan) {
        int rc = batch_current(ctx, N, &b);
        if (rc) return rc;
        if (b->inc_dy)
            for (int k = 0; k < K; k++)
                if (((ctx->grp.codes >> (2 * k)) & 3) == HANK_GROUP_CONS)
                    return fail(ctx, HANK_ERR_NOT_READY, "hank_get_group_outputs: the current tangent batch carries income directions (hank_jvp_income) and a HANK_GROUP_CONS "
                                "group rebuilds c from the inputs: its tangent is served again after hank_jvp");
        if (b->boundary)
            return fail(ctx, HANK_ERR_NOT_READY, "hank_get_group_outputs: the current tangent batch carries boundary seeds (hank_jvp_boundary); the group tangents "
                        "assume dD_0 = 0 and are served again after hank_jvp");
    }
    HIPC(ctx, join_side(ctx));
    Scratch sc;
    const double *d_dx = dxhh;
    double *d_a = agg_out, *d_da = dagg_out;
    if (!dev) {
        double *tmp = nullptr;
        if (tan) {
            HIPC(ctx, sc.alloc(&tmp, nh * P * N));
            HIPC(ctx, hipMemcpyAsync(tmp, dxhh, sizeof(double) * nh * P * N, hipMemcpyHostToDevice, ctx->stream));
            d_dx = tmp;
            HIPC(ctx, sc.alloc(&d_da, P * K * N));
        }
        if (agg_out) HIPC(ctx, sc.alloc(&d_a, P * K));
    }
    int rc = ensure_grp_record(ctx);
    if (rc) return rc;
    const int Nk = tan ? N : 0;
    double *T = nullptr;
    if (tan) {
        rc = grp_tangent_sums(ctx, *b, &T);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_grp_outputs, dim3((unsigned)((P * K * ((size_t)Nk + 1) + 255) / 256)), dim3(256), 0, ctx->stream, (int)P, (int)nh, K, Nk, d_dx,
                       ctx->grp.Y.get(), ctx->grp.S.get(), T, d_a, tan ? d_da : nullptr);
    HIPC(ctx, hipGetLastError());
    if (!dev) {
        if (agg_out) HIPC(ctx, hipMemcpyAsync(agg_out, d_a, sizeof(double) * P * K, hipMemcpyDeviceToHost, ctx->stream));
        if (tan) HIPC(ctx, hipMemcpyAsync(dagg_out, d_da, sizeof(double) * P * K * N, hipMemcpyDeviceToHost, ctx->stream));
        HIPC(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HANK_OK;
}
extern "C" {
int hank_get_group_outputs(hank_ctx *ctx, const double *dxhh, int32_t N, double *agg_out, double *dagg_out) {
    return group_outputs(ctx, dxhh, N, agg_out, dagg_out, false);
}
int hank_get_group_outputs_dev(hank_ctx *ctx, const double *d_dxhh, int32_t N, double *d_agg_out, double *d_dagg_out) {
    return group_outputs(ctx, d_dxhh, N, d_agg_out, d_dagg_out, true);
}
// The context's copies of W (G, K) and base[K]; K = 0 clears them. The record, the current tangent batch, the primal memo and the
// hank_set_het_outputs count stay as they are: only the groups' own share of the record (ensure_grp_record) is dropped.
int hank_set_group_outputs(hank_ctx *ctx, int32_t K, const double *W, const int32_t *base) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (K < 0 || K > HANK_GROUP_MAX) return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_group_outputs: bad argument: K must be 0..%d, got %d", HANK_GROUP_MAX, K);
    if (K > 0 && (!W || !base)) return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_group_outputs: null pointer");
    for (int k = 0; k < K; k++)
        if (base[k] < HANK_GROUP_MASS || base[k] > HANK_GROUP_CONS)
            return fail(ctx, HANK_ERR_BAD_ARG, "hank_set_group_outputs: bad argument: base[%d] = %d is none of HANK_GROUP_MASS, _POLICY, _CONS", k, base[k]);
    GroupSet &g = ctx->grp;
    const size_t P = ctx->c.P, G = ctx->c.G;
    if (g.K > 0) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (a reader of the old set may still be enqueued)
    g.valid = false;
    for (CotWork &cw : ctx->cws) cw.g_AG.reset();      // (hank_vjp_group's graphs hold the old set: see GroupSet)
    const int K_old = g.K;
    g.K = 0;      // (until the new set is complete: a failed allocation or copy leaves no groups set)
    if (K != K_old) {
        g.W.reset(); g.base.reset(); g.Y.reset(); g.S.reset();
        if (K == 0) return HANK_OK;
        HIPC(ctx, g.W.alloc(G * K)); HIPC(ctx, g.base.alloc(K));
        HIPC(ctx, g.Y.alloc(P * K)); HIPC(ctx, g.S.alloc(P * K * GRP_NS));
    }
    if (K == 0) return HANK_OK;
    HIPC(ctx, hipMemcpy(g.W.get(), W, sizeof(double) * G * K, hipMemcpyHostToDevice));
    HIPC(ctx, hipMemcpy(g.base.get(), base, sizeof(int32_t) * K, hipMemcpyHostToDevice));
    g.codes = grp_codes(base, K);
    g.K = K;
    return HANK_OK;
}
// hank_fake_news_group: hank_fake_news's precondition and refusals, for the context's groups: F (P, P, n_hh, K), Dv (P, n_hh, K)
int hank_fake_news_group(hank_ctx *ctx, double *F_out, double *Dv_out) {
    ENTER(ctx);
    if (!ctx || !F_out || !Dv_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    if (ctx->grp.K == 0) return fail(ctx, HANK_ERR_NOT_READY, "hank_fake_news_group: no groups are set: call hank_set_group_outputs first");
    return fake_news(ctx, 0, true, F_out, Dv_out);
}
}

// ---- hank_jvp_het[_dev]: every declared output's tangent from ONE pair of sweeps, boundary seeds included ----
// The request with a count (enqueue_tan_launch), seeded when a seed is given. For n_het > 2 the forward launches carry NX = n_het - 2 extra reductions
// (k_tan_fwd_hx): the in-period sums T_o,t = sum f_o,t dD_t - sum f_c,o,t D_t da'_t of Value and UCE (KrusellSmith.jl:80;
// ForwardIteration.jl:303-307 dots every key with the same D_t) from the dD_t the sweep itself carries — so a dD_0 seed
// (ForwardIteration.jl:293) needs nothing more, and a dV_P seed (BackwardIteration.jl:85) is already in dpol. k_het_outputs then
// assembles (P, n_het, N) as hank_get_het_outputs does (assemble_het_outputs).
// Launches: TAN_BACK P + 2 (P + 4 with seeds), TAN_FWD P + 3 (P + 5 with seeds), one more for n_het > 2; k_het_outputs (and
// k_bnd_cons) behind the spans. n_het <= 2 launches hank_jvp's / hank_jvp_boundary's own graphs.
// The batch is named as those two entries name theirs under the launch schedule, so the readers behave as they do after them.
static int enqueue_jvp_het(hank_ctx *ctx, const TanReq &q, int N, double *d_dagg_out, TanWork **out) {
    TanWork *w = nullptr;
    int rc = enqueue_tan_launch(ctx, q, N, &w);
    if (rc) return rc;
    rc = assemble_het_outputs(ctx, q.n_het, N, w->dxhh.get(), w->dagg_cm.get(), w->hx_T.get(), q.dD_init ? w->bnd_zm.get() : nullptr, nullptr, w->het_out.get());
    if (rc) return rc;
    if (d_dagg_out) HIPC(ctx, hipMemcpyAsync(d_dagg_out, w->het_out, sizeof(double) * ctx->c.P * q.n_het * N, hipMemcpyDeviceToDevice, ctx->stream));
    *out = w;
    return HANK_OK;
}
extern "C" {
int hank_jvp_het_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, const double *d_dvalue_end, const double *d_dD_init, int32_t N, double *d_dagg_out) {
    ENTER(ctx);
    const TanReq q{n_het, d_dxhh, d_dvalue_end, d_dD_init, hipMemcpyDeviceToDevice, d_dvalue_end || d_dD_init};
    const int rc = tan_seed_args(ctx, "hank_jvp_het", true, q, N, d_dagg_out, false);
    TanWork *w = nullptr;
    return rc ? rc : enqueue_jvp_het(ctx, q, N, d_dagg_out, &w);
}
int hank_jvp_het(hank_ctx *ctx, int32_t n_het, const double *dxhh, const double *dvalue_end, const double *dD_init, int32_t N, double *dagg_out) {
    ENTER(ctx);
    const TanReq q{n_het, dxhh, dvalue_end, dD_init, hipMemcpyHostToDevice, dvalue_end || dD_init};
    int rc = tan_seed_args(ctx, "hank_jvp_het", true, q, N, dagg_out, true);
    TanWork *w = nullptr;
    if (!rc) rc = enqueue_jvp_het(ctx, q, N, nullptr, &w);
    if (rc) return rc;
    // (the launches' tangent sweeps raise no device error: nothing to ask, as in hank_jvp)
    return tan_host_tail(ctx, dagg_out, w->het_out, (size_t)ctx->c.P * n_het * N);
}
}

extern "C" {
int hank_backward_step(hank_ctx *ctx, const double *value_next, const double *xhh_t, double *value_out, double *policy_out) {
    return granular_backward(ctx, value_next, nullptr, xhh_t, nullptr, 0, value_out, nullptr, policy_out, nullptr);
}
int hank_backward_step_dual(hank_ctx *ctx, const double *value_next, const double *dvalue_next,
                            const double *xhh_t, const double *dxhh_t, int32_t N, double *value_out,
                            double *dvalue_out, double *policy_out, double *dpolicy_out) {
    if (N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "N must be >= 1");
    return granular_backward(ctx, value_next, dvalue_next, xhh_t, dxhh_t, N, value_out, dvalue_out, policy_out, dpolicy_out);
}
}  // extern "C"

static void x_launch_vfi(XSection &sec, const XWork &X, const Consts &c, const XVfiArgs &a) { const size_t lds = x_lds_vfi(c); x_by_maxt(X, [&](auto mt) { XL(k_xvfi<decltype(mt)::value>); }); }
static void x_launch_stat(XSection &sec, const XWork &X, const Consts &c, const XStatArgs &a) { const size_t lds = x_lds_stat(c); x_by_maxt(X, [&](auto mt) { XL(k_xstat<decltype(mt)::value>); }); }
#undef XL
// A steady-state fixed point (in: IN_VFI | IN_POWER_METHOD) as ONE persistent launch on the group of XCD 0 (`launch` enqueues it on sync
// block 0), through to the verdict on this call's work. HANK_OK with *ran: the group formed, xs holds the kernel's {steps, converged}
// (d_state) and the error word was clean; HANK_OK without: it did not (or a wait timed out), the context has moved to the launches,
// d_state is zeroed for them and the word, taken here, held nothing. A forced schedule fails loudly.
template <typename Launch>
static int x_fixed_point(hank_ctx *ctx, ErrIn in, int *d_state, int xs[2], bool *ran, Launch launch) {
    hipStream_t s = ctx->stream;
    int rc = x_setup(ctx);
    XWork &X = ctx->xw;
    if (rc) return rc;
    XSection sec(ctx);
    HIPC(ctx, sec.opened());
    rc = x_sync_reset(sec, X.sync, 1, 4);
    if (rc) return rc;
    launch(sec, X);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, sec.close());
    XSync hsy;
    HIPC(ctx, hipMemcpyAsync(xs, d_state, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpyAsync(&hsy, X.sync, sizeof(XSync), hipMemcpyDeviceToHost, s));
    int e[4] = {0, 0, 0, 0};
    rc = take_error_word(ctx, e);
    if (rc) return rc;
    rc = x_status(ctx, in == IN_VFI ? "value iteration" : "power method", &hsy);
    X.last_blocks = 0;       // (this sync block has been judged here: a later call does not report it again)
    *ran = rc == HANK_OK;
    if (!*ran) {
        bool moved = false;
        rc = fallback_decision(ctx, rc, &moved);
        if (!moved) return rc;
        HIPC(ctx, hipMemsetAsync(d_state, 0, 2 * sizeof(int), s));
    }
    // ran or not: the word also speaks for the kernels in FRONT of the launch (the power method's lottery), which the launches do not run again
    return word_verdict(ctx, THIS_CALL, e, in, xs[0]);
}

// ---- steady state: the inner fixed point of get_xVals on the device (SteadyState.jl:132-141) ------------------
extern "C" int hank_vfi(hank_ctx *ctx, const double *xhh_t, double tol, int32_t max_iter, double *value_io, double *policy_out,
                        int32_t *iters_out, double *supnorm_out) {
    if (!ctx || !xhh_t || !value_io || !policy_out || max_iter < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument");
    if (!(1.0 + xhh_t[0] > 0.0)) return fail(ctx, HANK_ERR_DOMAIN, "1 + r must be positive");
    ENTER(ctx);
    { const int prc = path_refuses(ctx, "hank_vfi"); if (prc) return prc; }
    { const int pend = device_verdict(ctx, THE_RECORD); if (pend) return pend; }      // (what an earlier async sweep left pending)
    const Consts &c = ctx->c;
    const size_t G = c.G;
    hipStream_t s = ctx->stream;
    Scratch sc;
    double *V[2], *xt, *sK, *kc, *A, *B, *u, *v, *pol, *norm;
    int *ib, *state;
    HIPC(ctx, sc.alloc(&V[0], G)); HIPC(ctx, sc.alloc(&V[1], G)); HIPC(ctx, sc.alloc(&xt, 4)); HIPC(ctx, sc.alloc(&sK, G));
    HIPC(ctx, sc.alloc(&kc, G)); HIPC(ctx, sc.alloc(&A, G)); HIPC(ctx, sc.alloc(&B, G)); HIPC(ctx, sc.alloc(&u, G));
    HIPC(ctx, sc.alloc(&v, G)); HIPC(ctx, sc.alloc(&pol, G)); HIPC(ctx, sc.alloc(&norm, 1)); HIPC(ctx, sc.alloc(&ib, G));
    HIPC(ctx, sc.alloc(&state, 2));
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(V[0], value_io, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(xt, xhh_t, sizeof(double) * c.n_hh, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemsetAsync(state, 0, 2 * sizeof(int), s));
    zero_err(ctx, s);
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp);
    const double r = xhh_t[0], w = xhh_t[1], tr = c.n_hh > 2 ? xhh_t[2] : 0.0;
    int hstate[2] = {0, 0};
    auto finish = [&](const double *Vfin, int iters) -> int {
        double hn = 0.0;
        HIPC(ctx, hipMemcpyAsync(value_io, Vfin, sizeof(double) * G, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipMemcpyAsync(policy_out, pol, sizeof(double) * G, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipMemcpyAsync(&hn, norm, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));
        if (iters_out) *iters_out = iters;
        if (supnorm_out) *supnorm_out = hn;
        ctx->stats[VFI_ITERATIONS] += iters;
        ctx->errmsg[0] = 0;
        return HANK_OK;
    };
    const char *xve = getenv("HANK_XVFI");            // dev knob: 0 = per-step launches
    if (use_x_primal(ctx) && !(xve && atoi(xve) == 0)) {
        // the whole iteration as ONE persistent launch on the group of XCD 0 (k_xvfi): the vote on convergence rides on the group barrier
        int xs[2] = {0, 0};      // {steps, converged}
        bool ran = false;
        const int rc = x_fixed_point(ctx, IN_VFI, state, xs, &ran, [&](XSection &sec, const XWork &X) {
            XVfiArgs va{};
            va.c = c; va.V0 = V[0]; va.r = r; va.w = w; va.tr = tr; va.tol = tol; va.max_iter = max_iter; va.sy = X.sync; va.st_s = X.st_s;
            va.err = ctx->d_err; va.Vout = V[1]; va.pol = pol; va.iters = state; va.supnorm = norm;
            x_launch_vfi(sec, X, c, va);
        });
        if (rc) return rc;
        if (ran) return finish(V[1], xs[0]);
    }
    int done = 0;                      // steps enqueued
    const int chunk = 64;              // the stop flag travels to the host once per chunk; converged steps freeze the state
    while (!hstate[0] && done < max_iter) {
        const int n = std::min(chunk, max_iter - done);
        for (int k = 0; k < n; k++) {
            const int cur = (done + k) & 1;
            hipLaunchKernelGGL(k_egm_X, grd, blk, primal_lds(c), s, c, V[cur], xt, sK, kc, ctx->d_err, 0, (const int *)state);
            hipLaunchKernelGGL(k_egm_Y, grd, blk, 0, s, c, sK, r, w, tr, pol, ib, A, B, u, v, V[cur ^ 1], ctx->d_err, 0, (const int *)state);
            hipLaunchKernelGGL(k_vfi_check, dim3(1), dim3(1024), 0, s, V[cur ^ 1], V[cur], (int)G, tol, state, norm);
        }
        done += n;
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(hstate, state, sizeof(hstate), hipMemcpyDeviceToHost, s));
        int e[4], erc = take_error_word(ctx, e);      // (the chunk's synchronisation)
        if (!erc) erc = word_verdict(ctx, THIS_CALL, e, IN_VFI, hstate[1] + 1);
        if (erc) return erc;
    }
    return finish(V[hstate[1] & 1], hstate[1]);     // step k reads V[(k-1)&1] and writes V[k&1]
}

// ---- steady state: the stationary distribution by the power method on the device --------------------------------
// D <- Lambda(policy) D (Young lottery + exogenous transition: the forward step kernel of the hot path) until two
// iterates `check_every` steps apart differ by less than tol in the max norm, the rule of the host's power method
// (GeneralStructures.py:invariant_dist, used where the reference's direct solve of ForwardIteration.jl:436-442 is too
// large). The caller normalises the result.
extern "C" int hank_stationary_dist(hank_ctx *ctx, const double *policy, double *D_io, double tol, int32_t max_iter, int32_t check_every,
                                    int32_t *iters_out) {
    if (!ctx || !policy || !D_io || max_iter < 1 || check_every < 1) return fail(ctx, HANK_ERR_BAD_ARG, "bad argument");
    ENTER(ctx);
    { const int pend = device_verdict(ctx, THE_RECORD); if (pend) return pend; }      // (what an earlier async sweep left pending)
    const Consts &c = ctx->c;
    const size_t G = c.G;
    hipStream_t s = ctx->stream;
    Scratch sc;
    Record R{};      // ONE period of lottery record
    double *D[2], *Dchk, *aggp, *norm;
    int *state;
    HIPC(ctx, sc.alloc(&R.pol, G)); HIPC(ctx, sc.alloc(&R.lw, G)); HIPC(ctx, sc.alloc(&R.ig, G)); HIPC(ctx, sc.alloc(&R.lo, G));
    HIPC(ctx, sc.alloc(&R.start, (size_t)c.n_e * (c.n_a + 1))); HIPC(ctx, sc.alloc(&R.clo, c.n_e)); HIPC(ctx, sc.alloc(&R.seg, G));
    HIPC(ctx, sc.alloc(&R.lwg, G));
    HIPC(ctx, sc.alloc(&D[0], G)); HIPC(ctx, sc.alloc(&D[1], G)); HIPC(ctx, sc.alloc(&Dchk, G)); HIPC(ctx, sc.alloc(&aggp, 2 * (size_t)ctx->nbp));
    HIPC(ctx, sc.alloc(&norm, 1)); HIPC(ctx, sc.alloc(&state, 2));
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(R.pol, policy, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(D[0], D_io, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(Dchk, D_io, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemsetAsync(state, 0, 2 * sizeof(int), s));
    zero_err(ctx, s);
    hipLaunchKernelGGL(k_lottery, dim3((unsigned)c.n_e), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s, c, R, c.n_e, ctx->d_err, 1, 0);
    HIPC(ctx, hipGetLastError());
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp);
    int hstate[2] = {0, 0}, done = 0;
    const char *xse = getenv("HANK_XSTAT");           // dev knob: 0 = one launch per iteration
    if (use_x_primal(ctx) && !(xse && atoi(xse) == 0)) {
        // the whole power method as ONE persistent launch on the group of XCD 0 (k_xstat)
        int xs[2] = {0, 0};
        bool ran = false;
        const int rc = x_fixed_point(ctx, IN_POWER_METHOD, state, xs, &ran, [&](XSection &sec, const XWork &X) {
            XStatArgs sa{};
            sa.c = c; sa.R = R; sa.D0 = D[0]; sa.tol = tol; sa.max_iter = max_iter; sa.check_every = check_every; sa.sy = X.sync;
            sa.st_D = X.st_D; sa.Dout = D[1]; sa.iters = state;
            x_launch_stat(sec, X, c, sa);
        });
        if (rc) return rc;
        if (ran) {
            HIPC(ctx, hipMemcpyAsync(D_io, D[1], sizeof(double) * G, hipMemcpyDeviceToHost, s));
            HIPC(ctx, hipStreamSynchronize(s));
            if (iters_out) *iters_out = xs[0];
            ctx->errmsg[0] = 0;
            return HANK_OK;
        }
    }
    while (!hstate[0] && done < max_iter) {
        // a chunk = several checks; every check compares the iterate with the one check_every steps earlier
        for (int q = 0; q < 16 && done < max_iter; q++) {
            const int n = std::min((int)check_every, max_iter - done);
            for (int k = 0; k < n; k++, done++)
                hipLaunchKernelGGL(k_dist_iter, grd, blk, primal_lds(c), s, c, R, (const double *)D[done & 1], D[(done + 1) & 1], aggp, (const int *)state);
            hipLaunchKernelGGL(k_vfi_check, dim3(1), dim3(1024), 0, s, (const double *)D[done & 1], (const double *)Dchk, (int)G, tol, state, norm);
            HIPC(ctx, hipMemcpyAsync(Dchk, D[done & 1], sizeof(double) * G, hipMemcpyDeviceToDevice, s));
        }
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(hstate, state, sizeof(hstate), hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));
    }
    int e[4], erc = take_error_word(ctx, e);
    if (!erc) erc = word_verdict(ctx, THIS_CALL, e, IN_POWER_METHOD);
    if (erc) return erc;
    // once converged the iteration kernels stop touching the buffers: Dchk holds the last checked iterate
    HIPC(ctx, hipMemcpyAsync(D_io, Dchk, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    if (iters_out) *iters_out = done;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

static int granular_forward(hank_ctx *ctx, const double *policy, const double *dpolicy, const double *D_prev,
                            const double *dD_prev, int N, double *D_out, double *dD_out, double *agg_out, double *dagg_out) {
    if (!ctx || !policy || !D_prev || !D_out) return fail(ctx, HANK_ERR_BAD_ARG, "null pointer");
    if (N > 0 && (!dpolicy || !dD_prev || !dD_out)) return fail(ctx, HANK_ERR_BAD_ARG, "null tangent pointer");
    ENTER(ctx);
    const Consts &c = ctx->c;
    const size_t G = c.G, W = 1 + (size_t)N;
    hipStream_t s = ctx->stream;
    Scratch sc;
    double *pol, *dpol = nullptr, *Dp, *dDp = nullptr, *Dmid, *Do, *dDo = nullptr, *aggterm, *aggv;
    HIPC(ctx, sc.alloc(&pol, G)); HIPC(ctx, sc.alloc(&Dp, G)); HIPC(ctx, sc.alloc(&Dmid, G * W));
    HIPC(ctx, sc.alloc(&Do, G)); HIPC(ctx, sc.alloc(&aggterm, G * W)); HIPC(ctx, sc.alloc(&aggv, W));
    HIPC(ctx, sc.alloc(&dpol, G * (N ? N : 1))); HIPC(ctx, sc.alloc(&dDp, G * (N ? N : 1))); HIPC(ctx, sc.alloc(&dDo, G * (N ? N : 1)));
    HIPC(ctx, hipMemcpyAsync(pol, policy, sizeof(double) * G, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpyAsync(Dp, D_prev, sizeof(double) * G, hipMemcpyHostToDevice, s));
    if (N > 0) {
        HIPC(ctx, hipMemcpyAsync(dpol, dpolicy, sizeof(double) * G * N, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpyAsync(dDp, dD_prev, sizeof(double) * G * N, hipMemcpyHostToDevice, s));
    }
    HIPC(ctx, hipMemsetAsync(Dmid, 0, sizeof(double) * G * W, s));
    const unsigned nb = (unsigned)((G * W + 255) / 256);
    hipLaunchKernelGGL(k_scatter_general, dim3(nb), dim3(256), 0, s, c, pol, dpol, Dp, dDp, N, Dmid);
    hipLaunchKernelGGL(k_mix_general, dim3(nb), dim3(256), 0, s, c, Dmid, pol, dpol, N, Do, dDo, aggterm);
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)W), dim3(256), 0, s, aggterm, (int)G, (int)W, aggv);
    HIPC(ctx, hipGetLastError());
    std::vector<double> hagg(W);
    HIPC(ctx, hipMemcpyAsync(D_out, Do, sizeof(double) * G, hipMemcpyDeviceToHost, s));
    if (N > 0) HIPC(ctx, hipMemcpyAsync(dD_out, dDo, sizeof(double) * G * N, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpyAsync(hagg.data(), aggv, sizeof(double) * W, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    if (agg_out) *agg_out = hagg[0];
    if (dagg_out) for (int n = 0; n < N; n++) dagg_out[n] = hagg[1 + n];
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

extern "C" {
int hank_forward_step(hank_ctx *ctx, const double *policy, const double *D_prev, double *D_out, double *agg_out) {
    return granular_forward(ctx, policy, nullptr, D_prev, nullptr, 0, D_out, nullptr, agg_out, nullptr);
}
int hank_forward_step_dual(hank_ctx *ctx, const double *policy, const double *dpolicy, const double *D_prev,
                           const double *dD_prev, int32_t N, double *D_out, double *dD_out, double *agg_out, double *dagg_out) {
    if (N < 1) return fail(ctx, HANK_ERR_BAD_ARG, "N must be >= 1");
    return granular_forward(ctx, policy, dpolicy, D_prev, dD_prev, N, D_out, dD_out, agg_out, dagg_out);
}

}  // extern "C"

// ---- hank_primal_batch[_dev]: K input paths through one chain of launches (hank_scen.h) --------------------
// Scenario k is the launch family's hank_primal at x_k on a record of its own: the same bodies in the same order, so its policy and
// output 0 hold that entry's bits. The entry works on ScenWork only: the context's record, primal_done, both current batches, the
// memo, `stationary`, the schedule and the sweep counters stay as they were (hank_ss_jvp's rule). It reads what hank_set_boundary
// left (the terminal value, D_0, zd) and the model's grids.
constexpr int SCEN_KMAX = 64;

static int build_scenwork(hank_ctx *ctx, int K, ScenWork &w) {
    const Consts &c = ctx->c;
    const size_t P = c.P, G = c.G, d8 = P * G * sizeof(double), KK = (size_t)K;
    size_t off = 0;
    const size_t o_s = carve(off, d8), o_kc = carve(off, d8), o_A = carve(off, d8), o_B = carve(off, d8), o_u = carve(off, d8), o_v = carve(off, d8),
                 o_pol = carve(off, d8), o_lw = carve(off, d8), o_ig = carve(off, d8), o_D = carve(off, (P + 1) * G * sizeof(double)),
                 o_ib = carve(off, P * G * sizeof(int)), o_lo = carve(off, P * G * sizeof(int)),
                 o_st = carve(off, P * (size_t)c.n_e * (c.n_a + 1) * sizeof(int)), o_clo = carve(off, P * (size_t)c.n_e * sizeof(int));
    w.stride = off;      // (a multiple of 256: every scenario's arrays are aligned as scenario 0's)
    HIPC(ctx, w.slab.alloc(off * KK));
    char *b = w.slab;
    Record &R = w.R0;
    R = Record{};
    R.s = (double *)(b + o_s); R.kc = (double *)(b + o_kc); R.A = (double *)(b + o_A); R.B = (double *)(b + o_B);
    R.u = (double *)(b + o_u); R.v = (double *)(b + o_v); R.pol = (double *)(b + o_pol); R.lw = (double *)(b + o_lw);
    R.ig = (double *)(b + o_ig); R.Dseq = (double *)(b + o_D); R.ib = (int *)(b + o_ib); R.lo = (int *)(b + o_lo);
    R.start = (int *)(b + o_st); R.clo = (int *)(b + o_clo);
    const size_t nbp = ctx->nbp, NXM = (size_t)hx_count(ctx);
    HIPC(ctx, w.xhh.alloc((size_t)c.n_hh * P * KK));
    HIPC(ctx, w.aggpart.alloc(2 * P * nbp * KK));
    HIPC(ctx, w.agg_rm.alloc(2 * P * KK));
    HIPC(ctx, w.hxpart.alloc(NXM * P * nbp * KK));
    HIPC(ctx, w.hx_rm.alloc(NXM * P * KK));
    HIPC(ctx, w.out.alloc((size_t)het_max(ctx) * P * KK));
    HIPC(ctx, w.err.alloc(4 * KK));
    w.K = K;
    return HANK_OK;
}

// the two graphs of (K, n_het): ONE linear chain each on the context's own stream, backward then forward; no side stream
static int capture_scen_graphs(hank_ctx *ctx, ScenWork &w, int K, int n_het) {
    const Consts &c = ctx->c;
    const int P = c.P, NX = n_het > 2 ? n_het - 2 : 0;
    hipStream_t s = ctx->own_stream;
    const dim3 blk(RBP * c.n_e), grd(ctx->nbp, K);
    const size_t lds = primal_lds(c);
    const ScenArgs a{w.R0, w.stride, w.xhh.get(), w.err.get()};
    if (w.g_back || w.g_fwd) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (a batch of the _dev form may still be running the graphs released here)
    w.g_back.reset(); w.g_fwd.reset(); w.gK = 0;
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    hipLaunchKernelGGL(k_zero_i32, dim3((4 * K + 63) / 64), dim3(64), 0, s, w.err.get(), 4 * K);
    hipLaunchKernelGGL(k_scen_egm_X, grd, blk, lds, s, c, (const double *)ctx->d_ss_value.get(), a, P - 1);
    for (int t = P - 1; t >= 0; t--) hipLaunchKernelGGL(k_scen_egm_step, grd, blk, lds, s, c, a, t);
    hipLaunchKernelGGL(k_scen_lottery, dim3(P * c.n_e, K), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s, c, a, P * c.n_e);
    int rc = end_capture(ctx, &w.g_back);
    if (rc) return rc;
    HIPC(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int t = 0; t < P; t++)
        hipLaunchKernelGGL(k_scen_dist_step, grd, blk, lds, s, c, a, (const double *)ctx->d_ss_D, t, w.aggpart.get(), NX, w.hxpart.get());
    hipLaunchKernelGGL(k_reduce_parts, dim3(K * P, 1), dim3(256), 0, s, w.aggpart.get(), ctx->nbp, 2, w.agg_rm.get());
    if (NX > 0) hipLaunchKernelGGL(k_reduce_parts, dim3(K * P, 1), dim3(256), 0, s, w.hxpart.get(), ctx->nbp, NX, w.hx_rm.get());
    hipLaunchKernelGGL(k_scen_outputs, dim3((K * P + 255) / 256), dim3(256), 0, s, P, c.n_hh, n_het, K, (const double *)w.xhh.get(), (const double *)w.agg_rm.get(),
                       (const double *)ctx->d_zd.get(), (const double *)w.hx_rm.get(), w.out.get());
    rc = end_capture(ctx, &w.g_fwd);
    if (rc) { w.g_back.reset(); return rc; }
    w.gK = K; w.g_nhet = n_het;
    return HANK_OK;
}

static int ensure_scen(hank_ctx *ctx, int K, int n_het) {
    if (ctx->scen.K < K) {
        if (ctx->scen.K > 0) HIPC(ctx, hipStreamSynchronize(ctx->stream));      // (a batch enqueued by the _dev form may still run on the old buffers)
        ScenWork w;
        const int rc = build_scenwork(ctx, K, w);
        if (rc) return rc;      // (w goes, the context keeps what it had)
        ctx->scen = std::move(w);
    }
    if (ctx->scen.gK != K || ctx->scen.g_nhet != n_het) return capture_scen_graphs(ctx, ctx->scen, K, n_het);
    return HANK_OK;
}

// the K error words as status codes: status_out[k] (when given) for every scenario; the return value and the message are the
// lowest failing scenario's (k counts from 0, as status_out does; period, state and index from 1, as in every message)
static int scen_verdicts(hank_ctx *ctx, const int *words, int K, int32_t *status_out) {
    int first = HANK_OK, kfirst = -1;
    char keep[sizeof(ctx->errmsg)];
    for (int k = 0; k < K; k++) {
        const int rc = word_verdict(ctx, THIS_CALL, words + 4 * k, IN_SWEEP);
        if (status_out) status_out[k] = rc;
        if (rc && kfirst < 0) { first = rc; kfirst = k; memcpy(keep, ctx->errmsg, sizeof(keep)); }
    }
    if (kfirst < 0) { ctx->errmsg[0] = 0; return HANK_OK; }
    keep[sizeof(keep) - 1] = 0;
    return fail(ctx, first, "hank_primal_batch: scenario %d of %d: %.400s", kfirst, K, keep);
}
static int scen_pending_verdict(hank_ctx *ctx) {
    const int K = ctx->scen_pending;
    if (K <= 0) return HANK_OK;
    ctx->scen_pending = 0;
    std::vector<int> e(4 * (size_t)K);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    HIPC(ctx, hipMemcpy(e.data(), ctx->scen.err, e.size() * sizeof(int), hipMemcpyDeviceToHost));
    return scen_verdicts(ctx, e.data(), K, nullptr);      // (the next batch's graph clears the words)
}

static int primal_batch(hank_ctx *ctx, int n_het, const double *xhh, int K, double *agg_out, double *policy_out, int32_t *status_out, bool dev) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!xhh || !agg_out) return fail(ctx, HANK_ERR_BAD_ARG, "hank_primal_batch: null pointer");
    if (K < 1 || K > SCEN_KMAX) return fail(ctx, HANK_ERR_BAD_ARG, "hank_primal_batch: K must be 1..%d, got %d", SCEN_KMAX, K);
    int rc = het_count_ok(ctx, "hank_primal_batch", n_het, true);
    if (!rc) rc = path_refuses(ctx, "hank_primal_batch");
    if (rc) return rc;
    if (!ctx->boundary_set) return fail(ctx, HANK_ERR_NOT_READY, "hank_set_boundary must be called first");
    const Consts &c = ctx->c;
    const size_t P = c.P, G = c.G, nx = (size_t)c.n_hh * P, KK = (size_t)K;
    if (!dev)
        for (size_t k = 0; k < KK; k++)
            for (size_t t = 0; t < P; t++)
                if (!(1.0 + xhh[nx * k + c.n_hh * t] > 0.0)) return fail(ctx, HANK_ERR_DOMAIN, "hank_primal_batch: 1 + r must be positive (scenario %zu, period %zu)", k, t + 1);
    rc = ensure_scen(ctx, K, n_het);
    if (rc) return rc;
    ScenWork &w = ctx->scen;
    hipStream_t s = ctx->stream;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    ctx->scen_pending = 0;      // (the backward graph clears the words: an unread verdict of an earlier _dev batch goes with them)
    HIPC(ctx, hipMemcpyAsync(w.xhh, xhh, sizeof(double) * nx * KK, in, s));
    HIPC(ctx, ctx->spans.begin(SCEN_BACK, s));
    HIPC(ctx, hipGraphLaunch(w.g_back, s));
    HIPC(ctx, ctx->spans.end_begin(SCEN_BACK, c.P + 3, SCEN_FWD, s));
    HIPC(ctx, hipGraphLaunch(w.g_fwd, s));
    HIPC(ctx, ctx->spans.end(SCEN_FWD, s, c.P + (n_het > 2 ? 3 : 2)));
    HIPC(ctx, hipMemcpyAsync(agg_out, w.out, sizeof(double) * P * n_het * KK, back, s));
    if (policy_out) HIPC(ctx, hipMemcpy2DAsync(policy_out, sizeof(double) * P * G, w.R0.pol, w.stride, sizeof(double) * P * G, KK, back, s));
    if (dev) {
        ctx->scen_pending = K;      // the verdict arrives at hank_check
        return HANK_OK;
    }
    std::vector<int> e(4 * KK);
    HIPC(ctx, hipMemcpyAsync(e.data(), w.err, e.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));      // the call's one synchronisation
    return scen_verdicts(ctx, e.data(), K, status_out);
}

extern "C" {
int hank_primal_batch(hank_ctx *ctx, int32_t n_het, const double *xhh, int32_t K, double *agg_out, double *policy_out, int32_t *status_out) {
    return primal_batch(ctx, n_het, xhh, K, agg_out, policy_out, status_out, false);
}
int hank_primal_batch_dev(hank_ctx *ctx, int32_t n_het, const double *d_xhh, int32_t K, double *d_agg_out, double *d_policy_out) {
    return primal_batch(ctx, n_het, d_xhh, K, d_agg_out, d_policy_out, nullptr, true);
}
int hank_last_batch_timings(hank_ctx *ctx, double out_ms[2]) {
    if (!ctx || !out_ms) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; k++) HIPC(ctx, ctx->spans.read((Span)(SCEN_BACK + k), &out_ms[k], nullptr));
    return HANK_OK;
}
}

// ---- hank_ss_batch: the steady state's household side at K price vectors (hank_ssbatch.h) -----------------
// Scenario k is hank_vfi's launch branch at x_k, then hank_stationary_dist's, on a workspace of its own that lives for the call
// (Scratch): the context's record, primal_done, both current batches, the memo, `stationary`, the schedule and the sweep counters
// stay as they were; the context's error word is not touched (every scenario has its own). It needs no boundary.
//
// One loop of either kind: `enqueue` issues a chunk of launches for all K and returns the count of steps issued so far; the K stop
// words come back once per chunk; the loop ends when every scenario has stopped or `cap` steps are out.
template <typename Enqueue>
static int ssb_loop(hank_ctx *ctx, const SsbCtl *d_ctl, int K, int cap, std::vector<SsbCtl> &h, Span span, Enqueue enqueue) {
    hipStream_t s = ctx->stream;
    HIPC(ctx, ctx->spans.begin(span, s));
    int done = 0, launches = 0;
    bool all = false;
    while (!all && done < cap) {
        done = enqueue(done, &launches);
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(h.data(), d_ctl, sizeof(SsbCtl) * K, hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));
        all = true;
        for (int k = 0; k < K; k++) all = all && h[k].stop != 0;
    }
    HIPC(ctx, ctx->spans.end(span, s, launches));
    return HANK_OK;
}

extern "C" {
int hank_ss_batch(hank_ctx *ctx, int32_t n_het, const double *xhh, int32_t K, double vfi_tol, int32_t vfi_max_iter, double dist_tol, int32_t dist_max_iter,
                  int32_t check_every, double *value_io, double *policy_out, double *D_io, double *agg_out, int32_t *iters_out, double *supnorm_out,
                  int32_t *status_out) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!xhh || !value_io || !policy_out || !iters_out || !supnorm_out) return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_batch: null pointer");
    if (agg_out && !D_io) return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_batch: agg_out needs D_io (the aggregates are sums over the distribution)");
    if (K < 1 || K > SCEN_KMAX) return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_batch: K must be 1..%d, got %d", SCEN_KMAX, K);
    if (vfi_max_iter < 1 || dist_max_iter < 1 || check_every < 1) return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_batch: vfi_max_iter, dist_max_iter and check_every must be >= 1");
    if (agg_out) { const int hrc = het_count_ok(ctx, "hank_ss_batch", n_het, true); if (hrc) return hrc; }
    { const int prc = path_refuses(ctx, "hank_ss_batch"); if (prc) return prc; }
    const Consts &c = ctx->c;
    for (int k = 0; k < K; k++)
        if (!(1.0 + xhh[(size_t)c.n_hh * k] > 0.0)) return fail(ctx, HANK_ERR_DOMAIN, "hank_ss_batch: 1 + r must be positive (scenario %d of %d)", k, K);
    const size_t G = c.G, g8 = G * sizeof(double), g4 = G * sizeof(int), KK = (size_t)K, nbp = ctx->nbp;
    hipStream_t s = ctx->stream;
    // every scenario's arrays, carved alike: the value double buffer, the EGM step's one-period record, the lottery's, the distribution's
    size_t off = 0;
    const size_t o_V0 = carve(off, g8), o_V1 = carve(off, g8), o_s = carve(off, g8), o_kc = carve(off, g8), o_A = carve(off, g8), o_B = carve(off, g8),
                 o_u = carve(off, g8), o_v = carve(off, g8), o_pol = carve(off, g8), o_ib = carve(off, g4);
    size_t o_lw = 0, o_ig = 0, o_lo = 0, o_st = 0, o_clo = 0, o_D0 = 0, o_D1 = 0, o_Dc = 0, o_ap = 0;
    if (D_io) {
        o_lw = carve(off, g8); o_ig = carve(off, g8); o_lo = carve(off, g4); o_st = carve(off, (size_t)c.n_e * (c.n_a + 1) * sizeof(int));
        o_clo = carve(off, c.n_e * sizeof(int)); o_D0 = carve(off, g8); o_D1 = carve(off, g8); o_Dc = carve(off, g8); o_ap = carve(off, 2 * nbp * sizeof(double));
    }
    Scratch sc;
    char *b;
    double *xd, *expo, *outd = nullptr;
    int *err;
    SsbCtl *ctl;
    HIPC(ctx, sc.alloc(&b, off * KK)); HIPC(ctx, sc.alloc(&xd, (size_t)c.n_hh * KK)); HIPC(ctx, sc.alloc(&err, 4 * KK)); HIPC(ctx, sc.alloc(&ctl, 2 * KK));
    HIPC(ctx, sc.alloc(&expo, (D_io ? 3 : 2) * G * KK));
    if (agg_out) HIPC(ctx, sc.alloc(&outd, (size_t)n_het * KK));
    SsbArgs a{};
    a.V[0] = (double *)(b + o_V0); a.V[1] = (double *)(b + o_V1); a.sK = (double *)(b + o_s); a.kc = (double *)(b + o_kc); a.A = (double *)(b + o_A);
    a.B = (double *)(b + o_B); a.u = (double *)(b + o_u); a.v = (double *)(b + o_v); a.ib = (int *)(b + o_ib); a.R0.pol = (double *)(b + o_pol);
    if (D_io) {
        a.R0.lw = (double *)(b + o_lw); a.R0.ig = (double *)(b + o_ig); a.R0.lo = (int *)(b + o_lo); a.R0.start = (int *)(b + o_st); a.R0.clo = (int *)(b + o_clo);
        a.D[0] = (double *)(b + o_D0); a.D[1] = (double *)(b + o_D1); a.Dchk = (double *)(b + o_Dc); a.aggp = (double *)(b + o_ap);
    }
    a.stride = off; a.xhh = xd; a.err = err; a.vctl = ctl; a.dctl = ctl + KK;
    HIPC(ctx, join_side(ctx));
    HIPC(ctx, hipMemcpyAsync(xd, xhh, sizeof(double) * c.n_hh * KK, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemcpy2DAsync(a.V[0], off, value_io, g8, g8, KK, hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemsetAsync(err, 0, sizeof(int) * 4 * KK, s));
    HIPC(ctx, hipMemsetAsync(ctl, 0, sizeof(SsbCtl) * 2 * KK, s));
    const dim3 blk(RBP * c.n_e), grd((unsigned)nbp, (unsigned)K);
    const size_t lds = primal_lds(c);
    std::vector<SsbCtl> hv(KK), hd(KK);
    // 1. the value loops: three launches per step for all K, the stop words once per chunk of 64 steps
    int rc = ssb_loop(ctx, a.vctl, K, vfi_max_iter, hv, SSB_VALUE, [&](int done, int *launches) {
        const int n = std::min(64, (int)vfi_max_iter - done);
        for (int j = 0; j < n; j++) {
            const int cur = (done + j) & 1;
            hipLaunchKernelGGL(k_ssb_egm_X, grd, blk, lds, s, c, a, cur);
            hipLaunchKernelGGL(k_ssb_egm_Y, grd, blk, 0, s, c, a, cur);
            hipLaunchKernelGGL(k_ssb_vfi_check, dim3((unsigned)K), dim3(1024), 0, s, a, (int)G, cur, vfi_tol);
        }
        *launches += 3 * n;
        return done + n;
    });
    if (rc) return rc;
    if (D_io) {
        // 2. every scenario's lottery in one launch, then the power methods: a chunk = 16 checks, check_every iterations before each
        HIPC(ctx, hipMemcpy2DAsync(a.D[0], off, D_io, g8, g8, KK, hipMemcpyHostToDevice, s));
        HIPC(ctx, hipMemcpy2DAsync(a.Dchk, off, D_io, g8, g8, KK, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_ssb_lottery, dim3((unsigned)c.n_e, (unsigned)K), dim3(256), sizeof(int) * (2 * (size_t)c.n_a + 2), s, c, a);
        hipLaunchKernelGGL(k_ssb_dist_init, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, s, a, (int)K);
        rc = ssb_loop(ctx, a.dctl, K, dist_max_iter, hd, SSB_DIST, [&](int done, int *launches) {
            for (int q = 0; q < 16 && done < dist_max_iter; q++) {
                const int n = std::min((int)check_every, (int)dist_max_iter - done);
                for (int j = 0; j < n; j++, done++) hipLaunchKernelGGL(k_ssb_dist_iter, grd, blk, lds, s, c, a, done & 1);
                hipLaunchKernelGGL(k_ssb_dist_check, dim3((unsigned)K), dim3(1024), 0, s, a, (int)G, done & 1, n, dist_tol);
                *launches += n + 1;
            }
            return done;
        });
        if (rc) return rc;
        // 3. the outputs
        if (agg_out) {
            HIPC(ctx, hipMemsetAsync(outd, 0, sizeof(double) * n_het * KK, s));
            hipLaunchKernelGGL(k_ssb_outputs, dim3((unsigned)n_het, (unsigned)K), dim3(1024), 0, s, c, a, (int)n_het, outd);
            HIPC(ctx, hipMemcpyAsync(agg_out, outd, sizeof(double) * n_het * KK, hipMemcpyDeviceToHost, s));
        }
    } else {
        ctx->spans.invalidate({SSB_DIST});
    }
    double *Vexp = expo, *Pexp = expo + G * KK, *Dexp = D_io ? expo + 2 * G * KK : nullptr;
    hipLaunchKernelGGL(k_ssb_export, dim3((unsigned)((G + 255) / 256), (unsigned)K), dim3(256), 0, s, a, (int)G, Vexp, Pexp, Dexp);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipMemcpyAsync(value_io, Vexp, g8 * KK, hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipMemcpyAsync(policy_out, Pexp, g8 * KK, hipMemcpyDeviceToHost, s));
    if (D_io) HIPC(ctx, hipMemcpyAsync(D_io, Dexp, g8 * KK, hipMemcpyDeviceToHost, s));
    std::vector<int> e(4 * KK);
    HIPC(ctx, hipMemcpyAsync(e.data(), err, e.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));      // (the call's buffers go with it)
    // the verdict, per scenario: the value loop's word names the step that raised it; the lottery's is the power method's
    int first = HANK_OK, kfirst = -1;
    long long steps = 0;
    char keep[sizeof(ctx->errmsg)];
    for (int k = 0; k < K; k++) {
        iters_out[2 * k] = hv[k].n;
        iters_out[2 * k + 1] = D_io ? hd[k].n : 0;
        supnorm_out[k] = hv[k].norm;
        steps += hv[k].n;
        int vrc = word_verdict(ctx, THIS_CALL, &e[4 * k], IN_VFI, hv[k].n);
        if (!vrc) vrc = word_verdict(ctx, THIS_CALL, &e[4 * k], IN_POWER_METHOD);
        if (!vrc && e[4 * k]) vrc = word_verdict(ctx, THIS_CALL, &e[4 * k], IN_SWEEP);
        if (status_out) status_out[k] = vrc;
        if (vrc && kfirst < 0) { first = vrc; kfirst = k; memcpy(keep, ctx->errmsg, sizeof(keep)); }
    }
    ctx->stats[VFI_ITERATIONS] += steps;
    if (kfirst < 0) { ctx->errmsg[0] = 0; return HANK_OK; }
    keep[sizeof(keep) - 1] = 0;
    return fail(ctx, first, "hank_ss_batch: scenario %d of %d: %.400s", kfirst, K, keep);
}
int hank_last_ss_batch_timings(hank_ctx *ctx, double out_ms[2]) {
    if (!ctx || !out_ms) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; k++) HIPC(ctx, ctx->spans.read((Span)(SSB_VALUE + k), &out_ms[k], nullptr));
    return HANK_OK;
}
}  // extern "C"

// ---- derivatives through the steady state (hank_ssdiff.h) ------------------------------------------------
// The loop driver of all four fixed points, in the manner of hank_vfi's launch branch: a chunk of steps is enqueued (each step =
// the step kernel + the one-block check kernel), the stop word comes back once per chunk, and the steps enqueued behind a set stop
// word leave at once, so the state is the converged step's. step(k): the k-th step, 0-based (it reads buffer k & 1 of a ping-pong
// state and writes (k + 1) & 1: the final state sits in buffer iters & 1). Not converging is not an error: iters == max_iter.
// span: SS_VALUE or SS_DIST, the loop's time for hank_last_ss_timings.
template <typename Step>
static int ss_loop(hank_ctx *ctx, SsCtl *d_ctl, int max_iter, Step step, SsCtl *out, Span span) {
    hipStream_t s = ctx->stream;
    SsCtl h{};
    HIPC(ctx, ctx->spans.begin(span, s));      // (no host synchronisation for the timing: events on the stream)
    HIPC(ctx, hipMemsetAsync(d_ctl, 0, sizeof(SsCtl), s));
    int done = 0;
    const int chunk = 64;
    while (!h.stop && done < max_iter) {
        const int n = std::min(chunk, max_iter - done);
        for (int k = 0; k < n; k++) step(done + k);
        done += n;
        HIPC(ctx, hipGetLastError());
        HIPC(ctx, hipMemcpyAsync(&h, d_ctl, sizeof(SsCtl), hipMemcpyDeviceToHost, s));
        HIPC(ctx, hipStreamSynchronize(s));
    }
    HIPC(ctx, ctx->spans.end(span, s, 2 * done));
    *out = h;
    return HANK_OK;
}

// what both entries ask of their arguments and of the context, in hank_fake_news's order: the count of outputs (hank_vjp_het's
// rule), then the stationary record
static int ss_ready(hank_ctx *ctx, const char *name, int n_het, bool rest_ok) {
    int rc = het_count_ok(ctx, name, n_het, true, rest_ok);
    if (!rc) rc = path_refuses(ctx, name);
    if (rc) return rc;
    rc = stationary_record(ctx, name);
    if (rc) return rc;
    if (ctx->c.P < 2) return fail(ctx, HANK_ERR_BAD_ARG, "%s needs a record of at least two periods (T >= 3)", name);
    return HANK_OK;
}

static int ss_jvp(hank_ctx *ctx, int n_het, const double *dxhh, int N, double tol, int max_iter, double *dvalue_out, double *dpolicy_out, double *dD_out,
                  double *dagg_out, int32_t *iters_out, double *resid_out, bool dev) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    int rc = ss_ready(ctx, "hank_ss_jvp", n_het, dxhh && dagg_out && iters_out && resid_out && N >= 1 && max_iter >= 1 && tol >= 0.0);
    if (rc) return rc;
    const Consts &c = ctx->c;
    const size_t G = c.G, GV = (size_t)(c.n_a + KV) * c.n_e, NN = (size_t)N;
    const int NX = n_het > 2 ? n_het - 2 : 0, V = (N % 2 == 0) ? 2 : 1;
    hipStream_t s = ctx->stream;
    const TanGeom g = tan_geom(c.n_a, N, V);
    TanGeom gf = g;
    gf.ss = g.NC >= 16 ? 1 : 0;
    const int RGB = 2, RGF = gf.ss ? 2 : 1;
    const unsigned nbt = (g.nbx + RGB - 1) / RGB, nbf = (gf.nbx + RGF - 1) / RGF + KV, ny = (g.N + g.NC - 1) / g.NC;
    { const int src = ensure_seg(ctx); if (src) return src; }
    { const int src = ensure_lwg(ctx); if (src) return src; }
    HIPC(ctx, join_side(ctx));
    if (NX > 0) { rc = ensure_hx_record(ctx); if (rc) return rc; }
    Scratch sc;
    double *dx, *dxr, *dxw, *dxt, *ds[2], *dV, *dpol, *dD[2], *aggpart, *hxparts, *partsB, *partsF, *sig, *out, *expV = nullptr, *expP = nullptr, *expD = nullptr;
    SsCtl *ctl;
    HIPC(ctx, sc.alloc(&dx, (size_t)c.n_hh * NN)); HIPC(ctx, sc.alloc(&dxr, 2 * NN)); HIPC(ctx, sc.alloc(&dxw, 2 * NN)); HIPC(ctx, sc.alloc(&dxt, 2 * NN));
    HIPC(ctx, sc.alloc(&ds[0], G * NN)); HIPC(ctx, sc.alloc(&ds[1], G * NN)); HIPC(ctx, sc.alloc(&dV, G * NN)); HIPC(ctx, sc.alloc(&dpol, 2 * G * NN));
    HIPC(ctx, sc.alloc(&dD[0], GV * NN)); HIPC(ctx, sc.alloc(&dD[1], GV * NN)); HIPC(ctx, sc.alloc(&aggpart, 2 * (size_t)nbf * NN));
    HIPC(ctx, sc.alloc(&hxparts, (size_t)nbf * (NX ? NX : 1) * NN)); HIPC(ctx, sc.alloc(&partsB, 2 * (size_t)nbt * NN));
    HIPC(ctx, sc.alloc(&partsF, 3 * (size_t)nbf * NN)); HIPC(ctx, sc.alloc(&sig, NN)); HIPC(ctx, sc.alloc(&out, (size_t)n_het * NN));
    HIPC(ctx, sc.alloc(&ctl, 2));
    if (!dev && dvalue_out) HIPC(ctx, sc.alloc(&expV, G * NN));
    if (!dev && dpolicy_out) HIPC(ctx, sc.alloc(&expP, G * NN));
    if (!dev && dD_out) HIPC(ctx, sc.alloc(&expD, G * NN));
    HIPC(ctx, hipMemcpyAsync(dx, dxhh, sizeof(double) * c.n_hh * NN, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIPC(ctx, hipMemsetAsync(ds[0], 0, sizeof(double) * G * NN, s));
    HIPC(ctx, hipMemsetAsync(dV, 0, sizeof(double) * G * NN, s));
    HIPC(ctx, hipMemsetAsync(dD[0], 0, sizeof(double) * GV * NN, s));
    hankss_launch_in(s, dx, c.n_hh, N, dxr, dxw, dxt);
    SsCtl hv{}, hd{};
    // 1. dV <- B_V dV + B_x dx; the converged step leaves dV and da' (row 1 of dpol)
    rc = ss_loop(ctx, &ctl[0], max_iter, [&](int k) {
        hankss_launch_back(s, V, c, ctx->R, ctx->d_xhh.get(), dxr, dxw, dxt, g, nbt, ny, ds[k & 1], ds[(k + 1) & 1], dpol, dV, partsB, &ctl[0]);
        hankss_launch_check(s, partsB, (int)nbt, 2, N, tol, &ctl[0], nullptr);
    }, &hv, SS_VALUE);
    if (rc) return rc;
    // 2. dD <- Lambda dD + (dLambda da') D with that da'; the last step's reductions are dY's
    const double *dap = dpol + G * NN;
    rc = ss_loop(ctx, &ctl[1], max_iter, [&](int k) {
        hankss_launch_fwd(s, V, NX, c, ctx->R, gf, nbf, ny, dD[k & 1], dD[(k + 1) & 1], dap, aggpart, ctx->hx.f.get(), ctx->hx.fc.get(), hxparts, partsF, &ctl[1]);
        hankss_launch_check_dist(s, c, ctx->R.Dseq, partsF, (int)nbf, N, tol, dD[(k + 1) & 1], dD[k & 1], sig, &ctl[1]);
    }, &hd, SS_DIST);
    if (rc) return rc;
    const double *dDfin = dD[hd.iters & 1];
    hankss_launch_jvp_out(s, c.P, c.n_hh, n_het, N, (int)nbf, ctx->d_xhh.get(), dx, ctx->d_agg.get(), ctx->d_zd.get(), ctx->hx.S.get(), aggpart, hxparts, out);
    const dim3 tblk(BND_T, 8), tgrd((unsigned)((c.n_a + BND_T - 1) / BND_T), (unsigned)((N + BND_T - 1) / BND_T), (unsigned)c.n_e);
    const hipMemcpyKind back = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPC(ctx, hipMemcpyAsync(dagg_out, out, sizeof(double) * n_het * NN, back, s));
    // the exports (G, N) column-major; the host form stages each in a buffer of its own
    if (dvalue_out) {
        hipLaunchKernelGGL(k_bnd_out, tgrd, tblk, 0, s, dV, c.n_a, c.n_e, N, dev ? dvalue_out : expV);
        if (!dev) HIPC(ctx, hipMemcpyAsync(dvalue_out, expV, sizeof(double) * G * NN, hipMemcpyDeviceToHost, s));
    }
    if (dpolicy_out) {
        hipLaunchKernelGGL(k_bnd_out, tgrd, tblk, 0, s, dap, c.n_a, c.n_e, N, dev ? dpolicy_out : expP);
        if (!dev) HIPC(ctx, hipMemcpyAsync(dpolicy_out, expP, sizeof(double) * G * NN, hipMemcpyDeviceToHost, s));
    }
    if (dD_out) {
        hankss_launch_dist_out(s, dDfin, c.n_a, c.n_e, N, dev ? dD_out : expD);
        if (!dev) HIPC(ctx, hipMemcpyAsync(dD_out, expD, sizeof(double) * G * NN, hipMemcpyDeviceToHost, s));
    }
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipStreamSynchronize(s));      // (the call's buffers go with it)
    iters_out[0] = hv.iters; iters_out[1] = hd.iters;
    resid_out[0] = hv.resid; resid_out[1] = hd.resid;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

static int ss_vjp_loops(hank_ctx *ctx, int V, const AdjGeom &g, int NX, double tol, int max_iter, double *e[2], double *lam, double *pbar, double *nu[2], const double *vbar,
                        const double *yb, double *partS, double *partM, double *parts, double *cen, SsCtl *ctl, SsCtl *hn, SsCtl *hl) {
    const Consts &c = ctx->c;
    hipStream_t s = ctx->stream;
    const int M = g.MV * V;
    const size_t ldsA = adj_lds_dist(c, g, V), ldsB = adj_lds_egm(c, g, V), PG = (size_t)c.P * c.G;
    // 1. lam = sum_u (Lambda')^u g, re-centred every step (dev knob HANK_SS_RECENTRE=0: centred once, at the start — the series of the
    // plain formula, which stalls where D_ss is stationary only to the caller's accuracy: scripts/dev_ss_diff.py shows it)
    const char *rce = getenv("HANK_SS_RECENTRE");
    const bool recentre = !(rce && atoi(rce) == 0);
    int rc = ss_loop(ctx, &ctl[1], max_iter, [&](int k) {
        hankss_launch_lam(s, V, false, ldsA, c, ctx->R, g, e[k & 1], e[(k + 1) & 1], lam, parts, &ctl[1], cen, nullptr, 0, nullptr, PG, nullptr);
        hankss_launch_check(s, parts, g.nb, 3, M, tol, &ctl[1], recentre ? cen : nullptr);
    }, hl, SS_DIST);
    if (rc) return rc;
    // 2. pbar from lam (Sweep A's pbar line at one period)
    hankss_launch_lam(s, V, true, ldsA, c, ctx->R, g, lam, nullptr, nullptr, nullptr, nullptr, nullptr, yb, NX, ctx->hx.fc.get(), PG, pbar);
    // 3. nu <- B_V' nu + (P_V' pbar + Vbar)
    return ss_loop(ctx, &ctl[0], max_iter, [&](int k) {
        hankss_launch_nu(s, V, ldsB, c, ctx->R, g, ctx->d_adj_sb.get(), nu[k & 1], nu[(k + 1) & 1], pbar, vbar, partS, partM, parts, &ctl[0]);
        hankss_launch_check(s, parts, g.nb, 2, M, tol, &ctl[0], nullptr);
    }, hn, SS_VALUE);
}

static int ss_vjp(hank_ctx *ctx, int n_het, const double *agg_bar, const double *value_bar, const double *D_bar, int M, double tol, int max_iter, double *xhh_bar,
                  int32_t *iters_out, double *resid_out, bool dev) {
    if (!ctx) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    if (!agg_bar && !value_bar && !D_bar) return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_vjp: agg_bar, value_bar and D_bar are all NULL: nothing to pull back");
    int rc = ss_ready(ctx, "hank_ss_vjp", n_het, xhh_bar && iters_out && resid_out && M >= 1 && max_iter >= 1 && tol >= 0.0);
    if (rc) return rc;
    const Consts &c = ctx->c;
    const size_t G = c.G, MM = (size_t)M;
    const int NX = n_het > 2 ? n_het - 2 : 0, V = adj_lane_width(M);
    hipStream_t s = ctx->stream;
    const AdjGeom g = adj_geom(c.n_a, M);
    if (adj_lds_dist(c, g, V) > ctx->lds_max || adj_lds_egm(c, g, V) > ctx->lds_max)
        return fail(ctx, HANK_ERR_BAD_ARG, "hank_ss_vjp: n_e=%d needs more LDS per workgroup than the device has", c.n_e);
    if (!ctx->d_adj_sb) HIPC(ctx, ctx->d_adj_sb.alloc((size_t)c.P * c.n_e * ((size_t)c.n_a + 1)));
    HIPC(ctx, join_side(ctx));
    rc = ensure_adj_seg(ctx);
    if (rc) return rc;
    if (NX > 0) { rc = ensure_hx_record(ctx); if (rc) return rc; }
    Scratch sc;
    double *ybar = nullptr, *stage = nullptr, *yb, *e[2], *lam, *pbar, *nu[2], *vbar = nullptr, *partS, *partM, *parts, *xbar, *cen;
    SsCtl *ctl;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPC(ctx, sc.alloc(&yb, 4 * MM)); HIPC(ctx, sc.alloc(&e[0], G * MM)); HIPC(ctx, sc.alloc(&e[1], G * MM)); HIPC(ctx, sc.alloc(&lam, G * MM));
    HIPC(ctx, sc.alloc(&pbar, G * MM)); HIPC(ctx, sc.alloc(&nu[0], G * MM)); HIPC(ctx, sc.alloc(&nu[1], G * MM));
    HIPC(ctx, sc.alloc(&partS, 3 * (size_t)g.nb * MM)); HIPC(ctx, sc.alloc(&partM, 3 * (size_t)g.nb * MM)); HIPC(ctx, sc.alloc(&parts, 3 * (size_t)g.nb * MM)); HIPC(ctx, sc.alloc(&cen, MM));
    HIPC(ctx, sc.alloc(&xbar, (size_t)c.n_hh * MM)); HIPC(ctx, sc.alloc(&ctl, 2));
    if (agg_bar) {
        HIPC(ctx, sc.alloc(&ybar, (size_t)n_het * MM));
        HIPC(ctx, hipMemcpyAsync(ybar, agg_bar, sizeof(double) * n_het * MM, in, s));
    }
    hankss_launch_y_in(s, ybar, n_het, M, yb);
    const dim3 tblk(BND_T, 8), tgrd((unsigned)((c.n_a + BND_T - 1) / BND_T), (unsigned)((M + BND_T - 1) / BND_T), (unsigned)c.n_e);
    if (value_bar || D_bar) HIPC(ctx, sc.alloc(&stage, G * MM));
    if (value_bar) {
        HIPC(ctx, sc.alloc(&vbar, G * MM));
        HIPC(ctx, hipMemcpyAsync(stage, value_bar, sizeof(double) * G * MM, in, s));
        hipLaunchKernelGGL(k_bnd_in, tgrd, tblk, 0, s, (const double *)stage, c.n_a, c.n_e, c.n_a, M, vbar);
    }
    if (D_bar) HIPC(ctx, hipMemcpyAsync(stage, D_bar, sizeof(double) * G * MM, in, s));      // (behind k_bnd_in on the stream)
    hankss_launch_cot_in(s, c, ctx->R, ctx->d_xhh.get(), NX, yb, D_bar ? stage : nullptr, ctx->hx.f.get(), (size_t)c.P * G, M, e[0], lam);
    HIPC(ctx, hipMemsetAsync(nu[0], 0, sizeof(double) * G * MM, s));
    HIPC(ctx, hipMemsetAsync(cen, 0, sizeof(double) * MM, s));      // (k_ss_cot_in has centred e_0)
    SsCtl hn{}, hl{};
    rc = ss_vjp_loops(ctx, V, g, NX, tol, max_iter, e, lam, pbar, nu, vbar, yb, partS, partM, parts, cen, ctl, &hn, &hl);
    if (rc) return rc;
    hankss_launch_xbar(s, c.P, c.n_hh, M, g.nb, NX, ctx->d_xhh.get(), partS, partM, yb, ctx->d_agg.get(), ctx->d_zd.get(), ctx->hx.S.get(), xbar);
    HIPC(ctx, hipGetLastError());
    HIPC(ctx, hipMemcpyAsync(xhh_bar, xbar, sizeof(double) * c.n_hh * MM, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    HIPC(ctx, hipStreamSynchronize(s));
    iters_out[0] = hn.iters; iters_out[1] = hl.iters;
    resid_out[0] = hn.resid; resid_out[1] = hl.resid;
    ctx->errmsg[0] = 0;
    return HANK_OK;
}

extern "C" {
// (SteadyState.jl:195 differentiates the steady state's residual through the VFI of :132-141 and through invariant_dist's
// implicit-function tangent, ForwardIteration.jl:446-530)
int hank_ss_jvp(hank_ctx *ctx, int32_t n_het, const double *dxhh, int32_t N, double tol, int32_t max_iter, double *dvalue_out, double *dpolicy_out, double *dD_out,
                double *dagg_out, int32_t *iters_out, double *resid_out) {
    return ss_jvp(ctx, n_het, dxhh, N, tol, max_iter, dvalue_out, dpolicy_out, dD_out, dagg_out, iters_out, resid_out, false);
}
int hank_ss_jvp_dev(hank_ctx *ctx, int32_t n_het, const double *d_dxhh, int32_t N, double tol, int32_t max_iter, double *d_dvalue_out, double *d_dpolicy_out,
                    double *d_dD_out, double *d_dagg_out, int32_t *iters_out, double *resid_out) {
    return ss_jvp(ctx, n_het, d_dxhh, N, tol, max_iter, d_dvalue_out, d_dpolicy_out, d_dD_out, d_dagg_out, iters_out, resid_out, true);
}
int hank_ss_vjp(hank_ctx *ctx, int32_t n_het, const double *agg_bar, const double *value_bar, const double *D_bar, int32_t M, double tol, int32_t max_iter,
                double *xhh_bar, int32_t *iters_out, double *resid_out) {
    return ss_vjp(ctx, n_het, agg_bar, value_bar, D_bar, M, tol, max_iter, xhh_bar, iters_out, resid_out, false);
}
int hank_ss_vjp_dev(hank_ctx *ctx, int32_t n_het, const double *d_agg_bar, const double *d_value_bar, const double *d_D_bar, int32_t M, double tol, int32_t max_iter,
                    double *d_xhh_bar, int32_t *iters_out, double *resid_out) {
    return ss_vjp(ctx, n_het, d_agg_bar, d_value_bar, d_D_bar, M, tol, max_iter, d_xhh_bar, iters_out, resid_out, true);
}
int hank_last_ss_timings(hank_ctx *ctx, double *out_ms) {
    if (!ctx || !out_ms) return HANK_ERR_BAD_ARG;
    ENTER(ctx);
    HIPC(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 2; k++) HIPC(ctx, ctx->spans.read((Span)(SS_VALUE + k), &out_ms[k], nullptr));
    return HANK_OK;
}
}  // extern "C"
