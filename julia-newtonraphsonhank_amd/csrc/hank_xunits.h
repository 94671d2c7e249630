// hank_xunits.h — plain C++ on integers, no device code of its own: how ONE column's walk over the sources of ONE member's target
// rows is cut into the forward sweeps' work units (k_xfwd, hank_xsweep.h). A unit is a run [ta, tb) of target rows (relative to the
// member's first row r0) and the <= 64 consecutive sources [ja, ja + cnt) whose lottery brackets touch it; the unit that walks
// source row 0 of an open column while the virtual rows hold mass (vnz) carries nv = Sact extra lanes. The same greedy walk as
// k_xunits_fwd's ("extend the unit while it has <= 64 lanes"), in its bisection and chain form: xu_next finds a unit's end,
// xu_cut follows the chain. k_xdual_front (hank_xsweep.h) calls it with a thread per member and the column's start table in LDS;
// a CPU test compiles this header alone (tests/test_xunits_host.py). k_xunits_fwd keeps its own copy of the walk: calling this one
// there moved its instructions, and its code object stays what it was.
#pragma once

#if defined(__HIPCC__)
#define XU_FN __host__ __device__ __forceinline__
#else
#define XU_FN static inline
#endif

namespace hank {

constexpr int XU_ROWS = 63;         // target rows of a member (XRW, hank_xsweep.h) — and so the most units one column can have
constexpr int XU_LANES = 64;        // lanes of a unit: sources + virtual lanes

XU_FN int xu_min(int a, int b) { return a < b ? a : b; }
XU_FN int xu_max(int a, int b) { return a > b ? a : b; }

struct XuCut { int n, mlo, mhi, anyv; };      // units of the column, the members their sources belong to (from m on both sides), a unit has virtual lanes

// the encoding k_xfwd reads: {e | ja << 4 | cnt << 16, ta | tb << 8 | nv << 16}
XU_FN void xu_encode(int e, int ja, int cnt, int ta, int tb, int nv, int *x, int *y) {
    *x = e | (ja << 4) | (cnt << 16);
    *y = ta | (tb << 8) | (nv << 16);
}

// S(r): start[r] of the column for the absolute target row r in [0, n_a], any value clamped into [0, n_a] (a record that is not
// a lottery must not turn into a long walk or an out-of-range row).
// Sources of a unit that starts at relative row a and ends before b; has0: source row 0 would be its first lane and brings the virtual rows
template <typename S>
XU_FN int xu_lanes(S s, int clo, bool vnz, int r0, int a, int b, int *ja_out, bool *has0_out) {
    const int ja = s(r0 + a - 1 < 0 ? 0 : r0 + a - 1);
    *ja_out = ja;
    *has0_out = ja == 0 && clo <= 0 && vnz;
    return xu_max(s(r0 + b) - ja, 0);
}
// does the unit that starts with source ja (has0: and brings the virtual rows) still fit 64 lanes when it ends before relative row b?
template <typename S>
XU_FN bool xu_fits(S s, int ja, bool has0, int Sact, int r0, int b) {
    const int c2 = xu_max(s(r0 + b) - ja, 0);
    return c2 + ((has0 && c2 > 0) ? Sact : 0) <= XU_LANES;
}
// the end of the unit that STARTS at relative row a < nrows: the largest b in [a + 1, nrows] with every step up to it fitting 64
// lanes (the lane count is monotone in b: a bisection)
template <typename S>
XU_FN int xu_next(S s, int clo, bool vnz, int Sact, int r0, int nrows, int a) {
    int ja; bool has0;
    (void)xu_lanes(s, clo, vnz, r0, a, a + 1, &ja, &has0);
    auto fits = [&](int b) { return xu_fits(s, ja, has0, Sact, r0, b); };
    int lo = a + 1, hi = nrows;
    if (lo < hi && fits(lo + 1)) {
        if (fits(hi)) lo = hi;
        else {
            lo = lo + 1;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (fits(mid)) lo = mid; else hi = mid; }
        }
    }
    return lo;
}
// The cut of column e for member m (rows [r0, r0 + nrows)): next(ta) = xu_next(.., ta) however the caller has it (computed on the
// spot, or in advance); emit(k, x, y): unit k of the column, k < cap. Empty units (no source) are skipped, as
// k_xunits_fwd skips them. Every step advances by at least one row, so a column has at most nrows <= XU_ROWS units.
template <typename S, typename Next, typename Emit>
XU_FN XuCut xu_cut(S s, Next next, Emit emit, int clo, bool vnz, int r0, int nrows, int Sact, int e, int m, int cap) {
    XuCut q;
    q.n = 0; q.mlo = m; q.mhi = m; q.anyv = 0;
    int ta = 0;
    while (ta < nrows && q.n < cap) {
        const int tb = xu_min(xu_max(next(ta), ta + 1), nrows);
        int ja; bool has0;
        const int cnt = xu_lanes(s, clo, vnz, r0, ta, tb, &ja, &has0);
        const int nv = (has0 && cnt > 0) ? Sact : 0;
        if (cnt > 0) {
            int x, y;
            xu_encode(e, ja, cnt, ta, tb, nv, &x, &y);
            emit(q.n, x, y);
            q.mlo = xu_min(q.mlo, ja / XU_ROWS); q.mhi = xu_max(q.mhi, (ja + cnt - 1) / XU_ROWS);
            if (nv) q.anyv = 1;
            q.n++;
        }
        ta = tb;
    }
    return q;
}

// the serial form, for the host: start = the column's table [n_a + 1]; units: [cap][2]
static inline XuCut xu_cut_column(const int *start, int n_a, int clo, bool vnz, int r0, int nrows, int Sact, int e, int m, int *units, int cap) {
    auto s = [&](int r) { return xu_min(xu_max(start[xu_min(xu_max(r, 0), n_a)], 0), n_a); };
    auto next = [&](int ta) { return xu_next(s, clo, vnz, Sact, r0, nrows, ta); };
    auto emit = [&](int k, int x, int y) { units[2 * k] = x; units[2 * k + 1] = y; };
    return xu_cut(s, next, emit, clo, vnz, r0, nrows, Sact, e, m, cap);
}

}  // namespace hank
