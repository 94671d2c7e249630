// hank_geom.h — plain C++ on integers, no device code: the lane geometry of the tangent kernels (hank_kernels.h) and of the transposed
// ones (hank_adjoint.h) at a batch width, for every host driver that launches them (build_tanwork, build_cotwork, ss_jvp, ss_vjp:
// hank_hip.hip). A CPU test compiles this header alone (tests/test_geom_host.py).
#pragma once

namespace hank {

struct TanGeom { int N, NC, lgNC, nbx, ss; };   // ss: source-stationary forward kernel (see tan_fwd_body)   // nbx = regular row blocks = ceil(n_a / (64/NC))

// N directions at V per lane (2: double2 lanes, N even): g.N lanes of directions, NC of them (a power of two <= 64) across a wave,
// RB = 64 / NC rows per wave instruction. ss = 0: the forward form is the caller's choice.
static inline TanGeom tan_geom(int n_a, int N, int V) {
    const int NV = N / V;
    int NC = 1, lg = 0;
    while (NC < NV && NC < 64) { NC <<= 1; lg++; }
    const int RB = 64 / NC;
    TanGeom g;
    g.N = NV; g.NC = NC; g.lgNC = lg; g.nbx = (n_a + RB - 1) / RB;
    g.ss = 0;
    return g;
}

// MV = M / (columns per lane); NC lanes of a wave span the columns (a power of two <= 16), RB = 64 / NC rows per wave
// instruction; a block owns R rows (R + 2 <= ADJ_KS * RB) x all n_e columns; nb = ceil(n_a / R) row blocks
struct AdjGeom { int MV, NC, lgNC, R, nb; };

// Lane geometry per batch width M: two adjacent cotangent columns per lane for an even M (16-byte state / pbar accesses); at
// most 16 lanes span the columns (wider batches take more blocks in y), so a wave instruction moves RB = 64 / NC >= 4 rows;
// a block owns R = max(RB, 8) rows: its LDS tile (n_e x (R + 2) x NC lanes) stays below 48 KiB up to n_e = 16.
static inline int adj_lane_width(int M) { return M % 2 == 0 ? 2 : 1; }
static inline AdjGeom adj_geom(int n_a, int M) {
    AdjGeom g;
    g.MV = M / adj_lane_width(M);
    g.NC = 1; g.lgNC = 0;
    while (g.NC < g.MV && g.NC < 16) { g.NC <<= 1; g.lgNC++; }
    const int RB = 64 / g.NC;
    g.R = RB > 8 ? RB : 8;
    g.nb = (n_a + g.R - 1) / g.R;
    return g;
}

}  // namespace hank
