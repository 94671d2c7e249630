// hank_xspec.h — plain C++ on integers, no device code: which instance of the Dual pass's backward sweep (k_xdual_back<D, 768, NE,
// CRRA>, hank_xsweep.h) serves a context. beta, gamma, the grids and Pi are constructor arguments of a context and never change
// afterwards, so what the period loop would decide 299 times per sweep in every lane — how many productivity states the mixing
// runs over, which power CRRA's exponent is, whether the record diet is on — is decided once, here, and compiled in. A CPU test
// compiles this header alone (tests/test_xspec_host.py).
#pragma once
#include <string.h>

namespace hank {

// HANK_XSPEC (read at hank_create; anything else than these four words is the default): "1" = both halves, "0" = the generic instances, "ne" = NE only, "crra" = CRRA only — one library
// is its own A/B, and each half can be attributed. Unset = CRRA only: measured at 2000x11, T = 300, N = 32, the NE half showed no gain
// of its own and took back most of the CRRA half's, so it is off unless asked for.
enum { XSPEC_NE = 1, XSPEC_CRRA = 2 };
static inline int x_spec_mode(const char *env) {
    if (!env || !*env) return XSPEC_CRRA;
    if (strcmp(env, "0") == 0) return 0;
    if (strcmp(env, "ne") == 0) return XSPEC_NE;
    if (strcmp(env, "1") == 0) return XSPEC_NE | XSPEC_CRRA;
    return XSPEC_CRRA;
}

struct XSpec { int ne, crra; };      // the template arguments NE and CRRA; 0 = decided at run time
// NE: the grids BASELINE.md lists (4, 7, 11 productivity states); every other n_e keeps the run-time count.
// CRRA = 1: gamma = 2 with the record diet on (the calibration of examples/krusell_smith.yaml and of the one-asset HANK files);
// every other gamma, or a diet switched off (HANK_RECORD_DIET=0), keeps the generic powers.
static inline XSpec x_spec(int mode, int n_e, double gamma, int diet) {
    XSpec s;
    s.ne = (mode & XSPEC_NE) && (n_e == 4 || n_e == 7 || n_e == 11) ? n_e : 0;
    s.crra = (mode & XSPEC_CRRA) && gamma == 2.0 && diet != 0 ? 1 : 0;
    return s;
}

}  // namespace hank
