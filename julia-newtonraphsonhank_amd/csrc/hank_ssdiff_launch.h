// hank_ssdiff_launch.h — what hank_hip.hip sees of the steady-state derivative kernels (hank_ssdiff.h, compiled in hank_ssdiff.hip):
// one host launcher per kernel, ordinary functions of namespace hank on the argument structs of hank_device.h (the loops' control
// word SsCtl among them). V: columns per lane (2: double2 lanes, an even width; else 1).
#pragma once
#include "hank_device.h"

namespace hank {

void hankss_launch_in(hipStream_t s, const double *dxhh, int n_hh, int N, double *dxr, double *dxw, double *dxt);
void hankss_launch_back(hipStream_t s, int V, const Consts &c, const Record &R, const double *xhh, const double *dxr, const double *dxw, const double *dxt, const TanGeom &g,
                    unsigned nbt, unsigned ny, const double *dsIn, double *dsOut, double *dpol, double *dV, double *parts, const SsCtl *ctl);
// the forward step at the geometry build_tanwork picks for a width: the gather form with one row group (gf.ss == 0), the
// source-stationary form with two (gf.ss != 0); NX = 0, 1, 2 extra outputs with the record's f, f_c
void hankss_launch_fwd(hipStream_t s, int V, int NX, const Consts &c, const Record &R, const TanGeom &gf, unsigned nbf, unsigned ny, const double *dDin, double *dDout,
                   const double *dpol, double *aggpart, const double *hxf, const double *hxfc, double *hxparts, double *parts, const SsCtl *ctl);
void hankss_launch_check(hipStream_t s, const double *parts, int nb, int K, int N, double tol, SsCtl *ctl, double *sum_out);
void hankss_launch_check_dist(hipStream_t s, const Consts &c, const double *Dss, const double *parts, int nb, int N, double tol, double *dDnew, const double *dDold,
                          double *sig, SsCtl *ctl);
void hankss_launch_jvp_out(hipStream_t s, int P, int n_hh, int n_het, int N, int nbf, const double *xhh, const double *dxhh, const double *agg, const double *zd,
                       const double *hxS, const double *aggpart, const double *hxparts, double *out);
void hankss_launch_dist_out(hipStream_t s, const double *dD, int n_a, int n_e, int N, double *out);
void hankss_launch_y_in(hipStream_t s, const double *agg_bar, int n_het, int M, double *yb);
void hankss_launch_cot_in(hipStream_t s, const Consts &c, const Record &R, const double *xhh, int NX, const double *yb, const double *Dbar, const double *hxf, size_t PG,
                      int M, double *e0, double *lam);
// pb: the policy cotangent from the converged lam (eIn = lam) instead of one step; lds: adj_lds_dist of the geometry
void hankss_launch_lam(hipStream_t s, int V, bool pb, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const double *eIn, double *eOut, double *lam,
                   double *parts, const SsCtl *ctl, const double *cen, const double *yb, int NX, const double *hxfc, size_t PG, double *pbar);
void hankss_launch_nu(hipStream_t s, int V, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const int *sb, const double *nuIn, double *nuOut,
                  const double *pbar, const double *vbar, double *partS, double *partM, double *parts, const SsCtl *ctl);
void hankss_launch_xbar(hipStream_t s, int P, int n_hh, int M, int nb, int NX, const double *xhh, const double *partS, const double *partM, const double *yb,
                    const double *agg, const double *zd, const double *hxS, double *xhh_bar);

}  // namespace hank
