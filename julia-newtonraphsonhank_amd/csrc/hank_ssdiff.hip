// hank_ssdiff.hip — the device code of hank_ss_jvp / hank_ss_vjp (hank_ssdiff.h) and its host launchers (hank_ssdiff_launch.h), in a
// translation unit of their own: the sweep kernels of hank_hip.hip are compiled exactly as before. It includes hank_device.h, not the
// headers that define kernels, so its code object holds the k_ss_* kernels and nothing else.
#include "hank_ssdiff.h"

namespace hank {

template <typename VT> static const VT *cv(const double *p) { return reinterpret_cast<const VT *>(p); }
template <typename VT> static VT *mv(double *p) { return reinterpret_cast<VT *>(p); }

void hankss_launch_in(hipStream_t s, const double *dxhh, int n_hh, int N, double *dxr, double *dxw, double *dxt) {
    hipLaunchKernelGGL(k_ss_in, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, s, dxhh, n_hh, N, dxr, dxw, dxt);
}

template <typename VT>
static void back(hipStream_t s, const Consts &c, const Record &R, const double *xhh, const double *dxr, const double *dxw, const double *dxt, const TanGeom &g, unsigned nbt,
                 unsigned ny, const double *dsIn, double *dsOut, double *dpol, double *dV, double *parts, const SsCtl *ctl) {
    hipLaunchKernelGGL((k_ss_back<2, VT>), dim3(nbt, ny), dim3(64 * c.n_e), 0, s, c, R, xhh, cv<VT>(dxr), cv<VT>(dxw), cv<VT>(dxt), g, cv<VT>(dsIn), mv<VT>(dsOut), mv<VT>(dpol),
                       mv<VT>(dV), mv<VT>(parts), ctl);
}
void hankss_launch_back(hipStream_t s, int V, const Consts &c, const Record &R, const double *xhh, const double *dxr, const double *dxw, const double *dxt, const TanGeom &g,
                    unsigned nbt, unsigned ny, const double *dsIn, double *dsOut, double *dpol, double *dV, double *parts, const SsCtl *ctl) {
    if (V == 2) back<double2>(s, c, R, xhh, dxr, dxw, dxt, g, nbt, ny, dsIn, dsOut, dpol, dV, parts, ctl);
    else back<double>(s, c, R, xhh, dxr, dxw, dxt, g, nbt, ny, dsIn, dsOut, dpol, dV, parts, ctl);
}

template <typename VT, int NX>
static void fwd(hipStream_t s, const Consts &c, const Record &R, const TanGeom &gf, unsigned nbf, unsigned ny, const double *dDin, double *dDout, const double *dpol,
                double *aggpart, const double *hxf, const double *hxfc, double *hxparts, double *parts, const SsCtl *ctl) {
    const dim3 grd(nbf, ny), blk(64 * c.n_e);
    TanHx<VT, NX> hx{};
    if constexpr (NX > 0) hx = TanHx<VT, NX>{hxf, hxfc, mv<VT>(hxparts)};
    if (gf.ss) hipLaunchKernelGGL((k_ss_fwd<2, VT, true, NX>), grd, blk, 0, s, c, R, gf, cv<VT>(dDin), mv<VT>(dDout), cv<VT>(dpol), mv<VT>(aggpart), hx, mv<VT>(parts), ctl);
    else hipLaunchKernelGGL((k_ss_fwd<1, VT, false, NX>), grd, blk, 0, s, c, R, gf, cv<VT>(dDin), mv<VT>(dDout), cv<VT>(dpol), mv<VT>(aggpart), hx, mv<VT>(parts), ctl);
}
template <typename VT>
static void fwd_nx(hipStream_t s, int NX, const Consts &c, const Record &R, const TanGeom &gf, unsigned nbf, unsigned ny, const double *dDin, double *dDout, const double *dpol,
                   double *aggpart, const double *hxf, const double *hxfc, double *hxparts, double *parts, const SsCtl *ctl) {
    if (NX == 2) fwd<VT, 2>(s, c, R, gf, nbf, ny, dDin, dDout, dpol, aggpart, hxf, hxfc, hxparts, parts, ctl);
    else if (NX == 1) fwd<VT, 1>(s, c, R, gf, nbf, ny, dDin, dDout, dpol, aggpart, hxf, hxfc, hxparts, parts, ctl);
    else fwd<VT, 0>(s, c, R, gf, nbf, ny, dDin, dDout, dpol, aggpart, hxf, hxfc, hxparts, parts, ctl);
}
void hankss_launch_fwd(hipStream_t s, int V, int NX, const Consts &c, const Record &R, const TanGeom &gf, unsigned nbf, unsigned ny, const double *dDin, double *dDout,
                   const double *dpol, double *aggpart, const double *hxf, const double *hxfc, double *hxparts, double *parts, const SsCtl *ctl) {
    if (V == 2) fwd_nx<double2>(s, NX, c, R, gf, nbf, ny, dDin, dDout, dpol, aggpart, hxf, hxfc, hxparts, parts, ctl);
    else fwd_nx<double>(s, NX, c, R, gf, nbf, ny, dDin, dDout, dpol, aggpart, hxf, hxfc, hxparts, parts, ctl);
}

void hankss_launch_check(hipStream_t s, const double *parts, int nb, int K, int N, double tol, SsCtl *ctl, double *sum_out) {
    hipLaunchKernelGGL(k_ss_check, dim3(1), dim3(256), 0, s, parts, nb, K, N, tol, ctl, sum_out);
}
void hankss_launch_check_dist(hipStream_t s, const Consts &c, const double *Dss, const double *parts, int nb, int N, double tol, double *dDnew, const double *dDold,
                          double *sig, SsCtl *ctl) {
    hipLaunchKernelGGL(k_ss_check_dist, dim3(1), dim3(1024), 0, s, c, Dss, parts, nb, N, tol, dDnew, dDold, sig, ctl);
}
void hankss_launch_jvp_out(hipStream_t s, int P, int n_hh, int n_het, int N, int nbf, const double *xhh, const double *dxhh, const double *agg, const double *zd,
                       const double *hxS, const double *aggpart, const double *hxparts, double *out) {
    hipLaunchKernelGGL(k_ss_jvp_out, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, P, n_hh, n_het, N, nbf, xhh, dxhh, agg, zd, hxS, aggpart, hxparts, out);
}
void hankss_launch_dist_out(hipStream_t s, const double *dD, int n_a, int n_e, int N, double *out) {
    hipLaunchKernelGGL(k_ss_dist_out, dim3((unsigned)(((size_t)n_a * n_e * N + 255) / 256)), dim3(256), 0, s, dD, n_a, n_e, N, out);
}
void hankss_launch_y_in(hipStream_t s, const double *agg_bar, int n_het, int M, double *yb) {
    hipLaunchKernelGGL(k_ss_y_in, dim3((unsigned)((4 * M + 255) / 256)), dim3(256), 0, s, agg_bar, n_het, M, yb);
}
void hankss_launch_cot_in(hipStream_t s, const Consts &c, const Record &R, const double *xhh, int NX, const double *yb, const double *Dbar, const double *hxf, size_t PG,
                      int M, double *e0, double *lam) {
    hipLaunchKernelGGL(k_ss_cot_in, dim3((unsigned)M), dim3(256), 0, s, c, R, xhh, NX, yb, Dbar, hxf, PG, M, e0, lam);
}

template <typename VT>
static void lam_v(hipStream_t s, bool pb, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const double *eIn, double *eOut, double *lam, double *parts,
                  const SsCtl *ctl, const double *cen, const double *yb, int NX, const double *hxfc, size_t PG, double *pbar) {
    const dim3 blk(64 * c.n_e), grd((unsigned)g.nb, (unsigned)((g.MV + g.NC - 1) / g.NC));
    if (pb) hipLaunchKernelGGL((k_ss_lam<VT, true>), grd, blk, lds, s, c, R, g, cv<VT>(eIn), mv<VT>(eOut), mv<VT>(lam), mv<VT>(parts), ctl, cv<VT>(cen), cv<VT>(yb), NX, hxfc, PG, mv<VT>(pbar));
    else hipLaunchKernelGGL((k_ss_lam<VT, false>), grd, blk, lds, s, c, R, g, cv<VT>(eIn), mv<VT>(eOut), mv<VT>(lam), mv<VT>(parts), ctl, cv<VT>(cen), cv<VT>(yb), NX, hxfc, PG, mv<VT>(pbar));
}
void hankss_launch_lam(hipStream_t s, int V, bool pb, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const double *eIn, double *eOut, double *lam,
                   double *parts, const SsCtl *ctl, const double *cen, const double *yb, int NX, const double *hxfc, size_t PG, double *pbar) {
    if (V == 2) lam_v<double2>(s, pb, lds, c, R, g, eIn, eOut, lam, parts, ctl, cen, yb, NX, hxfc, PG, pbar);
    else lam_v<double>(s, pb, lds, c, R, g, eIn, eOut, lam, parts, ctl, cen, yb, NX, hxfc, PG, pbar);
}

template <typename VT>
static void nu_v(hipStream_t s, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const int *sb, const double *nuIn, double *nuOut, const double *pbar,
                 const double *vbar, double *partS, double *partM, double *parts, const SsCtl *ctl) {
    const dim3 blk(64 * c.n_e), grd((unsigned)g.nb, (unsigned)((g.MV + g.NC - 1) / g.NC));
    hipLaunchKernelGGL((k_ss_nu<VT>), grd, blk, lds, s, c, R, g, sb, cv<VT>(nuIn), mv<VT>(nuOut), cv<VT>(pbar), cv<VT>(vbar), mv<VT>(partS), mv<VT>(partM), mv<VT>(parts), ctl);
}
void hankss_launch_nu(hipStream_t s, int V, size_t lds, const Consts &c, const Record &R, const AdjGeom &g, const int *sb, const double *nuIn, double *nuOut,
                  const double *pbar, const double *vbar, double *partS, double *partM, double *parts, const SsCtl *ctl) {
    if (V == 2) nu_v<double2>(s, lds, c, R, g, sb, nuIn, nuOut, pbar, vbar, partS, partM, parts, ctl);
    else nu_v<double>(s, lds, c, R, g, sb, nuIn, nuOut, pbar, vbar, partS, partM, parts, ctl);
}
void hankss_launch_xbar(hipStream_t s, int P, int n_hh, int M, int nb, int NX, const double *xhh, const double *partS, const double *partM, const double *yb,
                    const double *agg, const double *zd, const double *hxS, double *xhh_bar) {
    hipLaunchKernelGGL(k_ss_xbar, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, s, P, n_hh, M, nb, NX, xhh, partS, partM, yb, agg, zd, hxS, xhh_bar);
}

}  // namespace hank
