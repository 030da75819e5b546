// The unary samplers (MI355X / gfx950) + their stateless C ABI.
//
// Device versions of
//   dispmap_ncc.m:107-115,222-276  parabola sampling of the NCC volume -> NCC unary
//   dispmap_ncc.m:208-221     winner-takes-all initial disparity
//   dispmap_globalstereo.m:336-345,355-375,405 + imrender/vgg/vgg_interp2.cxx:245-322
//                             photo-consistency unary (warp, bilinear gather, ephoto)
// All are independent per pixel: one thread each, coalesced along the column-major pixel index (MATLAB layout),
// images served from L2.  HBM-bound streaming kernels; no contraction (-ffp-contract=off) so that + - * / match numpy.
#include "gs_sample.h"
#include "ncc_sample.h"
#include "terms_host.h"

namespace stereo {
namespace {

// ---- NCC sampling (dispmap_ncc.m:222-276) -----------------------------------

__global__ __launch_bounds__(kTB) void ncc_unary_kernel(const double *ncc, int H, int W, int D, int layout,
                                                       const double *dv, double dmin, double dmax,
                                                       double unary_weight, const double *assign, double *U,
                                                       int ascending) {
  const int64_t px = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t Npx = (int64_t)H * W;
  if (px >= Npx) return;
  const double x = (double)(px / H + 1), y = (double)(px % H + 1);
  const double disp = plane_disp(assign + 4 * (size_t)px, x, y);
  U[px] = ncc_unary_at(ncc, Npx, D, layout, px, dv, dmin, dmax, unary_weight, disp, ascending);
}

__global__ __launch_bounds__(kTB) void ncc_best_disp_kernel(const double *ncc, int H, int W, int D, int layout,
                                                           const double *dv, double *best) {
  const int64_t px = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t Npx = (int64_t)H * W;
  if (px >= Npx) return;
  int t2 = 1;
  double y2 = vol(ncc, Npx, D, layout, px, 0);
  for (int i = 1; i < D; ++i) {
    const double v = vol(ncc, Npx, D, layout, px, i);
    if (v > y2) { y2 = v; t2 = i + 1; }  // max(...,[],3): first maximum
  }
  const bool ok = t2 < D && t2 > 1;
  double r, pp, q, d2;
  lagrange(ncc, Npx, D, layout, px, dv, t2, y2, ok, r, pp, q, d2);
  best[px] = ok ? -pp / r / 2 : d2;
}

// ---- globalstereo unary -------------------------------------------------------

__global__ __launch_bounds__(kTB) void globalstereo_unary_kernel(const double *im0, const double *im1, int H,
                                                                int W, int C, const double *P2 /*4x3 col major*/,
                                                                double d_min, double d_step, double col_thresh,
                                                                const double *assign, double *U) {
  const int64_t px = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t Npx = (int64_t)H * W;
  if (px >= Npx) return;
  const double x = (double)(px / H + 1), y = (double)(px % H + 1);
  U[px] = gs_unary_at(im0, im1, H, W, C, P2, d_min, d_step, col_thresh, px, x, y, plane_disp(assign + 4 * (size_t)px, x, y));
}
}  // namespace

void launch_ncc_unary(const double *ncc, int H, int W, int D, int layout, const double *dv, double dmin, double dmax,
                      double unary_weight, const double *assign, double *U, int ascending) {
  hipLaunchKernelGGL(ncc_unary_kernel, dim3(blocks((int64_t)H * W)), dim3(kTB), 0, 0, ncc, H, W, D, layout, dv, dmin, dmax,
                     unary_weight, assign, U, ascending);
}

void launch_ncc_best_disp(const double *ncc, int H, int W, int D, int layout, const double *dv, double *best) {
  hipLaunchKernelGGL(ncc_best_disp_kernel, dim3(blocks((int64_t)H * W)), dim3(kTB), 0, 0, ncc, H, W, D, layout, dv, best);
}

void launch_globalstereo_unary(const double *im0, const double *im1, int H, int W, int C, const double *P2, double d_min,
                               double d_step, double col_thresh, const double *assign, double *U) {
  hipLaunchKernelGGL(globalstereo_unary_kernel, dim3(blocks((int64_t)H * W)), dim3(kTB), 0, 0, im0, im1, H, W, C, P2, d_min,
                     d_step, col_thresh, assign, U);
}

}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_ncc_unary(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                     double unary_weight, const double *assignment, double *U, char *err, size_t errcap) {
  if (!ncc || !disparities || !assignment || !U || D < 1) return fail("stereo_ncc_unary: bad argument", err, errcap);
  return guarded_sync("stereo_ncc_unary", err, errcap, [&] {
    const size_t npx = (size_t)H * W;
    check_planes(assignment, npx);
    double dmin, dmax;
    disparity_range(disparities, D, dmin, dmax);
    DevBuf<double> dn, dd, da, out;
    dn.upload(ncc, npx * D); dd.upload(disparities, D); da.upload(assignment, 4 * npx); out.alloc(npx);
    launch_ncc_unary(dn.p, H, W, D, layout, dd.p, dmin, dmax, unary_weight, da.p, out.p,
                     strictly_ascending(disparities, D) ? 1 : 0);
    download(U, out, npx);
  });
}

int stereo_ncc_best_disp(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                         double *best, char *err, size_t errcap) {
  if (!ncc || !disparities || !best || D < 1) return fail("stereo_ncc_best_disp: bad argument", err, errcap);
  return guarded_sync("stereo_ncc_best_disp", err, errcap, [&] {
    const size_t npx = (size_t)H * W;
    DevBuf<double> dn, dd, out;
    dn.upload(ncc, npx * D); dd.upload(disparities, D); out.alloc(npx);
    launch_ncc_best_disp(dn.p, H, W, D, layout, dd.p, out.p);
    download(best, out, npx);
  });
}

int stereo_globalstereo_unary(const double *im0, const double *im1, int H, int W, int C, const double *P2,
                              double d_min, double d_step, double col_thresh, const double *assignment,
                              double *U, char *err, size_t errcap) {
  if (!im0 || !im1 || !P2 || !assignment || !U || C < 1) return fail("stereo_globalstereo_unary: bad argument", err, errcap);
  return guarded_sync("stereo_globalstereo_unary", err, errcap, [&] {
    const size_t npx = (size_t)H * W;
    check_planes(assignment, npx);
    DevBuf<double> d0, d1, dP, da, out;
    d0.upload(im0, npx * C); d1.upload(im1, npx * C); dP.upload(P2, 12); da.upload(assignment, 4 * npx);
    out.alloc(npx);
    launch_globalstereo_unary(d0.p, d1.p, H, W, C, dP.p, d_min, d_step, col_thresh, da.p, out.p);
    download(U, out, npx);
  });
}

}  // extern "C"
