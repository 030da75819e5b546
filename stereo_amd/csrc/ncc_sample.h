// The NCC sampler (dispmap_ncc.m:222-276) and the plane -> disparity rule (dispmap_super.m:318-328) as
// device functions: one copy for every kernel that evaluates the volume at a real disparity
// (unary.hip: ncc_unary_kernel, ncc_best_disp_kernel; band.hip: band_unary_kernel; plane_band.hip:
// plane_band_unary_kernel; pyramid_volume.hip: the two reduce_volume kernels).  Compiled with
// -ffp-contract=off, so + - * / match numpy whichever kernel they are inlined into.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace stereo {

__device__ __forceinline__ double plane_disp(const double *pl, double x, double y) {
  // -(sum(assignment(1:2,:).*points) + assignment(4,:)) ./ assignment(3,:)
  const double s = pl[0] * x + pl[1] * y;
  return -(s + pl[3]) / pl[2];
}

__device__ __forceinline__ double vol(const double *ncc, int64_t Npx, int D, int layout, int64_t px, int k) {
  return layout == 0 ? ncc[(size_t)k * Npx + px] : ncc[(size_t)px * D + k];
}

__device__ __forceinline__ void lagrange(const double *ncc, int64_t Npx, int D, int layout, int64_t px,
                                         const double *dv, int t2 /*1-based*/, double y2, bool ok, double &r,
                                         double &pp, double &q, double &d2) {
  const int t1 = ok ? t2 - 1 : t2, t3 = ok ? t2 + 1 : t2;
  const double d1 = dv[t1 - 1], d3 = dv[t3 - 1];
  d2 = dv[t2 - 1];
  const double y1 = vol(ncc, Npx, D, layout, px, t1 - 1), y3 = vol(ncc, Npx, D, layout, px, t3 - 1);
  const double a = y1 / (d1 - d2) / (d1 - d3);
  const double b = y2 / (d2 - d1) / (d2 - d3);
  const double c = y3 / (d3 - d1) / (d3 - d2);
  r = a + b + c;
  pp = -(a * (d2 + d3) + b * (d1 + d3) + c * (d1 + d2));
  q = a * d2 * d3 + b * d1 * d3 + c * d1 * d2;
}

// The nearest slice of `disp`, one based, ties to the LARGER index (dispmap_ncc.m:230-236: a scan over all
// slices with "<="; the index keeps its initial 1 if no comparison succeeds, i.e. for a NaN disparity).  It depends on
// the disparity and the slices alone, not on the pixel: a kernel whose lanes share a disparity looks it up once
// (pyramid_volume.hip).  ascending: dv is strictly ascending (the host checked).
__device__ __forceinline__ int ncc_nearest_slice(const double *dv, int D, double disp, int ascending) {
  int t2 = 1;
  if (ascending) {
    // strictly ascending samples: |disp - dv[i]| falls, then rises (rounding is monotone), so the
    // scan's answer is the later of the two samples around disp -- found by bisection -- unless
    // further samples tie with it after rounding, which the short forward walk covers
    if (disp == disp) {
      int lo = 0, hi = D;  // first index with dv[i] > disp
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (dv[mid] > disp) hi = mid; else lo = mid + 1; }
      int j = lo > 0 ? lo - 1 : 0;
      double best = fabs(disp - dv[j]);
      // (an earlier sample can tie with j only after rounding; the scan would still end on j or later)
      while (j + 1 < D && fabs(disp - dv[j + 1]) <= best) { ++j; best = fabs(disp - dv[j]); }
      t2 = j + 1;
    }
  } else {
    double smallest = fabs(disp - dv[0]);
    for (int i = 0; i < D; ++i) {
      const double nd = fabs(disp - dv[i]);
      if (nd <= smallest) { t2 = i + 1; smallest = nd; }
    }
  }
  return t2;
}

// sample_ncc_from_disp(disp) at pixel px, given the nearest slice t2 of disp (dispmap_ncc.m:237-249): the parabola
// through the slice and its two neighbours, the slice itself at the first and the last one, -1e6 outside the range.
// dmin / dmax: the smallest and largest of dv.  (For a NaN disparity t2 is 1 and the scan's y2 stays 1; what the
// parabola gives is then replaced twice over, so the slice's value stands in for it here.)
__device__ __forceinline__ double ncc_value_at_slice(const double *ncc, int64_t Npx, int D, int layout, int64_t px,
                                                     const double *dv, double dmin, double dmax, double disp, int t2) {
  const double y2 = vol(ncc, Npx, D, layout, px, t2 - 1);
  const bool ok = t2 < D && t2 > 1;
  double r, pp, q, d2;
  lagrange(ncc, Npx, D, layout, px, dv, t2, y2, ok, r, pp, q, d2);
  double v = r * (disp * disp) + pp * disp + q;
  if (t2 == 1) v = vol(ncc, Npx, D, layout, px, 0);
  if (t2 == D) v = vol(ncc, Npx, D, layout, px, D - 1);
  if (!(disp <= dmax && disp >= dmin)) v = -1e6;
  return v;
}

// sample_ncc_from_disp(disp) at pixel px (dispmap_ncc.m:222-249).
__device__ __forceinline__ double ncc_value_at(const double *ncc, int64_t Npx, int D, int layout, int64_t px,
                                               const double *dv, double dmin, double dmax, double disp, int ascending) {
  return ncc_value_at_slice(ncc, Npx, D, layout, px, dv, dmin, dmax, disp, ncc_nearest_slice(dv, D, disp, ascending));
}

// unary_weight * (1 - sample_ncc_from_disp(disp)) at pixel px (dispmap_ncc.m:107-115).
__device__ __forceinline__ double ncc_unary_at(const double *ncc, int64_t Npx, int D, int layout, int64_t px,
                                               const double *dv, double dmin, double dmax, double unary_weight,
                                               double disp, int ascending) {
  return unary_weight * (1 - ncc_value_at(ncc, Npx, D, layout, px, dv, dmin, dmax, disp, ascending));
}

}  // namespace stereo
