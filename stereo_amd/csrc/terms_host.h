// What the term builders share on the host (pairwise.hip, ncc_volume.hip, unary.hip, fusion.hip): the block size of
// their one-thread-per-element kernels, the scans of a caller's arrays, the copy back, the host clock, and the
// launchers of the kernels that the fusion context (fusion.hip) runs on its resident state.  Includes common.h, and
// with it the HIP runtime and the C ABI (stereo_hip.h).  A launcher takes the
// kernel's arguments, computes the grid and launches on the null stream; it is defined next to its kernel.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <stdexcept>

#include "common.h"

namespace stereo {

constexpr int kTB = 256;

inline unsigned blocks(int64_t n) { return (unsigned)((n + kTB - 1) / kTB); }

inline void check_planes(const double *pl, int64_t M) {
  for (int64_t i = 0; i < M; ++i)
    if (pl[4 * i + 2] == 0) throw std::runtime_error("Infinite disparity");  // dispmap_super.m:323-325
}

template <class T>
void download(T *dst, const DevBuf<T> &b, size_t n) {
  STEREO_HIP_CHECK(hipMemcpy(dst, b.p, n * sizeof(T), hipMemcpyDeviceToHost));
}

inline bool strictly_ascending(const double *d, int D) {
  for (int i = 0; i < D; ++i)
    if (!(d[i] == d[i]) || (i > 0 && !(d[i] > d[i - 1]))) return false;
  return true;
}

// smallest and largest of the D >= 1 sample positions of an NCC volume (what its sampler clamps to)
inline void disparity_range(const double *disparities, int D, double &dmin, double &dmax) {
  dmin = dmax = disparities[0];
  for (int i = 1; i < D; ++i) { dmin = std::min(dmin, disparities[i]); dmax = std::max(dmax, disparities[i]); }
}

inline double wall_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// pairwise.hip
void launch_pairwise_terms(int kernel, int64_t E, const uint32_t *conn, const double *points, const double *cur,
                           const double *prop, const double *w, double tol, double d_min, double d_step, double *E00,
                           double *E01, double *E10, double *E11);
void launch_trws_positions(int64_t E, int K, int64_t N, const uint32_t *conn, const double *points, const double *props,
                           double d_min, double d_step, double *q, double *qprim);
// unary.hip
void launch_ncc_unary(const double *ncc, int H, int W, int D, int layout, const double *dv, double dmin, double dmax,
                      double unary_weight, const double *assign, double *U, int ascending);
void launch_ncc_best_disp(const double *ncc, int H, int W, int D, int layout, const double *dv, double *best);
void launch_globalstereo_unary(const double *im0, const double *im1, int H, int W, int C, const double *P2, double d_min,
                               double d_step, double col_thresh, const double *assign, double *U);

}  // namespace stereo
