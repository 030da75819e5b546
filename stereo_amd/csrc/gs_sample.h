// The photo-consistency unary of dispmap_globalstereo (dispmap_globalstereo.m:355-375, ephoto :405, and the
// 'linear' branch of imrender/vgg/vgg_interp2.cxx:245-322 with oobv = -1000) at one pixel, as a device
// function: one copy for every kernel that evaluates it at a plane's disparity (unary.hip:
// globalstereo_unary_kernel; plane_band.hip: plane_band_unary_kernel).  Compiled with -ffp-contract=off,
// so + - * / match numpy whichever kernel it is inlined into.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace stereo {

// px: the pixel, (x, y) = (px / H + 1, px % H + 1) its point; plane_d: the disparity of the pixel's plane at that
// point, before the rescaling.  P2: self.P(:,:,2), 4 x 3 column major, read at constant indices only (so a
// by-value kernel argument stays in scalar registers).
__device__ __forceinline__ double gs_unary_at(const double *im0, const double *im1, int H, int W, int C,
                                              const double *P2, double d_min, double d_step, double col_thresh,
                                              int64_t px, double x, double y, double plane_d) {
  const int64_t Npx = (int64_t)H * W;
  const double dhat = (plane_d - d_min) / d_step;
  const double disp = d_step * (dhat + d_min);  // dispmap_globalstereo.m:356 (sic)
  double T[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    T[k] = (x * P2[4 * k] + y * P2[4 * k + 1]) + (1.0 * P2[4 * k + 2] + disp * P2[4 * k + 3]);
  const double Nn = 1.0 / T[2];
  const double X = T[0] * Nn, Y = T[1] * Nn;
  const double oobv = -1000.0, dw = (double)W, dh = (double)H;
  double ssd = 0;
  for (int c = 0; c < C; ++c) {
    const double *A = im1 + (size_t)c * Npx;
    double o = oobv;
    if (X >= 1 && Y >= 1) {  // vgg_interp2.cxx:260-317
      if (X < dw) {
        if (Y < dh) {
          const int xi = (int)X, yi = (int)Y;
          const double u = X - xi, v = Y - yi;
          const size_t k = (size_t)H * (xi - 1) + yi - 1;
          o = A[k] + (A[k + H] - A[k]) * u;
          o += ((A[k + 1] - o) + (A[k + H + 1] - A[k + 1]) * u) * v;
        } else if (Y == dh) {
          const int xi = (int)X;
          const double u = X - xi;
          const size_t k = (size_t)H * xi - 1;
          o = A[k] + (A[k + H] - A[k]) * u;
        }
      } else if (X == dw) {
        if (Y < dh) {
          const int yi = (int)Y;
          const double v = Y - yi;
          const size_t k = (size_t)H * (W - 1) + yi - 1;
          o = A[k] + (A[k + 1] - A[k]) * v;
        } else if (Y == dh) {
          o = A[(size_t)H * W - 1];
        }
      }
    }
    const double m = o - im0[(size_t)c * Npx + px];
    ssd = ssd + m * m;
  }
  return log(2.0) - log(exp(ssd * (-1.0 / (col_thresh * C))) + 1.0);
}

}  // namespace stereo
