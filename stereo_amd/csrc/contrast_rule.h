// The contrast rule of DESIGN.md 6.12 on the device, written once: the contrast of two pixels, max_c |im(a, c) - im(b, c)|,
// and the piecewise linear ramp.  Plain fp64 in the header's order (include/stereo_hip.h; -ffp-contract=off): the same
// bits as tests/contrast_restate.py.  Read by contrast.hip (weights of edges and scanline steps) and map_filter.hip
// (weights of a window's taps).
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "stereo_hip.h"

namespace stereo {

// one channel of g(a, b): `va`, `vb` are the two pixels' values in it; `ok` is cleared when the difference is not finite
__device__ __forceinline__ double contrast_channel(double g, double va, double vb, bool &ok) {
  const double d = fabs(va - vb);
  ok = ok && isfinite(d);
  return fmax(g, d);
}

// g(a, b) of an image in global memory
__device__ __forceinline__ double contrast(const double *__restrict__ im, int64_t N, int C, int64_t a, int64_t b, bool &ok) {
  double g = 0.0;
  for (int c = 0; c < C; ++c) g = contrast_channel(g, im[a + N * c], im[b + N * c], ok);
  return g;
}

__device__ __forceinline__ double ramp(double g, const stereo_contrast_params &p) {
  if (g <= p.g0) return p.w_high;
  if (g >= p.g1) return p.w_low;
  return p.w_high + (p.w_low - p.w_high) * ((g - p.g0) / (p.g1 - p.g0));
}

// The ramp's parameter rule, shared by every entry that takes a stereo_contrast_params: "" or what is wrong
inline const char *contrast_params_error(const stereo_contrast_params &p) {
  const double v[4] = {p.w_high, p.w_low, p.g0, p.g1};
  for (double x : v)
    if (!(x >= 0.0) || !std::isfinite(x)) return "w_high, w_low, g0 and g1 must be finite and non-negative";
  if (p.g0 > p.g1) return "g0 must not be above g1";
  return "";
}

}  // namespace stereo
