// What the two band builders share (band.hip: a band around a disparity map; plane_band.hip: a band around a
// plane map): the label-fastest element index, the launch sizes and the argument checks of the offsets and sizes.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "stereo_hip.h"

namespace stereo {
namespace band {

constexpr int kTB = 256;
constexpr int kMaxOffsets = 512;
constexpr unsigned kMaxGrid = 1u << 20;   // blocks of one launch; a block strides over what is left

// Element t = item * K + k of a K x M label-fastest array, for the 256 consecutive t of a block: the 64-bit
// division is done once per block on uniform values, a lane divides a number below 256 + K.
struct BandIndex {
  int64_t item;
  int k;
};
__device__ __forceinline__ BandIndex band_index(int64_t block_first, int K) {
  const int64_t item0 = block_first / K;
  const uint32_t local = (uint32_t)(block_first - item0 * K) + threadIdx.x;
  const uint32_t up = local / (uint32_t)K;
  return {item0 + up, (int)(local - up * (uint32_t)K)};
}

// ---------------------------------------------------------------- argument checks (no device call)

inline int check_offsets(const std::string &what, const double *offsets, int K, char *err, size_t errcap) {
  if (K < 1 || K > kMaxOffsets)
    return fail(what + ": the number of offsets must be 1 .. " + std::to_string(kMaxOffsets) + " (got " + std::to_string(K) + ")", err, errcap);
  if (!offsets) return fail(what + ": offsets must not be NULL", err, errcap);
  bool zero = false;
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(offsets[k])) return fail(what + ": offsets[" + std::to_string(k) + "] is not finite", err, errcap);
    if (k > 0 && !(offsets[k] > offsets[k - 1]))
      return fail(what + ": offsets must be strictly ascending (offsets[" + std::to_string(k) + "] <= offsets[" + std::to_string(k - 1) + "])", err, errcap);
    zero = zero || offsets[k] == 0.0;
  }
  if (!zero) return fail(what + ": offsets must contain 0.0 (the base labelling must be one of the band's)", err, errcap);
  return 0;
}

inline int check_sizes(const std::string &what, int H, int W, char *err, size_t errcap) {
  if (H < 1 || W < 1) return fail(what + ": H and W must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31)) return fail(what + ": H * W must be below 2^31", err, errcap);
  return 0;
}

template <class F>
int guarded(const char *what, char *err, size_t errcap, F f) {
  if (stereo_hip_device_count() < 1)
    return fail(std::string(what) + ": no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  try {
    f();
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  } catch (const std::exception &e) {
    return fail(std::string(what) + ": " + e.what(), err, errcap);
  }
}

inline unsigned grid_for(int64_t elements) {
  const int64_t b = (elements + kTB - 1) / kTB;
  return (unsigned)(b < 1 ? 1 : b > (int64_t)kMaxGrid ? (int64_t)kMaxGrid : b);
}

}  // namespace band
}  // namespace stereo
