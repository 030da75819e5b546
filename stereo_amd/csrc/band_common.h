// What the four level builders share (band.hip: a band around a disparity map; plane_band.hip: a band around a plane
// map; candidates.hip and plane_candidates.hip: per-pixel label / plane sets), one copy of each: the label-fastest
// element index, the clamp of a tap, the launch sizes, what the host reads off the slice positions, every argument
// check and scan, and the device buffers of a host entry's outputs.  The index prologue of the positions kernels is
// not here: shared, it changed their instruction order.
// (carry.hip and pyramid_volume.hip take the index and the launch sizes from here.)
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
constexpr int kMaxStagedSlices = 4096;    // 32 KiB of LDS; beyond it a unary kernel reads the slices where they are
constexpr int kMaxTap = 1 << 15;          // |dy|, |dx| below it: a tap never needs more than the int32 it is stored in

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

// The pixel a gather kernel reads for tap t at pixel `item` of a column-major H x W map: (y + dy_t, x + dx_t)
// clamped to the image.
__device__ __forceinline__ int64_t tapped_pixel(int64_t item, int H, int W, const int32_t *__restrict__ taps, int t) {
  const uint32_t px = (uint32_t)item, x = px / (uint32_t)H, y = px - x * (uint32_t)H;
  int64_t ys = (int64_t)y + taps[2 * t], xs = (int64_t)x + taps[2 * t + 1];
  ys = ys < 0 ? 0 : ys > H - 1 ? H - 1 : ys;
  xs = xs < 0 ? 0 : xs > W - 1 ? W - 1 : xs;
  return xs * H + ys;
}

// what the host reads off the slice positions before a launch that samples the NCC volume
struct SliceRange {
  double dmin, dmax;
  int ascending;
};
inline SliceRange slice_range(const double *disparities, int D) {
  double dmin = disparities[0], dmax = disparities[0];
  bool ascending = disparities[0] == disparities[0];
  for (int i = 1; i < D; ++i) {
    dmin = disparities[i] < dmin ? disparities[i] : dmin;
    dmax = disparities[i] > dmax ? disparities[i] : dmax;
    ascending = ascending && disparities[i] > disparities[i - 1];
  }
  return {dmin, dmax, ascending ? 1 : 0};
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

inline int check_k(const std::string &what, int K, char *err, size_t errcap) {
  if (K < 1 || K > kMaxOffsets)
    return fail(what + ": the number of candidates K must be 1 .. " + std::to_string(kMaxOffsets) + " (got " + std::to_string(K) + ")", err, errcap);
  return 0;
}

// the NCC volume of a unary
inline int check_volume(const std::string &what, const void *ncc, int D, int layout, const void *disparities, char *err,
                        size_t errcap) {
  if (D < 1) return fail(what + ": D must be at least 1", err, errcap);
  if (layout != 0 && layout != 1) return fail(what + ": layout must be 0 (H x W x D) or 1 (D x N, label fastest)", err, errcap);
  if (!ncc || !disparities) return fail(what + ": ncc and disparities must not be NULL", err, errcap);
  return 0;
}

// the images of the photo-consistency unary
inline int check_gs(const std::string &what, const void *im0, const void *im1, int C, const void *P2, double d_step, char *err,
                    size_t errcap) {
  if (C < 1) return fail(what + ": C must be at least 1", err, errcap);
  if (!im0 || !im1 || !P2) return fail(what + ": im0, im1 and P2 must not be NULL", err, errcap);
  if (d_step == 0) return fail(what + ": d_step must not be 0 (the photo-consistency unary divides by it)", err, errcap);
  return 0;
}

inline int check_edges(const std::string &what, int64_t E, const void *conn, const void *q, const void *qprim, char *err,
                       size_t errcap) {
  if (E < 0) return fail(what + ": E must not be negative", err, errcap);
  if (E > 0 && (!conn || !q || !qprim)) return fail(what + ": conn, q and qprim must not be NULL", err, errcap);
  return 0;
}

// `own` / `table`: the names of the two arrays ("base" and "cand", "planes" and "pcand")
inline int check_gather(const std::string &what, const char *own, const char *table, const void *own_p, int H, int W,
                        const double *offsets, int Ko, const void *sources, int M, const int32_t *taps, int T,
                        const void *table_p, char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (M < 0 || T < 0) return fail(what + ": M and T must not be negative", err, errcap);
  if (!own_p || !table_p) return fail(what + ": " + own + " and " + table + " must not be NULL", err, errcap);
  if (int rc = check_offsets(what, offsets, Ko, err, errcap)) return rc;
  const int64_t K = (int64_t)Ko + (int64_t)M * T;
  if (K > kMaxOffsets)
    return fail(what + ": the number of candidates K = Ko + M * T must be 1 .. " + std::to_string(kMaxOffsets) + " (got " + std::to_string(K) + ")", err, errcap);
  if ((int64_t)M * T > 0) {
    if (!sources || !taps) return fail(what + ": sources and taps must not be NULL when M * T > 0", err, errcap);
    for (int t = 0; t < 2 * T; ++t)
      if (taps[t] <= -kMaxTap || taps[t] >= kMaxTap)
        return fail(what + ": tap " + std::to_string(t / 2) + " has |dy| or |dx| of 2^15 or more", err, errcap);
  }
  return 0;
}

// ---------------------------------------------------------------- scans of a host entry's arrays

inline int check_conn(const std::string &what, const uint32_t *conn, int64_t E, size_t n, char *err, size_t errcap) {
  for (int64_t e = 0; e < 2 * E; ++e)
    if (conn[e] >= n) return fail(what + ": conn names a pixel outside 0 .. H*W - 1 (edge " + std::to_string(e / 2) + ")", err, errcap);
  return 0;
}

inline int check_labels(const std::string &what, const int32_t *labels, size_t n, int K, char *err, size_t errcap) {
  for (size_t i = 0; i < n; ++i)
    if (labels[i] < 1 || labels[i] > K)
      return fail(what + ": label " + std::to_string(labels[i]) + " at pixel " + std::to_string(i) + " is outside 1 .. " + std::to_string(K), err, errcap);
  return 0;
}

// Element t of an array with K entries per pixel (K == 0: one entry per pixel and no label to name), pixels column
// major in an image of H rows (H == 0: the pixel is named by its index).
inline std::string pixel_name(int64_t t, int H, int K = 0) {
  const int64_t i = K > 0 ? t / K : t;
  const std::string pixel = H > 0 ? "pixel (row " + std::to_string(i % H) + ", column " + std::to_string(i / H) + ")"
                                  : "pixel " + std::to_string(i);
  return K > 0 ? pixel + ", label " + std::to_string(t % K + 1) : pixel;
}

// every value of `map` (`name`: "base", "source m", "cand") is finite
inline int check_finite(const std::string &what, const std::string &name, const double *map, int64_t N, int H, int K, char *err,
                        size_t errcap) {
  for (int64_t t = 0; t < N * (K > 0 ? K : 1); ++t)
    if (!std::isfinite(map[t])) return fail(what + ": " + name + " is not finite at " + pixel_name(t, H, K), err, errcap);
  return 0;
}

// every plane of `planes` is finite and has c != 0; `name`: "planes", "source m", "pcand", or "" for the plain plane
// array of the plane band, whose messages do not name it
inline int check_planes(const std::string &what, const std::string &name, const double *planes, int64_t N, int H, int K,
                        char *err, size_t errcap) {
  for (int64_t t = 0; t < N * (K > 0 ? K : 1); ++t) {
    const double *p = planes + 4 * t;
    const bool finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
    if (finite && p[2] != 0) continue;
    const std::string subject = finite ? ": Infinite disparity (c == 0) " + (name.empty() ? "" : "in " + name + " ") + "at "
                                       : ": " + (name.empty() ? "a plane" : name) + " is not finite at ";
    return fail(what + subject + pixel_name(t, H, K), err, errcap);
  }
  return 0;
}

inline unsigned grid_for(int64_t elements) {
  const int64_t b = (elements + kTB - 1) / kTB;
  return (unsigned)(b < 1 ? 1 : b > (int64_t)kMaxGrid ? (int64_t)kMaxGrid : b);
}

// the edge list and the three outputs of a host inputs entry: on the device, the outputs fetched after the launches
struct HostOutputs {
  DevBuf<double> du, dq, dqp;
  DevBuf<uint32_t> dc;
  size_t nu, ne;
  HostOutputs(size_t n, int K, int64_t E, const uint32_t *conn) : nu(n * K), ne((size_t)E * K) {
    du.alloc(nu);
    if (E > 0) { dc.upload(conn, 2 * (size_t)E); dq.alloc(ne); dqp.alloc(ne); }
  }
  void fetch(double *unary, double *q, double *qprim) {
    STEREO_HIP_CHECK(hipMemcpy(unary, du.p, nu * sizeof(double), hipMemcpyDeviceToHost));
    if (ne > 0) {
      STEREO_HIP_CHECK(hipMemcpy(q, dq.p, ne * sizeof(double), hipMemcpyDeviceToHost));
      STEREO_HIP_CHECK(hipMemcpy(qprim, dqp.p, ne * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
};

}  // namespace band
}  // namespace stereo
