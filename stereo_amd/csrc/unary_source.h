// The two unary sources of the plane builders (plane_band.hip: a band around a plane map; plane_candidates.hip:
// per-pixel plane sets): the NCC sampler of dispmap_ncc (ncc_sample.h) and the photo-consistency term of
// dispmap_globalstereo (gs_sample.h), one copy of each, behind one interface.  begin(): what the block prepares
// once (the NCC source copies the D slice positions into LDS, for the reason band.hip gives); at(): the unary of
// pixel px, whose point is (x, y), for a plane whose disparity there is `disp`.  What the host works out before a
// launch with the NCC source (slice_range(), kMaxStagedSlices) is in band_common.h.
#pragma once
#include <cstdint>

#include "band_common.h"
#include "gs_sample.h"
#include "ncc_sample.h"

namespace stereo {
namespace band {

template <bool kStageSlices>
struct NccSource {
  const double *ncc;
  int D, layout;
  const double *dv;
  double dmin, dmax, unary_weight;
  int ascending;
  __device__ __forceinline__ const double *begin(double *lds) const {
    if (!kStageSlices) return dv;
    for (int i = threadIdx.x; i < D; i += kTB) lds[i] = dv[i];
    __syncthreads();
    return lds;
  }
  __device__ __forceinline__ double at(const double *slices, int H, int64_t Npx, int64_t px, double x, double y, double disp) const {
    return stereo::ncc_unary_at(ncc, Npx, D, layout, px, slices, dmin, dmax, unary_weight, disp, ascending);
  }
};
struct GsSource {
  const double *im0, *im1;
  int W, C;
  double P2[12];   // by value: read at constant indices, it stays in scalar registers
  double d_min, d_step, col_thresh;
  __device__ __forceinline__ const double *begin(double *) const { return nullptr; }
  __device__ __forceinline__ double at(const double *, int H, int64_t, int64_t px, double x, double y, double disp) const {
    return stereo::gs_unary_at(im0, im1, H, W, C, P2, d_min, d_step, col_thresh, px, x, y, disp);
  }
};

}  // namespace band
}  // namespace stereo
