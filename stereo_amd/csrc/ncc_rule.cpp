// The path rule of the NCC volume (ncc_rule.h) and its C entry for tests.
#include "ncc_rule.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/stereo_hip.h"
#include "ncc_geometry.h"

namespace stereo {

NccChoice ncc_rule(int H, int W, const double *h_disp, int D, int patchsize, int layout, int cus, bool naive, bool rowlanes) {
  NccChoice out;
  bool staged = patchsize == 2 && !naive;
  for (int i = 0; i < D && staged; ++i) staged = h_disp[i] >= 0 && h_disp[i] < W && h_disp[i] == std::floor(h_disp[i]);
  if (!staged) return out;
  out.path = NccPath::Cross;
  // (ncc_lane_kernel stages 96 columns of the right image per row: the disparities of every 64-label
  //  chunk must span less than that minus the workgroup's own columns)
  bool lanes_ok = layout == 1 && !rowlanes;
  int span = 0;
  for (int c0 = 0; c0 < D && lanes_ok; c0 += 64) {
    double lo = h_disp[c0], hi = h_disp[c0];
    for (int i = c0; i < std::min(D, c0 + 64); ++i) { lo = std::min(lo, h_disp[i]); hi = std::max(hi, h_disp[i]); }
    span = std::max(span, (int)(hi - lo));
  }
  lanes_ok = lanes_ok && span + 5 + 8 <= kNlSeg1;
  if (!lanes_ok) return out;
  // enough workgroups for every CU: the columns are cut so that row tiles x column chunks x 64-label
  // chunks reach ~2 workgroups per CU (each chunk re-computes four columns of products)
  const int rt = (H + kNlRows - 1) / kNlRows, dc = (D + 63) / 64;
  int chunks = std::max(1, (2 * cus + rt * dc - 1) / (rt * dc));
  int cols = std::max(8, (W + chunks - 1) / chunks);
  cols = std::min({cols, kNlSeg0 - 5, kNlSeg1 - 5 - span});   // what the staged segments hold (two columns per step: one more product column)
  chunks = (W + cols - 1) / cols;
  out.path = NccPath::Lanes;
  out.span = span; out.cols = cols; out.chunks = chunks;
  return out;
}

}  // namespace stereo

extern "C" int stereo_ncc_volume_rule(int H, int W, const double *disparities, int D, int patchsize, int layout, int cus,
                                      int naive, int rowlanes, int *path, int *cols, int *chunks, int *span, char *err,
                                      size_t errcap) {
  const bool bad = !disparities || H < 1 || W < 1 || D < 1 || patchsize < 0 || (layout != 0 && layout != 1) || cus < 1;
  if (err && errcap) {
    std::strncpy(err, bad ? "stereo_ncc_volume_rule: bad argument" : "", errcap - 1);
    err[errcap - 1] = 0;
  }
  if (bad) return 1;
  const stereo::NccChoice c = stereo::ncc_rule(H, W, disparities, D, patchsize, layout, cus, naive != 0, rowlanes != 0);
  if (path) *path = (int)c.path;
  if (cols) *cols = c.cols;
  if (chunks) *chunks = c.chunks;
  if (span) *span = c.span;
  return 0;
}
