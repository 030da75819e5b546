// Which kernel computes an NCC volume, and on what grid: the one place that decides it (host only, no HIP).
//
//   PerTap  ncc_volume_kernel: any patch size, any disparities
//   Cross   ncc_cross_kernel: 5 x 5 patch and every disparity an integer in [0, W) (what dispmap_ncc.m:24 always asks
//           for); lane = image row, either layout
//   Lanes   ncc_lane_kernel: the same and the label-fastest layout; lane = disparity.  It stages kNlSeg1 columns of the
//           right image per row: the disparities of every 64-label chunk must span less than that minus the
//           workgroup's own columns
// STEREO_HIP_NCC_NAIVE forces PerTap, STEREO_HIP_NCC_ROWLANES keeps Lanes out (ncc_volume.hip reads them).
#pragma once

namespace stereo {

enum class NccPath : int { PerTap = 0, Cross = 1, Lanes = 2 };

struct NccChoice {
  NccPath path = NccPath::PerTap;
  // Lanes only (0 otherwise): the largest max - min of a 64-label chunk, the columns per workgroup, and the column
  // chunks of the grid (row tiles x 64-label chunks x chunks)
  int span = 0, cols = 0, chunks = 0;
};

// h_disp: the D disparities, on the host; layout 0: H x W x D (MATLAB), 1: D x N label fastest; cus: compute units of
// the device; naive, rowlanes: the two switches
NccChoice ncc_rule(int H, int W, const double *h_disp, int D, int patchsize, int layout, int cus, bool naive, bool rowlanes);

}  // namespace stereo
