// Tile constants of the staged NCC volume kernels (ncc_volume.hip) that the host path rule (ncc_rule.cpp) needs too.
// Plain constants, no HIP.
#pragma once

namespace stereo {

// ncc_cross_kernel
constexpr int kNccRows = 60;    // output rows per wave (64 lanes = 60 + 2 x 2 halo rows)
constexpr int kNccWaves = 8;    // disparities per workgroup (a 1024-thread workgroup would cap the wave at 128 VGPRs: spills)
constexpr int kNccCols = 32;    // columns per workgroup

// ncc_lane_kernel: a workgroup is 16 waves = 16 image rows, 12 output rows + the 2 + 2 rows the 5 x 5 window needs
constexpr int kNlWaves = 16;
constexpr int kNlRows = kNlWaves - 4;
// columns of the row segments it stages per wave: seg1 (right image) and seg0 (left image)
constexpr int kNlSeg1 = 96, kNlSeg0 = 36;

}  // namespace stereo
