// The reduction of a summed scanline volume S (D x N, label fastest) to labels and confidence, and to a map where the
// labels have one shared positions vector: scanline_finish_kernel of scanline.hip, launched on `s` without waiting.
// map == NULL: positions is not read (scanline_edges.hip: positions are per edge there).  D <= 256.
#pragma once
#include <cstdint>

#include "common.h"

namespace stereo {

void scanline_finish(const double *S, const double *positions, int D, int64_t N, int32_t *labels, double *map,
                     double *confidence, hipStream_t s);

}  // namespace stereo
