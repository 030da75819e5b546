// Image pyramid: the NCC volume of a coarser level as the 2 x 2 block mean of the finer volume,
// sampled at the finer disparities the coarser slices stand for.  No reference counterpart; the definition is in
// include/stereo_hip.h.
//
// One thread makes one output element; the lanes of a wave run along the output's fastest index.
//   layout 1 (D x N, label fastest; what the pair solve uses): a block takes 256 consecutive elements j + Kc pc of
//     the output and strides over the rest; its lanes read neighbouring slices of the same four volume columns,
//     which are the same cache lines.  The nearest slice of sample_at[j] depends on j alone: a block looks all Kc
//     of them up once, into LDS, before its first element.
//   layout 0 (H x W x D): the lanes run along yc as in pyramid_reduce_kernel, a block is `blockDim.x` rows of the
//     output columns (xc, j) it strides over, j outermost: j is uniform in a block, so its slice is looked up once
//     per j on the scalar unit and every slice base is a uniform 64-bit offset; a lane adds its 32-bit row.
// Every load is unconditional at a clamped address; only the stores are predicated.
#include <cmath>
#include <cstdint>
#include <string>

#include "band_common.h"
#include "common.h"
#include "ncc_sample.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::band::band_index;
using stereo::band::BandIndex;
using stereo::guarded;
using stereo::band::kTB;

// out = 0.25 (((v00 + v10) + v01) + v11): the sampler's value at the four fine pixels (rows y0, y1 of the columns
// x0, x1), the image reduction's order.
__device__ __forceinline__ double block_mean(const double *__restrict__ ncc, int H, int64_t Npx, int D, int layout,
                                             int y0, int y1, int x0, int x1, const double *__restrict__ dv, double dmin,
                                             double dmax, double disp, int t2) {
  const int c0 = H * x0, c1 = H * x1;   // (below 2^31: H * W is)
  const double v00 = stereo::ncc_value_at_slice(ncc, Npx, D, layout, c0 + y0, dv, dmin, dmax, disp, t2);
  const double v10 = stereo::ncc_value_at_slice(ncc, Npx, D, layout, c0 + y1, dv, dmin, dmax, disp, t2);
  const double v01 = stereo::ncc_value_at_slice(ncc, Npx, D, layout, c1 + y0, dv, dmin, dmax, disp, t2);
  const double v11 = stereo::ncc_value_at_slice(ncc, Npx, D, layout, c1 + y1, dv, dmin, dmax, disp, t2);
  return 0.25 * (((v00 + v10) + v01) + v11);
}

constexpr int kMaxStagedSamples = 8192;   // 32 KiB of LDS; beyond it every lane looks its own slice up

template <bool kStageSlices>
__global__ __launch_bounds__(kTB) void pyramid_volume_labels_kernel(const double *__restrict__ ncc, int H, int W, int D,
                                                                   int Hc, int Wc, const double *__restrict__ dv,
                                                                   double dmin, double dmax,
                                                                   const double *__restrict__ sample_at, int Kc,
                                                                   int ascending, double *__restrict__ out) {
  extern __shared__ int staged_slice[];
  if (kStageSlices) {
    for (int j = threadIdx.x; j < Kc; j += kTB) staged_slice[j] = stereo::ncc_nearest_slice(dv, D, sample_at[j], ascending);
    __syncthreads();
  }
  const int64_t Npx = (int64_t)H * W;
  const int Nc = Hc * Wc;
  const int64_t total = (int64_t)Nc * Kc;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, Kc);
    const bool live = ix.item < Nc;
    const int pc = live ? (int)ix.item : Nc - 1;
    const int xc = pc / Hc, yc = pc - xc * Hc;
    const int y0 = 2 * yc, x0 = 2 * xc;
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const double disp = sample_at[ix.k];
    const int t2 = kStageSlices ? staged_slice[ix.k] : stereo::ncc_nearest_slice(dv, D, disp, ascending);
    const double v = block_mean(ncc, H, Npx, D, 1, y0, y1, x0, x1, dv, dmin, dmax, disp, t2);
    if (live) out[first + threadIdx.x] = v;
  }
}

// (gridDim.y and gridDim.z stop at 65535: a block of a wider problem takes every gridDim-th column and slice.)
__global__ void pyramid_volume_slices_kernel(const double *__restrict__ ncc, int H, int W, int D, int Hc, int Wc,
                                             const double *__restrict__ dv, double dmin, double dmax,
                                             const double *__restrict__ sample_at, int Kc, int ascending,
                                             double *__restrict__ out) {
  const int yc = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = yc < Hc;
  const int y0 = 2 * (live ? yc : Hc - 1);       // 2 (Hc - 1) <= H - 1
  const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const int64_t Npx = (int64_t)H * W;
  for (int j = blockIdx.z; j < Kc; j += gridDim.z) {
    const double disp = sample_at[j];
    const int t2 = stereo::ncc_nearest_slice(dv, D, disp, ascending);
    for (int xc = blockIdx.y; xc < Wc; xc += gridDim.y) {
      const int x0 = 2 * xc;
      const int x1 = x0 + 1 < W ? x0 + 1 : W - 1;
      const double v = block_mean(ncc, H, Npx, D, 0, y0, y1, x0, x1, dv, dmin, dmax, disp, t2);
      if (live) out[(size_t)Hc * ((size_t)xc + (size_t)Wc * (size_t)j) + yc] = v;
    }
  }
}

// ---------------------------------------------------------------- arguments (no device call)

int check_args(const char *name, const void *ncc, int H, int W, int D, int layout, const double *disparities,
               const double *sample_at, int Kc, const void *out, char *err, size_t errcap) {
  const std::string what(name);
  if (H < 1 || W < 1 || D < 1 || Kc < 1) return fail(what + ": H, W, D and Kc must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(what + ": H * W must be below 2^31 (rows, columns and pixel counts are int32)", err, errcap);
  const int64_t Nc = (int64_t)((H + 1) / 2) * (int64_t)((W + 1) / 2);
  const int64_t most = ((int64_t)1 << 60) - 1;   // elements of 8 bytes whose byte count is below 2^63
  if (Nc > most / Kc) return fail(what + ": Hc * Wc * Kc must be below 2^63 / 8 (the output's bytes are counted in int64)", err, errcap);
  if ((int64_t)H * (int64_t)W > most / D) return fail(what + ": H * W * D must be below 2^63 / 8 (the volume's bytes are counted in int64)", err, errcap);
  if (layout != 0 && layout != 1) return fail(what + ": layout must be 0 (H x W x D) or 1 (D x N, label fastest)", err, errcap);
  if (!ncc || !disparities || !sample_at || !out)
    return fail(what + ": ncc, disparities, sample_at and out must not be NULL", err, errcap);
  if (out == ncc) return fail(what + ": out must not alias ncc (the reduction does not work in place)", err, errcap);
  for (int i = 0; i < D; ++i)
    if (!std::isfinite(disparities[i])) return fail(what + ": disparities[" + std::to_string(i) + "] is not finite", err, errcap);
  for (int j = 0; j < Kc; ++j)
    if (!std::isfinite(sample_at[j])) return fail(what + ": sample_at[" + std::to_string(j) + "] is not finite", err, errcap);
  return 0;
}

// `disparities`: the host vector (checked; min, max and the order of the slices come from it); `d_disparities` /
// `d_sample_at`: the two vectors in device memory, which the kernels read
void launch(const double *ncc, int H, int W, int D, int layout, const double *disparities, const double *d_disparities,
            const double *d_sample_at, int Kc, double *out, hipStream_t s) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  double dmin = disparities[0], dmax = disparities[0];
  bool ascending = true;
  for (int i = 1; i < D; ++i) {
    dmin = disparities[i] < dmin ? disparities[i] : dmin;
    dmax = disparities[i] > dmax ? disparities[i] : dmax;
    ascending = ascending && disparities[i] > disparities[i - 1];
  }
  if (layout == 1) {
    const int64_t chunks = ((int64_t)Hc * Wc * Kc + kTB - 1) / kTB;
    const unsigned blocks = (unsigned)(chunks < 2048 ? chunks : 2048);   // 8 per CU; a block strides over the rest
    if (Kc <= kMaxStagedSamples)
      hipLaunchKernelGGL(pyramid_volume_labels_kernel<true>, dim3(blocks), dim3(kTB), (size_t)Kc * sizeof(int), s, ncc, H, W, D,
                         Hc, Wc, d_disparities, dmin, dmax, d_sample_at, Kc, ascending ? 1 : 0, out);
    else
      hipLaunchKernelGGL(pyramid_volume_labels_kernel<false>, dim3(blocks), dim3(kTB), 0, s, ncc, H, W, D, Hc, Wc,
                         d_disparities, dmin, dmax, d_sample_at, Kc, ascending ? 1 : 0, out);
  } else {
    const int tb = Hc <= 64 ? 64 : 256;
    const dim3 grid((unsigned)((Hc + tb - 1) / tb), (unsigned)(Wc < 65535 ? Wc : 65535), (unsigned)(Kc < 65535 ? Kc : 65535));
    hipLaunchKernelGGL(pyramid_volume_slices_kernel, grid, dim3(tb), 0, s, ncc, H, W, D, Hc, Wc, d_disparities, dmin, dmax,
                       d_sample_at, Kc, ascending ? 1 : 0, out);
  }
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_pyramid_reduce_volume_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                        const double *d_disparities, const double *sample_at, const double *d_sample_at,
                                        int Kc, double *out, void *stream, char *err, size_t errcap) {
  const char *name = "stereo_pyramid_reduce_volume_device";
  if (int rc = check_args(name, ncc, H, W, D, layout, disparities, sample_at, Kc, out, err, errcap)) return rc;
  if (!d_disparities || !d_sample_at) return fail(std::string(name) + ": d_disparities and d_sample_at must not be NULL", err, errcap);
  return guarded(name, err, errcap,
                 [&] { launch(ncc, H, W, D, layout, disparities, d_disparities, d_sample_at, Kc, out, (hipStream_t)stream); });
}

int stereo_pyramid_reduce_volume(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                 const double *sample_at, int Kc, double *out, char *err, size_t errcap) {
  const char *name = "stereo_pyramid_reduce_volume";
  if (int rc = check_args(name, ncc, H, W, D, layout, disparities, sample_at, Kc, out, err, errcap)) return rc;
  return guarded(name, err, errcap, [&] {
    const size_t n = (size_t)H * W * D, nc = (size_t)((H + 1) / 2) * ((W + 1) / 2) * Kc;
    stereo::DevBuf<double> dn, dd, ds, o;
    dn.upload(ncc, n); dd.upload(disparities, D); ds.upload(sample_at, Kc); o.alloc(nc);
    launch(dn.p, H, W, D, layout, disparities, dd.p, ds.p, Kc, o.p, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, o.p, nc * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
