// Image pyramid: the 2 x 2 box reduction of an image and the expansion of a coarse
// disparity map to the next finer scale.  No reference counterpart.
//
// Images are H x W x C and maps H x W, column major: element (y, x, c) at y + H (x + W c).  In both
// kernels one thread makes one output element, the lanes of a wave run along y (consecutive addresses
// on every load and store), a block is `blockDim.x` consecutive rows of one output column, the grid is
// (y-tile, column).  Every load is unconditional at a clamped address; only the stores are predicated.
// The 64-bit index arithmetic is on the block's column, which is uniform; a lane adds its 32-bit row.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "common.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::HipError;

// ---------------------------------------------------------------- reduce
//
// out(yc, xc, c) = 0.25 (((a00 + a10) + a01) + a11), a_ij = im(min(2 yc + i, H - 1), min(2 xc + j, W - 1), c).
// A column of the grid is j = xc + Wc c, so the output element is at yc + Hc j.
// (gridDim.y stops at 65535: a block of a wider image takes every gridDim.y-th column.)
__global__ void pyramid_reduce_kernel(const double *__restrict__ im, int H, int W, int C, int Hc, int Wc,
                                      double *__restrict__ out) {
  const int yc = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = yc < Hc;
  const int y0 = 2 * (live ? yc : Hc - 1);       // 2 (Hc - 1) <= H - 1
  const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const int64_t columns = (int64_t)Wc * C;
  for (int64_t j = blockIdx.y; j < columns; j += gridDim.y) {
    const int c = (int)(j / Wc);
    const int xc = (int)(j - (int64_t)c * Wc);
    const int x0 = 2 * xc;
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const double *__restrict__ p0 = im + (size_t)H * ((size_t)x0 + (size_t)W * c);
    const double *__restrict__ p1 = im + (size_t)H * ((size_t)x1 + (size_t)W * c);
    const double a00 = p0[y0], a10 = p0[y1], a01 = p1[y0], a11 = p1[y1];
    if (live) out[(size_t)Hc * (size_t)j + yc] = 0.25 * (((a00 + a10) + a01) + a11);
  }
}

// ---------------------------------------------------------------- expand
//
// Fine pixel (y, x): parent (yc, xc) = (y >> 1, x >> 1); ny = yc + 1 for an odd y, yc - 1 for an even one, clamped to
// 0 .. Hc - 1, nx the same from x and Wc.  Candidates 0: (yc, xc), 1: (ny, xc), 2: (yc, nx), 3: (ny, nx).
// Guided = false: out = 2 d_coarse(candidate 0), source 0.  Guided = true: among the candidates with a finite
// disparity, the first one whose squared colour distance to the fine pixel no later one undercuts.
__device__ inline int neighbour(int v, int vc, int nc) {
  const int n = (v & 1) ? vc + 1 : vc - 1;
  return n < 0 ? 0 : n > nc - 1 ? nc - 1 : n;
}

template <bool Guided>
__global__ void pyramid_expand_kernel(const double *__restrict__ d_coarse, int Hc, int Wc, int H, int W,
                                      const double *__restrict__ im_fine, const double *__restrict__ im_coarse, int C,
                                      double *__restrict__ out, int32_t *__restrict__ source) {
  const int yt = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = yt < H;
  const int y = live ? yt : H - 1;
  const int yc = y >> 1;
  const int ny = neighbour(y, yc, Hc);
  const size_t fine_plane = (size_t)H * W, coarse_plane = (size_t)Hc * Wc;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t x = blockIdx.y; x < W; x += gridDim.y) {
    const int xc = (int)x >> 1;
    const size_t col = (size_t)Hc * xc;
    double *__restrict__ o = out + (size_t)H * (size_t)x;
    if (!Guided) {
      const double d = d_coarse[col + yc];
      if (live) {
        o[y] = 2.0 * d;
        if (source) source[(size_t)H * (size_t)x + y] = 0;
      }
      continue;
    }
    const size_t ncol = (size_t)Hc * neighbour((int)x, xc, Wc);
    const double d[4] = {d_coarse[col + yc], d_coarse[col + ny], d_coarse[ncol + yc], d_coarse[ncol + ny]};
    double dist[4] = {0.0, 0.0, 0.0, 0.0};
    const double *__restrict__ f = im_fine + (size_t)H * (size_t)x;
    const double *__restrict__ g0 = im_coarse + col;
    const double *__restrict__ g1 = im_coarse + ncol;
    for (int c = 0; c < C; ++c) {
      const double v = f[y];
      const double e0 = v - g0[yc], e1 = v - g0[ny], e2 = v - g1[yc], e3 = v - g1[ny];
      dist[0] = dist[0] + e0 * e0;
      dist[1] = dist[1] + e1 * e1;
      dist[2] = dist[2] + e2 * e2;
      dist[3] = dist[3] + e3 * e3;
      f += fine_plane;
      g0 += coarse_plane;
      g1 += coarse_plane;
    }
    int32_t best = -1;
    double best_dist = nan, best_d = nan;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool take = isfinite(d[k]) && (best < 0 || dist[k] < best_dist);
      best = take ? k : best;
      best_dist = take ? dist[k] : best_dist;
      best_d = take ? d[k] : best_d;
    }
    if (live) {
      o[y] = best >= 0 ? 2.0 * best_d : nan;
      if (source) source[(size_t)H * (size_t)x + y] = best;
    }
  }
}

// ---------------------------------------------------------------- arguments

int check_sizes(const std::string &what, int H, int W, int C, char *err, size_t errcap) {
  if (H < 1 || W < 1 || C < 1) return fail(what + ": H, W and C must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(what + ": H * W must be below 2^31 (rows, columns and pixel counts are int32)", err, errcap);
  return 0;
}

int reduce_args(const char *name, const void *im, int H, int W, int C, const void *out, char *err, size_t errcap) {
  const std::string what(name);
  if (!im || !out) return fail(what + ": im and out must not be NULL", err, errcap);
  if (out == im) return fail(what + ": out must not alias im (the reduction does not work in place)", err, errcap);
  return check_sizes(what, H, W, C, err, errcap);
}

int expand_args(const char *name, const void *d_coarse, int Hc, int Wc, int H, int W, int mode, const void *im_fine,
                const void *im_coarse, int C, const void *out, const void *source, char *err, size_t errcap) {
  const std::string what(name);
  if (mode != 0 && mode != 1) return fail(what + ": mode must be 0 (nearest) or 1 (guided)", err, errcap);
  if (!d_coarse || !out) return fail(what + ": d_coarse and out must not be NULL", err, errcap);
  if (mode == 1 && (!im_fine || !im_coarse))
    return fail(what + ": im_fine and im_coarse must not be NULL in mode 1", err, errcap);
  if (int rc = check_sizes(what, H, W, C, err, errcap)) return rc;
  if (Hc != (H + 1) / 2 || Wc != (W + 1) / 2)
    return fail(what + ": coarse and fine sizes do not match (Hc = (H + 1) / 2 and Wc = (W + 1) / 2 are required)", err,
                errcap);
  if (out == d_coarse || (mode == 1 && (out == im_fine || out == im_coarse)))
    return fail(what + ": out must not alias an input", err, errcap);
  if (source && (source == d_coarse || source == out || (mode == 1 && (source == im_fine || source == im_coarse))))
    return fail(what + ": source must not alias an input or out", err, errcap);
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

dim3 grid_for(int rows, int64_t columns, int tb) {
  return dim3((unsigned)((rows + tb - 1) / tb), (unsigned)(columns < 65535 ? columns : 65535));
}

void launch_reduce(const double *im, int H, int W, int C, double *out, hipStream_t s) {
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int tb = Hc <= 64 ? 64 : 256;
  hipLaunchKernelGGL(pyramid_reduce_kernel, grid_for(Hc, (int64_t)Wc * C, tb), dim3(tb), 0, s, im, H, W, C, Hc, Wc, out);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_expand(const double *d_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                   const double *im_coarse, int C, double *out, int32_t *source, hipStream_t s) {
  const int tb = H <= 64 ? 64 : 256;
  if (mode == 1)
    hipLaunchKernelGGL(pyramid_expand_kernel<true>, grid_for(H, W, tb), dim3(tb), 0, s, d_coarse, Hc, Wc, H, W, im_fine,
                       im_coarse, C, out, source);
  else
    hipLaunchKernelGGL(pyramid_expand_kernel<false>, grid_for(H, W, tb), dim3(tb), 0, s, d_coarse, Hc, Wc, H, W, im_fine,
                       im_coarse, C, out, source);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_pyramid_reduce_device(const double *im, int H, int W, int C, double *out, void *stream, char *err,
                                 size_t errcap) {
  if (int rc = reduce_args("stereo_pyramid_reduce_device", im, H, W, C, out, err, errcap)) return rc;
  return guarded("stereo_pyramid_reduce_device", err, errcap, [&] { launch_reduce(im, H, W, C, out, (hipStream_t)stream); });
}

int stereo_pyramid_expand_device(const double *d_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                                 const double *im_coarse, int C, double *out, int32_t *source, void *stream, char *err,
                                 size_t errcap) {
  if (int rc = expand_args("stereo_pyramid_expand_device", d_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out, source,
                           err, errcap))
    return rc;
  return guarded("stereo_pyramid_expand_device", err, errcap, [&] {
    launch_expand(d_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out, source, (hipStream_t)stream);
  });
}

int stereo_pyramid_reduce(const double *im, int H, int W, int C, double *out, char *err, size_t errcap) {
  if (int rc = reduce_args("stereo_pyramid_reduce", im, H, W, C, out, err, errcap)) return rc;
  return guarded("stereo_pyramid_reduce", err, errcap, [&] {
    const size_t n = (size_t)H * W * C, nc = (size_t)((H + 1) / 2) * ((W + 1) / 2) * C;
    stereo::DevBuf<double> a, o;
    a.upload(im, n); o.alloc(nc);
    launch_reduce(a.p, H, W, C, o.p, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, o.p, nc * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int stereo_pyramid_expand(const double *d_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                          const double *im_coarse, int C, double *out, int32_t *source, char *err, size_t errcap) {
  if (int rc = expand_args("stereo_pyramid_expand", d_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out, source, err,
                           errcap))
    return rc;
  return guarded("stereo_pyramid_expand", err, errcap, [&] {
    const size_t n = (size_t)H * W, nc = (size_t)Hc * Wc;
    stereo::DevBuf<double> d, f, g, o;
    stereo::DevBuf<int32_t> src;
    d.upload(d_coarse, nc); o.alloc(n);
    if (mode == 1) {
      f.upload(im_fine, n * C); g.upload(im_coarse, nc * C);
    }
    if (source) src.alloc(n);
    launch_expand(d.p, Hc, Wc, H, W, mode, f.p, g.p, C, o.p, source ? src.p : nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, o.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (source) STEREO_HIP_CHECK(hipMemcpy(source, src.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
