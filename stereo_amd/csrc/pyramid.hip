// Image pyramid: the 2 x 2 box reduction of an image and the expansion of a coarse
// disparity map to the next finer scale -- and of a coarse plane map, as planes.  No
// reference counterpart.
//
// Images are H x W x C and maps H x W, column major: element (y, x, c) at y + H (x + W c); a plane map
// is 4 x N, pixel (y, x) at 4 (y + H x).  In every
// kernel one thread makes one output element, the lanes of a wave run along y (consecutive addresses
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
using stereo::guarded;

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

// The candidate numbering and the guided choice, written once for the map and the plane expansion.
// at[k]: candidate k's element yc + Hc xc of a Hc x Wc array.
struct Footprint {
  size_t at[4];
};
__device__ __forceinline__ Footprint footprint(int y, int x, int Hc, int Wc) {
  const int yc = y >> 1, xc = x >> 1;
  const int ny = neighbour(y, yc, Hc);
  const size_t col = (size_t)Hc * xc, ncol = (size_t)Hc * neighbour(x, xc, Wc);
  return {{col + yc, col + ny, ncol + yc, ncol + ny}};
}
// Among the candidates with ok[k], the first one whose squared colour distance to the fine pixel no later one
// undercuts; -1 if none is ok.  f: the fine pixel's first channel.  All four distances are formed, from loads at
// addresses that are always valid.
__device__ __forceinline__ int guided_choice(const bool ok[4], const Footprint &fp, const double *__restrict__ f, size_t fine_plane,
                                    const double *__restrict__ g, size_t coarse_plane, int C) {
  double dist[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < C; ++c) {
    const double v = *f;
    const double e0 = v - g[fp.at[0]], e1 = v - g[fp.at[1]], e2 = v - g[fp.at[2]], e3 = v - g[fp.at[3]];
    dist[0] = dist[0] + e0 * e0;
    dist[1] = dist[1] + e1 * e1;
    dist[2] = dist[2] + e2 * e2;
    dist[3] = dist[3] + e3 * e3;
    f += fine_plane;
    g += coarse_plane;
  }
  int best = -1;
  double best_dist = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool take = ok[k] && (best < 0 || dist[k] < best_dist);
    best = take ? k : best;
    best_dist = take ? dist[k] : best_dist;
  }
  return best;
}

template <bool Guided>
__global__ void pyramid_expand_kernel(const double *__restrict__ d_coarse, int Hc, int Wc, int H, int W,
                                      const double *__restrict__ im_fine, const double *__restrict__ im_coarse, int C,
                                      double *__restrict__ out, int32_t *__restrict__ source) {
  const int yt = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = yt < H;
  const int y = live ? yt : H - 1;
  const size_t fine_plane = (size_t)H * W, coarse_plane = (size_t)Hc * Wc;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t x = blockIdx.y; x < W; x += gridDim.y) {
    const Footprint fp = footprint(y, (int)x, Hc, Wc);
    const size_t px = (size_t)H * (size_t)x + y;
    if (!Guided) {
      const double d = d_coarse[fp.at[0]];
      if (live) {
        out[px] = 2.0 * d;
        if (source) source[px] = 0;
      }
      continue;
    }
    const double d[4] = {d_coarse[fp.at[0]], d_coarse[fp.at[1]], d_coarse[fp.at[2]], d_coarse[fp.at[3]]};
    const bool ok[4] = {isfinite(d[0]), isfinite(d[1]), isfinite(d[2]), isfinite(d[3])};
    const int best = guided_choice(ok, fp, im_fine + px, fine_plane, im_coarse, coarse_plane, C);
    if (live) {
      out[px] = best >= 0 ? 2.0 * d[best] : nan;
      if (source) source[px] = best;
    }
  }
}

// ---------------------------------------------------------------- expand_planes
//
// The same candidates and the same choice on a coarse PLANE map (4 x Nc, 32 contiguous bytes per pixel, moved as two
// 16-byte accesses): a candidate is valid when its four components are finite and c != 0.  The chosen plane [a b c d]
// becomes [a, b, c, (2 d + 0.5 a) + 0.5 b]: planes live in 1-based pixel coordinates, the fine pixel x sits at the
// coarse coordinate (x + 0.5) / 2, and one coarse disparity unit is two fine ones.  The transform is the same at
// every pixel, the replicated last row or column of an odd size included.  No valid candidate (nearest: candidate 0
// not valid): four NaN; source -1 (guided) or 0 (nearest).  A wave stores 2 KiB in a row.
struct Plane {
  double2 ab, cd;
};
__device__ __forceinline__ Plane load_plane(const double *p) {
  const double2 *v = reinterpret_cast<const double2 *>(p);
  return {v[0], v[1]};
}
__device__ __forceinline__ bool plane_ok(const Plane &p) {
  return isfinite(p.ab.x) && isfinite(p.ab.y) && isfinite(p.cd.x) && isfinite(p.cd.y) && p.cd.x != 0.0;
}

template <bool Guided>
__global__ void pyramid_expand_planes_kernel(const double *__restrict__ p_coarse, int Hc, int Wc, int H, int W,
                                             const double *__restrict__ im_fine, const double *__restrict__ im_coarse,
                                             int C, double *__restrict__ out, int32_t *__restrict__ source) {
  const int yt = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = yt < H;
  const int y = live ? yt : H - 1;
  const size_t fine_plane = (size_t)H * W, coarse_plane = (size_t)Hc * Wc;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t x = blockIdx.y; x < W; x += gridDim.y) {
    const Footprint fp = footprint(y, (int)x, Hc, Wc);
    const size_t px = (size_t)H * (size_t)x + y;
    Plane p = load_plane(p_coarse + 4 * fp.at[0]);
    int best = 0;
    bool valid = plane_ok(p);
    if (Guided) {
      const Plane p1 = load_plane(p_coarse + 4 * fp.at[1]), p2 = load_plane(p_coarse + 4 * fp.at[2]),
                  p3 = load_plane(p_coarse + 4 * fp.at[3]);
      const bool ok[4] = {valid, plane_ok(p1), plane_ok(p2), plane_ok(p3)};
      best = guided_choice(ok, fp, im_fine + px, fine_plane, im_coarse, coarse_plane, C);
      auto pick = [best](double v0, double v1, double v2, double v3) { return best == 1 ? v1 : best == 2 ? v2 : best == 3 ? v3 : v0; };
      p = Plane{make_double2(pick(p.ab.x, p1.ab.x, p2.ab.x, p3.ab.x), pick(p.ab.y, p1.ab.y, p2.ab.y, p3.ab.y)),
                make_double2(pick(p.cd.x, p1.cd.x, p2.cd.x, p3.cd.x), pick(p.cd.y, p1.cd.y, p2.cd.y, p3.cd.y))};
      valid = best >= 0;
    }
    if (live) {
      double2 *o = reinterpret_cast<double2 *>(out + 4 * px);
      o[0] = valid ? p.ab : make_double2(nan, nan);
      o[1] = valid ? make_double2(p.cd.x, (2.0 * p.cd.y + 0.5 * p.ab.x) + 0.5 * p.ab.y) : make_double2(nan, nan);
      if (source) source[px] = best;
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

// (`coarse`: what the entry calls its coarse input, d_coarse or p_coarse)
int expand_args(const char *name, const void *d_coarse, int Hc, int Wc, int H, int W, int mode, const void *im_fine,
                const void *im_coarse, int C, const void *out, const void *source, char *err, size_t errcap,
                const char *coarse = "d_coarse") {
  const std::string what(name);
  if (mode != 0 && mode != 1) return fail(what + ": mode must be 0 (nearest) or 1 (guided)", err, errcap);
  if (!d_coarse || !out) return fail(what + ": " + coarse + " and out must not be NULL", err, errcap);
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

// expand_args' refusals, and for the plane buffers (4 doubles per pixel) the overlaps a plain pointer comparison
// does not see: the images and `source` inside the fine planes.
int expand_planes_args(const char *name, const double *p_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                       const double *im_coarse, int C, const double *out, const int32_t *source, bool device, char *err,
                       size_t errcap) {
  if (int rc = expand_args(name, p_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out, source, err, errcap, "p_coarse"))
    return rc;
  const std::string what(name);
  const char *o0 = (const char *)out, *o1 = o0 + 32 * (size_t)H * W;
  const char *c0 = (const char *)p_coarse, *c1 = c0 + 32 * (size_t)Hc * Wc;
  auto overlaps = [](const char *a0, const char *a1, const char *b0, const char *b1) { return a0 < b1 && b0 < a1; };
  if (overlaps(o0, o1, c0, c1)) return fail(what + ": out must not alias an input", err, errcap);
  if (source) {
    const char *s0 = (const char *)source, *s1 = s0 + 4 * (size_t)H * W;
    if (overlaps(s0, s1, o0, o1) || overlaps(s0, s1, c0, c1)) return fail(what + ": source must not alias an input or out", err, errcap);
  }
  if (mode == 1) {
    const char *f0 = (const char *)im_fine, *g0 = (const char *)im_coarse;
    if (overlaps(o0, o1, f0, f0 + 8 * (size_t)H * W * C) || overlaps(o0, o1, g0, g0 + 8 * (size_t)Hc * Wc * C))
      return fail(what + ": out must not alias an input", err, errcap);
  }
  if (device && ((((uintptr_t)p_coarse) | ((uintptr_t)out)) & 15) != 0)
    return fail(what + ": p_coarse and out must be 16-byte aligned (a plane moves as two 16-byte accesses)", err, errcap);
  return 0;
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

void launch_expand_planes(const double *p_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                          const double *im_coarse, int C, double *out, int32_t *source, hipStream_t s) {
  const int tb = H <= 64 ? 64 : 256;
  if (mode == 1)
    hipLaunchKernelGGL(pyramid_expand_planes_kernel<true>, grid_for(H, W, tb), dim3(tb), 0, s, p_coarse, Hc, Wc, H, W,
                       im_fine, im_coarse, C, out, source);
  else
    hipLaunchKernelGGL(pyramid_expand_planes_kernel<false>, grid_for(H, W, tb), dim3(tb), 0, s, p_coarse, Hc, Wc, H, W,
                       im_fine, im_coarse, C, out, source);
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

int stereo_pyramid_expand_planes_device(const double *p_coarse, int Hc, int Wc, int H, int W, int mode,
                                        const double *im_fine, const double *im_coarse, int C, double *out,
                                        int32_t *source, void *stream, char *err, size_t errcap) {
  if (int rc = expand_planes_args("stereo_pyramid_expand_planes_device", p_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C,
                                  out, source, true, err, errcap))
    return rc;
  return guarded("stereo_pyramid_expand_planes_device", err, errcap, [&] {
    launch_expand_planes(p_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out, source, (hipStream_t)stream);
  });
}

int stereo_pyramid_expand_planes(const double *p_coarse, int Hc, int Wc, int H, int W, int mode, const double *im_fine,
                                 const double *im_coarse, int C, double *out, int32_t *source, char *err, size_t errcap) {
  if (int rc = expand_planes_args("stereo_pyramid_expand_planes", p_coarse, Hc, Wc, H, W, mode, im_fine, im_coarse, C, out,
                                  source, false, err, errcap))
    return rc;
  return guarded("stereo_pyramid_expand_planes", err, errcap, [&] {
    const size_t n = (size_t)H * W, nc = (size_t)Hc * Wc;
    stereo::DevBuf<double> p, f, g, o;
    stereo::DevBuf<int32_t> src;
    p.upload(p_coarse, 4 * nc); o.alloc(4 * n);
    if (mode == 1) {
      f.upload(im_fine, n * C); g.upload(im_coarse, nc * C);
    }
    if (source) src.alloc(n);
    launch_expand_planes(p.p, Hc, Wc, H, W, mode, f.p, g.p, C, o.p, source ? src.p : nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, o.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (source) STEREO_HIP_CHECK(hipMemcpy(source, src.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
