// Local plane fit (the definition: include/stereo_hip.h): every pixel's plane is replaced by the
// least-squares plane through the surface its neighbours' planes draw, each taken at its own pixel.  This is what
// creates a slant: bands move a plane along the disparity axis and candidates copy planes, neither tilts one.
//
// Planes are 4 x N doubles, pixels column major (pixel (y, x) at 4 (y + H x)); a plane moves as two 16-byte accesses.
// A workgroup of 256 threads makes a tile of kTileY x kTileX pixels.  It first stages z -- every plane's disparity at
// its own pixel, NaN for a plane without one and for a position outside the image -- of the tile and a halo of `radius`
// pixels in LDS: (kTileY + 2 r) (kTileX + 2 r) doubles, 20 KiB at r = 8, so a plane is read from memory once per tile
// that needs it, not once per tap.  Lanes run along y in the staging, the tap walk and the store: a wave's 64 planes
// are 2 KiB in a row, and its LDS reads of one tap are 64 consecutive doubles.  Wave w of the block then walks the
// columns 4 w .. 4 w + 3 of the tile, one after the other: (2 r + 1)^2 taps from LDS, nine sums in registers (the six
// whole-number ones in int32), three divisions at the end.
#include <cmath>
#include <cstdint>
#include <string>

#include "band_common.h"
#include "common.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::band::check_sizes;
using stereo::guarded;

constexpr int kTileY = 64, kTileX = 16, kThreads = 256, kColumnsPerWave = kTileX / (kThreads / kTileY);
constexpr int kMaxRadius = 8;

struct Plane {
  double2 ab, cd;
};
__device__ __forceinline__ Plane load_plane(const double *p) {
  const double2 *v = reinterpret_cast<const double2 *>(p);
  return {v[0], v[1]};
}
__device__ __forceinline__ void store_plane(double *p, const Plane &pl) {
  double2 *v = reinterpret_cast<double2 *>(p);
  v[0] = pl.ab;
  v[1] = pl.cd;
}
__device__ __forceinline__ bool plane_ok(const Plane &p) {
  return isfinite(p.ab.x) && isfinite(p.ab.y) && isfinite(p.cd.x) && isfinite(p.cd.y) && p.cd.x != 0.0;
}

// (the grid's y stops at 65535: a block of a wider image takes every gridDim.y-th column tile)
__global__ __launch_bounds__(kThreads) void planes_fit_local_kernel(const double *__restrict__ planes, int H, int W, int r,
                                                                   double tau, double *__restrict__ out, int32_t *bad) {
  extern __shared__ double fit_z[];
  const int LH = kTileY + 2 * r, LW = kTileX + 2 * r;
  const int y0 = (int)blockIdx.x * kTileY;
  const int ly = (int)threadIdx.x % kTileY, wave = (int)threadIdx.x / kTileY;
  const int y = y0 + ly;
  const double nan = __builtin_nan("");
  const int tiles = (W + kTileX - 1) / kTileX;
  for (int tile = (int)blockIdx.y; tile < tiles; tile += (int)gridDim.y) {
    const int x0 = tile * kTileX;
    for (int l = (int)threadIdx.x; l < LH * LW; l += kThreads) {
      const int lx = l / LH, yy = y0 - r + (l - lx * LH), xx = x0 - r + lx;
      double z = nan;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const Plane p = load_plane(planes + 4 * ((size_t)H * (size_t)xx + (size_t)yy));
        const double s = p.ab.x * (double)(xx + 1) + p.ab.y * (double)(yy + 1);
        z = plane_ok(p) ? -(s + p.cd.y) / p.cd.x : nan;
      }
      fit_z[l] = z;
    }
    __syncthreads();
    for (int j = 0; j < kColumnsPerWave; ++j) {
      const int lx = wave * kColumnsPerWave + j, x = x0 + lx;
      if (x >= W || y >= H) continue;                  // (no barrier below this line inside the loop)
      const double *centre = fit_z + (size_t)(lx + r) * LH + (ly + r);
      const double z0 = *centre;
      const size_t px = (size_t)H * (size_t)x + (size_t)y;
      if (!isfinite(z0)) {                             // (rare) a plane without a disparity is copied through
        const Plane own = load_plane(planes + 4 * px);
        if (!plane_ok(own)) {
          if (bad) atomicAdd(bad, 1);
          store_plane(out + 4 * px, own);
          continue;
        }
      }
      // The six sums that do not see e are whole numbers below 2^15, exact in any number format and any order: they are
      // kept in int32 (a tap's dx, dy and their products are wave-uniform scalars) and converted once, which leaves
      // three fp64 sums -- five fp64 operations per tap instead of fourteen -- and the bits of the definition.
      int ni = 0, Sxi = 0, Syi = 0, Sxxi = 0, Sxyi = 0, Syyi = 0;
      double Sz = 0.0, Sxz = 0.0, Syz = 0.0;
      for (int dx = -r; dx <= r; ++dx) {
        const double *column = centre + dx * LH;
        const double fx = (double)dx;
        for (int dy = -r; dy <= r; ++dy) {
          const double e = column[dy] - z0;
          if (!(fabs(e) <= tau)) continue;
          ni += 1;
          Sxi += dx;
          Syi += dy;
          Sxxi += dx * dx;
          Sxyi += dx * dy;
          Syyi += dy * dy;
          Sz = Sz + e;
          Sxz = Sxz + fx * e;
          Syz = Syz + (double)dy * e;
        }
      }
      const double n = (double)ni, Sx = (double)Sxi, Sy = (double)Syi, Sxx = (double)Sxxi, Sxy = (double)Sxyi, Syy = (double)Syyi;
      const double c00 = Syy * n - Sy * Sy, c01 = Sxy * n - Sy * Sx, c02 = Sxy * Sy - Syy * Sx;
      const double det = (Sxx * c00 - Sxy * c01) + Sx * c02;
      double al = 0.0, be = 0.0, ga = 0.0;
      if (n >= 3.0 && det > 0.0) {
        const double c11 = Sxx * n - Sx * Sx, c12 = Sxx * Sy - Sxy * Sx, c22 = Sxx * Syy - Sxy * Sxy;
        al = ((c00 * Sxz - c01 * Syz) + c02 * Sz) / det;
        be = ((c11 * Syz - c01 * Sxz) - c12 * Sz) / det;
        ga = ((c02 * Sxz - c12 * Syz) + c22 * Sz) / det;
      }
      const double g = ((z0 + ga) - al * (double)(x + 1)) - be * (double)(y + 1);
      store_plane(out + 4 * px, Plane{make_double2(-al, -be), make_double2(1.0, -g)});
    }
    __syncthreads();                                   // the next tile overwrites fit_z
  }
}

int fit_args(const char *name, const double *planes, int H, int W, int radius, double tau, const double *out, bool device,
             char *err, size_t errcap) {
  const std::string what(name);
  if (!planes || !out) return fail(what + ": planes and out must not be NULL", err, errcap);
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (radius < 1 || radius > kMaxRadius)
    return fail(what + ": radius must be 1 .. " + std::to_string(kMaxRadius) + " (got " + std::to_string(radius) + ")", err, errcap);
  if (!(tau >= 0.0)) return fail(what + ": tau must be at least 0 (+inf is allowed, NaN is not)", err, errcap);
  const char *p0 = (const char *)planes, *o0 = (const char *)out;
  const size_t bytes = 32 * (size_t)H * W;
  if (p0 < o0 + bytes && o0 < p0 + bytes)
    return fail(what + ": out must not alias planes (a pixel reads its neighbours' planes)", err, errcap);
  if (device && ((((uintptr_t)planes) | ((uintptr_t)out)) & 15) != 0)
    return fail(what + ": planes and out must be 16-byte aligned (a plane moves as two 16-byte accesses)", err, errcap);
  return 0;
}

void launch_fit(const double *planes, int H, int W, int radius, double tau, double *out, int32_t *bad, hipStream_t s) {
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  const int tiles = (W + kTileX - 1) / kTileX;
  const dim3 grid((unsigned)((H + kTileY - 1) / kTileY), (unsigned)(tiles < 65535 ? tiles : 65535));
  const size_t lds = (size_t)(kTileY + 2 * radius) * (kTileX + 2 * radius) * sizeof(double);
  hipLaunchKernelGGL(planes_fit_local_kernel, grid, dim3(kThreads), lds, s, planes, H, W, radius, tau, out, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_planes_fit_local_device(const double *planes, int H, int W, int radius, double tau, double *out, int32_t *bad,
                                   void *stream, char *err, size_t errcap) {
  if (int rc = fit_args("stereo_planes_fit_local_device", planes, H, W, radius, tau, out, true, err, errcap)) return rc;
  return guarded("stereo_planes_fit_local_device", err, errcap,
                 [&] { launch_fit(planes, H, W, radius, tau, out, bad, (hipStream_t)stream); });
}

int stereo_planes_fit_local(const double *planes, int H, int W, int radius, double tau, double *out, int32_t *bad, char *err,
                            size_t errcap) {
  if (int rc = fit_args("stereo_planes_fit_local", planes, H, W, radius, tau, out, false, err, errcap)) return rc;
  return guarded("stereo_planes_fit_local", err, errcap, [&] {
    const size_t n = (size_t)H * W;
    stereo::DevBuf<double> p, o;
    stereo::DevBuf<int32_t> b;
    p.upload(planes, 4 * n); o.alloc(4 * n); b.alloc(1);
    launch_fit(p.p, H, W, radius, tau, o.p, b.p, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, o.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (bad) STEREO_HIP_CHECK(hipMemcpy(bad, b.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
