// Map filter: the image-guided weighted median of a disparity map over a (2r+1)^2 window, r = 1 .. 4,
// with the pixel every output value came from.  No reference counterpart.  The definition: include/stereo_hip.h; restated
// in tests/map_filter_restate.py.
//
// One launch, one thread per pixel, lanes along y: a workgroup owns kTileH x kTileW pixels and stages their window's
// d -- a value that is not finite, or lies outside the image, as NaN, which no comparison selects -- in LDS.  The guide
// is staged one channel at a time into a second tile, and pixel_weight after it; a thread's (2r+1)^2 tap weights then
// live in registers.  For every candidate tap j a thread sums the weights of the taps i with d_i <= d_j in tap order (two
// candidates per pass over the taps: two independent chains of adds on one read of d_i) and keeps the smallest d_j whose
// doubled sum reaches the total: (2r+1)^4 compare-select-add steps per pixel.  A selection, plain fp64 adds in the
// definition's order and one product per tap (-ffp-contract=off): the outputs are the restatement's bits.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "common.h"
#include "contrast_rule.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;

constexpr int kMaxRadius = 4;
constexpr int kTileH = 64, kTileW = 4;       // one wave per tile column
constexpr int kBlock = kTileH * kTileW;

// The (kTileH + 2 R) x (kTileW + 2 R) window of `src` around the tile at (y0, x0) into `tile`, column major; `outside`
// where the image ends.  CANONICAL: a value that is not finite becomes NaN.
template <int R, bool CANONICAL>
__device__ __forceinline__ void stage(double *tile, const double *__restrict__ src, int H, int W, int y0, int x0,
                                      double outside) {
  constexpr int SH = kTileH + 2 * R, SW = kTileW + 2 * R;
  for (int e = threadIdx.x; e < SH * SW; e += kBlock) {
    const int tx = e / SH, ty = e - tx * SH;
    const int y = y0 - R + ty;
    const int64_t x = (int64_t)x0 - R + tx;              // (x0 + kTileW + R may pass 2^31 on a one-row map)
    double v = outside;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      v = src[(int64_t)y + (int64_t)H * x];
      if (CANONICAL && !isfinite(v)) v = outside;
    }
    tile[e] = v;
  }
}

template <int R, bool GUIDED, bool WEIGHTED>
__global__ void __launch_bounds__(kBlock)
    map_median_kernel(const double *__restrict__ d, int H, int W, const double *__restrict__ im, int C,
                      stereo_contrast_params par, const double *__restrict__ pixel_weight,
                      const int32_t *__restrict__ targets, double *__restrict__ out, int32_t *__restrict__ source,
                      int32_t *kept) {
  constexpr int S = 2 * R + 1, T = S * S;
  constexpr int SH = kTileH + 2 * R, SW = kTileW + 2 * R;
  // The T weights live in registers.  So do the T values of d where both fit a wave's 512 (the compiler hoists the
  // loop's LDS reads by itself); at r = 4 with weights they do not -- 324 registers and the loop's own spill to
  // scratch -- so there every pass over the taps reads d from LDS again: a compiler-only fence keeps the reads in the loop.
  constexpr bool kRereadTaps = (GUIDED || WEIGHTED) && 4 * T > 200;
  __shared__ double dt[SH * SW];
  __shared__ double gt[(GUIDED || WEIGHTED) ? SH * SW : 1];

  const int nby = (H + kTileH - 1) / kTileH;
  const int bx = (int)(blockIdx.x / (unsigned)nby), by = (int)(blockIdx.x - (unsigned)bx * (unsigned)nby);
  const int y0 = by * kTileH, x0 = bx * kTileW;
  const int ly = threadIdx.x % kTileH, lx = threadIdx.x / kTileH;
  const int y = y0 + ly, x = x0 + lx;
  const bool inside = y < H && x < W;
  const int64_t p = (int64_t)y + (int64_t)H * x;
  const bool active = inside && (!targets || targets[p] != 0);
  const double own = inside ? d[p] : 0.0;

  // a tile without a target copies and leaves (the same decision in every thread: no barrier is skipped by some)
  if (!__syncthreads_or(active)) {
    if (inside) {
      out[p] = own;
      if (source) source[p] = (int32_t)p;
    }
    return;
  }

  const double nan = std::numeric_limits<double>::quiet_NaN();
  stage<R, true>(dt, d, H, W, y0, x0, nan);
  const int base = (ly + R) + SH * (lx + R);           // this thread's pixel in a tile

  double w[(GUIDED || WEIGHTED) ? T : 1];
  if (GUIDED) {
    const int64_t N = (int64_t)H * W;
#pragma unroll
    for (int i = 0; i < T; ++i) w[i] = 0.0;             // the contrasts first, channel by channel
    for (int c = 0; c < C; ++c) {
      __syncthreads();                                   // (the tile's readers of the channel before are done)
      stage<R, false>(gt, im + N * c, H, W, y0, x0, 0.0);
      __syncthreads();
      if (active) {
        bool ok = true;
        const double centre = gt[base];
#pragma unroll
        for (int dx = -R; dx <= R; ++dx)
#pragma unroll
          for (int dy = -R; dy <= R; ++dy) {
            const int i = (dx + R) * S + (dy + R);
            w[i] = stereo::contrast_channel(w[i], centre, gt[base + dy + SH * dx], ok);
          }
      }
    }
#pragma unroll
    for (int i = 0; i < T; ++i) w[i] = stereo::ramp(w[i], par);
  }
  if (WEIGHTED) {
    __syncthreads();
    stage<R, false>(gt, pixel_weight, H, W, y0, x0, 0.0);
  }
  __syncthreads();                                       // dt, and gt with pixel_weight, are staged
  if (!active) {                                         // past H or W, or not a target: no loop
    if (inside) {
      out[p] = own;
      if (source) source[p] = (int32_t)p;
    }
    return;
  }
  if (WEIGHTED) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx)
#pragma unroll
      for (int dy = -R; dy <= R; ++dy) {
        const int i = (dx + R) * S + (dy + R);
        const double pw = gt[base + dy + SH * dx];
        w[i] = GUIDED ? w[i] * pw : pw;
      }
  }

  double total = 0.0;
#pragma unroll
  for (int dx = -R; dx <= R; ++dx)
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
      const double di = dt[base + dy + SH * dx];
      const double wi = (GUIDED || WEIGHTED) ? w[(dx + R) * S + (dy + R)] : 1.0;
      total += di == di ? wi : 0.0;
    }

  double res = own;
  int32_t src = (int32_t)p;
  if (total > 0.0) {
    const int corner = base - R - SH * R;                // tap 0
    double best = std::numeric_limits<double>::infinity();
#pragma unroll 1
    for (int j = 0; j < T; j += 2) {
      const int jx0 = j / S, jx1 = (j + 1) / S;
      const double v0 = dt[corner + (j - jx0 * S) + SH * jx0];
      const double v1 = j + 1 < T ? dt[corner + (j + 1 - jx1 * S) + SH * jx1] : nan;
      double a0 = 0.0, a1 = 0.0;
      if (kRereadTaps) __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
      for (int dx = -R; dx <= R; ++dx)
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
          const double di = dt[base + dy + SH * dx];
          const double wi = (GUIDED || WEIGHTED) ? w[(dx + R) * S + (dy + R)] : 1.0;
          a0 += di <= v0 ? wi : 0.0;
          a1 += di <= v1 ? wi : 0.0;
        }
      if (2.0 * a0 >= total && v0 < best) best = v0;     // (a NaN candidate sums to 0 and never qualifies)
      if (2.0 * a1 >= total && v1 < best) best = v1;
    }
    // the first tap in tap order with a positive weight and the value: walked backwards, the last hit stays
#pragma unroll
    for (int dx = R; dx >= -R; --dx)
#pragma unroll
      for (int dy = R; dy >= -R; --dy) {
        const double di = dt[base + dy + SH * dx];
        const double wi = (GUIDED || WEIGHTED) ? w[(dx + R) * S + (dy + R)] : 1.0;
        if (wi > 0.0 && di == best) {
          res = di;
          src = (int32_t)(p + dy + (int64_t)H * dx);
        }
      }
  } else {
    atomicAdd(kept, 1);
  }
  out[p] = res;
  if (source) source[p] = src;
}

struct Args {
  const double *d;
  int H, W, radius;
  const double *im;
  int C;
  const stereo_contrast_params *params;
  const double *pixel_weight;
  const int32_t *targets;
  double *out;
  int32_t *source, *kept;
};

int check_args(const std::string &w, const Args &a, char *err, size_t errcap) {
  if (a.H < 1 || a.W < 1) return fail(w + ": H and W must be at least 1", err, errcap);
  if ((int64_t)a.H * (int64_t)a.W >= ((int64_t)1 << 31))
    return fail(w + ": H * W must be below 2^31 (pixel ids are int32)", err, errcap);
  if (a.radius < 1 || a.radius > kMaxRadius)
    return fail(w + ": radius must be 1 .. " + std::to_string(kMaxRadius) + " (got " + std::to_string(a.radius) + ")", err,
                errcap);
  if (!a.d || !a.out || !a.kept) return fail(w + ": d, out and kept must not be NULL", err, errcap);
  if ((a.im != nullptr) != (a.params != nullptr))
    return fail(w + ": im and params must be given together, or neither", err, errcap);
  if (a.im) {
    if (a.C < 1) return fail(w + ": C must be at least 1 with an image", err, errcap);
    if (const char *wrong = stereo::contrast_params_error(*a.params); *wrong) return fail(w + ": " + wrong, err, errcap);
  }
  const void *inputs[4] = {a.d, a.im, a.pixel_weight, a.targets};
  for (const void *in : inputs)
    if (in && (in == (const void *)a.out || in == (const void *)a.source || in == (const void *)a.kept))
      return fail(w + ": out, source and kept must not be an input", err, errcap);
  if ((const void *)a.out == (const void *)a.source || (const void *)a.out == (const void *)a.kept ||
      (a.source && (const void *)a.source == (const void *)a.kept))
    return fail(w + ": out, source and kept must be three arrays", err, errcap);
  return 0;
}

template <int R, bool GUIDED, bool WEIGHTED>
void launch_one(const Args &a, hipStream_t s) {
  const int64_t blocks = (int64_t)((a.H + kTileH - 1) / kTileH) * ((a.W + kTileW - 1) / kTileW);
  const stereo_contrast_params par = a.params ? *a.params : stereo_contrast_params{1.0, 1.0, 0.0, 0.0};
  hipLaunchKernelGGL((map_median_kernel<R, GUIDED, WEIGHTED>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a.d, a.H, a.W, a.im,
                     a.C, par, a.pixel_weight, a.targets, a.out, a.source, a.kept);
}

template <int R>
void launch_radius(const Args &a, hipStream_t s) {
  if (a.im) {
    if (a.pixel_weight) launch_one<R, true, true>(a, s);
    else launch_one<R, true, false>(a, s);
  } else {
    if (a.pixel_weight) launch_one<R, false, true>(a, s);
    else launch_one<R, false, false>(a, s);
  }
}

void launch(const Args &a, hipStream_t s) {
  STEREO_HIP_CHECK(hipMemsetAsync(a.kept, 0, sizeof(int32_t), s));
  switch (a.radius) {
    case 1: launch_radius<1>(a, s); break;
    case 2: launch_radius<2>(a, s); break;
    case 3: launch_radius<3>(a, s); break;
    default: launch_radius<4>(a, s); break;
  }
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_map_filter_max_radius(void) { return kMaxRadius; }

int stereo_map_weighted_median_device(const double *d, int H, int W, int radius, const double *im, int C,
                                      const stereo_contrast_params *params, const double *pixel_weight,
                                      const int32_t *targets, double *out, int32_t *source, int32_t *kept, void *stream,
                                      char *err, size_t errcap) {
  const char *what = "stereo_map_weighted_median_device";
  const Args a{d, H, W, radius, im, C, params, pixel_weight, targets, out, source, kept};
  if (int rc = check_args(what, a, err, errcap)) return rc;
  return guarded(what, err, errcap, [&] { launch(a, (hipStream_t)stream); });
}

int stereo_map_weighted_median(const double *d, int H, int W, int radius, const double *im, int C,
                               const stereo_contrast_params *params, const double *pixel_weight, const int32_t *targets,
                               double *out, int32_t *source, int32_t *kept, char *err, size_t errcap) {
  const std::string what = "stereo_map_weighted_median";
  if (int rc = check_args(what, Args{d, H, W, radius, im, C, params, pixel_weight, targets, out, source, kept}, err, errcap))
    return rc;
  const size_t n = (size_t)H * W;
  if (im)
    for (size_t i = 0; i < n * C; ++i)
      if (!std::isfinite(im[i]))
        return fail(what + ": im must be finite (pixel " + std::to_string(i % n) + ", channel " + std::to_string(i / n) + ")",
                    err, errcap);
  if (pixel_weight)
    for (size_t i = 0; i < n; ++i)
      if (!(pixel_weight[i] >= 0.0) || !std::isfinite(pixel_weight[i]))
        return fail(what + ": a pixel weight must be finite and non-negative (pixel " + std::to_string(i) + ")", err, errcap);
  return guarded(what.c_str(), err, errcap, [&] {
    stereo::DevBuf<double> dd, di, dw, dout;
    stereo::DevBuf<int32_t> dtg, dsrc, dkept;
    dd.upload(d, n); dout.alloc(n); dkept.alloc(1);
    if (im) di.upload(im, n * C);
    if (pixel_weight) dw.upload(pixel_weight, n);
    if (targets) dtg.upload(targets, n);
    if (source) dsrc.alloc(n);
    launch(Args{dd.p, H, W, radius, di.p, C, params, dw.p, dtg.p, dout.p, dsrc.p, dkept.p}, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (source) STEREO_HIP_CHECK(hipMemcpy(source, dsrc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    STEREO_HIP_CHECK(hipMemcpy(kept, dkept.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
