// Image-guided smoothness weights: the contrast of two pixels, max_c |im(a, c) - im(b, c)|, through a
// piecewise linear ramp, as the alphas of any edge list and as the R x N step weights of scanline directions.  No
// reference counterpart.  The definition: include/stereo_hip.h; restated in tests/contrast_restate.py.
//
// Both kernels are one thread per output and bound by their loads (2 C doubles read per double written).  The rule is
// plain fp64 in the header's order (-ffp-contract=off): the outputs are the restatement's bits.
#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "contrast_rule.h"
#include "stereo_hip.h"

namespace {

using stereo::contrast;
using stereo::fail;
using stereo::guarded;
using stereo::ramp;

constexpr int kBlock = 256;
constexpr int kMaxDirections = 8;

struct Directions {
  int dy[kMaxDirections], dx[kMaxDirections];
};

__global__ void __launch_bounds__(kBlock)
    contrast_edge_kernel(const double *__restrict__ im, int64_t N, int C, const uint32_t *__restrict__ conn, int64_t E,
                         stereo_contrast_params p, double *__restrict__ alphas, int32_t *bad) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= E) return;
  const int64_t a = conn[2 * e], b = conn[2 * e + 1];
  bool ok = a < N && b < N;
  double w = 0.0;
  if (ok) {
    const double g = contrast(im, N, C, a, b, ok);
    if (ok) w = ramp(g, p);
  }
  if (!ok) atomicAdd(bad, 1);
  alphas[e] = w;
}

__global__ void __launch_bounds__(kBlock)
    contrast_step_kernel(const double *__restrict__ im, int H, int W, int C, Directions dirs, int R, stereo_contrast_params p,
                         double *__restrict__ wstep) {
  const int64_t N = (int64_t)H * W;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N * R) return;
  const int r = (int)(i / N);
  const int64_t q = i - (int64_t)r * N;
  const int x = (int)(q / H), y = (int)(q - (int64_t)x * H);
  int dy = 0, dx = 0;
#pragma unroll
  for (int j = 0; j < kMaxDirections; ++j)        // (a select per entry: an indexed read of a by-value array is scratch)
    if (j == r) { dy = dirs.dy[j]; dx = dirs.dx[j]; }
  const int yp = y - dy, xp = x - dx;
  double w = 0.0;
  if (yp >= 0 && yp < H && xp >= 0 && xp < W) {
    bool ok = true;
    w = ramp(contrast(im, N, C, q, (int64_t)yp + (int64_t)H * xp, ok), p);
  }
  wstep[i] = w;
}

int check_image(const std::string &w, const void *im, int H, int W, int C, const stereo_contrast_params *p, char *err,
                size_t errcap) {
  if (H < 1 || W < 1 || C < 1) return fail(w + ": H, W and C must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(w + ": H * W must be below 2^31 (pixel ids are int32)", err, errcap);
  if (!im || !p) return fail(w + ": im and params must not be NULL", err, errcap);
  if (const char *wrong = stereo::contrast_params_error(*p); *wrong) return fail(w + ": " + wrong, err, errcap);
  return 0;
}

int check_edges(const std::string &w, const void *im, int H, int W, int C, const void *conn, int64_t E,
                const stereo_contrast_params *p, const void *alphas, char *err, size_t errcap) {
  if (int rc = check_image(w, im, H, W, C, p, err, errcap)) return rc;
  if (E < 0) return fail(w + ": E must not be negative", err, errcap);
  if (!alphas || (E > 0 && !conn)) return fail(w + ": conn and alphas must not be NULL (conn may be at E = 0)", err, errcap);
  if (alphas == im || alphas == conn) return fail(w + ": alphas must not be an input", err, errcap);
  return 0;
}

int check_steps(const std::string &w, const void *im, int H, int W, int C, const int32_t *directions, int R,
                const stereo_contrast_params *p, const void *wstep, Directions &dirs, char *err, size_t errcap) {
  if (int rc = check_image(w, im, H, W, C, p, err, errcap)) return rc;
  if (R < 1 || R > kMaxDirections)
    return fail(w + ": R (the number of directions) must be 1 .. " + std::to_string(kMaxDirections), err, errcap);
  if (!directions || !wstep) return fail(w + ": directions and wstep must not be NULL", err, errcap);
  if (wstep == im) return fail(w + ": wstep must not be im", err, errcap);
  dirs = Directions{};
  for (int r = 0; r < R; ++r) {
    const int dy = directions[2 * r], dx = directions[2 * r + 1];
    if (dy < -1 || dy > 1 || dx < -1 || dx > 1 || (dy == 0 && dx == 0))
      return fail(w + ": a direction must be (dy, dx) with dy, dx in {-1, 0, 1}, not both 0 (direction " + std::to_string(r) +
                  " is (" + std::to_string(dy) + ", " + std::to_string(dx) + "))", err, errcap);
    dirs.dy[r] = dy; dirs.dx[r] = dx;
  }
  return 0;
}

int check_finite_image(const std::string &w, const double *im, size_t n, char *err, size_t errcap) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(im[i])) return fail(w + ": im must be finite", err, errcap);
  return 0;
}

void launch_edges(const double *im, int H, int W, int C, const uint32_t *conn, int64_t E, const stereo_contrast_params &p,
                  double *alphas, int32_t *bad, hipStream_t s) {
  STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (E < 1) return;
  hipLaunchKernelGGL(contrast_edge_kernel, dim3((unsigned)((E + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, im,
                     (int64_t)H * W, C, conn, E, p, alphas, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_steps(const double *im, int H, int W, int C, const Directions &dirs, int R, const stereo_contrast_params &p,
                  double *wstep, hipStream_t s) {
  const int64_t total = (int64_t)H * W * R;
  hipLaunchKernelGGL(contrast_step_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, im, H, W, C,
                     dirs, R, p, wstep);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_contrast_edge_weights_device(const double *im, int H, int W, int C, const uint32_t *conn, int64_t E,
                                        const stereo_contrast_params *params, double *alphas, int32_t *bad, void *stream,
                                        char *err, size_t errcap) {
  const char *what = "stereo_contrast_edge_weights_device";
  if (int rc = check_edges(what, im, H, W, C, conn, E, params, alphas, err, errcap)) return rc;
  if (!bad) return fail(std::string(what) + ": bad must not be NULL", err, errcap);
  return guarded(what, err, errcap, [&] { launch_edges(im, H, W, C, conn, E, *params, alphas, bad, (hipStream_t)stream); });
}

int stereo_contrast_edge_weights(const double *im, int H, int W, int C, const uint32_t *conn, int64_t E,
                                 const stereo_contrast_params *params, double *alphas, char *err, size_t errcap) {
  const std::string what = "stereo_contrast_edge_weights";
  if (int rc = check_edges(what, im, H, W, C, conn, E, params, alphas, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  for (int64_t e = 0; e < E; ++e)
    for (int j = 0; j < 2; ++j)
      if (conn[2 * e + j] >= n)
        return fail(what + ": edge " + std::to_string(e) + " (" + std::to_string(conn[2 * e]) + ", " +
                    std::to_string(conn[2 * e + 1]) + ") has an endpoint outside 0 .. " + std::to_string(n - 1), err, errcap);
  if (int rc = check_finite_image(what, im, n * C, err, errcap)) return rc;
  return guarded(what.c_str(), err, errcap, [&] {
    stereo::DevBuf<double> a, o;
    stereo::DevBuf<uint32_t> cn;
    stereo::DevBuf<int32_t> bad;
    a.upload(im, n * C); cn.upload(conn, (size_t)(2 * E)); o.alloc((size_t)E); bad.alloc(1);
    launch_edges(a.p, H, W, C, cn.p, E, *params, o.p, bad.p, nullptr);
    if (E > 0) STEREO_HIP_CHECK(hipMemcpy(alphas, o.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost));
    else STEREO_HIP_CHECK(hipDeviceSynchronize());
  });
}

int stereo_contrast_step_weights_device(const double *im, int H, int W, int C, const int32_t *directions, int R,
                                        const stereo_contrast_params *params, double *wstep, void *stream, char *err,
                                        size_t errcap) {
  const char *what = "stereo_contrast_step_weights_device";
  Directions dirs;
  if (int rc = check_steps(what, im, H, W, C, directions, R, params, wstep, dirs, err, errcap)) return rc;
  return guarded(what, err, errcap, [&] { launch_steps(im, H, W, C, dirs, R, *params, wstep, (hipStream_t)stream); });
}

int stereo_contrast_step_weights(const double *im, int H, int W, int C, const int32_t *directions, int R,
                                 const stereo_contrast_params *params, double *wstep, char *err, size_t errcap) {
  const std::string what = "stereo_contrast_step_weights";
  Directions dirs;
  if (int rc = check_steps(what, im, H, W, C, directions, R, params, wstep, dirs, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite_image(what, im, n * C, err, errcap)) return rc;
  return guarded(what.c_str(), err, errcap, [&] {
    stereo::DevBuf<double> a, o;
    a.upload(im, n * C); o.alloc(n * R);
    launch_steps(a.p, H, W, C, dirs, R, *params, o.p, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(wstep, o.p, n * R * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
