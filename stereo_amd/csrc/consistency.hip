// Left-right consistency: cross-check of two disparity maps, and the per-row fill of
// the pixels the check rejects.  No reference counterpart.
//
// Maps are H x W column major, element (y, x) at y + H x.  In both kernels the lanes of a wave run
// along y, so a wave reads and writes consecutive addresses whichever column it works on; nothing
// walks memory along a row (stride H).  Neither kernel synchronises across workgroups.
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "common.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;

constexpr int kFillRows = 64;       // rows of one fill workgroup: one per lane
constexpr int kFillMaxChunks = 16;  // waves of one fill workgroup (1024 threads)
constexpr int kFillChunks = 16;     // the largest: every doubling up to 16 still pays (profiles/lr_check_timing.txt)
constexpr int kWalkAhead = 8;       // columns of a walk whose loads are issued together

// ---------------------------------------------------------------- cross-check
//
// One thread per pixel; a block is `blockDim.x` consecutive rows of one column, the grid is (y-tile, x).
// (gridDim.y stops at 65535: a block of a wider map takes every gridDim.y-th column.)
__device__ void lr_check_pixel(const double *__restrict__ d_ref, const double *__restrict__ d_other, int H, int W, int y,
                               int x, int direction, double tol, int32_t *__restrict__ status,
                               double *__restrict__ residual) {
  const size_t i = (size_t)y + (size_t)H * x;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double d = d_ref[i];
  int32_t st;
  double res = nan;
  if (!isfinite(d)) {
    st = 4;
  } else {
    const double xr = direction > 0 ? (double)x - d : (double)x + d;
    const double xf = floor(xr + 0.5);  // nearest column, ties to the higher index
    if (!(xf >= 0.0 && xf <= (double)(W - 1))) {
      st = 3;
    } else {
      const double dr = d_other[(size_t)y + (size_t)H * (int)xf];
      if (!isfinite(dr)) {
        st = 4;
      } else {
        res = d - dr;
        st = fabs(res) <= tol ? 0 : res < 0.0 ? 1 : 2;
      }
    }
  }
  status[i] = st;
  if (residual) residual[i] = res;
}

__global__ void lr_check_kernel(const double *__restrict__ d_ref, const double *__restrict__ d_other, int H, int W,
                                int direction, double tol, int32_t *__restrict__ status, double *__restrict__ residual) {
  const int y = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (y >= H) return;
  for (int64_t x = blockIdx.y; x < W; x += gridDim.y)
    lr_check_pixel(d_ref, d_other, H, W, y, (int)x, direction, tol, status, residual);
}

// ---------------------------------------------------------------- fill
//
// A workgroup takes 64 consecutive rows (lane = row) and `chunks` waves; wave c takes the c-th
// contiguous chunk of columns, chunk c starting at column c * ceil(W / chunks).  Every pixel between two
// neighbouring consistent pixels of a row gets the same answer, so a pixel needs two (column, disparity)
// pairs: the consistent pixel before it and the one after it.
//
//   walk 1, right to left over the chunk, reads `status` and `d_ref` and carries per lane the nearest
//     consistent (column, disparity) to the right.  It writes that pair to `source` and `filled` -- final at
//     a consistent pixel (x, d), tentative elsewhere (-1: none in this chunk) -- and puts the chunk's first
//     and last consistent pair into LDS.
//   one barrier.  Every wave takes as its incoming carries the last pair of the nearest earlier chunk that
//     has one and the first pair of the nearest later chunk that has one.
//   walk 2, left to right, reads `source` and `filled` back (the wave's own stores), carries the last
//     consistent pair, applies the rule and overwrites the pixels that are not consistent.
//
// No load of either walk is at an address that depends on a carry: kWalkAhead columns are issued together.
// Lanes past H and waves whose chunk is empty skip the memory accesses, not the barrier.
__global__ void __launch_bounds__(kFillRows *kFillMaxChunks)
    lr_fill_kernel(const double *__restrict__ d_ref, const int32_t *__restrict__ status, int H, int W,
                   double *__restrict__ filled, int32_t *__restrict__ source) {
  __shared__ int32_t first_col[kFillMaxChunks][kFillRows];
  __shared__ int32_t last_col[kFillMaxChunks][kFillRows];
  __shared__ double first_d[kFillMaxChunks][kFillRows];
  __shared__ double last_d[kFillMaxChunks][kFillRows];
  const int lane = (int)threadIdx.x & (kFillRows - 1);
  const int c = (int)threadIdx.x / kFillRows;
  const int chunks = (int)blockDim.x / kFillRows;
  const int y = (int)blockIdx.x * kFillRows + lane;
  const bool active = y < H;
  const int per = (W + chunks - 1) / chunks;
  const int64_t begin = (int64_t)c * per;
  const int x0 = begin < W ? (int)begin : W;
  const int x1 = begin + per < W ? (int)(begin + per) : W;
  const size_t row = (size_t)(active ? y : 0);
  const size_t Hs = (size_t)H;
  const double nan = std::numeric_limits<double>::quiet_NaN();

  int32_t rcol = -1, lastc = -1;
  double rd = nan, lastd = nan;
  if (active) {
    // (a full group without a predicate on its loads: the compiler keeps them in flight together; a predicated
    //  load gets a wait of its own.  The columns left over go one by one.)
    auto visit = [&](int xx, int32_t s, double d) {
      if (s == 0) {
        rcol = xx;
        rd = d;
        if (lastc < 0) {
          lastc = xx;
          lastd = d;
        }
      }
      source[row + Hs * xx] = rcol;
      filled[row + Hs * xx] = rd;
    };
    int x = x1;
    for (; x - x0 >= kWalkAhead; x -= kWalkAhead) {
      int32_t s[kWalkAhead];
      double d[kWalkAhead];
#pragma unroll
      for (int j = 0; j < kWalkAhead; ++j) {
        s[j] = status[row + Hs * (x - 1 - j)];
        d[j] = d_ref[row + Hs * (x - 1 - j)];
      }
#pragma unroll
      for (int j = 0; j < kWalkAhead; ++j) visit(x - 1 - j, s[j], d[j]);
    }
    for (; x > x0; --x) visit(x - 1, status[row + Hs * (x - 1)], d_ref[row + Hs * (x - 1)]);
  }
  first_col[c][lane] = rcol;
  first_d[c][lane] = rd;
  last_col[c][lane] = lastc;
  last_d[c][lane] = lastd;
  __syncthreads();
  if (!active || x0 >= x1) return;

  int32_t lcol = -1, rin = -1;
  double ld = nan, rin_d = nan;
  for (int k = c - 1; k >= 0 && lcol < 0; --k) {
    lcol = last_col[k][lane];
    ld = last_d[k][lane];
  }
  for (int k = c + 1; k < chunks && rin < 0; ++k) {
    rin = first_col[k][lane];
    rin_d = first_d[k][lane];
  }

  auto visit = [&](int xx, int32_t src, double d) {
    if (src == xx) {
      lcol = xx;
      ld = d;
    } else {
      const int32_t r = src >= 0 ? src : rin;
      const double dr = src >= 0 ? d : rin_d;
      // the smaller disparity (the background); the left one unless the right one is strictly smaller
      const bool take_right = r >= 0 && (lcol < 0 || dr < ld);
      filled[row + Hs * xx] = take_right ? dr : lcol >= 0 ? ld : nan;
      source[row + Hs * xx] = take_right ? r : lcol;
    }
  };
  int x = x0;
  for (; x1 - x >= kWalkAhead; x += kWalkAhead) {
    int32_t src[kWalkAhead];
    double d[kWalkAhead];
#pragma unroll
    for (int j = 0; j < kWalkAhead; ++j) {
      src[j] = source[row + Hs * (x + j)];
      d[j] = filled[row + Hs * (x + j)];
    }
#pragma unroll
    for (int j = 0; j < kWalkAhead; ++j) visit(x + j, src[j], d[j]);
  }
  for (; x < x1; ++x) visit(x, source[row + Hs * x], filled[row + Hs * x]);
}

int check_sizes(const char *what, int H, int W, char *err, size_t errcap) {
  if (H < 1 || W < 1) return fail(std::string(what) + ": H and W must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(std::string(what) + ": H * W must be below 2^31 (columns and pixel counts are int32)", err, errcap);
  return 0;
}

int check_args(const char *what, const void *d_ref, const void *d_other, int H, int W, int direction, double tol,
               const void *status, char *err, size_t errcap) {
  if (!d_ref || !d_other || !status) return fail(std::string(what) + ": d_ref, d_other and status must not be NULL", err, errcap);
  if (direction != 1 && direction != -1) return fail(std::string(what) + ": direction must be +1 or -1", err, errcap);
  if (!(tol >= 0.0)) return fail(std::string(what) + ": tol must be non-negative", err, errcap);
  return check_sizes(what, H, W, err, errcap);
}

int fill_args(const char *what, const void *d_ref, const void *status, int H, int W, const void *filled,
              const void *source_or_null, int chunks,
              char *err, size_t errcap) {
  if (!d_ref || !status || !filled) return fail(std::string(what) + ": d_ref, status and filled must not be NULL", err, errcap);
  // walk 1 writes tentative values to filled / source while other waves still read d_ref / status
  if (filled == d_ref) return fail(std::string(what) + ": filled must not be d_ref (the fill does not work in place)", err, errcap);
  if (status == (const void *)source_or_null) return fail(std::string(what) + ": source must not be status (the fill does not work in place)", err, errcap);
  if (chunks < 1 || chunks > kFillMaxChunks) return fail(std::string(what) + ": chunks must be 1 .. " + std::to_string(kFillMaxChunks), err, errcap);
  return check_sizes(what, H, W, err, errcap);
}

void launch_check(const double *d_ref, const double *d_other, int H, int W, int direction, double tol, int32_t *status,
                  double *residual, hipStream_t s) {
  const int tb = H <= 64 ? 64 : 256;
  const unsigned ytiles = (unsigned)((H + tb - 1) / tb);
  hipLaunchKernelGGL(lr_check_kernel, dim3(ytiles, (unsigned)(W < 65535 ? W : 65535)), dim3(tb), 0, s, d_ref, d_other, H, W,
                     direction, tol, status, residual);
  STEREO_HIP_CHECK(hipGetLastError());
}

// `source` doubles as walk 1's output; a caller that does not want it gets a scratch array in its place
void launch_fill(const double *d_ref, const int32_t *status, int H, int W, double *filled, int32_t *source, int chunks,
                 hipStream_t s) {
  stereo::StreamBuf<int32_t> scratch;
  if (!source) {
    scratch.alloc((size_t)H * W, s);
    source = scratch.p;
  }
  hipLaunchKernelGGL(lr_fill_kernel, dim3((unsigned)((H + kFillRows - 1) / kFillRows)), dim3(kFillRows * chunks), 0, s, d_ref,
                     status, H, W, filled, source);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_lr_fill_chunks(void) { return kFillChunks; }

int stereo_lr_check_device(const double *d_ref, const double *d_other, int H, int W, int direction, double tol,
                           int32_t *status, double *residual, void *stream, char *err, size_t errcap) {
  if (int rc = check_args("stereo_lr_check_device", d_ref, d_other, H, W, direction, tol, status, err, errcap)) return rc;
  return guarded("stereo_lr_check_device", err, errcap,
                 [&] { launch_check(d_ref, d_other, H, W, direction, tol, status, residual, (hipStream_t)stream); });
}

int stereo_lr_fill_device_chunks(const double *d_ref, const int32_t *status, int H, int W, double *filled, int32_t *source,
                                 int chunks, void *stream, char *err, size_t errcap) {
  if (int rc = fill_args("stereo_lr_fill_device", d_ref, status, H, W, filled, source, chunks, err, errcap)) return rc;
  return guarded("stereo_lr_fill_device", err, errcap,
                 [&] { launch_fill(d_ref, status, H, W, filled, source, chunks, (hipStream_t)stream); });
}

int stereo_lr_fill_device(const double *d_ref, const int32_t *status, int H, int W, double *filled, int32_t *source,
                          void *stream, char *err, size_t errcap) {
  return stereo_lr_fill_device_chunks(d_ref, status, H, W, filled, source, kFillChunks, stream, err, errcap);
}

int stereo_lr_check(const double *d_ref, const double *d_other, int H, int W, int direction, double tol, int32_t *status,
                    double *residual, char *err, size_t errcap) {
  if (int rc = check_args("stereo_lr_check", d_ref, d_other, H, W, direction, tol, status, err, errcap)) return rc;
  return guarded("stereo_lr_check", err, errcap, [&] {
    const size_t n = (size_t)H * W;
    stereo::DevBuf<double> a, b, res;
    stereo::DevBuf<int32_t> st;
    a.upload(d_ref, n); b.upload(d_other, n); st.alloc(n);
    if (residual) res.alloc(n);
    launch_check(a.p, b.p, H, W, direction, tol, st.p, residual ? res.p : nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(status, st.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (residual) STEREO_HIP_CHECK(hipMemcpy(residual, res.p, n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int stereo_lr_fill(const double *d_ref, const int32_t *status, int H, int W, double *filled, int32_t *source, char *err,
                   size_t errcap) {
  if (int rc = fill_args("stereo_lr_fill", d_ref, status, H, W, filled, source, kFillChunks, err, errcap)) return rc;
  return guarded("stereo_lr_fill", err, errcap, [&] {
    const size_t n = (size_t)H * W;
    stereo::DevBuf<double> a, out;
    stereo::DevBuf<int32_t> st, src;
    a.upload(d_ref, n); st.upload(status, n); out.alloc(n); src.alloc(n);
    launch_fill(a.p, st.p, H, W, out.p, src.p, kFillChunks, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(filled, out.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (source) STEREO_HIP_CHECK(hipMemcpy(source, src.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
