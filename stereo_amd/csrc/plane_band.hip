// Band refinement around a solved plane map (the definition: include/stereo_hip.h).
// From the 4 x N planes of an assignment and K offsets, the TRW-S inputs of the problem whose label k at pixel i
// means pixel i's own plane moved by offsets_k along the disparity axis, [a_i b_i c_i d_i - c_i offsets_k]:
// unary (K x N) by the NCC sampler (ncc_sample.h) or by the photo-consistency term of dispmap_globalstereo
// (gs_sample.h), q / qprim (K x E) by the plane -> disparity rule with the rescaling of stereo_trws_positions,
// and the planes a labelling selects.
//
// The layout is band.hip's, and the index, the launch sizes, the argument checks, the scans of a host entry's arrays
// and HostOutputs are the shared ones of band_common.h: the outputs are label fastest, a lane is one (pixel, k) or
// (edge, k) element of them in storage order (every wave stores 512 consecutive bytes), and the 64-bit division by K is
// done once per block on uniform values.  The K lanes of a pixel or an edge read the same planes, so those come from cache.  A pixel's
// point is [id / H + 1, id % H + 1], formed in the kernel; no points array is read.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "band_common.h"
#include "common.h"
#include "stereo_hip.h"
#include "unary_source.h"

namespace {

using stereo::fail;
using stereo::guarded;
using namespace stereo::band;   // band_common.h: the indices, the launch sizes, every check and scan, HostOutputs; the sources

// The plane of label k at a pixel: one fp64 multiplication and one fp64 subtraction (no contraction: the file is
// compiled with -ffp-contract=off).
__device__ __forceinline__ double shifted_d(double c, double d, double delta) { return d - c * delta; }

__device__ __forceinline__ bool plane_ok(double a, double b, double c, double d) {
  return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d) && c != 0.0;
}

// The two unary sources, NccSource<kStageSlices> and GsSource: unary_source.h.

template <class Source>
__global__ __launch_bounds__(kTB) void plane_band_unary_kernel(Source src, int H, int64_t Npx, const double *__restrict__ planes,
                                                              const double *__restrict__ offsets, int K,
                                                              double *__restrict__ U, int32_t *bad) {
  extern __shared__ double plane_band_lds[];
  const double *prepared = src.begin(plane_band_lds);
  const int64_t total = Npx * K;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, K);
    if (ix.item >= Npx) continue;
    const double *pl = planes + 4 * ix.item;
    const double a = pl[0], b = pl[1], c = pl[2], d = pl[3];
    if (bad && ix.k == 0 && !plane_ok(a, b, c, d)) atomicAdd(bad, 1);
    const uint32_t id = (uint32_t)ix.item, col = id / (uint32_t)H;      // (Npx < 2^31)
    const double x = (double)(col + 1), y = (double)(id - col * (uint32_t)H + 1);
    const double sh[4] = {a, b, c, shifted_d(c, d, offsets[ix.k])};
    U[first + threadIdx.x] = src.at(prepared, H, Npx, ix.item, x, y, stereo::plane_disp(sh, x, y));
  }
}

// q(k, e) = the shifted plane of the edge's second pixel at that pixel's point, qprim(k, e) = the shifted plane of its
// first pixel at the same point (dispmap_super.m:177-183, the order trws_positions_kernel writes), rescaled by
// (v - d_min) / d_step when d_step != 0.  An edge that names a pixel outside 0 .. N - 1 reads nothing and gets NaN.
// This kernel writes 16 of every 18 bytes of a band problem.  As band_positions_kernel: a block takes
// kPosPerThread * 256 consecutive elements, a thread kPosPerThread of them 256 apart; every load is unconditional at
// a clamped address, so the loads of a thread's elements are in flight together, and only the stores are predicated.
// Two elements per thread, not the band's four: an element holds two planes (16 VGPRs) where the band holds two
// doubles, and four of them cost half the waves per SIMD (DESIGN.md 6.3 has the measurement; the flag is for it).
#ifndef PLANE_BAND_POS_PER_THREAD
#define PLANE_BAND_POS_PER_THREAD 2
#endif
constexpr int kPosPerThread = PLANE_BAND_POS_PER_THREAD;
__global__ __launch_bounds__(kTB) void plane_band_positions_kernel(int64_t E, int K, int H, int64_t Npx,
                                                                  const uint32_t *__restrict__ conn,
                                                                  const double *__restrict__ planes,
                                                                  const double *__restrict__ offsets, double d_min,
                                                                  double d_step, double *__restrict__ q,
                                                                  double *__restrict__ qprim) {
  const int64_t total = E * K;
  constexpr int64_t kChunk = (int64_t)kTB * kPosPerThread;
  const double nan = __builtin_nan("");
  for (int64_t first = (int64_t)blockIdx.x * kChunk; first < total; first += (int64_t)gridDim.x * kChunk) {
    const int64_t item0 = first / K;                       // (uniform: once per block and chunk)
    const uint32_t rem0 = (uint32_t)(first - item0 * K);
    uint32_t i1[kPosPerThread], i2[kPosPerThread];
    double delta[kPosPerThread], p1[kPosPerThread][4], p2[kPosPerThread][4];
    bool live[kPosPerThread];
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      const uint32_t off = (uint32_t)u * kTB + threadIdx.x;
      live[u] = first + off < total;
      const uint32_t local = rem0 + off, up = local / (uint32_t)K;
      const int64_t e = live[u] ? item0 + up : 0;
      i1[u] = conn[2 * e];
      i2[u] = conn[2 * e + 1];
      delta[u] = offsets[local - up * (uint32_t)K];
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      const double *a1 = planes + 4 * (size_t)(i1[u] < Npx ? i1[u] : 0);
      const double *a2 = planes + 4 * (size_t)(i2[u] < Npx ? i2[u] : 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) { p1[u][j] = a1[j]; p2[u][j] = a2[j]; }
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      if (!live[u]) continue;
      const int64_t t = first + (int64_t)u * kTB + threadIdx.x;
      const bool named = i1[u] < Npx && i2[u] < Npx;
      const uint32_t id = named ? i2[u] : 0, col = id / (uint32_t)H;
      const double x = (double)(col + 1), y = (double)(id - col * (uint32_t)H + 1);
      p1[u][3] = shifted_d(p1[u][2], p1[u][3], delta[u]);
      p2[u][3] = shifted_d(p2[u][2], p2[u][3], delta[u]);
      double v = stereo::plane_disp(p2[u], x, y), vp = stereo::plane_disp(p1[u], x, y);
      if (d_step != 0) { v = (v - d_min) / d_step; vp = (vp - d_min) / d_step; }
      q[t] = named ? v : nan;
      qprim[t] = named ? vp : nan;
    }
  }
}

// refined_i = [a_i b_i c_i d_i - c_i offsets_{label_i - 1}]; a label outside 1 .. K, or a plane that is not finite or
// has c == 0, gives four NaN and counts in `bad`.
__global__ __launch_bounds__(kTB) void plane_band_apply_kernel(int64_t Npx, int K, const double *__restrict__ planes,
                                                              const int32_t *__restrict__ labels,
                                                              const double *__restrict__ offsets,
                                                              double *__restrict__ refined, int32_t *bad) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < Npx; i += (int64_t)gridDim.x * kTB) {
    const int32_t l = labels[i];
    const double *pl = planes + 4 * i;
    const double a = pl[0], b = pl[1], c = pl[2], d = pl[3];
    const bool in = l >= 1 && l <= K;
    const bool ok = in && plane_ok(a, b, c, d);
    if (bad && !ok) atomicAdd(bad, 1);
    const double moved = shifted_d(c, d, offsets[in ? l - 1 : 0]);
    double *out = refined + 4 * i;
    out[0] = ok ? a : nan; out[1] = ok ? b : nan; out[2] = ok ? c : nan; out[3] = ok ? moved : nan;
  }
}

// ---------------------------------------------------------------- argument checks (no device call)

// the part of an inputs entry's checks that does not depend on the unary source
int check_band(const std::string &what, int H, int W, const void *planes, const double *offsets, int K, int64_t E,
               const void *conn, const void *unary, const void *q, const void *qprim, char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (int rc = check_edges(what, E, conn, q, qprim, err, errcap)) return rc;
  if (!planes || !unary) return fail(what + ": planes and unary must not be NULL", err, errcap);
  return check_offsets(what, offsets, K, err, errcap);
}

int check_apply(const std::string &what, const void *planes, int64_t N, const void *labels, const double *offsets, int K,
                const void *refined, char *err, size_t errcap) {
  if (N < 1) return fail(what + ": N must be at least 1", err, errcap);
  if (N >= ((int64_t)1 << 31)) return fail(what + ": N must be below 2^31", err, errcap);
  if (!planes || !labels || !refined) return fail(what + ": planes, labels and refined must not be NULL", err, errcap);
  return check_offsets(what, offsets, K, err, errcap);
}

void launch_positions(int H, int64_t Npx, const double *planes, const double *d_offsets, int K, int64_t E, const uint32_t *conn,
                      double d_min, double d_step, double *q, double *qprim, hipStream_t s) {
  if (E <= 0) return;
  hipLaunchKernelGGL(plane_band_positions_kernel, dim3(grid_for((E * K + kPosPerThread - 1) / kPosPerThread)), dim3(kTB), 0, s, E,
                     K, H, Npx, conn, planes, d_offsets, d_min, d_step, q, qprim);
  STEREO_HIP_CHECK(hipGetLastError());
}

// `disparities`: the host vector (min, max and the order of the slices come from it); `d_disparities` / `d_offsets`:
// the short vectors in device memory, which the kernels read
void launch_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities, const double *d_disparities,
                double unary_weight, const double *planes, const double *d_offsets, int K, int64_t E, const uint32_t *conn,
                double *unary, double *q, double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  const SliceRange r = slice_range(disparities, D);
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (D <= kMaxStagedSlices) {
    const NccSource<true> src{ncc, D, layout, d_disparities, r.dmin, r.dmax, unary_weight, r.ascending};
    hipLaunchKernelGGL(plane_band_unary_kernel<NccSource<true>>, dim3(grid_for(Npx * K)), dim3(kTB), (size_t)D * sizeof(double), s,
                       src, H, Npx, planes, d_offsets, K, unary, bad);
  } else {
    const NccSource<false> src{ncc, D, layout, d_disparities, r.dmin, r.dmax, unary_weight, r.ascending};
    hipLaunchKernelGGL(plane_band_unary_kernel<NccSource<false>>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, src, H, Npx, planes,
                       d_offsets, K, unary, bad);
  }
  STEREO_HIP_CHECK(hipGetLastError());
  launch_positions(H, Npx, planes, d_offsets, K, E, conn, 0.0, 0.0, q, qprim, s);
}

void launch_gs(const double *im0, const double *im1, int H, int W, int C, const double *P2, double d_min, double d_step,
               double col_thresh, const double *planes, const double *d_offsets, int K, int64_t E, const uint32_t *conn,
               double *unary, double *q, double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  GsSource src{im0, im1, W, C, {}, d_min, d_step, col_thresh};
  std::memcpy(src.P2, P2, sizeof(src.P2));
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(plane_band_unary_kernel<GsSource>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, src, H, Npx, planes, d_offsets, K,
                     unary, bad);
  STEREO_HIP_CHECK(hipGetLastError());
  launch_positions(H, Npx, planes, d_offsets, K, E, conn, d_min, d_step, q, qprim, s);
}

void launch_apply(const double *planes, int64_t N, const int32_t *labels, const double *d_offsets, int K, double *refined,
                  int32_t *bad, hipStream_t s) {
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(plane_band_apply_kernel, dim3(grid_for(N)), dim3(kTB), 0, s, N, K, planes, labels, d_offsets, refined, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_plane_band_inputs_ncc_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                        const double *d_disparities, double unary_weight, const double *planes,
                                        const double *offsets, const double *d_offsets, int K, int64_t E, const uint32_t *conn,
                                        double *unary, double *q, double *qprim, int32_t *bad, void *stream, char *err,
                                        size_t errcap) {
  const char *what = "stereo_plane_band_inputs_ncc_device";
  if (int rc = check_band(what, H, W, planes, offsets, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  if (!d_disparities || !d_offsets) return fail(std::string(what) + ": d_disparities and d_offsets must not be NULL", err, errcap);
  return guarded(what, err, errcap, [&] {
    launch_ncc(ncc, H, W, D, layout, disparities, d_disparities, unary_weight, planes, d_offsets, K, E, conn, unary, q, qprim, bad,
               (hipStream_t)stream);
  });
}

int stereo_plane_band_inputs_globalstereo_device(const double *im0, const double *im1, int H, int W, int C, const double *P2,
                                                 double d_min, double d_step, double col_thresh, const double *planes,
                                                 const double *offsets, const double *d_offsets, int K, int64_t E,
                                                 const uint32_t *conn, double *unary, double *q, double *qprim, int32_t *bad,
                                                 void *stream, char *err, size_t errcap) {
  const char *what = "stereo_plane_band_inputs_globalstereo_device";
  if (int rc = check_band(what, H, W, planes, offsets, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_gs(what, im0, im1, C, P2, d_step, err, errcap)) return rc;
  if (!d_offsets) return fail(std::string(what) + ": d_offsets must not be NULL", err, errcap);
  return guarded(what, err, errcap, [&] {
    launch_gs(im0, im1, H, W, C, P2, d_min, d_step, col_thresh, planes, d_offsets, K, E, conn, unary, q, qprim, bad,
              (hipStream_t)stream);
  });
}

int stereo_plane_band_apply_device(const double *planes, int64_t N, const int32_t *labels, const double *offsets,
                                   const double *d_offsets, int K, double *refined, int32_t *bad, void *stream, char *err,
                                   size_t errcap) {
  const char *what = "stereo_plane_band_apply_device";
  if (int rc = check_apply(what, planes, N, labels, offsets, K, refined, err, errcap)) return rc;
  if (!d_offsets) return fail(std::string(what) + ": d_offsets must not be NULL", err, errcap);
  return guarded(what, err, errcap, [&] { launch_apply(planes, N, labels, d_offsets, K, refined, bad, (hipStream_t)stream); });
}

int stereo_plane_band_inputs_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                 double unary_weight, const double *planes, const double *offsets, int K, int64_t E,
                                 const uint32_t *conn, double *unary, double *q, double *qprim, char *err, size_t errcap) {
  const std::string what = "stereo_plane_band_inputs_ncc";
  if (int rc = check_band(what, H, W, planes, offsets, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "", planes, (int64_t)n, H, 0, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_plane_band_inputs_ncc", err, errcap, [&] {
    stereo::DevBuf<double> dn, dp, dd, doff;
    dn.upload(ncc, n * D); dp.upload(planes, 4 * n); dd.upload(disparities, D); doff.upload(offsets, K);
    HostOutputs out(n, K, E, conn);
    launch_ncc(dn.p, H, W, D, layout, disparities, dd.p, unary_weight, dp.p, doff.p, K, E, out.dc.p, out.du.p, out.dq.p, out.dqp.p,
               nullptr, nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_plane_band_inputs_globalstereo(const double *im0, const double *im1, int H, int W, int C, const double *P2,
                                          double d_min, double d_step, double col_thresh, const double *planes,
                                          const double *offsets, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
                                          double *qprim, char *err, size_t errcap) {
  const std::string what = "stereo_plane_band_inputs_globalstereo";
  if (int rc = check_band(what, H, W, planes, offsets, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_gs(what, im0, im1, C, P2, d_step, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "", planes, (int64_t)n, H, 0, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_plane_band_inputs_globalstereo", err, errcap, [&] {
    stereo::DevBuf<double> d0, d1, dp, doff;
    d0.upload(im0, n * C); d1.upload(im1, n * C); dp.upload(planes, 4 * n); doff.upload(offsets, K);
    HostOutputs out(n, K, E, conn);
    launch_gs(d0.p, d1.p, H, W, C, P2, d_min, d_step, col_thresh, dp.p, doff.p, K, E, out.dc.p, out.du.p, out.dq.p, out.dqp.p, nullptr,
              nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_plane_band_apply(const double *planes, int64_t N, const int32_t *labels, const double *offsets, int K,
                            double *refined, char *err, size_t errcap) {
  const std::string what = "stereo_plane_band_apply";
  if (int rc = check_apply(what, planes, N, labels, offsets, K, refined, err, errcap)) return rc;
  if (int rc = check_planes(what, "", planes, N, 0, 0, err, errcap)) return rc;
  if (int rc = check_labels(what, labels, (size_t)N, K, err, errcap)) return rc;
  return guarded("stereo_plane_band_apply", err, errcap, [&] {
    stereo::DevBuf<double> dp, doff, out;
    stereo::DevBuf<int32_t> dl;
    dp.upload(planes, 4 * (size_t)N); dl.upload(labels, (size_t)N); doff.upload(offsets, K); out.alloc(4 * (size_t)N);
    launch_apply(dp.p, N, dl.p, doff.p, K, out.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(refined, out.p, 4 * (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
