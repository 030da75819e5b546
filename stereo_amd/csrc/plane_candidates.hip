// Plane candidates: per-pixel plane sets propagated from neighbours (the definition:
// include/stereo_hip.h).  A plane candidate table `pcand` (4 x K x N, component fastest, then label, then pixel)
// says what label k means at pixel i: a plane [a b c d] of its own.  gather builds the table from the planes of an
// assignment, the band's offsets and M source plane maps read at T taps; inputs makes the TRW-S problem of ANY table
// -- unary by the NCC sampler or the photo-consistency term (unary_source.h), q / qprim by the plane -> disparity rule
// with the rescaling of stereo_trws_positions -- and apply reads the planes a labelling selects.
//
// The lane mapping is the band's (band.hip): a lane is one (pixel, k) or (edge, k) element in storage order, the
// 64-bit division by K is done once per block on uniform values; the index, the clamp of a tap (tapped_pixel), the
// launch sizes, slice_range(), the argument checks but the alignment, the scans of a host entry's arrays and
// HostOutputs are in band_common.h.  A plane is 32 contiguous bytes and moves as two
// 16-byte accesses; a wave of the gather stores 2 KiB in a row.  A pixel's point is [id / H + 1, id % H + 1], formed
// in the kernel.
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

// one plane in registers: [a b] and [c d], each a 16-byte access
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
__device__ __forceinline__ double disp_of(const Plane &p, double x, double y) {
  const double pl[4] = {p.ab.x, p.ab.y, p.cd.x, p.cd.y};
  return stereo::plane_disp(pl, x, y);
}

// pcand[:, k, i] = [a_i b_i c_i d_i - c_i offsets_k] for k < Ko (the plane band's label: one fp64 multiplication, one
// fp64 subtraction; the file is compiled with -ffp-contract=off);
// pcand[:, Ko + m T + t, (y, x)] = src_m[:, clamp(y + dy_t), clamp(x + dx_t)], the four doubles copied.
// `bad` counts the pixels at which the own plane or a source's plane is not finite or has c == 0 (the lane k == 0 of
// the pixel looks).
__global__ __launch_bounds__(kTB) void plane_candidates_gather_kernel(int64_t Npx, int H, int W, const double *__restrict__ planes,
                                                                     const double *__restrict__ offsets, int Ko,
                                                                     const double *__restrict__ sources, int M,
                                                                     const int32_t *__restrict__ taps, int T,
                                                                     double *__restrict__ pcand, int32_t *bad) {
  const int K = Ko + M * T;
  const int64_t total = Npx * K;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, K);
    if (ix.item >= Npx) continue;
    if (bad && ix.k == 0) {
      bool ok = plane_ok(load_plane(planes + 4 * ix.item));
      if (T > 0)
        for (int m = 0; m < M; ++m) ok = ok && plane_ok(load_plane(sources + 4 * ((int64_t)m * Npx + ix.item)));
      if (!ok) atomicAdd(bad, 1);
    }
    Plane p;
    if (ix.k < Ko) {
      p = load_plane(planes + 4 * ix.item);
      p.cd.y = p.cd.y - p.cd.x * offsets[ix.k];
    } else {
      const int j = ix.k - Ko, m = j / T, t = j - m * T;
      p = load_plane(sources + 4 * ((int64_t)m * Npx + tapped_pixel(ix.item, H, W, taps, t)));
    }
    store_plane(pcand + 4 * (first + threadIdx.x), p);
  }
}

// unary(k, i) = the source's unary of pixel i for the disparity of plane pcand[:, k, i] at the pixel's own point.
// `bad` counts the pixels with a candidate that is not finite or has c == 0: a lane tests the plane it has loaded
// anyway, and only a lane that finds one looks at the pixel's lower labels to see whether it is the first
// (DESIGN.md 6.7 has the measurement that chose this over a loop in the lane k == 0).
template <class Source>
__global__ __launch_bounds__(kTB) void plane_candidates_unary_kernel(Source src, int H, int64_t Npx,
                                                                    const double *__restrict__ pcand, int K,
                                                                    double *__restrict__ U, int32_t *bad) {
  extern __shared__ double plane_candidates_lds[];
  const double *prepared = src.begin(plane_candidates_lds);
  const int64_t total = Npx * K;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, K);
    if (ix.item >= Npx) continue;
    const int64_t t = first + threadIdx.x;
    const Plane p = load_plane(pcand + 4 * t);
    if (bad && !plane_ok(p)) {     // (rare) the pixel counts once: at its first label that offends
      bool first_of_pixel = true;
      for (int k = 0; k < ix.k; ++k) first_of_pixel = first_of_pixel && plane_ok(load_plane(pcand + 4 * (t - ix.k + k)));
      if (first_of_pixel) atomicAdd(bad, 1);
    }
    const uint32_t id = (uint32_t)ix.item, col = id / (uint32_t)H;      // (Npx < 2^31)
    const double x = (double)(col + 1), y = (double)(id - col * (uint32_t)H + 1);
    U[t] = src.at(prepared, H, Npx, ix.item, x, y, disp_of(p, x, y));
  }
}

// q(k, e) = plane pcand[:, k, i2] at the point of i2, qprim(k, e) = plane pcand[:, k, i1] at the same point
// (dispmap_super.m:177-183, the order trws_positions_kernel writes), rescaled by (v - d_min) / d_step when
// d_step != 0.  An edge that names a pixel outside 0 .. N - 1 reads pixel 0 and gets NaN.  This kernel writes 16 of
// every 18 bytes of a problem.  The shape of plane_band_positions_kernel: a block takes kPosPerThread * 256
// consecutive elements, a thread kPosPerThread of them 256 apart; every load is unconditional at a clamped address,
// so the loads of a thread's elements are in flight together, and only the stores are predicated.  Unlike the plane
// band's K lanes, which share two planes from cache, every element loads two planes of its own: 64 bytes read per
// 16 stored (the K lanes of an edge read 32 K contiguous bytes per endpoint).  One element per thread, not the plane
// band's two: with 1, 2 and 4 the kernel took 3489, 3830 and 3751 us at 2000 x 3000, K = 17, and the three lie within
// 6 % of each other elsewhere (36 / 56 / 94 VGPRs, 8 / 8 / 5 waves per SIMD; DESIGN.md 6.8 has the measurement; the
// flag is for it).
#ifndef PLANE_CAND_POS_PER_THREAD
#define PLANE_CAND_POS_PER_THREAD 1
#endif
constexpr int kPosPerThread = PLANE_CAND_POS_PER_THREAD;
__global__ __launch_bounds__(kTB) void plane_candidates_positions_kernel(int64_t E, int K, int H, int64_t Npx,
                                                                        const uint32_t *__restrict__ conn,
                                                                        const double *__restrict__ pcand, double d_min,
                                                                        double d_step, double *__restrict__ q,
                                                                        double *__restrict__ qprim) {
  const int64_t total = E * K;
  constexpr int64_t kChunk = (int64_t)kTB * kPosPerThread;
  const double nan = __builtin_nan("");
  for (int64_t first = (int64_t)blockIdx.x * kChunk; first < total; first += (int64_t)gridDim.x * kChunk) {
    const int64_t item0 = first / K;                       // (uniform: once per block and chunk)
    const uint32_t rem0 = (uint32_t)(first - item0 * K);
    uint32_t i1[kPosPerThread], i2[kPosPerThread], k[kPosPerThread];
    Plane p1[kPosPerThread], p2[kPosPerThread];
    bool live[kPosPerThread];
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      const uint32_t off = (uint32_t)u * kTB + threadIdx.x;
      live[u] = first + off < total;
      const uint32_t local = rem0 + off, up = local / (uint32_t)K;
      const int64_t e = live[u] ? item0 + up : 0;
      i1[u] = conn[2 * e];
      i2[u] = conn[2 * e + 1];
      k[u] = local - up * (uint32_t)K;
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      p1[u] = load_plane(pcand + 4 * ((int64_t)(i1[u] < Npx ? i1[u] : 0) * K + k[u]));
      p2[u] = load_plane(pcand + 4 * ((int64_t)(i2[u] < Npx ? i2[u] : 0) * K + k[u]));
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      if (!live[u]) continue;
      const int64_t t = first + (int64_t)u * kTB + threadIdx.x;
      const bool named = i1[u] < Npx && i2[u] < Npx;
      const uint32_t id = named ? i2[u] : 0, col = id / (uint32_t)H;
      const double x = (double)(col + 1), y = (double)(id - col * (uint32_t)H + 1);
      double v = disp_of(p2[u], x, y), vp = disp_of(p1[u], x, y);
      if (d_step != 0) { v = (v - d_min) / d_step; vp = (vp - d_min) / d_step; }
      q[t] = named ? v : nan;
      qprim[t] = named ? vp : nan;
    }
  }
}

// out[:, i] = pcand[:, label_i - 1, i], copied; a label outside 1 .. K gives four NaN and counts in `bad`.
__global__ __launch_bounds__(kTB) void plane_candidates_apply_kernel(int64_t Npx, int K, const double *__restrict__ pcand,
                                                                    const int32_t *__restrict__ labels,
                                                                    double *__restrict__ out, int32_t *bad) {
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < Npx; i += (int64_t)gridDim.x * kTB) {
    const int32_t l = labels[i];
    const bool in = l >= 1 && l <= K;
    if (bad && !in) atomicAdd(bad, 1);
    Plane p = load_plane(pcand + 4 * (i * K + (in ? l - 1 : 0)));
    if (!in) { p.ab.x = nan; p.ab.y = nan; p.cd.x = nan; p.cd.y = nan; }
    store_plane(out + 4 * i, p);
  }
}

// ---------------------------------------------------------------- argument checks (no device call)

// the part of an inputs entry's checks that does not depend on the unary source
int check_inputs(const std::string &what, int H, int W, const void *pcand, int K, int64_t E, const void *conn, const void *unary,
                 const void *q, const void *qprim, char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (int rc = check_edges(what, E, conn, q, qprim, err, errcap)) return rc;
  if (!pcand || !unary) return fail(what + ": pcand and unary must not be NULL", err, errcap);
  return check_k(what, K, err, errcap);
}

int check_apply(const std::string &what, const void *pcand, int H, int W, int K, const void *labels, const void *out, char *err,
                size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (!pcand || !labels || !out) return fail(what + ": pcand, labels and out must not be NULL", err, errcap);
  return check_k(what, K, err, errcap);
}

// the device forms move a plane as two 16-byte accesses
int check_aligned(const std::string &what, const char *name, const void *p, char *err, size_t errcap) {
  if (((uintptr_t)p & 15) != 0) return fail(what + ": " + name + " must be 16-byte aligned", err, errcap);
  return 0;
}

// ---------------------------------------------------------------- launches

void launch_gather(const double *planes, int H, int W, const double *d_offsets, int Ko, const double *sources, int M,
                   const int32_t *d_taps, int T, double *pcand, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(plane_candidates_gather_kernel, dim3(grid_for(Npx * (Ko + M * T))), dim3(kTB), 0, s, Npx, H, W, planes,
                     d_offsets, Ko, sources, M, d_taps, T, pcand, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_positions(int H, int64_t Npx, const double *pcand, int K, int64_t E, const uint32_t *conn, double d_min, double d_step,
                      double *q, double *qprim, hipStream_t s) {
  if (E <= 0) return;
  hipLaunchKernelGGL(plane_candidates_positions_kernel, dim3(grid_for((E * K + kPosPerThread - 1) / kPosPerThread)), dim3(kTB), 0, s,
                     E, K, H, Npx, conn, pcand, d_min, d_step, q, qprim);
  STEREO_HIP_CHECK(hipGetLastError());
}

// `disparities`: the host vector (min, max and the order of the slices come from it); `d_disparities`: the same in
// device memory, which the kernel reads
void launch_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities, const double *d_disparities,
                double unary_weight, const double *pcand, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
                double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  const SliceRange r = slice_range(disparities, D);
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (D <= kMaxStagedSlices) {
    const NccSource<true> src{ncc, D, layout, d_disparities, r.dmin, r.dmax, unary_weight, r.ascending};
    hipLaunchKernelGGL(plane_candidates_unary_kernel<NccSource<true>>, dim3(grid_for(Npx * K)), dim3(kTB),
                       (size_t)D * sizeof(double), s, src, H, Npx, pcand, K, unary, bad);
  } else {
    const NccSource<false> src{ncc, D, layout, d_disparities, r.dmin, r.dmax, unary_weight, r.ascending};
    hipLaunchKernelGGL(plane_candidates_unary_kernel<NccSource<false>>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, src, H, Npx,
                       pcand, K, unary, bad);
  }
  STEREO_HIP_CHECK(hipGetLastError());
  launch_positions(H, Npx, pcand, K, E, conn, 0.0, 0.0, q, qprim, s);
}

void launch_gs(const double *im0, const double *im1, int H, int W, int C, const double *P2, double d_min, double d_step,
               double col_thresh, const double *pcand, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
               double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  GsSource src{im0, im1, W, C, {}, d_min, d_step, col_thresh};
  std::memcpy(src.P2, P2, sizeof(src.P2));
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(plane_candidates_unary_kernel<GsSource>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, src, H, Npx, pcand, K,
                     unary, bad);
  STEREO_HIP_CHECK(hipGetLastError());
  launch_positions(H, Npx, pcand, K, E, conn, d_min, d_step, q, qprim, s);
}

void launch_apply(const double *pcand, int H, int W, int K, const int32_t *labels, double *out, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(plane_candidates_apply_kernel, dim3(grid_for(Npx)), dim3(kTB), 0, s, Npx, K, pcand, labels, out, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_plane_candidates_gather_device(const double *planes, int H, int W, const double *offsets, const double *d_offsets,
                                          int Ko, const double *sources, int M, const int32_t *taps, const int32_t *d_taps,
                                          int T, double *pcand, int32_t *bad, void *stream, char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_gather_device";
  if (int rc = check_gather(what, "planes", "pcand", planes, H, W, offsets, Ko, sources, M, taps, T, pcand, err, errcap)) return rc;
  if (!d_offsets) return fail(what + ": d_offsets must not be NULL", err, errcap);
  const bool taken = (int64_t)M * T > 0;
  if (taken && !d_taps) return fail(what + ": d_taps must not be NULL when M * T > 0", err, errcap);
  if (int rc = check_aligned(what, "planes", planes, err, errcap)) return rc;
  if (int rc = check_aligned(what, "pcand", pcand, err, errcap)) return rc;
  if (taken)
    if (int rc = check_aligned(what, "sources", sources, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_gather_device", err, errcap,
                 [&] { launch_gather(planes, H, W, d_offsets, Ko, sources, M, d_taps, T, pcand, bad, (hipStream_t)stream); });
}

int stereo_plane_candidates_inputs_ncc_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                              const double *d_disparities, double unary_weight, const double *pcand, int K,
                                              int64_t E, const uint32_t *conn, double *unary, double *q, double *qprim,
                                              int32_t *bad, void *stream, char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_inputs_ncc_device";
  if (int rc = check_inputs(what, H, W, pcand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  if (!d_disparities) return fail(what + ": d_disparities must not be NULL", err, errcap);
  if (int rc = check_aligned(what, "pcand", pcand, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_inputs_ncc_device", err, errcap, [&] {
    launch_ncc(ncc, H, W, D, layout, disparities, d_disparities, unary_weight, pcand, K, E, conn, unary, q, qprim, bad,
               (hipStream_t)stream);
  });
}

int stereo_plane_candidates_inputs_globalstereo_device(const double *im0, const double *im1, int H, int W, int C,
                                                       const double *P2, double d_min, double d_step, double col_thresh,
                                                       const double *pcand, int K, int64_t E, const uint32_t *conn,
                                                       double *unary, double *q, double *qprim, int32_t *bad, void *stream,
                                                       char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_inputs_globalstereo_device";
  if (int rc = check_inputs(what, H, W, pcand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_gs(what, im0, im1, C, P2, d_step, err, errcap)) return rc;
  if (int rc = check_aligned(what, "pcand", pcand, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_inputs_globalstereo_device", err, errcap, [&] {
    launch_gs(im0, im1, H, W, C, P2, d_min, d_step, col_thresh, pcand, K, E, conn, unary, q, qprim, bad, (hipStream_t)stream);
  });
}

int stereo_plane_candidates_apply_device(const double *pcand, int H, int W, int K, const int32_t *labels, double *out,
                                         int32_t *bad, void *stream, char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_apply_device";
  if (int rc = check_apply(what, pcand, H, W, K, labels, out, err, errcap)) return rc;
  if (int rc = check_aligned(what, "pcand", pcand, err, errcap)) return rc;
  if (int rc = check_aligned(what, "out", out, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_apply_device", err, errcap,
                 [&] { launch_apply(pcand, H, W, K, labels, out, bad, (hipStream_t)stream); });
}

int stereo_plane_candidates_gather(const double *planes, int H, int W, const double *offsets, int Ko, const double *sources,
                                   int M, const int32_t *taps, int T, double *pcand, char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_gather";
  if (int rc = check_gather(what, "planes", "pcand", planes, H, W, offsets, Ko, sources, M, taps, T, pcand, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "planes", planes, (int64_t)n, H, 0, err, errcap)) return rc;
  const bool taken = (int64_t)M * T > 0;
  for (int m = 0; taken && m < M; ++m)
    if (int rc = check_planes(what, "source " + std::to_string(m), sources + 4 * (size_t)m * n, (int64_t)n, H, 0, err, errcap)) return rc;
  const size_t K = (size_t)Ko + (size_t)M * T;
  return guarded("stereo_plane_candidates_gather", err, errcap, [&] {
    stereo::DevBuf<double> dp, doff, ds, dc;
    stereo::DevBuf<int32_t> dt;
    dp.upload(planes, 4 * n); doff.upload(offsets, Ko); dc.alloc(4 * n * K);
    if (taken) { ds.upload(sources, 4 * n * M); dt.upload(taps, 2 * (size_t)T); }
    launch_gather(dp.p, H, W, doff.p, Ko, ds.p, M, dt.p, T, dc.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(pcand, dc.p, 4 * n * K * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int stereo_plane_candidates_inputs_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                       double unary_weight, const double *pcand, int K, int64_t E, const uint32_t *conn,
                                       double *unary, double *q, double *qprim, char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_inputs_ncc";
  if (int rc = check_inputs(what, H, W, pcand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "pcand", pcand, (int64_t)n, H, K, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_inputs_ncc", err, errcap, [&] {
    stereo::DevBuf<double> dn, dd, dcand;
    dn.upload(ncc, n * D); dd.upload(disparities, D); dcand.upload(pcand, 4 * n * K);
    HostOutputs out(n, K, E, conn);
    launch_ncc(dn.p, H, W, D, layout, disparities, dd.p, unary_weight, dcand.p, K, E, out.dc.p, out.du.p, out.dq.p, out.dqp.p,
               nullptr, nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_plane_candidates_inputs_globalstereo(const double *im0, const double *im1, int H, int W, int C, const double *P2,
                                                double d_min, double d_step, double col_thresh, const double *pcand, int K,
                                                int64_t E, const uint32_t *conn, double *unary, double *q, double *qprim,
                                                char *err, size_t errcap) {
  const std::string what = "stereo_plane_candidates_inputs_globalstereo";
  if (int rc = check_inputs(what, H, W, pcand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (int rc = check_gs(what, im0, im1, C, P2, d_step, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "pcand", pcand, (int64_t)n, H, K, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_inputs_globalstereo", err, errcap, [&] {
    stereo::DevBuf<double> d0, d1, dcand;
    d0.upload(im0, n * C); d1.upload(im1, n * C); dcand.upload(pcand, 4 * n * K);
    HostOutputs out(n, K, E, conn);
    launch_gs(d0.p, d1.p, H, W, C, P2, d_min, d_step, col_thresh, dcand.p, K, E, out.dc.p, out.du.p, out.dq.p, out.dqp.p, nullptr,
              nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_plane_candidates_apply(const double *pcand, int H, int W, int K, const int32_t *labels, double *out, char *err,
                                  size_t errcap) {
  const std::string what = "stereo_plane_candidates_apply";
  if (int rc = check_apply(what, pcand, H, W, K, labels, out, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_planes(what, "pcand", pcand, (int64_t)n, H, K, err, errcap)) return rc;
  if (int rc = check_labels(what, labels, n, K, err, errcap)) return rc;
  return guarded("stereo_plane_candidates_apply", err, errcap, [&] {
    stereo::DevBuf<double> dcand, dout;
    stereo::DevBuf<int32_t> dl;
    dcand.upload(pcand, 4 * n * K); dl.upload(labels, n); dout.alloc(4 * n);
    launch_apply(dcand.p, H, W, K, dl.p, dout.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, dout.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
