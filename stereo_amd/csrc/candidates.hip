// Candidate bands: per-pixel label sets propagated from neighbours (the definition:
// include/stereo_hip.h).  A candidate table `cand` (K x N, label fastest) says what label k means at pixel i: a
// disparity of its own, not base_i + a shared offset.  gather builds the table from a base map, the band's offsets
// and M source maps read at T taps; inputs makes the TRW-S problem of ANY table (unary by the NCC sampler of
// ncc_sample.h, q / qprim by the plane -> disparity rule on the plane [0 0 1 -cand]); apply reads the map a labelling
// selects.
//
// The lane mapping is the band's (band.hip): a lane is one (pixel, k) or (edge, k) element in storage order, every
// wave stores 512 consecutive bytes, the 64-bit division by K is done once per block on uniform values.  The index,
// the clamp of a tap (tapped_pixel), the launch sizes, slice_range(), the argument checks (check_gather takes the
// names of this file's two arrays), the scans of a host entry's arrays and HostOutputs are in band_common.h.
#include <cmath>
#include <cstdint>
#include <string>

#include "band_common.h"
#include "common.h"
#include "ncc_sample.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;
using namespace stereo::band;   // band_common.h: the indices, the launch sizes, every check and scan, HostOutputs

// The disparity of a label whose candidate is c: plane_disp of [0 0 1 -c], i.e. c with the plane's sign of zero
// (-0 for c == 0), as band_disp gives it for base + delta.
__device__ __forceinline__ double cand_disp(double c) {
  const double pl[4] = {0.0, 0.0, 1.0, -c};
  return stereo::plane_disp(pl, 1.0, 1.0);
}

// cand[k, i] = base_i + offsets_k for k < Ko; cand[Ko + m T + t, (y, x)] = src_m[clamp(y + dy_t), clamp(x + dx_t)].
// `bad` counts the pixels at which the base or a source is not finite (the lane k == 0 of the pixel looks).
__global__ __launch_bounds__(kTB) void candidates_gather_kernel(int64_t Npx, int H, int W, const double *__restrict__ base,
                                                               const double *__restrict__ offsets, int Ko,
                                                               const double *__restrict__ sources, int M,
                                                               const int32_t *__restrict__ taps, int T,
                                                               double *__restrict__ cand, int32_t *bad) {
  const int K = Ko + M * T;
  const int64_t total = Npx * K;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, K);
    if (ix.item >= Npx) continue;
    if (bad && ix.k == 0) {
      bool finite = isfinite(base[ix.item]);
      if (T > 0)
        for (int m = 0; m < M; ++m) finite = finite && isfinite(sources[(int64_t)m * Npx + ix.item]);
      if (!finite) atomicAdd(bad, 1);
    }
    double v;
    if (ix.k < Ko) {
      v = base[ix.item] + offsets[ix.k];
    } else {
      const int j = ix.k - Ko, m = j / T, t = j - m * T;
      v = sources[(int64_t)m * Npx + tapped_pixel(ix.item, H, W, taps, t)];
    }
    cand[first + threadIdx.x] = v;
  }
}

// unary(k, i) = unary_weight * (1 - sample(cand[k, i])).  The D slice positions are staged in LDS as in
// band_unary_kernel (DESIGN.md 6.2 has the measurement).  `bad` counts the pixels with a candidate that is not
// finite: a lane tests the candidate it has loaded anyway, and only a lane that finds one looks at the pixel's
// lower labels to see whether it is the first (a loop over K in the lane k == 0 of every pixel cost 17 - 37 % of the
// builder's time).
template <bool kStageSlices>
__global__ __launch_bounds__(kTB) void candidates_unary_kernel(const double *__restrict__ ncc, int64_t Npx, int D, int layout,
                                                              const double *__restrict__ dv, double dmin, double dmax,
                                                              double unary_weight, const double *__restrict__ cand, int K,
                                                              int ascending, double *__restrict__ U, int32_t *bad) {
  extern __shared__ double staged_slices[];
  const double *slices = dv;
  if (kStageSlices) {
    for (int i = threadIdx.x; i < D; i += kTB) staged_slices[i] = dv[i];
    __syncthreads();
    slices = staged_slices;
  }
  const int64_t total = Npx * K;
  for (int64_t first = (int64_t)blockIdx.x * kTB; first < total; first += (int64_t)gridDim.x * kTB) {
    const BandIndex ix = band_index(first, K);
    if (ix.item >= Npx) continue;
    const int64_t t = first + threadIdx.x;
    const double c = cand[t];
    if (bad && !isfinite(c)) {     // (rare) the pixel counts once: at its first label that is not finite
      bool first_of_pixel = true;
      for (int k = 0; k < ix.k; ++k) first_of_pixel = first_of_pixel && isfinite(cand[t - ix.k + k]);
      if (first_of_pixel) atomicAdd(bad, 1);
    }
    U[t] = stereo::ncc_unary_at(ncc, Npx, D, layout, ix.item, slices, dmin, dmax, unary_weight, cand_disp(c), ascending);
  }
}

// q(k, e) = the disparity of label k at the edge's second pixel, qprim(k, e) at its first: K consecutive doubles of
// the table per endpoint.  The shape of band_positions_kernel: a block takes kPosPerThread * 256 consecutive elements,
// a thread kPosPerThread of them 256 apart; every load is unconditional at a clamped address, only the stores are
// predicated.  An edge that names a pixel outside 0 .. N - 1 reads pixel 0 and gets NaN.
constexpr int kPosPerThread = 4;
__global__ __launch_bounds__(kTB) void candidates_positions_kernel(int64_t E, int K, int64_t Npx, const uint32_t *__restrict__ conn,
                                                                  const double *__restrict__ cand, double *__restrict__ q,
                                                                  double *__restrict__ qprim) {
  const int64_t total = E * K;
  constexpr int64_t kChunk = (int64_t)kTB * kPosPerThread;
  const double nan = __builtin_nan("");
  for (int64_t first = (int64_t)blockIdx.x * kChunk; first < total; first += (int64_t)gridDim.x * kChunk) {
    const int64_t item0 = first / K;                       // (uniform: once per block and chunk)
    const uint32_t rem0 = (uint32_t)(first - item0 * K);
    uint32_t i1[kPosPerThread], i2[kPosPerThread], k[kPosPerThread];
    double c1[kPosPerThread], c2[kPosPerThread];
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
      c1[u] = cand[(int64_t)(i1[u] < Npx ? i1[u] : 0) * K + k[u]];
      c2[u] = cand[(int64_t)(i2[u] < Npx ? i2[u] : 0) * K + k[u]];
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      if (!live[u]) continue;
      const int64_t t = first + (int64_t)u * kTB + threadIdx.x;
      q[t] = i2[u] < Npx ? cand_disp(c2[u]) : nan;
      qprim[t] = i1[u] < Npx ? cand_disp(c1[u]) : nan;
    }
  }
}

// out_i = cand[label_i - 1, i], copied; a label outside 1 .. K gives NaN and counts in `bad`.
__global__ __launch_bounds__(kTB) void candidates_apply_kernel(int64_t Npx, int K, const double *__restrict__ cand,
                                                              const int32_t *__restrict__ labels, double *__restrict__ out,
                                                              int32_t *bad) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < Npx; i += (int64_t)gridDim.x * kTB) {
    const int32_t l = labels[i];
    const bool in = l >= 1 && l <= K;
    if (bad && !in) atomicAdd(bad, 1);
    out[i] = in ? cand[i * K + (l - 1)] : __builtin_nan("");
  }
}

// ---------------------------------------------------------------- argument checks (no device call)

int check_inputs(const std::string &what, const void *ncc, int H, int W, int D, int layout, const double *disparities,
                 const void *cand, int K, int64_t E, const void *conn, const void *unary, const void *q, const void *qprim,
                 char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  if (int rc = check_edges(what, E, conn, q, qprim, err, errcap)) return rc;
  if (!cand || !unary) return fail(what + ": cand and unary must not be NULL", err, errcap);
  return check_k(what, K, err, errcap);
}

int check_apply(const std::string &what, const void *cand, int H, int W, int K, const void *labels, const void *out, char *err,
                size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (!cand || !labels || !out) return fail(what + ": cand, labels and out must not be NULL", err, errcap);
  return check_k(what, K, err, errcap);
}

void launch_gather(const double *base, int H, int W, const double *d_offsets, int Ko, const double *sources, int M,
                   const int32_t *d_taps, int T, double *cand, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(candidates_gather_kernel, dim3(grid_for(Npx * (Ko + M * T))), dim3(kTB), 0, s, Npx, H, W, base, d_offsets, Ko,
                     sources, M, d_taps, T, cand, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities, const double *d_disparities,
                   double unary_weight, const double *cand, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
                   double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  const SliceRange r = slice_range(disparities, D);
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (D <= kMaxStagedSlices)
    hipLaunchKernelGGL(candidates_unary_kernel<true>, dim3(grid_for(Npx * K)), dim3(kTB), (size_t)D * sizeof(double), s, ncc, Npx,
                       D, layout, d_disparities, r.dmin, r.dmax, unary_weight, cand, K, r.ascending, unary, bad);
  else
    hipLaunchKernelGGL(candidates_unary_kernel<false>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, ncc, Npx, D, layout,
                       d_disparities, r.dmin, r.dmax, unary_weight, cand, K, r.ascending, unary, bad);
  STEREO_HIP_CHECK(hipGetLastError());
  if (E > 0) {
    hipLaunchKernelGGL(candidates_positions_kernel, dim3(grid_for((E * K + kPosPerThread - 1) / kPosPerThread)), dim3(kTB), 0, s, E,
                       K, Npx, conn, cand, q, qprim);
    STEREO_HIP_CHECK(hipGetLastError());
  }
}

void launch_apply(const double *cand, int H, int W, int K, const int32_t *labels, double *out, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(candidates_apply_kernel, dim3(grid_for(Npx)), dim3(kTB), 0, s, Npx, K, cand, labels, out, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_candidates_gather_device(const double *base, int H, int W, const double *offsets, const double *d_offsets, int Ko,
                                    const double *sources, int M, const int32_t *taps, const int32_t *d_taps, int T,
                                    double *cand, int32_t *bad, void *stream, char *err, size_t errcap) {
  const std::string what = "stereo_candidates_gather_device";
  if (int rc = check_gather(what, "base", "cand", base, H, W, offsets, Ko, sources, M, taps, T, cand, err, errcap)) return rc;
  if (!d_offsets) return fail(what + ": d_offsets must not be NULL", err, errcap);
  if ((int64_t)M * T > 0 && !d_taps) return fail(what + ": d_taps must not be NULL when M * T > 0", err, errcap);
  return guarded("stereo_candidates_gather_device", err, errcap,
                 [&] { launch_gather(base, H, W, d_offsets, Ko, sources, M, d_taps, T, cand, bad, (hipStream_t)stream); });
}

int stereo_candidates_inputs_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                    const double *d_disparities, double unary_weight, const double *cand, int K, int64_t E,
                                    const uint32_t *conn, double *unary, double *q, double *qprim, int32_t *bad, void *stream,
                                    char *err, size_t errcap) {
  const std::string what = "stereo_candidates_inputs_device";
  if (int rc = check_inputs(what, ncc, H, W, D, layout, disparities, cand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  if (!d_disparities) return fail(what + ": d_disparities must not be NULL", err, errcap);
  return guarded("stereo_candidates_inputs_device", err, errcap, [&] {
    launch_inputs(ncc, H, W, D, layout, disparities, d_disparities, unary_weight, cand, K, E, conn, unary, q, qprim, bad,
                  (hipStream_t)stream);
  });
}

int stereo_candidates_apply_device(const double *cand, int H, int W, int K, const int32_t *labels, double *out, int32_t *bad,
                                   void *stream, char *err, size_t errcap) {
  if (int rc = check_apply("stereo_candidates_apply_device", cand, H, W, K, labels, out, err, errcap)) return rc;
  return guarded("stereo_candidates_apply_device", err, errcap,
                 [&] { launch_apply(cand, H, W, K, labels, out, bad, (hipStream_t)stream); });
}

int stereo_candidates_gather(const double *base, int H, int W, const double *offsets, int Ko, const double *sources, int M,
                             const int32_t *taps, int T, double *cand, char *err, size_t errcap) {
  const std::string what = "stereo_candidates_gather";
  if (int rc = check_gather(what, "base", "cand", base, H, W, offsets, Ko, sources, M, taps, T, cand, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite(what, "base", base, (int64_t)n, H, 0, err, errcap)) return rc;
  const bool taken = (int64_t)M * T > 0;
  for (int m = 0; taken && m < M; ++m)
    if (int rc = check_finite(what, "source " + std::to_string(m), sources + (size_t)m * n, (int64_t)n, H, 0, err, errcap)) return rc;
  const size_t K = (size_t)Ko + (size_t)M * T;
  return guarded("stereo_candidates_gather", err, errcap, [&] {
    stereo::DevBuf<double> db, doff, ds, dc;
    stereo::DevBuf<int32_t> dt;
    db.upload(base, n); doff.upload(offsets, Ko); dc.alloc(n * K);
    if (taken) { ds.upload(sources, n * M); dt.upload(taps, 2 * (size_t)T); }
    launch_gather(db.p, H, W, doff.p, Ko, ds.p, M, dt.p, T, dc.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(cand, dc.p, n * K * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int stereo_candidates_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities, double unary_weight,
                             const double *cand, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
                             double *qprim, char *err, size_t errcap) {
  const std::string what = "stereo_candidates_inputs";
  if (int rc = check_inputs(what, ncc, H, W, D, layout, disparities, cand, K, E, conn, unary, q, qprim, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite(what, "cand", cand, (int64_t)n, H, K, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_candidates_inputs", err, errcap, [&] {
    stereo::DevBuf<double> dn, dcand, dd;
    dn.upload(ncc, n * D); dcand.upload(cand, n * K); dd.upload(disparities, D);
    HostOutputs out(n, K, E, conn);
    launch_inputs(dn.p, H, W, D, layout, disparities, dd.p, unary_weight, dcand.p, K, E, out.dc.p, out.du.p, out.dq.p, out.dqp.p,
                  nullptr, nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_candidates_apply(const double *cand, int H, int W, int K, const int32_t *labels, double *out, char *err,
                            size_t errcap) {
  const std::string what = "stereo_candidates_apply";
  if (int rc = check_apply(what, cand, H, W, K, labels, out, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite(what, "cand", cand, (int64_t)n, H, K, err, errcap)) return rc;
  if (int rc = check_labels(what, labels, n, K, err, errcap)) return rc;
  return guarded("stereo_candidates_apply", err, errcap, [&] {
    stereo::DevBuf<double> dcand, dout;
    stereo::DevBuf<int32_t> dl;
    dcand.upload(cand, n * K); dl.upload(labels, n); dout.alloc(n);
    launch_apply(dcand.p, H, W, K, dl.p, dout.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
