// Band refinement around a solved disparity map (the definition: include/stereo_hip.h).
// From a map `base` and K offsets, the TRW-S inputs of the problem whose label k at pixel i means the
// fronto-parallel plane [0 0 1 -(base_i + offsets_k)]: unary (K x N) by the NCC sampler of ncc_sample.h,
// q / qprim (K x E) by the plane -> disparity rule, and the map a labelling selects.
//
// All three output arrays are label fastest, and a lane is one (pixel, k) or (edge, k) element of them in
// storage order: every wave stores 512 consecutive bytes.  The K lanes of a pixel sample neighbouring
// slices of one volume column; in the label-fastest volume (layout 1) those are the same cache lines, so
// the column's span comes from memory once and the lanes' three loads each are served from cache.  LDS holds the
// D slice positions of the unary kernel and nothing else.
//
// What this file shares with plane_band.hip, candidates.hip and plane_candidates.hip -- the element index, the launch
// sizes, slice_range(), the argument checks, the scans of a host entry's arrays and HostOutputs -- is in band_common.h.
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

// The disparity of label k at a pixel whose base is b: plane_disp of [0 0 1 -(b + delta)].  The plane's
// s = 0 x + 0 y is +0 at every pixel, so no pixel coordinate is formed; the value is b + delta, with the
// sign of zero that the plane gives (-0 for b + delta == 0).
__device__ __forceinline__ double band_disp(double b, double delta) {
  const double pl[4] = {0.0, 0.0, 1.0, -(b + delta)};
  return stereo::plane_disp(pl, 1.0, 1.0);
}

// kStageSlices: the block copies the D slice positions into LDS first.  The nearest-slice search and the parabola read
// them a dozen times per lane, each read waiting for the one before (bisection); from LDS that chain is several
// times shorter than from the vector cache (DESIGN.md 6.2 has the measurement that asked for it).
template <bool kStageSlices>
__global__ __launch_bounds__(kTB) void band_unary_kernel(const double *__restrict__ ncc, int64_t Npx, int D, int layout,
                                                        const double *__restrict__ dv, double dmin, double dmax,
                                                        double unary_weight, const double *__restrict__ base,
                                                        const double *__restrict__ offsets, int K, int ascending,
                                                        double *__restrict__ U, int32_t *bad) {
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
    const double b = base[ix.item];
    if (bad && ix.k == 0 && !isfinite(b)) atomicAdd(bad, 1);
    const double disp = band_disp(b, offsets[ix.k]);
    U[first + threadIdx.x] = stereo::ncc_unary_at(ncc, Npx, D, layout, ix.item, slices, dmin, dmax, unary_weight, disp, ascending);
  }
}

// q(k, e) = disparity of label k at the edge's second pixel, qprim(k, e) at its first (dispmap_super.m:177-183, the
// order trws_positions_kernel writes).  An edge that names a pixel outside 0 .. N - 1 reads nothing and gets NaN.
// This kernel writes 16 of every 18 bytes of a band problem.  A block takes kPosPerThread * 256 consecutive elements,
// a thread kPosPerThread of them 256 apart (each wave instruction still stores 512 consecutive bytes); every load
// is unconditional at a clamped address, so the loads of a thread's elements are in flight together, and only the
// stores are predicated (DESIGN.md 6.1 records what a predicate per load cost the fill kernel).
constexpr int kPosPerThread = 4;
__global__ __launch_bounds__(kTB) void band_positions_kernel(int64_t E, int K, int64_t Npx, const uint32_t *__restrict__ conn,
                                                            const double *__restrict__ base,
                                                            const double *__restrict__ offsets, double *__restrict__ q,
                                                            double *__restrict__ qprim) {
  const int64_t total = E * K;
  constexpr int64_t kChunk = (int64_t)kTB * kPosPerThread;
  const double nan = __builtin_nan("");
  for (int64_t first = (int64_t)blockIdx.x * kChunk; first < total; first += (int64_t)gridDim.x * kChunk) {
    const int64_t item0 = first / K;                       // (uniform: once per block and chunk)
    const uint32_t rem0 = (uint32_t)(first - item0 * K);
    uint32_t i1[kPosPerThread], i2[kPosPerThread];
    double delta[kPosPerThread], b1[kPosPerThread], b2[kPosPerThread];
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
      b1[u] = base[i1[u] < Npx ? i1[u] : 0];
      b2[u] = base[i2[u] < Npx ? i2[u] : 0];
    }
#pragma unroll
    for (int u = 0; u < kPosPerThread; ++u) {
      if (!live[u]) continue;
      const int64_t t = first + (int64_t)u * kTB + threadIdx.x;
      q[t] = i2[u] < Npx ? band_disp(b2[u], delta[u]) : nan;
      qprim[t] = i1[u] < Npx ? band_disp(b1[u], delta[u]) : nan;
    }
  }
}

// refined_i = base_i + offsets_{label_i - 1}; a label outside 1 .. K gives NaN and counts in `bad`.
__global__ __launch_bounds__(kTB) void band_apply_kernel(int64_t Npx, int K, const double *__restrict__ base,
                                                        const int32_t *__restrict__ labels,
                                                        const double *__restrict__ offsets, double *__restrict__ refined,
                                                        int32_t *bad) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < Npx; i += (int64_t)gridDim.x * kTB) {
    const int32_t l = labels[i];
    const bool in = l >= 1 && l <= K;
    if (bad && !in) atomicAdd(bad, 1);
    refined[i] = in ? base[i] + offsets[l - 1] : __builtin_nan("");
  }
}

// ---------------------------------------------------------------- argument checks (no device call)

int check_inputs(const std::string &what, const void *ncc, int H, int W, int D, int layout, const double *disparities,
                 const void *base, const double *offsets, int K, int64_t E, const void *conn, const void *unary,
                 const void *q, const void *qprim, char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (int rc = check_volume(what, ncc, D, layout, disparities, err, errcap)) return rc;
  if (int rc = check_edges(what, E, conn, q, qprim, err, errcap)) return rc;
  if (!base || !unary) return fail(what + ": base and unary must not be NULL", err, errcap);
  return check_offsets(what, offsets, K, err, errcap);
}

int check_apply(const std::string &what, const void *base, int H, int W, const void *labels, const double *offsets, int K,
                const void *refined, char *err, size_t errcap) {
  if (int rc = check_sizes(what, H, W, err, errcap)) return rc;
  if (!base || !labels || !refined) return fail(what + ": base, labels and refined must not be NULL", err, errcap);
  return check_offsets(what, offsets, K, err, errcap);
}

// `disparities` / `offsets`: the host vectors (checked; min, max and the order of the slices come from them);
// `d_disparities` / `d_offsets`: the same values in device memory, which the kernels read
void launch_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                   const double *d_disparities, double unary_weight, const double *base, const double *d_offsets, int K,
                   int64_t E, const uint32_t *conn, double *unary, double *q, double *qprim, int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  const SliceRange r = slice_range(disparities, D);
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (D <= kMaxStagedSlices)
    hipLaunchKernelGGL(band_unary_kernel<true>, dim3(grid_for(Npx * K)), dim3(kTB), (size_t)D * sizeof(double), s, ncc, Npx, D,
                       layout, d_disparities, r.dmin, r.dmax, unary_weight, base, d_offsets, K, r.ascending, unary, bad);
  else
    hipLaunchKernelGGL(band_unary_kernel<false>, dim3(grid_for(Npx * K)), dim3(kTB), 0, s, ncc, Npx, D, layout, d_disparities,
                       r.dmin, r.dmax, unary_weight, base, d_offsets, K, r.ascending, unary, bad);
  STEREO_HIP_CHECK(hipGetLastError());
  if (E > 0) {
    hipLaunchKernelGGL(band_positions_kernel, dim3(grid_for((E * K + kPosPerThread - 1) / kPosPerThread)), dim3(kTB), 0, s, E, K, Npx, conn, base, d_offsets, q, qprim);
    STEREO_HIP_CHECK(hipGetLastError());
  }
}

void launch_apply(const double *base, int H, int W, const int32_t *labels, const double *d_offsets, int K, double *refined,
                  int32_t *bad, hipStream_t s) {
  const int64_t Npx = (int64_t)H * W;
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(band_apply_kernel, dim3(grid_for(Npx)), dim3(kTB), 0, s, Npx, K, base, labels, d_offsets, refined, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_band_max_offsets(void) { return kMaxOffsets; }

int stereo_band_inputs_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                              const double *d_disparities, double unary_weight, const double *base, const double *offsets,
                              const double *d_offsets, int K, int64_t E, const uint32_t *conn, double *unary, double *q,
                              double *qprim, int32_t *bad, void *stream, char *err, size_t errcap) {
  if (int rc = check_inputs("stereo_band_inputs_device", ncc, H, W, D, layout, disparities, base, offsets, K, E, conn, unary, q,
                            qprim, err, errcap))
    return rc;
  if (!d_disparities || !d_offsets) return fail("stereo_band_inputs_device: d_disparities and d_offsets must not be NULL", err, errcap);
  return guarded("stereo_band_inputs_device", err, errcap, [&] {
    launch_inputs(ncc, H, W, D, layout, disparities, d_disparities, unary_weight, base, d_offsets, K, E, conn, unary, q, qprim,
                  bad, (hipStream_t)stream);
  });
}

int stereo_band_apply_device(const double *base, int H, int W, const int32_t *labels, const double *offsets,
                             const double *d_offsets, int K, double *refined, int32_t *bad, void *stream, char *err,
                             size_t errcap) {
  if (int rc = check_apply("stereo_band_apply_device", base, H, W, labels, offsets, K, refined, err, errcap)) return rc;
  if (!d_offsets) return fail("stereo_band_apply_device: d_offsets must not be NULL", err, errcap);
  return guarded("stereo_band_apply_device", err, errcap,
                 [&] { launch_apply(base, H, W, labels, d_offsets, K, refined, bad, (hipStream_t)stream); });
}

int stereo_band_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities, double unary_weight,
                       const double *base, const double *offsets, int K, int64_t E, const uint32_t *conn, double *unary,
                       double *q, double *qprim, char *err, size_t errcap) {
  const std::string what = "stereo_band_inputs";
  if (int rc = check_inputs(what, ncc, H, W, D, layout, disparities, base, offsets, K, E, conn, unary, q, qprim, err, errcap))
    return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite(what, "base", base, (int64_t)n, H, 0, err, errcap)) return rc;
  if (int rc = check_conn(what, conn, E, n, err, errcap)) return rc;
  return guarded("stereo_band_inputs", err, errcap, [&] {
    stereo::DevBuf<double> dn, db, dd, doff;
    dn.upload(ncc, n * D); db.upload(base, n); dd.upload(disparities, D); doff.upload(offsets, K);
    HostOutputs out(n, K, E, conn);
    launch_inputs(dn.p, H, W, D, layout, disparities, dd.p, unary_weight, db.p, doff.p, K, E, out.dc.p, out.du.p, out.dq.p,
                  out.dqp.p, nullptr, nullptr);
    out.fetch(unary, q, qprim);
  });
}

int stereo_band_apply(const double *base, int H, int W, const int32_t *labels, const double *offsets, int K, double *refined,
                      char *err, size_t errcap) {
  const std::string what = "stereo_band_apply";
  if (int rc = check_apply(what, base, H, W, labels, offsets, K, refined, err, errcap)) return rc;
  const size_t n = (size_t)H * W;
  if (int rc = check_finite(what, "base", base, (int64_t)n, H, 0, err, errcap)) return rc;
  if (int rc = check_labels(what, labels, n, K, err, errcap)) return rc;
  return guarded("stereo_band_apply", err, errcap, [&] {
    stereo::DevBuf<double> db, doff, out;
    stereo::DevBuf<int32_t> dl;
    db.upload(base, n); dl.upload(labels, n); doff.upload(offsets, K); out.alloc(n);
    launch_apply(db.p, H, W, dl.p, doff.p, K, out.p, nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(refined, out.p, n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
