// Messages carried from one band level or pyramid scale to the next (the definition:
// include/stereo_hip.h).  Every new edge's row is the old row of the edge it inherits from, read as a piecewise
// linear function on the old level's offset axis, sampled at the new level's offsets, flat outside the old range,
// shifted so that its minimum is zero and scaled.
//
// A streaming kernel: 8 K_old bytes in and 8 K_new bytes out per edge, plus the edge's two indices and one shift.
// Mapping as in trws_beliefs.hip: a group of G lanes per output row, G = the power of two >= K_new up to 64, so a
// wave holds 64 / G rows and stores them as one contiguous span; above 64 labels one wave per row with a strided
// label loop.  A group takes four rows per step, their loads in flight together (a row's loads hang on each other).  Both offset vectors sit in LDS (at most 36 KiB); a lane finds its interval by bisection there.  Where
// the old row fits the group (K_old <= G) it is loaded once, one value per lane, and a lane fetches its two
// neighbours with cross-lane reads; otherwise it reads the two neighbours from memory (one row's lanes read within
// the same 8 K_old bytes, so the row still comes from memory once).  The row minimum is a cross-lane reduction on
// (value, label) pairs, which keeps the first minimum.  Plain C++; the only atomic is the `bad` counter.
#include <cmath>
#include <cstdint>
#include <string>

#include "band_common.h"
#include "carry_host.h"
#include "common.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;
using stereo::band::kMaxGrid;
using stereo::band::kTB;
using stereo::carry::Args;

static_assert(stereo::carry::kMaxNewLabels == stereo::band::kMaxOffsets, "K_new is a band's K");

constexpr int kWave = 64;

constexpr int kRowsPerGroup = 4;   // rows a lane group takes per step, their loads in flight together

// One output row for the G lanes of its group.  Every lane of the wave comes through here (the cross-lane reads need
// whole groups); `row`: the group has a row at all, `live`: it is not a zero row.
// kLaneRow: K_old <= G, the old row lies one value per lane of the group (`mine`)
template <bool kLaneRow>
__device__ __forceinline__ void carry_row(bool row, bool live, double t, const double *__restrict__ src, double mine,
                                          double *__restrict__ dst, const double *so, const double *sn, int K_old, int K_new,
                                          int G, int sub, double stretch, double gain) {
  const double first = so[0], last = so[K_old - 1];
  // this lane's smallest value and its (first) label
  double m = __builtin_huge_val(), own = 0.0;
  int mj = 0x7fffffff;
  for (int j0 = 0; j0 < K_new; j0 += G) {
    const int j = j0 + sub;
    const bool valid = j < K_new;
    const double u = t + stretch * sn[valid ? j : 0];
    int i = 0, i1 = 0;
    bool inside = false;
    if (u <= first) {
    } else if (u >= last) {
      i = i1 = K_old - 1;
    } else {
      int hi = K_old - 1;                         // so[i] <= u < so[hi]
      while (hi - i > 1) {
        const int mid = (i + hi) >> 1;
        if (so[mid] <= u) i = mid; else hi = mid;
      }
      i1 = i + 1 < K_old ? i + 1 : i;
      inside = i1 > i;
    }
    double a, b;
    if (kLaneRow) {
      a = __shfl(mine, i, G);
      b = __shfl(mine, i1, G);
    } else {
      const bool load = live && valid;
      a = load ? src[i] : 0.0;
      b = load ? src[i1] : 0.0;
    }
    double v = a;
    if (inside) {
      const double w = (u - so[i]) / (so[i1] - so[i]);
      v = a + w * (b - a);
    }
    if (!live) v = 0.0;
    if (valid) {
      if (v < m) { m = v; mj = j; }
      own = v;
      if (K_new > G && row) dst[j] = v;           // (several labels per lane: normalised in a second pass)
    }
  }
  // across the group (G lanes, aligned: the xor partners stay inside it); equal values: the lower label
  for (int off = G >> 1; off > 0; off >>= 1) {
    const double om = __shfl_xor(m, off, kWave);
    const int oj = __shfl_xor(mj, off, kWave);
    if (om < m || (om == m && oj < mj)) { m = om; mj = oj; }
  }
  if (!row) return;
  if (K_new <= G) {
    if (sub < K_new) dst[sub] = live ? gain * (own - m) : 0.0;
  } else {
    for (int j = sub; j < K_new; j += G) dst[j] = live ? gain * (dst[j] - m) : 0.0;
  }
}

// A row's loads hang on each other (the edge's indices, then the shift and the old row) and a row is short, so a lane
// group takes kRowsPerGroup rows per step and issues each stage's loads for all of them before it uses any.
template <bool kLaneRow>
__global__ __launch_bounds__(kTB) void band_carry_kernel(const double *__restrict__ M_old, int64_t E_old, int K_old,
                                                        const double *__restrict__ off_old,
                                                        const int32_t *__restrict__ edge_src,
                                                        const int32_t *__restrict__ receiver_new, int64_t N_new,
                                                        const double *__restrict__ shift, double stretch, double gain,
                                                        const double *__restrict__ off_new, int K_new, int64_t E_new,
                                                        int lg, double *__restrict__ M_new, int32_t *bad) {
  extern __shared__ __attribute__((aligned(16))) double carry_offsets[];
  double *so = carry_offsets, *sn = carry_offsets + K_old;
  for (int i = threadIdx.x; i < K_old; i += kTB) so[i] = off_old[i];
  for (int i = threadIdx.x; i < K_new; i += kTB) sn[i] = off_new[i];
  __syncthreads();
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const int rows = kTB >> lg;                       // rows the block's groups take side by side
  const int64_t step = (int64_t)rows * kRowsPerGroup;
  // every lane of a block takes the same number of steps (the cross-lane reads need whole groups)
  for (int64_t e0 = (int64_t)blockIdx.x * step; e0 < E_new; e0 += (int64_t)gridDim.x * step) {
    int64_t e[kRowsPerGroup], s[kRowsPerGroup], r[kRowsPerGroup];
    bool row[kRowsPerGroup], live[kRowsPerGroup];
    double t[kRowsPerGroup], mine[kRowsPerGroup];
#pragma unroll
    for (int u = 0; u < kRowsPerGroup; ++u) {
      e[u] = e0 + (int64_t)u * rows + (threadIdx.x >> lg);
      row[u] = e[u] < E_new;
      s[u] = r[u] = -1;
      if (row[u]) {
        s[u] = edge_src ? (int64_t)edge_src[e[u]] : e[u];
        r[u] = receiver_new[e[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsPerGroup; ++u) {
      const bool r_in = r[u] >= 0 && r[u] < N_new;
      const bool offending = row[u] && (s[u] >= E_old || !r_in);
      if (offending && sub == 0 && bad) atomicAdd(bad, 1);
      t[u] = (row[u] && r_in) ? shift[r[u]] : __builtin_nan("");
      live[u] = row[u] && !offending && s[u] >= 0;        // (and a finite shift: below, once it is here)
      mine[u] = 0.0;
      if (kLaneRow && live[u] && sub < K_old) mine[u] = M_old[(size_t)s[u] * K_old + sub];
    }
#pragma unroll
    for (int u = 0; u < kRowsPerGroup; ++u) {
      const bool finite = isfinite(t[u]);
      live[u] = live[u] && finite;
      if (!finite) mine[u] = 0.0;
      carry_row<kLaneRow>(row[u], live[u], t[u], M_old + (size_t)(live[u] ? s[u] : 0) * K_old, mine[u],
                          M_new + (size_t)(row[u] ? e[u] : 0) * K_new, so, sn, K_old, K_new, G, sub, stretch, gain);
    }
  }
}

int group_log2(int K) {
  int lg = 0;
  while ((1 << lg) < K && lg < 6) ++lg;
  return lg;
}

void launch_carry(const Args &a, int32_t *bad, hipStream_t s) {
  if (bad) STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (a.E_new == 0) return;
  const int lg = group_log2(a.K_new);
  const int64_t step = (int64_t)(kTB >> lg) * kRowsPerGroup;
  const int64_t blocks = (a.E_new + step - 1) / step;
  const dim3 grid((unsigned)(blocks > (int64_t)kMaxGrid ? (int64_t)kMaxGrid : blocks));
  const size_t lds = (size_t)(a.K_old + a.K_new) * sizeof(double);
  if (a.K_old <= (1 << lg))
    hipLaunchKernelGGL(band_carry_kernel<true>, grid, dim3(kTB), lds, s, a.M_old, a.E_old, a.K_old, a.d_off_old, a.edge_src,
                       a.receiver_new, a.N_new, a.shift, a.stretch, a.gain, a.d_off_new, a.K_new, a.E_new, lg, a.M_new, bad);
  else
    hipLaunchKernelGGL(band_carry_kernel<false>, grid, dim3(kTB), lds, s, a.M_old, a.E_old, a.K_old, a.d_off_old, a.edge_src,
                       a.receiver_new, a.N_new, a.shift, a.stretch, a.gain, a.d_off_new, a.K_new, a.E_new, lg, a.M_new, bad);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int stereo_band_carry_device(const double *M_old, int64_t E_old, int K_old, const double *off_old, const double *d_off_old,
                             const int32_t *edge_src, const int32_t *receiver_new, int64_t N_new, const double *shift,
                             double stretch, double gain, const double *off_new, const double *d_off_new, int K_new,
                             int64_t E_new, double *M_new, int32_t *bad, void *stream, char *err, size_t errcap) {
  Args a;
  a.M_old = M_old; a.E_old = E_old; a.K_old = K_old; a.off_old = off_old; a.edge_src = edge_src;
  a.receiver_new = receiver_new; a.N_new = N_new; a.shift = shift; a.stretch = stretch; a.gain = gain;
  a.off_new = off_new; a.K_new = K_new; a.E_new = E_new; a.M_new = M_new; a.bad = bad;
  a.device_form = true; a.d_off_old = d_off_old; a.d_off_new = d_off_new;
  if (int rc = stereo::carry::check_args("stereo_band_carry_device", a, err, errcap)) return rc;
  return guarded("stereo_band_carry_device", err, errcap, [&] { launch_carry(a, bad, (hipStream_t)stream); });
}

int stereo_band_carry(const double *M_old, int64_t E_old, int K_old, const double *off_old, const int32_t *edge_src,
                      const int32_t *receiver_new, int64_t N_new, const double *shift, double stretch, double gain,
                      const double *off_new, int K_new, int64_t E_new, double *M_new, int64_t *bad, char *err,
                      size_t errcap) {
  Args a;
  a.M_old = M_old; a.E_old = E_old; a.K_old = K_old; a.off_old = off_old; a.edge_src = edge_src;
  a.receiver_new = receiver_new; a.N_new = N_new; a.shift = shift; a.stretch = stretch; a.gain = gain;
  a.off_new = off_new; a.K_new = K_new; a.E_new = E_new; a.M_new = M_new; a.bad = bad;
  if (int rc = stereo::carry::check_args("stereo_band_carry", a, err, errcap)) return rc;
  return guarded("stereo_band_carry", err, errcap, [&] {
    stereo::DevBuf<double> dm, doo, dsh, don, dout;
    stereo::DevBuf<int32_t> dsrc, drecv, dbad;
    dm.upload(M_old, (size_t)E_old * K_old); doo.upload(off_old, K_old); don.upload(off_new, K_new);
    dsh.upload(shift, (size_t)N_new); drecv.upload(receiver_new, (size_t)E_new);
    if (edge_src) dsrc.upload(edge_src, (size_t)E_new);
    dout.alloc((size_t)E_new * K_new); dbad.alloc(1);
    Args d = a;
    d.M_old = dm.p; d.d_off_old = doo.p; d.d_off_new = don.p; d.shift = dsh.p; d.receiver_new = drecv.p;
    d.edge_src = edge_src ? dsrc.p : nullptr; d.M_new = dout.p;
    launch_carry(d, dbad.p, nullptr);
    int32_t n = 0;
    STEREO_HIP_CHECK(hipMemcpy(&n, dbad.p, sizeof(n), hipMemcpyDeviceToHost));
    if (E_new > 0) STEREO_HIP_CHECK(hipMemcpy(M_new, dout.p, (size_t)E_new * K_new * sizeof(double), hipMemcpyDeviceToHost));
    if (bad) *bad = n;
  });
}

}  // extern "C"
