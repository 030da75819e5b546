// Scanline aggregation: directional chain min-marginals of a D x N unary volume under the model's own
// pairwise term on one shared positions vector, summed over up to 8 directions, and the reduction of the sum to
// labels, map and confidence.  No reference counterpart.  The definition: include/stereo_hip.h.
//
// One launch per direction on one stream; the first writes S, the later ones add into it (every (pixel, label) lies on
// exactly one chain of a direction, so nothing is atomic).  A chain is serial along its pixels and parallel over its
// labels.  A workgroup is ONE wave, so the barrier of a step costs nothing and chains of different lengths never wait
// for each other across waves.
//
//   D <= 64 (scanline_direction_kernel<LG>): a chain has a group of G = 2^LG lanes, G the power of two >= D, so a wave
//     carries 64 / G chains (D = 3: 16 chains); lane `sub` of a group holds label `sub`.  Row `sub` of the table
//     V[k, l] = w * min(v(|pos_k - pos_l|), tol) does not change along the chain: the lane forms it once and keeps it in
//     registers (2 G VGPRs; +Inf in the columns past D, which therefore never win).  The previous pixel's vector
//     L(p - r, .) goes through LDS: every lane stores its entry, one barrier, and the unrolled loop over l reads
//     L(p - r, l) at an address all lanes of a group share -- a broadcast; the groups of a wave read G doubles apart.
//     Two buffers taken in turn make one barrier per step enough.  A step is then G broadcast reads, G adds and G
//     minima (two running minima, so consecutive v_min_f64 do not wait for each other; a minimum of finite doubles does
//     not depend on its order).
//   64 < D <= 256 (scanline_direction_wide_kernel<LPL, QUAD>): one chain per wave, a lane holds LPL = ceil(D / 64)
//     labels, label = lane + 64 j; a row of V no longer fits in registers, so V is formed in the loop from pos_l in LDS.
//
// Memory: per step a chain reads D doubles of U and, from the second direction on, reads and writes D doubles of S, each
// a contiguous row (label fastest).  None of these loads depends on the recurrence, so the D <= 64 kernel keeps the rows
// of the next kAhead pixels in flight in a register ring: with less than one wave per SIMD (375 x 450 has at most 824
// chains for 1024 SIMDs) nothing else hides the latency of a load.
// Every candidate L + V is one add, U + min is one add, the product in V comes last (-ffp-contract=off): S equals the
// restatement (tests/scanline_restate.py) bit for bit.
//
// Weighted form (stereo_scanline_aggregate_weighted): the step into pixel p along direction r weighs
// wstep[r, p] instead of w_r.  It is the template parameter WEIGHTED of the same two kernels, and the unweighted
// instantiations are instruction for instruction what they were without it: the kernels' weight argument is a double
// or a pointer by instantiation (Weight<>), the table row holds min(v, tol) without the weight, and the product
// ws * row[l] is formed in the l loop (one more fp64 multiply per l).  S equals tests/scanline_weighted_restate.py bit
// for bit.
//
// Chains of a direction (dy, dx), predecessor (y - dy, x - dx), pixel id = y + H x:
//   dx == 0: W chains of H pixels from row 0 (dy > 0) or H - 1;  dy == 0: H chains of W pixels from column 0 or W - 1;
//   diagonal: H + W - 1 chains.  The first H start on the column border (column 0 for dx > 0, W - 1 otherwise), one per
//   row; the other W - 1 on the row border (row 0 for dy > 0, H - 1 otherwise), at the columns off the column border.
//   A chain ends where either coordinate would leave the image.
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "common.h"
#include "scanline_finish.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;

constexpr int kWave = 64;
constexpr int kMaxLabels = 256;
constexpr int kMaxDirections = 8;
constexpr int kFinishBlock = 256;
constexpr int kAhead = 4;       // pixels of a chain whose rows of U and S are in flight (D <= 64)

__host__ __device__ inline int chain_count(int H, int W, int dy, int dx) {
  return dx == 0 ? W : dy == 0 ? H : H + W - 1;
}

// chain c of the direction: its first pixel and its number of pixels
__device__ __forceinline__ void chain_start(int H, int W, int dy, int dx, int c, int &y0, int &x0, int &len) {
  const int yb = dy > 0 ? 0 : H - 1, xb = dx > 0 ? 0 : W - 1;
  if (dx == 0) {
    y0 = yb; x0 = c; len = H;
  } else if (dy == 0) {
    y0 = c; x0 = xb; len = W;
  } else {
    if (c < H) { y0 = c; x0 = xb; }
    else { y0 = yb; x0 = xb + dx * (c - H + 1); }
    const int ny = dy > 0 ? H - y0 : y0 + 1, nx = dx > 0 ? W - x0 : x0 + 1;
    len = ny < nx ? ny : nx;
  }
}

// the longest chain of the wave, as a scalar
__device__ __forceinline__ int wave_max(int v) {
  for (int off = kWave >> 1; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return __builtin_amdgcn_readfirstlane(v);
}

// The weight argument of a direction's launch: the direction's w_r, or (WEIGHTED) the direction's N
// step weights, wstep[r, .], read at the pixel a step enters.
template <bool WEIGHTED>
using Weight = typename std::conditional<WEIGHTED, const double *, double>::type;

// D <= 2^LG <= 64: a group of 2^LG lanes per chain, the lane's row of V in registers
// WEIGHTED: the row kept is b[l] = min(v(|pos_k - pos_l|), tol) without a weight; the step's weight is one double per
// chain and step, loaded by every lane of the group from one address and carried in the ring next to the rows of U and
// S (its load does not depend on the recurrence either); a candidate is prev[l] + ws * b[l], the product first.
// The padded columns l >= D: 0 * Inf is a NaN, so they must never be a product of the weight with +Inf.  The select
// is made ONCE, on the other operand, not after each product and not by bounding the loop at D (which would index the
// register row dynamically): b[l] = 0 there and the entries of `prev` past D, which no lane ever writes, are set to
// +Inf, so a padded candidate is Inf + ws * 0 = Inf for every finite ws and never wins.
template <int LG, bool WEIGHTED>
__global__ void __launch_bounds__(kWave)
    scanline_direction_kernel(const double *__restrict__ unary, const double *__restrict__ positions, int H, int W, int D,
                              int kernel, double tol, Weight<WEIGHTED> w, int dy, int dx, int chains, int accumulate,
                              double *S) {
  constexpr int G = 1 << LG;
  __shared__ double prev[2][kWave];
  const int lane = (int)threadIdx.x;
  const int sub = lane & (G - 1);
  const int first = lane & ~(G - 1);             // the group's place in a buffer of `prev`
  const int64_t c = (int64_t)blockIdx.x * (kWave >> LG) + (lane >> LG);
  int y0 = 0, x0 = 0, len = 0;
  if (c < chains) chain_start(H, W, dy, dx, (int)c, y0, x0, len);
  const int steps = wave_max(len);
  const bool valid = sub < D;
  const double inf = __builtin_huge_val();
  const double pk = valid ? positions[sub] : 0.0;
  double vrow[G];
#pragma unroll
  for (int l = 0; l < G; ++l) {
    const double d = fabs(pk - positions[l < D ? l : 0]);
    const double v = kernel == 2 ? d * d : d;
    if constexpr (WEIGHTED) vrow[l] = l < D ? fmin(v, tol) : 0.0;
    else vrow[l] = l < D ? w * fmin(v, tol) : inf;
  }
  // the entries past D are never written.  Unweighted: 0 + Inf = Inf, never a NaN; WEIGHTED: Inf + ws * 0 (above)
  const double pad = WEIGHTED && !valid ? inf : 0.0;
  prev[0][lane] = pad;
  prev[1][lane] = pad;
  __syncthreads();

  const int64_t row0 = ((int64_t)y0 + (int64_t)H * x0) * D + sub;
  const int64_t stride = ((int64_t)dy + (int64_t)H * dx) * D;
  double ub[kAhead], sb[kAhead], wb[WEIGHTED ? kAhead : 1];
  auto fetch = [&](int t, double &u, double &s, double &ws) {
    u = s = 0.0;
    if (t < len && valid) {
      u = unary[row0 + t * stride];
      if (accumulate) s = S[row0 + t * stride];
    }
    if constexpr (WEIGHTED) {                     // (pixel 0 of a chain has no predecessor: its entry is not read)
      ws = 0.0;
      if (t > 0 && t < len) ws = w[(int64_t)y0 + (int64_t)H * x0 + t * ((int64_t)dy + (int64_t)H * dx)];
    }
  };
#pragma unroll
  for (int i = 0; i < kAhead; ++i) fetch(i, ub[i], sb[i], wb[WEIGHTED ? i : 0]);
  for (int t0 = 0; t0 < steps; t0 += kAhead) {
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int t = t0 + i;
      if (t < steps) {                            // (wave uniform)
        const double u = ub[i], s = sb[i], ws = WEIGHTED ? wb[WEIGHTED ? i : 0] : 0.0;
        fetch(t + kAhead, ub[i], sb[i], wb[WEIGHTED ? i : 0]);
        double L = u;
        if (t > 0) {
          const double *pv = prev[(t - 1) & 1] + first;
          double m0 = inf, m1 = inf;
#pragma unroll
          for (int l = 0; l < G; l += 2) {
            if constexpr (WEIGHTED) {
              m0 = fmin(m0, pv[l] + ws * vrow[l]);
              if constexpr (G > 1) m1 = fmin(m1, pv[l + 1] + ws * vrow[l + 1]);
            } else {
              m0 = fmin(m0, pv[l] + vrow[l]);
              if constexpr (G > 1) m1 = fmin(m1, pv[l + 1] + vrow[l + 1]);
            }
          }
          L = u + fmin(m0, m1);
        }
        if (t < len && valid) {
          S[row0 + t * stride] = accumulate ? s + L : L;
          prev[t & 1][lane] = L;
        }
        __syncthreads();
      }
    }
  }
}

// 64 < D <= 256: one chain per wave, LPL labels per lane; QUAD: the quadratic kernel
// WEIGHTED: w is the step's weight, loaded one step ahead (one address for the wave); the loop runs to D, so there are
// no padded columns here
template <int LPL, bool QUAD, bool WEIGHTED>
__global__ void __launch_bounds__(kWave)
    scanline_direction_wide_kernel(const double *__restrict__ unary, const double *__restrict__ positions, int H, int W,
                                   int D, double tol, Weight<WEIGHTED> w, int dy, int dx, int chains, int accumulate,
                                   double *S) {
  __shared__ double pos[LPL * kWave];
  __shared__ double prev[2][LPL * kWave];
  const int lane = (int)threadIdx.x;
  const int c = (int)blockIdx.x;
  int y0 = 0, x0 = 0, len = 0;
  if (c < chains) chain_start(H, W, dy, dx, c, y0, x0, len);
  len = __builtin_amdgcn_readfirstlane(len);

  double pk[LPL];
  bool valid[LPL];
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const int k = lane + j * kWave;
    valid[j] = k < D;
    pk[j] = valid[j] ? positions[k] : 0.0;
    pos[k] = pk[j];
    prev[0][k] = 0.0;
    prev[1][k] = 0.0;
  }
  __syncthreads();

  int64_t row = ((int64_t)y0 + (int64_t)H * x0) * D + lane;
  const int64_t stride = ((int64_t)dy + (int64_t)H * dx) * D;
  // WEIGHTED: the weight of the step into pixel t + 1 is loaded one step ahead, with the rows of pixel t (it does not
  // depend on the recurrence); pixel 0 has no predecessor and its entry is not read
  [[maybe_unused]] int64_t pix = (int64_t)y0 + (int64_t)H * x0;
  [[maybe_unused]] double wnext = 0.0;
  const double inf = __builtin_huge_val();
  for (int t = 0; t < len; ++t) {
    double u[LPL], s[LPL], m[LPL];
    double ws;
    if constexpr (WEIGHTED) {
      ws = wnext;
      pix += (int64_t)dy + (int64_t)H * dx;
      if (t + 1 < len) wnext = w[pix];
    } else {
      ws = w;
    }
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
      u[j] = s[j] = 0.0;
      if (valid[j]) {
        u[j] = unary[row + j * kWave];
        if (accumulate) s[j] = S[row + j * kWave];
      }
      m[j] = t > 0 ? inf : 0.0;
    }
    if (t > 0) {
      const double *pv = prev[(t - 1) & 1];
      for (int l = 0; l < D; ++l) {
        const double a = pv[l], q = pos[l];
#pragma unroll
        for (int j = 0; j < LPL; ++j) {
          const double d = fabs(pk[j] - q);
          m[j] = fmin(m[j], a + ws * fmin(QUAD ? d * d : d, tol));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < LPL; ++j) {
      if (valid[j]) {
        const double L = t > 0 ? u[j] + m[j] : u[j];
        S[row + j * kWave] = accumulate ? s[j] + L : L;
        prev[t & 1][lane + j * kWave] = L;
      }
    }
    __syncthreads();
    row += stride;
  }
}

// S to labels, map and confidence: a group of 1 << lg lanes per pixel, a strided loop above 64 labels
// (trws_beliefs_finish_kernel's reduction: the lexicographic (value, label) minimum and the second-smallest value)
__global__ void __launch_bounds__(kFinishBlock)
    scanline_finish_kernel(const double *__restrict__ S, const double *__restrict__ positions, int D, int64_t N, int lg,
                           int32_t *__restrict__ labels, double *__restrict__ map, double *__restrict__ conf) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kFinishBlock / kWave) + (int)threadIdx.x / kWave;
  const int64_t p = wave * (kWave >> lg) + (lane >> lg);
  if (p >= N) return;                             // (whole groups: the xor partners below stay inside a group)
  const int G = 1 << lg;
  const int sub = lane & (G - 1);
  const size_t row = (size_t)p * D;
  double m1 = __builtin_huge_val(), m2 = __builtin_huge_val();
  int a1 = 0x7fffffff;
  for (int k = sub; k < D; k += G) {
    const double d = S[row + k];
    if (d < m1) { m2 = m1; m1 = d; a1 = k; }
    else if (d < m2) m2 = d;
  }
  for (int off = G >> 1; off > 0; off >>= 1) {
    const double o1 = __shfl_xor(m1, off, kWave), o2 = __shfl_xor(m2, off, kWave);
    const int oa = __shfl_xor(a1, off, kWave);
    if (o1 < m1 || (o1 == m1 && oa < a1)) { m2 = m1 < o2 ? m1 : o2; m1 = o1; a1 = oa; }
    else m2 = m2 < o1 ? m2 : o1;
  }
  if (sub == 0) {
    if (a1 >= D) a1 = 0;                          // (a row without one finite value below +Inf: still a label in range)
    labels[p] = a1 + 1;
    if (map) map[p] = positions[a1];
    if (conf) conf[p] = D == 1 ? __builtin_huge_val() : m2 - m1;
  }
}

int lanes_log2(int D) {
  int lg = 0;
  while ((1 << lg) < D && lg < 6) ++lg;
  return lg;
}

int check_args(const char *what, const void *unary, int H, int W, int D, const void *positions, int kernel, double tol,
               const int32_t *directions, const double *weights, bool weighted, int R, const void *S, bool need_S,
               const void *labels, char *err, size_t errcap) {
  // weighted: `weights` are the R x N step weights (their values are the host form's to check)
  const std::string w(what), wname(weighted ? "step_weights" : "weights");
  if (H < 1 || W < 1) return fail(w + ": H and W must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(w + ": H * W must be below 2^31 (pixel ids are int32)", err, errcap);
  if (D < 1 || D > kMaxLabels) return fail(w + ": D must be 1 .. " + std::to_string(kMaxLabels), err, errcap);
  if (kernel != 1 && kernel != 2) return fail(w + ": kernel must be 1 (truncated linear) or 2 (truncated quadratic)", err, errcap);
  if (!(tol >= 0.0)) return fail(w + ": tol must be non-negative", err, errcap);
  if (R < 1 || R > kMaxDirections) return fail(w + ": R (the number of directions) must be 1 .. " + std::to_string(kMaxDirections), err, errcap);
  if (!unary || !positions || !directions || !weights || !labels || (need_S && !S))
    return fail(w + ": unary, positions, directions, " + wname + (need_S ? ", S and labels must not be NULL"
                                                                         : " and labels must not be NULL"), err, errcap);
  if (S == unary) return fail(w + ": S must not be unary (the aggregation does not work in place)", err, errcap);
  if (weighted && S == weights) return fail(w + ": S must not be step_weights", err, errcap);
  for (int r = 0; r < R; ++r) {
    const int dy = directions[2 * r], dx = directions[2 * r + 1];
    if (dy < -1 || dy > 1 || dx < -1 || dx > 1 || (dy == 0 && dx == 0))
      return fail(w + ": a direction must be (dy, dx) with dy, dx in {-1, 0, 1}, not both 0 (direction " + std::to_string(r) +
                  " is (" + std::to_string(dy) + ", " + std::to_string(dx) + "))", err, errcap);
    if (!weighted && (!(weights[r] >= 0.0) || !std::isfinite(weights[r])))
      return fail(w + ": a weight must be finite and non-negative (weight " + std::to_string(r) + ")", err, errcap);
  }
  return 0;
}

template <int LG, bool WEIGHTED>
void launch_narrow(dim3 grid, hipStream_t s, const double *unary, const double *positions, int H, int W, int D, int kernel,
                   double tol, Weight<WEIGHTED> w, int dy, int dx, int chains, int acc, double *S) {
  hipLaunchKernelGGL((scanline_direction_kernel<LG, WEIGHTED>), grid, dim3(kWave), 0, s, unary, positions, H, W, D, kernel, tol, w, dy, dx,
                     chains, acc, S);
}

template <int LPL, bool WEIGHTED>
void launch_wide(dim3 grid, hipStream_t s, const double *unary, const double *positions, int H, int W, int D, int kernel,
                 double tol, Weight<WEIGHTED> w, int dy, int dx, int chains, int acc, double *S) {
  if (kernel == 2)
    hipLaunchKernelGGL((scanline_direction_wide_kernel<LPL, true, WEIGHTED>), grid, dim3(kWave), 0, s, unary, positions, H, W, D, tol, w,
                       dy, dx, chains, acc, S);
  else
    hipLaunchKernelGGL((scanline_direction_wide_kernel<LPL, false, WEIGHTED>), grid, dim3(kWave), 0, s, unary, positions, H, W, D, tol, w,
                       dy, dx, chains, acc, S);
}

template <bool WEIGHTED>
void launch_direction(const double *unary, const double *positions, int H, int W, int D, int kernel, double tol,
                      Weight<WEIGHTED> w, int dy, int dx, bool accumulate, double *S, hipStream_t s) {
  const int chains = chain_count(H, W, dy, dx);
  const int lg = lanes_log2(D);
  const int per_wave = D > kWave ? 1 : kWave >> lg;
  const dim3 grid((unsigned)((chains + per_wave - 1) / per_wave));
  const int acc = accumulate ? 1 : 0;
#define STEREO_SCANLINE_ARGS grid, s, unary, positions, H, W, D, kernel, tol, w, dy, dx, chains, acc, S
  if (D > 3 * kWave) launch_wide<4, WEIGHTED>(STEREO_SCANLINE_ARGS);
  else if (D > 2 * kWave) launch_wide<3, WEIGHTED>(STEREO_SCANLINE_ARGS);
  else if (D > kWave) launch_wide<2, WEIGHTED>(STEREO_SCANLINE_ARGS);
  else switch (lg) {
    case 0: launch_narrow<0, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    case 1: launch_narrow<1, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    case 2: launch_narrow<2, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    case 3: launch_narrow<3, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    case 4: launch_narrow<4, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    case 5: launch_narrow<5, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
    default: launch_narrow<6, WEIGHTED>(STEREO_SCANLINE_ARGS); break;
  }
#undef STEREO_SCANLINE_ARGS
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_all(const double *unary, int H, int W, int D, const double *positions, int kernel, double tol,
                const int32_t *directions, const double *weights, bool weighted, int R, double *S, int32_t *labels,
                double *map, double *confidence, hipStream_t s) {
  const int64_t N = (int64_t)H * W;
  for (int r = 0; r < R; ++r) {
    const int dy = directions[2 * r], dx = directions[2 * r + 1];
    if (weighted) launch_direction<true>(unary, positions, H, W, D, kernel, tol, weights + N * r, dy, dx, r > 0, S, s);
    else launch_direction<false>(unary, positions, H, W, D, kernel, tol, weights[r], dy, dx, r > 0, S, s);
  }
  stereo::scanline_finish(S, positions, D, (int64_t)H * W, labels, map, confidence, s);
}

// the bodies of the four entries, below them: `weighted` says what `weights` is (R doubles, or R x N step weights)
int aggregate_device(const char *what, const double *unary, int H, int W, int D, const double *positions, int kernel,
                     double tol, const int32_t *directions, const double *weights, bool weighted, int R, double *S,
                     int32_t *labels, double *map, double *confidence, void *stream, char *err, size_t errcap);
int aggregate_host(const char *what, const double *unary, int H, int W, int D, const double *positions, int kernel, double tol,
                   const int32_t *directions, const double *weights, bool weighted, int R, double *S, int32_t *labels,
                   double *map, double *confidence, char *err, size_t errcap);

}  // namespace

// (scanline_finish.h: the reduction as scanline_edges.hip launches it too)
void stereo::scanline_finish(const double *S, const double *positions, int D, int64_t N, int32_t *labels, double *map,
                             double *confidence, hipStream_t s) {
  const int lg = lanes_log2(D);
  const int64_t per_block = (int64_t)(kFinishBlock / kWave) * (kWave >> lg);
  hipLaunchKernelGGL(scanline_finish_kernel, dim3((unsigned)((N + per_block - 1) / per_block)), dim3(kFinishBlock), 0, s, S,
                     positions, D, N, lg, labels, map, confidence);
  STEREO_HIP_CHECK(hipGetLastError());
}

extern "C" {

int stereo_scanline_max_labels(void) { return kMaxLabels; }

int stereo_scanline_aggregate_device(const double *unary, int H, int W, int D, const double *positions, int kernel,
                                     double tol, const int32_t *directions, const double *weights, int R, double *S,
                                     int32_t *labels, double *map, double *confidence, void *stream, char *err,
                                     size_t errcap) {
  return aggregate_device("stereo_scanline_aggregate_device", unary, H, W, D, positions, kernel, tol, directions, weights,
                          false, R, S, labels, map, confidence, stream, err, errcap);
}

int stereo_scanline_aggregate_weighted_device(const double *unary, int H, int W, int D, const double *positions, int kernel,
                                              double tol, const int32_t *directions, const double *step_weights, int R,
                                              double *S, int32_t *labels, double *map, double *confidence, void *stream,
                                              char *err, size_t errcap) {
  return aggregate_device("stereo_scanline_aggregate_weighted_device", unary, H, W, D, positions, kernel, tol, directions,
                          step_weights, true, R, S, labels, map, confidence, stream, err, errcap);
}

int stereo_scanline_aggregate(const double *unary, int H, int W, int D, const double *positions, int kernel, double tol,
                              const int32_t *directions, const double *weights, int R, double *S, int32_t *labels,
                              double *map, double *confidence, char *err, size_t errcap) {
  return aggregate_host("stereo_scanline_aggregate", unary, H, W, D, positions, kernel, tol, directions, weights, false, R, S,
                        labels, map, confidence, err, errcap);
}

int stereo_scanline_aggregate_weighted(const double *unary, int H, int W, int D, const double *positions, int kernel,
                                       double tol, const int32_t *directions, const double *step_weights, int R, double *S,
                                       int32_t *labels, double *map, double *confidence, char *err, size_t errcap) {
  return aggregate_host("stereo_scanline_aggregate_weighted", unary, H, W, D, positions, kernel, tol, directions,
                        step_weights, true, R, S, labels, map, confidence, err, errcap);
}

}  // extern "C"

namespace {

int aggregate_device(const char *what, const double *unary, int H, int W, int D, const double *positions, int kernel,
                     double tol, const int32_t *directions, const double *weights, bool weighted, int R, double *S,
                     int32_t *labels, double *map, double *confidence, void *stream, char *err, size_t errcap) {
  if (int rc = check_args(what, unary, H, W, D, positions, kernel, tol, directions, weights, weighted, R, S, true, labels, err,
                          errcap))
    return rc;
  return guarded(what, err, errcap, [&] {
    launch_all(unary, H, W, D, positions, kernel, tol, directions, weights, weighted, R, S, labels, map, confidence,
               (hipStream_t)stream);
  });
}

int aggregate_host(const char *what, const double *unary, int H, int W, int D, const double *positions, int kernel, double tol,
                   const int32_t *directions, const double *weights, bool weighted, int R, double *S, int32_t *labels,
                   double *map, double *confidence, char *err, size_t errcap) {
  if (int rc = check_args(what, unary, H, W, D, positions, kernel, tol, directions, weights, weighted, R, S, false, labels, err,
                          errcap))
    return rc;
  const size_t n = (size_t)H * W, dn = n * (size_t)D;
  for (int k = 0; k < D; ++k)
    if (!std::isfinite(positions[k])) return fail(std::string(what) + ": positions must be finite", err, errcap);
  for (size_t i = 0; i < dn; ++i)
    if (!std::isfinite(unary[i])) return fail(std::string(what) + ": unary must be finite", err, errcap);
  if (weighted)                                   // (the entries that are read: those of pixels with a predecessor)
    for (int r = 0; r < R; ++r) {
      const int dy = directions[2 * r], dx = directions[2 * r + 1];
      for (int x = 0; x < W; ++x)
        for (int y = 0; y < H; ++y) {
          if (y - dy < 0 || y - dy >= H || x - dx < 0 || x - dx >= W) continue;
          const double v = weights[(size_t)r * n + (size_t)x * H + y];
          if (!(v >= 0.0) || !std::isfinite(v))
            return fail(std::string(what) + ": a step weight must be finite and non-negative (direction " + std::to_string(r) +
                        ", pixel " + std::to_string((size_t)x * H + y) + ")", err, errcap);
        }
    }
  return guarded(what, err, errcap, [&] {
    stereo::DevBuf<double> u, pos, vol, m, conf, wst;
    stereo::DevBuf<int32_t> lab;
    u.upload(unary, dn); pos.upload(positions, (size_t)D); vol.alloc(dn); lab.alloc(n);
    if (weighted) wst.upload(weights, n * (size_t)R);
    if (map) m.alloc(n);
    if (confidence) conf.alloc(n);
    launch_all(u.p, H, W, D, pos.p, kernel, tol, directions, weighted ? wst.p : weights, weighted, R, vol.p, lab.p,
               map ? m.p : nullptr, confidence ? conf.p : nullptr, nullptr);
    STEREO_HIP_CHECK(hipMemcpy(labels, lab.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (S) STEREO_HIP_CHECK(hipMemcpy(S, vol.p, dn * sizeof(double), hipMemcpyDeviceToHost));
    if (map) STEREO_HIP_CHECK(hipMemcpy(map, m.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (confidence) STEREO_HIP_CHECK(hipMemcpy(confidence, conf.p, n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

}  // namespace
