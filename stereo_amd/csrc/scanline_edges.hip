// Scanline aggregation on per-edge positions: the directional chain min-marginals of scanline.hip on
// the general model a TRW-S plan is bound to -- q / qprim K x E, one alpha per edge, K <= 64 -- along the four axis
// directions of the image grid, the edge table that finds a pixel pair's edges, and the terms of a labelling's energy.
// No reference counterpart.  The definition: include/stereo_hip.h.
//
// scanline_edges_direction_kernel<LG, QUAD> has scanline_direction_kernel's layout: a workgroup is ONE wave, a chain
// has a group of G = 2^LG >= K lanes, lane `sub` holds label `sub`, the previous pixel's vector goes through LDS with
// one barrier per step on two buffer sets taken in turn, and the lanes past K hold +Inf there (they never win and
// never make a NaN).  What differs: the step table
//     T[k, l] = alpha_a * min(v(|qprim(l, a) - q(k, a)|), tol) + alpha_b * min(v(|qprim(k, b) - q(l, b)|), tol)
// (a the edge oriented p' -> p, b the edge oriented p -> p') changes at every step, so no row of it lives in registers.
// Per step a lane loads its own q(sub, a), qprim(sub, a), q(sub, b), qprim(sub, b), alpha_a and alpha_b; the two
// l-indexed vectors qprim(., a) and q(., b) go into LDS next to L(p', .), and the unrolled loop over l is three
// broadcast reads, two |.| with min and product, one add, one add and one minimum (two running minima).  An absent
// slot runs the same code with alpha = 0 and positions 0: + 0.0.
//
// None of the loads depends on the recurrence: the rows of the next kAhead pixels (U, S and the four edge rows) are in
// flight in a register ring, and the table entries, from which an edge row's address comes, one ring turn further.
// Every candidate L + T is one add, U + min is one add, T is one add of two products (-ffp-contract=off): S equals the
// restatement (tests/scanline_edges_restate.py) bit for bit.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "scanline_finish.h"
#include "stereo_hip.h"

namespace {

using stereo::fail;
using stereo::guarded;

constexpr int kWave = 64;
constexpr int kMaxLabels = 64;
constexpr int kMaxDirections = 8;
constexpr int kBlock = 256;
constexpr int kAhead = 4;       // pixels of a chain whose rows are in flight

// ---- the edge table -------------------------------------------------------------------------------------------------

enum EdgeFault { kEdgeOk = 0, kEdgeLoop, kEdgeRange, kEdgeFar };

// the place of edge (i1, i2) in the table of an H x W grid of N pixels, or why it has none
__host__ __device__ inline EdgeFault edge_slot(uint32_t i1, uint32_t i2, int H, int64_t N, int64_t &index) {
  if (i1 == i2) return kEdgeLoop;
  if ((int64_t)i1 >= N || (int64_t)i2 >= N) return kEdgeRange;
  const int64_t lo = i1 < i2 ? i1 : i2, hi = i1 < i2 ? i2 : i1;
  int axis;
  if (hi - lo == 1 && hi % H != 0) axis = 0;        // (hi % H == 0: the first row of the next column)
  else if (hi - lo == H) axis = 1;
  else return kEdgeFar;
  index = (i1 < i2 ? 0 : 1) + 2 * (axis + 2 * hi);
  return kEdgeOk;
}

__global__ void __launch_bounds__(kBlock)
    scanline_edges_table_kernel(const uint32_t *__restrict__ conn, int64_t E, int H, int64_t N, int32_t *table, int32_t *bad) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= E) return;
  int64_t index = 0;
  if (edge_slot(conn[2 * e], conn[2 * e + 1], H, N, index) != kEdgeOk || atomicCAS(&table[index], -1, (int32_t)e) != -1)
    atomicAdd(bad, 1);
}

// ---- one direction --------------------------------------------------------------------------------------------------

template <int LG, bool QUAD>
__global__ void __launch_bounds__(kWave)
    scanline_edges_direction_kernel(const double *__restrict__ unary, const int32_t *__restrict__ table,
                                    const double *__restrict__ q, const double *__restrict__ qprim,
                                    const double *__restrict__ alphas, int H, int W, int K, int64_t E, double tol, int dy, int dx,
                                    int chains, int accumulate, double *S) {
  constexpr int G = 1 << LG;
  __shared__ double prevL[2][kWave], prevA[2][kWave], prevB[2][kWave];
  const int lane = (int)threadIdx.x;
  const int sub = lane & (G - 1);
  const int first = lane & ~(G - 1);             // the group's place in a buffer
  const int64_t c = (int64_t)blockIdx.x * (kWave >> LG) + (lane >> LG);
  const bool active = c < chains && sub < K;
  const int len = dx == 0 ? H : W;                // (every chain of an axis direction has this many pixels)
  const int64_t y0 = dx == 0 ? (dy > 0 ? 0 : H - 1) : c, x0 = dx == 0 ? c : (dx > 0 ? 0 : W - 1);
  const int64_t p0 = y0 + (int64_t)H * x0;
  const int64_t step = (int64_t)dy + (int64_t)H * dx;
  const bool up = step > 0;                       // the predecessor has the smaller pixel id: the pair is stored at p
  const int axis = dx != 0 ? 1 : 0;
  const double inf = __builtin_huge_val();
  const int2 *table2 = reinterpret_cast<const int2 *>(table);
  prevL[0][lane] = prevL[1][lane] = sub < K ? 0.0 : inf;
  prevA[0][lane] = prevA[1][lane] = 0.0;
  prevB[0][lane] = prevB[1][lane] = 0.0;
  __syncthreads();

  // step t's pair (p', p): a = the edge oriented p' -> p, b = the edge oriented p -> p' (-1: absent)
  auto lookup = [&](int t, int &ea, int &eb) {
    ea = eb = -1;
    if (active && t >= 1 && t < len) {
      const int64_t pix = p0 + (int64_t)t * step - (up ? 0 : step);
      const int2 v = table2[axis + 2 * pix];
      ea = up ? v.x : v.y;
      eb = up ? v.y : v.x;
      if (ea >= E) ea = -1;
      if (eb >= E) eb = -1;
    }
  };
  // ring entry of step t: U and S of p; of edge a the lane's q (k side) and qprim (l side), of edge b the lane's qprim
  // (k side) and q (l side); the two weights
  double ub[kAhead], sb[kAhead], ka[kAhead], la[kAhead], kb[kAhead], lb[kAhead], wa[kAhead], wb[kAhead];
  int ea[kAhead], eb[kAhead];
  auto fetch = [&](int t, int i, int a, int b) {
    ub[i] = sb[i] = ka[i] = la[i] = kb[i] = lb[i] = wa[i] = wb[i] = 0.0;
    if (active && t < len) {
      const int64_t row = (p0 + (int64_t)t * step) * K + sub;
      ub[i] = unary[row];
      if (accumulate) sb[i] = S[row];
      if (a >= 0) { ka[i] = q[(int64_t)a * K + sub]; la[i] = qprim[(int64_t)a * K + sub]; wa[i] = alphas[a]; }
      if (b >= 0) { kb[i] = qprim[(int64_t)b * K + sub]; lb[i] = q[(int64_t)b * K + sub]; wb[i] = alphas[b]; }
    }
  };
#pragma unroll
  for (int i = 0; i < kAhead; ++i) lookup(i, ea[i], eb[i]);
#pragma unroll
  for (int i = 0; i < kAhead; ++i) {
    fetch(i, i, ea[i], eb[i]);
    lookup(i + kAhead, ea[i], eb[i]);
  }
  for (int t0 = 0; t0 < len; t0 += kAhead) {
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int t = t0 + i;
      if (t < len) {                              // (wave uniform)
        const double u = ub[i], s = sb[i], qk = ka[i], pk = kb[i], alpha_a = wa[i], alpha_b = wb[i];
        fetch(t + kAhead, i, ea[i], eb[i]);
        lookup(t + 2 * kAhead, ea[i], eb[i]);
        double L = u;
        if (t > 0) {
          const double *pv = prevL[(t - 1) & 1] + first, *pa = prevA[(t - 1) & 1] + first, *pb = prevB[(t - 1) & 1] + first;
          auto candidate = [&](int l) {
            const double da = fabs(pa[l] - qk), db = fabs(pk - pb[l]);
            const double ca = alpha_a * fmin(QUAD ? da * da : da, tol), cb = alpha_b * fmin(QUAD ? db * db : db, tol);
            return pv[l] + (ca + cb);
          };
          double m0 = inf, m1 = inf;
#pragma unroll
          for (int l = 0; l < G; l += 2) {
            m0 = fmin(m0, candidate(l));
            if constexpr (G > 1) m1 = fmin(m1, candidate(l + 1));
          }
          L = u + fmin(m0, m1);
        }
        if (active) {
          const int next = (i + 1) % kAhead;      // (a constant once unrolled; holds step t + 1 by now: its l sides go where step t + 1 reads them)
          S[(p0 + (int64_t)t * step) * K + sub] = accumulate ? s + L : L;
          prevL[t & 1][lane] = L;
          prevA[t & 1][lane] = la[next];
          prevB[t & 1][lane] = lb[next];
        }
        __syncthreads();
      }
    }
  }
}

// ---- the terms of a labelling's energy ------------------------------------------------------------------------------

__global__ void __launch_bounds__(kBlock)
    scanline_edges_energy_kernel(const double *__restrict__ unary, int K, int64_t N, int64_t E, const uint32_t *__restrict__ conn,
                                 const double *__restrict__ q, const double *__restrict__ qprim,
                                 const double *__restrict__ alphas, int quad, double tol, const int32_t *__restrict__ labels,
                                 double *__restrict__ terms, int32_t *bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= N + E) return;
  double term = 0.0;
  if (i < N) {
    const int x = labels[i];
    if (x < 1 || x > K) atomicAdd(bad, 1);
    else term = unary[(x - 1) + (int64_t)K * i];
  } else {
    const int64_t e = i - N;
    const int64_t i1 = conn[2 * e], i2 = conn[2 * e + 1];
    if (i1 < N && i2 < N) {
      const int x1 = labels[i1], x2 = labels[i2];
      if (x1 >= 1 && x1 <= K && x2 >= 1 && x2 <= K) {
        const double d = fabs(qprim[(x1 - 1) + (int64_t)K * e] - q[(x2 - 1) + (int64_t)K * e]);
        term = alphas[e] * fmin(quad ? d * d : d, tol);
      }
    }
  }
  terms[i] = term;
}

// ---- host -----------------------------------------------------------------------------------------------------------

int lanes_log2(int K) {
  int lg = 0;
  while ((1 << lg) < K && lg < 6) ++lg;
  return lg;
}

int check_grid(const std::string &w, int H, int W, char *err, size_t errcap) {
  if (H < 1 || W < 1) return fail(w + ": H and W must be at least 1", err, errcap);
  if ((int64_t)H * (int64_t)W >= ((int64_t)1 << 31))
    return fail(w + ": H * W must be below 2^31 (pixel ids are int32)", err, errcap);
  return 0;
}

int check_edges(const std::string &w, int64_t E, char *err, size_t errcap) {
  if (E < 0 || E >= ((int64_t)1 << 31)) return fail(w + ": E must be 0 .. 2^31 - 1 (edge ids are int32)", err, errcap);
  return 0;
}

int check_model(const std::string &w, int K, int kernel, double tol, char *err, size_t errcap) {
  if (K < 1 || K > kMaxLabels) return fail(w + ": K must be 1 .. " + std::to_string(kMaxLabels), err, errcap);
  if (kernel != 1 && kernel != 2) return fail(w + ": kernel must be 1 (truncated linear) or 2 (truncated quadratic)", err, errcap);
  if (!(tol >= 0.0)) return fail(w + ": tol must be non-negative", err, errcap);
  return 0;
}

int check_directions(const std::string &w, const int32_t *directions, int R, char *err, size_t errcap) {
  if (R < 1 || R > kMaxDirections) return fail(w + ": R (the number of directions) must be 1 .. " + std::to_string(kMaxDirections), err, errcap);
  if (!directions) return fail(w + ": directions must not be NULL", err, errcap);
  for (int r = 0; r < R; ++r) {
    const int dy = directions[2 * r], dx = directions[2 * r + 1];
    const std::string which = " (direction " + std::to_string(r) + " is (" + std::to_string(dy) + ", " + std::to_string(dx) + "))";
    if (dy < -1 || dy > 1 || dx < -1 || dx > 1 || (dy == 0 && dx == 0))
      return fail(w + ": a direction must be (dy, dx) out of (0, 1), (0, -1), (1, 0), (-1, 0)" + which, err, errcap);
    if (dy != 0 && dx != 0)
      return fail(w + ": a direction must be (dy, dx) out of (0, 1), (0, -1), (1, 0), (-1, 0): the model has no diagonal edges" + which, err, errcap);
  }
  return 0;
}

// the host table; the message names the first offending edge
int build_table(const std::string &w, const uint32_t *conn, int64_t E, int H, int W, int32_t *table, char *err, size_t errcap) {
  const int64_t N = (int64_t)H * W;
  for (int64_t i = 0; i < 4 * N; ++i) table[i] = -1;
  for (int64_t e = 0; e < E; ++e) {
    const uint32_t i1 = conn[2 * e], i2 = conn[2 * e + 1];
    const std::string edge = w + ": edge " + std::to_string(e) + " (" + std::to_string(i1) + ", " + std::to_string(i2) + ") ";
    int64_t index = 0;
    switch (edge_slot(i1, i2, H, N, index)) {
      case kEdgeLoop: return fail(edge + "is a self-loop", err, errcap);
      case kEdgeRange: return fail(edge + "has an endpoint outside 0 .. " + std::to_string(N - 1), err, errcap);
      case kEdgeFar: return fail(edge + "does not join two 4-neighbours of the " + std::to_string(H) + " x " + std::to_string(W) + " grid", err, errcap);
      default: break;
    }
    if (table[index] != -1)
      return fail(edge + "is the second edge in this orientation between its pixels (edge " + std::to_string(table[index]) + " is the first)", err, errcap);
    table[index] = (int32_t)e;
  }
  return 0;
}

template <int LG>
void launch_lg(bool quad, dim3 grid, hipStream_t s, const double *unary, const int32_t *table, const double *q, const double *qprim,
               const double *alphas, int H, int W, int K, int64_t E, double tol, int dy, int dx, int chains, int acc, double *S) {
  if (quad)
    hipLaunchKernelGGL((scanline_edges_direction_kernel<LG, true>), grid, dim3(kWave), 0, s, unary, table, q, qprim, alphas, H, W, K,
                       E, tol, dy, dx, chains, acc, S);
  else
    hipLaunchKernelGGL((scanline_edges_direction_kernel<LG, false>), grid, dim3(kWave), 0, s, unary, table, q, qprim, alphas, H, W,
                       K, E, tol, dy, dx, chains, acc, S);
}

void launch_all(int kernel, const double *unary, int H, int W, int K, int64_t E, const int32_t *table, const double *q,
                const double *qprim, const double *alphas, double tol, const int32_t *directions, int R, double *S,
                int32_t *labels, double *confidence, hipStream_t s) {
  const int lg = lanes_log2(K);
  const int per_wave = kWave >> lg;
  const bool quad = kernel == 2;
  for (int r = 0; r < R; ++r) {
    const int dy = directions[2 * r], dx = directions[2 * r + 1];
    const int chains = dx == 0 ? W : H;
    const dim3 grid((unsigned)((chains + per_wave - 1) / per_wave));
    const int acc = r > 0 ? 1 : 0;
#define STEREO_SCANLINE_EDGES_ARGS quad, grid, s, unary, table, q, qprim, alphas, H, W, K, E, tol, dy, dx, chains, acc, S
    switch (lg) {
      case 0: launch_lg<0>(STEREO_SCANLINE_EDGES_ARGS); break;
      case 1: launch_lg<1>(STEREO_SCANLINE_EDGES_ARGS); break;
      case 2: launch_lg<2>(STEREO_SCANLINE_EDGES_ARGS); break;
      case 3: launch_lg<3>(STEREO_SCANLINE_EDGES_ARGS); break;
      case 4: launch_lg<4>(STEREO_SCANLINE_EDGES_ARGS); break;
      case 5: launch_lg<5>(STEREO_SCANLINE_EDGES_ARGS); break;
      default: launch_lg<6>(STEREO_SCANLINE_EDGES_ARGS); break;
    }
#undef STEREO_SCANLINE_EDGES_ARGS
    STEREO_HIP_CHECK(hipGetLastError());
  }
  stereo::scanline_finish(S, nullptr, K, (int64_t)H * W, labels, nullptr, confidence, s);
}

int check_aggregate(const std::string &w, int kernel, const void *unary, int H, int W, int K, int64_t E, const void *edges,
                    const char *edges_name, const void *q, const void *qprim, const void *alphas, double tol,
                    const int32_t *directions, int R, const void *S, bool need_S, const void *labels, char *err, size_t errcap) {
  if (int rc = check_grid(w, H, W, err, errcap)) return rc;
  if (int rc = check_model(w, K, kernel, tol, err, errcap)) return rc;
  if (int rc = check_edges(w, E, err, errcap)) return rc;
  if (int rc = check_directions(w, directions, R, err, errcap)) return rc;
  if (!unary || !labels || (need_S && !S))
    return fail(w + (need_S ? ": unary, S and labels must not be NULL" : ": unary and labels must not be NULL"), err, errcap);
  const bool is_table = std::string(edges_name) == "table";      // (the table is needed at E = 0 too: it says so)
  if (((is_table || E > 0) && !edges) || (E > 0 && (!q || !qprim || !alphas)))
    return fail(w + ": " + edges_name + ", q, qprim and alphas must not be NULL" +
                (is_table ? " (q, qprim and alphas may be at E = 0)" : " (they may be at E = 0)"), err, errcap);
  if (S == unary) return fail(w + ": S must not be unary (the aggregation does not work in place)", err, errcap);
  return 0;
}

}  // namespace

extern "C" {

int stereo_scanline_edges_max_labels(void) { return kMaxLabels; }

int stereo_scanline_edges_table(const uint32_t *conn, int64_t E, int H, int W, int32_t *table, char *err, size_t errcap) {
  const std::string w = "stereo_scanline_edges_table";
  if (int rc = check_grid(w, H, W, err, errcap)) return rc;
  if (int rc = check_edges(w, E, err, errcap)) return rc;
  if (!table || (E > 0 && !conn)) return fail(w + ": conn and table must not be NULL (conn may be at E = 0)", err, errcap);
  return build_table(w, conn, E, H, W, table, err, errcap);
}

int stereo_scanline_edges_table_device(const uint32_t *conn, int64_t E, int H, int W, int32_t *table, int32_t *bad, void *stream,
                                       char *err, size_t errcap) {
  const char *what = "stereo_scanline_edges_table_device";
  const std::string w = what;
  if (int rc = check_grid(w, H, W, err, errcap)) return rc;
  if (int rc = check_edges(w, E, err, errcap)) return rc;
  if (!table || !bad || (E > 0 && !conn)) return fail(w + ": conn, table and bad must not be NULL (conn may be at E = 0)", err, errcap);
  return guarded(what, err, errcap, [&] {
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    STEREO_HIP_CHECK(hipMemsetAsync(table, 0xff, (size_t)(4 * N) * sizeof(int32_t), s));
    STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
    if (E > 0) {
      hipLaunchKernelGGL(scanline_edges_table_kernel, dim3((unsigned)((E + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, conn, E, H, N,
                         table, bad);
      STEREO_HIP_CHECK(hipGetLastError());
    }
  });
}

int stereo_scanline_edges_aggregate_device(int kernel, const double *unary, int H, int W, int K, int64_t E, const int32_t *table,
                                           const double *q, const double *qprim, const double *alphas, double tol,
                                           const int32_t *directions, int R, double *S, int32_t *labels, double *confidence,
                                           void *stream, char *err, size_t errcap) {
  const char *what = "stereo_scanline_edges_aggregate_device";
  if (int rc = check_aggregate(what, kernel, unary, H, W, K, E, table, "table", q, qprim, alphas, tol, directions, R, S, true, labels,
                               err, errcap))
    return rc;
  return guarded(what, err, errcap, [&] {
    launch_all(kernel, unary, H, W, K, E, table, q, qprim, alphas, tol, directions, R, S, labels, confidence, (hipStream_t)stream);
  });
}

int stereo_scanline_edges_aggregate(int kernel, const double *unary, int H, int W, int K, int64_t E, const uint32_t *conn,
                                    const double *q, const double *qprim, const double *alphas, double tol,
                                    const int32_t *directions, int R, double *S, int32_t *labels, double *confidence, char *err,
                                    size_t errcap) {
  const char *what = "stereo_scanline_edges_aggregate";
  const std::string w = what;
  if (int rc = check_aggregate(w, kernel, unary, H, W, K, E, conn, "conn", q, qprim, alphas, tol, directions, R, S, false, labels, err,
                               errcap))
    return rc;
  const size_t n = (size_t)H * W, kn = n * (size_t)K, ke = (size_t)E * (size_t)K;
  for (size_t i = 0; i < kn; ++i)
    if (!std::isfinite(unary[i])) return fail(w + ": unary must be finite", err, errcap);
  for (size_t i = 0; i < ke; ++i)
    if (!std::isfinite(q[i]) || !std::isfinite(qprim[i])) return fail(w + ": q and qprim must be finite", err, errcap);
  for (int64_t e = 0; e < E; ++e)
    if (!(alphas[e] >= 0.0) || !std::isfinite(alphas[e]))
      return fail(w + ": an alpha must be finite and non-negative (edge " + std::to_string(e) + ")", err, errcap);
  std::vector<int32_t> table(4 * n);
  if (int rc = build_table(w, conn, E, H, W, table.data(), err, errcap)) return rc;
  return guarded(what, err, errcap, [&] {
    stereo::DevBuf<double> u, dq, dqp, da, vol, conf;
    stereo::DevBuf<int32_t> tab, lab;
    u.upload(unary, kn); dq.upload(q, ke); dqp.upload(qprim, ke); da.upload(alphas, (size_t)E); tab.upload(table.data(), 4 * n);
    vol.alloc(kn); lab.alloc(n);
    if (confidence) conf.alloc(n);
    launch_all(kernel, u.p, H, W, K, E, tab.p, dq.p, dqp.p, da.p, tol, directions, R, vol.p, lab.p, confidence ? conf.p : nullptr,
               nullptr);
    STEREO_HIP_CHECK(hipMemcpy(labels, lab.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (S) STEREO_HIP_CHECK(hipMemcpy(S, vol.p, kn * sizeof(double), hipMemcpyDeviceToHost));
    if (confidence) STEREO_HIP_CHECK(hipMemcpy(confidence, conf.p, n * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int stereo_scanline_edges_energy_device(int kernel, const double *unary, int K, int64_t N, int64_t E, const uint32_t *conn,
                                        const double *q, const double *qprim, const double *alphas, double tol,
                                        const int32_t *labels, double *terms, int32_t *bad, void *stream, char *err,
                                        size_t errcap) {
  const char *what = "stereo_scanline_edges_energy_device";
  const std::string w = what;
  if (N < 1 || N >= ((int64_t)1 << 31)) return fail(w + ": N must be 1 .. 2^31 - 1 (pixel ids are int32)", err, errcap);
  if (int rc = check_model(w, K, kernel, tol, err, errcap)) return rc;
  if (int rc = check_edges(w, E, err, errcap)) return rc;
  if (!unary || !labels || !terms || !bad) return fail(w + ": unary, labels, terms and bad must not be NULL", err, errcap);
  if (E > 0 && (!conn || !q || !qprim || !alphas))
    return fail(w + ": conn, q, qprim and alphas must not be NULL (they may be at E = 0)", err, errcap);
  return guarded(what, err, errcap, [&] {
    hipStream_t s = (hipStream_t)stream;
    STEREO_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(scanline_edges_energy_kernel, dim3((unsigned)((N + E + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, unary, K, N, E,
                       conn, q, qprim, alphas, kernel == 2 ? 1 : 0, tol, labels, terms, bad);
    STEREO_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
