// TRW-S sweep kernel for 512 < K <= 4096 labels with ONE shared, finite, strictly ascending positions
// vector (q(:,e) = qprim(:,e) = pos for every edge), both smoothness kernels, both message modes, any
// graph the generic kernel takes.  Part of libstereo_hip.so; overview in trws_plan.hip, DESIGN.md 4.6.
//
// Same schedule as trws_generic.hip (persistent launch per sweep, run tickets, dependency flags with
// the epoch, bounded spin, primal pass fused into the forward sweep, lb_pos_node / lb_pos_edge), but a
// message of 8-32 KB fits neither a wave's registers nor the generic kernel's LDS hand-over slots:
//  * LDS holds Di, DiBackward, H = gamma Di - m, the positions and the list of useful sources (h < vTrunc);
//  * a node's outgoing messages are computed one after another by the whole workgroup, a thread owning
//    destinations t = tid, tid + kLBlock, ...;
//  * every message travels through HBM only: write-through stores (st_sc1), s_waitcnt vmcnt(0) before the
//    completion flag, ld_sc1 reads of messages produced inside the launch (also the workgroup's own).
// Messages (positions ascending: the sort permutation is the identity, sources in label order):
//  * alpha == 0: min H everywhere (typeStereoLinear.h:390-396);
//  * MINPLUS: min over the useful sources -- or, when there are more of them than the truncation window
//    is wide, over the sources within the window (a source farther than lambda, or sqrt(lambda (1 + 1e-9))
//    for kernel 2, costs >= vTrunc bit for bit) -- truncated at vTrunc;
//  * exact, kernel 1: the same min-plus (smallest and second smallest cost) plus the certificate of
//    trws_wide_kernel: delta margins to the second cost and to vTrunc, and the tangency count (a useful
//    cone i matches destination t when |cost_i(t) - h_t| <= delta; only i itself may match);
//  * exact, kernel 2: the same min-plus plus the hull-slope certificate of message_quad_fast;
//  * a failed certificate, STEREO_HIP_TRWS_CERTIFICATE=0, alpha <= 0 or lambda < 0: the reference's serial
//    construction (build_envelope) on one lane, its stack in a per-workgroup slab of global memory
//    (3 (K + 2) doubles do not fit next to Di).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stereo_hip.h"
#include "common.h"
#include "trws_dev.h"
#include "trws_launch.h"

namespace stereo {
namespace {

constexpr int kLBlock = 512;
constexpr int kLWaves = kLBlock / kWave;
constexpr int kLChunks = kLargeMaxK / kLBlock;  // destinations per thread at most
constexpr int kLRed = 64;                        // doubles of reduction scratch

static_assert(kLChunks * kLWaves <= kWave, "one wave scans the compaction counts");

// Workgroup reductions (every thread gets the result).  `red` is used by this call only; the caller
// separates two uses of the same slots by a barrier.
__device__ __forceinline__ void block_min_max(double &lo, double &hi, double *red, int lane, int wave) {
  wave_min_max_dpp(lo, hi);
  if (lane == 0) { red[wave] = lo; red[kLWaves + wave] = hi; }
  __syncthreads();
  lo = red[0]; hi = red[kLWaves];
#pragma unroll
  for (int w = 1; w < kLWaves; ++w) { lo = min_raw(lo, red[w]); hi = max_raw(hi, red[kLWaves + w]); }
}

__device__ __forceinline__ int block_sum(int v, int *red, int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kLWaves; ++w) s += red[w];
  return s;
}

struct LargeLds {
  double *Di, *Dbs, *H, *P, *red;
  int *ul, *cnt;
};

// One outgoing message of the node by the whole workgroup.  Returns vMin (uniform).
template <int KERNEL, int MODE>
__device__ double large_message(const DevParams &p, int e, double gamma, const LargeLds &L, double *slab, int tid,
                                int lane, int wave) {
  const int K = p.K;
  const double inf = __builtin_huge_val();
  double *m = p.msg + (size_t)e * K;
  const double alpha = p.alpha[e];
  const double *P = L.P;
  double *H = L.H;
  // ---- H = gamma Di - m (m: this node's own message of the previous sweep)
  double lo = inf, hi = -inf;
  for (int k = tid; k < K; k += kLBlock) {
    const double h = gamma * L.Di[k] - m[k];
    H[k] = h;
    lo = min_raw(lo, h); hi = max_raw(hi, h);
  }
  block_min_max(lo, hi, L.red, lane, wave);
  const double hmin = lo, hmax = hi;
  double vmin = hmin;
  if (alpha == 0) {
    // typeStereoLinear.h:390-396 / typeStereoQuadratic.h: the message is min H everywhere
    for (int k = tid; k < K; k += kLBlock) st_sc1(m + k, hmin - hmin);
    __syncthreads();
    return hmin;
  }
  const double vtrunc = hmin + alpha * p.lambda;
  // ---- the useful sources (h < vTrunc) in label (= position) order: counts per (chunk, wave), one
  // wave scans them, every thread places its own
  const int nchunk = (K + kLBlock - 1) / kLBlock;
  for (int c = 0; c < nchunk; ++c) {
    const int k = c * kLBlock + tid;
    const unsigned long long um = __builtin_amdgcn_ballot_w64(k < K && H[k] < vtrunc);
    if (lane == 0) L.cnt[c * kLWaves + wave] = __builtin_popcountll(um);
  }
  __syncthreads();
  if (wave == 0) {
    const int n = nchunk * kLWaves;
    const int v = lane < n ? L.cnt[lane] : 0;
    int s = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int o = __shfl_up(s, off, kWave);
      if (lane >= off) s += o;
    }
    if (lane < n) L.cnt[kWave + lane] = s - v;  // exclusive offsets
    if (lane == kWave - 1) L.cnt[2 * kWave] = s;
  }
  __syncthreads();
  const int nu = L.cnt[2 * kWave];
  for (int c = 0; c < nchunk; ++c) {
    const int k = c * kLBlock + tid;
    const bool useful = k < K && H[k] < vtrunc;
    const unsigned long long um = __builtin_amdgcn_ballot_w64(useful);
    if (useful) L.ul[L.cnt[kWave + c * kLWaves + wave] + __builtin_popcountll(um & ((1ull << lane) - 1))] = k;
  }
  __syncthreads();
  const int w = p.window;
  const bool sparse = nu <= 2 * w + 1;
  // (a negative weight or truncation: neither the window argument nor vMin = min H holds)
  const bool plain = alpha > 0 && p.lambda >= 0;
  bool serial = MODE == STEREO_TRWS_MESSAGES_EXACT && (!p.certificate || !plain);
  if (MODE != STEREO_TRWS_MESSAGES_EXACT && !plain) {
    // the brute-force min-plus over every source, as trws_generic.hip runs it
    double vloc = inf;
    for (int t = tid; t < K; t += kLBlock) {
      double best = vtrunc;
      for (int s = 0; s < K; ++s) {
        const double c = pair_cost<KERNEL>(alpha, P[t] - P[s], H[s]);
        best = c < best ? c : best;
      }
      vloc = min_raw(vloc, best);
    }
    double dummy = -inf;
    block_min_max(vloc, dummy, L.red + 2 * kLWaves, lane, wave);
    for (int t = tid; t < K; t += kLBlock) {
      double best = vtrunc;
      for (int s = 0; s < K; ++s) {
        const double c = pair_cost<KERNEL>(alpha, P[t] - P[s], H[s]);
        best = c < best ? c : best;
      }
      st_sc1(m + t, best - vloc);
    }
    __syncthreads();
    return vloc;
  }
  if (MODE != STEREO_TRWS_MESSAGES_EXACT) {
    // ---- plain min-plus: every other source costs >= vTrunc; min over t of the result is min H
    // (destination t sees source t at distance 0)
    for (int t = tid; t < K; t += kLBlock) {
      const double pt = P[t];
      double m1 = inf;
      if (sparse) {
        for (int jj = 0; jj < nu; ++jj) {
          const int j = L.ul[jj];
          m1 = min_raw(m1, pair_cost<KERNEL>(alpha, pt - P[j], H[j]));
        }
      } else {
        const int s0 = t - w < 0 ? 0 : t - w, s1 = t + w > K - 1 ? K - 1 : t + w;
        for (int s = s0; s <= s1; ++s) m1 = min_raw(m1, pair_cost<KERNEL>(alpha, pt - P[s], H[s]));
      }
      st_sc1(m + t, (m1 < vtrunc ? m1 : vtrunc) - hmin);
    }
    __syncthreads();
    return hmin;
  }
  if (!serial) {
    // ---- certified min-plus (trws_wide_kernel's certificate for each smoothness kernel)
    double delta;
    bool bad;
    const double ap0 = alpha * p.pos_first, ap1 = alpha * p.pos_last;
    if (KERNEL == 1) {
      const double mag = max_raw(fabs(hmin), fabs(hmax)) + 2 * max_raw(fabs(ap0), fabs(ap1));
      delta = 1e-9 * (mag + fabs(alpha * p.lambda));
      bad = !(delta < inf);
    } else {
      const double pmax = max_raw(fabs(p.pos_first), fabs(p.pos_last));
      const double scale = max_raw(fabs(hmin), fabs(hmax)) + 2 * (alpha * pmax * pmax);
      delta = 1e-9 * (scale + fabs(alpha * p.lambda) + fabs(vtrunc));
      bad = !(delta < inf) || !(p.pos_gap > 4e-8) || !(1e-13 * scale * (p.pos_last - p.pos_first) < delta * p.pos_gap);
    }
    int matches = 0;
    if (!bad) {
      for (int t = tid; t < K && !bad; t += kLBlock) {
        const double pt = P[t], ht = H[t];
        double m1 = inf, m2 = inf;
        if (sparse) {
          for (int jj = 0; jj < nu; ++jj) {
            const int j = L.ul[jj];
            const double cst = pair_cost<KERNEL>(alpha, pt - P[j], H[j]);
            const double lo_ = min_raw(m1, cst), hi_ = max_raw(m1, cst);
            m2 = min_raw(m2, hi_);  // second smallest; equal costs of two sources count
            m1 = lo_;
            if (KERNEL == 1) matches += fabs(cst - ht) <= delta ? 1 : 0;
          }
        } else {
          const int s0 = t - w < 0 ? 0 : t - w, s1 = t + w > K - 1 ? K - 1 : t + w;
          for (int s = s0; s <= s1; ++s) {
            const double cst = pair_cost<KERNEL>(alpha, pt - P[s], H[s]);
            const double lo_ = min_raw(m1, cst), hi_ = max_raw(m1, cst);
            m2 = min_raw(m2, hi_);
            m1 = lo_;
          }
          if (KERNEL == 1) {
            // the tangency count over every useful cone, not only the window's
            for (int jj = 0; jj < nu; ++jj) {
              const int j = L.ul[jj];
              const double cst = pair_cost<1>(alpha, pt - P[j], H[j]);
              matches += fabs(cst - ht) <= delta ? 1 : 0;
            }
          }
        }
        bad = bad || (m1 < vtrunc && !(m2 - m1 > delta && vtrunc - m1 > delta));
        // the value goes out now (vMin = min H, see above); a failed certificate overwrites it below
        st_sc1(m + t, (m1 < vtrunc ? m1 : vtrunc) - hmin);
      }
    }
    bad = __syncthreads_or(bad);
    if (KERNEL == 1 && !bad) bad = block_sum(matches, L.cnt + 2 * kWave + 8, lane, wave) != nu;
    serial = bad;
    if (serial && tid == 0 && p.fallbacks) atomicAdd(p.fallbacks, 1);
  } else if (tid == 0 && p.fallbacks) {
    atomicAdd(p.fallbacks, 1);
  }
  if (serial) {
    // ---- the reference's serial construction (typeStereoLinear.h:401-479 / typeStereoQuadratic.h:407-501)
    const int Kp = p.Kp;
    double *sh = slab, *sq = slab + (Kp + 2), *z = slab + 2 * (Kp + 2);
    if (tid == 0) {
      build_envelope<KERNEL>(K, alpha, H, P, sh, sq, z);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // while (z[j+1] < t) ++j: the first such j grows with t, so a thread resumes where its previous
    // (smaller) destination stopped
    double vloc = inf;
    int j = 0;
    for (int t = tid; t < K; t += kLBlock) {
      const double pt = P[t];
      while (z[j + 1] < pt) ++j;
      const double c = pair_cost<KERNEL>(alpha, pt - sq[j], sh[j]);
      vloc = min_raw(vloc, c < vtrunc ? c : vtrunc);
    }
    double dummy = -inf;
    block_min_max(vloc, dummy, L.red + 2 * kLWaves, lane, wave);
    vmin = vloc;
    j = 0;
    for (int t = tid; t < K; t += kLBlock) {
      const double pt = P[t];
      while (z[j + 1] < pt) ++j;
      const double c = pair_cost<KERNEL>(alpha, pt - sq[j], sh[j]);
      st_sc1(m + t, (c < vtrunc ? c : vtrunc) - vmin);
    }
  }
  __syncthreads();  // H, the list and the reduction slots are free for the next message
  return vmin;
}

// ---- persistent dataflow sweep (the schedule of trws_generic.hip's trws_persistent_kernel) ----------
template <int KERNEL, bool BACKWARD, int MODE, bool PRIMAL, bool UPDATE>
__global__ __launch_bounds__(kLBlock) void trws_large_kernel(DevParams p, int epoch) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int K = p.K, Kp = p.Kp;
  LargeLds L;
  L.Di = lds;
  L.Dbs = lds + Kp;
  L.H = lds + 2 * Kp;
  L.P = lds + 3 * Kp;
  L.red = lds + 4 * Kp;
  L.ul = (int *)(lds + 4 * Kp + kLRed);
  L.cnt = L.ul + Kp;  // 2 * kWave + 1 + 8 + kLWaves ints
  int *s_run = L.cnt + 3 * kWave;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  double *slab = p.large_scratch + (size_t)blockIdx.x * 3 * (size_t)(Kp + 2);
  constexpr int D = BACKWARD ? 1 : 0;
  const int32_t *optr = BACKWARD ? p.bptr : p.fptr, *oidx = BACKWARD ? p.bidx : p.fidx;
  const int32_t *iptr = BACKWARD ? p.fptr : p.bptr, *iidx = BACKWARD ? p.fidx : p.bidx;
  const int N = p.N;
  for (int k = tid; k < K; k += kLBlock) L.P[k] = p.pos[k];
  __syncthreads();
  for (;;) {
    if (tid == 0) *s_run = next_run<D>(p);
    __syncthreads();
    const int run = *s_run;
    __syncthreads();
    if (run >= p.nruns[D]) break;
    const int p0 = p.run_ptr[D][run], p1 = p.run_ptr[D][run + 1];
    for (int pos = p0; pos < p1; ++pos) {
      const int r = BACKWARD ? N - 1 - pos : pos;
      const int node = p.order[r];
      const int o0 = optr[r], o1 = optr[r + 1], i0 = iptr[r], i1 = iptr[r + 1];
      // ---- wait for the incoming neighbours that other workgroups own
      const int d0 = p.dep_ptr[D][r], nd = p.dep_ptr[D][r + 1] - d0;
      int gave_up = 0;
      if (tid < nd) {
        const int32_t *flag = p.done + p.dep_rank[D][d0 + tid];
        int spins = 0, v;
        long long t0 = 0;
        while ((v = ld_sc1(flag)) < epoch) {
          if (!keep_waiting(p, spins, t0, p.dep_rank[D][d0 + tid] >= p.n_own)) {
            report_give_up(p, r, p.dep_rank[D][d0 + tid], v, epoch);
            gave_up = 1;
            break;
          }
        }
      }
      if (__syncthreads_or(gave_up)) return;  // bounded spin: the host reports the failure
      // ---- primal of the previous iteration (needs the outgoing messages before the update)
      if (PRIMAL) {
        double bestv = __builtin_huge_val();
        int besti = 0x7fffffff;
        for (int k = tid; k < K; k += kLBlock) {
          double db = p.unary[(size_t)node * K + k];
          // incoming list of the forward order = backward edges (minimize.cpp:240-247)
          for (int i = i0; i < i1; ++i) {
            const int e = iidx[i];
            const int ks = ld_sc1(p.x + p.tail[e]);
            const double alpha = p.alpha[e];
            const double d = p.mdir[e] == 0 ? L.P[ks] - L.P[k] : L.P[k] - L.P[ks];
            const double v = KERNEL == 1 ? fabs(d) : d * d;
            db += alpha * (v < p.lambda ? v : p.lambda);
          }
          L.Dbs[k] = db;
          double di = db;
          for (int i = o0; i < o1; ++i) di += p.msg[(size_t)oidx[i] * K + k];
          if (di < bestv) { bestv = di; besti = k; }
        }
        wave_argmin(bestv, besti);
        if (lane == 0) { L.red[wave] = bestv; ((int *)(L.red + kLWaves))[wave] = besti; }
        __syncthreads();
        if (tid == 0) {
          double v = L.red[0];
          int bi = ((int *)(L.red + kLWaves))[0];
          for (int w = 1; w < kLWaves; ++w) {
            const double rv = L.red[w];
            const int ri = ((int *)(L.red + kLWaves))[w];
            if (rv < v || (rv == v && ri < bi)) { v = rv; bi = ri; }
          }
          st_sc1(p.x + node, bi);
          p.eterms[r] = L.Dbs[bi];
        }
        __syncthreads();
      }
      if (UPDATE) {
        // ---- Di = D + outgoing-list messages (from the previous sweep) + incoming ones (this sweep, HBM)
        double vloc = __builtin_huge_val();
        for (int k = tid; k < K; k += kLBlock) {
          double acc = p.unary[(size_t)node * K + k];
          for (int i = o0; i < o1; ++i) acc += p.msg[(size_t)oidx[i] * K + k];
          for (int i = i0; i < i1; ++i) acc += ld_sc1(p.msg + (size_t)iidx[i] * K + k);
          L.Di[k] = acc;
          vloc = acc < vloc ? acc : vloc;
        }
        if (BACKWARD) {
          vloc = wave_min(vloc);
          if (lane == 0) L.red[2 * kLWaves + wave] = vloc;
          __syncthreads();
          double vmin = L.red[2 * kLWaves];
#pragma unroll
          for (int w = 1; w < kLWaves; ++w) vmin = L.red[2 * kLWaves + w] < vmin ? L.red[2 * kLWaves + w] : vmin;
          for (int k = tid; k < K; k += kLBlock) L.Di[k] -= vmin;
          if (tid == 0) p.lbterms[p.lb_pos_node[r]] = vmin;
        }
        __syncthreads();  // Di complete
        const double gamma = p.gamma[r];
        for (int i = o0; i < o1; ++i) {
          const int e = oidx[i];
          const double v = large_message<KERNEL, MODE>(p, e, gamma, L, slab, tid, lane, wave);
          if (BACKWARD && tid == 0) p.lbterms[p.lb_pos_edge[e]] = v;
        }
      }
      // ---- publish: every storing wave drains, then one lane raises the flag
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) st_sc1(p.done + r, epoch);
    }
  }
}

}  // namespace

size_t large_lds_bytes(int Kp) {
  return sizeof(double) * (size_t)(4 * Kp + kLRed) + sizeof(int) * (size_t)(Kp + 3 * kWave + 2);
}

size_t large_scratch_doubles(int Kp) { return 3 * (size_t)(Kp + 2); }

// rows: [smoothness kernel 1 | 2][message mode 0 | 1]
#define LARGE_ENTRY(BW, PR, UP, KER, MD) (const void *)trws_large_kernel<KER, BW, MD, PR, UP>,
#define LARGE_ROW(KER, MD) {TRWS_SWEEP_VARIANTS(LARGE_ENTRY, KER, MD)}
static const SweepRow kLargeKernels[4] = {LARGE_ROW(1, 0), LARGE_ROW(1, 1), LARGE_ROW(2, 0), LARGE_ROW(2, 1)};
#undef LARGE_ROW
#undef LARGE_ENTRY

void large_set_attributes(int lds) { set_max_dynamic_lds(kLargeKernels, 4, lds); }

void launch_large(int kernel, int mode, int what, int blocks, size_t lds, hipStream_t s, const DevParams &p, int epoch) {
  launch_sweep(kLargeKernels[(kernel == 1 ? 0 : 1) * 2 + (mode == 0 ? 0 : 1)], what, blocks, kLBlock, lds, s, p, epoch);
}

}  // namespace stereo
