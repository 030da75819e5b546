// The speculative schedule (trws_graph.h: Sweep::Spec): first what both runners share (word layout, LDS
// waits, publisher, the segment commit; trws_wspec.h holds the wide kernel's runner), then the RUNNER of trws_pipe_kernel
// with shared uniformly spaced positions and the linear kernel.  One workgroup draws the runner's ticket and walks the whole cut run
// computing nothing but the recurrence that makes the run serial:
//   wave 0      messages: Di of node i from the staged prefix sum and the row(s) node i - 1 handed over, H = gamma Di - m,
//               plain windowed min-plus (what message_regs returns whenever its certificate holds), the row for node i + 1
//               stays in registers -- no certificate, no tangency keys, no barrier, ~100 instructions per visit;
//   wave 1      labels of the primal pass: x_i from x_(i-1), exact (the same operations as the primal wave of a visit);
//   waves 2-9   loaders: host-made record of node i (trws_runner_records.h), its foreign flags, unary + message rows, prefix
//               sum in list order, into a ring of kRunSlots staged nodes in LDS (node i belongs to loader i mod 8);
//   wave 10     publisher: at every cut, the rows / label of the node in front go to p.spec_rows / p.spec_x, drained, then
//               the segment's flag done[N + s].
// Nothing here decides a result: the segments recompute every visit with the certified routine and compare what they
// started from with what the segment in front produced (spec_commit).  A wrong row costs a second walk of one or
// more segments, never a wrong bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trws_dev.h"
#include "trws_runner_records.h"

namespace stereo {
namespace {

// ==== shared by both runners (this file: trws_pipe_kernel, K <= 64; trws_wspec.h: trws_wide_kernel, 64 < K <= 256) ====
// A runner's LDS: a ring of staged nodes, slot layout in rows of R = 64 C labels (C: 64-label chunks per lane) -- prefix
// sum P | up to three staged rows of the tail | old rows of the (up to two) messages to compute | unary | the node's own
// (outgoing) rows | words -- then per runner the H table(s), the rows for the publisher and 64 words:
//   labels consumed 13 | label published x 2: 16 | slots freed 18 | label x 2: 20 | node x 2: 22 | row kinds x 2: 24 |
//   rows published, per message wave, x 2: 32-39 (the rest per runner)
constexpr int kSwConsP = 13, kSwPubP = 16, kSwFree = 18, kSwLabel = 20, kSwNode = 22, kSwKinds = 24, kSwPubM = 32;
// words of a staged node: tail length | tail kinds (a nibble each: 0-2 staged row, 8 / 9 first / second handed-over row;
// the length once more in bits 16-) | messages to compute (0, 1, 2) | cut: segment that starts behind this node (0: none)
// | kinds of that segment's first node's rows (a nibble per row) | n_out | incoming rows | their label (-1: the node in
// front) x 4 | their direction bits | node id | word 15: the TAG, schedule position + 1, written last (behind a release
// fence): a reader that finds it finds the node.  doubles 8-15: alpha x 2, gamma, alpha of the incoming rows x 4
constexpr int kRsNt = 0, kRsKinds = 1, kRsNmsg = 2, kRsCut = 5, kRsPubKinds = 6, kRsNout = 7, kRsNin = 8, kRsSrc = 9, kRsMd = 13,
              kRsNode = 14, kRsTag = 15;

// Words of the runner's LDS, addressed AS LDS: through a generic pointer these become flat accesses, whose completion is
// counted together with the global loads -- a loader that polls a word would wait for the rows it has just requested
// for its next node; the fences are LDS-only for the same reason.
typedef __attribute__((address_space(3))) int spec_lds_int;
__device__ __forceinline__ int lds_load(const int *w) { return __hip_atomic_load((const spec_lds_int *)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_store(int *w, int v) { __hip_atomic_store((spec_lds_int *)w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// The dynamic LDS allocation as a role of the runner addresses it.  The roles are real (noinline) functions: there the
// compiler finds the allocation's offset in a table in memory, and between the compiler barriers of a visit it loads
// that word again -- a scalar load and a full wait on the path of every visit.  Read once and pinned to a scalar
// register, the offset is a value like any other for the whole walk.
typedef __attribute__((address_space(3))) double spec_lds_double;
__device__ __forceinline__ double *pinned_lds(double *dyn) {
  unsigned off = (unsigned)(size_t)(spec_lds_double *)dyn;
  asm volatile("" : "+s"(off));
  return (double *)(spec_lds_double *)(size_t)off;
}
#define SPEC_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local")
#define SPEC_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local")

// The bound of the waits below.  Everything a runner's waves wait for inside the workgroup ends with a loader's wait for
// another workgroup, which is bounded by the wall clock and raises the abort word when it gives up; a wait looks at that
// word (and, as a last resort against a hang, at the clock itself) every MASK + 1 polls.
template <int MASK>
__device__ __forceinline__ bool spec_keep_waiting(int &spins, long long &t0, int *abort_word, int32_t *abort_flag, long long spin_ticks) {
  spins = (spins + 1) & MASK;
  if (spins != 0) return true;
  if (lds_load(abort_word) || ld_sc1(abort_flag)) return false;
  const long long now = (long long)wall_clock64();
  if (t0 == 0) { t0 = now | 1; return true; }
  if (now - t0 > 4 * spin_ticks) { lds_store(abort_word, 1); return false; }
  return true;
}
// Waits until *word >= want.  SLEEP: an s_sleep between polls; without it (waits inside a loader's turn or the labels'
// visit, which are short) the clock is looked at every 4096 polls.
template <bool SLEEP>
__device__ __forceinline__ bool run_wait_i(const int *word, int want, int *abort_word, int32_t *abort_flag, long long spin_ticks) {
  int spins = 0;
  long long t0 = 0;
  while (lds_load(word) < want) {
    if (SLEEP) __builtin_amdgcn_s_sleep(1);
    if (!spec_keep_waiting<SLEEP ? 1023 : 4095>(spins, t0, abort_word, abort_flag, spin_ticks)) return false;
  }
  SPEC_ACQUIRE();
  return true;
}
// (the same as a call: the slow path of a visit that found its node not staged yet)
__device__ __attribute__((noinline)) bool run_wait(const int *word, int want, int *abort_word, int32_t *abort_flag, long long spin_ticks) {
  return run_wait_i<true>(word, want, abort_word, abort_flag, spin_ticks);
}
// ... until all of words[0 .. N - 1] >= want (N = 1: the sleeping wait; N = 4: 16-byte aligned, the four words come with
// ONE LDS read per look)
template <int N>
__device__ __forceinline__ bool run_wait_n(const int *words, int want, int *abort_word, int32_t *abort_flag, long long spin_ticks) {
  static_assert(N == 1 || N == 4, "run_wait_n");
  if (N == 1) return run_wait_i<true>(words, want, abort_word, abort_flag, spin_ticks);
  typedef int spec_v4i __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) const volatile spec_v4i spec_lds_v4i;
  int spins = 0;
  long long t0 = 0;
  for (;;) {
    const spec_v4i v = *(spec_lds_v4i *)words;
    if (min(min(v.x, v.y), min(v.z, v.w)) >= want) break;
    if (!spec_keep_waiting<4095>(spins, t0, abort_word, abort_flag, spin_ticks)) return false;
  }
  SPEC_ACQUIRE();
  return true;
}

// Arguments of a real (non-inlined) device function arrive in vector registers and the compiler must take them, and
// everything loaded through them, for lane-varying: every branch on such a value becomes an exec-mask region, every loop
// bound a mask loop.  They ARE uniform: the fields the runner and the commit use are read once and declared so.
template <class T>
__device__ __forceinline__ T uniform_value(T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "uniform_value");
  if (sizeof(T) == 4) {
    int w;
    __builtin_memcpy(&w, &v, 4);
    w = __builtin_amdgcn_readfirstlane(w);
    __builtin_memcpy(&v, &w, 4);
  } else {
    int w[2];
    __builtin_memcpy(w, &v, 8);
    w[0] = __builtin_amdgcn_readfirstlane(w[0]); w[1] = __builtin_amdgcn_readfirstlane(w[1]);
    __builtin_memcpy(&v, w, 8);
  }
  return v;
}
__device__ __forceinline__ DevParams uniform_params(const DevParams *pp) {
  DevParams q;
#define U(f) q.f = uniform_value(pp->f)
  U(K); U(lambda); U(unary); U(msg); U(pos); U(alpha); U(x); U(done); U(abort_flag); U(spin_ticks); U(n_own); U(N);
  U(desc[0]); U(desc[1]); U(window); U(uniform_step); U(spec_c0[0]); U(spec_c0[1]); U(spec_c1[0]); U(spec_c1[1]);
  U(spec_len); U(spec_nseg); U(spec_max_len); U(spec_rows); U(spec_x); U(spec_undo); U(spec_stat); U(timeline); U(tl_stride); U(debug);
  U(run_rec[0]); U(run_rec[1]);
#undef U
  return q;
}

// The first ticket of a sweep, drawn before the visit loops exist: ticket 0 is the runner's (run -1), which the workgroup
// that draws it serves at once; `word`: an LDS word the visit loops do not hold yet.
template <int D>
__device__ __forceinline__ int draw_first_ticket(const DevParams &p, int *word) {
  if (threadIdx.x == 0) *word = next_run<D>(p);
  __syncthreads();
  const int run = __builtin_amdgcn_readfirstlane(*word);
  __syncthreads();
  return run;
}

// ---- the publisher: at every cut the rows / label of the node in front go to p.spec_rows / p.spec_x, drained, then the
// segment's flag done[N + s].  RL: the runner's layout (C chunks, LDS base, rows for the publisher, words, abort word).
template <class RL, bool PRIMAL, bool UPDATE>
__device__ __attribute__((noinline)) void run_publisher(const DevParams *pp_, int epoch_) {
  extern __shared__ __attribute__((aligned(16))) double spec_lds[];
  const DevParams p = uniform_params(pp_);
  constexpr int R = RL::C * kWave;
  double *rb = spec_lds + RL::kBase;
  int *abort_word = (int *)spec_lds + RL::kAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  const int epoch = __builtin_amdgcn_readfirstlane(epoch_);
  const int K = p.K;
  int *rw = (int *)(rb + RL::kWords);
  for (int s = 1; s < p.spec_nseg; ++s) {
    const int ps = s & 1;
    if (UPDATE) {
      if (!run_wait_n<RL::C>(rw + kSwPubM + 4 * ps, s, abort_word, p.abort_flag, p.spin_ticks)) return;
      const double *pb = rb + RL::kPub + ps * 2 * R;
      const int kinds = lds_load(rw + kSwKinds + ps);
#pragma unroll
      for (int c = 0; c < RL::C; ++c) {
        const int kk = c * kWave + lane;
        if (kk < K) {
          double a0 = pb[kk], a1 = pb[R + kk];
          if ((p.debug & 16384) && s % 3 == 1 && kk == 0) a0 = __longlong_as_double(__double_as_longlong(a0) ^ 1ll);   // (development: a wrong row)
          if ((p.debug & 65536) && s % 3 == 1 && (kk & 1)) a0 += 0.375;                                                // (development: a VERY wrong row)
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int kd = (kinds >> (4 * k)) & 15;
            if (kd) st_sc1(p.spec_rows + ((size_t)s * 8 + k) * K + kk, kd == 8 ? a0 : a1);
          }
        }
      }
    }
    if (PRIMAL) {
      if (!run_wait_i<true>(rw + kSwPubP + ps, s, abort_word, p.abort_flag, p.spin_ticks)) return;
      int label = lds_load(rw + kSwLabel + ps);
      if ((p.debug & 32768) && s % 5 == 2) label = label > 0 ? label - 1 : (K > 1 ? 1 : 0);                          // (development: a wrong label)
      if (lane == 0) st_sc1(p.spec_x + s, label);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) { st_sc1(p.done + p.N + s, epoch); lds_store(rw + kSwFree, s); }
  }
}

// ---- commit of a speculative segment (called by all WAVES waves of the workgroup behind the barrier that ended the
// segment's last visit: the storer has drained the last node's rows).  The segment in front commits first (its flag);
// then what this segment started from is compared, bit for bit, with what that segment's last node really handed over:
// equal -> every visit here saw the sequential sweep's inputs and the nodes' flags go up; different (the runner's plain
// min-plus row was not the reference's envelope, or a row of the runner's was stale) -> the overwritten rows are put back
// and the caller walks the visits again from the real rows.  ctl: the kernel's control words ([1] abort, [3] walk again,
// [VERDICT] free between visits).  Returns 0 committed, 1 walk again (ctl[3] set), 2 gave up (p.abort_flag raised: the
// abort word may also have come from a wait of the visits that reports nothing itself).
template <int C, int WAVES, int VERDICT, bool BACKWARD, bool PRIMAL, bool UPDATE>
__device__ __attribute__((noinline)) int spec_commit(const DevParams *pp_, int epoch_, int p0_, int p1_, int seg_, int compare_, int ctl_off_) {
  extern __shared__ __attribute__((aligned(16))) double spec_lds[];
  const DevParams &p = *pp_;
  const int epoch = epoch_, p0 = p0_, p1 = p1_, seg = seg_, compare = compare_;
  constexpr int D = BACKWARD ? 1 : 0;
  constexpr int DW = TrwsGraph::kDescWords;
  const int32_t *desc = p.desc[D];
  int *ctl = (int *)spec_lds + ctl_off_;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int K = p.K;
  if (compare) {
    if (wave == 0) {
      int differ = 0;
      if (!wait_flag(p, p.N + p.spec_nseg + seg, epoch, -2)) { if (lane == 0) ctl[1] = 1; }
      else {
        const int w = desc[(size_t)p0 * DW + lane];
        const int f = __builtin_amdgcn_readlane(w, 2);
        const int nout = f & 15, ntot = nout + ((f >> 4) & 15);
        for (int j = nout; j < ntot; ++j) {
          if (__builtin_amdgcn_readlane(w, 12 + j) < 0) continue;
          if (UPDATE) {
            const size_t ea = ((size_t)seg * 8 + j) * K, eb = (size_t)__builtin_amdgcn_readlane(w, 4 + j) * K;
            for (int c = 0; c < C; ++c) {
              const int kk = c * kWave + lane, kc = kk < K ? kk : K - 1;
              const double a = ld_sc1(p.spec_rows + ea + kc), b = ld_sc1(p.msg + eb + kc);
              differ |= UNI(__double_as_longlong(a) != __double_as_longlong(b)) ? 1 : 0;
            }
          }
          if (PRIMAL) differ |= ld_sc1(p.spec_x + seg) != ld_sc1(p.x + __builtin_amdgcn_readlane(w, 32 + j)) ? 1 : 0;
        }
      }
      if (lane == 0) ctl[VERDICT] = differ;
    }
    __syncthreads();
    const int differ = __builtin_amdgcn_readfirstlane(ctl[VERDICT]);
    const int gave_up = __builtin_amdgcn_readfirstlane(ctl[1]);
    __syncthreads();
    if (tid == 0) ctl[VERDICT] = 0;
    if (gave_up) { if (tid == 0) st_sc1(p.abort_flag, 1); return 2; }
    if (differ) {
      if (UPDATE) {
        for (int pos = p0 + wave; pos < p1; pos += WAVES) {
          const int w = desc[(size_t)pos * DW + lane];
          const int nout = __builtin_amdgcn_readlane(w, 2) & 15;
          for (int j = 0; j < nout && j < 4; ++j) {
            const size_t em = (size_t)__builtin_amdgcn_readlane(w, 4 + j) * K, eu = ((size_t)(seg * p.spec_max_len + (pos - p0)) * 4 + j) * K;
            for (int c = 0; c < C; ++c) {
              const int kk = c * kWave + lane;
              if (kk < K) st_sc1(p.msg + em + kk, ld_sc1(p.spec_undo + eu + kk));
            }
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // (the second walk's plain loads must not find this CU's L1 holding anything of the first)
      }
      if (tid == 0) { ctl[3] = 1; if (p.spec_stat) atomicAdd(p.spec_stat, 1ull); }
      __syncthreads();
      return 1;
    }
  }
  if (wave == 0) {
    // the segment behind first (the commits are a serial chain), then the nodes' own flags
    if (seg + 1 < p.spec_nseg && lane == 0) st_sc1(p.done + p.N + p.spec_nseg + seg + 1, epoch);
    for (int pos = p0 + lane; pos < p1; pos += kWave) st_sc1(p.done + desc[(size_t)pos * DW + 1], epoch);
    if (lane == 0 && p.spec_stat) atomicAdd(p.spec_stat + 1, 1ull);
  }
  return 0;
}

// ---- the runner's entry: ring words and tags cleared, +inf on both sides of the H table(s), RL::prepare, the roles by
// wave -- RL::kMsgWaves message waves, the labels, RL::kLoaders loaders, the publisher -- and the development stamps
// (timeline[2 tl_stride + D]; spec_stat[8 + 4 D + ...]: when the messages, the labels, the last loader and the publisher
// were done, 100 MHz ticks since the roles started).  RL also gives the layout (C, base, slots, tables, words, abort word)
// and kOverlay: the runner's LDS overlays the visit loops' (which clear it, so an abort word left up goes to p.abort_flag).
// (noinline, parameters through a pointer to their copy in global memory, LDS through the dynamic allocation's own
//  symbol: nothing of this routine -- registers, scalars, the parameter block's address -- leaks into the kernel it is
//  called from, whose visit loops sit at the register limits; it is called before they exist)
template <class RL, bool BACKWARD, bool PRIMAL, bool UPDATE>
__device__ __attribute__((noinline)) void chain_runner(const DevParams *pp_, int epoch_) {
  extern __shared__ __attribute__((aligned(16))) double spec_lds[];
  const DevParams &p = *pp_;
  const int epoch = epoch_;
  constexpr int R = RL::C * kWave, M = RL::kMsgWaves, D = BACKWARD ? 1 : 0;
  double *rb = spec_lds + RL::kBase;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int c0 = p.spec_c0[D], c1 = p.spec_c1[D];
  int *rw = (int *)(rb + RL::kWords);
  if (tid < 64) rw[tid] = 0;
  if (tid < RL::kSlots) ((int *)(rb + tid * RL::kSlotDoubles + RL::kSc))[kRsTag] = 0;   // (no node staged)
  if (tid < 32 * RL::kTabs) {
    const int t = tid >> 5, e = tid & 31;
    rb[RL::kTab + t * (R + 32) + (e < 16 ? e : R + e)] = __builtin_huge_val();
  }
  RL::prepare(p, rb, tid);
  if (p.timeline && tid == 0) p.timeline[((size_t)2 * p.tl_stride + D) * 2] = wall_clock64();
  __syncthreads();
  const unsigned long long trole0 = wall_clock64();
  if (wave < M) { if (UPDATE) { __builtin_amdgcn_s_setprio(3); RL::template messages<BACKWARD>(pp_, wave); __builtin_amdgcn_s_setprio(0); } }
  else if (wave == M) { if (PRIMAL) { __builtin_amdgcn_s_setprio(3); RL::template labels<BACKWARD>(pp_); __builtin_amdgcn_s_setprio(0); } }
  else if (wave < M + 1 + RL::kLoaders) RL::template loader<BACKWARD, PRIMAL, UPDATE>(pp_, epoch, wave - M - 1);
  else if (wave == M + 1 + RL::kLoaders) run_publisher<RL, PRIMAL, UPDATE>(pp_, epoch);
  if (p.timeline && p.spec_stat && (tid & (kWave - 1)) == 0 && (wave == 0 || wave == M || wave == M + RL::kLoaders || wave == M + 1 + RL::kLoaders))
    p.spec_stat[8 + 4 * D + (wave == 0 ? 0 : wave == M ? 1 : wave == M + RL::kLoaders ? 2 : 3)] = wall_clock64() - trole0;
  __syncthreads();
  if (RL::kOverlay && lds_load((int *)spec_lds + RL::kAbortInt) && tid == 0) st_sc1(p.abort_flag, 1);
  if (p.timeline && tid == 0) p.timeline[((size_t)2 * p.tl_stride + D) * 2 + 1] = wall_clock64();
  if (p.spec_stat && tid == 0) atomicAdd(p.spec_stat + 2, (unsigned long long)(c1 - c0));
  if (RL::kOverlay) __syncthreads();
}

// ==== the runner of trws_pipe_kernel (K <= 64: one label per lane) ====================================================
constexpr int kRunSlots = 10;
constexpr int kRunLoaders = 8;
constexpr int kRunRowP = 0, kRunRowS = 64, kRunRowM = 256, kRunRowTH = 384, kRunRowOUT = 448, kRunSc = 704;
constexpr int kRunSlotDoubles = kRunSc + 16;
constexpr int kRunTab = kRunSlots * kRunSlotDoubles;   // 16 + 64 + 16: H with +inf on both sides
constexpr int kRunPub = kRunTab + 96;                  // 2 x (2 rows): what the publisher stores
constexpr int kRunWords = kRunPub + 256;               // 64 ints (above; 12: nodes consumed by the message wave)
constexpr int kRunDoubles = kRunWords + 32;
constexpr int kRunDummy = 32;                           // 64 more words: where the lanes that have nothing to say store (run_visit_m)
constexpr int kRwConsM = 12;
constexpr int kRunBase = kPipeLdsDoubles, kRunAbortInt = 2 * kPipeCtlOff + 1;   // (behind the visit loops' LDS; abort word: ctl[1])

#define RLI(v, i) __builtin_amdgcn_readlane((v), (i))

// ---- wave 0: the message recurrence ------------------------------------------------------------------------------
// What a visit reads from its staged node, requested in one go and WITHOUT waiting for the node to be there: the words
// first (tag included: one instruction, one snapshot), the rows behind a compiler barrier -- LDS serves a wave's
// requests in order, so rows that follow a tag that was found are the node's.  The next node's requests go out while
// this node's window is computed; a tag that was not there yet is waited for at the top of the next visit.
struct RunNodeM {
  int sw;
  double sd, P, S0, S1, S2, M0, M1;
};
__device__ __forceinline__ void run_request_m(const double *sl, int lane, RunNodeM &n) {
  n.sw = ((const int *)(sl + kRunSc))[lane & 15];
  asm volatile("" ::: "memory");
  n.sd = sl[kRunSc + 8 + (lane & 7)];
  n.P = sl[kRunRowP + lane]; n.S0 = sl[kRunRowS + lane]; n.S1 = sl[kRunRowS + 64 + lane]; n.S2 = sl[kRunRowS + 128 + lane];
  n.M0 = sl[kRunRowM + lane]; n.M1 = sl[kRunRowM + 64 + lane];
}
// What the routine needs of the launch parameters, as uniform values (read once by chain_runner).
struct RunArgsM {
  int K, window, c0, c1;
  double lambda, step;
  int32_t *abort_flag;
  long long spin_ticks;
  unsigned long long *stat;
};

// One visit of the recurrence.  `cur`: the node's words and rows (asked for during the previous visit), `nxt`: where the
// next node's go.  Everything that steers the visit is a scalar; the lanes only ever do the arithmetic.
template <bool BACKWARD, int G>
__device__ __forceinline__ bool run_visit_m(const RunArgsM &a, double *rb, int *rw, double *tabl, int *cons_word, int lane, bool act, int i, int &slot_off,
                                            RunNodeM &cur, RunNodeM &nxt, double &A0, double &A1, double (&ad)[4 * G], double &alpha_have, double &al,
                                            int *abort_word) {
  const double inf = __builtin_huge_val();
  if (__builtin_amdgcn_readlane(cur.sw, kRsTag) != i + 1) {   // (not there yet when it was asked for)
    const long long t0_ = (long long)wall_clock64();
    // (a real call's result arrives in a vector register: say that it is uniform, or the loop gets exec-mask exits)
    if (!__builtin_amdgcn_readfirstlane((int)run_wait((const int *)(rb + slot_off + kRunSc) + kRsTag, i + 1, abort_word, a.abort_flag, a.spin_ticks))) return false;
    run_request_m(rb + slot_off, lane, cur);
    if (a.stat && lane == 0) { atomicAdd(a.stat + 3 + 2 * (BACKWARD ? 1 : 0), 1ull); atomicAdd(a.stat + 4 + 2 * (BACKWARD ? 1 : 0), (unsigned long long)((long long)wall_clock64() - t0_)); }
  }
  const int sw = cur.sw;
  const int key = __builtin_amdgcn_readlane(sw, kRsKinds), nmsg = __builtin_amdgcn_readlane(sw, kRsNmsg), cut = __builtin_amdgcn_readlane(sw, kRsCut);
  double Di = cur.P;
  // the tail of the node's list from the first handed-over row on, in list order (the order of the reference's additions)
  // (the direction's common keys first, on a copy of the key that is opaque to the compiler: one chain of equality
  //  tests becomes a search tree, which put two dozen scalar instructions and seven branches in front of two additions.
  //  Forward, every chain node but two has 0x20098.  Backward it is the handed-over pair with the interior row behind it,
  //  0x30098, or in between, 0x30908, about half the chain each: ONE test for the two, the order by a select)
  int key_first = key;
  asm volatile("" : "+s"(key_first));
  const bool between = BACKWARD && key_first == 0x30908;
  if (BACKWARD) key_first ^= between ? 0x30908 ^ 0x30098 : 0;
  if (!BACKWARD && __builtin_expect(key_first == 0x20098, 1)) { Di += A0; Di += A1; }               // handed over, handed over
  else if (BACKWARD && __builtin_expect(key_first == 0x30098, 1)) { Di += A0; Di += between ? cur.S0 : A1; Di += between ? A1 : cur.S0; }
  else if (key == 0x20098) { Di += A0; Di += A1; }
  else if (key == 0x30908) { Di += A0; Di += cur.S0; Di += A1; }
  else if (key == 0x30098) { Di += A0; Di += A1; Di += cur.S0; }
  else if (key == 0x41908) { Di += A0; Di += cur.S0; Di += A1; Di += cur.S1; }
  else {
    const int nt = key >> 16;
    for (int t = 0; t < nt; ++t) {
      const int kd = (key >> (4 * t)) & 15;
      if (kd == 8) Di += A0; else if (kd == 9) Di += A1; else if (kd == 0) Di += cur.S0; else if (kd == 1) Di += cur.S1; else Di += cur.S2;
    }
  }
  if (BACKWARD) Di -= wave_min_dpp(act ? Di : inf);   // minimize.cpp:79-83 (the node's own lower-bound term)
  const double sd = cur.sd, mold0 = cur.M0, mold1 = cur.M1;
  const double gamma = readlane_f64(sd, 2);
  // this node's words and rows are in registers: its place in the ring is free (one store instruction without an
  // exec-mask region: lane 0 hits the word, the other lanes words of their own nobody reads), and the next node's are
  // asked for
  lds_store(cons_word, i + 1 - a.c0);
  slot_off += kRunSlotDoubles;
  if (slot_off == kRunSlots * kRunSlotDoubles) slot_off = 0;
  if (i + 1 < a.c1) run_request_m(rb + slot_off, lane, nxt);
  double R0 = 0, R1 = 0;
  for (int m = 0; m < nmsg; ++m) {
    const double alpha = readlane_f64(sd, m);
    const double h = gamma * Di - (m == 0 ? mold0 : mold1);   // (lanes beyond K: the loader staged -inf as their old message, so h = +inf)
    double out = 0;   // (alpha == 0: typeStereoLinear.h:390-396, a constant row, normalised)
    if (alpha != 0) {
      *tabl = h;
      if (__builtin_expect(alpha != alpha_have, 0)) {
        // (a real branch: as a select the refresh costs every message 4 G multiplies and 8 G conditional moves)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int d = 0; d < 4 * G; ++d) ad[d] = alpha * ((double)(d + 1) * a.step);
        al = alpha * a.lambda;
        alpha_have = alpha;
      }
      // the window's reads go out behind the write of h and IN FRONT of the reduction, whose two dozen instructions
      // then hide their latency (LDS serves one wave's requests in order: the reads need the write and nothing else)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      double lo[4 * G], hi[4 * G];
#pragma unroll
      for (int d = 0; d < 4 * G; ++d) { lo[d] = tabl[-(d + 1)]; hi[d] = tabl[d + 1]; }
      __builtin_amdgcn_sched_barrier(0);
      const double hmin = wave_min_dpp(h);
      __builtin_amdgcn_sched_barrier(0);   // (or the window's first additions, and the wait for its reads, move up into the reduction)
      const double vtrunc = hmin + al;
      double ma = h, mb = hi[0] + ad[0];   // (two chains; the truncation value joins last: a minimum is exact in any order)
#pragma unroll
      for (int d = 0; d < 4 * G; ++d) { ma = min_raw(ma, lo[d] + ad[d]); if (d > 0) mb = min_raw(mb, hi[d] + ad[d]); }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      out = min_raw(min_raw(ma, mb), vtrunc) - hmin;
    }
    if (m == 0) R0 = out; else R1 = out;
  }
  A0 = R0; A1 = nmsg == 2 ? R1 : R0;
  if (cut) {
    // the rows the segment behind this node starts from: to the publisher
    const int ps = cut & 1;
    if (__builtin_amdgcn_readfirstlane(lds_load(rw + kSwFree)) < cut - 2 &&
        !__builtin_amdgcn_readfirstlane((int)run_wait(rw + kSwFree, cut - 2, abort_word, a.abort_flag, a.spin_ticks))) return false;
    double *pb = rb + kRunPub + ps * 128;
    pb[lane] = A0; pb[64 + lane] = A1;
    if (lane == 0) lds_store(rw + kSwKinds + ps, __builtin_amdgcn_readlane(sw, kRsPubKinds));
    SPEC_RELEASE();
    if (lane == 0) lds_store(rw + kSwPubM + 4 * ps, cut);
  }
  return true;
}

template <bool BACKWARD, int G>
__device__ __forceinline__ void run_messages_g(const RunArgsM &a, double *rb, int lane, int *abort_word) {
  const bool act = lane < a.K;
  int *rw = (int *)(rb + kRunWords);
  double *tabl = rb + kRunTab + 16 + lane;   // this lane's entry of the H table
  int *cons_word = lane == 0 ? rw + kRwConsM : (int *)(rb + kRunDoubles) + lane;   // (kRunDummy words behind the runner's LDS)
  double ad[4 * G];   // alpha |d step| of the window's index distances, for the weight seen last
#pragma unroll
  for (int d = 0; d < 4 * G; ++d) ad[d] = 0;
  double alpha_have = 0;   // (never a weight that takes the window path)
  double al = 0;           // alpha lambda for that weight
  double A0 = 0, A1 = 0;
  RunNodeM na, nb;
  run_request_m(rb, lane, na);
  nb = na;
  int slot_off = 0;
  // (two visits per trip: the nodes' registers swap roles instead of being copied)
  for (int i = a.c0; i < a.c1; i += 2) {
    if (!run_visit_m<BACKWARD, G>(a, rb, rw, tabl, cons_word, lane, act, i, slot_off, na, nb, A0, A1, ad, alpha_have, al, abort_word)) return;
    if (i + 1 < a.c1 && !run_visit_m<BACKWARD, G>(a, rb, rw, tabl, cons_word, lane, act, i + 1, slot_off, nb, na, A0, A1, ad, alpha_have, al, abort_word)) return;
  }
}

template <bool BACKWARD>
__device__ __attribute__((noinline)) void run_messages(const DevParams *pp) {
  extern __shared__ __attribute__((aligned(16))) double run_lds[];
  constexpr int D = BACKWARD ? 1 : 0;
  RunArgsM a;
  a.K = uniform_value(pp->K); a.window = uniform_value(pp->window); a.c0 = uniform_value(pp->spec_c0[D]); a.c1 = uniform_value(pp->spec_c1[D]);
  a.lambda = uniform_value(pp->lambda); a.step = uniform_value(pp->uniform_step);
  a.abort_flag = uniform_value(pp->abort_flag); a.spin_ticks = uniform_value(pp->spin_ticks); a.stat = uniform_value(pp->spec_stat);
  double *lds0 = pinned_lds(run_lds);
  double *rb = lds0 + kRunBase;
  int *abort_word = (int *)lds0 + kRunAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  // the window in groups of four entries (entries beyond it cost >= vTrunc bit for bit, finish_inputs checks the spacing);
  // windows of more than eight entries keep the plain schedule (spec_active, trws_plan.hip)
  if (a.window <= 4) run_messages_g<BACKWARD, 1>(a, rb, lane, abort_word);
  else run_messages_g<BACKWARD, 2>(a, rb, lane, abort_word);
}

// ---- wave 1: the labels of the primal pass (minimize.cpp:223-264, as the primal wave of a visit computes them) ------
struct RunNodeP {
  int sw;
  double sd, TH, O0, O1, O2, O3;
};
__device__ __forceinline__ void run_request_p(const double *sl, int lane, RunNodeP &n) {
  n.sw = ((const int *)(sl + kRunSc))[lane & 15];
  asm volatile("" ::: "memory");
  n.sd = sl[kRunSc + 8 + (lane & 7)];
  n.TH = sl[kRunRowTH + lane];
  n.O0 = sl[kRunRowOUT + lane]; n.O1 = sl[kRunRowOUT + 64 + lane]; n.O2 = sl[kRunRowOUT + 128 + lane]; n.O3 = sl[kRunRowOUT + 192 + lane];
}
// What the labels need of the launch parameters, as uniform values.
struct RunArgsP {
  int c0, c1;
  double lambda;
  int32_t *abort_flag;
  long long spin_ticks;
};
// One visit of the labels' recurrence, built like run_visit_m: the node's words and rows were asked for during the visit
// before, the waits are calls whose result is declared uniform (inlined, their look at the abort flag in global memory
// makes every exit of the walk an exec-mask region), the word that frees the ring slot is stored by all lanes (lane 0
// hits the word, the others the words nobody reads) and the ring offset is carried, not divided out.
__device__ __forceinline__ bool run_visit_p(const RunArgsP &a, double *rb, int *rw, int *cons_word, int lane, bool act, double posk, int i, int &slot_off,
                                            RunNodeP &cur, RunNodeP &nxt, int &xprev, int *abort_word) {
  const double inf = __builtin_huge_val();
  if (RLI(cur.sw, kRsTag) != i + 1) {
    if (!__builtin_amdgcn_readfirstlane((int)run_wait((const int *)(rb + slot_off + kRunSc) + kRsTag, i + 1, abort_word, a.abort_flag, a.spin_ticks))) return false;
    run_request_p(rb + slot_off, lane, cur);
  }
  const int sw = cur.sw;
  const double sd = cur.sd;
  const int nout = RLI(sw, kRsNout), nin = RLI(sw, kRsNin), md = RLI(sw, kRsMd), cut = RLI(sw, kRsCut);
  double db = act ? cur.TH : 0.0;
  const double o0 = cur.O0, o1 = cur.O1, o2 = cur.O2, o3 = cur.O3;
  lds_store(cons_word, i + 1 - a.c0);
  slot_off += kRunSlotDoubles;
  if (slot_off == kRunSlots * kRunSlotDoubles) slot_off = 0;
  if (i + 1 < a.c1) run_request_p(rb + slot_off, lane, nxt);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < nin) {
      const int src = RLI(sw, kRsSrc + k);
      const int ks = src < 0 ? xprev : src;
      const double pks = readlane_f64(posk, ks);
      const double d = ((md >> k) & 1) == 0 ? pks - posk : posk - pks;
      db += readlane_f64(sd, 3 + k) * min_raw(fabs(d), a.lambda);
    }
  }
  double di = db;
  if (nout > 0) di += o0;
  if (nout > 1) di += o1;
  if (nout > 2) di += o2;
  if (nout > 3) di += o3;
  const double dim = act ? di : inf;
  const double vbest = wave_min_dpp(dim);
  xprev = __builtin_ctzll(__builtin_amdgcn_ballot_w64(dim == vbest));
  if (cut) {
    const int ps = cut & 1;
    if (__builtin_amdgcn_readfirstlane(lds_load(rw + kSwFree)) < cut - 2 &&
        !__builtin_amdgcn_readfirstlane((int)run_wait(rw + kSwFree, cut - 2, abort_word, a.abort_flag, a.spin_ticks))) return false;
    SPEC_ACQUIRE();
    if (lane == 0) { rw[kSwLabel + ps] = xprev; rw[kSwNode + ps] = RLI(sw, kRsNode); }
    SPEC_RELEASE();
    if (lane == 0) lds_store(rw + kSwPubP + ps, cut);
  }
  return true;
}
template <bool BACKWARD>
__device__ __attribute__((noinline)) void run_labels(const DevParams *pp) {
  extern __shared__ __attribute__((aligned(16))) double run_lds[];
  constexpr int D = BACKWARD ? 1 : 0;
  RunArgsP a;
  a.c0 = uniform_value(pp->spec_c0[D]); a.c1 = uniform_value(pp->spec_c1[D]); a.lambda = uniform_value(pp->lambda);
  a.abort_flag = uniform_value(pp->abort_flag); a.spin_ticks = uniform_value(pp->spin_ticks);
  const int K = uniform_value(pp->K);
  const double *pos = uniform_value(pp->pos);
  double *lds0 = pinned_lds(run_lds);
  double *rb = lds0 + kRunBase;
  int *abort_word = (int *)lds0 + kRunAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  const bool act = lane < K;
  int *rw = (int *)(rb + kRunWords);
  int *cons_word = lane == 0 ? rw + kSwConsP : (int *)(rb + kRunDoubles) + lane;   // (kRunDummy, as the message wave's)
  const double posk = act ? pos[lane] : 0.0;
  int xprev = 0;
  RunNodeP na, nb;
  run_request_p(rb, lane, na);
  nb = na;
  int slot_off = 0;
  // (two visits per trip: the nodes' registers swap roles instead of being copied)
  for (int i = a.c0; i < a.c1; i += 2) {
    if (!run_visit_p(a, rb, rw, cons_word, lane, act, posk, i, slot_off, na, nb, xprev, abort_word)) return;
    if (i + 1 < a.c1 && !run_visit_p(a, rb, rw, cons_word, lane, act, posk, i + 1, slot_off, nb, na, xprev, abort_word)) return;
  }
}

// ---- waves 2-9: staging ---------------------------------------------------------------------------------------------
// A loader works from the node's host-made record (trws_runner_records.h): which rows to load in front of and behind
// the foreign flags, where each goes in the ring slot, the staged words, gamma.  What is left to a turn is what depends
// on the sweep: the loads, the two waits, the twin verdict, the labels, the stores and the tag.

// r[s] for a uniform s: a tree of selects on the bits of s.  (The rows are eight named values, not an array: handed to
// a routine by reference the array went to scratch memory, every load waited for and stored there.)
__device__ __forceinline__ double run_pick4(int s, double r0, double r1, double r2, double r3) {
  const bool b0 = s & 1, b1 = s & 2;
  const double a0 = b0 ? r1 : r0, a1 = b0 ? r3 : r2;
  return b1 ? a1 : a0;
}
__device__ __forceinline__ double run_pick8(int s, double r0, double r1, double r2, double r3, double r4, double r5, double r6, double r7) {
  return (s & 4) ? run_pick4(s, r4, r5, r6, r7) : run_pick4(s, r0, r1, r2, r3);
}
template <bool BACKWARD, bool PRIMAL, bool UPDATE>
__device__ __attribute__((noinline)) void run_loader(const DevParams *pp_, int epoch_, int lw_) {
  extern __shared__ __attribute__((aligned(16))) double run_lds[];
  const DevParams p = uniform_params(pp_);
  double *lds0 = pinned_lds(run_lds);
  double *rb = lds0 + kRunBase;
  int *abort_word = (int *)lds0 + kRunAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  const int epoch = __builtin_amdgcn_readfirstlane(epoch_), lw = __builtin_amdgcn_readfirstlane(lw_);
  constexpr int D = BACKWARD ? 1 : 0;
  const int c0 = p.spec_c0[D], n = p.spec_c1[D] - c0;   // (positions count from the run's first: j = i - c0)
  const int32_t *rec = p.run_rec[D] + lane;
  const int K = p.K;
  const int lk = lane < K ? lane : K - 1;
  int *rw = (int *)(rb + kRunWords);
  const bool alane = (unsigned)(lane - kRecAlphaEdge) < 8u;   // the lanes that hold the edges of the node's weights
  static_assert(kRunLoaders <= kRunSlots, "run_loader: a loader's first node has a ring slot of its own");
  int slot_off = lw * kRunSlotDoubles;
  // (the record of this wave's NEXT node is asked for before the current one is worked on)
  int v2 = 0;
  if (lw < n) v2 = rec[(size_t)lw * kRecWords];
  for (int j = lw; j < n; j += kRunLoaders) {
    const int v = v2;
    if (j + kRunLoaders < n) v2 = rec[(size_t)(j + kRunLoaders) * kRecWords];
    const int nout = RLI(v, kRecNout), ndep = RLI(v, kRecNdep);
    // the node's own data (nobody writes it before the segment that holds the node walks it)
    const double theta = *(p.unary + (size_t)((unsigned long long)(unsigned)RLI(v, kRsNode) * (unsigned long long)(unsigned)K) + lk);
    double ad = p.alpha[alane ? v : 0];   // lane 16 + d: the weight that goes to double d of the staged node
    // (one uniform test per row that exists, then out)
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0;
#define RUN_ROW(k) (p.msg + (size_t)((unsigned long long)(unsigned)RLI(v, kRecEdge + k) * (unsigned long long)(unsigned)K) + lk)
    if (nout > 0) { r0 = *RUN_ROW(0);
    if (nout > 1) { r1 = *RUN_ROW(1);
    if (nout > 2) { r2 = *RUN_ROW(2);
    if (nout > 3) { r3 = *RUN_ROW(3);
    if (nout > 4) { r4 = *RUN_ROW(4);
    if (nout > 5) { r5 = *RUN_ROW(5);
    if (nout > 6) { r6 = *RUN_ROW(6);
    if (nout > 7) { r7 = *RUN_ROW(7); } } } } } } } }
    // foreign dependencies (everything but the node in front), then their rows and labels
    if (ndep > 0) wait_for_dependencies_w(p, ndep, __shfl(v, kRecDep + (lane & 3), kWave), RLI(v, kRecRank), epoch, lane, abort_word);
    if (lds_load(abort_word)) return;
    int word = v;   // lanes 0-14: the staged words; 9-12 take the labels found behind the flags, 2 the twin verdict
    const int fetch = RLI(v, kRecFetch);
    if (fetch) {
      const int labels = RLI(v, kRecLabels), lane0 = kRsSrc - nout;
#define RUN_FETCH(k) \
      if ((fetch >> k) & 1) { \
        if (UPDATE) r##k = ld_sc1(RUN_ROW(k)); \
        if (PRIMAL && ((labels >> k) & 1)) { const int xv = ld_sc1(p.x + RLI(v, kRecOther + k)); word = lane == lane0 + k ? xv : word; } \
      }
      RUN_FETCH(0) RUN_FETCH(1) RUN_FETCH(2) RUN_FETCH(3) RUN_FETCH(4) RUN_FETCH(5) RUN_FETCH(6) RUN_FETCH(7)
#undef RUN_FETCH
    }
#undef RUN_ROW
    // the ring slot: both recurrences have taken the node that had it into their registers
    double *sl = rb + slot_off;
    slot_off += kRunLoaders * kRunSlotDoubles;
    if (slot_off >= kRunSlots * kRunSlotDoubles) slot_off -= kRunSlots * kRunSlotDoubles;
    if (UPDATE && !run_wait_i<true>(rw + kRwConsM, j - kRunSlots + 1, abort_word, p.abort_flag, p.spin_ticks)) return;
    if (PRIMAL && !run_wait_i<true>(rw + kSwConsP, j - kRunSlots + 1, abort_word, p.abort_flag, p.spin_ticks)) return;
    int nmsg = RLI(v, kRsNmsg);
    if (UPDATE) {
      // P = ((theta + r0) + r1) + ... over exactly the first kfirst rows, in list order
      double P = theta;
      const int kfirst = RLI(v, kRecKfirst);
      if (kfirst > 0) { P += r0;
      if (kfirst > 1) { P += r1;
      if (kfirst > 2) { P += r2;
      if (kfirst > 3) { P += r3;
      if (kfirst > 4) { P += r4;
      if (kfirst > 5) { P += r5;
      if (kfirst > 6) { P += r6;
      if (kfirst > 7) { P += r7; } } } } } } } }
      sl[kRunRowP + lane] = P;
      const int st0 = RLI(v, kRecStage);
      if (st0 >= 0) {   // (staged rows are numbered in list order: no second without a first)
        sl[kRunRowS + lane] = run_pick8(st0, r0, r1, r2, r3, r4, r5, r6, r7);
        const int st1 = RLI(v, kRecStage + 1);
        if (st1 >= 0) {
          sl[kRunRowS + 64 + lane] = run_pick8(st1, r0, r1, r2, r3, r4, r5, r6, r7);
          const int st2 = RLI(v, kRecStage + 2);
          if (st2 >= 0) sl[kRunRowS + 128 + lane] = run_pick8(st2, r0, r1, r2, r3, r4, r5, r6, r7);
        }
      }
      // the old rows of the messages to the next node (lanes beyond K: -inf, which makes the recurrence's
      // H = gamma Di - m = +inf there without a select); the two are ONE message if weights and old rows agree
      // (positions are shared)
      const int m0k = RLI(v, kRecMsg), m1k = RLI(v, kRecMsg + 1), twin = RLI(v, kRecTwin);
      double m0 = 0, m1 = 0;
      if (m0k >= 0) { m0 = run_pick4(m0k, r0, r1, r2, r3); sl[kRunRowM + lane] = lane < K ? m0 : -__builtin_huge_val(); }
      if (m1k >= 0) { m1 = run_pick4(m1k, r0, r1, r2, r3); sl[kRunRowM + 64 + lane] = lane < K ? m1 : -__builtin_huge_val(); }
      if (twin) {
        bool same = RLI(__double2hiint(ad), kRecAlphaEdge) == RLI(__double2hiint(ad), kRecAlphaEdge + 1) &&
                    RLI(__double2loint(ad), kRecAlphaEdge) == RLI(__double2loint(ad), kRecAlphaEdge + 1);
        if (twin == 2) same = same && !UNI(lane < K && __double_as_longlong(m0) != __double_as_longlong(m1));
        nmsg = same ? 1 : 2;
      }
    }
    if (PRIMAL) {
      sl[kRunRowTH + lane] = theta;
      if (nout > 0) { sl[kRunRowOUT + lane] = r0;
      if (nout > 1) { sl[kRunRowOUT + 64 + lane] = r1;
      if (nout > 2) { sl[kRunRowOUT + 128 + lane] = r2;
      if (nout > 3) { sl[kRunRowOUT + 192 + lane] = r3; } } } }
    }
    word = lane == kRsNmsg ? nmsg : word;
    if (lane < kRsTag) ((int *)(sl + kRunSc))[lane] = word;
    // doubles 8-15: alpha of the two messages, gamma (MRFEnergy.cpp:207-228; its bits come with the record), alpha of
    // the incoming rows
    const double g = __hiloint2double(RLI(v, kRecGamma + 1), RLI(v, kRecGamma));
    ad = lane == kRecAlphaEdge + 2 ? g : ad;
    if (alane) sl[kRunSc + 8 - kRecAlphaEdge + lane] = ad;
    SPEC_RELEASE();
    if (lane == 0) lds_store((int *)(sl + kRunSc) + kRsTag, c0 + j + 1);
  }
}

// the narrow runner's layout and roles for chain_runner: wave 0 messages, wave 1 labels, waves 2-9 loaders, wave 10
// publisher (wave 11 idle)
struct PipeRunner {
  static constexpr int C = 1, kBase = kRunBase, kAbortInt = kRunAbortInt, kSlots = kRunSlots, kSlotDoubles = kRunSlotDoubles,
                       kSc = kRunSc, kTab = kRunTab, kTabs = 1, kPub = kRunPub, kWords = kRunWords, kMsgWaves = 1, kLoaders = kRunLoaders;
  static constexpr bool kOverlay = false;
  static __device__ __forceinline__ void prepare(const DevParams &, double *, int) {}
  template <bool BACKWARD>
  static __device__ __forceinline__ void messages(const DevParams *pp, int) { run_messages<BACKWARD>(pp); }
  template <bool BACKWARD>
  static __device__ __forceinline__ void labels(const DevParams *pp) { run_labels<BACKWARD>(pp); }
  template <bool BACKWARD, bool PRIMAL, bool UPDATE>
  static __device__ __forceinline__ void loader(const DevParams *pp, int epoch, int lw) { run_loader<BACKWARD, PRIMAL, UPDATE>(pp, epoch, lw); }
};

#undef RLI

}  // namespace
}  // namespace stereo
