// QPBO max-flow: what the device code and the host driver share -- the graph as the kernel sees it, the control
// words, agent-scope loads and stores, the workgroup vote and the grid barrier.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace stereo {

constexpr int kQB = 256;

struct QpboDev {
  int n;             // doubled node count
  int m;             // arcs
  const int32_t *aptr, *head, *rev;  // arcs grouped by tail; rev[a] = reverse arc
  double *r, *delta, *ex, *snk;
  int32_t *h, *h2;
  // Improve launch only (else nullptr): the exact heights at the moment the current node was fixed
  int32_t *keep;
  int32_t *counters;  // [0] active nodes, [1] frontier size (next), [2] changed flag
  // tiling for the block-local relabelling: tile T owns positions [T * 1024, (T + 1) * 1024);
  // perm[pos] = node or -1, pos_of[node] = pos.  A tile holds nodes that are close in the graph
  // (a 16 x 32 pixel patch and its mates when the grid shape is known).
  const int32_t *perm, *pos_of;
  int ntiles;
  // graphs with at most four arcs per node: what a tile needs to know about its arcs, by tile position, so that
  // a tile is loaded in two dependent round trips (this table | the state it points to) instead of four
  // (node -> arc range -> heads -> their positions).  13 words per position, one array per word:
  // [0] first arc | degree << 28, [1 + k] head of arc k, [5 + k] slot of the head in this tile | index of the
  // reverse arc among the head's arcs << 10, or -1 - (the head's tile), [9 + k] reverse arc.  Filled at the
  // start of a launch (the heads depend on the move), kept for the Improve launch of the same move.
  int32_t *tab;
  unsigned long long *hx;   // tiled rounds: hx_pack word per node (nullptr: no tiled rounds)
  // tiled rounds: dirty[parity][tile] == number of the round = the tile holds excess that can still move, or
  // flow was pushed into it across its border in the round before; other tiles are skipped.  (Round numbers
  // instead of flags that are cleared: every workgroup reads ALL marks of a round to find its share of the
  // marked tiles, see `collect`, so nothing may change them while the round runs.)
  int32_t *dirty;
  // the same idea for the label-correcting relabelling: rdirty[parity][tile] = a height next to
  // the tile (or inside it) went down in the last step
  int32_t *rdirty;
};

// What the host decides about a launch's schedule (QpboOptions and the graph), by value to the kernel
struct QpboSchedule {
  int relabel_every;    // rounds between two exact relabellings at most (the interval doubles up to it) ...
  int first_interval;   // ... starting here
  int stall_permille;   // progress, in thousandths of the active nodes per round, below which a round counts as stagnant
  int max_rounds;
  int tiled;            // local rounds of a tiled round; 0: plain rounds only
  int switch_at;        // plain rounds before the tiled ones, at most
  int wrap_at;          // tiled rounds after which the round numbers start again from 0
  bool adaptive;        // leave the plain rounds early when the excess drains slowly (the slow-tail test)
  bool final_relabel;   // (development) always run the final relabelling
};

constexpr int kMB = 1024;
// ctl words: [0] barrier counter, [1] abort, [2..4] "changed" slots, [5..7] active-count slots,
// [8] rounds done, [9] global relabels done
struct QpboCtl { enum { kBar = 0, kAbort = 1, kChanged = 2, kActive = 5, kRounds = 8, kRelabels = 9, kNext = 16, kWords = 20 }; };   // [16..18]: result words of the Improve search, used in turn
constexpr int kGridSpinLimit = 1 << 24;
constexpr int kImproveBlocks = 64;    // workgroups of an Improve launch (see QpboSolver::maxflow)
// -DSTEREO_HIP_QPBO_PROFILE: workgroup 0 adds up where its time goes (10 ns ticks and event counts in
// counters[1200 ..], printed with STEREO_HIP_QPBO_VERBOSE): relabelling = init pass | tile set-up | tile
// relaxation | grid barriers; tiled rounds = tile load | local rounds | store | grid barriers
#ifdef STEREO_HIP_QPBO_PROFILE
#define QPROF_T(var) const long long var = wall_clock64()
#define QPROF_ADD(slot, val) do { if (blockIdx.x == 0 && threadIdx.x == 0 && g.counters) g.counters[1200 + (slot)] += (int)(val); } while (0)
#else
#define QPROF_T(var) do {} while (0)
#define QPROF_ADD(slot, val) do {} while (0)
#endif
__device__ __forceinline__ int ldc(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stc(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ldc(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stc(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// One word per node for the tiled rounds: height | height at the last grid barrier << 24 | round of the store << 48.
// A tile reads its outside neighbours' heights AS OF THE BARRIER (only then does exactly the higher endpoint of an
// arc pair push), but tiles are stored while others are still being loaded -- a workgroup's second tile of a round
// starts when its neighbours' first tiles are done.  The owner stores all three in one word, the reader takes the
// old height if the word was written in the running round: the same result whatever the timing.
__device__ __forceinline__ unsigned long long hx_pack(int cur, int prev, int round) {
  return (unsigned long long)(unsigned)cur | ((unsigned long long)(unsigned)prev << 24) | ((unsigned long long)(round & 0xffff) << 48);
}
__device__ __forceinline__ int hx_at_barrier(unsigned long long w, int round) {
  const int cur = (int)(w & 0xffffffu), prev = (int)((w >> 24) & 0xffffffu);
  return (int)(w >> 48) == (round & 0xffff) ? prev : cur;
}
__device__ __forceinline__ double ldc(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stc(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// "Did any thread of the workgroup say yes" on the barrier the caller needs anyway: a wave with a yes stores a
// flag, one s_barrier, everybody reads it.  Three flags in turn -- the next one is cleared while this one is in
// use (its last readers passed the previous call's barrier) -- instead of __syncthreads_or's workgroup reduction,
// which costs several times the relaxation step it guards (0.93 us per step measured, 16 waves).
// Called by all threads; s_any[0..2] zero before the first call.
__device__ __forceinline__ bool wg_any(bool pred, int *s_any, int &slot) {
  if (__builtin_amdgcn_ballot_w64(pred) != 0 && (threadIdx.x & 63) == 0) s_any[slot] = 1;
  const int nxt = slot == 2 ? 0 : slot + 1;
  if (threadIdx.x == 0) s_any[nxt] = 0;
  __syncthreads();
  const bool r = s_any[slot] != 0;
  slot = nxt;
  return r;
}

__device__ __forceinline__ bool grid_sync(int32_t *ctl, unsigned &gen) {
  __syncthreads();
  if (threadIdx.x == 0) {
    ++gen;
    __hip_atomic_fetch_add(ctl + QpboCtl::kBar, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int target = (int)(gen * gridDim.x);
    int spins = 0;
    while (__hip_atomic_load(ctl + QpboCtl::kBar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kGridSpinLimit) {  // bounded: never hang the device
        __hip_atomic_store(ctl + QpboCtl::kAbort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
  __syncthreads();
  return __hip_atomic_load(ctl + QpboCtl::kAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}

}  // namespace stereo
