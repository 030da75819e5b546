// QPBO roof-duality binary fusion on MI355X (gfx950): the max-flow kernel and its host driver (C ABI: qpbo_plan.hip).
//
// Replaces the reference's rd_mex gateway + QPBO v1.3 library for this path
// (cpp/rd_mex.cpp:14-100; cpp/QPBO-v1.3.src/QPBO.cpp:408-507 AddPairwiseTerm,
// QPBO.h:760-807 ComputeWeights, QPBO.cpp:786-816 + QPBO_extra.cpp:137-239
// MergeParallelEdges, QPBO.cpp:818-845 Solve, QPBO_maxflow.cpp:477-617 maxflow,
// QPBO_postprocessing.cpp:10-120 ComputeWeakPersistencies, QPBO_extra.cpp:1151-1233
// Improve, QPBO.cpp:847-917 energy / lower bound).
//
// Construction: every neighbour pair's directed 2x2 tables are
// summed (the reversed ones transposed), normal-formed once, and laid out as the
// doubled graph: node v < N is x_v, node v + N its mate.  A submodular pair (i,j)
// gives arcs i->j, j->i and the mirror j'->i', i'->j'; a supermodular pair gives
// i->j', j'->i and j->i', i'->j.  Arc a and its reverse are a, a^1.
//
// Max-flow: deterministic synchronous push-relabel.  Every iteration is
//   K1 push      (thread per node, old heights; a pair of arcs is only ever
//                 modified by the one endpoint whose height is larger)
//   K2 gather    (each node adds the flow pushed into it in its own arc order,
//                 then relabels from the post-push residual graph)
// with periodic global relabelling (frontier BFS from the sink).  Nothing depends
// on scheduling or atomics' arrival order, so results are bitwise reproducible.
// Strong persistency only needs T = {v : v reaches the sink in the residual
// graph}: x_i = 1 iff i in T, x_i = 0 iff mate(i) in T (QPBO.cpp:840-844); T is
// the same for every maximum flow/preflow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "common.h"
#include "qpbo_dev.h"
#include "qpbo_solver.h"

namespace stereo {
namespace {

// ---- the whole max-flow in ONE launch -------------------------------------------------------
// A loop of launches is launch bound (round 1 measured ~800 launches of a few microseconds of
// work each for a Teddy move).  This kernel runs synchronous rounds -- push | barrier |
// gather + relabel | barrier -- and the level-synchronous global relabelling between grid-wide
// barriers: one workgroup of 1024 threads per CU, all resident (cooperative launch), nodes
// in a grid-stride loop.  Everything one workgroup writes and another reads inside the launch
// (heights, residuals, pushed amounts) goes through agent-scope (sc1) accesses -- the XCDs' L2s are
// not coherent for plain accesses inside a launch -- so the barrier itself needs no cache
// write-back / invalidate: __syncthreads drains the stores, one atomic counter does the rest.
// Same arithmetic in the same per-node order as the kernels above, so results are reproducible.
// improve_perm != nullptr: the launch is the whole loop of QPBO::Improve (QPBO_extra.cpp:1190-1200) --
// find the next node of the permutation that is not strongly labelled, fix it to 0 with the
// reference's INFTY term, maximise the flow again from the current heights, until the permutation
// is exhausted -- instead of one launch and three host round trips per fixed node (round 2: 100-250
// re-solves of ~0.3 ms each on the hard globalstereo moves).  improve_N = number of variables.
// (qpbo_maxflow_kernel, below its two helpers)

// The INFTY of QPBO::Improve's AddUnaryTerm(i, 0, INFTY): max(-t_i + sum of outgoing residuals, t_i + sum of incoming) + 1
// evaluated on node i with terminal capacity t_i = tcap (QPBO_extra.cpp:241-254, :1177-1187), same summation order as
// the reference
__device__ __forceinline__ double improve_infty(const QpboDev &g, int i, double tcap) {
  double c1 = -tcap, c2 = tcap;
  for (int a = g.aptr[i]; a < g.aptr[i + 1]; ++a) { c1 += ldc(g.r + a); c2 += ldc(g.r + g.rev[a]); }
  return (c1 > c2 ? c1 : c2) + 1;
}

// When the next exact relabelling is due, for the plain and the tiled rounds alike.  Excess that cannot reach the
// sink any more only climbs one level per round; an exact relabelling retires it at once.  Early relabels are cheap
// (few BFS levels) and usually end the solve after a handful of rounds, so the interval starts small and doubles.
struct RelabelClock {
  int since_relabel, interval, stagnant, last_active;
  __device__ __forceinline__ void start(const QpboSchedule &sch, int active) {
    since_relabel = 0; stagnant = 0; last_active = active;
    interval = sch.relabel_every < sch.first_interval ? sch.relabel_every : sch.first_interval;
  }
  // after every round: relabel now?
  __device__ __forceinline__ bool tick(const QpboSchedule &sch, int active) {
    ++since_relabel;
    stagnant = (long long)active * 1000 >= (long long)last_active * (1000 - sch.stall_permille) ? stagnant + 1 : 0;  // no progress: what is left is probably cut off
    last_active = active;
    return active > 0 && (since_relabel >= interval || (stagnant >= 2 && since_relabel >= 4));
  }
  __device__ __forceinline__ void relabelled(const QpboSchedule &sch, int active) {
    since_relabel = 0; stagnant = 0; last_active = active;
    interval = interval * 2 < sch.relabel_every ? interval * 2 : sch.relabel_every;
  }
};

__global__ __launch_bounds__(kMB) void qpbo_maxflow_kernel(QpboDev g, int32_t *ctl, QpboSchedule sch, const int32_t *improve_perm,
                                                            int improve_N) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];  // tile state of the tiled rounds
  __shared__ int s_red;
  __shared__ int s_h[kMB + 1];   // [kMB]: n, the height an arc without residual capacity leads to
  __shared__ int s_h2[kMB];      // tiled rounds: the heights being written while s_h is read, and the other way round
  __shared__ int s_any[3];
  int any_slot = 0;
  if (threadIdx.x < 3) s_any[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_h[kMB] = g.n;
  __syncthreads();
  // The marked tiles of a round / relabelling step, dealt out evenly: every workgroup reads all marks, ranks the
  // marked tiles (ballot + wave counts, the same list everywhere, no atomics) and takes ranks b, b + #workgroups, ...
  // With the fixed tile -> workgroup map a step lasted as long as the workgroup that happened to own two or three
  // marked tiles (some 190 of 658 are marked in a round of the hard globalstereo moves: 73 us per round against
  // ~35 for one tile); results do not depend on who processes a tile.
  constexpr int kMaxMine = 64;
  __shared__ int s_mine[kMaxMine];
  __shared__ int s_wcnt[kMB / 64];
  const bool dealt = g.ntiles <= kMaxMine * (int)gridDim.x;
  auto collect = [&](const int32_t *marks, int tag) -> int {
    if (!dealt) return (g.ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // candidates of the fixed map
    int total = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < g.ntiles; base += kMB) {
      const int T = base + threadIdx.x;
      const bool f = T < g.ntiles && ldc(marks + T) == tag;
      const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
      if (lane == 0) s_wcnt[wave] = __builtin_popcountll(b);
      __syncthreads();
      int before = total, chunk = 0;
#pragma unroll
      for (int w = 0; w < kMB / 64; ++w) {
        const int c = s_wcnt[w];
        before += w < wave ? c : 0;
        chunk += c;
      }
      if (f) {
        const int rank = before + __builtin_popcountll(b & ((1ull << lane) - 1ull));
        if (rank % (int)gridDim.x == (int)blockIdx.x) s_mine[rank / (int)gridDim.x] = T;
      }
      total += chunk;
      __syncthreads();
    }
    return total > (int)blockIdx.x ? (total - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  };
  int RG = 0;   // relabelling steps so far in this launch: the marks of step RG are rdirty[RG & 1][tile] == RG
  unsigned gen = 0;
  const int n = g.n;
  const int first = blockIdx.x * kMB + threadIdx.x, stride = gridDim.x * kMB;
  int32_t *h = g.h, *h2 = g.h2;
  // rotating flag slots, one ring per flag family: written in phase k of that family, read after its
  // barrier, cleared one phase (of the same family) later
  int slotA = 0, slotC = 0;
  auto ld = [&](int w) { return __hip_atomic_load(ctl + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  auto clear_next = [&](int base, int slot) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_store(ctl + base + (slot + 1) % 3, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  int G = 0;   // tiled rounds of this launch so far (marks, pushed-amount buffers and hx words are numbered by it)
  bool hx_refresh_all = false;
  const bool tabbed = g.tab != nullptr && sch.tiled > 0;
  const size_t tabn = (size_t)g.ntiles * kMB;
  if (tabbed && improve_perm == nullptr) {
    for (int T = blockIdx.x; T < g.ntiles; T += gridDim.x) {
      const size_t p = (size_t)T * kMB + threadIdx.x;
      const int v = g.perm[p];
      int a0 = 0, deg = 0;
      if (v >= 0) { a0 = g.aptr[v]; deg = g.aptr[v + 1] - a0; }
      int w4[4], rv4[4], pw4[4], aw4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = k < deg ? a0 + k : 0;
        const int w = g.head[a], rv = g.rev[a];
        w4[k] = k < deg ? w : 0; rv4[k] = k < deg ? rv : 0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) { pw4[k] = g.pos_of[w4[k]]; aw4[k] = g.aptr[w4[k]]; }
      g.tab[p] = a0 | (deg << 28);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g.tab[(1 + k) * tabn + p] = w4[k];
        g.tab[(5 + k) * tabn + p] = pw4[k] / kMB == T ? ((pw4[k] % kMB) | ((rv4[k] - aw4[k]) << 10)) : -1 - pw4[k] / kMB;
        g.tab[(9 + k) * tabn + p] = rv4[k];
      }
    }
    // (plain stores, read by whichever workgroup is dealt the tile: written back before the barrier, and the
    // relabelling every solve starts with invalidates before anybody reads)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (!grid_sync(ctl, gen)) return;
  }
  // Exact distances to the sink in the residual graph, then #active nodes.  Label correcting
  // instead of one grid barrier per BFS level: every workgroup relaxes h[v] = min(h[v], h[w] + 1)
  // over the residual arcs of its tile (heights in LDS, arc status in registers) until nothing
  // changes inside the tile, then the tiles exchange their boundary heights at a grid barrier;
  // done when no tile changed.  The fixpoint is the BFS distance whatever the schedule, so the
  // result is deterministic, and a front crosses a whole tile per barrier instead of one level.
  int relabels_done = 0;
  int incremental = 0;   // the solve is one of an Improve step: its first relabelling starts from the heights that are there
  [[maybe_unused]] int improve_steps_dbg = 0;   // (STEREO_HIP_QPBO_CHECK_CONFINED)
  int fixed_node = 0;        // the node the current Improve step fixed
  bool keep_valid = false;   // g.keep holds the exact heights of the flow the current Improve step started from
  auto global_relabel = [&](int &active) -> bool {
    constexpr int kArcRegs = 8;
    const long long t_in = wall_clock64();
    const unsigned gen_in = gen;
    // (`warm`: the heights are the exact distances of a flow that was maximal before a unary term
    // changed -- Improve.  Kept as the starting point of the label correction they stay a valid
    // labelling (every residual arc still sees at most one level down once the relaxation has
    // converged, sink arcs are re-seeded), which is all the push phase needs; far fewer passes.)
    const bool warm = incremental != 0 && relabels_done == 0;
    // (`confined`: a later relabelling of the same Improve step.  Fixing node i hands excess to i alone,
    // and i had no path to the sink (keep_valid is only set then): the excess moves only through nodes that had none either, so no
    // residual arc changes on the old shortest path of a node that had one -- its distance can only have
    // gone down (a shorter way through i's mate).  The snapshot of the exact heights at the moment of
    // the fix is therefore an upper bound of the distances for those nodes, n for all others, and the
    // label correction started from ANY upper bound ends in the same fixpoint, the BFS distances: the
    // same heights as the search from scratch, but the front only crosses the region the fix touched.)
    const bool confined = !warm && keep_valid;
    // (`local`: inside such a step only the tiles the step has touched are looked at.  The step's first, warm
    // relabelling lowers the nodes that can reach the new sink arc at i's mate -- the tiles where that happened are
    // recorded in `touched` --, and from then on distances only grow (pushes along admissible arcs never shorten a
    // path), for nodes of that set alone: every other node keeps the height it has.  So the first pass relaxes the
    // tiles whose input changed instead of all of them; the dirty marks carry the rest as before.)
    const bool local = keep_valid && (warm || confined);
    int32_t *touched = g.keep ? g.keep + n : nullptr;
    int32_t *rd_first = g.rdirty + (size_t)((RG + 1) & 1) * g.ntiles;   // marks of the first step
    ++relabels_done;
    QPROF_T(qp0);
    auto start_height = [&](int v, double snk_v, int cur_h, int keep_h) {
      const int old_h = warm ? cur_h : (confined ? keep_h : n);
      const int new_h = snk_v > 0 ? 1 : (old_h < n ? old_h : n);
      stc(h + v, new_h);
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
      // development check: outside the touched tiles a confined relabelling starts from the heights that are there
      if (local && confined && g.counters && new_h != cur_h && !ldc(touched + g.pos_of[v] / kMB)) atomicAdd(g.counters + 1107, 1);
#endif
      if (local && warm && new_h < cur_h) {   // a new sink arc: this node's tile and the tiles of its neighbours
        const int T = g.pos_of[v] / kMB;
        stc(touched + T, 1); stc(rd_first + T, RG + 1);
        for (int a = g.aptr[v]; a < g.aptr[v + 1]; ++a) stc(rd_first + g.pos_of[g.head[a]] / kMB, RG + 1);
      }
    };
    constexpr bool kLocalPasses = true;
    if (local && kLocalPasses) {
      // Only what the step can have changed: its first relabelling starts from heights that are exact but for the
      // new sink arc at the fixed node's mate (and the fixed node itself); a later one resets the touched tiles,
      // every other node has the height it started the step with (the check build verifies exactly that).
      if (warm) {
        if (blockIdx.x == 0 && threadIdx.x < 2) {
          const int v = fixed_node + (threadIdx.x ? improve_N : 0);
          start_height(v, ldc(g.snk + v), ldc(h + v), n);
        }
      } else {
        for (int T = blockIdx.x; T < g.ntiles; T += gridDim.x) {
          if (!ldc(touched + T)) continue;
          const int v = g.perm[T * kMB + threadIdx.x];
          if (v >= 0) start_height(v, ldc(g.snk + v), ldc(h + v), ldc(g.keep + v));
        }
      }
    } else {
      // (four nodes per thread requested together: the loads are agent-scope and would otherwise go one by one)
      for (int v0 = first; v0 < n; v0 += 4 * stride) {
        double sk4[4];
        int ch4[4], kh4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int v = v0 + u * stride < n ? v0 + u * stride : v0;
          sk4[u] = ldc(g.snk + v);
          ch4[u] = (warm || local) ? ldc(h + v) : n;
          kh4[u] = confined ? ldc(g.keep + v) : n;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (v0 + u * stride < n) start_height(v0 + u * stride, sk4[u], ch4[u], kh4[u]);
      }
    }
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
    // development check: the local pass left every node where the pass over all nodes would have put it
    if (local && kLocalPasses && g.counters) {
      __syncthreads();
      for (int v = first; v < n; v += stride) {
        const int cur_h = ldc(h + v);
        const int old_h = warm ? cur_h : ldc(g.keep + v);
        const int want = ldc(g.snk + v) > 0 ? 1 : (old_h < n ? old_h : n);
        const bool mine_to_write = warm ? (v == fixed_node || v == fixed_node + improve_N) : ldc(touched + g.pos_of[v] / kMB) != 0;
        if (!mine_to_write && want != cur_h && atomicAdd(g.counters + 1108, 1) == 0) {
          g.counters[1110] = v; g.counters[1111] = cur_h; g.counters[1112] = want; g.counters[1113] = warm ? 1 : 0;
        }
      }
    }
#endif
    // A tile is relaxed again only if a height next to it went down in the last step (every tile in
    // the first): once a tile has reached its fixpoint it stays there until an input changes.  The
    // search front crosses the image, the warm search of an Improve step touches a small region.
    if (!local) {
      for (int T = first; T < g.ntiles; T += stride) stc(rd_first + T, RG + 1);
    } else if (confined) {
      for (int T = first; T < g.ntiles; T += stride)
        if (ldc(touched + T)) stc(rd_first + T, RG + 1);
    }
    // (everything another workgroup may have written inside the launch -- heights, residuals, excess, sink
    // capacities -- is read with agent-scope loads; an acquire fence here, i.e. an invalidate of the whole L2 per
    // relabelling, cost more than those loads: STEREO_HIP_QPBO_PROFILE, `init`)
    QPROF_T(qp1);
    QPROF_ADD(0, qp1 - qp0);
    if (!grid_sync(ctl, gen)) return false;
    QPROF_ADD(3, wall_clock64() - qp1);
    for (;;) {
      slotC = (slotC + 1) % 3;
      clear_next(QpboCtl::kChanged, slotC);
      bool any_changed = false;
      ++RG;
      int32_t *rd_in = g.rdirty + (size_t)(RG & 1) * g.ntiles, *rd_out = g.rdirty + (size_t)((RG + 1) & 1) * g.ntiles;
      const int mine = collect(rd_in, RG);
      for (int j = 0; j < mine; ++j) {
        int T;
        if (dealt) T = s_mine[j];
        else {
          T = blockIdx.x + j * gridDim.x;
          if (ldc(rd_in + T) != RG) continue;
        }
        QPROF_T(qp2);
        const int v = g.perm[T * kMB + threadIdx.x];
        int my = n, a0 = 0, a1 = 0;
        int lidx[kArcRegs];  // residual arc to a node of this tile: its slot in s_h; every other arc: the slot that holds n
        int extT[kArcRegs];  // tile of the arc's head if it is another tile (whatever the residual), else -1
        int ext_best = n;    // what the residual arcs that leave the tile allow (their heads do not move during this step)
        if (tabbed) {
          // the arc table of the tile position, then the state it points to: two dependent round trips
          const size_t p = (size_t)T * kMB + threadIdx.x;
          const int ta = g.tab[p];
          int tw[4], tl[4], hwk[4];
          double rk[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) { tw[k] = g.tab[(1 + k) * tabn + p]; tl[k] = g.tab[(5 + k) * tabn + p]; }
          a0 = ta & 0x0fffffff; a1 = a0 + (int)((unsigned)ta >> 28);
          my = v >= 0 ? ldc(h + v) : n;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            hwk[k] = ldc(h + tw[k]);
            rk[k] = ldc(g.r + (a0 + k < a1 ? a0 + k : 0));
          }
#pragma unroll
          for (int k = 0; k < kArcRegs; ++k) { lidx[k] = kMB; extT[k] = -1; }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (a0 + k < a1) {
              const bool inside = tl[k] >= 0;
              if (!inside) extT[k] = -1 - tl[k];
              if (rk[k] > 0) {
                if (inside) lidx[k] = tl[k] & (kMB - 1);
                else ext_best = hwk[k] + 1 < ext_best ? hwk[k] + 1 : ext_best;
              }
            }
          }
          s_h[threadIdx.x] = my;
        } else {
          if (v >= 0) {
            my = ldc(h + v);
            a0 = g.aptr[v]; a1 = g.aptr[v + 1];
          }
          s_h[threadIdx.x] = my;
          // heads, then everything that hangs on them, requested together: three dependent round trips per tile
          int wk[kArcRegs], pwk[kArcRegs], hwk[kArcRegs];
          double rk[kArcRegs];
          const int nk = sch.tiled > 0 ? 4 : kArcRegs;   // (tiled rounds: at most four arcs per node)
#pragma unroll
          for (int k = 0; k < kArcRegs; ++k) wk[k] = (k < nk && a0 + k < a1) ? g.head[a0 + k] : 0;
#pragma unroll
          for (int k = 0; k < kArcRegs; ++k) {
            pwk[k] = 0; hwk[k] = n; rk[k] = 0.0;
            if (k < nk) {
              pwk[k] = g.pos_of[wk[k]];
              hwk[k] = ldc(h + wk[k]);
              rk[k] = a0 + k < a1 ? ldc(g.r + a0 + k) : 0.0;
            }
          }
#pragma unroll
          for (int k = 0; k < kArcRegs; ++k) {
            lidx[k] = kMB; extT[k] = -1;
            if (a0 + k < a1) {
              const bool inside = pwk[k] / kMB == T;
              if (!inside) extT[k] = pwk[k] / kMB;
              if (rk[k] > 0) {
                if (inside) lidx[k] = pwk[k] % kMB;
                else ext_best = hwk[k] + 1 < ext_best ? hwk[k] + 1 : ext_best;
              }
            }
          }
        }
        __syncthreads();
        QPROF_T(qp3);
        QPROF_ADD(1, qp3 - qp2); QPROF_ADD(4, 1);
        const int start = my;
        bool ch;
        if (sch.tiled > 0) {
          // (tiled rounds are only switched on for graphs with at most four arcs per node: the 4-connected grid)
          do {
            QPROF_ADD(5, 1);
            int best = ext_best < my ? ext_best : my;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int hw = s_h[lidx[k]] + 1;
              best = hw < best ? hw : best;
            }
            ch = best < my;
            if (ch) { my = best; s_h[threadIdx.x] = my; }  // heights only decrease: racing readers are harmless
          } while (wg_any(ch, s_any, any_slot));
        } else {
          do {
            QPROF_ADD(5, 1);
            int best = ext_best < my ? ext_best : my;
#pragma unroll
            for (int k = 0; k < kArcRegs; ++k) {
              const int hw = s_h[lidx[k]] + 1;
              best = hw < best ? hw : best;
            }
            for (int a = a0 + kArcRegs; a < a1; ++a) {  // nodes of higher degree: the rest from memory
              if (!(ldc(g.r + a) > 0)) continue;
              const int w = g.head[a], pw = g.pos_of[w];
              const int hw = pw / kMB == T ? s_h[pw % kMB] : ldc(h + w);
              best = hw + 1 < best ? hw + 1 : best;
            }
            ch = best < my;
            if (ch) { my = best; s_h[threadIdx.x] = my; }
          } while (wg_any(ch, s_any, any_slot));
        }
        if (my < start) {
          stc(h + v, my); any_changed = true;
          if (local) stc(touched + T, 1);
          // whoever has a residual arc INTO v may come down now: the tiles of v's neighbours
#pragma unroll
          for (int k = 0; k < kArcRegs; ++k)
            if (extT[k] >= 0) stc(rd_out + extT[k], RG + 1);
          for (int a = a0 + kArcRegs; a < a1; ++a) {
            const int tw = g.pos_of[g.head[a]] / kMB;
            if (tw != T) stc(rd_out + tw, RG + 1);
          }
        }
        __syncthreads();
        QPROF_ADD(2, wall_clock64() - qp3);
      }
      if (wg_any(any_changed, s_any, any_slot) && threadIdx.x == 0)
        __hip_atomic_store(ctl + QpboCtl::kChanged + slotC, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      QPROF_T(qp4);
      if (!grid_sync(ctl, gen)) return false;
      QPROF_ADD(3, wall_clock64() - qp4); QPROF_ADD(6, 1);
      if (!ld(QpboCtl::kChanged + slotC)) break;
    }
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
    // development check: exact distances are tight (a node below n without a sink arc has a residual arc one
    // level down); a start that was NOT an upper bound leaves nodes that hang in the air
    if ((confined || local) && g.counters) {
      for (int v = first; v < n; v += stride) {
        const int hv = ldc(h + v);
        if (hv >= n || ldc(g.snk + v) > 0) continue;
        bool sup = false;
        for (int a = g.aptr[v]; a < g.aptr[v + 1]; ++a) sup = sup || (ldc(g.r + a) > 0 && ldc(h + g.head[a]) == hv - 1);
        if (!sup && atomicAdd(g.counters + 1100, 1) == 0) {
          g.counters[1101] = v; g.counters[1102] = hv; g.counters[1103] = ldc(g.keep + v);
          g.counters[1104] = ldc(g.ex + v) > 0; g.counters[1105] = relabels_done; g.counters[1106] = improve_steps_dbg;
        }
      }
    }
#endif
    slotA = (slotA + 1) % 3;
    clear_next(QpboCtl::kActive, slotA);
    int cnt = 0;
    if (local && kLocalPasses) {
      // (a node that can move excess inside such a step was lowered by the step: it lies in a touched tile)
      for (int T = blockIdx.x; T < g.ntiles; T += gridDim.x) {
        if (!ldc(touched + T)) continue;
        const int v = g.perm[T * kMB + threadIdx.x];
        if (v >= 0) {
          const int hh = ldc(h + v);
          cnt += (ldc(g.ex + v) > 0 && hh < n) ? 1 : 0;
          if (g.hx) stc(g.hx + v, hx_pack(hh, hh, 0));   // (the heights the next tiled round reads)
        }
      }
      if (hx_refresh_all && g.hx)
        for (int v = first; v < n; v += stride) { const int hh = ldc(h + v); stc(g.hx + v, hx_pack(hh, hh, 0)); }
    } else {
      for (int v0 = first; v0 < n; v0 += 4 * stride) {
        double e4[4];
        int h4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int v = v0 + u * stride < n ? v0 + u * stride : v0;
          e4[u] = ldc(g.ex + v); h4[u] = ldc(h + v);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) cnt += (v0 + u * stride < n && e4[u] > 0 && h4[u] < n) ? 1 : 0;
        if (g.hx) {   // (the heights the next tiled round reads)
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (v0 + u * stride < n) stc(g.hx + v0 + u * stride, hx_pack(h4[u], h4[u], 0));
        }
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
#pragma unroll
        for (int u = 0; u < 4; ++u)   // development check: inside a local step excess only moves in touched tiles
          if (local && g.counters && v0 + u * stride < n && e4[u] > 0 && h4[u] < n && !ldc(touched + g.pos_of[v0 + u * stride] / kMB))
            atomicAdd(g.counters + 1107, 1);
#endif
      }
    }
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
    if (local && kLocalPasses && g.counters)   // development check: nothing that can move excess outside the touched tiles
      for (int v = first; v < n; v += stride)
        if (ldc(g.ex + v) > 0 && ldc(h + v) < n && !ldc(touched + g.pos_of[v] / kMB)) atomicAdd(g.counters + 1109, 1);
#endif
    hx_refresh_all = false;
    cnt = wg_any(cnt > 0, s_any, any_slot) ? cnt : 0;
    if (threadIdx.x == 0) s_red = 0;
    __syncthreads();
    if (cnt) atomicAdd(&s_red, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_red)
      __hip_atomic_fetch_add(ctl + QpboCtl::kActive + slotA, s_red, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!grid_sync(ctl, gen)) return false;
    active = ld(QpboCtl::kActive + slotA);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // statistics: #relabels, their barriers and time (10 ns ticks)
      ctl[QpboCtl::kRelabels] += 1;
      ctl[11] += (int)(wall_clock64() - t_in);
      ctl[12] += (int)(gen - gen_in);
    }
    return true;
  };

  int improve_from = 0, improve_steps = 0;
  bool heights_copied = false;   // the solve that just ended wrote g.h after its last grid barrier
  bool solve = improve_perm == nullptr;   // the Improve launch starts from a maximal flow: first find a node to fix
  for (;;) {
    if (solve) {
      int active = 0;
      relabels_done = 0;
      if (!global_relabel(active)) return;
      int rounds = 0;
      RelabelClock clock;
      clock.start(sch, active);

      // When to leave the plain rounds for the tiled ones: at round `switch_at` at the latest, and earlier if
      // the excess left over by an exact relabelling drains slowly -- two rounds after the relabelling more
      // than 70 % of it is still there (real NCC fusion moves: 1748 -> 1463, a long tail the tiled rounds
      // cut short; noisy synthetic terms: 322 -> 65, done within a dozen plain rounds).
      int after_relabel = -1;
      bool slow_tail = false;
      while (active > 0 && rounds < sch.max_rounds && (sch.tiled <= 0 || (rounds < sch.switch_at && !slow_tail))) {
        // ---- push (old heights; a pair of arcs is only modified by the endpoint that is higher)
        for (int v = first; v < n; v += stride) {
          double e = ldc(g.ex + v);
          const int hv = ldc(h + v);
          if (!(e > 0) || hv >= n) continue;
          if (hv == 1) {
            const double sk = ldc(g.snk + v);
            if (sk > 0) {
              const double d = e < sk ? e : sk;
              stc(g.snk + v, sk - d);   // (written through: the local passes of an Improve step read it from another workgroup)
              e -= d;
            }
          }
          const int a0 = g.aptr[v], a1 = g.aptr[v + 1];
          // the first eight arcs: residuals, heads, reverse arcs and head heights are requested together
          // (three dependent round trips instead of three per arc); decisions stay in arc order
          constexpr int kB = 8;
          double rb[kB];
          int hb[kB], wb[kB], bb[kB];
#pragma unroll
          for (int k = 0; k < kB; ++k) {
            const int a = a0 + k < a1 ? a0 + k : a0;
            rb[k] = a0 + k < a1 ? ldc(g.r + a) : 0.0;
            wb[k] = g.head[a]; bb[k] = g.rev[a];
          }
#pragma unroll
          for (int k = 0; k < kB; ++k) hb[k] = (a0 + k < a1 && rb[k] > 0) ? ldc(h + wb[k]) : n;
#pragma unroll
          for (int k = 0; k < kB; ++k) {
            if (a0 + k < a1 && e > 0 && rb[k] > 0 && hv == hb[k] + 1) {
              const double d = e < rb[k] ? e : rb[k];
              stc(g.r + a0 + k, rb[k] - d);
              stc(g.r + bb[k], ldc(g.r + bb[k]) + d);
              stc(g.delta + a0 + k, d);
              e -= d;
            }
          }
          for (int a = a0 + kB; a < a1 && e > 0; ++a) {
            const double ra = ldc(g.r + a);
            if (ra > 0 && hv == ldc(h + g.head[a]) + 1) {
              const double d = e < ra ? e : ra;
              const int b = g.rev[a];
              stc(g.r + a, ra - d);
              stc(g.r + b, ldc(g.r + b) + d);
              stc(g.delta + a, d);
              e -= d;
            }
          }
          stc(g.ex + v, e);
        }
        if (!grid_sync(ctl, gen)) return;
        // ---- gather the pushed flow in the node's own arc order, relabel from the post-push residual graph
        slotA = (slotA + 1) % 3;
        clear_next(QpboCtl::kActive, slotA);
        int cnt = 0;
        for (int v = first; v < n; v += stride) {
          double e = ldc(g.ex + v);
          const int a0 = g.aptr[v], a1 = g.aptr[v + 1];
          constexpr int kB = 8;
          int bb[kB];
          double db[kB];
#pragma unroll
          for (int k = 0; k < kB; ++k) bb[k] = g.rev[a0 + k < a1 ? a0 + k : a0];
#pragma unroll
          for (int k = 0; k < kB; ++k) db[k] = a0 + k < a1 ? ldc(g.delta + bb[k]) : 0.0;
#pragma unroll
          for (int k = 0; k < kB; ++k)
            if (db[k] != 0) { e += db[k]; stc(g.delta + bb[k], 0.0); }
          for (int a = a0 + kB; a < a1; ++a) {
            const int b = g.rev[a];
            const double d = ldc(g.delta + b);
            if (d != 0) { e += d; stc(g.delta + b, 0.0); }
          }
          stc(g.ex + v, e);
          int hv = ldc(h + v);
          if (e > 0 && hv < n) {
            int hmin = n;
            if (ldc(g.snk + v) > 0) hmin = 0;
            double rb[kB];
            int hw8[kB];
#pragma unroll
            for (int k = 0; k < kB; ++k) rb[k] = a0 + k < a1 ? ldc(g.r + a0 + k) : 0.0;
#pragma unroll
            for (int k = 0; k < kB; ++k) hw8[k] = rb[k] > 0 ? ldc(h + g.head[a0 + k]) : n;
#pragma unroll
            for (int k = 0; k < kB; ++k) hmin = hw8[k] < hmin ? hw8[k] : hmin;
            for (int a = a0 + kB; a < a1; ++a)
              if (ldc(g.r + a) > 0) {
                const int hw = ldc(h + g.head[a]);
                hmin = hw < hmin ? hw : hmin;
              }
            if (hmin + 1 > hv) hv = hmin + 1 < n ? hmin + 1 : n;
            if (hv < n) ++cnt;
          }
          stc(h2 + v, hv);
        }
        if (threadIdx.x == 0) s_red = 0;
        __syncthreads();
        if (cnt) atomicAdd(&s_red, cnt);
        __syncthreads();
        if (threadIdx.x == 0 && s_red)
          __hip_atomic_fetch_add(ctl + QpboCtl::kActive + slotA, s_red, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!grid_sync(ctl, gen)) return;
        active = ld(QpboCtl::kActive + slotA);
        if (g.counters && blockIdx.x == 0 && threadIdx.x == 0 && rounds < 1024) g.counters[16 + rounds] = active;
        { int32_t *t = h; h = h2; h2 = t; }
        ++rounds;
        const bool relabel_now = clock.tick(sch, active);
        if (sch.adaptive && after_relabel > 0 && clock.since_relabel == 2 && (long long)active * 10 > (long long)after_relabel * 7) slow_tail = true;
        if (relabel_now) {
          if (!global_relabel(active)) return;
          clock.relabelled(sch, active);
          after_relabel = active;
        }
      }
      // ---- tiled rounds (every node has at most four arcs: the 4-connected grid) ------------------
      // One round per grid barrier moves excess one hop; on instances with strong smoothness the flow
      // has to travel hundreds of pixels.  Here a workgroup takes its tile (a 16 x 32 pixel patch and
      // its mates: excess, heights, sink capacities and the residuals of the tile's own arcs) into
      // LDS and runs up to `tiled` synchronous push / gather + relabel rounds there between two grid
      // barriers.  Arcs that leave the tile are pushed on in the first local round only, when both
      // endpoints see the heights of the last barrier (so still only the higher endpoint of an arc pair
      // pushes); the amount goes into delta[parity][arc] and the owner of the reverse arc takes it in
      // at the start of its next round.  Same per-node arithmetic order in every run: deterministic.
      bool exact = false;
      if (sch.tiled > 0 && active > 0 && rounds < sch.max_rounds) {
        const long long t_tiled = wall_clock64();
        const int rounds_in = rounds;
        // hand-over from the plain rounds: heights into g.h, excess and sink capacities written through
        // (from here on the workgroup that owns a node's tile reads and writes them)
        for (int v = first; v < n; v += stride) {
          const int hh = ldc(h + v);
          if (h != g.h) stc(g.h + v, hh);
          if (g.hx) stc(g.hx + v, hx_pack(hh, hh, 0));
          stc(g.ex + v, ldc(g.ex + v)); stc(g.snk + v, ldc(g.snk + v));
        }
        h = g.h; h2 = g.h2;
        // (G, the round number: pushes of round G land in delta buffer G & 1)
        // Few tiles hold excess after the plain rounds (7k active nodes in some dozens of 660 tiles on
        // the long globalstereo moves): a tile without excess that can move and without flow arriving
        // over its border does not change in a round, so it is skipped -- exactly, not heuristically.
        // After an exact relabelling every tile is looked at once (nodes may have become active again).
        auto mark_all_dirty = [&]() {
          // (hx words carry 16 bits of the round number: long before they wrap, start again from 0 and have the
          // relabelling that follows every call rewrite all words as "not stored in any round"; nothing is in transit here)
          // The dirty marks are raw round numbers too: at the wrap both planes are cleared (by the thread that
          // then writes the tile's new mark, so the two stores are ordered), or marks left from the launch's
          // first rounds 2, 3, ... would compare equal to the restarted round numbers.
          // STEREO_HIP_QPBO_WRAP_AT=<n> (1 .. 4095, development): wrap that early, so that a test reaches the wrap at all
          // (tests/test_rd_gpu.py::test_round_numbers_wrap).
          const bool wrap = G > sch.wrap_at;
          if (wrap) { G = 0; hx_refresh_all = true; }
          for (int T = first; T < g.ntiles; T += stride) {
            if (wrap) { stc(g.dirty + T, 0); stc(g.dirty + (size_t)g.ntiles + T, 0); }
            stc(g.dirty + (size_t)((G + 1) & 1) * g.ntiles + T, G + 1);
          }
        };
        mark_all_dirty();
        if (!grid_sync(ctl, gen)) return;
        double *s_d = dyn_lds;   // [thread][arc]: what a neighbour inside the tile pushed over the reverse of that arc
        // L local rounds (L == 0: only take in what was pushed across tile borders); counts the active
        // nodes and one more per workgroup that pushed across a border (that flow is still in transit)
        auto tile_round = [&](int L) -> bool {
          ++G;
          double *dout = g.delta + (size_t)(G & 1) * g.m, *din = g.delta + (size_t)((G + 1) & 1) * g.m;
          int32_t *dirty_in = g.dirty + (size_t)(G & 1) * g.ntiles, *dirty_out = g.dirty + (size_t)((G + 1) & 1) * g.ntiles;
          slotA = (slotA + 1) % 3;
          clear_next(QpboCtl::kActive, slotA);
          int cnt = 0;
          bool crossed = false;
          const int mine = collect(dirty_in, G);
          for (int j = 0; j < mine; ++j) {
            int T;
            if (dealt) T = s_mine[j];
            else {
              T = blockIdx.x + j * gridDim.x;
              if (ldc(dirty_in + T) != G) continue;
            }
            QPROF_T(qt0);
            const int v = g.perm[T * kMB + threadIdx.x];
            const bool valid = v >= 0;
            int loc[4] = {-1, -1, -1, -1}, rvk[4] = {0, 0, 0, 0}, exth[4] = {n, n, n, n}, extT[4] = {0, 0, 0, 0}, a0 = 0, deg = 0;
            double e = 0;
            int hv = n;
            double sk = 0, rk[4] = {0, 0, 0, 0}, e0_in = 0;
            {
              // the arc table of the tile position, then the state it points to: two dependent round trips
              // (tiled rounds are for graphs with at most four arcs per node, and those always have the table)
              const size_t p = (size_t)T * kMB + threadIdx.x;
              const int ta = g.tab[p];
              int tw[4], tl[4], rvs[4], hwk[4];
              double din_k[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                tw[k] = g.tab[(1 + k) * tabn + p]; tl[k] = g.tab[(5 + k) * tabn + p]; rvs[k] = g.tab[(9 + k) * tabn + p];
              }
              a0 = ta & 0x0fffffff; deg = (int)((unsigned)ta >> 28);
              const int vv = valid ? v : 0;
              e = ldc(g.ex + vv); hv = ldc(h + vv); sk = ldc(g.snk + vv);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                rk[k] = ldc(g.r + (k < deg ? a0 + k : 0));
                hwk[k] = hx_at_barrier(ldc(g.hx + tw[k]), G); din_k[k] = ldc(din + rvs[k]);
              }
              if (!valid) { e = 0; hv = n; sk = 0; }
              e0_in = e;
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                if (k < deg) {
                  if (tl[k] >= 0) { loc[k] = tl[k] & (kMB - 1); rvk[k] = tl[k] >> 10; din_k[k] = 0; }
                  else { exth[k] = hwk[k]; extT[k] = -1 - tl[k]; }
                } else {
                  rk[k] = 0; din_k[k] = 0;
                }
              }
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                if (k < deg && din_k[k] != 0) {  // flow that arrived over this arc's reverse during the last round
                  e += din_k[k]; rk[k] += din_k[k];
                  stc(din + rvs[k], 0.0);
                }
              }
            }
            // A node's excess, sink capacity and residuals are only ever changed by its own thread: they stay in
            // registers for the local rounds.  LDS holds what neighbours read (heights, two buffers in turn: a round
            // writes the new ones where nobody is reading) and what they write (the amounts pushed over a local arc).
#pragma unroll
            for (int k = 0; k < 4; ++k) s_d[threadIdx.x * 4 + k] = 0;
            int *hcur = s_h, *hnext = s_h2;
            hcur[threadIdx.x] = hv;
            const int h0 = hv;  // height at the barrier
            // what this thread has to write back: bit 0 excess, bit 1 sink capacity, bits 2 .. 5 the residuals
            // (most nodes of a tile do not move in a round; a store that is written through costs what a load does)
            int wrote = (e0_in != e) ? 0x3d : 0;   // flow taken in over the border: excess and residuals changed
            __syncthreads();
            QPROF_T(qt1);
            QPROF_ADD(8, qt1 - qt0); QPROF_ADD(12, 1);
            for (int l = 0; l < L; ++l) {
              QPROF_ADD(13, 1);
              // the neighbours' heights of this round, requested together (the buffer being read does not change
              // before the round's last barrier: the push and the relabel below see the same values)
              int hw4[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) hw4[k] = hcur[loc[k] >= 0 ? loc[k] : threadIdx.x];
#pragma unroll
              for (int k = 0; k < 4; ++k) hw4[k] = loc[k] >= 0 ? hw4[k] : exth[k];
              // push (a pair of arcs is only modified by the endpoint that is higher)
              if (valid && e > 0 && hv < n) {
                if (hv == 1 && sk > 0) {
                  const double d = e < sk ? e : sk;
                  sk -= d;
                  e -= d;
                  wrote |= 3;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  if (k < deg && e > 0 && rk[k] > 0) {
                    const bool local = loc[k] >= 0;
                    const int hw = hw4[k];
                    if ((local || l == 0) && hv == hw + 1) {
                      const double d = e < rk[k] ? e : rk[k];
                      rk[k] -= d;
                      wrote |= 1 | (4 << k);
                      if (local) s_d[loc[k] * 4 + rvk[k]] = d;
                      else { stc(dout + a0 + k, d); stc(dirty_out + extT[k], G + 1); crossed = true; }
                      e -= d;
                    }
                  }
                }
              }
              __syncthreads();
              // gather in the node's own arc order, relabel from the post-push residual graph
              int newh = hv;
              if (valid) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  if (k < deg) {
                    const double d = s_d[threadIdx.x * 4 + k];
                    if (d != 0) { e += d; rk[k] += d; s_d[threadIdx.x * 4 + k] = 0; wrote |= 1 | (4 << k); }
                  }
                }
                if (e > 0 && hv < n) {
                  int hmin = sk > 0 ? 0 : n;
#pragma unroll
                  for (int k = 0; k < 4; ++k) {
                    // outside heights are lower bounds.  An outside neighbour that stood exactly one above
                    // this node at the barrier may have pushed to it in this round; the residual that gives
                    // this node's arc arrives with the next round, so the arc counts as open until then.
                    if (k < deg && (rk[k] > 0 || (loc[k] < 0 && exth[k] == h0 + 1)))
                      hmin = hw4[k] < hmin ? hw4[k] : hmin;
                  }
                  if (hmin + 1 > hv) newh = hmin + 1 < n ? hmin + 1 : n;
                }
              }
              hnext[threadIdx.x] = newh;   // (the other buffer: the old heights are still being read)
              hv = newh;
              { int *t = hcur; hcur = hnext; hnext = t; }
              if (!wg_any(valid && e > 0 && hv < n, s_any, any_slot)) break;
            }
            QPROF_T(qt2);
            QPROF_ADD(9, qt2 - qt1);
            if (valid) {
              if (wrote & 1) stc(g.ex + v, e);   // (written through: read by other workgroups)
              if (wrote & 2) stc(g.snk + v, sk);
              if (hv != h0) {   // (an unchanged height leaves a word whose current-height field is right whatever its round)
                stc(h + v, hv);
                stc(g.hx + v, hx_pack(hv, h0, G));
              }
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (k < deg && (wrote & (4 << k))) stc(g.r + a0 + k, rk[k]);
              if (e > 0 && hv < n) ++cnt;
            }
            // (also the barrier before the tile buffers are reused)
            const int left = wg_any(valid && e > 0 && hv < n, s_any, any_slot);
            if (left && threadIdx.x == 0) stc(dirty_out + T, G + 1);
            QPROF_ADD(10, wall_clock64() - qt2);
          }
          QPROF_T(qt3);
          if (threadIdx.x == 0) s_red = 0;
          __syncthreads();
          if (cnt) atomicAdd(&s_red, cnt);
          if (crossed) atomicOr(&s_red, 1 << 30);
          __syncthreads();
          if (threadIdx.x == 0 && s_red)
            __hip_atomic_fetch_add(ctl + QpboCtl::kActive + slotA, (s_red & ((1 << 30) - 1)) + (s_red >> 30), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
          if (!grid_sync(ctl, gen)) return false;
          QPROF_ADD(11, wall_clock64() - qt3); QPROF_ADD(14, 1);
          active = ld(QpboCtl::kActive + slotA);
          return true;
        };
        do {
          while (active > 0 && rounds < sch.max_rounds) {
            if (!tile_round(sch.tiled)) return;
            if (blockIdx.x == 0 && threadIdx.x == 0 && g.counters && rounds < 1024) g.counters[16 + rounds] = active;
            ++rounds;
            if (clock.tick(sch, active)) {
              if (!tile_round(0)) return;  // nothing in transit while the residual graph is searched
              mark_all_dirty();
              if (!global_relabel(active)) return;
              clock.relabelled(sch, active);
            }
          }
          mark_all_dirty();
          if (!global_relabel(active)) return;  // exact heights: anything left over is cut off
        } while (active > 0 && rounds < sch.max_rounds);
        exact = true;
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl[13] += (int)(wall_clock64() - t_tiled); ctl[14] += rounds - rounds_in; }
      }

      // heights may be stale lower bounds: one exact BFS defines T; leave it in g.h
      // (unless nothing has been pushed since the last relabelling and that one was exact -- from scratch, confined, or
      //  the warm one of an Improve step whose fixed node was cut off from the sink, where the old heights are upper
      //  bounds: most Improve steps find nothing to push after their warm relabelling, and this second one was three of
      //  their seven grid barriers)
      if (!exact && clock.since_relabel == 0 && (relabels_done > 1 || incremental == 0 || keep_valid) && !sch.final_relabel) exact = true;
      if (!exact && !global_relabel(active)) return;
      heights_copied = h != g.h;
      if (h != g.h) {
        for (int v = first; v < n; v += stride) stc(g.h + v, ldc(h + v));
      }
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl[QpboCtl::kRounds] += rounds;
        if (rounds >= sch.max_rounds && active > 0) ctl[QpboCtl::kAbort] = 2;
      }
      h = g.h; h2 = g.h2;
    }  // solve
    if (!improve_perm) break;
    // ---- Improve: the next node of the permutation whose two sides are both / neither connected to the
    // sink (not strongly labelled).  Heights in g.h are exact and written through.
    //
    // A step is TRIVIAL if its node i is cut off from the sink (height n, and so is its mate's) and no residual arc
    // leads into the mate: fixing i hands i excess that cannot move and gives the mate a sink arc that lowers nobody
    // but the mate itself (height 1) -- no node becomes active, the flow stays maximal; the step's warm relabelling
    // would find exactly that in three grid barriers.  Such a step changes the terminal capacities of i and its mate
    // and the mate's height, nothing else: it does not change which other entries of the permutation are ambiguous,
    // nor whether their steps are trivial (heights of other variables, residuals), nor the INFTY of another node
    // (its own terminals and arcs).  So all trivial steps in front of the first non-trivial ambiguous entry commute
    // with each other and are applied TOGETHER, each by the thread that owns the entry, behind the one barrier of the
    // search -- which now looks for the first NON-TRIVIAL ambiguous entry.  (99 % of the Improve steps of the Teddy
    // pair's example_global moves are trivial: 2045 of 2071 in the longest one, 114 ms of grid barriers before.)
    {
      // (excess and sink capacities are written through wherever they are stored: nothing to write back
      // before another workgroup's thread rewrites a node's terminal capacities below)
      const int N = improve_N;
      // (three result words in turn: the one of the NEXT step is cleared before this step's barrier -- its last readers
      //  passed the barrier of the step before)
      int32_t *word = ctl + QpboCtl::kNext + improve_steps % 3, *other = ctl + QpboCtl::kNext + (improve_steps + 1) % 3;
      if (improve_steps == 0 && blockIdx.x == 0 && threadIdx.x == 0) { stc(word, N); stc(other, N); }   // both start at "none"
      // (every workgroup's final heights and terminal capacities are in memory: a solve ends with the grid barriers of
      // its last relabelling, so the barrier is only needed if heights were copied after them -- and in the first step,
      // between the initialisation of the result words and their use)
      if (improve_steps == 0 || heights_copied) {
        if (!grid_sync(ctl, gen)) return;
      }
      heights_copied = false;
      if (improve_steps > 0 && blockIdx.x == 0 && threadIdx.x == 0) stc(other, N);
      if (g.keep) {   // the starting point of this step's later relabellings (global_relabel, `confined`)
        for (int v = first; v < n; v += stride) stc(g.keep + v, ldc(g.h + v));
        for (int T = first; T < g.ntiles; T += stride) stc(g.keep + n + T, 0);   // `touched`, global_relabel
      }
      // AddUnaryTerm(i, 0, INFTY)
      auto fix_to_zero = [&](int i, bool trivial_step) {
        const int im = i + N;
        const double exi = ldc(g.ex + i), ski = ldc(g.snk + i), exm = ldc(g.ex + im), skm = ldc(g.snk + im);
        const double INFTY = improve_infty(g, i, exi - ski);
        const double t0 = exi - ski + INFTY, t1 = exm - skm - INFTY;
        stc(g.ex + i, t0 > 0 ? t0 : 0.0); stc(g.snk + i, t0 < 0 ? -t0 : 0.0);
        stc(g.ex + im, t1 > 0 ? t1 : 0.0); stc(g.snk + im, t1 < 0 ? -t1 : 0.0);
        if (trivial_step) {   // what the step's relabelling would leave behind (t1 < 0: the mate has a sink arc now)
          stc(g.h + i, n); stc(g.h + im, 1);
          if (g.hx) { stc(g.hx + i, hx_pack(n, n, 0)); stc(g.hx + im, hx_pack(1, 1, 0)); }
          if (g.keep) { stc(g.keep + i, n); stc(g.keep + im, 1); }
        }
      };
      auto is_trivial = [&](int i) -> bool {   // (i ambiguous) cut off from the sink, no residual arc into the mate
        if (sch.final_relabel || !g.keep || ldc(g.h + i) < n) return false;
        const int im = i + N;
        bool t = true;
        for (int a = g.aptr[im]; a < g.aptr[im + 1]; ++a) t = t && !(ldc(g.r + g.rev[a]) > 0);
        if (!t) return false;
        // ... and the mate really ends up with a sink arc (t1 < 0 in fix_to_zero, which a trivial step's h[mate] = 1 relies
        // on): the doubled graph's symmetry says so -- excess stuck at an ambiguous node's mate is rounding residue --, but
        // that is an argument; this is the check (the same INFTY)
        const double INFTY = improve_infty(g, i, ldc(g.ex + i) - ldc(g.snk + i));
        return ldc(g.ex + im) - ldc(g.snk + im) - INFTY < 0;
      };
      int mine = N;
      for (int j = improve_from + first; j < N; j += stride) {
        const int i = improve_perm[j];
        if ((ldc(g.h + i) < n) != (ldc(g.h + i + N) < n)) continue;
        if (!is_trivial(i)) { mine = j; break; }   // (ascending j: the first one is this thread's smallest)
      }
      if (threadIdx.x == 0) s_red = N;
      __syncthreads();
      if (mine < N) atomicMin(&s_red, mine);
      __syncthreads();
      if (threadIdx.x == 0 && s_red < N) __hip_atomic_fetch_min(word, s_red, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!grid_sync(ctl, gen)) return;
      const int next = ldc(word);
      // the trivial steps in front of it, all at once
      {
        int done = 0;
        for (int j = improve_from + first; j < (next < N ? next : N); j += stride) {
          const int i = improve_perm[j];
          if ((ldc(g.h + i) < n) != (ldc(g.h + i + N) < n)) continue;
          fix_to_zero(i, true);
          ++done;
        }
        if (done && g.counters) atomicAdd(g.counters + 1302, done);   // (statistics)
      }
      if (next >= N) break;
      // (the argument for `confined` needs the node that receives the excess to be cut off from the sink: "neither
      // side connected".  The other ambiguous case, both sides connected, sends the new excess through nodes that
      // do have a path and lengthens distances there: those steps relabel from scratch.)
      fixed_node = improve_perm[next];
      keep_valid = g.keep != nullptr && ldc(g.keep + fixed_node) >= n;
      if (blockIdx.x == 0 && threadIdx.x == 0 && g.counters) g.counters[keep_valid ? 1300 : 1301] += 1;   // (statistics: steps of either kind)
      if (blockIdx.x == 0 && threadIdx.x == 0) fix_to_zero(fixed_node, false);
      improve_from = next + 1;
      ++improve_steps;
      improve_steps_dbg = improve_steps;
      incremental = 1;   // the heights stay a valid labelling when a unary term changes: warm search
      solve = true;
      // the new terminal capacities -- of the fixed node and its mate, and of the trivial steps in front of it, whose
      // mates' heights other workgroups wrote as well: everybody meets them behind a grid barrier
      if (!grid_sync(ctl, gen)) return;
    }
  }  // for (;;)
}

}  // namespace

// ------------------------------------------------------------------ solver

void QpboSolver::bind(int64_t N, const std::vector<int32_t> &aptr) {
  n = (int)(2 * N); m = (int)aptr.back();
  d_aptr.upload(aptr.data(), aptr.size());
  max_degree = 0;
  for (int v = 0; v < n; ++v) max_degree = std::max(max_degree, (int)(aptr[v + 1] - aptr[v]));
  d_head.alloc(m); d_rev.alloc(m); d_r.alloc(m); d_delta.alloc((size_t)2 * std::max(m, 1));
  d_ex.alloc(n); d_snk.alloc(n); d_h.alloc(n); d_h2.alloc(n); d_cnt.alloc(2048);
  g.n = n; g.m = m; g.aptr = d_aptr.p; g.head = d_head.p; g.rev = d_rev.p; g.r = d_r.p;
  g.delta = d_delta.p; g.ex = d_ex.p; g.snk = d_snk.p; g.h = d_h.p; g.h2 = d_h2.p; g.counters = d_cnt.p;
  set_tiling(N, 0, 0);
}

void QpboSolver::upload() {
  bind(P.N, P.aptr);
  d_head.upload(P.head.data(), P.head.size());
  d_rev.upload(P.rev.data(), P.rev.size());
  d_r.upload(P.cap.data(), P.cap.size());
  STEREO_HIP_CHECK(hipMemset(d_delta.p, 0, sizeof(double) * 2 * std::max(m, 1)));
  std::vector<double> ex(n), snk(n);
  for (int v = 0; v < n; ++v) {  // QPBO_maxflow.cpp:135-150: tr_cap > 0 source arc, < 0 sink arc
    ex[v] = P.tr[v] > 0 ? P.tr[v] : 0.0;
    snk[v] = P.tr[v] < 0 ? -P.tr[v] : 0.0;
  }
  snk0 = snk;
  d_ex.upload(ex.data(), n); d_snk.upload(snk.data(), n);
  STEREO_HIP_CHECK(hipMemset(d_cnt.p, 0, sizeof(int32_t) * 2048));
  STEREO_HIP_CHECK(hipDeviceSynchronize());
}

void QpboSolver::set_tiling(int64_t Nn, int H, int W) {
  const int half = kMB / 2;
  std::vector<int32_t> perm, posof(2 * Nn, -1);
  if (H > 0 && W > 0 && (int64_t)H * W == Nn) {
    const int tw = 16, th = half / tw, tc = (W + tw - 1) / tw, tr = (H + th - 1) / th;
    perm.assign((size_t)tc * tr * kMB, -1);
    for (int64_t v = 0; v < Nn; ++v) {
      const int col = (int)(v / H), row = (int)(v % H);
      const int64_t T = (int64_t)(col / tw) * tr + row / th;
      const int sl = (col % tw) * th + row % th;
      perm[T * kMB + sl] = (int32_t)v; perm[T * kMB + half + sl] = (int32_t)(v + Nn);
    }
  } else {
    const int64_t nt = (Nn + half - 1) / half;
    perm.assign((size_t)nt * kMB, -1);
    for (int64_t v = 0; v < Nn; ++v) {
      perm[(v / half) * kMB + v % half] = (int32_t)v;
      perm[(v / half) * kMB + half + v % half] = (int32_t)(v + Nn);
    }
  }
  for (size_t q = 0; q < perm.size(); ++q)
    if (perm[q] >= 0) posof[perm[q]] = (int32_t)q;
  d_perm.upload(perm.data(), perm.size()); d_posof.upload(posof.data(), posof.size());
  g.perm = d_perm.p; g.pos_of = d_posof.p; g.ntiles = (int)(perm.size() / kMB);
  d_dirty.alloc((size_t)4 * std::max(g.ntiles, 1));
  STEREO_HIP_CHECK(hipMemset(d_dirty.p, 0, sizeof(int32_t) * 4 * std::max(g.ntiles, 1)));
  g.dirty = d_dirty.p; g.rdirty = d_dirty.p + (size_t)2 * std::max(g.ntiles, 1);
  // graphs with at most four arcs per node: the tiled rounds' height words (heights fit their 24-bit fields) and
  // the arc table by tile position (QpboDev::tab)
  g.hx = nullptr;
  if (max_degree <= 4 && 2 * Nn < (1 << 24)) {
    d_hx.alloc((size_t)2 * Nn);
    g.hx = d_hx.p;
  }
  g.tab = nullptr;
  if (max_degree <= 4) {
    d_tab.alloc((size_t)13 * perm.size());
    g.tab = d_tab.p;
  }
}

void QpboSolver::improve(const QpboOptions &opt, const std::vector<int32_t> &perm, std::vector<int32_t> &h) {
  // one cooperative launch walks the whole permutation (qpbo_maxflow_kernel, improve_perm)
  // (kept across calls: hipMalloc / hipFree per Improve call cost more than the upload)
  if (d_iperm.n < perm.size()) d_iperm.alloc(perm.size());
  STEREO_HIP_CHECK(hipMemcpy(d_iperm.p, perm.data(), sizeof(int32_t) * perm.size(), hipMemcpyHostToDevice));
  // the relabellings inside an Improve step start from the heights of the flow the step began with
  // (qpbo_maxflow_kernel, `confined`)
  if (opt.confined) {
    if (d_keep.n < (size_t)n + (size_t)std::max(g.ntiles, 1)) d_keep.alloc((size_t)n + (size_t)std::max(g.ntiles, 1));   // heights + one mark per tile
    g.keep = d_keep.p;
  }
  try {
    maxflow(opt, d_iperm.p);
  } catch (...) {
    g.keep = nullptr;
    throw;
  }
  g.keep = nullptr;
  h.resize(n);
  STEREO_HIP_CHECK(hipMemcpy(h.data(), g.h, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
}

void QpboSolver::maxflow(const QpboOptions &opt, const int32_t *improve_perm) {
  if (d_ctl.n < (size_t)QpboCtl::kWords) d_ctl.alloc(QpboCtl::kWords);
  STEREO_HIP_CHECK(hipMemsetAsync(d_ctl.p, 0, sizeof(int32_t) * QpboCtl::kWords, 0));
  // tile marks are round numbers counted from the start of a launch: none left over from the last one
  if (d_dirty.p) STEREO_HIP_CHECK(hipMemsetAsync(d_dirty.p, 0, sizeof(int32_t) * d_dirty.n, 0));
  // (device properties and the occupancy of the kernel are asked once per process and device:
  // an Improve pass calls this function hundreds of times)
  // (thread local: stereo_hip_set_device selects a device per host thread, and two threads
  // driving different devices must not see each other's half-written entries)
  static thread_local int cached_dev = -1, cached_cus = 0, cached_per_cu = 0;
  int dev = 0;
  STEREO_HIP_CHECK(hipGetDevice(&dev));
  if (dev != cached_dev) {
    int c = 0, pc = 0;
    STEREO_HIP_CHECK(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
    STEREO_HIP_CHECK(hipFuncSetAttribute((const void *)qpbo_maxflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 4 * kMB)));
    STEREO_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, qpbo_maxflow_kernel, kMB, sizeof(double) * 4 * kMB));
    cached_cus = c; cached_per_cu = pc; cached_dev = dev;
  }
  const int cus = cached_cus, per_cu = cached_per_cu;
  if (per_cu < 1) throw HipError{"qpbo_maxflow_kernel does not fit on a CU"};
  int blocks = std::min(cus * std::min(per_cu, 2), std::max(g.ntiles, 1));
  blocks = std::max(blocks, 1);
  // The Improve loop is thousands of tiny steps, each a handful of grid barriers over a few touched tiles: its cost is
  // the barrier, which grows with the number of workgroups that meet there (swept on the Teddy pair's example_global
  // moves, tools/sweep_qpbo.sh).
  if (improve_perm) blocks = std::min(blocks, opt.improve_blocks);
  QpboDev gg = g;
  int32_t *ctl = d_ctl.p;
  // tiled rounds: every node has at most four arcs and the pushed-amount buffer has two halves
  const bool can_tile = max_degree <= 4 && g.hx != nullptr && d_delta.n >= (size_t)2 * std::max(m, 1);
  QpboSchedule sch{};
  sch.relabel_every = opt.relabel_every; sch.first_interval = opt.first_interval; sch.stall_permille = opt.stall_permille;
  sch.max_rounds = 1 << 21;
  sch.tiled = can_tile ? opt.tiled : 0; sch.switch_at = opt.switch_at;
  sch.wrap_at = opt.wrap_at ? opt.wrap_at : 60000;   // (the hx words carry 16 bits of the round number)
  sch.adaptive = opt.adaptive; sch.final_relabel = opt.final_relabel;
  const size_t dyn = sch.tiled ? sizeof(double) * 4 * kMB : 0;
  int improve_N = (int)P.N;
  void *args[] = {&gg, &ctl, &sch, &improve_perm, &improve_N};
  STEREO_HIP_CHECK(hipLaunchCooperativeKernel((const void *)qpbo_maxflow_kernel, dim3(blocks), dim3(kMB), args, dyn, 0));
  int32_t host_ctl[QpboCtl::kWords];
  STEREO_HIP_CHECK(hipMemcpy(host_ctl, d_ctl.p, sizeof(host_ctl), hipMemcpyDeviceToHost));
#ifdef STEREO_HIP_QPBO_CHECK_CONFINED
  {
    int32_t dbg[16];
    STEREO_HIP_CHECK(hipMemcpy(dbg, d_cnt.p + 1100, sizeof(dbg), hipMemcpyDeviceToHost));
    if (dbg[8] || dbg[9])
      std::fprintf(stderr, "[stereo_hip qpbo] confined check: local passes: %d nodes left at another height than the full pass (first v=%d has %d wants %d, warm %d), %d active nodes outside the touched tiles\n",
                   dbg[8], dbg[10], dbg[11], dbg[12], dbg[13], dbg[9]);
    if (dbg[0] || dbg[7])
      std::fprintf(stderr, "[stereo_hip qpbo] confined check: %d unsupported nodes, %d heights outside the touched tiles changed; first v=%d (N=%d) h=%d keep=%d excess=%d relabel#%d step %d\n",
                   dbg[0], dbg[7], dbg[1], (int)P.N, dbg[2], dbg[3], dbg[4], dbg[5], dbg[6]);
    STEREO_HIP_CHECK(hipMemset(d_cnt.p + 1100, 0, sizeof(dbg)));
  }
#endif
  if (host_ctl[QpboCtl::kAbort] == 1) throw HipError{"stereo_rd: grid barrier gave up (device-side spin bound)"};
  if (host_ctl[QpboCtl::kAbort] == 2) throw HipError{"stereo_rd: push-relabel did not converge within the round bound"};
  if (opt.verbose) {
    std::fprintf(stderr, "[stereo_hip qpbo] relabels: %.3f ms, %d barriers; tiled section: %.3f ms, %d rounds\n", host_ctl[11] * 1e-5,
                 host_ctl[12], host_ctl[13] * 1e-5, host_ctl[14]);
    if (improve_perm) {
      int32_t st[3] = {0, 0, 0};
      STEREO_HIP_CHECK(hipMemcpy(st, d_cnt.p + 1300, sizeof(st), hipMemcpyDeviceToHost));
      STEREO_HIP_CHECK(hipMemset(d_cnt.p + 1300, 0, sizeof(st)));
      std::fprintf(stderr, "[stereo_hip qpbo] Improve steps: %d trivial (no residual arc into the fixed node's mate: no solve), %d with the fixed node cut off "
                           "from the sink (confined relabellings), %d with both sides connected\n", st[2], st[0], st[1]);
    }
#ifdef STEREO_HIP_QPBO_PROFILE
    int32_t q[16];
    STEREO_HIP_CHECK(hipMemcpy(q, d_cnt.p + 1200, sizeof(q), hipMemcpyDeviceToHost));
    STEREO_HIP_CHECK(hipMemset(d_cnt.p + 1200, 0, sizeof(q)));
    std::fprintf(stderr, "[stereo_hip qpbo] workgroup 0, relabelling: init %.3f ms, tile set-up %.3f ms (%d tiles), relaxation %.3f ms (%d iterations), "
                 "grid barriers %.3f ms (%d steps); tiled rounds: load %.3f ms (%d tiles), local rounds %.3f ms (%d), store %.3f ms, reduction + grid barrier %.3f ms (%d rounds)\n",
                 q[0] * 1e-5, q[1] * 1e-5, q[4], q[2] * 1e-5, q[5], q[3] * 1e-5, q[6], q[8] * 1e-5, q[12], q[9] * 1e-5, q[13], q[10] * 1e-5, q[11] * 1e-5, q[14]);
#endif
    std::vector<int32_t> tr(1040);
    (void)hipMemcpy(tr.data(), d_cnt.p, sizeof(int32_t) * 1040, hipMemcpyDeviceToHost);
    std::fprintf(stderr, "[stereo_hip qpbo] active per round:");
    for (int i = 0; i < host_ctl[QpboCtl::kRounds] && i < 1024; i += (i < 32 ? 1 : 8)) std::fprintf(stderr, " %d", tr[16 + i]);
    std::fprintf(stderr, "\n");
  }
  iterations += host_ctl[QpboCtl::kRounds];
  relabels += host_ctl[QpboCtl::kRelabels];
}

}  // namespace stereo
