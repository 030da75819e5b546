// QPBO max-flow, host driver: the environment switches of one entry-point call and the solver object (device
// buffers, tiling, the cooperative launch, the Improve pass).  Defined in qpbo_maxflow.hip; used by qpbo_plan.hip.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"
#include "qpbo_dev.h"
#include "qpbo_host.h"

namespace stereo {

// Read from the environment once per entry-point call (stereo_rd, stereo_rd_plan_solve,
// stereo_rd_plan_solve_device) and handed down: callers and tests change the variables between calls.
struct QpboOptions {
  int relabel_every = 256;   // STEREO_HIP_QPBO_RELABEL_EVERY (>= 1)
  int tiled = 16;            // STEREO_HIP_QPBO_TILED: local rounds per tiled round, 0 = plain rounds only
  int switch_at = 16;        // STEREO_HIP_QPBO_SWITCH (>= 0): plain rounds first, most moves end within a dozen of them
  int first_interval = 4;    // STEREO_HIP_QPBO_FIRST_INTERVAL (>= 1): first relabelling after four rounds -- by then the
                             // excess that is cut off from the sink just climbs
  bool adaptive = true;      // STEREO_HIP_QPBO_ADAPTIVE: the slow-tail test of the plain rounds
  // a round that retires less than 1 % of the active nodes counts as stagnant (two of them bring the next exact
  // relabelling forward): excess that is cut off climbs one level per round, a trickle of it still reaching the
  // sink is not progress (swept 0 / 2 / 5 / 10 / 20 / 50: 107 -> 112 moves/s on example_global from 10 on, same labels up to 20)
  int stall_permille = 10;   // STEREO_HIP_QPBO_STALL_PERMILLE (0 .. 999)
  bool final_relabel = false;  // STEREO_HIP_QPBO_FINAL_RELABEL (development): always run the final relabelling
  int wrap_at = 0;           // STEREO_HIP_QPBO_WRAP_AT (development, 0 .. 4095): wrap the round numbers that early, 0 = default
  int improve_blocks = kImproveBlocks;   // STEREO_HIP_QPBO_IMPROVE_BLOCKS (>= 1)
  bool confined = true;      // STEREO_HIP_QPBO_CONFINED: 0 = every relabelling of an Improve step from scratch (round 3)
  bool weak_full = false;    // STEREO_HIP_QPBO_WEAK_FULL: weak persistency on the whole residual network
  bool verbose = false;      // STEREO_HIP_QPBO_VERBOSE
  bool rd_cache = true;      // STEREO_HIP_RD_CACHE: stereo_rd keeps the plan of the last connectivity
  static QpboOptions from_env();
};

struct QpboSolver {
  QpboProblem P;
  int n = 0, m = 0;
  DevBuf<int32_t> d_aptr, d_head, d_rev, d_h, d_h2, d_cnt, d_flags, d_ctl, d_perm, d_posof, d_dirty, d_keep, d_tab, d_iperm;
  DevBuf<double> d_r, d_delta, d_ex, d_snk;
  DevBuf<unsigned long long> d_hx;
  std::vector<double> snk0;
  QpboDev g{};
  int64_t iterations = 0, relabels = 0;
  int max_degree = 0;  // arcs per doubled node (4 on the 4-connected grid)

  // Device buffers for a doubled graph of N variables with the arc ranges `aptr` (2 N + 1 entries, uploaded), QpboDev
  // filled in, the index-range tiling.  Heads, reverse arcs, capacities and terminals are the caller's to fill.
  void bind(int64_t N, const std::vector<int32_t> &aptr);
  // the host-built problem P: bind, then its arcs, capacities and terminals
  void upload();
  // Tiles of the block-local relabelling.  With the grid shape (pixels numbered col * H + row):
  // a 16 column x 32 row patch and its mates; otherwise 512 consecutive nodes and their mates.
  void set_tiling(int64_t Nn, int H, int W);
  // The Improve loop over a permutation of the nodes (QPBO_extra.cpp:1190-1200): every node that is
  // not strongly labelled when its turn comes is fixed to 0 and the flow is maximised again.
  // `h` returns the final heights.
  void improve(const QpboOptions &opt, const std::vector<int32_t> &perm, std::vector<int32_t> &h);
  // One cooperative launch runs the whole max-flow (qpbo_maxflow_kernel); with `improve_perm` (device) the whole Improve loop.
  void maxflow(const QpboOptions &opt, const int32_t *improve_perm = nullptr);
};

}  // namespace stereo
