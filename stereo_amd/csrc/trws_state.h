// The solver state's host-side rules (the C ABI: include/stereo_hip.h), host only: the key of a
// connectivity, what a load refuses, and which rows of a state a strip is authoritative for.  Shared by plan creation,
// trws_state.hip and the host-only entries in trws_graph_views.cpp.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/stereo_hip.h"
#include "trws_graph.h"

namespace stereo {

// FNV-1a, 64 bit, one step per uint32 word of the 2 x E connectivity
inline uint64_t trws_connectivity_key(const uint32_t *conn, int64_t E) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t i = 0; i < 2 * E; ++i) { h ^= conn[i]; h *= 0x100000001b3ull; }
  return h;
}

// Why a plan created with these facts does not take the state (the field by name), or "" if it does.  message_mode:
// as given at creation; its STEREO_TRWS_ORDER_INDEX bit must agree, exact / min-plus may differ.
inline std::string trws_state_refusal(const stereo_trws_state_header &h, int kernel, int K, int64_t N, int64_t E, uint64_t key,
                                      int message_mode) {
  auto differs = [](const char *field, long long have, long long want) {
    return std::string("the state's ") + field + " (" + std::to_string(have) + ") is not the plan's (" + std::to_string(want) + ")";
  };
  if (h.magic != STEREO_TRWS_STATE_MAGIC) return "magic: not a TRW-S solver state";
  if (h.version != STEREO_TRWS_STATE_VERSION) return differs("version", h.version, STEREO_TRWS_STATE_VERSION);
  if (h.kernel != kernel) return differs("kernel", h.kernel, kernel);
  if (h.K != K) return differs("K", h.K, K);
  if (h.N != N) return differs("N", h.N, N);
  if (h.E != E) return differs("E", h.E, E);
  if (h.connectivity_key != key) return "connectivity_key: the state belongs to another connectivity";
  if ((h.message_mode & STEREO_TRWS_ORDER_INDEX) != (message_mode & STEREO_TRWS_ORDER_INDEX))
    return "message_mode: the state's STEREO_TRWS_ORDER_INDEX bit is not the plan's (another node order)";
  if (h.phase < 0 || h.phase > 2) return "phase: " + std::to_string(h.phase) + " is not 0, 1 or 2";
  if (h.iterations < 0) return "iterations: negative";
  return "";
}

// take[e] = 1 where strip `strip` holds the valid copy of edge row e at rest in `phase`: the strip that owns the end the
// row's message points INTO -- the endpoint later in the node order after a forward sweep (phase 1), the earlier one
// after a backward sweep (phase 0).  g: built with the owner table (tail has the lower rank).
inline void strip_state_rows(const TrwsGraph &g, int strip, int phase, uint8_t *take) {
  const int64_t E = (int64_t)g.tail.size();
  for (int64_t e = 0; e < E; ++e) take[e] = g.owner[phase == 1 ? g.head[e] : g.tail[e]] == strip ? 1 : 0;
}

// One strip's part of a grouped gather / scatter launch (trws_state.hip): rows of its local [n_rows][K] message array
// and its local labels against the arrays of the whole problem, through its local -> global ids.
struct StateBlock {
  double *msg;
  int32_t *x;
  const int64_t *ledges, *lnodes;
  const uint8_t *take;   // gather: per local row, 1 = the strip's copy is the valid one; NULL: every row
  int64_t n_rows, n_labels;
  int K, lg;             // lg: log2 of the lanes that share a row
};

}  // namespace stereo
