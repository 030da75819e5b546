// The TRW-S plan object and what the units around it share (internal; the C ABI is include/stereo_hip.h).
// The header comment of trws_plan.hip has the map of the plan's host code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/stereo_hip.h"
#include "common.h"
#include "trws_batch.h"
#include "trws_family.h"
#include "trws_graph.h"
#include "trws_dev.h"
#include "trws_launch.h"
#include "trws_state.h"

namespace stereo {

constexpr int kCtlWords = 8;  // d_ctl: ticket, abort flag, four words of give-up report, two spare

static_assert(kFamilyPipeMaxK == kWave && kFamilyPipe2MaxK == 2 * kWave && kFamilyWideMaxK == 4 * kWave &&
              kFamilyGenericMaxK == kGenericMaxK && kFamilyLargeMaxK == kLargeMaxK, "trws_family.h restates the kernels' label ranges");

// The environment switches a plan freezes at creation (the last three are read by the gateway and by trws_graph.cpp: spec_segment_length).
// Creation reads its switches through this table and the gateway's cache key is made of the same table: a cached
// plan must not outlive them.
enum TrwsSwitch { kSwFast, kSwSpec, kSwGranules, kSwCertificate, kSwSpinSeconds, kSwProf, kSwTimeline, kSwFineGrained, kSwGpus, kSwSpecSeg, kSwBeliefsStrips, kSwRowChunk, kSwIterateAhead, kSwCount };
constexpr const char *kTrwsSwitchNames[kSwCount] = {
    "STEREO_HIP_TRWS_FAST", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_CERTIFICATE", "STEREO_HIP_TRWS_SPIN_SECONDS",
    "STEREO_HIP_TRWS_PROF", "STEREO_HIP_TRWS_TIMELINE", "STEREO_HIP_STRIPS_FINEGRAINED", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC_SEG",
    "STEREO_HIP_TRWS_BELIEFS_STRIPS", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_ITERATE_AHEAD"};
// STEREO_HIP_TRWS_ROW_CHUNK unset: positions per sub-row run of the K <= 64 family in the forward and in the backward
// sweep; 0: whole rows.  Measured: the backward sweep wants more workgroups than there are and gains
// from pieces, the forward sweep sits at the line and only pays for their hand-overs.  The switch takes "n" for both
// sweeps or "f,b".
constexpr int kRowChunkDefault[2] = {0, 112};
inline const char *trws_switch(TrwsSwitch s) { return std::getenv(kTrwsSwitchNames[s]); }
inline std::string trws_env_key() {
  std::string k;
  for (const char *name : kTrwsSwitchNames) {
    const char *v = std::getenv(name);
    k += v ? v : "-";
    k += '|';
  }
  return k;
}

}  // namespace stereo

struct stereo_trws_plan {
  int kernel = 1, K = 0, Kp = 0, mode = 0, device = 0;
  int64_t N = 0, E = 0;
  // what a solver state is checked against (trws_state.h): the key of the connectivity given at creation, and
  // STEREO_TRWS_ORDER_INDEX if the plan was created with it (mode has the message mode alone)
  uint64_t conn_key = 0;
  int order_flag = 0;
  std::shared_ptr<const stereo::TrwsGraph> graph;  // host-side analysis; shared with the cache of the last connectivity
  // device copies of the graph
  stereo::DevBuf<int32_t> d_tail, d_order, d_fptr, d_fidx, d_bptr, d_bidx, d_lbn, d_lbe, d_x;
  stereo::DevBuf<uint8_t> d_mdir;
  stereo::DevBuf<double> d_gamma, d_msg, d_lbterms, d_eterms;
  // tagged-granule hand-over of trws_pipe_kernel (DevParams::gran / xgran); unallocated: off
  stereo::DevBuf<unsigned long long> d_gran, d_xgran;
  // persistent sweep schedule
  stereo::DevBuf<int32_t> d_run_order[2], d_chain_run_ptr[2], d_chain_run_order[2];
  stereo::DevBuf<int32_t> d_run_ptr[2], d_dep_ptr[2], d_dep_rank[2], d_done, d_ctl;  // d_ctl: [ticket, abort, give-up report x 4]
  stereo::DevBuf<int8_t> d_in_slot[2];
  stereo::DevBuf<int32_t> d_desc[2];
  // sub-row runs (trws_graph.h: Sweep::Chunked) of the directions that have them: what the plan's OWN launches on the
  // K <= 64 kernel walk instead of the chain schedule (strip groups and batches, the members' own launches inside a
  // batch included, keep that one)
  bool sub_rows[2] = {false, false};
  stereo::DevBuf<int32_t> d_sub_desc[2], d_sub_run_ptr[2], d_sub_run_order[2];
  stereo::DevBuf<int32_t> d_sub_spec_run_ptr[2], d_sub_spec_run_order[2], d_sub_spec_kind[2];
  // the runner's chain records (trws_runner_records.h) per direction, [0] over the chain schedule's descriptors, [1]
  // over the sub-row schedule's, and the segment geometry {c0, c1, seg_len, nseg} each was built for
  stereo::DevBuf<int32_t> d_run_rec[2][2];
  int32_t run_rec_geom[2][2][4] = {};
  // which sweep kernel runs the plan (trws_family.h): the facts and the families still possible are fixed at creation,
  // the family follows every upload / bind (finish_inputs)
  stereo::TrwsPlanFacts facts;
  unsigned families = 0;
  stereo::TrwsFamily family = stereo::TrwsFamily::None;
  stereo::DevBuf<double> d_large_scr;  // trws_large_kernel: its serial construction's stack, one slab per workgroup
  bool pos_ascending = false;  // shared positions finite and strictly ascending
  double pos_first = 0, pos_last = 0, pos_gap = 0;
  int window = 0;
  double uniform_step = 0;
  stereo::DevBuf<unsigned long long> d_fallbacks, d_prof, d_timeline;
  bool certificate = true;
  int epoch = 0;
  long long spin_ticks = 0;  // wall-clock bound of a wait for another workgroup (100 MHz ticks)
  bool fwd_pending = false;  // the forward sweep of the next iteration has already run
  int grid_blocks = 0;
  // inputs (owned unless bound)
  stereo::DevBuf<double> o_unary, o_q, o_qprim, o_pos, o_alpha;
  stereo::DevBuf<uint16_t> d_perm_q, d_perm_qp, d_perm_pos;
  const double *unary = nullptr, *q = nullptr, *qprim = nullptr, *pos = nullptr, *alpha = nullptr;
  double lambda = 0;
  bool have_inputs = false;
  stereo::PinnedBuf<double> h_lb, h_en;
  stereo::PinnedBuf<int32_t> h_x, h_ctl;
  hipStream_t issue_stream = nullptr;
  stereo_trws_plan *timed_by = nullptr;  // first plan of the group launch this plan was issued in
  double energy = 0, lb = 0;
  int64_t iterations = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // the lower-bound terms of an iteration go to the host on their own stream while the next
  // launch (forward sweep + primal) runs, and are summed there meanwhile
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_bwd = nullptr, ev_lb = nullptr;
  bool lb_in_flight = false;
  // The backward sweep of the NEXT iteration, launched behind the fused launch before the host has this iteration's
  // sums (stereo_trws_plan_iterate).  Pending: it has been launched and no iteration has taken it yet.
  // Until one does, its lower-bound terms wait in h_lb_next, its sweep launch is not counted, and h_held has what
  // d_fallbacks [0] and d_spec_stat [1 .. 32] read before it: a caller sees the plan as if the sweep had not run.
  bool bwd_pending = false;
  bool ahead_allowed = true;   // STEREO_HIP_TRWS_ITERATE_AHEAD is not 0 (measurement aid: the sweep behind the sums again)
  hipEvent_t ev_ahead = nullptr;   // recorded behind the pending sweep: a call on another stream waits for it
  stereo::PinnedBuf<double> h_lb_next;
  stereo::PinnedBuf<unsigned long long> h_held;
  int64_t held_launches = 0;
  // ev_fwd: the fused launch and the copies behind it on its stream are done; ev_end: the iteration's terms are on the host
  hipEvent_t ev_lb_next = nullptr, ev0_next = nullptr, ev_fwd = nullptr, ev_end = nullptr;
  double sweep_ms = 0;
  int64_t sweep_launches = 0;
  bool time_sweeps = false;
  // row strips (one plan per strip; see DevParams)
  int nstrips = 1, strip = 0;
  stereo::DevBuf<int32_t> d_tickets[2];
  int ntickets[2] = {0, 0};
  int64_t n_lb = 0, n_en = 0;  // lower-bound / energy terms this plan writes (strip-local with strips)
  // what the arrays on the device are sized for: the whole problem, or with strips the strip's own
  // nodes + halo and the edges with an own endpoint (StripLayout, trws_graph.h)
  int64_t Nl = 0, El = 0;
  std::unique_ptr<stereo::StripLayout> layout;
  stereo::DevBuf<int64_t> d_lnodes, d_ledges;  // local -> global ids, for gathering the strip's inputs
  double *peer_msg[2] = {nullptr, nullptr};
  int32_t *peer_done[2] = {nullptr, nullptr}, *peer_x[2] = {nullptr, nullptr};
  bool need_peer[2] = {false, false};
  void *ipc_mapped[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  stereo::DevBuf<stereo::DevParams> d_group;         // parameters of the strips launched together with this one (first plan of a group)
  stereo::PinnedBuf<stereo::DevParams> h_group;
  hipStream_t own_stream = nullptr;  // strips launch concurrently: never on the NULL stream
  bool issued = false;
  int cus = 256;
  // speculative schedule of the long serial run (trws_graph.h: Sweep::Spec; trws_spec.h)
  stereo::DevBuf<int32_t> d_spec_run_ptr[2], d_spec_run_order[2], d_spec_kind[2], d_spec_x;
  stereo::DevBuf<double> d_spec_rows, d_spec_undo;
  stereo::DevBuf<unsigned long long> d_spec_stat;
  stereo::DevBuf<stereo::DevParams> d_self;
  stereo::PinnedBuf<stereo::DevParams> h_self;
  bool self_sent = false;
  bool spec_allowed = false;   // the graph has such a run in both directions and STEREO_HIP_TRWS_SPEC is not 0
  bool spec_window = false;    // the positions are uniformly spaced over the window rounded up to four (finish_inputs)
  // node beliefs (stereo_trws_plan_keep_min_marginals): phase 1's partial sums D_i + firstForward
  // messages, K x N in node-id order; allocated only while the flag is on.  mm_ready: phase 1 ran in the last iteration
  // A strip keeps them for its own nodes only (K x n_own, by strip-local id) and walks lists of its own
  // (trws_graph.h: StripBeliefLists), built and uploaded when the flag is turned on.
  bool keep_mm = false, mm_ready = false;
  stereo::DevBuf<double> d_belief;
  stereo::DevBuf<int32_t> d_bel_own, d_bel_fptr, d_bel_fidx, d_bel_bptr, d_bel_bidx;
  // The block tables of the grouped belief launches this plan was the first plan of (phase 1 at [0], phase 2 at
  // [kMaxGroup]) and what was sent last: a table goes to the device again only when it changes.
  stereo::DevBuf<stereo::BeliefBlock> d_bel_table;
  stereo::BeliefBlock bel_sent[2][stereo::kMaxGroup];
  int bel_sent_n[2] = {0, 0};
  // solver state.  state_loaded_at: the iteration count a loaded state came with, -1: none since the
  // last reset (a strip whose count still equals it has no terms of its own to sum energy and bound from).  Allocated
  // by the first save / load of a strip group on one device: the strip's authoritative rows by local edge id per
  // phase, and -- with the first plan of a group -- the block tables of the grouped gather [0] and scatter [kMaxGroup]
  // launches with what was sent last
  int64_t state_loaded_at = -1;
  stereo::DevBuf<uint8_t> d_state_take[2];
  stereo::DevBuf<stereo::StateBlock> d_state_table;
  stereo::StateBlock state_sent[2][stereo::kMaxGroup];
  int state_sent_n[2] = {0, 0};
  ~stereo_trws_plan() {
    for (int w = 0; w < 2; ++w)
      for (int k = 0; k < 3; ++k)
        if (ipc_mapped[w][k]) (void)hipIpcCloseMemHandle(ipc_mapped[w][k]);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_bwd) (void)hipEventDestroy(ev_bwd);
    if (ev_lb) (void)hipEventDestroy(ev_lb);
    if (ev_lb_next) (void)hipEventDestroy(ev_lb_next);
    if (ev0_next) (void)hipEventDestroy(ev0_next);
    if (ev_end) (void)hipEventDestroy(ev_end);
    if (ev_fwd) (void)hipEventDestroy(ev_fwd);
    if (ev_ahead) (void)hipEventDestroy(ev_ahead);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
  }
};

// Independent plans that share the launches of a sweep (stereo_trws_batch_*).  The members stay the
// caller's; the batch owns the table of their parameter blocks and its control words.
struct stereo_trws_batch {
  std::vector<stereo_trws_plan *> members;
  std::vector<char> stopped;      // per member: met max_relgap in a batch iteration; stays out until stereo_trws_batch_reset
  int device = 0;
  int capacity = 0;               // workgroups of one launch that are resident together
  // one region of kMaxGroup blocks per launch of an iteration (forward, backward, fused): the members of a launch, compacted
  stereo::DevBuf<stereo::DevParams> d_table;
  stereo::PinnedBuf<stereo::DevParams> h_table;
  stereo::DevBuf<unsigned long long> d_ctl;   // kBatchCtlWords (BatchArgs::ctl)
  int64_t launches = 0;           // sweep launches issued (a batch split for capacity counts each part)
};

namespace stereo {

// trws_plan.hip
bool spec_active(const stereo_trws_plan *P);   // the speculative schedule runs with the plan's current inputs
// allow_spec: the speculative schedule (a plan's own launches); allow_sub: its sub-row runs (a single plan, no batch)
DevParams make_params(stereo_trws_plan *P, bool allow_spec = true, bool allow_sub = true);
// the plan's own launches walk direction d's sub-row runs; the speculative schedule over the runs they walk
bool own_sub_rows(const stereo_trws_plan *P, int d);
const TrwsGraph::Sweep::Spec &own_spec(const stereo_trws_plan *P, int d);
// trws_plan_create.hip: the runner's chain records of direction d over the chain schedule's descriptors (sub false) or
// the sub-row schedule's, for the segment geometry make_params binds with them; built and uploaded again only if that
// geometry is not the one the device copy was made for.  Returns the device copy.
const int32_t *runner_records(stereo_trws_plan *P, int d, bool sub);
size_t persistent_lds_bytes(bool large, int Kp);   // dynamic LDS of the generic / the large family's sweep kernel
constexpr int kHeldWords = 33;                     // stereo_trws_plan::h_held
// the state of a minimisation: zero messages, labels, flags, counters of iterations (a pending sweep is discarded first)
void reset_state(stereo_trws_plan *P);
void discard_backward_ahead(stereo_trws_plan *P);
// the buffers and events of a backward sweep launched ahead, on first use (issue_backward_ahead; a loaded phase-2 state)
void ensure_ahead_buffers(stereo_trws_plan *P);

// trws_inputs.hip: what an upload or bind leaves to do on the device and on the positions
void run_argsort(const double *vals, uint16_t *perm, int K, int64_t count, hipStream_t s);
void fix_equal_positions(const double *d_vals, uint16_t *d_perm, int K, int64_t count);
void gather_rows(const double *d_full, const int64_t *d_rows, int64_t n, int width, double *d_out);
// the plan's sort permutations for its current inputs (shared positions or q / qprim per edge)
void sort_positions(stereo_trws_plan *P);
// K doubles from the device to hp; true iff they are finite and strictly ascending
bool positions_ascend(const double *d_pos, int K, std::vector<double> &hp);
// ascending shared positions with lambda >= 0: the plan's truncation window, uniform_step and spec_window
void analyse_window(stereo_trws_plan *P, const std::vector<double> &hp);

// trws_plan_debug.hip: what stereo_trws_plan_destroy prints under STEREO_HIP_TRWS_TIMELINE / _PROF
void print_timeline(const stereo_trws_plan *plan);
void print_profile(const stereo_trws_plan *plan);

}  // namespace stereo
