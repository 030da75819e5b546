// What the stages of the host-side graph analysis (build_trws_graph, trws_graph.h) pass to each other.  Internal to
// the trws_graph*.cpp files (file map: trws_plan.hip).
#pragma once
#include <chrono>
#include <cstdio>
#include <optional>

#include "trws_graph.h"

namespace stereo {

// One sweep direction seen from the node that is visited: incoming / outgoing lists by rank, processing positions.
struct DirView {
  const TrwsGraph &g;
  const int d;
  const int64_t N;
  const std::vector<int32_t> &iptr, &iidx, &optr, &oidx;
  const int32_t *const own;   // per NODE, nullptr with one strip
  DirView(const TrwsGraph &g_, int d_)
      : g(g_), d(d_), N(g_.N), iptr(d_ == 0 ? g_.bptr : g_.fptr), iidx(d_ == 0 ? g_.bidx : g_.fidx),
        optr(d_ == 0 ? g_.fptr : g_.bptr), oidx(d_ == 0 ? g_.fidx : g_.bidx), own(g_.nstrips > 1 ? g_.owner.data() : nullptr) {}
  // processing position <-> rank (position p is rank p forward, rank N-1-p backward; its own inverse)
  int64_t position(int32_t r) const { return d == 0 ? (int64_t)r : N - 1 - (int64_t)r; }
  int32_t rank_at(int64_t p) const { return d == 0 ? (int32_t)p : (int32_t)(N - 1 - p); }
  // rank at the other end of an incoming edge / node at the other end of an incoming, of an outgoing edge
  int32_t other_end(int32_t e_in) const { return g.rank[other_node(e_in)]; }
  int32_t other_node(int32_t e_in) const { return d == 0 ? g.tail[e_in] : g.head[e_in]; }
  int32_t far_node(int32_t e_out) const { return d == 0 ? g.head[e_out] : g.tail[e_out]; }
  int32_t strip_of(int32_t r) const { return own ? own[g.order[r]] : 0; }
  // slot of edge e in the outgoing list of rank o (only the first kMaxSlots can hand over in LDS); -1: none
  int slot_in(int32_t o, int32_t e) const {
    int slot = -1;
    for (int32_t w = optr[o]; w < optr[o + 1] && w - optr[o] < TrwsGraph::kMaxSlots; ++w)
      if (oidx[w] == e) slot = w - optr[o];
    return slot;
  }
};

// foreign dependencies of one node: at most kMaxSlots incoming edges where the descriptor-driven kernels apply
struct Deps {
  int32_t v[TrwsGraph::kMaxSlots]; int32_t n = 0;
  const int32_t *begin() const { return v; }
  const int32_t *end() const { return v + n; }
  size_t size() const { return (size_t)n; }
  int32_t operator[](int k) const { return v[k]; }
  void push_back(int32_t x) { v[n++] = x; }
  void assign(const int32_t *a, const int32_t *b) { n = 0; for (; a != b; ++a) v[n++] = *a; }
};

// What a descriptor-driven kernel walks in one direction.  The chain schedule is one, the rank-contiguous fallback is
// one, the sub-row stage makes a third from the chain schedule's; finish_schedule derives everything else from it.
struct RunSet {
  explicit RunSet(const std::vector<int32_t> &positions) : chain_rank(positions) {}
  bool chain = false;                 // runs are paths of the dependency DAG (false: the rank-contiguous fallback)
  const std::vector<int32_t> &chain_rank;   // schedule position -> rank: Sweep::chain_rank, built once per direction
  std::vector<int32_t> run_ptr;       // R+1 offsets into schedule positions
  std::vector<int32_t> run_order;     // ticket -> run (run_of_ticket: empty = identity)
  std::vector<int32_t> pred, pred2;   // by rank: the node one / two visits earlier in the run that hands over in LDS, or -1
  std::vector<Deps> deps;             // by rank: the nodes whose completion flags are waited for
  int64_t runs() const { return (int64_t)run_ptr.size() - 1; }
};

// STEREO_HIP_GRAPH_VERBOSE: time since the previous stage, on stderr
class StageClock {
 public:
  explicit StageClock(bool on) : on_(on), last_(std::chrono::steady_clock::now()) {}
  void done(const char *stage) {
    if (!on_) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[graph] -> %s: %.1f ms\n", stage, std::chrono::duration<double, std::milli>(now - last_).count());
    last_ = now;
  }
 private:
  bool on_;
  std::chrono::steady_clock::time_point last_;
};

// The ticket look-ahead rule: with fewer workgroups than runs, waiting never blocks a strip's dispenser if a run only
// looks ahead to the very next ticket of its strip and that one looks ahead to nobody.  order: ticket -> run over all
// strips (a strip's tickets are the positions among its own runs); run_of: by rank.
bool look_ahead_ok(const std::vector<int32_t> &order, const std::vector<int32_t> &strip_of_run, int nstrips,
                   const std::vector<int32_t> &run_of, const std::vector<Deps> &deps);

// ---- trws_graph_schedule.cpp
// cut: as for the rank-contiguous runs (more of those than resident workgroups); resident: workgroups certain to be
// resident where the tickets may outnumber them, 0: never.  Falls back to the runs of S (contiguous_runs).  Fills
// S.chain_rank, which the RunSet refers to.
RunSet chain_schedule(const DirView &v, TrwsGraph::Sweep &S, bool cut, int64_t resident, StageClock &clock);
// The chain schedule's runs cut into pieces of at most row_chunk positions (`whole`: the run that stays in one piece,
// or -1), with their ticket order.  Consumes the chain schedule's RunSet; empty: no such runs.
std::optional<RunSet> sub_row_runs(const DirView &v, RunSet chain, int32_t whole, int64_t row_chunk);

// ---- trws_graph_desc.cpp
struct Finished {
  bool terminates = false;            // the loader protocol terminates on the runs
  std::vector<int32_t> desc, run_strip;
  TrwsGraph::Sweep::Spec spec;
};
// res: the workgroups certain to be resident where the tickets may outnumber them (0: never); with_resident: the
// plain runs' protocol must terminate with that many, too.
Finished finish_schedule(const DirView &v, const RunSet &runs, int64_t res, bool with_resident, int seg_len, StageClock &clock);

}  // namespace stereo
