// Host-only views of the graph analysis for tests and tools (extern "C", no device needed).  See trws_graph.h.
#include "trws_graph.h"

#include "../../include/stereo_hip.h"
#include "common.h"
#include "trws_state.h"

#include <algorithm>

namespace {
stereo::TrwsGraphOptions strips(const int32_t *owner, int nstrips) {
  stereo::TrwsGraphOptions opt;
  opt.owner = owner; opt.nstrips = nstrips;
  return opt;
}
}  // namespace

extern "C" int stereo_trws_analyze(int64_t N, int64_t E, const uint32_t *conn, int64_t *rank,
                                   int64_t *tail, int64_t *head, int32_t *mdir, int64_t *fwd_ptr,
                                   int64_t *fwd_idx, int64_t *bwd_ptr, int64_t *bwd_idx,
                                   int64_t *level, char *err, size_t errcap) {
  stereo::TrwsGraph g;
  std::string gerr;
  if (!conn && E > 0) return stereo::fail("stereo_trws_analyze: NULL connectivity", err, errcap);
  if (!stereo::build_trws_graph(N, E, conn, stereo::TrwsGraphOptions(), g, gerr)) return stereo::fail(gerr, err, errcap);
  const int L = (int)g.level_ptr.size() - 1;
  if (level)
    for (int l = 0; l < L; ++l)
      for (int32_t k = g.level_ptr[l]; k < g.level_ptr[l + 1]; ++k) level[g.order[g.level_ranks[k]]] = l;
  int64_t pf = 0, pb = 0;
  for (int64_t i = 0; i < N; ++i) {
    const int32_t r = g.rank[i];
    if (rank) rank[i] = r;
    if (fwd_ptr) fwd_ptr[i] = pf;
    if (bwd_ptr) bwd_ptr[i] = pb;
    for (int32_t k = g.fptr[r]; k < g.fptr[r + 1]; ++k, ++pf) if (fwd_idx) fwd_idx[pf] = g.fidx[k];
    for (int32_t k = g.bptr[r]; k < g.bptr[r + 1]; ++k, ++pb) if (bwd_idx) bwd_idx[pb] = g.bidx[k];
  }
  if (fwd_ptr) fwd_ptr[N] = pf;
  if (bwd_ptr) bwd_ptr[N] = pb;
  for (int64_t e = 0; e < E; ++e) {
    if (tail) tail[e] = g.tail[e];
    if (head) head[e] = g.head[e];
    if (mdir) mdir[e] = g.mdir[e];
  }
  return 0;
}

namespace {
// what a schedule view asks for and where it goes (any output may be NULL)
struct ScheduleView {
  const char *who = "";
  int64_t max_resident_runs = 0, row_chunk = 0, chunk_resident = 0;
  const int32_t *owner = nullptr;
  int nstrips = 1, direction = 0;
  int64_t *rank_at = nullptr, *run_ptr = nullptr, *nruns = nullptr, *ticket_run = nullptr, *pred_rank = nullptr, *dep_ptr = nullptr,
          *dep_rank = nullptr, *run_strip = nullptr, *remote = nullptr, *chunk_info = nullptr;
  int32_t *desc = nullptr;
};

int schedule_impl(int64_t N, int64_t E, const uint32_t *conn, const ScheduleView &o, char *err, size_t errcap) {
  stereo::TrwsGraph g;
  std::string gerr;
  if (!conn && E > 0) return stereo::fail(std::string(o.who) + ": NULL connectivity", err, errcap);
  if (o.direction != 0 && o.direction != 1) return stereo::fail(std::string(o.who) + ": direction must be 0 or 1", err, errcap);
  stereo::TrwsGraphOptions opt;
  opt.max_resident_runs = o.max_resident_runs; opt.owner = o.owner; opt.nstrips = o.nstrips;
  opt.row_chunk_forward = o.row_chunk; opt.chunk_resident = o.chunk_resident;
  if (!stereo::build_trws_graph(N, E, conn, opt, g, gerr)) return stereo::fail(gerr, err, errcap);
  if (!g.fast_ok) return stereo::fail(std::string(o.who) + ": graph not eligible for the descriptor-driven kernels", err, errcap);
  const stereo::TrwsGraph::Sweep &S = g.sweep[o.direction];
  constexpr int W = stereo::TrwsGraph::kDescWords;
  // the sub-row runs where the direction has them (chunk_info[0]), the chain schedule otherwise
  const bool sub = S.chunked.ok;
  const std::vector<int32_t> &S_desc = sub ? S.chunked.desc : S.desc, &S_run_ptr = sub ? S.chunked.run_ptr : S.chain_run_ptr;
  const std::vector<int32_t> &S_run_order = sub ? S.chunked.run_order : S.chain_run_order;
  if (o.chunk_info) {
    const stereo::TrwsGraph::Sweep::Spec &sp = sub ? S.chunked.spec : S.spec;
    o.chunk_info[0] = sub ? 1 : 0; o.chunk_info[1] = S.chunked.chunk; o.chunk_info[2] = sp.ok ? 1 : 0; o.chunk_info[3] = sp.ok ? sp.run : -1;
  }
  if (o.desc) std::copy(S_desc.begin(), S_desc.end(), o.desc);
  const int64_t R = (int64_t)S_run_ptr.size() - 1;
  if (o.nruns) *o.nruns = R;
  for (int64_t p = 0; p < N; ++p) if (o.rank_at) o.rank_at[p] = S.chain_rank[p];
  for (int64_t k = 0; k <= R; ++k) if (o.run_ptr) o.run_ptr[k] = S_run_ptr[k];
  for (int64_t t = 0; t < R; ++t) if (o.ticket_run) o.ticket_run[t] = stereo::run_of_ticket(S_run_order, t);
  for (int64_t k = 0; k < R; ++k) if (o.run_strip) o.run_strip[k] = S.chain_run_strip.empty() ? 0 : S.chain_run_strip[k];
  // predecessor and dependencies as the kernels see them: from the descriptors
  int64_t dp = 0;
  std::vector<int64_t> pos_of(N);
  for (int64_t p = 0; p < N; ++p) pos_of[S.chain_rank[p]] = p;
  for (int64_t r = 0; r < N; ++r) {
    const int32_t *D = &S_desc[(size_t)pos_of[r] * W];
    const int nout = stereo::desc_nout(D), nin = stereo::desc_nin(D), nd = stereo::desc_ndep(D);
    int64_t pr = -1;
    for (int k = nout; k < nout + nin; ++k) {
      const int32_t slot = D[stereo::kDescSlot + k];
      if (slot >= 0 && slot < 8) pr = g.rank[D[stereo::kDescOther + k]];
    }
    if (o.pred_rank) o.pred_rank[r] = pr;
    if (o.remote) o.remote[r] = (uint32_t)D[stereo::kDescRemote];
    if (o.dep_ptr) o.dep_ptr[r] = dp;
    for (int k = 0; k < nd; ++k, ++dp) if (o.dep_rank) o.dep_rank[dp] = D[stereo::kDescDep + k];
  }
  if (o.dep_ptr) o.dep_ptr[N] = dp;
  return 0;
}
}  // namespace

extern "C" int stereo_trws_schedule(int64_t N, int64_t E, const uint32_t *conn, int64_t max_resident_runs,
                                    int direction, int64_t *rank_at, int64_t *run_ptr, int64_t *nruns,
                                    int64_t *ticket_run, int64_t *pred_rank, int64_t *dep_ptr,
                                    int64_t *dep_rank, char *err, size_t errcap) {
  ScheduleView o;
  o.who = "stereo_trws_schedule"; o.max_resident_runs = max_resident_runs; o.direction = direction;
  o.rank_at = rank_at; o.run_ptr = run_ptr; o.nruns = nruns; o.ticket_run = ticket_run; o.pred_rank = pred_rank;
  o.dep_ptr = dep_ptr; o.dep_rank = dep_rank;
  return schedule_impl(N, E, conn, o, err, errcap);
}

extern "C" int stereo_trws_schedule_strips(int64_t N, int64_t E, const uint32_t *conn, int64_t max_resident_runs,
                                           int direction, const int32_t *owner, int nstrips, int64_t *rank_at,
                                           int64_t *run_ptr, int64_t *nruns, int64_t *ticket_run,
                                           int64_t *pred_rank, int64_t *dep_ptr, int64_t *dep_rank,
                                           int64_t *run_strip, int64_t *remote, char *err, size_t errcap) {
  if (nstrips > 1 && !owner) return stereo::fail("stereo_trws_schedule_strips: NULL owner", err, errcap);
  ScheduleView o;
  o.who = "stereo_trws_schedule_strips"; o.max_resident_runs = max_resident_runs; o.direction = direction;
  o.owner = owner; o.nstrips = nstrips;
  o.rank_at = rank_at; o.run_ptr = run_ptr; o.nruns = nruns; o.ticket_run = ticket_run; o.pred_rank = pred_rank;
  o.dep_ptr = dep_ptr; o.dep_rank = dep_rank; o.run_strip = run_strip; o.remote = remote;
  return schedule_impl(N, E, conn, o, err, errcap);
}

// Host-only view of the sub-row runs (trws_graph.h: Sweep::Chunked), for CPU tests: stereo_trws_schedule's arrays for the
// runs of at most row_chunk positions that a launch with chunk_resident resident workgroups would walk, and their
// descriptors (N x kDescWords, may be NULL).  chunk_info[0..3] = the direction has sub-row runs (0: the arrays are the
// chain schedule's, as from stereo_trws_schedule), chunk length, the speculative schedule exists, its cut run.
extern "C" int stereo_trws_schedule_chunked(int64_t N, int64_t E, const uint32_t *conn, int64_t max_resident_runs, int direction,
                                            int64_t row_chunk, int64_t chunk_resident, int64_t *chunk_info, int64_t *rank_at,
                                            int64_t *run_ptr, int64_t *nruns, int64_t *ticket_run, int64_t *pred_rank,
                                            int64_t *dep_ptr, int64_t *dep_rank, int32_t *desc, char *err, size_t errcap) {
  if (row_chunk < 0 || chunk_resident < 0) return stereo::fail("stereo_trws_schedule_chunked: bad argument", err, errcap);
  ScheduleView o;
  o.who = "stereo_trws_schedule_chunked"; o.max_resident_runs = max_resident_runs; o.direction = direction;
  o.row_chunk = row_chunk; o.chunk_resident = chunk_resident; o.chunk_info = chunk_info; o.desc = desc;
  o.rank_at = rank_at; o.run_ptr = run_ptr; o.nruns = nruns; o.ticket_run = ticket_run; o.pred_rank = pred_rank;
  o.dep_ptr = dep_ptr; o.dep_rank = dep_rank;
  return schedule_impl(N, E, conn, o, err, errcap);
}

// Host-only view of the speculative schedule (trws_graph.h: Sweep::Spec), for CPU tests of its dependency structure.
// info[0..5] = ok, cut run (index in the chain schedule), c0, c1, segment length, segments; the arrays (may be NULL)
// take the schedule with the cut run as segments: run_ptr (runs + 1), kind (runs), ticket_run (tickets = runs + 1,
// -1 = the runner); *nruns = runs.  Together with stereo_trws_schedule (positions, dependencies) that is everything
// the kernels walk.
extern "C" int stereo_trws_spec_schedule(int64_t N, int64_t E, const uint32_t *conn, int direction, int64_t *info,
                                         int64_t *nruns, int64_t *run_ptr, int64_t *kind, int64_t *ticket_run, char *err,
                                         size_t errcap) {
  if (!conn || !info || (direction != 0 && direction != 1)) return stereo::fail("stereo_trws_spec_schedule: bad argument", err, errcap);
  stereo::TrwsGraph g;
  std::string gerr;
  if (!stereo::build_trws_graph(N, E, conn, stereo::TrwsGraphOptions(), g, gerr)) return stereo::fail(gerr, err, errcap);
  const stereo::TrwsGraph::Sweep::Spec &sp = g.sweep[direction].spec;
  info[0] = sp.ok ? 1 : 0; info[1] = sp.run; info[2] = sp.c0; info[3] = sp.c1; info[4] = sp.seg_len; info[5] = sp.nseg;
  if (nruns) *nruns = (int64_t)sp.kind.size();
  for (size_t k = 0; run_ptr && k < sp.run_ptr.size(); ++k) run_ptr[k] = sp.run_ptr[k];
  for (size_t k = 0; kind && k < sp.kind.size(); ++k) kind[k] = sp.kind[k];
  for (size_t k = 0; ticket_run && k < sp.run_order.size(); ++k) ticket_run[k] = sp.run_order[k];
  return 0;
}

// Host-only view of the descriptors of the chain schedule (N x kDescWords int32, schedule order), for CPU tests of
// what the host marks in them (word 57: the granule hand-over).  Same graph as stereo_trws_spec_schedule.
extern "C" int stereo_trws_descriptors_host(int64_t N, int64_t E, const uint32_t *conn, int direction, int32_t *desc,
                                            char *err, size_t errcap) {
  if (!conn || !desc || (direction != 0 && direction != 1)) return stereo::fail("stereo_trws_descriptors_host: bad argument", err, errcap);
  try {
    stereo::TrwsGraph g;
    std::string gerr;
    if (!stereo::build_trws_graph(N, E, conn, stereo::TrwsGraphOptions(), g, gerr)) return stereo::fail(gerr, err, errcap);
    if (!g.fast_ok) return stereo::fail("stereo_trws_descriptors_host: graph outside the descriptor-driven kernels' range", err, errcap);
    std::copy(g.sweep[direction].desc.begin(), g.sweep[direction].desc.end(), desc);
  } catch (const std::exception &e) {
    return stereo::fail(std::string("stereo_trws_descriptors_host: ") + e.what(), err, errcap);
  }
  return 0;
}

// Host-only view of what one strip stores and of its renumbered descriptors (no device needed):
// lets a CPU test check that the ids a strip writes into its neighbours' arrays are the ids the
// neighbours use themselves.
extern "C" int stereo_trws_strip_layout_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner,
                                             int nstrips, int strip, int direction, int64_t *n_nodes, int64_t *n_own,
                                             int64_t *n_edges, int64_t *n_visits, int32_t *nodes, int32_t *edges,
                                             int32_t *desc, char *err, size_t errcap) {
  if (!conn || !owner || nstrips < 1 || strip < 0 || strip >= nstrips || (direction != 0 && direction != 1))
    return stereo::fail("stereo_trws_strip_layout_host: bad argument", err, errcap);
  if (nstrips < 2)  // (one strip is the plain plan: no owner table is kept for it)
    return stereo::fail("stereo_trws_strip_layout_host: a strip layout needs at least two strips", err, errcap);
  try {
    stereo::TrwsGraph g;
    std::string gerr;
    if (!stereo::build_trws_graph(N, E, conn, strips(owner, nstrips), g, gerr)) return stereo::fail(gerr, err, errcap);
    if (!g.fast_ok) return stereo::fail("stereo_trws_strip_layout_host: graph outside the descriptor-driven kernels' range", err, errcap);
    stereo::StripLayout L;
    if (!stereo::build_strip_layout(g, strip, L, gerr)) return stereo::fail(gerr, err, errcap);
    if (n_nodes) *n_nodes = (int64_t)L.nodes.size();
    if (n_own) *n_own = L.n_own;
    if (n_edges) *n_edges = (int64_t)L.edges.size();
    if (n_visits) *n_visits = (int64_t)(L.desc[direction].size() / stereo::TrwsGraph::kDescWords);
    if (nodes) std::copy(L.nodes.begin(), L.nodes.end(), nodes);
    if (edges) std::copy(L.edges.begin(), L.edges.end(), edges);
    if (desc) std::copy(L.desc[direction].begin(), L.desc[direction].end(), desc);
    return 0;
  } catch (const std::exception &e) {
    return stereo::fail(std::string("stereo_trws_strip_layout_host: ") + e.what(), err, errcap);
  }
}

// Host-only view of the lists the belief kernels walk on one strip (build_strip_belief_lists): own (n_own entries,
// strip-local node ids in rank order), fptr / bptr (n_own + 1), fidx / bidx (n_fwd / n_bwd strip-local edge ids).
// nstrips == 1: the whole problem (owner may be NULL).
extern "C" int stereo_trws_strip_belief_lists_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner,
                                                   int nstrips, int strip, int64_t *n_own, int64_t *n_fwd, int64_t *n_bwd,
                                                   int32_t *own, int32_t *fptr, int32_t *fidx, int32_t *bptr, int32_t *bidx,
                                                   char *err, size_t errcap) {
  if (!conn || nstrips < 1 || strip < 0 || strip >= nstrips || (nstrips > 1 && !owner))
    return stereo::fail("stereo_trws_strip_belief_lists_host: bad argument", err, errcap);
  try {
    stereo::TrwsGraph g;
    std::string gerr;
    if (!stereo::build_trws_graph(N, E, conn, strips(nstrips > 1 ? owner : nullptr, nstrips), g, gerr)) return stereo::fail(gerr, err, errcap);
    stereo::StripLayout L;
    if (nstrips > 1) {
      if (!g.fast_ok) return stereo::fail("stereo_trws_strip_belief_lists_host: graph outside the descriptor-driven kernels' range", err, errcap);
      if (!stereo::build_strip_layout(g, strip, L, gerr)) return stereo::fail(gerr, err, errcap);
    }
    stereo::StripBeliefLists B;
    if (!stereo::build_strip_belief_lists(g, strip, L.nodes, L.edges, B, gerr)) return stereo::fail(gerr, err, errcap);
    if (n_own) *n_own = (int64_t)B.own.size();
    if (n_fwd) *n_fwd = (int64_t)B.fidx.size();
    if (n_bwd) *n_bwd = (int64_t)B.bidx.size();
    if (own) std::copy(B.own.begin(), B.own.end(), own);
    if (fptr) std::copy(B.fptr.begin(), B.fptr.end(), fptr);
    if (fidx) std::copy(B.fidx.begin(), B.fidx.end(), fidx);
    if (bptr) std::copy(B.bptr.begin(), B.bptr.end(), bptr);
    if (bidx) std::copy(B.bidx.begin(), B.bidx.end(), bidx);
    return 0;
  } catch (const std::exception &e) {
    return stereo::fail(std::string("stereo_trws_strip_belief_lists_host: ") + e.what(), err, errcap);
  }
}

// Host-only views of the solver state's rules (trws_state.h): what a load refuses, and the edge rows a
// strip is authoritative for.
extern "C" int stereo_trws_state_check(const stereo_trws_state_header *header, int kernel, int K, int64_t N, int64_t E,
                                       const uint32_t *conn, int message_mode, char *why, size_t cap) {
  if (!header || (!conn && E > 0) || E < 0) return stereo::fail("stereo_trws_state_check: bad argument", why, cap);
  const std::string r = stereo::trws_state_refusal(*header, kernel, K, N, E, stereo::trws_connectivity_key(conn, E), message_mode);
  if (!r.empty()) return stereo::fail("stereo_trws_state_check: " + r, why, cap);
  if (why && cap) why[0] = 0;
  return 0;
}

extern "C" int stereo_trws_strip_state_rows_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner, int nstrips,
                                                 int strip, int phase, uint8_t *take) {
  if (!conn || !owner || !take || nstrips < 2 || strip < 0 || strip >= nstrips || (phase != 0 && phase != 1))
    return stereo::fail("stereo_trws_strip_state_rows_host: bad argument (strips have phases 0 and 1)", nullptr, 0);
  try {
    stereo::TrwsGraph g;
    std::string gerr;
    if (!stereo::build_trws_graph(N, E, conn, strips(owner, nstrips), g, gerr)) return stereo::fail(gerr, nullptr, 0);
    stereo::strip_state_rows(g, strip, phase, take);
    return 0;
  } catch (const std::exception &e) {
    return stereo::fail(std::string("stereo_trws_strip_state_rows_host: ") + e.what(), nullptr, 0);
  }
}

