// Host-side graph analysis for the TRW-S path: the reference's node order and lists, the rank-contiguous runs, and
// build_trws_graph's list of stages.  See trws_graph.h; file map in trws_plan.hip.
#include "trws_graph_stages.h"

#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <queue>
#include <thread>

namespace stereo {
namespace {

// Boundary set of the ordering heuristic (ordering.cpp:70-152).  The reference
// keeps a LIFO-prepended doubly linked list and scans it for the FIRST node of
// minimum remaining degree, which is O(|boundary|) per pick.  The same pick is
// "minimum degree, ties broken by most recent insertion": one max-heap of
// insertion stamps per degree value, with lazy invalidation.
class Boundary {
 public:
  explicit Boundary(int max_deg) : buckets_(max_deg + 1), cur_(max_deg + 1) {}
  void push(int deg, int64_t stamp, int32_t node) {
    buckets_[deg].emplace(stamp, node);
    if (deg < cur_) cur_ = deg;
  }
  // entry is current iff the node is still in the boundary with this degree/stamp
  template <class Valid>
  bool pop(Valid valid, int32_t &node) {
    const int nb = (int)buckets_.size();
    while (cur_ < nb) {
      auto &h = buckets_[cur_];
      while (!h.empty()) {
        auto top = h.top();
        h.pop();
        if (valid(top.second, cur_, top.first)) {
          node = top.second;
          return true;
        }
      }
      ++cur_;
    }
    return false;
  }

 private:
  std::vector<std::priority_queue<std::pair<int64_t, int32_t>>> buckets_;
  int cur_;
};

// the reference's per-node linked lists of forward / backward edges (by NODE), and the node degrees
struct Lists {
  std::vector<int32_t> firstF, firstB, nextF, nextB, deg;
};

// ---- stage: input checks; AddEdge: prepend to the tail's forward and the head's backward list
bool read_edges(int64_t N, int64_t E, const uint32_t *conn, const TrwsGraphOptions &opt, TrwsGraph &g, Lists &L, std::string &err) {
  if (N <= 0 || E < 0) { err = "build_trws_graph: empty problem"; return false; }
  if (N >= INT32_MAX || E >= INT32_MAX) { err = "build_trws_graph: more than 2^31 nodes/edges"; return false; }
  g = TrwsGraph();
  g.N = N; g.E = E;
  const int nstrips = opt.nstrips;
  if (nstrips < 1) { err = "build_trws_graph: nstrips must be >= 1"; return false; }
  if (nstrips > 1 && !opt.owner) { err = "build_trws_graph: strips need an owner per node"; return false; }
  g.nstrips = nstrips;
  if (nstrips > 1) {
    g.owner.assign(opt.owner, opt.owner + N);
    for (int64_t i = 0; i < N; ++i)
      if (g.owner[i] < 0 || g.owner[i] >= nstrips) { err = "build_trws_graph: owner out of range"; return false; }
  }
  const int32_t *own = nstrips > 1 ? g.owner.data() : nullptr;  // per node
  g.tail.resize(E); g.head.resize(E); g.mdir.assign(E, 0);
  L.firstF.assign(N, -1); L.firstB.assign(N, -1); L.nextF.resize(E); L.nextB.resize(E); L.deg.assign(N, 0);
  for (int64_t e = 0; e < E; ++e) {
    uint32_t a = conn[2 * e], b = conn[2 * e + 1];
    if (a >= (uint64_t)N || b >= (uint64_t)N) { err = "connectivity index out of range"; return false; }
    if (a == b) { err = "self loops are not supported"; return false; }
    if (own && std::abs(own[a] - own[b]) > 1) { err = "strips must form a chain: an edge joins strips that are not neighbours"; return false; }
    g.tail[e] = (int32_t)a; g.head[e] = (int32_t)b;
    L.nextF[e] = L.firstF[a]; L.firstF[a] = (int32_t)e;
    L.nextB[e] = L.firstB[b]; L.firstB[b] = (int32_t)e;
    ++L.deg[a]; ++L.deg[b];
  }
  return true;
}

// ---- stage: SetAutomaticOrdering (or, as a labelled option, the node index order).  Consumes L.deg.
bool order_nodes(TrwsGraph &g, Lists &L, int ordering, std::string &err) {
  const int64_t N = g.N;
  std::vector<int32_t> &deg = L.deg;
  g.order.resize(N); g.rank.assign(N, -1);
  if (ordering == 1) {
    for (int64_t i = 0; i < N; ++i) { g.order[i] = (int32_t)i; g.rank[i] = (int32_t)i; }
    return true;
  }
  const int max_deg = *std::max_element(deg.begin(), deg.end());
  std::vector<uint8_t> where(N, 2);  // 2 untouched list, 1 boundary, 0 ordered
  std::vector<int64_t> stamp(N, 0);
  // untouched nodes never change degree, so the outer "first node of minimum
  // degree in index order" is a cursor over nodes sorted by (degree, index)
  std::vector<int32_t> by_deg(N);
  std::iota(by_deg.begin(), by_deg.end(), 0);
  std::stable_sort(by_deg.begin(), by_deg.end(), [&](int32_t x, int32_t y) { return deg[x] < deg[y]; });
  int64_t cursor = 0, counter = 0, count = 0;
  Boundary bnd(max_deg);
  auto valid = [&](int32_t n, int d, int64_t s) { return where[n] == 1 && deg[n] == d && stamp[n] == s; };
  while (count < N) {
    while (cursor < N && where[by_deg[cursor]] != 2) ++cursor;
    if (cursor >= N) { err = "ordering: internal error"; return false; }
    int32_t seed = by_deg[cursor];
    where[seed] = 1; stamp[seed] = ++counter;
    bnd.push(deg[seed], stamp[seed], seed);
    int32_t i;
    while (bnd.pop(valid, i)) {
      where[i] = 0; g.rank[i] = (int32_t)count; g.order[count++] = i;
      for (int pass = 0; pass < 2; ++pass) {
        for (int32_t e = pass == 0 ? L.firstF[i] : L.firstB[i]; e >= 0; e = pass == 0 ? L.nextF[e] : L.nextB[e]) {
          int32_t j = pass == 0 ? g.head[e] : g.tail[e];
          if (where[j] == 0) continue;
          --deg[j];
          if (where[j] == 2) { where[j] = 1; stamp[j] = ++counter; }
          bnd.push(deg[j], stamp[j], j);
        }
      }
    }
  }
  return true;
}

// ---- stage: CompleteGraphConstruction: orient low -> high rank, rebuild lists
void orient_edges(TrwsGraph &g, Lists &L) {
  std::vector<int32_t> &firstF = L.firstF, &firstB = L.firstB, &nextF = L.nextF, &nextB = L.nextB;
  std::fill(firstB.begin(), firstB.end(), -1);
  for (int64_t r = 0; r < g.N; ++r) {
    int32_t i = g.order[r], eprev = -1;
    for (int32_t e = firstF[i]; e >= 0;) {
      int32_t j = g.head[e];
      if (g.rank[i] < g.rank[j]) {
        nextB[e] = firstB[j]; firstB[j] = e;
        eprev = e; e = nextF[e];
      } else {
        int32_t enext = nextF[e];
        g.mdir[e] ^= 1; g.tail[e] = j; g.head[e] = i;
        if (eprev >= 0) nextF[eprev] = enext; else firstF[i] = enext;
        nextF[e] = firstF[j]; firstF[j] = e;
        nextB[e] = firstB[i]; firstB[i] = e;
        e = enext;
      }
    }
  }
}

// ---- stage: flatten to CSR by rank, gamma, levels, lower-bound term positions
void flatten_lists(TrwsGraph &g, const Lists &L) {
  const int64_t N = g.N, E = g.E;
  const int32_t *own = g.nstrips > 1 ? g.owner.data() : nullptr;
  g.fptr.assign(N + 1, 0); g.bptr.assign(N + 1, 0);
  g.fidx.resize(E); g.bidx.resize(E); g.gamma.resize(N);
  int64_t pf = 0, pb = 0;
  std::vector<int32_t> level(N, 0);
  int32_t nlev = 0;
  for (int64_t r = 0; r < N; ++r) {
    int32_t i = g.order[r];
    g.fptr[r] = (int32_t)pf; g.bptr[r] = (int32_t)pb;
    for (int32_t e = L.firstF[i]; e >= 0; e = L.nextF[e]) g.fidx[pf++] = e;
    int32_t lv = 0;
    for (int32_t e = L.firstB[i]; e >= 0; e = L.nextB[e]) {
      g.bidx[pb++] = e;
      lv = std::max(lv, level[g.rank[g.tail[e]]] + 1);
    }
    level[r] = lv; nlev = std::max(nlev, lv + 1);
    int nf = (int)(pf - g.fptr[r]), nbk = (int)(pb - g.bptr[r]);
    int ni = std::max(nf, nbk);
    g.gamma[r] = ni > 0 ? (double)1 / ni : 1.0;  // isolated node: no edge ever reads gamma
  }
  g.fptr[N] = (int32_t)pf; g.bptr[N] = (int32_t)pb;
  g.level_ptr.assign(nlev + 1, 0);
  for (int64_t r = 0; r < N; ++r) ++g.level_ptr[level[r] + 1];
  for (int32_t l = 0; l < nlev; ++l) {
    g.max_level_nodes = std::max<int64_t>(g.max_level_nodes, g.level_ptr[l + 1]);
    g.level_ptr[l + 1] += g.level_ptr[l];
  }
  g.level_ranks.resize(N);
  {
    std::vector<int32_t> fill(g.level_ptr.begin(), g.level_ptr.end() - 1);
    for (int64_t r = 0; r < N; ++r) g.level_ranks[fill[level[r]]++] = (int32_t)r;
  }
  g.lb_pos_node.resize(N); g.lb_pos_edge.assign(E, -1);
  g.strip_lb_terms.assign(g.nstrips, 0); g.strip_nodes.assign(g.nstrips, 0); g.e_pos.resize(N);
  for (int64_t r = N - 1; r >= 0; --r) {
    int64_t &pos = g.strip_lb_terms[own ? own[g.order[r]] : 0];  // the node that computes a term owns it
    g.lb_pos_node[r] = (int32_t)pos++;
    for (int32_t k = g.bptr[r]; k < g.bptr[r + 1]; ++k) g.lb_pos_edge[g.bidx[k]] = (int32_t)pos++;
  }
  for (int64_t r = 0; r < N; ++r) g.e_pos[r] = (int32_t)g.strip_nodes[own ? own[g.order[r]] : 0]++;
  g.lb_terms = 0;
  for (int64_t v : g.strip_lb_terms) g.lb_terms = std::max(g.lb_terms, v);
  if (g.nstrips == 1) g.lb_terms = g.strip_lb_terms[0];
}

// Dispense the rank-contiguous runs by the level of their first node; keep the order only if every foreign
// dependency then lies in a run dispensed earlier (otherwise workgroups could all be waiting for a run nobody
// has picked up yet).
void order_contiguous_runs(const DirView &v, TrwsGraph::Sweep &S, const std::vector<int32_t> &lev) {
  const int64_t N = v.N, R = (int64_t)S.run_ptr.size() - 1;
  std::vector<int32_t> order(R);
  for (int64_t k = 0; k < R; ++k) order[k] = (int32_t)k;
  auto first_lev = [&](int32_t k) { return lev[v.rank_at(S.run_ptr[k])]; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return first_lev(x) < first_lev(y); });
  std::vector<int32_t> ticket_of_run(R), run_of_pos(N);
  for (int64_t t = 0; t < R; ++t) ticket_of_run[order[t]] = (int32_t)t;
  for (int64_t k = 0; k < R; ++k)
    for (int64_t p = S.run_ptr[k]; p < S.run_ptr[k + 1]; ++p) run_of_pos[p] = (int32_t)k;
  for (int64_t r = 0; r < N; ++r) {
    const int32_t mine = run_of_pos[v.position((int32_t)r)];
    for (int32_t q = S.dep_ptr[r]; q < S.dep_ptr[r + 1]; ++q) {
      const int32_t theirs = run_of_pos[v.position(S.dep_rank[q])];
      if (theirs != mine && ticket_of_run[theirs] > ticket_of_run[mine]) return;
    }
  }
  S.run_order = order;
}

// ---- stage: rank-contiguous runs, what the generic and large kernels walk (Sweep::run_ptr .. in_slot)
// cut == false: a run ends only where the node does not hang on one of the two previous
// visits.  cut == true (used when there are more runs than resident workgroups): a run also
// ends in front of a node whose dependency level jumps (it will wait long for a foreign
// node -- e.g. the last node of a grid row waits for the border chain -- and would pin a
// workgroup meanwhile), and runs are dispensed by the level of their first node.
void contiguous_runs(const DirView &v, TrwsGraph::Sweep &S, bool cut) {
  const int64_t N = v.N;
  S.run_ptr.clear(); S.dep_ptr.assign(N + 1, 0); S.dep_rank.clear(); S.in_slot.assign(v.g.E, -1);
  S.run_order.clear();
  std::vector<std::vector<int32_t>> tmp_deps(N);  // filled per rank in processing order
  std::vector<int32_t> lev(N, 0);  // dependency level within this sweep direction
  constexpr int32_t kJump = 8;
  int64_t run_start = 0;
  for (int64_t p = 0; p < N; ++p) {
    const int32_t r = v.rank_at(p);
    // ranks visited one and two steps earlier (hand-over through LDS is kept for two visits); 0: not in this run
    auto dist_to = [&](int32_t other) {
      if (v.own && v.strip_of(other) != v.strip_of(r)) return 0;
      if (p - 1 >= run_start && other == v.rank_at(p - 1)) return 1;
      if (p - 2 >= run_start && other == v.rank_at(p - 2)) return 2;
      return 0;
    };
    // pass 1: does this node hang on one of the last two visits of the current run?
    bool chained = false;
    int32_t lv = 0;
    for (int32_t k = v.iptr[r]; k < v.iptr[r + 1]; ++k) {
      const int32_t other = v.other_end(v.iidx[k]);
      if (dist_to(other)) chained = true;
      lv = std::max(lv, lev[other] + 1);
    }
    lev[r] = lv;
    if (cut && chained && p >= 1 && lv > lev[v.rank_at(p - 1)] + kJump) chained = false;
    if (!chained) { S.run_ptr.push_back((int32_t)p); run_start = p; }
    std::vector<int32_t> &deps = tmp_deps[r];
    for (int32_t k = v.iptr[r]; k < v.iptr[r + 1]; ++k) {
      const int32_t e = v.iidx[k], other = v.other_end(e);
      if (const int dist = dist_to(other)) {
        // in_slot = slot in that node's outgoing list + 8 * (dist - 1)
        const int slot = v.slot_in(other, e);
        if (slot >= 0) S.in_slot[k] = (int8_t)(slot + 8 * (dist - 1));
      } else if (std::find(deps.begin(), deps.end(), other) == deps.end()) {
        deps.push_back(other);
      }
    }
  }
  S.run_ptr.push_back((int32_t)N);
  int64_t dp = 0;
  for (int64_t r = 0; r < N; ++r) {
    S.dep_ptr[r] = (int32_t)dp;
    for (int32_t x : tmp_deps[r]) { S.dep_rank.push_back(x); ++dp; }
  }
  S.dep_ptr[N] = (int32_t)dp;
  if (cut) order_contiguous_runs(v, S, lev);
}

// The rank-contiguous runs of one direction, cut where there are more of them than resident workgroups.  Returns
// whether there are: the chain schedule is then cut by the same rule.
bool choose_contiguous_runs(TrwsGraph &g, int d, int64_t max_resident_runs) {
  const DirView v(g, d);
  TrwsGraph::Sweep &S = g.sweep[d];
  contiguous_runs(v, S, false);
  auto too_many = [&] { return max_resident_runs > 0 && (int64_t)S.run_ptr.size() - 1 > max_resident_runs; };
  if (too_many()) {
    contiguous_runs(v, S, true);
    // a cut turns the hand-over from the previous visit into a foreign dependency; the fast
    // kernels take at most four per node
    bool ok = true;
    for (int64_t r = 0; r < g.N && ok; ++r) ok = S.dep_ptr[r + 1] - S.dep_ptr[r] <= kMaxDeps;
    if (!ok) contiguous_runs(v, S, false);
  }
  S.run_strip.clear();
  if (v.own)
    for (size_t k = 0; k + 1 < S.run_ptr.size(); ++k) S.run_strip.push_back(v.strip_of(v.rank_at(S.run_ptr[k])));
  return too_many();
}

// every node has <= 8 incident edges and <= 4 foreign dependencies per direction
bool within_descriptor_range(const TrwsGraph &g) {
  for (int64_t r = 0; r < g.N; ++r) {
    if ((g.fptr[r + 1] - g.fptr[r]) + (g.bptr[r + 1] - g.bptr[r]) > TrwsGraph::kMaxSlots) return false;
    for (int d = 0; d < 2; ++d)
      if (g.sweep[d].dep_ptr[r + 1] - g.sweep[d].dep_ptr[r] > kMaxDeps) return false;
  }
  return true;
}

// ---- the descriptor-driven kernels' schedules of one direction, stage by stage.  Returns whether the loader protocol
// terminates on the chain schedule.
bool build_direction(TrwsGraph &g, int d, const TrwsGraphOptions &opt, bool cut, int seg_len) {
  StageClock clock(d == 0 && std::getenv("STEREO_HIP_GRAPH_VERBOSE"));
  const DirView v(g, d);
  TrwsGraph::Sweep &S = g.sweep[d];
  // (the look-ahead rule is checked whenever there are more runs than CUs: one workgroup per CU is all that is certain
  // to be resident, whatever max_resident_runs the caller derived from its kernel's LDS use)
  const int64_t resident =
      opt.max_resident_runs > 0 ? std::min(opt.max_resident_runs, std::max<int64_t>(opt.certainly_resident, 1)) : 0;
  RunSet runs = chain_schedule(v, S, cut, resident, clock);
  S.chain_run_ptr = runs.run_ptr; S.chain_run_order = runs.run_order;   // (per run, not per node)
  Finished fin = finish_schedule(v, runs, resident, false, seg_len, clock);
  S.desc = std::move(fin.desc); S.chain_run_strip = std::move(fin.run_strip); S.spec = std::move(fin.spec);
  // ---- sub-row runs (trws_graph.h: Sweep::Chunked).  Kept only if everything the chain schedule is checked for holds
  // with chunk_resident workgroups; otherwise the direction keeps whole rows.
  S.chunked = TrwsGraph::Sweep::Chunked();
  const int64_t row_chunk = d == 1 && opt.row_chunk_backward >= 0 ? opt.row_chunk_backward : opt.row_chunk_forward;
  const int64_t chunk_resident = std::max<int64_t>(opt.chunk_resident, 1);
  const bool wanted = row_chunk > 0 && runs.chain && !v.own && fin.terminates && runs.runs() > chunk_resident;
  const std::optional<RunSet> pieces =
      wanted ? sub_row_runs(v, std::move(runs), S.spec.ok ? S.spec.run : -1, row_chunk) : std::nullopt;
  if (pieces) {
    Finished sub = finish_schedule(v, *pieces, chunk_resident, true, seg_len, clock);
    // (one speculative schedule serves both sets of runs: the plan's buffers are sized by it)
    const TrwsGraph::Sweep::Spec &a = S.spec, &b = sub.spec;
    if (sub.terminates && (!a.ok || (b.ok && b.c0 == a.c0 && b.c1 == a.c1 && b.nseg == a.nseg))) {
      TrwsGraph::Sweep::Chunked &C = S.chunked;
      C.ok = true; C.chunk = (int32_t)row_chunk;
      C.desc = std::move(sub.desc); C.run_ptr = pieces->run_ptr; C.run_order = pieces->run_order;
      if (a.ok) C.spec = std::move(sub.spec);
    }
  }
  return fin.terminates;
}

}  // namespace

int spec_segment_length() {
  int L = 16;
  if (const char *e = std::getenv("STEREO_HIP_TRWS_SPEC_SEG")) L = std::atoi(e);
  return std::max(4, std::min(L, 48));
}

bool build_trws_graph(int64_t N, int64_t E, const uint32_t *conn, const TrwsGraphOptions &opt, TrwsGraph &g, std::string &err) {
  StageClock clock(std::getenv("STEREO_HIP_GRAPH_VERBOSE"));
  {
    Lists lists;
    if (!read_edges(N, E, conn, opt, g, lists, err)) return false;
    clock.done("edges");
    if (!order_nodes(g, lists, opt.ordering, err)) return false;
    clock.done("node order");
    orient_edges(g, lists);
    clock.done("orientation");
    flatten_lists(g, lists);
    clock.done("lists, levels, lower-bound positions");
  }
  bool cut[2];
  for (int d = 0; d < 2; ++d) cut[d] = choose_contiguous_runs(g, d, opt.max_resident_runs);
  clock.done("rank-contiguous runs");
  g.fast_ok = within_descriptor_range(g);
  if (g.fast_ok) {
    const int seg_len = opt.seg_len > 0 ? opt.seg_len : spec_segment_length();
    // the two sweep directions are independent of each other: one host thread each
    bool protocol_ok[2] = {true, true};
    std::thread backward([&] { protocol_ok[1] = build_direction(g, 1, opt, cut[1], seg_len); });
    protocol_ok[0] = build_direction(g, 0, opt, cut[0], seg_len);
    backward.join();
    if (!protocol_ok[0] || !protocol_ok[1]) {
      // a schedule the host cannot show to terminate is never launched: the generic kernel takes the graph
      g.fast_ok = false;
      for (int d = 0; d < 2; ++d) {
        TrwsGraph::Sweep &S = g.sweep[d];
        S.desc = std::vector<int32_t>(); S.chain_rank.clear(); S.chain_run_ptr.clear(); S.chain_run_order.clear();
        S.chain_run_strip.clear(); S.spec = TrwsGraph::Sweep::Spec(); S.chunked = TrwsGraph::Sweep::Chunked();
      }
    }
  }
  clock.done("end");
  return true;
}

}  // namespace stereo
