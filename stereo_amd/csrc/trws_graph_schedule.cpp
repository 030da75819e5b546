// Host-side graph analysis for the TRW-S path: which runs the descriptor-driven kernels walk in one direction -- the
// chain schedule, its rank-contiguous fallback, the sub-row runs -- and in which order workgroups draw them.
// See trws_graph.h; file map in trws_plan.hip.
#include "trws_graph_stages.h"

#include <algorithm>
#include <set>

namespace stereo {

bool look_ahead_ok(const std::vector<int32_t> &order, const std::vector<int32_t> &strip_of_run, int nstrips,
                   const std::vector<int32_t> &run_of, const std::vector<Deps> &deps) {
  const int64_t R = (int64_t)order.size();
  std::vector<int32_t> ticket_of_run(R), seen(nstrips, 0);
  for (int64_t t = 0; t < R; ++t) ticket_of_run[order[t]] = seen[strip_of_run[order[t]]]++;
  std::vector<std::vector<int32_t>> ahead(nstrips);  // per strip and ticket: farthest ticket it waits for, minus its own
  for (int s = 0; s < nstrips; ++s) ahead[s].assign(seen[s], 0);
  for (size_t r = 0; r < deps.size(); ++r)
    for (int32_t x : deps[r]) {
      const int32_t rm = run_of[r], rt = run_of[x];
      if (strip_of_run[rm] != strip_of_run[rt]) continue;
      const int32_t mine = ticket_of_run[rm], theirs = ticket_of_run[rt];
      ahead[strip_of_run[rm]][mine] = std::max(ahead[strip_of_run[rm]][mine], theirs - mine);
    }
  for (const auto &a : ahead)
    for (size_t t = 0; t < a.size(); ++t)
      if (a[t] > 1 || (a[t] == 1 && t + 1 < a.size() && a[t + 1] > 0)) return false;
  return true;
}

namespace {

// the chain runs as linked paths: by rank run_of / pred / next_of, by run run_head / first_lev
struct ChainRuns {
  std::vector<int32_t> run_of, pred, next_of, run_head, first_lev;
};

// ---- stage: chain runs.  A node extends the run of the node visited two steps or one step
// earlier if it depends on it and that node is still the last one of its run; two steps
// first, which is what separates two interleaved rows (s0 s1 s2 s3 ...: s3 hangs on s1 AND
// on s2, s4 only on s2) into the runs s0 s1 s3 s5 ... and s2 s4 s6 ...
// cut: a run also ends in front of a node whose dependency level jumps (contiguous_runs, trws_graph.cpp).
ChainRuns chain_runs(const DirView &v, bool cut) {
  const int64_t N = v.N;
  ChainRuns c;
  c.run_of.assign(N, -1); c.pred.assign(N, -1); c.next_of.assign(N, -1);
  std::vector<int32_t> lev(N, 0), run_tail;
  constexpr int32_t kJump = 8;
  for (int64_t p = 0; p < N; ++p) {
    const int32_t r = v.rank_at(p);
    int32_t lv = 0, best = -1;
    for (int32_t k = v.iptr[r]; k < v.iptr[r + 1]; ++k) {
      const int32_t o = v.other_end(v.iidx[k]);
      lv = std::max(lv, lev[o] + 1);
      const int64_t back = p - v.position(o);
      if ((back != 1 && back != 2) || run_tail[c.run_of[o]] != o) continue;
      if (v.own && v.strip_of(o) != v.strip_of(r)) continue;  // a run stays inside one strip
      if (best < 0 || v.position(o) < v.position(best)) best = o;
    }
    lev[r] = lv;
    if (cut && best >= 0 && lv > lev[best] + kJump) best = -1;
    if (best >= 0) {
      c.run_of[r] = c.run_of[best]; c.next_of[best] = r; run_tail[c.run_of[r]] = r; c.pred[r] = best;
    } else {
      c.run_of[r] = (int32_t)c.run_head.size(); c.run_head.push_back(r); run_tail.push_back(r); c.first_lev.push_back(lv);
    }
  }
  return c;
}

// ---- stage: foreign dependencies per rank (everything but the predecessor in the run); false: a node has more
// than the descriptor holds (deps is then incomplete)
bool foreign_deps(const DirView &v, const std::vector<int32_t> &pred, std::vector<Deps> &deps) {
  deps.assign(v.N, Deps());
  for (int64_t r = 0; r < v.N; ++r) {
    for (int32_t k = v.iptr[r]; k < v.iptr[r + 1]; ++k) {
      const int32_t o = v.other_end(v.iidx[k]);
      if (o != pred[r] && std::find(deps[r].begin(), deps[r].end(), o) == deps[r].end()) deps[r].push_back(o);
    }
    if (deps[r].size() > (size_t)kMaxDeps) return false;
  }
  return true;
}

// ---- stage: ticket order.  Runs are numbered by the position of their first node; a dependency can
// then live in a run with a LARGER number (the two interleaved rows need each other).  That
// is harmless while every run has its own resident workgroup.  With fewer workgroups than
// runs it must be shown that waiting never blocks the dispenser: the look-ahead rule.
// With strips every strip has its own dispenser and its own (smaller) set of workgroups: the
// tickets that count are the positions among the strip's OWN runs, a dependency in another
// strip's run is served by that strip's workgroups, and the test is made whatever the run count
// (a strip may be launched with fewer workgroups than it has runs: logical strips that share a
// device, max_workgroups, a partitioned GPU).
// false: no order passes the rule.
bool ticket_order(const DirView &v, const ChainRuns &c, const std::vector<Deps> &deps, bool cut, int64_t resident,
                  std::vector<int32_t> &order) {
  const int64_t R = (int64_t)c.run_head.size();
  order.resize(R);
  for (int64_t k = 0; k < R; ++k) order[k] = (int32_t)k;
  if (cut) std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return c.first_lev[x] < c.first_lev[y]; });
  if (!((resident > 0 && R > resident) || v.g.nstrips > 1)) return true;
  std::vector<int32_t> strip_of_run(R, 0);
  if (v.own) for (int64_t k = 0; k < R; ++k) strip_of_run[k] = v.strip_of(c.run_head[k]);
  if (look_ahead_ok(order, strip_of_run, v.g.nstrips, c.run_of, deps)) return true;
  if (!cut) return false;
  for (int64_t k = 0; k < R; ++k) order[k] = (int32_t)k;  // try creation order before giving up
  return look_ahead_ok(order, strip_of_run, v.g.nstrips, c.run_of, deps);
}

// the chain runs laid out run after run
RunSet chain_run_set(ChainRuns &&c, std::vector<Deps> &&deps, const std::vector<int32_t> &order, std::vector<int32_t> &chain_rank) {
  const int64_t R = (int64_t)c.run_head.size();
  RunSet s(chain_rank);
  s.chain = true;
  chain_rank.clear();
  for (int64_t k = 0; k < R; ++k) {
    s.run_ptr.push_back((int32_t)chain_rank.size());
    for (int32_t r = c.run_head[k]; r >= 0; r = c.next_of[r]) chain_rank.push_back(r);
  }
  s.run_ptr.push_back((int32_t)chain_rank.size());
  bool identity = true;
  for (int64_t k = 0; k < R; ++k) identity = identity && order[k] == (int32_t)k;
  if (!identity) s.run_order = order;
  s.pred2.assign(c.pred.size(), -1);   // (a chain hands over from the previous visit only)
  s.pred = std::move(c.pred); s.deps = std::move(deps);
  return s;
}

// the rank-contiguous runs of contiguous_runs (hand-over from one or two visits back)
RunSet contiguous_run_set(const DirView &v, TrwsGraph::Sweep &S) {
  const int64_t N = v.N;
  RunSet s(S.chain_rank);
  S.chain_rank.resize(N);
  for (int64_t p = 0; p < N; ++p) S.chain_rank[p] = v.rank_at(p);
  s.run_ptr = S.run_ptr; s.run_order = S.run_order;
  s.pred.assign(N, -1); s.pred2.assign(N, -1); s.deps.assign(N, Deps());
  for (int64_t r = 0; r < N; ++r) s.deps[r].assign(S.dep_rank.data() + S.dep_ptr[r], S.dep_rank.data() + S.dep_ptr[r + 1]);
  for (int64_t k = 0; k < s.runs(); ++k)
    for (int64_t p = s.run_ptr[k]; p < s.run_ptr[k + 1]; ++p) {
      if (p - 1 >= s.run_ptr[k]) s.pred[s.chain_rank[p]] = s.chain_rank[p - 1];
      if (p - 2 >= s.run_ptr[k]) s.pred2[s.chain_rank[p]] = s.chain_rank[p - 2];
    }
  return s;
}

}  // namespace

RunSet chain_schedule(const DirView &v, TrwsGraph::Sweep &S, bool cut, int64_t resident, StageClock &clock) {
  ChainRuns c = chain_runs(v, cut);
  clock.done("dir0 chain runs");
  std::vector<Deps> deps;
  std::vector<int32_t> order;
  bool ok = foreign_deps(v, c.pred, deps);
  clock.done("dir0 dependencies");
  ok = ok && ticket_order(v, c, deps, cut, resident, order);
  RunSet runs = ok ? chain_run_set(std::move(c), std::move(deps), order, S.chain_rank) : contiguous_run_set(v, S);
  clock.done("dir0 tickets");
  return runs;
}

namespace {

// Sub-row runs while their tickets are being dealt: where the pieces start, and the runs that makes.
struct Pieces {
  std::vector<uint8_t> starts;                 // by position: a run starts here
  std::vector<int32_t> pos_of;                 // by rank
  std::vector<int32_t> run_at;                 // by position
  std::vector<int32_t> run_ptr, run_order, first_ready;
  std::vector<int32_t> ready_at, done_at;      // by rank, in quarter visits (lay_out_pieces)
};

// what the node at position q waits for: its foreign dependencies, and at the start of a piece its predecessor
template <class F>
void each_wait(const RunSet &chain, const Pieces &P, int64_t q, F &&f) {
  const int32_t r = chain.chain_rank[q];
  for (int32_t x : chain.deps[r]) f(x);
  if (P.starts[q] && chain.pred[r] >= 0) f(chain.pred[r]);
}

// When a node can start, in quarter visits: a visit takes 4, one of the speculative schedule's runner 1, and
// a row from another run arrives 3 behind the end of the visit that made it (row lag = hand-over + visit,
// DESIGN.md 4.4) -- the dependency level counts every hop as one visit, and would draw the first pieces of
// all rows before the second piece of the first.  Then the runs the starts make, each with the time of its first node.
void lay_out_pieces(const DirView &v, const RunSet &chain, int32_t whole, Pieces &P) {
  const int64_t N = v.N;
  std::vector<int32_t> &ready_at = P.ready_at, &done_at = P.done_at;
  for (int64_t pp = 0; pp < N; ++pp) {
    const int32_t r = v.rank_at(pp);
    const int64_t q = P.pos_of[r];
    int32_t t = 0;
    for (int32_t x : chain.deps[r]) t = std::max(t, done_at[x] + 3);
    if (chain.pred[r] >= 0) t = std::max(t, done_at[chain.pred[r]] + (P.starts[q] ? 3 : 0));
    ready_at[r] = t;
    done_at[r] = t + (whole >= 0 && q >= chain.run_ptr[whole] && q < chain.run_ptr[whole + 1] ? 1 : 4);
  }
  P.run_ptr.clear(); P.run_order.clear(); P.first_ready.clear();
  for (int64_t q = 0; q < N; ++q) {
    if (P.starts[q]) { P.run_ptr.push_back((int32_t)q); P.first_ready.push_back(ready_at[chain.chain_rank[q]]); }
    P.run_at[q] = (int32_t)P.run_ptr.size() - 1;
  }
  P.run_ptr.push_back((int32_t)N);
}

// Tickets: of the runs whose producers all have theirs, the one whose first node can start first (then the
// earliest position).  Where two runs wait for each other (the first pieces of the two interleaved rows) no run is
// ready: returns the position in front of which the lowest run left must be cut once more -- its first node that
// waits for a run without a ticket -- or -2 if there is no such cut; -1: every run has its ticket.
int64_t deal_tickets(const RunSet &chain, Pieces &P) {
  const int64_t N = (int64_t)chain.chain_rank.size(), RC = (int64_t)P.run_ptr.size() - 1;
  std::vector<std::vector<int32_t>> feeds(RC);
  std::vector<int32_t> waits(RC, 0);
  std::vector<uint8_t> drawn(RC, 0);
  for (int64_t q = 0; q < N; ++q)
    each_wait(chain, P, q, [&](int32_t x) {
      const int32_t kx = P.run_at[P.pos_of[x]], kq = P.run_at[q];
      if (kx != kq) { feeds[kx].push_back(kq); ++waits[kq]; }
    });
  typedef std::pair<int32_t, int32_t> Key;   // (start of the first node, run)
  std::set<Key> ready, left;
  for (int64_t k = 0; k < RC; ++k) {
    left.insert(Key(P.first_ready[k], (int32_t)k));
    if (!waits[k]) ready.insert(Key(P.first_ready[k], (int32_t)k));
  }
  while (!left.empty()) {
    if (ready.empty()) {
      const int32_t k = left.begin()->second;
      int64_t q = P.run_ptr[k];
      for (; q < P.run_ptr[k + 1]; ++q) {
        bool served = true;
        each_wait(chain, P, q, [&](int32_t x) { const int32_t kx = P.run_at[P.pos_of[x]]; served = served && (kx == k || drawn[kx]); });
        if (!served) break;
      }
      return q == P.run_ptr[k] || q == P.run_ptr[k + 1] ? -2 : q;
    }
    const Key top = *ready.begin();
    ready.erase(top); left.erase(top);
    drawn[top.second] = 1;
    P.run_order.push_back(top.second);
    for (int32_t k : feeds[top.second])
      if (--waits[k] == 0) ready.insert(Key(P.first_ready[k], k));
  }
  return -1;
}

}  // namespace

// ---- stage: sub-row runs (trws_graph.h: Sweep::Chunked): the same positions, every ordinary run longer than row_chunk cut
// into consecutive runs of at most row_chunk positions.  The first node of such a run has no predecessor in LDS
// any more: the last node of the run in front becomes one more foreign dependency, its rows come from memory (or
// as granules).  Tickets follow the wavefront: a linear extension of the runs' dependencies that prefers the
// run whose first node can start first.
std::optional<RunSet> sub_row_runs(const DirView &v, RunSet chain, int32_t whole, int64_t row_chunk) {
  const int64_t N = v.N;
  Pieces P;
  P.starts.assign(N + 1, 0); P.pos_of.resize(N); P.run_at.resize(N); P.ready_at.resize(N); P.done_at.resize(N);
  for (int64_t q = 0; q < N; ++q) P.pos_of[chain.chain_rank[q]] = (int32_t)q;
  for (int64_t k = 0; k < chain.runs(); ++k) {
    const int64_t a = chain.run_ptr[k], b = chain.run_ptr[k + 1];
    for (int64_t at = a; at < b; at += k == whole ? b - a : row_chunk) P.starts[at] = 1;
  }
  // deal the tickets; where no run is ready, cut once more and deal again.  No such cut: whole rows.
  for (int round = 0;; ++round) {
    lay_out_pieces(v, chain, whole, P);
    const int64_t q = deal_tickets(chain, P);
    if (q == -1) break;
    if (q < 0 || round >= 64) return std::nullopt;
    P.starts[q] = 1;
  }
  // a piece's first node: the node in front is one more foreign dependency (the fast kernels take four)
  bool any = false;
  std::vector<int32_t> run_of(N);
  for (int64_t q = 0; q < N; ++q) {
    const int32_t r = chain.chain_rank[q];
    run_of[r] = P.run_at[q];
    if (!P.starts[q] || chain.pred[r] < 0) continue;
    if (chain.deps[r].size() >= (size_t)kMaxDeps) return std::nullopt;
    chain.deps[r].push_back(chain.pred[r]); chain.pred[r] = -1; any = true;
  }
  if (!any) return std::nullopt;
  // the look-ahead rule of the chain schedule's tickets, on these (a linear extension looks ahead to nobody)
  if (!look_ahead_ok(P.run_order, std::vector<int32_t>(P.run_order.size(), 0), 1, run_of, chain.deps)) return std::nullopt;
  chain.run_ptr = std::move(P.run_ptr); chain.run_order = std::move(P.run_order);
  return chain;
}

}  // namespace stereo
