// Host-side graph analysis for the TRW-S path: what follows from a RunSet -- the descriptors, the proof that the loader
// protocol terminates, lazy flags, the speculative schedule and the granule marks.  Written once, for the chain
// schedule and for its sub-row runs alike.  See trws_graph.h; file map in trws_plan.hip.
#include "trws_graph_stages.h"

#include <algorithm>
#include <thread>

namespace stereo {
namespace {

constexpr int W = TrwsGraph::kDescWords;

// word 43: which outgoing messages (and whose copy of the flag / label) live in a neighbouring strip's memory
uint32_t remote_word(const DirView &v, int32_t r, int nout) {
  uint32_t remote = 0;
  if (!v.own) return remote;
  const int32_t mine = v.strip_of(r);
  for (int k = 0; k < nout && k < 8; ++k) {
    const int32_t theirs = v.own[v.far_node(v.oidx[v.optr[r] + k])];
    if (theirs == mine) continue;
    remote |= 1u << k;
    if (theirs > mine) remote |= (1u << (8 + k)) | (1u << 17); else remote |= 1u << 16;
  }
  return remote;
}

// word 56, twins: outgoing messages k and k' that go to the SAME neighbour (the reference's neighbourhood holds every
// pair of pixels as two directed edges, dispmap_super.m:279-302, and the orientation step turns both the same
// way): nibble k = k' (k itself without a twin).  Pairs only, mutual; what makes twins carry the same
// message -- equal weights, shared positions, equal old messages -- is the kernel's to check at run time.
uint32_t twin_word(const DirView &v, int32_t r, int nout) {
  int tw[8];
  for (int k = 0; k < 8; ++k) tw[k] = k;
  for (int k = 0; k < nout && k < 8; ++k) {
    if (tw[k] != k) continue;
    const int32_t to_k = v.far_node(v.oidx[v.optr[r] + k]);
    for (int k2 = k + 1; k2 < nout && k2 < 8; ++k2)
      if (tw[k2] == k2 && v.far_node(v.oidx[v.optr[r] + k2]) == to_k) { tw[k] = k2; tw[k2] = k; break; }
  }
  uint32_t twin = 0;
  for (int k = 0; k < 8; ++k) twin |= (uint32_t)tw[k] << (4 * k);
  return twin;
}

// the descriptor of the visit at schedule position p (layout: trws_graph.h)
void describe_visit(const DirView &v, const RunSet &runs, int64_t p, int32_t *D) {
  const TrwsGraph &g = v.g;
  const int32_t r = runs.chain_rank[p];
  const int nout = v.optr[r + 1] - v.optr[r], nin = v.iptr[r + 1] - v.iptr[r];
  const Deps &deps = runs.deps[r];
  const int nd = (int)deps.size();
  const int32_t pm = runs.pred[r], pm2 = runs.pred2[r];
  uint32_t md = 0, fetch = 0, pk[2] = {0, 0};
  for (int k = 0; k < 8; ++k) {
    int32_t e = 0, slot = -1, lbe = 0, xn = 0;
    if (k < nout) {
      e = v.oidx[v.optr[r] + k];
      lbe = g.lb_pos_edge[e];
    } else if (k < nout + nin) {
      e = v.iidx[v.iptr[r] + (k - nout)];
      // slot of the edge in the outgoing list of the node visited one (0..7) or two (8..15) steps earlier
      const int32_t o = v.other_end(e);
      const int dist = (pm >= 0 && o == pm) ? 1 : (pm2 >= 0 && o == pm2) ? 2 : 0;
      const int s = dist ? v.slot_in(o, e) : -1;
      if (s >= 0) slot = s + 8 * (dist - 1);
      xn = v.other_node(e);  // the other endpoint: its label feeds the primal
      if (slot < 0) fetch |= 1u << k;
    }
    if (k < nout + nin && g.mdir[e]) md |= 1u << k;
    D[kDescEdge + k] = e; D[kDescSlot + k] = slot; D[kDescLbEdge + k] = lbe; D[kDescOther + k] = xn;
    // slots once more, one byte each (0xff = none), for the compute waves
    pk[k >> 2] |= (uint32_t)(uint8_t)(int8_t)slot << (8 * (k & 3));
  }
  D[kDescNode] = g.order[r];
  D[kDescRank] = r;
  // bit 12: a loader may wait for this node's foreign dependencies while the node two visits
  // earlier in the run is still being computed (its result only becomes visible one visit
  // later): true if every dependency comes before that node in this sweep's order -- what is
  // waited for can then not depend on anything this workgroup still holds back.  False where
  // two chains feed each other (the interleaved last rows).
  const int32_t before = pm >= 0 ? runs.pred[pm] : -1;
  const int32_t bound = before >= 0 ? before : pm >= 0 ? pm : r;
  bool ahead = true;
  for (int k = 0; k < nd; ++k) ahead = ahead && (v.d == 0 ? deps[k] < bound : deps[k] > bound);
  D[kDescCounts] = desc_pack(nout, nin, nd, ahead, md);
  D[kDescLbNode] = g.lb_pos_node[r];
  for (int k = 0; k < kMaxDeps; ++k) D[kDescDep + k] = k < nd ? deps[k] : 0;
  D[kDescRemote] = (int32_t)remote_word(v, r, nout);
  D[kDescEpos] = g.e_pos[r];
  D[kDescSlotBytes] = (int32_t)pk[0]; D[kDescSlotBytes + 1] = (int32_t)pk[1];
  D[kDescFetch] = (int32_t)fetch;
  D[kDescTwin] = (int32_t)twin_word(v, r, nout);
}

// ---- stage: descriptors, in schedule order (every position is independent of the others: host threads)
void describe_visits(const DirView &v, const RunSet &runs, std::vector<int32_t> &desc) {
  const int64_t N = v.N;
  auto describe = [&](int64_t pa, int64_t pb) {
    for (int64_t p = pa; p < pb; ++p) describe_visit(v, runs, p, &desc[(size_t)p * W]);
  };
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int64_t T = std::max<int64_t>(1, std::min<int64_t>({(int64_t)hw / 2, 32, N / 4096 + 1}));
  std::vector<std::thread> pool;
  for (int64_t t = 1; t < T; ++t) pool.emplace_back(describe, N * t / T, N * (t + 1) / T);
  describe(0, N / T);
  for (auto &th : pool) th.join();
}

// ---- stage: does the loader protocol terminate on this schedule?  (trws.py: simulate_look_ahead and
// simulate_spec_schedule state the rules and DESIGN.md 4.1 the kernel lines behind them; this is the same
// fixed point, by a work list instead of rounds: linear time.)
// The visit that computes position i of a run ends at a workgroup barrier the loader reaches only once the
// foreign dependencies of position i + 1 are visible -- and those of position i + 2 where bit 12 lets it wait
// two visits ahead --, and the storer raises node i's completion flag behind that barrier.  (Only
// trws_wide_kernel's loader B waits two visits ahead; the rule is applied whatever kernel a plan will pick --
// a superset of the constraints of trws_pipe_kernel and trws_pipe2_kernel, so what terminates under it
// terminates there, at the price of refusing a few graphs those two could take.)  Every run gets a workgroup of
// its own here (the ticket order with fewer workgroups is look_ahead_ok's); granules only ever make a row
// visible EARLIER.  On the image grid the chain builder never lets two runs wait for each other this way; on
// other graphs it can (two runs whose second nodes each hang on the other's first node), and such a graph must
// not reach the descriptor-driven kernels.
// The speculative schedule (sp != nullptr) makes rows visible LATER: a node of the cut run is visible to
// everybody else only when its SEGMENT commits (the storer holds a segment's flags back, spec_commit raises
// them), segment q commits behind segment q - 1, starts behind the runner's cut q, and the runner walks the
// cut run waiting for every node's foreign dependencies.  A one-node run that hangs on a node of a segment and
// feeds a later node of the SAME segment then stops that segment for good -- speculative_schedule's `fine` test
// only looks at dependencies inside the cut run.  Ordinary runs keep the loader coupling above.
// wgs > 0: only wgs workgroups are resident; they draw the tickets in order, a finished task frees its workgroup
// for the next ticket (every task is monotone, so which tasks ever finish does not depend on timing).
bool protocol_terminates(const RunSet &runs, const std::vector<int32_t> &desc, const TrwsGraph::Sweep::Spec *sp, int64_t wgs) {
  const int64_t N = (int64_t)runs.chain_rank.size();
  const std::vector<int32_t> &rptr = sp ? sp->run_ptr : runs.run_ptr;
  const int64_t T = (int64_t)rptr.size() - 1;
  const int64_t nseg = sp ? sp->nseg : 0, L = sp ? sp->seg_len : 1;
  // what a task can wait for: [0, N) a node's flag, N + q the runner's cut q, N + nseg + q segment q's commit
  std::vector<uint8_t> fired(N + 2 * nseg, 0);
  std::vector<int32_t> wait_head(N + 2 * nseg, -1), wait_next(T + 1, -1), ended(T + 1, 0), work;
  auto blocked_on = [&](int64_t pos) -> int32_t {   // first dependency of the node at `pos` nobody can see yet
    for (int32_t x : runs.deps[runs.chain_rank[pos]])
      if (!fired[x]) return x;
    return -1;
  };
  auto wait = [&](int64_t key, int32_t t) { wait_next[t] = wait_head[key]; wait_head[key] = t; };   // (one key at a time)
  auto fire = [&](int64_t key) {
    fired[key] = 1;
    for (int32_t w = wait_head[key]; w >= 0; w = wait_next[w]) work.push_back(w);
    wait_head[key] = -1;
  };
  if (sp) fired[N] = 1;
  const int64_t ntickets = T + (sp ? 1 : 0);   // task T: the runner
  int64_t finished = 0, started = 0;
  auto start_more = [&]() {
    for (; started < ntickets && (wgs <= 0 || started < wgs + finished); ++started) {
      const int32_t k = sp ? sp->run_order[started] : run_of_ticket(runs.run_order, started);
      work.push_back(k < 0 ? (int32_t)T : k);
    }
  };
  start_more();
  while (!work.empty() || (start_more(), !work.empty())) {
    const int32_t k = work.back();
    work.pop_back();
    if (k == T) {   // the runner: ended = nodes walked
      for (;;) {
        const int64_t cur = sp->c0 + ended[k];
        if (cur >= sp->c1) { ++finished; break; }
        const int32_t x = blocked_on(cur);
        if (x >= 0) { wait(x, k); break; }
        const int64_t off = ++ended[k];
        if (sp->c0 + off < sp->c1 && off % L == 0 && off / L < nseg) fire(N + off / L);
      }
      continue;
    }
    const int64_t a = rptr[k], b = rptr[k + 1];
    const int64_t seg = sp ? (int64_t)sp->kind[k] - 1 : -1;
    if (seg >= 0) {   // a segment: ended = nodes walked; nothing is visible before the commit
      if (!fired[N + seg]) { wait(N + seg, k); continue; }
      int32_t x = -1;
      while (a + ended[k] < b && (x = blocked_on(a + ended[k])) < 0) ++ended[k];
      if (x >= 0) { wait(x, k); continue; }
      if (seg > 0 && !fired[N + nseg + seg - 1]) { wait(N + nseg + seg - 1, k); continue; }
      for (int64_t pos = a; pos < b; ++pos) fire(runs.chain_rank[pos]);
      fire(N + nseg + seg);
      ++finished;
      continue;
    }
    for (;;) {   // an ordinary run: ended = visits ended (the lead-in visit first)
      if (ended[k] == b - a + 1) { ++finished; break; }
      const int64_t i = a + ended[k] - 1;   // computed by the visit about to end (a - 1: the lead-in visit)
      int32_t x = i + 1 < b ? blocked_on(i + 1) : -1;
      if (x < 0 && i + 2 < b && desc_ahead(&desc[(size_t)(i + 2) * W])) x = blocked_on(i + 2);
      if (x >= 0) { wait(x, k); break; }
      ++ended[k];
      if (i >= a) fire(runs.chain_rank[i]);
    }
  }
  return finished == T + (sp ? 1 : 0);
}

// ---- stage: lazy flags.  Completion flags are raised either in the middle of the next visit (costs a store
// drain on that run's critical path, but the dependent run can follow closely) or
// lazily at its end (free).  A run is "lazy" if nobody else reads its flags before it
// has finished anyway: no node of another run depends on any node but its last.
// run_at: by rank, the run of the node.
void mark_eager_runs(const RunSet &runs, const std::vector<int32_t> &run_at, std::vector<int32_t> &desc) {
  const int64_t N = (int64_t)runs.chain_rank.size(), R = runs.runs();
  std::vector<uint8_t> eager(R, 0);
  for (int64_t r = 0; r < N; ++r)
    for (int32_t x : runs.deps[r]) {
      const int32_t kx = run_at[x];
      if (x != runs.chain_rank[runs.run_ptr[kx + 1] - 1]) eager[kx] = 1;
    }
  for (int64_t k = 0; k < R; ++k)
    for (int64_t p = runs.run_ptr[k]; p < runs.run_ptr[k + 1]; ++p) desc[(size_t)p * W + kDescEager] = eager[k];
}

// Can the runner recompute the row every visit of the run [sp.c0, sp.c1) hands on, and has every dependency inside
// the run committed before the runner gets there?
bool runner_can_walk(const RunSet &runs, const std::vector<int32_t> &desc, const TrwsGraph::Sweep::Spec &sp) {
  const int64_t L = sp.seg_len;
  auto seg_of = [&](int64_t p) { return (int32_t)std::min<int64_t>((p - sp.c0) / L, sp.nseg - 1); };
  std::vector<int64_t> pos_of(runs.chain_rank.size(), -1);
  for (int64_t p = sp.c0; p < sp.c1; ++p) pos_of[runs.chain_rank[p]] = p;
  for (int64_t p = sp.c0; p < sp.c1; ++p) {
    const int32_t *D = &desc[(size_t)p * W];
    const int nout = desc_nout(D), nin = desc_nin(D), nd = desc_ndep(D), ntot = nout + nin;
    if (nout > 4 || nin > 4) return false;
    int nfresh = 0, kfirst = ntot, slots[2] = {-1, -1};
    for (int k = nout; k < ntot; ++k) {
      const int sl = D[kDescSlot + k];
      if (sl < 0) continue;
      if (sl >= 4) return false;   // only what the node in front hands over, from its first four messages
      if (nfresh == 0) kfirst = k;
      ++nfresh;
      if (slots[0] < 0 || slots[0] == sl) slots[0] = sl;
      else if (slots[1] < 0 || slots[1] == sl) slots[1] = sl;
      else return false;
    }
    if (p == sp.c0 ? nfresh != 0 : (nfresh < 1)) return false;
    if (ntot - kfirst > 4 || (ntot - kfirst) - nfresh > 3) return false;
    // a dependency inside the run must have committed before the runner gets here: an earlier segment
    for (int k = 0; k < nd; ++k) {
      const int32_t x = D[kDescDep + k];
      if (pos_of[x] >= 0 && seg_of(pos_of[x]) >= seg_of(p)) return false;
    }
  }
  return true;
}

// ---- stage: speculative schedule of the one long serial run (trws_graph.h: Sweep::Spec); !ok: none
TrwsGraph::Sweep::Spec speculative_schedule(const RunSet &runs, const std::vector<int32_t> &desc, int seg_len, int64_t res) {
  typedef TrwsGraph::Sweep::Spec Spec;
  const int64_t R = runs.runs();
  Spec sp;
  int64_t best = -1, len1 = 0, len2 = 0;
  for (int64_t k = 0; k < R; ++k) {
    const int64_t len = runs.run_ptr[k + 1] - runs.run_ptr[k];
    if (len > len1) { len2 = len1; len1 = len; best = k; } else if (len > len2) len2 = len;
  }
  const int L = seg_len;
  sp.run = (int32_t)best; sp.c0 = runs.run_ptr[best]; sp.c1 = runs.run_ptr[best + 1];
  sp.seg_len = L; sp.nseg = (int32_t)(len1 / L); sp.max_len = (int32_t)(len1 - (int64_t)(sp.nseg - 1) * L);
  if (!(sp.nseg >= 8 && sp.nseg < (1 << 20) && len1 + 8 >= 2 * len2) || !runner_can_walk(runs, desc, sp)) return Spec();
  for (int64_t k = 0; k < R; ++k) {
    if (k == best) for (int32_t q = 0; q < sp.nseg; ++q) { sp.run_ptr.push_back(sp.c0 + q * L); sp.kind.push_back(1 + q); }
    else { sp.run_ptr.push_back(runs.run_ptr[k]); sp.kind.push_back(0); }
  }
  sp.run_ptr.push_back(runs.run_ptr[R]);
  // tickets: the runner's first, whatever the direction (the workgroup that draws it serves it before anything
  // else, trws_pipe.hip; it waits for what it needs, holding one CU of 256), then the chain schedule's order
  // with the cut run's ticket replaced by its segments'
  sp.run_order.push_back(-1);
  for (int64_t t = 0; t < R; ++t) {
    const int32_t k = run_of_ticket(runs.run_order, t);
    if (k == best) for (int32_t q = 0; q < sp.nseg; ++q) sp.run_order.push_back((int32_t)best + q);
    else sp.run_order.push_back(k < best ? k : k + sp.nseg - 1);
  }
  sp.ok = true;
  // (never a schedule the host cannot show to terminate: such a graph keeps the plain chain schedule)
  // (with every task resident, and -- where the tickets outnumber the workgroups certain to be resident -- with
  //  that many workgroups drawing tickets in order: a segment holds its workgroup until it commits)
  const int64_t Wres = res > 0 && (int64_t)sp.run_order.size() > res ? res : 0;
  if (protocol_terminates(runs, desc, &sp, 0) && (Wres == 0 || protocol_terminates(runs, desc, &sp, Wres))) return sp;
  return Spec();
}

// ---- stage: tagged-granule hand-over (word 57, trws_graph.h): the rows a node fetches from another ordinary run that
// drew an earlier ticket come as granules, published by the producer as soon as they are final; everything
// else -- the speculative schedule's cut run `cut` (its segments hold their flags back until they commit, a granule
// must never show an uncommitted row), rows of the same run, strips -- keeps the completion flags.
// (serial: a consumer marks its producer's descriptor too)
void mark_granules(const TrwsGraph &g, const RunSet &runs, const std::vector<int32_t> &run_at, int32_t cut, std::vector<int32_t> &desc) {
  const int64_t N = (int64_t)runs.chain_rank.size(), R = runs.runs();
  std::vector<int32_t> pos_at(N), ticket_of(R);
  for (int64_t p = 0; p < N; ++p) pos_at[runs.chain_rank[p]] = (int32_t)p;
  for (int64_t t = 0; t < R; ++t) ticket_of[run_of_ticket(runs.run_order, t)] = (int32_t)t;
  for (int64_t p = 0; p < N; ++p) {
    const int32_t kr = run_at[runs.chain_rank[p]];
    if (kr == cut) continue;
    int32_t *D = &desc[(size_t)p * W];
    const int nd = desc_ndep(D);
    const uint32_t fetch = (uint32_t)D[kDescFetch];
    uint32_t gm = 0;
    for (int k = 0; k < 8; ++k) {
      if (!((fetch >> k) & 1)) continue;
      const int32_t ko = run_at[g.rank[D[kDescOther + k]]];
      if (ko != kr && ko != cut && ticket_of[ko] < ticket_of[kr]) gm |= 1u << k;
    }
    if (__builtin_popcount(gm) > 4) gm = 0;   // (the kernel sweeps at most four granule rows)
    if (!gm) continue;
    // a dependency whose rows all come as granules is no longer waited for by its flag
    uint32_t flags = 0;
    for (int q = 0; q < nd; ++q) {
      bool feeds = false, covered = true;
      for (int k = 0; k < 8; ++k)
        if (((fetch >> k) & 1) && g.rank[D[kDescOther + k]] == D[kDescDep + q]) { feeds = true; covered = covered && ((gm >> k) & 1); }
      if (!(feeds && covered)) flags |= 1u << q;
    }
    D[kDescGran] |= (int32_t)(gm | (flags << 16));
    for (int k = 0; k < 8; ++k) {
      if (!((gm >> k) & 1)) continue;
      int32_t *P = &desc[(size_t)pos_at[g.rank[D[kDescOther + k]]] * W];
      const int pout = desc_nout(P);
      for (int j = 0; j < pout; ++j)
        if (P[kDescEdge + j] == D[kDescEdge + k]) P[kDescGran] |= (int32_t)((1u << (8 + j)) | (1u << 20));
    }
  }
}

}  // namespace

Finished finish_schedule(const DirView &v, const RunSet &runs, int64_t res, bool with_resident, int seg_len, StageClock &clock) {
  const int64_t N = v.N, R = runs.runs();
  Finished out;
  out.desc.assign((size_t)N * W, 0);
  clock.done("dir0 descriptor allocation");
  describe_visits(v, runs, out.desc);
  clock.done("dir0 descriptors");
  out.terminates = protocol_terminates(runs, out.desc, nullptr, 0);
  if (out.terminates && with_resident) out.terminates = protocol_terminates(runs, out.desc, nullptr, res);
  clock.done("dir0 protocol check");
  std::vector<int32_t> run_at(N);   // by rank
  for (int64_t k = 0; k < R; ++k)
    for (int64_t p = runs.run_ptr[k]; p < runs.run_ptr[k + 1]; ++p) run_at[runs.chain_rank[p]] = (int32_t)k;
  mark_eager_runs(runs, run_at, out.desc);
  if (v.own)
    for (int64_t k = 0; k < R; ++k) out.run_strip.push_back(v.strip_of(runs.chain_rank[runs.run_ptr[k]]));
  if (runs.chain && !v.own && R >= 2) out.spec = speculative_schedule(runs, out.desc, seg_len, res);
  if (!v.own) mark_granules(v.g, runs, run_at, out.spec.ok ? out.spec.run : -1, out.desc);
  clock.done("dir0 marks");
  return out;
}

}  // namespace stereo
