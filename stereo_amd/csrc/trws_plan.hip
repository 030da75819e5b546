// TRW-S simultaneous fusion on MI355X (gfx950): the plan object's host logic and its C ABI.
//
// Replaces the reference's trws_mex gateway + MRFEnergy core + TypeStereo*
// message update (cpp/trws_mex.cpp, cpp/trw-s/{minimize,ordering,MRFEnergy}.cpp,
// cpp/trw-s/typeStereo{Linear,Quadratic}.h).  Built with -ffp-contract=off: the
// reference runs SSE2 doubles without FMA and every value below is computed
// with the same association of + - * / so results are bit identical.
//
// Layout in HBM (all label-fastest, exactly MATLAB's K x N / K x E column major):
//   unary [N][K]   messages [E][K]   q,qprim [E][K] (or one shared positions[K])
//   perm_q, perm_qp [E][K] uint16: ascending sort permutation of q(:,e), qprim(:,e)
// Work decomposition: the reference node order induces a dependency DAG.  One persistent
// launch per sweep walks it as a dataflow: workgroups draw "runs" (a grid row, the border
// chain) from a ticket counter and hand messages over in LDS inside a run, through HBM +
// completion flags between runs.  Five kernel families, identical results
// (stereo_trws_plan_path), one translation unit each over the common device header trws_dev.h:
//   trws_pipe.hip     K <= 64, role-specialised waves, both smoothness kernels
//   trws_pipe2.hip    64 < K <= 128, two labels per lane, both smoothness kernels, per-edge positions
//   trws_wide.hip     64 < K <= 256, shared strictly ascending positions
//   trws_generic.hip  everything else (any graph, K <= 512, min-plus message mode)
//   trws_large.hip    512 < K <= 4096, shared strictly ascending positions (any graph, both modes)
// Which one runs a plan is decided in ONE place, trws_family.h (the rule as a table: DESIGN.md 4.8).
// The three descriptor-driven families walk the chain schedule of trws_graph.h; messages take a
// certified min-plus fast path and fall back to the reference's serial envelope
// construction when the certificate fails.
//
// The host code around the kernels, by concern:
//   trws_family.h/.cpp   the kernel-family rule (host only)
//   trws_graph.h         graph analysis (host only), one stage per function behind build_trws_graph: trws_graph.cpp order,
//                        lists, rank-contiguous runs · trws_graph_schedule.cpp chain schedule, sub-row runs ·
//                        trws_graph_desc.cpp descriptors, protocol proof, marks · trws_graph_strips.cpp strip layouts ·
//                        trws_graph_views.cpp host views for tests · trws_graph_stages.h what the stages pass on
//   trws_runner_records.h/.cpp  the K <= 64 runner's chain records, made from the bound descriptors (host only)
//   trws_plan.h          struct stereo_trws_plan, the table of creation-time switches (internal)
//   trws_plan_create.hip creation (with the cache of the last graph analysis) and destruction
//   trws_plan.hip        this file: inputs, iterations, results, strip wiring, min-marginals
//   trws_inputs.hip      sort permutations of the positions, analysis of a shared positions vector
//   trws_plan_debug.hip  timeline / profiler printouts, development aids, stereo_trws_messages
//   trws_state.h/.hip    solver state: save / load, its refusal rule, the strips' gather and scatter
//   trws_gateway.hip     what trws_mex reaches: stereo_trws, its plan cache, row strips behind it
#include <algorithm>
#include <cstring>
#include <limits>

#include "trws_plan.h"

namespace stereo {

std::string &last_error() {
  static thread_local std::string s;
  return s;
}

// The speculative schedule runs where its runner's arithmetic is what message_regs returns under a passed certificate:
// trws_pipe_kernel, linear kernel, certified messages, shared strictly ascending positions, uniformly spaced over the
// truncation window (rounded up to a multiple of four entries, at most eight: the runner keeps the window in registers).
bool spec_active(const stereo_trws_plan *P) {
  // (and a handful of resident workgroups: the runner, the segment that commits, the segments in between)
  // (trws_pipe_kernel, or trws_wide_kernel with an even label count: its vector loaders, trws_wspec.h)
  const bool kernel_has_it = P->family == TrwsFamily::Pipe || (P->family == TrwsFamily::Wide && (P->K & 1) == 0 && P->facts.exact);
  return P->spec_allowed && P->grid_blocks >= 8 && kernel_has_it && P->nstrips == 1 && P->kernel == 1 && P->certificate && P->pos != nullptr &&
         P->pos_ascending && P->window <= 8 && P->uniform_step != 0 && P->spec_window;
}

bool own_sub_rows(const stereo_trws_plan *P, int d) { return P->sub_rows[d] && P->family == TrwsFamily::Pipe && P->nstrips == 1; }
const TrwsGraph::Sweep::Spec &own_spec(const stereo_trws_plan *P, int d) {
  return own_sub_rows(P, d) ? P->graph->sweep[d].chunked.spec : P->graph->sweep[d].spec;
}

// allow_spec: the plan's own launches (speculative schedule); false: a launch it shares with other plans.
// allow_sub: its sub-row runs as well -- a single plan only, not a member's own launches inside a batch.
DevParams make_params(stereo_trws_plan *P, bool allow_spec, bool allow_sub) {
  DevParams p{};
  p.K = P->K; p.Kp = P->Kp; p.kernel = P->kernel; p.lambda = P->lambda;
  p.unary = P->unary; p.msg = P->d_msg.p; p.q = P->q; p.qprim = P->qprim; p.pos = P->pos;
  p.perm_q = P->d_perm_q.p; p.perm_qp = P->d_perm_qp.p; p.perm_pos = P->d_perm_pos.p;
  p.alpha = P->alpha; p.mdir = P->d_mdir.p; p.tail = P->d_tail.p; p.order = P->d_order.p;
  p.fptr = P->d_fptr.p; p.fidx = P->d_fidx.p; p.bptr = P->d_bptr.p; p.bidx = P->d_bidx.p;
  p.gamma = P->d_gamma.p; p.lb_pos_node = P->d_lbn.p; p.lb_pos_edge = P->d_lbe.p;
  p.lbterms = P->d_lbterms.p; p.eterms = P->d_eterms.p; p.x = P->d_x.p;
  // the descriptor-driven kernels walk the chain schedule (trws_graph.h), the generic ones the
  // rank-contiguous runs
  const bool chain = pipelined(P->family);
  for (int d = 0; d < 2; ++d) {
    if (chain) {
      p.run_ptr[d] = P->d_chain_run_ptr[d].p; p.nruns[d] = (int)P->graph->sweep[d].chain_run_ptr.size() - 1;
      p.run_order[d] = P->d_chain_run_order[d].p;
    } else {
      p.run_ptr[d] = P->d_run_ptr[d].p; p.nruns[d] = (int)P->graph->sweep[d].run_ptr.size() - 1;
      p.run_order[d] = P->d_run_order[d].p;
    }
    p.dep_ptr[d] = P->d_dep_ptr[d].p; p.dep_rank[d] = P->d_dep_rank[d].p;
    p.in_slot[d] = P->d_in_slot[d].p;
  }
  for (int d = 0; d < 2; ++d) {
    if (P->nstrips > 1) {  // the strip's own runs, already in ticket order
      p.run_ptr[d] = P->d_chain_run_ptr[d].p; p.nruns[d] = P->ntickets[d]; p.run_order[d] = nullptr;
    }
    p.ntickets[d] = p.nruns[d];
  }
  p.peer_msg0 = P->peer_msg[0]; p.peer_msg1 = P->peer_msg[1];
  p.peer_done0 = P->peer_done[0]; p.peer_done1 = P->peer_done[1];
  p.peer_x0 = P->peer_x[0]; p.peer_x1 = P->peer_x[1];
  p.gran = P->d_gran.p; p.xgran = P->d_xgran.p;
  p.done = P->d_done.p; p.ticket = P->d_ctl.p; p.abort_flag = P->d_ctl.p + 1; p.N = (int)P->Nl;
  p.spin_ticks = P->spin_ticks;
  p.n_own = P->layout ? (int)P->layout->n_own : (int)P->Nl;
  p.fallbacks = P->d_fallbacks.p; p.certificate = P->certificate ? 1 : 0;
  // MINPLUS in the wide-label regime: the wide kernel's plain min-plus branch
  p.lean = (P->family == TrwsFamily::Wide && !P->facts.exact) ? 1 : 0;
  p.prof = P->d_prof.p;
  p.timeline = P->d_timeline.p;
  p.desc[0] = P->d_desc[0].p; p.desc[1] = P->d_desc[1].p;
  p.prof_run = -1;
  p.large_scratch = P->d_large_scr.p;
  p.window = P->window;
  p.uniform_step = P->uniform_step;
  p.pos_first = P->pos_first; p.pos_last = P->pos_last;
  p.debug = 0;
  if (const char *dbg = std::getenv("STEREO_HIP_TRWS_DEBUG")) p.debug = std::atoi(dbg);
  p.tl_stride = p.nruns[0];
  p.self = P->d_self.p;
  bool sub[2] = {false, false};
  for (int d = 0; d < 2 && allow_spec && allow_sub; ++d) {
    if (!(sub[d] = own_sub_rows(P, d))) continue;
    const TrwsGraph::Sweep::Chunked &C = P->graph->sweep[d].chunked;
    p.run_ptr[d] = P->d_sub_run_ptr[d].p; p.nruns[d] = p.ntickets[d] = (int)C.run_ptr.size() - 1;
    p.run_order[d] = P->d_sub_run_order[d].p; p.desc[d] = P->d_sub_desc[d].p;
    p.tl_stride = std::max(p.nruns[0], p.nruns[1]);
  }
  if (allow_spec && spec_active(P)) {
    // the chain schedule with the long run cut into segments + the runner's ticket
    for (int d = 0; d < 2; ++d) {
      const TrwsGraph::Sweep::Spec &sp = sub[d] ? P->graph->sweep[d].chunked.spec : P->graph->sweep[d].spec;
      p.run_ptr[d] = (sub[d] ? P->d_sub_spec_run_ptr[d] : P->d_spec_run_ptr[d]).p; p.nruns[d] = (int)sp.kind.size();
      p.run_order[d] = (sub[d] ? P->d_sub_spec_run_order[d] : P->d_spec_run_order[d]).p; p.ntickets[d] = (int)sp.run_order.size();
      p.spec_kind[d] = (sub[d] ? P->d_sub_spec_kind[d] : P->d_spec_kind[d]).p; p.spec_c0[d] = sp.c0; p.spec_c1[d] = sp.c1;
      if (P->family == TrwsFamily::Pipe) p.run_rec[d] = runner_records(P, d, sub[d]);
    }
    const TrwsGraph::Sweep::Spec &sp = P->graph->sweep[0].spec;   // (the same segments over either set of runs)
    p.spec_len = sp.seg_len; p.spec_nseg = sp.nseg; p.spec_max_len = sp.max_len;
    p.spec_rows = P->d_spec_rows.p; p.spec_x = P->d_spec_x.p; p.spec_undo = P->d_spec_undo.p; p.spec_stat = P->d_spec_stat.p;
    p.tl_stride = std::max(p.nruns[0], p.nruns[1]);
  }
  p.win_ok = (P->pos_ascending && P->window <= 16 && !(p.debug & 256)) ? 1 : 0;
  p.pos_gap = P->pos_gap;
  if (const char *pr = std::getenv("STEREO_HIP_TRWS_PROF_RUN")) p.prof_run = std::atoi(pr);
  return p;
}

size_t persistent_lds_bytes(bool large, int Kp) { return large ? large_lds_bytes(Kp) : generic_lds_bytes(Kp); }

namespace {

// One persistent launch: 0 = forward, 1 = backward, 2 = forward + primal of the
// previous iteration, 3 = primal only.
void launch_persistent(stereo_trws_plan *P, const DevParams &p, int what, hipStream_t s) {
  const int epoch = ++P->epoch;
  STEREO_HIP_CHECK(hipMemsetAsync(P->d_ctl.p, 0, sizeof(int32_t), s));  // ticket = 0
  switch (P->family) {
    case TrwsFamily::Wide: launch_wide(P->kernel, what, std::min(P->grid_blocks, P->cus), s, p, epoch); break;
    case TrwsFamily::Pipe2: launch_pipe2(P->kernel, P->pos != nullptr, what, std::min(P->grid_blocks, P->cus), s, p, epoch); break;
    case TrwsFamily::Pipe: {
      int blocks = P->grid_blocks;
      static const char *be = std::getenv("STEREO_HIP_TRWS_BLOCKS");   // (development: workgroups of a pipelined sweep launch)
      if (be && std::atoi(be) > 0) blocks = std::min(blocks, std::atoi(be));
      // (development, STEREO_HIP_TRWS_TIMELINE=first: the fused launches leave the timeline alone, so that direction 0 keeps
      //  the plan's first forward launch -- the only one without a primal pass; a single plan's own K <= 64 launches only,
      //  which is where the row-lag record of DESIGN.md 4.4 is taken: groups, batches and the other families ignore it)
      static const bool tl_first = [] { const char *c = std::getenv("STEREO_HIP_TRWS_TIMELINE"); return c && std::string(c) == "first"; }();
      if (tl_first && what == 2) {
        DevParams q = p;
        q.timeline = nullptr;
        launch_pipe(P->kernel, P->pos != nullptr, what, blocks, s, q, epoch);
        break;
      }
      launch_pipe(P->kernel, P->pos != nullptr, what, blocks, s, p, epoch);
      break;
    }
    case TrwsFamily::Large: launch_large(P->kernel, P->mode, what, P->grid_blocks, persistent_lds_bytes(true, P->Kp), s, p, epoch); break;
    default: launch_generic(P->kernel, P->mode, what, P->grid_blocks, persistent_lds_bytes(false, P->Kp), s, p, epoch);
  }
  if (what != 3) P->sweep_launches += 1;
}

// One fused launch for the plans G[0 .. n) whose parameter blocks lie at `table` in that order: the strips of a group,
// or -- B given -- members of a batch (what: as in launch_persistent).  Strips and the one-per-CU families divide the
// grid statically; a batch on the K <= 64 kernel gets workgroups that move between its members, and a batch whose
// static shares do not fit the device together is split into consecutive launches (trws_batch_partition).
void launch_table(stereo_trws_plan *const *G, int n, const DevParams *table, int what, hipStream_t s, int epoch, stereo_trws_batch *B) {
  stereo_trws_plan *P0 = G[0];
  const bool one_per_cu = P0->family == TrwsFamily::Wide || P0->family == TrwsFamily::Pipe2;
  int blocks[kMaxGroup];
  for (int i = 0; i < n; ++i) {
    stereo_trws_plan *P = G[i];
    STEREO_HIP_CHECK(hipMemsetAsync(P->d_ctl.p, 0, sizeof(int32_t), s));  // ticket = 0
    blocks[i] = one_per_cu ? std::min(P->grid_blocks, P->cus) : P->grid_blocks;
    if (what != 3) P->sweep_launches += 1;
  }
  const bool floating = B && !one_per_cu;
  for (int at = 0; at < n;) {
    BatchArgs ba{};
    GroupArgs &ga = ba.g;
    ga.pp = table + at;
    if (B) {
      ga.n = trws_batch_partition(blocks + at, n - at, B->capacity, floating, ga.first);
    } else {   // strips wait for each other: all of them in this launch, shares one behind the other
      ga.n = n;
      for (int i = 0; i < n; ++i) ga.first[i + 1] = ga.first[i] + blocks[i];
    }
    const int total = ga.first[ga.n];
    switch (P0->family) {   // (the callers let the pipelined families through only)
      case TrwsFamily::Wide: launch_wide_group(P0->kernel, what, total, s, ga, epoch); break;
      case TrwsFamily::Pipe2: launch_pipe2_group(P0->kernel, P0->pos != nullptr, what, total, s, ga, epoch); break;
      default:
        if (B) { ba.ctl = B->d_ctl.p; launch_pipe_batch(P0->kernel, P0->pos != nullptr, what, total, s, ba, epoch); }
        else launch_pipe_group(P0->kernel, P0->pos != nullptr, what, total, s, ga, epoch);
    }
    if (B) B->launches += 1;
    at += ga.n;
  }
  STEREO_HIP_CHECK(hipGetLastError());
}

// ... for the strips of a group: one state, one epoch
void launch_group(stereo_trws_plan *const *G, int n, int what, hipStream_t s) {
  const int epoch = G[0]->epoch + 1;
  for (int i = 0; i < n; ++i) ++G[i]->epoch;
  launch_table(G, n, G[0]->d_group.p, what, s, epoch, nullptr);
}

// ... for the members of a batch that take part in launch `what`: all of G, but in the forward sweep of a first
// iteration (what 0) only those whose forward sweep has not run yet.  Members come with epochs of their own (one may
// have iterated alone); an epoch only has to exceed every epoch its plan has seen -- flags are compared with <, granule
// tags with == against values that are all older -- so the launch takes one above the highest and every member adopts it.
void launch_batch(stereo_trws_batch *B, stereo_trws_plan *const *G, const DevParams *params, int n, int what, hipStream_t s) {
  stereo_trws_plan *in[kMaxGroup];
  DevParams *h = B->h_table.p + (size_t)what * kMaxGroup, *d = B->d_table.p + (size_t)what * kMaxGroup;
  int m = 0, epoch = 0;
  for (int i = 0; i < n; ++i) {
    if (what == 0 && G[i]->fwd_pending) continue;
    if (what == 1 && G[i]->bwd_pending) continue;   // (its backward sweep has run too: issue_backward_ahead)
    epoch = std::max(epoch, G[i]->epoch + 1);
    h[m] = params[i];
    in[m++] = G[i];
  }
  for (int i = 0; i < m; ++i) in[i]->epoch = epoch;
  STEREO_HIP_CHECK(hipMemcpyAsync(d, h, sizeof(DevParams) * m, hipMemcpyHostToDevice, s));
  launch_table(in, m, d, what, s, epoch, B);
}

// What the belief kernels walk on a plan: the whole problem's lists by rank, or a strip's own (StripBeliefLists).
struct BeliefLists {
  const int32_t *order, *fptr, *fidx, *bptr, *bidx;
  int64_t n;
};
BeliefLists belief_lists(const stereo_trws_plan *P) {
  if (P->layout) return {P->d_bel_own.p, P->d_bel_fptr.p, P->d_bel_fidx.p, P->d_bel_bptr.p, P->d_bel_bidx.p, P->layout->n_own};
  return {P->d_order.p, P->d_fptr.p, P->d_fidx.p, P->d_bptr.p, P->d_bidx.p, P->N};
}

// The arguments of one grouped belief launch (phase 1 or 2) for the plans G[0 .. m), with the block table on the
// device: it lives with G[0] and is sent only when it differs from what was sent last -- a blocking copy, behind
// everything on the device where the table may still be read (phase 2: launches on the caller's streams; phase 1's
// last reader is behind the collect of the previous iteration).  Called before anything of the iteration is launched.
BeliefGroupArgs belief_group(stereo_trws_plan *const *G, int m, int phase) {
  stereo_trws_plan *P0 = G[0];
  BeliefBlock blocks[kMaxGroup];
  BeliefGroupArgs ga{};
  ga.n = m;
  for (int i = 0; i < m; ++i) {
    const stereo_trws_plan *P = G[i];
    const BeliefLists L = belief_lists(P);
    BeliefBlock &b = blocks[i];
    std::memset(&b, 0, sizeof(b));   // (compared bytewise below)
    b.in = phase == 1 ? P->unary : P->d_belief.p; b.msg = P->d_msg.p; b.order = L.order;
    b.ptr = phase == 1 ? L.fptr : L.bptr; b.idx = phase == 1 ? L.fidx : L.bidx;
    b.map = (phase == 2 && P->layout) ? P->d_lnodes.p : nullptr;
    b.out = phase == 1 ? P->d_belief.p : nullptr;
    b.n = L.n; b.K = P->K; b.lg = beliefs_lanes_log2(P->K);
    ga.first[i + 1] = ga.first[i] + beliefs_workgroups(L.n, P->K);
  }
  const int w = phase - 1;
  if (!P0->d_bel_table.p) P0->d_bel_table.alloc(2 * kMaxGroup);
  if (P0->bel_sent_n[w] != m || std::memcmp(P0->bel_sent[w], blocks, sizeof(BeliefBlock) * m) != 0) {
    if (phase == 2) STEREO_HIP_CHECK(hipDeviceSynchronize());
    STEREO_HIP_CHECK(hipMemcpy(P0->d_bel_table.p + (size_t)w * kMaxGroup, blocks, sizeof(BeliefBlock) * m, hipMemcpyHostToDevice));
    std::memcpy(P0->bel_sent[w], blocks, sizeof(BeliefBlock) * m);
    P0->bel_sent_n[w] = m;
  }
  ga.pp = P0->d_bel_table.p + (size_t)w * kMaxGroup;
  return ga;
}

// One iteration's launches and device-to-host copies for the plans of one launch (one plan, the strips of a
// group, or the members of a batch), without waiting for any of them.  launch(what) is the one thing that differs: the
// plan's own launch (stereo_trws_plan_iterate), the group launch (the issue entries) or the batch launch
// (stereo_trws_batch_iterate); beliefs: with phase 1 of the node beliefs, for every plan that keeps them.
// Strips are in one state; the members of a batch need not be: launch(0) is for the plans whose forward sweep has
// not run yet, and the batch launch leaves the others out of it.  The same holds for launch(1) and a plan whose backward
// sweep is pending (issue_backward_ahead): the iteration takes that sweep and its terms instead of launching one.
// ahead: issue_backward_ahead follows and sends the energy terms itself, past the sweep it launches.
template <class Launch>
void issue_iteration(stereo_trws_plan *const *plans, int n, hipStream_t s, bool beliefs, Launch launch, bool ahead = false) {
  stereo_trws_plan *P0 = plans[0];
  // node beliefs, phase 1: one plan keeps them -- its own launch; several (logical strips, batch members) -- one launch
  stereo_trws_plan *keeping[kMaxGroup];
  int nkeep = 0;
  for (int i = 0; beliefs && i < n; ++i)
    if (plans[i]->keep_mm) keeping[nkeep++] = plans[i];
  BeliefGroupArgs bel{};
  if (nkeep > 1) bel = belief_group(keeping, nkeep, 1);
  // a pending backward sweep may still be running on the stream of the call that launched it
  for (int i = 0; i < n; ++i)
    if (plans[i]->bwd_pending && plans[i]->issue_stream != s) STEREO_HIP_CHECK(hipStreamWaitEvent(s, plans[i]->ev_ahead, 0));
  if (P0->bwd_pending) std::swap(P0->ev0, P0->ev0_next);   // (recorded in front of the pending sweep)
  else if (P0->time_sweeps) STEREO_HIP_CHECK(hipEventRecord(P0->ev0, s));
  bool fwd_due = false, bwd_due = false;
  for (int i = 0; i < n; ++i) { fwd_due = fwd_due || !plans[i]->fwd_pending; bwd_due = bwd_due || !plans[i]->bwd_pending; }
  if (fwd_due) launch(0);
  if (bwd_due) launch(1);
  // the backward sweep's lower-bound terms travel while the next launch runs
  if (bwd_due) STEREO_HIP_CHECK(hipEventRecord(P0->ev_bwd, s));
  for (int i = 0; i < n; ++i) {
    stereo_trws_plan *P = plans[i];
    if (P->bwd_pending) {   // the pending sweep becomes this iteration's: its terms are on their way already
      std::swap(P->h_lb.p, P->h_lb_next.p);
      std::swap(P->ev_lb, P->ev_lb_next);
      P->sweep_launches += P->held_launches;
      P->held_launches = 0; P->bwd_pending = false; P->lb_in_flight = true;
      continue;
    }
    STEREO_HIP_CHECK(hipStreamWaitEvent(P->copy_stream, P0->ev_bwd, 0));
    STEREO_HIP_CHECK(hipMemcpyAsync(P->h_lb.p, P->d_lbterms.p, sizeof(double) * P->n_lb, hipMemcpyDeviceToHost, P->copy_stream));
    STEREO_HIP_CHECK(hipEventRecord(P->ev_lb, P->copy_stream));
    P->lb_in_flight = true;
  }
  // every firstForward edge holds this iteration's backward message into its tail now (in a strip's own copy too: the
  // row of an edge is written by its two ends' visits only, and the strip's backward launch waited for both)
  if (nkeep == 1) {
    stereo_trws_plan *P = keeping[0];
    const BeliefLists L = belief_lists(P);
    launch_beliefs_accum(P->unary, P->d_msg.p, L.order, L.fptr, L.fidx, P->K, L.n, P->d_belief.p, s);
  } else if (nkeep > 1) {
    launch_beliefs_accum_group(bel, s);
  }
  launch(2);  // forward sweep of the NEXT iteration fused with this iteration's primal
  for (int i = 0; beliefs && i < n; ++i) plans[i]->mm_ready = plans[i]->keep_mm;
  if (P0->time_sweeps) STEREO_HIP_CHECK(hipEventRecord(P0->ev1, s));
  for (int i = 0; i < n; ++i) {
    stereo_trws_plan *P = plans[i];
    P->fwd_pending = true;
    if (!ahead) STEREO_HIP_CHECK(hipMemcpyAsync(P->h_en.p, P->d_eterms.p, sizeof(double) * P->n_en, hipMemcpyDeviceToHost, s));
    STEREO_HIP_CHECK(hipMemcpyAsync(P->h_ctl.p, P->d_ctl.p, kCtlWords * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    P->issued = true; P->issue_stream = s; P->timed_by = P0;
  }
}

// The backward sweep of the iteration AFTER the one issued last, right behind its fused launch: the device goes on while
// the host waits for that iteration's terms, copies and sums them.  Whether the loop goes on is not known yet, so nothing
// of the sweep shows until an iteration takes it (issue_iteration): the terms go to a buffer of their own, the launch is
// not counted, and the counters the sweep adds to are read first.  The energy terms of the issued iteration -- nothing a
// backward sweep writes -- go to the host on the copy stream, so that the sweep starts right behind the fused launch.
// A single plan's own launches only, behind issue_iteration(.., ahead = true).
void issue_backward_ahead(stereo_trws_plan *P, const DevParams &p, hipStream_t s) {
  ensure_ahead_buffers(P);
  STEREO_HIP_CHECK(hipMemcpyAsync(P->h_held.p, P->d_fallbacks.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (P->d_spec_stat.p)
    STEREO_HIP_CHECK(hipMemcpyAsync(P->h_held.p + 1, P->d_spec_stat.p, sizeof(unsigned long long) * 32, hipMemcpyDeviceToHost, s));
  STEREO_HIP_CHECK(hipEventRecord(P->ev_fwd, s));
  STEREO_HIP_CHECK(hipStreamWaitEvent(P->copy_stream, P->ev_fwd, 0));
  STEREO_HIP_CHECK(hipMemcpyAsync(P->h_en.p, P->d_eterms.p, sizeof(double) * P->n_en, hipMemcpyDeviceToHost, P->copy_stream));
  STEREO_HIP_CHECK(hipEventRecord(P->ev_end, P->copy_stream));   // what collect_iteration waits for instead of the stream
  // d_lbterms is free once the issued iteration's terms have left it
  if (P->lb_in_flight) STEREO_HIP_CHECK(hipStreamWaitEvent(s, P->ev_lb, 0));
  STEREO_HIP_CHECK(hipEventRecord(P->ev0_next, s));
  const int64_t counted = P->sweep_launches;
  launch_persistent(P, p, 1, s);
  P->held_launches = P->sweep_launches - counted; P->sweep_launches = counted;
  STEREO_HIP_CHECK(hipEventRecord(P->ev_bwd, s));
  STEREO_HIP_CHECK(hipEventRecord(P->ev_ahead, s));   // (ev_bwd is recorded again by every iteration; this one stays)
  STEREO_HIP_CHECK(hipStreamWaitEvent(P->copy_stream, P->ev_bwd, 0));
  STEREO_HIP_CHECK(hipMemcpyAsync(P->h_lb_next.p, P->d_lbterms.p, sizeof(double) * P->n_lb, hipMemcpyDeviceToHost, P->copy_stream));
  STEREO_HIP_CHECK(hipEventRecord(P->ev_lb_next, P->copy_stream));
  P->bwd_pending = true;
}

}  // namespace

void ensure_ahead_buffers(stereo_trws_plan *P) {
  if (P->h_lb_next.p) return;
  P->h_lb_next.alloc(P->n_lb); P->h_held.alloc(kHeldWords);
  std::memset(P->h_held.p, 0, sizeof(unsigned long long) * kHeldWords);
  STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_lb_next, hipEventDisableTiming));
  STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_end, hipEventDisableTiming));
  STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_fwd, hipEventDisableTiming));
  STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_ahead, hipEventDisableTiming));
  STEREO_HIP_CHECK(hipEventCreate(&P->ev0_next));
}

// A pending backward sweep that no iteration will take (new inputs, a reset): wait for it and give the counters back
// what they read before it.  Its messages and flags go with the state that is reset.
void discard_backward_ahead(stereo_trws_plan *P) {
  if (!P->bwd_pending) return;
  STEREO_HIP_CHECK(hipStreamSynchronize(P->issue_stream));
  STEREO_HIP_CHECK(hipStreamSynchronize(P->copy_stream));
  STEREO_HIP_CHECK(hipMemcpy(P->d_fallbacks.p, P->h_held.p, sizeof(unsigned long long), hipMemcpyHostToDevice));
  if (P->d_spec_stat.p)
    STEREO_HIP_CHECK(hipMemcpy(P->d_spec_stat.p, P->h_held.p + 1, sizeof(unsigned long long) * 32, hipMemcpyHostToDevice));
  P->bwd_pending = false; P->held_launches = 0;
}

// Zero messages (MRFEnergy.cpp:115-133), labels, flags and every piece of iteration state.
void reset_state(stereo_trws_plan *P) {
  discard_backward_ahead(P);
  STEREO_HIP_CHECK(hipMemset(P->d_msg.p, 0, sizeof(double) * (size_t)P->El * P->K));
  STEREO_HIP_CHECK(hipMemset(P->d_x.p, 0, sizeof(int32_t) * P->Nl));
  STEREO_HIP_CHECK(hipMemset(P->d_done.p, 0, sizeof(int32_t) * P->d_done.n));
  if (P->d_gran.p) STEREO_HIP_CHECK(hipMemset(P->d_gran.p, 0, sizeof(unsigned long long) * P->d_gran.n));   // (tags: epochs restart)
  if (P->d_xgran.p) STEREO_HIP_CHECK(hipMemset(P->d_xgran.p, 0, sizeof(unsigned long long) * P->d_xgran.n));
  STEREO_HIP_CHECK(hipMemset(P->d_ctl.p, 0, sizeof(int32_t) * kCtlWords));
  STEREO_HIP_CHECK(hipDeviceSynchronize());
  P->iterations = 0; P->energy = 0; P->lb = 0; P->epoch = 0; P->fwd_pending = false;
  P->lb_in_flight = false; P->issued = false; P->mm_ready = false; P->state_loaded_at = -1;
}

namespace {

void finish_inputs(stereo_trws_plan *P) {
  // New inputs start a new minimisation: the forward sweep of the next iteration has usually run
  // already with the OLD inputs (the fused launch of issue_iteration), so the
  // messages on the device belong to no state the reference could be in with the new ones.
  if (P->iterations > 0 || P->fwd_pending) reset_state(P);
  // one shared positions vector that is finite and strictly ascending opens the wide and the large family
  std::vector<double> hp;
  const bool asc = P->pos && positions_ascend(P->pos, P->K, hp);
  const TrwsInputFacts in{P->pos != nullptr, asc, P->lambda};
  const char *why = nullptr;
  const TrwsFamily family = trws_family(P->facts, &in, &why);
  if (family == TrwsFamily::None) {
    P->family = trws_family(P->facts, nullptr, &why);
    if (P->family == TrwsFamily::Large) P->have_inputs = false;   // (no family to fall back to)
    throw HipError{why};
  }
  sort_positions(P);
  P->family = family;
  P->uniform_step = 0; P->pos_ascending = false; P->window = 0; P->spec_window = false;
  P->pos_first = P->pos_last = P->pos_gap = 0;   // (of the positions before: a plan keeps its state across uploads now)
  const bool windowed = asc && P->lambda >= 0;
  if (windowed || family == TrwsFamily::Large) {
    P->pos_first = hp[0]; P->pos_last = hp[P->K - 1];
    P->pos_gap = std::numeric_limits<double>::infinity();
    for (int k = 1; k < P->K; ++k) P->pos_gap = std::min(P->pos_gap, hp[k] - hp[k - 1]);
  }
  if (windowed) analyse_window(P, hp);
  P->have_inputs = true;
}

// What stereo_trws_plan_upload and the two bind entries check alike; *shared: one positions vector instead of q / qprim.
int check_inputs(const char *who, const stereo_trws_plan *P, const double *unary, const double *q, const double *qprim,
                 const double *positions, const double *alphas, double tol, bool *shared, char *err, size_t errcap) {
  if (!P || !unary || !alphas) return fail(std::string(who) + ": NULL argument", err, errcap);
  *shared = (q == nullptr && qprim == nullptr);
  if (*shared && !positions) return fail(std::string(who) + ": need q/qprim or positions", err, errcap);
  if (!*shared && (!q || !qprim)) return fail(std::string(who) + ": q and qprim must both be given", err, errcap);
  // what no family takes even with the best of positions is refused before anything is copied
  const TrwsInputFacts at_best{*shared, *shared, tol};
  const char *why = nullptr;
  if (trws_family(P->facts, &at_best, &why) == TrwsFamily::None) return fail(why, err, errcap);
  return 0;
}

void set_inputs(stereo_trws_plan *P, const double *unary, const double *q, const double *qprim, const double *positions,
                const double *alphas, bool shared, double tol) {
  P->unary = unary; P->alpha = alphas; P->lambda = tol;
  P->pos = shared ? positions : nullptr;
  P->q = shared ? nullptr : q; P->qprim = shared ? nullptr : qprim;
}
}  // namespace
}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_hip_abi_version(void) { return STEREO_HIP_ABI_VERSION; }

int stereo_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

__global__ void warm_up_kernel() {}

int stereo_hip_warm_up(void) {
  if (stereo_hip_device_count() < 1) return 1;
  if (hipFree(nullptr) != hipSuccess) return 1;
  hipLaunchKernelGGL(warm_up_kernel, dim3(1), dim3(64), 0, 0);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  // every runtime service the QPBO path uses (cooperative launch, occupancy query, function
  // attributes, the Improve kernels) once, on a frustrated triangle that stays unlabelled
  const double U[3] = {0, 0, 0}, same[3] = {1, 1, 1}, diff[3] = {0, 0, 0};
  const uint32_t conn[6] = {0, 1, 1, 2, 2, 0};
  double lab[3], en = 0, lb = 0, nu = 0;
  char err[256];
  return stereo_rd(U, U, same, diff, diff, same, conn, 3, 3, 1, lab, &en, &lb, &nu, err, sizeof(err));
}

int stereo_hip_device_cus(void) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}

int stereo_hip_set_device(int device) {
  if (hipSetDevice(device) != hipSuccess) {
    last_error() = "hipSetDevice failed";
    return 1;
  }
  return 0;
}

const char *stereo_hip_last_error(void) { return last_error().c_str(); }

int stereo_trws_plan_upload(stereo_trws_plan *P, const double *unary, const double *q,
                            const double *qprim, const double *positions, const double *alphas,
                            double tol, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  bool shared = false;
  if (int rc = check_inputs("stereo_trws_plan_upload", P, unary, q, qprim, positions, alphas, tol, &shared, err, errcap)) return rc;
  try {
    discard_backward_ahead(P);   // (it still reads the inputs that are about to be overwritten)
    const size_t K = P->K;
    // a strip keeps the rows of its own nodes + halo and of the edges with an own endpoint
    std::vector<double> part;
    auto rows = [&](const double *full, const std::vector<int32_t> &ids, size_t width) {
      part.resize(ids.size() * width);
      for (size_t i = 0; i < ids.size(); ++i) std::memcpy(&part[i * width], full + (size_t)ids[i] * width, sizeof(double) * width);
      return part.data();
    };
    const bool local = P->nstrips > 1;
    P->o_unary.upload(local ? rows(unary, P->layout->nodes, K) : unary, (size_t)P->Nl * K);
    P->o_alpha.upload(local ? rows(alphas, P->layout->edges, 1) : alphas, (size_t)P->El);
    if (shared) {
      P->o_pos.upload(positions, K);
      P->o_q.release(); P->o_qprim.release();
    } else {
      P->o_q.upload(local ? rows(q, P->layout->edges, K) : q, (size_t)P->El * K);
      P->o_qprim.upload(local ? rows(qprim, P->layout->edges, K) : qprim, (size_t)P->El * K);
    }
    set_inputs(P, P->o_unary.p, P->o_q.p, P->o_qprim.p, P->o_pos.p, P->o_alpha.p, shared, tol);
    finish_inputs(P);
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

// strip_local: the arrays are strip-local already (stereo_trws_plan_bind_device_strip); otherwise they cover the whole
// problem and a strip gathers its rows into arrays of its own (the caller may free the full ones afterwards)
static int bind_device(const char *who, bool strip_local, stereo_trws_plan *P, const double *d_unary, const double *d_q,
                       const double *d_qprim, const double *d_positions, const double *d_alphas, double tol, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  bool shared = false;
  if (int rc = check_inputs(who, P, d_unary, d_q, d_qprim, d_positions, d_alphas, tol, &shared, err, errcap)) return rc;
  try {
    discard_backward_ahead(P);   // (nothing reads the arrays bound before once this call has returned)
    if (P->nstrips > 1 && !strip_local) {
      auto rows = [&](const double *full, DevBuf<double> &own, const DevBuf<int64_t> &ids, int64_t n, int width) {
        own.alloc((size_t)n * width);
        gather_rows(full, ids.p, n, width, own.p);
        return (const double *)own.p;
      };
      d_unary = rows(d_unary, P->o_unary, P->d_lnodes, P->Nl, P->K);
      d_alphas = rows(d_alphas, P->o_alpha, P->d_ledges, P->El, 1);
      if (!shared) {
        d_q = rows(d_q, P->o_q, P->d_ledges, P->El, P->K);
        d_qprim = rows(d_qprim, P->o_qprim, P->d_ledges, P->El, P->K);
      }
      STEREO_HIP_CHECK(hipDeviceSynchronize());
    }
    set_inputs(P, d_unary, d_q, d_qprim, d_positions, d_alphas, shared, tol);
    finish_inputs(P);
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_bind_device(stereo_trws_plan *P, const double *d_unary, const double *d_q,
                                 const double *d_qprim, const double *d_positions,
                                 const double *d_alphas, double tol, char *err, size_t errcap) {
  return bind_device("stereo_trws_plan_bind_device", false, P, d_unary, d_q, d_qprim, d_positions, d_alphas, tol, err, errcap);
}

int stereo_trws_plan_bind_device_strip(stereo_trws_plan *P, const double *d_unary, const double *d_q,
                                       const double *d_qprim, const double *d_positions,
                                       const double *d_alphas, double tol, char *err, size_t errcap) {
  return bind_device("stereo_trws_plan_bind_device_strip", true, P, d_unary, d_q, d_qprim, d_positions, d_alphas, tol, err, errcap);
}

int stereo_trws_plan_strip_layout(stereo_trws_plan *P, int64_t *n_nodes, int64_t *n_own, int64_t *n_edges,
                                  int32_t *nodes, int32_t *edges) {
  if (!P) return 1;
  if (n_nodes) *n_nodes = P->Nl;
  if (n_own) *n_own = P->n_en;
  if (n_edges) *n_edges = P->El;
  for (int64_t i = 0; nodes && i < P->Nl; ++i) nodes[i] = P->layout ? P->layout->nodes[i] : (int32_t)i;
  for (int64_t e = 0; edges && e < P->El; ++e) edges[e] = P->layout ? P->layout->edges[e] : (int32_t)e;
  return 0;
}

int stereo_trws_plan_reset(stereo_trws_plan *P, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_reset: NULL plan", err, errcap);
  try {
    reset_state(P);
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

// Waits for the iteration issued last and sums its lower-bound and energy terms in the
// reference's order (minimize.cpp:82,92 and :260): sequential, bit exact.  Returns false if a
// sweep gave up waiting on a dependency flag.
static bool collect_iteration(stereo_trws_plan *P, hipStream_t s, double *lb_out, double *en_out) {
  double lb = 0, en = 0;
  if (P->lb_in_flight) {  // summed while the forward sweep + primal launch is still running
    STEREO_HIP_CHECK(hipEventSynchronize(P->ev_lb));
    for (int64_t i = 0; i < P->n_lb; ++i) lb += P->h_lb.p[i];
  }
  // (with the next backward sweep behind it on the stream, the iteration's own end)
  if (P->bwd_pending) STEREO_HIP_CHECK(hipEventSynchronize(P->ev_end)); else STEREO_HIP_CHECK(hipStreamSynchronize(s));
  P->issued = false;
  if (P->h_ctl.p[1]) return false;
  if (P->time_sweeps && (!P->timed_by || P->timed_by->time_sweeps)) {
    float ms = 0;
    stereo_trws_plan *T = P->timed_by ? P->timed_by : P;
    STEREO_HIP_CHECK(hipEventElapsedTime(&ms, T->ev0, T->ev1));
    P->sweep_ms += ms;
  }
  if (!P->lb_in_flight)
    for (int64_t i = 0; i < P->n_lb; ++i) lb += P->h_lb.p[i];
  P->lb_in_flight = false;
  for (int64_t i = 0; i < P->n_en; ++i) en += P->h_en.p[i];
  *lb_out = lb; *en_out = en;
  return true;
}

// What a sweep that gave up says (h_ctl[2..5] = report_give_up's words; all zero when the give-up came
// from a wait inside a workgroup, which has no report).
static std::string gave_up_text(const stereo_trws_plan *P) {
  const int32_t *c = P->h_ctl.p;
  char b[512];
  const double secs = (double)P->spin_ticks / 1e8;
  if (c[2] == 0 && c[3] == 0 && c[4] == 0 && c[5] == 0) {
    std::snprintf(b, sizeof(b), "stereo_trws: a persistent sweep gave up waiting on a dependency flag (strip %d of %d, device %d)",
                  P->strip, P->nstrips, P->device);
  } else {
    const bool halo = P->layout && (int64_t)c[3] >= P->layout->n_own;  // (strip-local ids: own nodes first, then the halo)
    std::snprintf(b, sizeof(b), "stereo_trws: a persistent sweep gave up waiting on a dependency flag: strip %d of %d (device %d), "
                  "the visit of rank %d waited %.0f s for the completion flag of rank %d (found %d, expected epoch %d)%s",
                  P->strip, P->nstrips, P->device, c[2], secs, c[3], c[4], c[5],
                  halo ? " -- a node of the NEIGHBOURING strip: is that strip's process / launch running?" : "");
  }
  return b;
}

static int strip_ready(stereo_trws_plan *P, const char *who, char *err, size_t errcap) {
  if (!P) return fail(std::string(who) + ": NULL plan", err, errcap);
  if (!P->have_inputs) return fail(std::string(who) + ": no inputs uploaded/bound", err, errcap);
  for (int w = 0; w < 2; ++w)
    if (P->need_peer[w] && !(P->peer_msg[w] && P->peer_done[w] && P->peer_x[w]))
      return fail(std::string(who) + ": strip is not connected to its " + (w ? "next" : "previous") + " neighbour", err, errcap);
  return 0;
}

// The parameters of a plan's OWN launches (speculative schedule included), with the block once more in global memory:
// chain_runner / spec_commit and, in the K <= 64 kernels, every role of every launch (trws_pipe.hip) read their parameters
// there; sent when it changes.  The copy is a blocking hipMemcpy and does not wait for a sweep issued ahead on a
// non-blocking stream (issue_backward_ahead).  The last iteration of an iterate call issues nothing ahead; a call that
// stops early on its gap leaves a sweep issued, and a block that CHANGES before the next call (another switch in the
// environment, other inputs) would then be rewritten under that sweep -- as it always could under the speculative
// runner; the block of an unchanged plan compares equal and is not sent again.
static DevParams own_params(stereo_trws_plan *P, bool allow_sub = true) {
  const DevParams p = make_params(P, true, allow_sub);
  if (!P->self_sent || std::memcmp(P->h_self.p, &p, sizeof(DevParams)) != 0) {
    std::memcpy(P->h_self.p, &p, sizeof(DevParams));
    STEREO_HIP_CHECK(hipMemcpy(P->d_self.p, P->h_self.p, sizeof(DevParams), hipMemcpyHostToDevice));
    P->self_sent = true;
  }
  return p;
}

int stereo_trws_plan_iterate(stereo_trws_plan *P, int iters, double max_relgap, void *stream,
                             int *done_iters, int *stopped, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_iterate: NULL plan", err, errcap);
  if (!P->have_inputs) return fail("stereo_trws_plan_iterate: no inputs uploaded/bound", err, errcap);
  if (P->nstrips > 1)
    return fail("stereo_trws_plan_iterate: a strip iterates through stereo_trws_plan_issue / _collect / _commit "
                "(its energy and bound are partial sums)", err, errcap);
  if (done_iters) *done_iters = 0;
  if (stopped) *stopped = 0;
  hipStream_t s = (hipStream_t)stream;
  try {
    const DevParams p = own_params(P);
    for (int it = 0; it < iters; ++it) {
      // another iteration is asked for: its backward sweep runs while the host sums this one's terms.  (Node beliefs
      // hang on the state between the two launches: a plan that keeps them waits.)
      const bool ahead = it + 1 < iters && !P->keep_mm && P->ahead_allowed;
      issue_iteration(&P, 1, s, true, [&](int what) { launch_persistent(P, p, what, s); }, ahead);
      if (ahead) issue_backward_ahead(P, p, s);
      double lb = 0, en = 0;
      if (!collect_iteration(P, s, &lb, &en)) { P->mm_ready = false; return fail(gave_up_text(P), err, errcap); }
      P->lb = lb; P->energy = en; P->iterations += 1;
      if (done_iters) *done_iters += 1;
      const double rel_gap = (en - lb) / en;  // minimize.cpp:105
      if (rel_gap < max_relgap) {
        if (stopped) *stopped = 1;
        break;
      }
    }
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plans_issue(stereo_trws_plan *const *plans, int n, void *stream, char *err, size_t errcap) {
  DeviceScope device_scope_(plans && n > 0 && plans[0] ? plans[0]->device : -1);
  if (!plans || n < 1 || n > kMaxGroup) return fail("stereo_trws_plans_issue: need 1 .. 16 plans", err, errcap);
  for (int i = 0; i < n; ++i) {
    if (int rc = strip_ready(plans[i], "stereo_trws_plans_issue", err, errcap)) return rc;
    stereo_trws_plan *P = plans[i], *P0 = plans[0];
    if (P->issued) return fail("stereo_trws_plans_issue: the previous iteration has not been collected", err, errcap);
    if (P->device != P0->device || P->graph != P0->graph || P->K != P0->K || P->kernel != P0->kernel ||
        P->epoch != P0->epoch || P->fwd_pending != P0->fwd_pending || P->bwd_pending != P0->bwd_pending || P->family != P0->family ||
        (P->pos == nullptr) != (P0->pos == nullptr) || P->mode != P0->mode)
      return fail("stereo_trws_plans_issue: the plans are not strips of one problem on one device in the same state", err, errcap);
    if (!pipelined(P->family))
      return fail("stereo_trws_plans_issue: strips run on the pipelined kernels only (K <= 64; K <= 128 with per-edge "
                  "positions; K <= 256 with shared ascending positions)", err, errcap);
  }
  try {
    stereo_trws_plan *P0 = plans[0];
    hipStream_t s = stream ? (hipStream_t)stream : P0->own_stream;
    if (!s) return fail("stereo_trws_plans_issue: a plain plan needs an explicit stream here", err, errcap);
    if (P0->d_group.n < (size_t)n) { P0->d_group.alloc(kMaxGroup); P0->h_group.alloc(kMaxGroup); }
    for (int i = 0; i < n; ++i) P0->h_group.p[i] = make_params(plans[i], false);   // (group launches keep the plain chain schedule)
    STEREO_HIP_CHECK(hipMemcpyAsync(P0->d_group.p, P0->h_group.p, sizeof(DevParams) * n, hipMemcpyHostToDevice, s));
    issue_iteration(plans, n, s, true, [&](int what) { launch_group(plans, n, what, s); });
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_issue(stereo_trws_plan *P, void *stream, char *err, size_t errcap) {
  return stereo_trws_plans_issue(&P, 1, stream, err, errcap);
}

int stereo_trws_plan_collect(stereo_trws_plan *P, double *lb_part, double *energy_part, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_collect: NULL plan", err, errcap);
  if (!P->issued) return fail("stereo_trws_plan_collect: nothing was issued", err, errcap);
  try {
    double lb = 0, en = 0;
    if (!collect_iteration(P, P->issue_stream, &lb, &en)) { P->mm_ready = false; return fail(gave_up_text(P), err, errcap); }
    if (lb_part) *lb_part = lb;
    if (energy_part) *energy_part = en;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_commit(stereo_trws_plan *P, double lower_bound, double energy, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_commit: NULL plan", err, errcap);
  P->lb = lower_bound; P->energy = energy; P->iterations += 1;
  return 0;
}

// ---- batches: independent plans that share the launches of a sweep ----------------------------------

// the admission rule (trws_batch.h) on the members as they are NOW: at creation, and again before every iteration --
// an upload may have moved a member to another kernel family since
static int batch_admit(const char *who, stereo_trws_plan *const *plans, int n, char *err, size_t errcap) {
  TrwsBatchMember facts[kBatchMaxMembers];
  for (int i = 0; plans && i < n && i < kBatchMaxMembers; ++i) {
    const stereo_trws_plan *P = plans[i];
    TrwsBatchMember &f = facts[i];
    f.present = P != nullptr;
    if (!P) continue;
    for (int j = 0; j < i; ++j) f.repeated = f.repeated || plans[j] == P;
    f.nstrips = P->nstrips; f.have_inputs = P->have_inputs; f.family = P->family; f.kernel = P->kernel;
    f.exact = P->mode == STEREO_TRWS_MESSAGES_EXACT; f.shared = P->pos != nullptr; f.device = P->device;
  }
  std::string why;
  if (trws_batch_admit(plans ? facts : nullptr, n, &why) >= 0) return fail(std::string(who) + ": " + why, err, errcap);
  return 0;
}

int stereo_trws_batch_create(stereo_trws_plan *const *plans, int n, stereo_trws_batch **out, char *err, size_t errcap) {
  if (!out) return fail("stereo_trws_batch_create: NULL argument", err, errcap);
  *out = nullptr;
  if (int rc = batch_admit("stereo_trws_batch_create", plans, n, err, errcap)) return rc;
  DeviceScope device_scope_(plans[0]->device);
  try {
    std::unique_ptr<stereo_trws_batch> B(new stereo_trws_batch);
    B->members.assign(plans, plans + n);
    B->stopped.assign(n, 0);
    B->device = plans[0]->device;
    // what stays resident together: the K <= 64 kernel as often per compute unit as the device says, the others once
    const stereo_trws_plan *P0 = plans[0];
    B->capacity = P0->cus * (P0->family == TrwsFamily::Pipe ? pipe_batch_resident_per_cu(P0->kernel, P0->pos != nullptr) : 1);
    // (development, as for a single plan's launch: fewer workgroups -- members then share them, and the K <= 64 kernel's float)
    if (const char *be = std::getenv("STEREO_HIP_TRWS_BLOCKS"))
      if (std::atoi(be) > 0) B->capacity = std::min(B->capacity, std::atoi(be));
    B->d_table.alloc(3 * kMaxGroup); B->h_table.alloc(3 * kMaxGroup);
    B->d_ctl.alloc(kBatchCtlWords);
    STEREO_HIP_CHECK(hipMemset(B->d_ctl.p, 0, sizeof(unsigned long long) * kBatchCtlWords));
    *out = B.release();
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

void stereo_trws_batch_destroy(stereo_trws_batch *B) {
  DeviceScope device_scope_(B ? B->device : -1);
  delete B;
}

int stereo_trws_batch_iterate(stereo_trws_batch *B, int iters, double max_relgap, int32_t *done_iters, char *err, size_t errcap) {
  if (!B) return fail("stereo_trws_batch_iterate: NULL batch", err, errcap);
  DeviceScope device_scope_(B->device);
  const int n = (int)B->members.size();
  for (int i = 0; done_iters && i < n; ++i) done_iters[i] = 0;
  if (int rc = batch_admit("stereo_trws_batch_iterate", B->members.data(), n, err, errcap)) return rc;
  for (int i = 0; i < n; ++i)
    if (B->members[i]->issued)
      return fail("stereo_trws_batch_iterate: member " + std::to_string(i) + " has an issued iteration that has not been collected", err, errcap);
  hipStream_t s = nullptr;
  try {
    // (batches keep the plain chain schedule, like the strip groups)
    DevParams all[kMaxGroup], own[kMaxGroup];
    for (int i = 0; i < n; ++i) { all[i] = make_params(B->members[i], false); own[i] = own_params(B->members[i], false); }
    for (int it = 0; it < iters; ++it) {
      stereo_trws_plan *G[kMaxGroup];
      DevParams params[kMaxGroup];
      int index[kMaxGroup], m = 0;
      for (int i = 0; i < n; ++i)
        if (!B->stopped[i]) { G[m] = B->members[i]; params[m] = all[i]; index[m++] = i; }
      if (m == 0) break;
      // Where the shared launch is known to lose (measured), the members take their own launches one after
      // the other -- the single plan's path, speculative schedule included; same bits either way: a batch of one, and
      // fewer than kBatchLargeMin members of the K <= 64 family that each fill the device alone (more runs than
      // resident workgroups: nothing idles for the others to use).
      bool own_launches = m == 1;
      if (!own_launches && G[0]->family == TrwsFamily::Pipe && m < kBatchLargeMin) {
        own_launches = true;
        for (int j = 0; j < m; ++j) own_launches = own_launches && G[j]->grid_blocks >= B->capacity;
      }
      if (!own_launches) issue_iteration(G, m, s, true, [&](int what) { launch_batch(B, G, params, m, what, s); });
      // every member commits its own sums, taken in the single plan's order; all are collected before any is reported
      int gave_up = -1;
      for (int j = 0; j < m; ++j) {
        stereo_trws_plan *P = G[j];
        if (own_launches) issue_iteration(&P, 1, s, true, [&](int what) { launch_persistent(P, own[index[j]], what, s); });
        double lb = 0, en = 0;
        if (!collect_iteration(P, s, &lb, &en)) { P->mm_ready = false; if (gave_up < 0) gave_up = j; continue; }
        P->lb = lb; P->energy = en; P->iterations += 1;
        if (done_iters) done_iters[index[j]] += 1;
        const double rel_gap = (en - lb) / en;  // minimize.cpp:105
        if (rel_gap < max_relgap) B->stopped[index[j]] = 1;
      }
      if (gave_up >= 0)
        return fail("stereo_trws_batch_iterate: member " + std::to_string(index[gave_up]) + ": " + gave_up_text(G[gave_up]), err, errcap);
    }
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_batch_reset(stereo_trws_batch *B, char *err, size_t errcap) {
  if (!B) return fail("stereo_trws_batch_reset: NULL batch", err, errcap);
  DeviceScope device_scope_(B->device);
  try {
    for (stereo_trws_plan *P : B->members) reset_state(P);
    std::fill(B->stopped.begin(), B->stopped.end(), 0);
    STEREO_HIP_CHECK(hipMemset(B->d_ctl.p, 0, sizeof(unsigned long long) * kBatchCtlWords));
    B->launches = 0;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_batch_stats(stereo_trws_batch *B, int64_t out[4]) {
  if (!B || !out) return 1;
  DeviceScope device_scope_(B->device);
  unsigned long long v[kBatchCtlWords] = {0};
  if (hipMemcpy(v, B->d_ctl.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  out[0] = (int64_t)v[0]; out[1] = B->launches; out[2] = 0; out[3] = B->capacity;
  return 0;
}

int stereo_trws_plan_connect(stereo_trws_plan *P, int which, stereo_trws_plan *peer, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P || !peer || (which != 0 && which != 1)) return fail("stereo_trws_plan_connect: bad argument", err, errcap);
  if (P->N != peer->N || P->E != peer->E || P->K != peer->K || P->nstrips != peer->nstrips ||
      peer->strip != P->strip + (which ? 1 : -1))
    return fail("stereo_trws_plan_connect: the peer is not the neighbouring strip of the same problem", err, errcap);
  try {
    if (peer->device != P->device) {  // one process driving several GPUs: map the neighbour's memory
      int can = 0;
      STEREO_HIP_CHECK(hipDeviceCanAccessPeer(&can, P->device, peer->device));
      if (!can) return fail("stereo_trws_plan_connect: no peer access between the two devices", err, errcap);
      int cur = 0;
      STEREO_HIP_CHECK(hipGetDevice(&cur));
      STEREO_HIP_CHECK(hipSetDevice(P->device));
      const hipError_t e = hipDeviceEnablePeerAccess(peer->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) STEREO_HIP_CHECK(e);
      (void)hipGetLastError();
      STEREO_HIP_CHECK(hipSetDevice(cur));
    }
    P->peer_msg[which] = peer->d_msg.p; P->peer_done[which] = peer->d_done.p; P->peer_x[which] = peer->d_x.p;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_ipc_export(stereo_trws_plan *P, void *handles, size_t cap, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P || !handles) return fail("stereo_trws_plan_ipc_export: NULL argument", err, errcap);
  if (cap < STEREO_TRWS_IPC_BYTES) return fail("stereo_trws_plan_ipc_export: buffer smaller than STEREO_TRWS_IPC_BYTES", err, errcap);
  static_assert(3 * sizeof(hipIpcMemHandle_t) <= STEREO_TRWS_IPC_BYTES, "STEREO_TRWS_IPC_BYTES");
  try {
    hipIpcMemHandle_t h[3];
    STEREO_HIP_CHECK(hipIpcGetMemHandle(&h[0], P->d_msg.p));
    STEREO_HIP_CHECK(hipIpcGetMemHandle(&h[1], P->d_done.p));
    STEREO_HIP_CHECK(hipIpcGetMemHandle(&h[2], P->d_x.p));
    std::memset(handles, 0, STEREO_TRWS_IPC_BYTES);
    std::memcpy(handles, h, sizeof(h));
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_ipc_connect(stereo_trws_plan *P, int which, const void *handles, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P || !handles || (which != 0 && which != 1)) return fail("stereo_trws_plan_ipc_connect: bad argument", err, errcap);
  try {
    hipIpcMemHandle_t h[3];
    std::memcpy(h, handles, sizeof(h));
    void *ptr[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) {
      if (P->ipc_mapped[which][k]) { (void)hipIpcCloseMemHandle(P->ipc_mapped[which][k]); P->ipc_mapped[which][k] = nullptr; }
      STEREO_HIP_CHECK(hipIpcOpenMemHandle(&ptr[k], h[k], hipIpcMemLazyEnablePeerAccess));
      P->ipc_mapped[which][k] = ptr[k];
    }
    P->peer_msg[which] = (double *)ptr[0]; P->peer_done[which] = (int32_t *)ptr[1]; P->peer_x[which] = (int32_t *)ptr[2];
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_strip_info(stereo_trws_plan *P, int *nstrips, int *strip, int64_t *own_nodes, int64_t *runs_forward,
                                int64_t *runs_backward, int *needs_previous, int *needs_next) {
  if (!P) return 1;
  if (nstrips) *nstrips = P->nstrips;
  if (strip) *strip = P->strip;
  if (own_nodes) *own_nodes = P->n_en;
  // (a whole problem: the runs its own launches walk -- the sub-row runs where it has them)
  auto own_runs = [&](int d) {
    const stereo::TrwsGraph::Sweep &S = P->graph->sweep[d];
    return (int64_t)(own_sub_rows(P, d) ? S.chunked.run_ptr.size() : S.chain_run_ptr.size()) - 1;
  };
  if (runs_forward) *runs_forward = P->nstrips > 1 ? P->ntickets[0] : own_runs(0);
  if (runs_backward) *runs_backward = P->nstrips > 1 ? P->ntickets[1] : own_runs(1);
  if (needs_previous) *needs_previous = P->need_peer[0] ? 1 : 0;
  if (needs_next) *needs_next = P->need_peer[1] ? 1 : 0;
  return 0;
}

int stereo_trws_plan_result(stereo_trws_plan *P, double *labelling, double *energy,
                            double *lower_bound, double *iterations, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_result: NULL plan", err, errcap);
  try {
    if (labelling) {
      STEREO_HIP_CHECK(hipMemcpy(P->h_x.p, P->d_x.p, sizeof(int32_t) * P->Nl, hipMemcpyDeviceToHost));
      if (P->layout) {  // a strip: its own nodes and halo; label 1 elsewhere
        for (int64_t i = 0; i < P->N; ++i) labelling[i] = 1.0;
        for (int64_t i = 0; i < P->Nl; ++i) labelling[P->layout->nodes[i]] = (double)(P->h_x.p[i] + 1);
      } else
      for (int64_t i = 0; i < P->N; ++i) labelling[i] = (double)(P->h_x.p[i] + 1);  // trws_mex.cpp:137
    }
    if (energy) *energy = P->energy;
    if (lower_bound) *lower_bound = P->lb;
    if (iterations) *iterations = (double)P->iterations;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_info(stereo_trws_plan *P, int64_t *rank, int64_t *levels,
                          int64_t *max_level_nodes, char *err, size_t errcap) {
  if (!P) return fail("stereo_trws_plan_info: NULL plan", err, errcap);
  if (rank) for (int64_t i = 0; i < P->N; ++i) rank[i] = P->graph->rank[i];
  if (levels) *levels = (int64_t)P->graph->level_ptr.size() - 1;
  if (max_level_nodes) *max_level_nodes = P->graph->max_level_nodes;
  return 0;
}

int stereo_trws_plan_path(stereo_trws_plan *P) {
  if (!P) return -1;
  return (int)P->family;
}

// the flag on a whole-problem plan or on a strip (who: the entry's name)
static int keep_min_marginals_impl(stereo_trws_plan *P, const char *who, int on, char *err, size_t errcap) {
  auto release = [&] {
    P->d_belief.release();
    P->d_bel_own.release(); P->d_bel_fptr.release(); P->d_bel_fidx.release(); P->d_bel_bptr.release(); P->d_bel_bidx.release();
    P->d_bel_table.release(); P->bel_sent_n[0] = P->bel_sent_n[1] = 0;
  };
  if (!on) {
    P->keep_mm = false; P->mm_ready = false;
    release();
    return 0;
  }
  if (P->keep_mm) return 0;
  if (P->issued) return fail(std::string(who) + ": the iteration issued last has not been collected", err, errcap);
  const size_t rows = P->layout ? (size_t)P->layout->n_own : (size_t)P->N;
  try {
    if (P->layout) {   // a strip: its own nodes by rank and their lists under strip-local ids
      StripBeliefLists B;
      std::string gerr;
      if (!build_strip_belief_lists(*P->graph, P->strip, P->layout->nodes, P->layout->edges, B, gerr)) return fail(gerr, err, errcap);
      P->d_bel_own.upload(B.own.data(), B.own.size());
      P->d_bel_fptr.upload(B.fptr.data(), B.fptr.size()); P->d_bel_fidx.upload(B.fidx.data(), B.fidx.size());
      P->d_bel_bptr.upload(B.bptr.data(), B.bptr.size()); P->d_bel_bidx.upload(B.bidx.data(), B.bidx.size());
      STEREO_HIP_CHECK(hipDeviceSynchronize());   // (the lists are host vectors of this scope)
    }
    P->d_belief.alloc(rows * P->K);
  } catch (const HipError &e) {
    release();
    return fail(std::string(who) + ": cannot allocate the " + std::to_string(8 * rows * P->K) +
                "-byte belief buffer (" + e.msg + ")", err, errcap);
  }
  P->keep_mm = true; P->mm_ready = false;
  return 0;
}

int stereo_trws_plan_keep_min_marginals(stereo_trws_plan *P, int on, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_keep_min_marginals: NULL plan", err, errcap);
  if (P->nstrips > 1)
    return fail("stereo_trws_plan_keep_min_marginals: a row strip has no min-marginals of the whole problem (a strip keeps those "
                "of its own nodes: stereo_trws_plan_strip_keep_min_marginals)", err, errcap);
  return keep_min_marginals_impl(P, "stereo_trws_plan_keep_min_marginals", on, err, errcap);
}

int stereo_trws_plan_strip_keep_min_marginals(stereo_trws_plan *P, int on, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return fail("stereo_trws_plan_strip_keep_min_marginals: NULL plan", err, errcap);
  return keep_min_marginals_impl(P, "stereo_trws_plan_strip_keep_min_marginals", on, err, errcap);
}

// what every read checks: the beliefs of the last iteration are there and nothing is in flight
static int beliefs_readable(const stereo_trws_plan *P, const char *who, char *err, size_t errcap) {
  if (!P->keep_mm || !P->mm_ready)
    return fail(std::string(who) + ": no min-marginals to read: turn them on with stereo_trws_plan_keep_min_marginals and "
                "iterate first (an upload, bind or reset discards them)", err, errcap);
  if (P->issued)
    return fail(std::string(who) + ": no min-marginals to read while an issued iteration has not been collected", err, errcap);
  return 0;
}

// strip: the entry takes a strip and returns its own nodes' rows (K x n_own, strip-local order)
static int min_marginals_impl(stereo_trws_plan *P, const char *who, double *mm, double *conf, int32_t *argmin, bool device,
                              bool strip, hipStream_t s, char *err, size_t errcap) {
  if (!P) return fail(std::string(who) + ": NULL plan", err, errcap);
  if (P->nstrips > 1 && !strip)
    return fail(std::string(who) + ": a row strip has no min-marginals of the whole problem (its own nodes' rows: "
                "stereo_trws_plan_strip_min_marginals, stereo_trws_plans_min_marginals_device)", err, errcap);
  if (int rc = beliefs_readable(P, who, err, errcap)) return rc;
  try {
    const BeliefLists L = belief_lists(P);
    const size_t KN = (size_t)L.n * P->K;
    if (device) {
      launch_beliefs_finish(P->d_belief.p, P->d_msg.p, L.order, L.bptr, L.bidx, P->K, L.n, mm, conf, argmin, s);
      return 0;
    }
    DevBuf<double> d_mm, d_conf;
    DevBuf<int32_t> d_arg;
    if (mm) d_mm.alloc(KN);
    if (conf) d_conf.alloc(L.n);
    if (argmin) d_arg.alloc(L.n);
    launch_beliefs_finish(P->d_belief.p, P->d_msg.p, L.order, L.bptr, L.bidx, P->K, L.n, d_mm.p, d_conf.p, d_arg.p, nullptr);
    if (mm) STEREO_HIP_CHECK(hipMemcpy(mm, d_mm.p, sizeof(double) * KN, hipMemcpyDeviceToHost));
    if (conf) STEREO_HIP_CHECK(hipMemcpy(conf, d_conf.p, sizeof(double) * L.n, hipMemcpyDeviceToHost));
    if (argmin) STEREO_HIP_CHECK(hipMemcpy(argmin, d_arg.p, sizeof(int32_t) * L.n, hipMemcpyDeviceToHost));
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int stereo_trws_plan_min_marginals(stereo_trws_plan *P, double *min_marginals, double *confidence, int32_t *argmin, char *err,
                                   size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  return min_marginals_impl(P, "stereo_trws_plan_min_marginals", min_marginals, confidence, argmin, false, false, nullptr, err, errcap);
}

int stereo_trws_plan_min_marginals_device(stereo_trws_plan *P, double *d_min_marginals, double *d_confidence,
                                          int32_t *d_argmin, void *stream, char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  return min_marginals_impl(P, "stereo_trws_plan_min_marginals_device", d_min_marginals, d_confidence, d_argmin, true, false,
                            (hipStream_t)stream, err, errcap);
}

int stereo_trws_plan_strip_min_marginals(stereo_trws_plan *P, double *min_marginals, double *confidence, int32_t *argmin,
                                         char *err, size_t errcap) {
  DeviceScope device_scope_(P ? P->device : -1);
  return min_marginals_impl(P, "stereo_trws_plan_strip_min_marginals", min_marginals, confidence, argmin, false, true, nullptr, err, errcap);
}

int stereo_trws_plans_min_marginals_device(stereo_trws_plan *const *plans, int n, double *d_min_marginals, double *d_confidence,
                                           int32_t *d_argmin, void *stream, char *err, size_t errcap) {
  const char *who = "stereo_trws_plans_min_marginals_device";
  DeviceScope device_scope_(plans && n > 0 && plans[0] ? plans[0]->device : -1);
  if (!plans || n < 1 || n > kMaxGroup) return fail(std::string(who) + ": need 1 .. 16 plans", err, errcap);
  for (int i = 0; i < n; ++i) {
    const stereo_trws_plan *P = plans[i], *P0 = plans[0];
    if (!P) return fail(std::string(who) + ": NULL plan", err, errcap);
    for (int j = 0; j < i; ++j)
      if (plans[j] == P) return fail(std::string(who) + ": a plan is named twice", err, errcap);
    if (P->device != P0->device || P->graph != P0->graph || P->K != P0->K || P->nstrips != P0->nstrips)
      return fail(std::string(who) + ": the plans are not strips of one problem on one device", err, errcap);
    if (int rc = beliefs_readable(P, who, err, errcap)) return rc;
  }
  try {
    hipStream_t s = (hipStream_t)stream;
    stereo_trws_plan *P0 = plans[0];
    if (n == 1) {
      const BeliefLists L = belief_lists(P0);
      if (P0->layout)
        launch_beliefs_finish_map(P0->d_belief.p, P0->d_msg.p, L.order, L.bptr, L.bidx, P0->d_lnodes.p, P0->K, L.n, d_min_marginals,
                                  d_confidence, d_argmin, s);
      else
        launch_beliefs_finish(P0->d_belief.p, P0->d_msg.p, L.order, L.bptr, L.bidx, P0->K, L.n, d_min_marginals, d_confidence, d_argmin, s);
      return 0;
    }
    launch_beliefs_finish_group(belief_group(plans, n, 2), d_min_marginals, d_confidence, d_argmin, s);
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

}  // extern "C"
