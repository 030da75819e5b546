// TRW-S plan creation: the shared graph analysis, the device copies of the graph and of its schedules, every
// buffer a plan owns; and its destruction.  File map: trws_plan.hip.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "trws_plan.h"
#include "trws_runner_records.h"

namespace stereo {
namespace {

// The analysis depends on the connectivity only (ordering, lists, schedules: 0.2-0.6 s at Teddy
// size); consecutive plans for the same image grid -- every trws() call of a fusion loop --
// share the last one.
struct GraphKey {
  int64_t N = -1, E = -1;
  const uint32_t *conn = nullptr;   // the caller's arrays in a key made for a lookup, the cache's copies in the one it keeps
  TrwsGraphOptions opt;             // (opt.owner likewise; read only with more than one strip)
  bool operator==(const GraphKey &o) const {
    return N == o.N && E == o.E && opt == o.opt && std::memcmp(conn, o.conn, sizeof(uint32_t) * 2 * (size_t)E) == 0 &&
           (opt.nstrips == 1 || std::memcmp(opt.owner, o.opt.owner, sizeof(int32_t) * (size_t)N) == 0);
  }
};

std::shared_ptr<const TrwsGraph> shared_graph_for(GraphKey key, std::string &gerr) {
  static std::mutex mutex;
  static struct { GraphKey key; std::vector<uint32_t> conn; std::vector<int32_t> owner; std::shared_ptr<const TrwsGraph> g; } cache;
  std::lock_guard<std::mutex> lock(mutex);
  if (cache.g && cache.key == key) return cache.g;
  auto fresh = std::make_shared<TrwsGraph>();
  if (!build_trws_graph(key.N, key.E, key.conn, key.opt, *fresh, gerr)) return nullptr;
  cache.g.reset();
  if (key.N <= (1 << 23)) {  // (3000 x 2000: 3 GB of descriptors stay in host memory until the next connectivity)
    cache.conn.assign(key.conn, key.conn + 2 * (size_t)key.E);
    if (key.opt.nstrips > 1) cache.owner.assign(key.opt.owner, key.opt.owner + key.N); else cache.owner.clear();
    cache.key = key; cache.key.conn = cache.conn.data(); cache.key.opt.owner = cache.owner.data();
    cache.g = fresh;
  } else {
    cache.conn.clear(); cache.owner.clear();
  }
  return fresh;
}

}  // namespace

const int32_t *runner_records(stereo_trws_plan *P, int d, bool sub) {
  const TrwsGraph::Sweep &S = P->graph->sweep[d];
  const TrwsGraph::Sweep::Spec &sp = sub ? S.chunked.spec : S.spec, &s0 = P->graph->sweep[0].spec;
  const int32_t geom[4] = {sp.c0, sp.c1, s0.seg_len, s0.nseg};
  DevBuf<int32_t> &buf = P->d_run_rec[d][sub ? 1 : 0];
  if (!buf.p || std::memcmp(geom, P->run_rec_geom[d][sub ? 1 : 0], sizeof(geom)) != 0) {
    std::vector<int32_t> rec;
    build_runner_records((sub ? S.chunked.desc : S.desc).data(), geom[0], geom[1], geom[2], geom[3], rec);
    buf.upload(rec.data(), rec.size());
    STEREO_HIP_CHECK(hipStreamSynchronize(nullptr));   // (`rec` goes away)
    std::memcpy(P->run_rec_geom[d][sub ? 1 : 0], geom, sizeof(geom));
  }
  return buf.p;
}

}  // namespace stereo

using namespace stereo;

extern "C" {

static int plan_create_impl(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn, int message_mode,
                            const int32_t *owner, int nstrips, int strip, int max_blocks,
                            stereo_trws_plan *share, bool strip_api, stereo_trws_plan **plan, char *err, size_t errcap) {
  if (!plan) return fail("stereo_trws_plan_create: plan is NULL", err, errcap);
  *plan = nullptr;
  if (nstrips < 1 || strip < 0 || strip >= nstrips) return fail("stereo_trws_plan_create: strip out of range", err, errcap);
  if (nstrips > 1 && !owner && !share) return fail("stereo_trws_plan_create: strips need an owner per node", err, errcap);
  if (kernel != 1 && kernel != 2) return fail("Unsupported kernel", err, errcap);
  const int ordering = (message_mode & STEREO_TRWS_ORDER_INDEX) ? 1 : 0;
  message_mode &= ~STEREO_TRWS_ORDER_INDEX;
  // What the rule (trws_family.h) allows at best: the resident-workgroup capacity is needed before the graph exists.
  TrwsPlanFacts facts;
  facts.kernel = kernel; facts.K = K; facts.exact = message_mode == STEREO_TRWS_MESSAGES_EXACT; facts.fast_ok = true;
  const char *why = nullptr;
  const unsigned at_best = trws_families_possible(facts, &why);
  if (!at_best) return fail(why, err, errcap);
  if (message_mode != STEREO_TRWS_MESSAGES_EXACT && message_mode != STEREO_TRWS_MESSAGES_MINPLUS)
    return fail("stereo_trws: unknown message mode", err, errcap);
  if (stereo_hip_device_count() < 1)
    return fail("stereo_trws: no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  try {
    std::unique_ptr<stereo_trws_plan> P(new stereo_trws_plan);
    P->kernel = kernel; P->K = K; P->Kp = (K + 1) & ~1; P->mode = message_mode; P->N = N; P->E = E;
    P->nstrips = nstrips; P->strip = strip;
    P->order_flag = ordering ? STEREO_TRWS_ORDER_INDEX : 0;
    P->conn_key = conn ? trws_connectivity_key(conn, E) : share ? share->conn_key : 0;
    std::string gerr;
    // Workgroups that stay resident: runs beyond that are cut / dispensed by dependency level.  The
    // bound comes from the device in use (a partitioned or masked MI355X exposes fewer CUs): one
    // workgroup per CU is what is certain to be resident, LDS decides how many more fit.
    STEREO_HIP_CHECK(hipGetDevice(&P->device));
    {
      int cus = 0;
      STEREO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, P->device));
      P->cus = std::max(cus, 1);
    }
    const int plds = (int)persistent_lds_bytes(possible(at_best, TrwsFamily::Large), P->Kp);
    const int64_t per_cu = std::min<int64_t>(std::max<int64_t>(1, (int64_t)(160 * 1024) / (int64_t)plds), 4);
    const int64_t capacity = possible(at_best, TrwsFamily::Wide) ? P->cus : P->cus * per_cu;
    if (share) {
      // the strips of one process share one analysis (it is the same on every strip)
      if (!share->graph || share->N != N || share->E != E || share->graph->nstrips != nstrips)
        return fail("stereo_trws_plan_create: the plan to share the graph analysis with belongs to another problem", err, errcap);
      P->graph = share->graph;
    } else {
      GraphKey key;
      TrwsGraphOptions &opt = key.opt;
      key.N = N; key.E = E; key.conn = conn;
      opt.max_resident_runs = capacity; opt.certainly_resident = P->cus; opt.nstrips = nstrips; opt.ordering = ordering;
      opt.seg_len = spec_segment_length(); opt.owner = nstrips > 1 ? owner : nullptr;
      // Sub-row runs: for a whole problem the K <= 64 kernel may run, in the directions with more runs
      // than the launch is certain to keep resident -- elsewhere a run finds a workgroup of its own anyway.
      if (possible(at_best, TrwsFamily::Pipe) && nstrips == 1) {
        opt.row_chunk_forward = kRowChunkDefault[0]; opt.row_chunk_backward = kRowChunkDefault[1];
        if (const char *c = trws_switch(kSwRowChunk)) {
          opt.row_chunk_forward = opt.row_chunk_backward = std::max(0, std::atoi(c));
          if (const char *comma = std::strchr(c, ',')) opt.row_chunk_backward = std::max(0, std::atoi(comma + 1));
        }
        opt.chunk_resident = max_blocks > 0 ? std::min<int64_t>(P->cus, max_blocks) : P->cus;
        if (const char *be = std::getenv("STEREO_HIP_TRWS_BLOCKS"))
          if (std::atoi(be) > 0) opt.chunk_resident = std::min<int64_t>(opt.chunk_resident, std::atoi(be));
      }
      P->graph = shared_graph_for(key, gerr);
      if (!P->graph) return fail(gerr, err, errcap);
    }
    const TrwsGraph &g = *P->graph;
    P->Nl = N; P->El = E;
    // the families the plan may run, and the one it runs until its inputs say more
    facts.fast_ok = g.fast_ok; facts.strips = nstrips > 1;
    if (const char *f = trws_switch(kSwFast)) facts.fast_switch = std::string(f) != "0";
    P->facts = facts;
    P->families = trws_families_possible(facts, &why);
    if (!P->families) return fail(why, err, errcap);
    P->family = trws_family(facts, nullptr, &why);
    if (nstrips > 1) {
      P->layout.reset(new StripLayout);
      if (!build_strip_layout(g, strip, *P->layout, gerr)) return fail(gerr, err, errcap);
      const StripLayout &L = *P->layout;
      P->Nl = (int64_t)L.nodes.size(); P->El = (int64_t)L.edges.size();
      std::vector<int64_t> ids(L.nodes.begin(), L.nodes.end());
      P->d_lnodes.upload(ids.data(), ids.size());
      ids.assign(L.edges.begin(), L.edges.end());
      P->d_ledges.upload(ids.data(), ids.size());
      for (int d = 0; d < 2; ++d) {
        P->d_desc[d].upload(L.desc[d].data(), L.desc[d].size());
        P->d_chain_run_ptr[d].upload(L.run_ptr[d].data(), L.run_ptr[d].size());
        P->ntickets[d] = (int)L.run_ptr[d].size() - 1;
        P->need_peer[d] = L.need_peer[d];
      }
      // (the generic kernels' index arrays are not needed: a strip runs a descriptor-driven kernel)
      P->layout->desc[0] = std::vector<int32_t>(); P->layout->desc[1] = std::vector<int32_t>();
    } else {
    P->d_tail.upload(g.tail.data(), g.tail.size());
    P->d_order.upload(g.order.data(), g.order.size());
    P->d_fptr.upload(g.fptr.data(), g.fptr.size());
    P->d_fidx.upload(g.fidx.data(), g.fidx.size());
    P->d_bptr.upload(g.bptr.data(), g.bptr.size());
    P->d_bidx.upload(g.bidx.data(), g.bidx.size());
    P->d_lbn.upload(g.lb_pos_node.data(), g.lb_pos_node.size());
    P->d_lbe.upload(g.lb_pos_edge.data(), g.lb_pos_edge.size());
    P->d_mdir.upload(g.mdir.data(), g.mdir.size());
    P->d_gamma.upload(g.gamma.data(), g.gamma.size());
    for (int d = 0; d < 2; ++d) {
      const TrwsGraph::Sweep &S = g.sweep[d];
      P->d_run_ptr[d].upload(S.run_ptr.data(), S.run_ptr.size());
      if (!S.run_order.empty()) P->d_run_order[d].upload(S.run_order.data(), S.run_order.size());
      P->d_dep_ptr[d].upload(S.dep_ptr.data(), S.dep_ptr.size());
      P->d_dep_rank[d].upload(S.dep_rank.data(), S.dep_rank.size());
      P->d_in_slot[d].upload(S.in_slot.data(), S.in_slot.size());
      if (g.fast_ok) {
        P->d_desc[d].upload(S.desc.data(), S.desc.size());
        P->d_chain_run_ptr[d].upload(S.chain_run_ptr.data(), S.chain_run_ptr.size());
        if (!S.chain_run_order.empty()) P->d_chain_run_order[d].upload(S.chain_run_order.data(), S.chain_run_order.size());
      }
      if (g.fast_ok && S.chunked.ok && possible(at_best, TrwsFamily::Pipe) && !share) {
        P->sub_rows[d] = true;
        P->d_sub_desc[d].upload(S.chunked.desc.data(), S.chunked.desc.size());
        P->d_sub_run_ptr[d].upload(S.chunked.run_ptr.data(), S.chunked.run_ptr.size());
        P->d_sub_run_order[d].upload(S.chunked.run_order.data(), S.chunked.run_order.size());
      }
    }
    }
    {
      const TrwsGraph::Sweep::Spec &s0 = g.sweep[0].spec, &s1 = g.sweep[1].spec;
      // (allocated whatever the message mode and the FAST switch say; trws_pipe_kernel, trws_wide_kernel with its vector loaders)
      TrwsPlanFacts any = facts;
      any.exact = true; any.fast_switch = true;
      const unsigned fam = trws_families_possible(any, &why);
      bool on = nstrips == 1 && s0.ok && s1.ok && s0.nseg == s1.nseg && s0.seg_len == s1.seg_len &&
                (possible(fam, TrwsFamily::Pipe) || (possible(fam, TrwsFamily::Wide) && (K & 1) == 0 && kernel == 1));
      if (const char *e = trws_switch(kSwSpec)) on = on && std::atoi(e) != 0;
      P->spec_allowed = on;
      if (on) {
        for (int d = 0; d < 2; ++d) {
          const TrwsGraph::Sweep::Spec &sp = g.sweep[d].spec;
          P->d_spec_run_ptr[d].upload(sp.run_ptr.data(), sp.run_ptr.size());
          P->d_spec_run_order[d].upload(sp.run_order.data(), sp.run_order.size());
          P->d_spec_kind[d].upload(sp.kind.data(), sp.kind.size());
          if (P->sub_rows[d]) {
            const TrwsGraph::Sweep::Spec &cs = g.sweep[d].chunked.spec;
            P->d_sub_spec_run_ptr[d].upload(cs.run_ptr.data(), cs.run_ptr.size());
            P->d_sub_spec_run_order[d].upload(cs.run_order.data(), cs.run_order.size());
            P->d_sub_spec_kind[d].upload(cs.kind.data(), cs.kind.size());
          }
          // the K <= 64 runner's chain records, for either descriptor set it can be launched on
          if (possible(fam, TrwsFamily::Pipe)) {
            runner_records(P.get(), d, false);
            if (P->sub_rows[d]) runner_records(P.get(), d, true);
          }
        }
        const size_t ml = (size_t)std::max(s0.max_len, s1.max_len);
        P->d_spec_rows.alloc((size_t)s0.nseg * 8 * K);
        P->d_spec_undo.alloc((size_t)s0.nseg * ml * 4 * K);
        P->d_spec_x.alloc(s0.nseg);
        P->d_spec_stat.alloc(32);
        STEREO_HIP_CHECK(hipMemset(P->d_spec_stat.p, 0, 32 * sizeof(unsigned long long)));
        STEREO_HIP_CHECK(hipMemset(P->d_spec_rows.p, 0, sizeof(double) * (size_t)s0.nseg * 8 * K));
        STEREO_HIP_CHECK(hipMemset(P->d_spec_x.p, 0, sizeof(int32_t) * s0.nseg));
      }
      P->d_self.alloc(1); P->h_self.alloc(1);
    }
    if (strip_api) STEREO_HIP_CHECK(hipStreamCreateWithFlags(&P->own_stream, hipStreamNonBlocking));
    P->n_lb = nstrips > 1 ? g.strip_lb_terms[strip] : g.lb_terms;
    P->n_en = nstrips > 1 ? g.strip_nodes[strip] : N;
    // Strips that may have a neighbour on ANOTHER GPU keep the three arrays the neighbour writes into
    // (messages, flags, labels) in fine-grained memory (common.h); strips that share the only visible
    // device (logical strips, tests) stay in ordinary memory.  STEREO_HIP_STRIPS_FINEGRAINED=0/1 overrides.
    bool fine = nstrips > 1 && stereo_hip_device_count() > 1;
    if (const char *fg = trws_switch(kSwFineGrained)) fine = nstrips > 1 && std::atoi(fg) != 0;
    // (behind the nodes' flags: the speculative schedule's, two per segment)
    const size_t n_flags = (size_t)P->Nl + (P->spec_allowed ? 2 * (size_t)g.sweep[0].spec.nseg + 2 : 0);
    if (fine) P->d_done.alloc_fine_grained(n_flags); else P->d_done.alloc(n_flags);
    P->d_ctl.alloc(kCtlWords);
    P->d_fallbacks.alloc(1);
    STEREO_HIP_CHECK(hipMemset(P->d_fallbacks.p, 0, sizeof(unsigned long long)));
    if (const char *c = trws_switch(kSwCertificate)) P->certificate = std::string(c) != "0";
    if (const char *c = trws_switch(kSwIterateAhead)) P->ahead_allowed = std::atoi(c) != 0;
    {
      // how long a visit may wait for another workgroup before the launch gives up: inside one launch
      // a flag is late by microseconds; a neighbouring strip's launch belongs to another process and
      // may start seconds later (code-object load, a busy host)
      double secs = nstrips > 1 ? 120.0 : 20.0;
      if (const char *c = trws_switch(kSwSpinSeconds)) secs = std::max(0.001, std::atof(c));
      P->spin_ticks = (long long)(secs * 1e8);
    }
    if (trws_switch(kSwProf)) { P->d_prof.alloc(64); STEREO_HIP_CHECK(hipMemset(P->d_prof.p, 0, 512)); }
    if (trws_switch(kSwTimeline))
      P->d_timeline.alloc(4 * std::max({g.sweep[0].run_ptr.size(), g.sweep[0].chain_run_ptr.size(), g.sweep[1].chain_run_ptr.size(),
                                         g.sweep[0].spec.kind.size() + 1, g.sweep[1].spec.kind.size() + 1,
                                         g.sweep[0].chunked.run_ptr.size(), g.sweep[1].chunked.run_ptr.size(),
                                         g.sweep[0].chunked.spec.kind.size() + 1, g.sweep[1].chunked.spec.kind.size() + 1}) + 8);
    STEREO_HIP_CHECK(hipMemset(P->d_done.p, 0, sizeof(int32_t) * P->d_done.n));
    STEREO_HIP_CHECK(hipMemset(P->d_ctl.p, 0, sizeof(int32_t) * kCtlWords));
    {
      // one workgroup per concurrently active run, capped by what stays resident
      int64_t runs = std::max<int64_t>((int64_t)g.sweep[0].run_ptr.size() - 1, 1);
      if (g.fast_ok)
        runs = std::max<int64_t>({runs, (int64_t)g.sweep[0].chain_run_ptr.size() - 1, (int64_t)g.sweep[1].chain_run_ptr.size() - 1});
      if (nstrips > 1) runs = std::max<int64_t>({1, (int64_t)P->ntickets[0], (int64_t)P->ntickets[1]});
      if (P->spec_allowed) runs = std::max<int64_t>({runs, (int64_t)g.sweep[0].spec.run_order.size(), (int64_t)g.sweep[1].spec.run_order.size()});
      for (int d = 0; d < 2; ++d)
        if (P->sub_rows[d])
          runs = std::max<int64_t>({runs, (int64_t)g.sweep[d].chunked.run_ptr.size() - 1,
                                    P->spec_allowed ? (int64_t)g.sweep[d].chunked.spec.run_order.size() : 0});
      P->grid_blocks = (int)std::min<int64_t>(runs, P->cus * per_cu);
      if (max_blocks > 0) P->grid_blocks = std::min(P->grid_blocks, max_blocks);
    }
    if (fine) P->d_msg.alloc_fine_grained((size_t)P->El * K); else P->d_msg.alloc((size_t)P->El * K);
    {
      // the granule hand-over between ordinary runs (trws_graph.h: kDescGran): trws_pipe_kernel of one plan;
      // STEREO_HIP_TRWS_GRANULES=0 keeps every row behind the completion flags
      bool gran = possible(P->families, TrwsFamily::Pipe) && nstrips == 1;
      if (const char *e = trws_switch(kSwGranules)) gran = gran && std::atoi(e) != 0;
      if (gran) {
        P->d_gran.alloc(2 * (size_t)P->El * K); P->d_xgran.alloc(P->Nl);
        STEREO_HIP_CHECK(hipMemset(P->d_gran.p, 0, sizeof(unsigned long long) * P->d_gran.n));
        STEREO_HIP_CHECK(hipMemset(P->d_xgran.p, 0, sizeof(unsigned long long) * P->d_xgran.n));
      }
    }
    if (possible(P->families, TrwsFamily::Large)) P->d_large_scr.alloc((size_t)P->grid_blocks * large_scratch_doubles(P->Kp));
    P->d_lbterms.alloc(P->n_lb);
    P->d_eterms.alloc(P->n_en);
    if (fine) P->d_x.alloc_fine_grained(P->Nl); else P->d_x.alloc(P->Nl);
    P->h_lb.alloc(P->n_lb); P->h_en.alloc(P->n_en); P->h_x.alloc(P->Nl); P->h_ctl.alloc(kCtlWords);
    std::memset(P->h_ctl.p, 0, sizeof(int32_t) * kCtlWords);
    STEREO_HIP_CHECK(hipMemset(P->d_msg.p, 0, sizeof(double) * (size_t)P->El * K));
    STEREO_HIP_CHECK(hipMemset(P->d_x.p, 0, sizeof(int32_t) * P->Nl));
    STEREO_HIP_CHECK(hipEventCreate(&P->ev0));
    STEREO_HIP_CHECK(hipEventCreate(&P->ev1));
    STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_bwd, hipEventDisableTiming));
    STEREO_HIP_CHECK(hipEventCreateWithFlags(&P->ev_lb, hipEventDisableTiming));
    STEREO_HIP_CHECK(hipStreamCreateWithFlags(&P->copy_stream, hipStreamNonBlocking));
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    // every sweep kernel may need more than the default 64 KiB of dynamic LDS
    if (plds > 160 * 1024) return fail("stereo_trws: K too large for LDS", err, errcap);
    if (possible(P->families, TrwsFamily::Large)) large_set_attributes(plds); else generic_set_attributes(plds);
    if (possible(P->families, TrwsFamily::Pipe) || strip_api) pipe_set_attributes();
    if (possible(P->families, TrwsFamily::Pipe2)) pipe2_set_attributes();
    if (possible(P->families, TrwsFamily::Wide) || strip_api) wide_set_attributes();
    *plan = P.release();
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  } catch (const std::exception &e) {
    return fail(std::string("stereo_trws_plan_create: ") + e.what(), err, errcap);
  }
}

int stereo_trws_plan_create(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn,
                            int message_mode, stereo_trws_plan **plan, char *err, size_t errcap) {
  return plan_create_impl(kernel, K, N, E, conn, message_mode, nullptr, 1, 0, 0, nullptr, false, plan, err, errcap);
}

int stereo_trws_plan_create_strip(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn, int message_mode,
                                  const int32_t *owner, int nstrips, int strip, int max_workgroups,
                                  stereo_trws_plan *share_analysis_with, stereo_trws_plan **plan, char *err,
                                  size_t errcap) {
  return plan_create_impl(kernel, K, N, E, conn, message_mode, owner, nstrips, strip, max_workgroups,
                          share_analysis_with, true, plan, err, errcap);
}

void stereo_trws_plan_destroy(stereo_trws_plan *plan) {
  DeviceScope device_scope_(plan ? plan->device : -1);
  if (plan && plan->bwd_pending) (void)hipDeviceSynchronize();   // (a backward sweep launched ahead may still be running)
  if (plan && plan->d_timeline.p) print_timeline(plan);
  if (plan && plan->d_prof.p) print_profile(plan);
  delete plan;
}

}  // extern "C"
