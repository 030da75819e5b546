// TRW-S solver state: save and restore (the C ABI and the meaning of a state: include/stereo_hip.h).
// File map: trws_plan.hip.
//
// No reference counterpart.  A state is the caller's view of a minimisation -- E x K messages in the caller's edge
// order, N labels by node id, a header -- so a plan of the whole problem moves it with plain copies: its arrays ARE
// that layout.  Row strips store rows under strip-local ids, and only one strip's copy of a cross-strip edge is valid
// at rest (trws_state.h: strip_state_rows), so they get four streaming kernels:
//   trws_state_gather_kernel          local [El][K] rows with the take mask set -> the global [E][K] rows
//   trws_state_scatter_kernel         the global rows -> every local row (all copies are written: harmless)
//   trws_state_gather_labels_kernel   own nodes' labels -> global node ids
//   trws_state_scatter_labels_kernel  global labels -> own and halo nodes
// through the strip's local -> global tables (d_ledges, d_lnodes).  Mapping as in trws_beliefs.hip: a group of
// G = 2^ceil(log2 K) lanes (at most 64) per row, lanes over labels, so a wave holds 64 / G rows; above 64 labels one
// wave per row with a strided label loop.  The logical strips of one device share ONE launch per kernel: a table of
// per-strip blocks in device memory, a workgroup finds its strip by a prefix over the strips' workgroup counts.
// Both directions are HBM-bound copies of 8 K bytes per row plus 8 bytes of index (and one mask byte in the gather).
#include <algorithm>
#include <cstring>
#include <vector>

#include "trws_plan.h"

namespace stereo {

// a grouped launch: workgroup b works for strip m with first[m] <= b < first[m + 1]
struct StateGroupArgs {
  const StateBlock *pp;
  int n;
  int first[kMaxGroup + 1];
};

namespace {

constexpr int kStateWave = 64;
constexpr int kStateBlock = 256;

// the strip a workgroup of a grouped launch works for
__device__ __forceinline__ int state_member(const StateGroupArgs &ga) {
  int m = 0;
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i) m = (i < ga.n && (int)blockIdx.x >= ga.first[i]) ? i : m;  // static indices only
  return m;
}

__device__ __forceinline__ int64_t state_row(unsigned block, int lg) {
  const int lane = threadIdx.x & (kStateWave - 1);
  const int64_t wave = (int64_t)block * (kStateBlock / kStateWave) + threadIdx.x / kStateWave;
  return wave * (kStateWave >> lg) + (lane >> lg);
}

}  // namespace

__global__ __launch_bounds__(kStateBlock) void trws_state_gather_kernel(StateGroupArgs ga, double *__restrict__ messages) {
  const int m = state_member(ga);
  const StateBlock &b = ga.pp[m];
  const int lg = b.lg, K = b.K;
  const int64_t r = state_row(blockIdx.x - (unsigned)ga.first[m], lg);
  if (r >= b.n_rows) return;
  if (b.take && !b.take[r]) return;
  const int G = 1 << lg, sub = threadIdx.x & (G - 1);
  const double *__restrict__ src = b.msg + (size_t)r * K;
  double *__restrict__ dst = messages + (size_t)b.ledges[r] * K;
  for (int k = sub; k < K; k += G) dst[k] = src[k];
}

__global__ __launch_bounds__(kStateBlock) void trws_state_scatter_kernel(StateGroupArgs ga, const double *__restrict__ messages) {
  const int m = state_member(ga);
  const StateBlock &b = ga.pp[m];
  const int lg = b.lg, K = b.K;
  const int64_t r = state_row(blockIdx.x - (unsigned)ga.first[m], lg);
  if (r >= b.n_rows) return;
  const int G = 1 << lg, sub = threadIdx.x & (G - 1);
  const double *__restrict__ src = messages + (size_t)b.ledges[r] * K;
  double *__restrict__ dst = b.msg + (size_t)r * K;
  for (int k = sub; k < K; k += G) dst[k] = src[k];
}

__global__ __launch_bounds__(kStateBlock) void trws_state_gather_labels_kernel(StateGroupArgs ga, int32_t *__restrict__ labels) {
  const int m = state_member(ga);
  const StateBlock &b = ga.pp[m];
  const int64_t i = (int64_t)(blockIdx.x - (unsigned)ga.first[m]) * kStateBlock + threadIdx.x;
  if (i < b.n_labels) labels[b.lnodes[i]] = b.x[i];
}

__global__ __launch_bounds__(kStateBlock) void trws_state_scatter_labels_kernel(StateGroupArgs ga, const int32_t *__restrict__ labels) {
  const int m = state_member(ga);
  const StateBlock &b = ga.pp[m];
  const int64_t i = (int64_t)(blockIdx.x - (unsigned)ga.first[m]) * kStateBlock + threadIdx.x;
  if (i < b.n_labels) b.x[i] = labels[b.lnodes[i]];
}

namespace {

int state_lanes_log2(int K) {
  int lg = 0;
  while ((1 << lg) < K && lg < 6) ++lg;
  return lg;
}

// The plans of one save / load in strip order, checked: one plan of a whole problem, or every strip of one problem once.
struct StateGroup {
  stereo_trws_plan *plans[kMaxGroup];
  int n = 0;
  bool single = false;
};

int state_group(const char *who, stereo_trws_plan *const *plans, int n, bool one_device, StateGroup &G, char *err, size_t errcap) {
  if (!plans || n < 1 || n > kMaxGroup) return fail(std::string(who) + ": need 1 .. 16 plans", err, errcap);
  for (int i = 0; i < n; ++i)
    if (!plans[i]) return fail(std::string(who) + ": NULL plan", err, errcap);
  const stereo_trws_plan *P0 = plans[0];
  G.n = n;
  G.single = n == 1 && P0->nstrips == 1;
  if (G.single) { G.plans[0] = plans[0]; return 0; }
  if (P0->nstrips != n)
    return fail(std::string(who) + ": a state belongs to the whole problem: name every one of its " + std::to_string(P0->nstrips) +
                " strips (" + std::to_string(n) + " given)", err, errcap);
  for (int i = 0; i < n; ++i) G.plans[i] = nullptr;
  for (int i = 0; i < n; ++i) {
    stereo_trws_plan *P = plans[i];
    if (P->graph != P0->graph || P->nstrips != n || P->K != P0->K || P->kernel != P0->kernel || P->conn_key != P0->conn_key ||
        P->order_flag != P0->order_flag || P->strip < 0 || P->strip >= n || G.plans[P->strip])
      return fail(std::string(who) + ": the plans are not the strips of one problem, each once", err, errcap);
    if (one_device && P->device != P0->device)
      return fail(std::string(who) + ": the strips are on devices of their own: use the entry with host arrays", err, errcap);
    G.plans[P->strip] = P;
  }
  for (int i = 0; i < n; ++i)
    if (G.plans[i]->issued)
      return fail(std::string(who) + ": strip " + std::to_string(i) + " has an issued iteration that has not been collected", err, errcap);
  return 0;
}

// the block table of a grouped launch on the device (w: 0 gather, 1 scatter), kept with the group's first plan and
// sent when it changes -- behind everything that may still read the old one
const StateBlock *state_table(stereo_trws_plan *P0, const StateBlock *blocks, int n, int w) {
  if (!P0->d_state_table.p) P0->d_state_table.alloc(2 * kMaxGroup);
  StateBlock *d = P0->d_state_table.p + (size_t)w * kMaxGroup;
  if (P0->state_sent_n[w] != n || std::memcmp(P0->state_sent[w], blocks, sizeof(StateBlock) * n) != 0) {
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    STEREO_HIP_CHECK(hipMemcpy(d, blocks, sizeof(StateBlock) * n, hipMemcpyHostToDevice));
    std::memcpy(P0->state_sent[w], blocks, sizeof(StateBlock) * n);
    P0->state_sent_n[w] = n;
  }
  return d;
}

// the strip's authoritative rows by LOCAL edge id, on the device (built by its first save in that phase)
const uint8_t *strip_take(stereo_trws_plan *P, int phase) {
  DevBuf<uint8_t> &d = P->d_state_take[phase];
  if (!d.p) {
    std::vector<uint8_t> take((size_t)P->E), local((size_t)P->El);
    strip_state_rows(*P->graph, P->strip, phase, take.data());
    for (int64_t e = 0; e < P->El; ++e) local[e] = take[P->layout->edges[e]];
    d.alloc(local.size());
    STEREO_HIP_CHECK(hipMemcpy(d.p, local.data(), local.size(), hipMemcpyHostToDevice));
  }
  return d.p;
}

// One grouped launch pair for the strips of G on stream s.  gather: local -> the caller's arrays; else the reverse.
void launch_strips(StateGroup &G, bool gather, int phase, double *d_messages, int32_t *d_labels, hipStream_t s) {
  StateBlock blocks[kMaxGroup];
  StateGroupArgs rows{}, labs{};
  rows.n = labs.n = G.n;
  for (int i = 0; i < G.n; ++i) {
    stereo_trws_plan *P = G.plans[i];
    StateBlock &b = blocks[i];
    std::memset(&b, 0, sizeof(b));   // (compared bytewise)
    b.msg = P->d_msg.p; b.x = P->d_x.p; b.ledges = P->d_ledges.p; b.lnodes = P->d_lnodes.p;
    b.take = gather ? strip_take(P, phase) : nullptr;
    b.n_rows = P->El; b.n_labels = gather ? P->layout->n_own : P->Nl;
    b.K = P->K; b.lg = state_lanes_log2(P->K);
    const int64_t rows_per_block = (int64_t)(kStateBlock / kStateWave) * (kStateWave >> b.lg);
    rows.first[i + 1] = rows.first[i] + (int)((b.n_rows + rows_per_block - 1) / rows_per_block);
    labs.first[i + 1] = labs.first[i] + (int)((b.n_labels + kStateBlock - 1) / kStateBlock);
  }
  rows.pp = labs.pp = state_table(G.plans[0], blocks, G.n, gather ? 0 : 1);
  if (gather) {
    if (d_messages && rows.first[G.n] > 0)
      hipLaunchKernelGGL(trws_state_gather_kernel, dim3((unsigned)rows.first[G.n]), dim3(kStateBlock), 0, s, rows, d_messages);
    if (d_labels && labs.first[G.n] > 0)
      hipLaunchKernelGGL(trws_state_gather_labels_kernel, dim3((unsigned)labs.first[G.n]), dim3(kStateBlock), 0, s, labs, d_labels);
  } else {
    if (rows.first[G.n] > 0)
      hipLaunchKernelGGL(trws_state_scatter_kernel, dim3((unsigned)rows.first[G.n]), dim3(kStateBlock), 0, s, rows, (const double *)d_messages);
    if (labs.first[G.n] > 0)
      hipLaunchKernelGGL(trws_state_scatter_labels_kernel, dim3((unsigned)labs.first[G.n]), dim3(kStateBlock), 0, s, labs, (const int32_t *)d_labels);
  }
  STEREO_HIP_CHECK(hipGetLastError());
}

int state_save(const char *who, stereo_trws_plan *const *plans, int n, stereo_trws_state_header *header, double *messages,
               int32_t *labels, bool device, hipStream_t s, char *err, size_t errcap) {
  if (!header) return fail(std::string(who) + ": NULL header", err, errcap);
  StateGroup G;
  if (int rc = state_group(who, plans, n, device, G, err, errcap)) return rc;
  stereo_trws_plan *P0 = G.plans[0];
  for (int i = 1; i < G.n; ++i) {
    const stereo_trws_plan *P = G.plans[i];
    if (P->iterations != P0->iterations || P->fwd_pending != P0->fwd_pending || P->bwd_pending != P0->bwd_pending ||
        P->energy != P0->energy || P->lb != P0->lb)
      return fail(std::string(who) + ": the strips are not in one state (strip " + std::to_string(i) + " is elsewhere than strip 0)", err, errcap);
  }
  if (!G.single && P0->bwd_pending) return fail(std::string(who) + ": a strip with a pending backward sweep", err, errcap);
  try {
    // everything the plans have in flight: after an iterate / collect that is a backward sweep launched ahead at most
    for (int i = 0; i < G.n; ++i) {
      stereo_trws_plan *P = G.plans[i];
      if (!P->bwd_pending) continue;
      DeviceScope scope(P->device);
      STEREO_HIP_CHECK(hipStreamSynchronize(P->issue_stream));
      STEREO_HIP_CHECK(hipStreamSynchronize(P->copy_stream));
    }
    stereo_trws_state_header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = STEREO_TRWS_STATE_MAGIC; h.version = STEREO_TRWS_STATE_VERSION;
    h.kernel = P0->kernel; h.K = P0->K; h.N = P0->N; h.E = P0->E;
    h.message_mode = P0->mode | P0->order_flag;
    h.connectivity_key = P0->conn_key;
    h.phase = P0->bwd_pending ? 2 : P0->fwd_pending ? 1 : 0;
    h.iterations = P0->iterations; h.energy = P0->energy; h.lower_bound = P0->lb;
    if (P0->bwd_pending)   // the pending sweep's bound, in the order collect_iteration sums it
      for (int64_t i = 0; i < P0->n_lb; ++i) h.lower_bound_next += P0->h_lb_next.p[i];
    if (!G.single && P0->iterations > 0 && P0->iterations != P0->state_loaded_at) {
      // Strips commit sums of per-strip partial sums, equal to the single plan's to rounding only.  A state is
      // canonical, so its energy and bound are summed once more from the terms of the iteration collected last (they
      // are still in the strips' host buffers), in the single plan's order: a strip's terms are that order restricted
      // to its nodes (trws_graph.cpp: flatten_lists -- lb_pos_node / lb_pos_edge, e_pos), so a cursor per strip merges them back.
      const TrwsGraph &g = *P0->graph;
      int64_t at[kMaxGroup] = {0};
      double lb = 0, en = 0;
      for (int64_t r = P0->N - 1; r >= 0; --r) {
        const int sidx = g.owner[g.order[r]];
        for (int32_t j = 0; j < 1 + g.bptr[r + 1] - g.bptr[r]; ++j) lb += G.plans[sidx]->h_lb.p[at[sidx]++];
      }
      for (int i = 0; i < G.n; ++i) at[i] = 0;
      for (int64_t r = 0; r < P0->N; ++r) {
        const int sidx = g.owner[g.order[r]];
        en += G.plans[sidx]->h_en.p[at[sidx]++];
      }
      h.lower_bound = lb; h.energy = en;
    }
    const size_t K = (size_t)P0->K;
    if (G.single) {
      DeviceScope scope(P0->device);
      if (device) {
        if (messages) STEREO_HIP_CHECK(hipMemcpyAsync(messages, P0->d_msg.p, sizeof(double) * (size_t)P0->E * K, hipMemcpyDeviceToDevice, s));
        if (labels) STEREO_HIP_CHECK(hipMemcpyAsync(labels, P0->d_x.p, sizeof(int32_t) * (size_t)P0->N, hipMemcpyDeviceToDevice, s));
      } else {
        if (messages) STEREO_HIP_CHECK(hipMemcpy(messages, P0->d_msg.p, sizeof(double) * (size_t)P0->E * K, hipMemcpyDeviceToHost));
        if (labels) STEREO_HIP_CHECK(hipMemcpy(labels, P0->d_x.p, sizeof(int32_t) * (size_t)P0->N, hipMemcpyDeviceToHost));
      }
    } else if (device) {
      DeviceScope scope(P0->device);
      launch_strips(G, true, h.phase, messages, labels, s);
    } else {
      std::vector<uint8_t> take((size_t)P0->E);
      std::vector<double> rows;
      std::vector<int32_t> x;
      for (int i = 0; i < G.n; ++i) {
        stereo_trws_plan *P = G.plans[i];
        DeviceScope scope(P->device);
        const StripLayout &L = *P->layout;
        if (messages) {
          rows.resize((size_t)P->El * K);
          STEREO_HIP_CHECK(hipMemcpy(rows.data(), P->d_msg.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
          strip_state_rows(*P->graph, P->strip, h.phase, take.data());
          for (int64_t e = 0; e < P->El; ++e)
            if (take[L.edges[e]]) std::memcpy(messages + (size_t)L.edges[e] * K, &rows[(size_t)e * K], sizeof(double) * K);
        }
        if (labels) {
          x.resize((size_t)P->Nl);
          STEREO_HIP_CHECK(hipMemcpy(x.data(), P->d_x.p, sizeof(int32_t) * x.size(), hipMemcpyDeviceToHost));
          for (int64_t j = 0; j < L.n_own; ++j) labels[L.nodes[j]] = x[j];
        }
      }
    }
    *header = h;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

int state_load(const char *who, stereo_trws_plan *const *plans, int n, const stereo_trws_state_header *header,
               const double *messages, const int32_t *labels, bool device, hipStream_t s, char *err, size_t errcap) {
  if (!header) return fail(std::string(who) + ": NULL header", err, errcap);
  StateGroup G;
  if (int rc = state_group(who, plans, n, device, G, err, errcap)) return rc;
  stereo_trws_plan *P0 = G.plans[0];
  const stereo_trws_state_header &h = *header;
  // (the header first: the arrays have the header's sizes, which must be the plan's before they are read)
  const std::string refusal = trws_state_refusal(h, P0->kernel, P0->K, P0->N, P0->E, P0->conn_key, P0->mode | P0->order_flag);
  if (!refusal.empty()) return fail(std::string(who) + ": " + refusal, err, errcap);
  if (!messages || !labels) return fail(std::string(who) + ": NULL argument", err, errcap);
  if (h.phase == 2 && !G.single)
    return fail(std::string(who) + ": phase: a phase-2 state (a backward sweep no iteration has taken) enters a single plan only, not strips",
                err, errcap);
  for (int i = 0; i < G.n; ++i)
    if (!G.plans[i]->have_inputs)
      return fail(std::string(who) + ": the plan has no inputs: upload or bind first, then load (an upload wipes the state)", err, errcap);
  try {
    const size_t K = (size_t)P0->K;
    for (int i = 0; i < G.n; ++i) {
      DeviceScope scope(G.plans[i]->device);
      reset_state(G.plans[i]);
    }
    if (G.single) {
      DeviceScope scope(P0->device);
      const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
      STEREO_HIP_CHECK(hipMemcpyAsync(P0->d_msg.p, messages, sizeof(double) * (size_t)P0->E * K, kind, s));
      STEREO_HIP_CHECK(hipMemcpyAsync(P0->d_x.p, labels, sizeof(int32_t) * (size_t)P0->N, kind, s));
      STEREO_HIP_CHECK(hipStreamSynchronize(s));
    } else if (device) {
      DeviceScope scope(P0->device);
      launch_strips(G, false, h.phase, const_cast<double *>(messages), const_cast<int32_t *>(labels), s);
      STEREO_HIP_CHECK(hipStreamSynchronize(s));
    } else {
      std::vector<double> rows;
      std::vector<int32_t> x;
      for (int i = 0; i < G.n; ++i) {
        stereo_trws_plan *P = G.plans[i];
        DeviceScope scope(P->device);
        const StripLayout &L = *P->layout;
        rows.resize((size_t)P->El * K);
        for (int64_t e = 0; e < P->El; ++e) std::memcpy(&rows[(size_t)e * K], messages + (size_t)L.edges[e] * K, sizeof(double) * K);
        x.resize((size_t)P->Nl);
        for (int64_t j = 0; j < P->Nl; ++j) x[j] = labels[L.nodes[j]];
        STEREO_HIP_CHECK(hipMemcpy(P->d_msg.p, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
        STEREO_HIP_CHECK(hipMemcpy(P->d_x.p, x.data(), sizeof(int32_t) * x.size(), hipMemcpyHostToDevice));
      }
    }
    for (int i = 0; i < G.n; ++i) {
      stereo_trws_plan *P = G.plans[i];
      P->iterations = h.iterations; P->energy = h.energy; P->lb = h.lower_bound;
      P->fwd_pending = h.phase >= 1;
      P->state_loaded_at = h.iterations;
    }
    if (h.phase == 2) {
      // The pending state of issue_backward_ahead without a sweep in flight: the bound as its one term, the events an
      // iteration waits for recorded at once, the counters held as they read now -- the loaded sweep adds nothing.
      stereo_trws_plan *P = P0;
      DeviceScope scope(P->device);
      ensure_ahead_buffers(P);
      std::fill(P->h_lb_next.p, P->h_lb_next.p + P->n_lb, 0.0);
      P->h_lb_next.p[0] = h.lower_bound_next;
      STEREO_HIP_CHECK(hipMemcpy(P->h_held.p, P->d_fallbacks.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
      if (P->d_spec_stat.p)
        STEREO_HIP_CHECK(hipMemcpy(P->h_held.p + 1, P->d_spec_stat.p, sizeof(unsigned long long) * 32, hipMemcpyDeviceToHost));
      P->issue_stream = nullptr;
      STEREO_HIP_CHECK(hipEventRecord(P->ev0_next, nullptr));
      STEREO_HIP_CHECK(hipEventRecord(P->ev_ahead, nullptr));
      STEREO_HIP_CHECK(hipEventRecord(P->ev_lb_next, P->copy_stream));
      P->held_launches = 0;
      P->bwd_pending = true;
    }
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

}  // namespace
}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_trws_plans_state_save(stereo_trws_plan *const *plans, int n, stereo_trws_state_header *header, double *messages,
                                 int32_t *labels, char *err, size_t errcap) {
  return state_save("stereo_trws_plans_state_save", plans, n, header, messages, labels, false, nullptr, err, errcap);
}

int stereo_trws_plans_state_load(stereo_trws_plan *const *plans, int n, const stereo_trws_state_header *header,
                                 const double *messages, const int32_t *labels, char *err, size_t errcap) {
  return state_load("stereo_trws_plans_state_load", plans, n, header, messages, labels, false, nullptr, err, errcap);
}

int stereo_trws_plans_state_save_device(stereo_trws_plan *const *plans, int n, stereo_trws_state_header *header,
                                        double *d_messages, int32_t *d_labels, void *stream, char *err, size_t errcap) {
  return state_save("stereo_trws_plans_state_save_device", plans, n, header, d_messages, d_labels, true, (hipStream_t)stream, err, errcap);
}

int stereo_trws_plans_state_load_device(stereo_trws_plan *const *plans, int n, const stereo_trws_state_header *header,
                                        const double *d_messages, const int32_t *d_labels, void *stream, char *err,
                                        size_t errcap) {
  return state_load("stereo_trws_plans_state_load_device", plans, n, header, d_messages, d_labels, true, (hipStream_t)stream, err, errcap);
}

int stereo_trws_plan_state_save(stereo_trws_plan *plan, stereo_trws_state_header *header, double *messages, int32_t *labels,
                                char *err, size_t errcap) {
  return state_save("stereo_trws_plan_state_save", &plan, 1, header, messages, labels, false, nullptr, err, errcap);
}

int stereo_trws_plan_state_load(stereo_trws_plan *plan, const stereo_trws_state_header *header, const double *messages,
                                const int32_t *labels, char *err, size_t errcap) {
  return state_load("stereo_trws_plan_state_load", &plan, 1, header, messages, labels, false, nullptr, err, errcap);
}

}  // extern "C"
