// QPBO roof-duality fusion, the C ABI: stereo_rd (what rd_mex calls; keeps the plan of the last connectivity) and
// stereo_rd_plan_* (graph layout and device buffers kept across moves, capacities built on the device), with the
// construction, labelling and reduction kernels around the max-flow of qpbo_maxflow.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/stereo_hip.h"
#include "common.h"
#include "qpbo_solver.h"

namespace stereo {
namespace {

// ---- device-side construction for the plan API ------------------------------------------
// The doubled graph has a fixed slot layout per neighbour pair (one outgoing arc at each of
// i, j, i', j'); only heads, reverse links and capacities depend on whether the summed table
// is submodular, so a fusion move re-builds the whole network with two streaming kernels.
struct RdPlanDev {
  int N, npairs;
  const int32_t *pair_i, *pair_j, *pe_ptr, *pe_edge;  // pe_edge: edge id * 2 + transposed bit
  const int32_t *slots;                                // 4 per pair: out of i, j, i', j'
  const int32_t *aptr;                                 // CSR by doubled node
  const int32_t *slot_pair;                            // per slot: pair * 2 + role (0 = i side, 1 = j side)
  const double *U0, *U1, *E00, *E01, *E10, *E11;
  int32_t *head, *rev;
  double *r, *ci, *cjs, *konst, *ex, *snk, *trv, *u0;
};

__global__ __launch_bounds__(kQB) void rd_pairs_kernel(RdPlanDev d) {
  const int k = blockIdx.x * kQB + threadIdx.x;
  if (k >= d.npairs) return;
  double A = 0, B = 0, C = 0, D = 0;
  for (int q = d.pe_ptr[k]; q < d.pe_ptr[k + 1]; ++q) {
    const int e = d.pe_edge[q] >> 1, tr = d.pe_edge[q] & 1;
    A += d.E00[e]; D += d.E11[e];
    if (tr) { B += d.E10[e]; C += d.E01[e]; } else { B += d.E01[e]; C += d.E10[e]; }
  }
  const bool sub = B + C >= A + D;  // QPBO.cpp:434
  double a = sub ? A : B, b = sub ? B : A, c = sub ? C : D, dd = sub ? D : C;
  double ci = dd - a, cj, cij, cji;   // QPBO.h:760-807
  b -= a; c -= dd;
  if (b < 0) { ci += -b; cj = b; cji = b + c; cij = 0; }
  else if (c < 0) { ci += c; cj = -c; cij = b + c; cji = 0; }
  else { cj = 0; cij = b; cji = c; }
  d.ci[k] = ci;
  d.cjs[k] = sub ? cj : -cj;
  d.konst[k] = sub ? A : B + cj;
  const int i = d.pair_i[k], j = d.pair_j[k], N = d.N;
  const int si = d.slots[4 * k], sj = d.slots[4 * k + 1], sim = d.slots[4 * k + 2], sjm = d.slots[4 * k + 3];
  if (sub) {  // i->j (cij), j->i (cji), j'->i' (cij), i'->j' (cji)
    d.head[si] = j; d.rev[si] = sj; d.r[si] = cij;
    d.head[sj] = i; d.rev[sj] = si; d.r[sj] = cji;
    d.head[sjm] = i + N; d.rev[sjm] = sim; d.r[sjm] = cij;
    d.head[sim] = j + N; d.rev[sim] = sjm; d.r[sim] = cji;
  } else {    // i->j' (cij), j'->i (cji), j->i' (cij), i'->j (cji)
    d.head[si] = j + N; d.rev[si] = sjm; d.r[si] = cij;
    d.head[sjm] = i; d.rev[sjm] = si; d.r[sjm] = cji;
    d.head[sj] = i + N; d.rev[sj] = sim; d.r[sj] = cij;
    d.head[sim] = j; d.rev[sim] = sj; d.r[sim] = cji;
  }
}

__global__ __launch_bounds__(kQB) void rd_nodes_kernel(RdPlanDev d) {
  const int v = blockIdx.x * kQB + threadIdx.x;
  if (v >= d.N) return;
  double t = 0;
  for (int s = d.aptr[v]; s < d.aptr[v + 1]; ++s) {
    const int pr = d.slot_pair[s];
    t += (pr & 1) ? d.cjs[pr >> 1] : d.ci[pr >> 1];
  }
  t += d.U1[v] - d.U0[v];  // QPBO.h:615-624
  d.trv[v] = t;
  d.ex[v] = t > 0 ? t : 0.0; d.snk[v] = t < 0 ? -t : 0.0;
  d.ex[v + d.N] = t < 0 ? -t : 0.0; d.snk[v + d.N] = t > 0 ? t : 0.0;  // mate: -t (QPBO.cpp:689)
}

// strong persistency on the device (QPBO.cpp:840-844): x_i = 1 iff i reaches the sink, 0 iff its
// mate does, -1 if both or neither; counts the -1s
__global__ __launch_bounds__(kQB) void rd_labels_kernel(int64_t N, int n, const int32_t *h, int8_t *label,
                                                       int32_t *unlabelled, int32_t *free_list = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * kQB + threadIdx.x;
  if (i >= N) return;
  const int li = h[i] < n ? 1 : 0, lm = h[i + N] < n ? 1 : 0;
  const int l = li == lm ? -1 : li;
  label[i] = (int8_t)l;
  if (l < 0) {
    const int slot = atomicAdd(unlabelled, 1);
    if (free_list) free_list[slot] = (int32_t)i;   // (in no particular order: the host sorts the few there are)
  }
}

// The residual arcs of the free nodes (both nodes of every unlabelled variable, ids ascending), for the weak
// persistency pass on the host: per node its arcs in list order -- head and two bits, residual capacity on the arc
// and on its reverse.  Only this travels, not the residual network.
__global__ __launch_bounds__(kQB) void rd_free_arcs_kernel(int cnt, int N, const int32_t *ids, const int32_t *aptr,
                                                          const int32_t *head, const int32_t *rev, const double *r,
                                                          int maxdeg, int32_t *out_head, uint8_t *out_flag) {
  const int t = blockIdx.x * kQB + threadIdx.x;
  if (t >= 2 * cnt) return;
  const int v = t < cnt ? ids[t] : ids[t - cnt] + N;
  const int a0 = aptr[v], deg = aptr[v + 1] - a0;
  for (int k = 0; k < maxdeg; ++k) {
    int w = -1;
    uint8_t f = 0;
    if (k < deg) {
      const int a = a0 + k;
      w = head[a];
      f = (uint8_t)((r[a] > 0 ? 1 : 0) | (r[rev[a]] > 0 ? 2 : 0));
    }
    out_head[(size_t)t * maxdeg + k] = w;
    out_flag[(size_t)t * maxdeg + k] = f;
  }
}

__global__ __launch_bounds__(kQB) void rd_set_labels_kernel(int cnt, const int32_t *ids, const int8_t *lab, int8_t *label) {
  const int t = blockIdx.x * kQB + threadIdx.x;
  if (t < cnt) label[ids[t]] = lab[t];
}

// fixed-shape reduction (same tree for every run): partial[b] = sum of a 2048-element chunk
__global__ __launch_bounds__(kQB) void det_sum_kernel(const double *x, int64_t n, double *partial) {
  __shared__ double sh[kQB];
  const int64_t base = (int64_t)blockIdx.x * (kQB * 8);
  double acc = 0;
  for (int k = 0; k < 8; ++k) {
    const int64_t i = base + (int64_t)k * kQB + threadIdx.x;
    if (i < n) acc += x[i];
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kQB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// flow absorbed by every node's sink arc: initial minus residual capacity
__global__ __launch_bounds__(kQB) void rd_absorbed_kernel(int n, const double *snk0, const double *snk, double *out) {
  const int v = blockIdx.x * kQB + threadIdx.x;
  if (v < n) out[v] = snk0[v] - snk[v];
}

// energy of a labelling from the caller's tables: per-node and per-edge terms
__global__ __launch_bounds__(kQB) void rd_energy_terms_kernel(int64_t N, int64_t E, const uint32_t *conn,
                                                              const int32_t *h, int n, const double *U0,
                                                              const double *U1, const double *E00,
                                                              const double *E01, const double *E10,
                                                              const double *E11, const int8_t *label,
                                                              double *terms) {
  const int64_t t = (int64_t)blockIdx.x * kQB + threadIdx.x;
  if (t < N) {
    terms[t] = label[t] == 1 ? U1[t] : U0[t];
  } else if (t < N + E) {
    const int64_t e = t - N;
    const int xi = label[conn[2 * e]] == 1, xj = label[conn[2 * e + 1]] == 1;
    terms[t] = xi ? (xj ? E11[e] : E10[e]) : (xj ? E01[e] : E00[e]);
  }
}

}  // namespace

QpboOptions QpboOptions::from_env() {
  QpboOptions o;
  auto num = [](const char *name, int dflt, int lo, int hi) {
    const char *e = std::getenv(name);
    return e ? std::min(hi, std::max(lo, std::atoi(e))) : dflt;
  };
  auto on = [](const char *name, bool dflt) {   // set to anything but 0
    const char *e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
  };
  o.relabel_every = num("STEREO_HIP_QPBO_RELABEL_EVERY", o.relabel_every, 1, INT32_MAX);
  o.tiled = num("STEREO_HIP_QPBO_TILED", o.tiled, 0, INT32_MAX);
  o.switch_at = num("STEREO_HIP_QPBO_SWITCH", o.switch_at, 0, INT32_MAX);
  o.first_interval = num("STEREO_HIP_QPBO_FIRST_INTERVAL", o.first_interval, 1, INT32_MAX);
  o.adaptive = on("STEREO_HIP_QPBO_ADAPTIVE", o.adaptive);
  o.stall_permille = num("STEREO_HIP_QPBO_STALL_PERMILLE", o.stall_permille, 0, 999);
  o.final_relabel = on("STEREO_HIP_QPBO_FINAL_RELABEL", o.final_relabel);
  o.wrap_at = num("STEREO_HIP_QPBO_WRAP_AT", o.wrap_at, 0, 4095);
  o.improve_blocks = num("STEREO_HIP_QPBO_IMPROVE_BLOCKS", o.improve_blocks, 1, INT32_MAX);
  o.confined = on("STEREO_HIP_QPBO_CONFINED", o.confined);
  o.weak_full = std::getenv("STEREO_HIP_QPBO_WEAK_FULL") != nullptr;   // (these two: set at all)
  o.verbose = std::getenv("STEREO_HIP_QPBO_VERBOSE") != nullptr;
  o.rd_cache = on("STEREO_HIP_RD_CACHE", o.rd_cache);
  return o;
}

}  // namespace stereo

using namespace stereo;

namespace {

int rd_plan_solve_host(stereo_rd_plan *P, const QpboOptions &opt, const double *U0, const double *U1, const double *E00,
                       const double *E01, const double *E10, const double *E11, int improve, double *labelling,
                       double *energy, double *lower_bound, double *num_unlabelled, char *err, size_t errcap);

struct RdPlanCache {
  std::mutex mu;
  stereo_rd_plan *plan = nullptr;
  int64_t N = 0, E = 0;
  int device = -1;
  std::vector<uint32_t> conn;
};

RdPlanCache &rd_plan_cache() {
  static RdPlanCache *C = new RdPlanCache;   // (never destroyed: the HIP runtime may be gone before static destructors run)
  return *C;
}

int rd_through_cached_plan(const QpboOptions &opt, const double *U0, const double *U1, const double *E00, const double *E01,
                           const double *E10, const double *E11, const uint32_t *conn, int64_t N, int64_t E, int improve,
                           double *labelling, double *energy, double *lower_bound, double *num_unlabelled, char *err, size_t errcap) {
  RdPlanCache *C = &rd_plan_cache();
  std::lock_guard<std::mutex> lock(C->mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail("stereo_rd: hipGetDevice failed", err, errcap);
  const bool hit = C->plan && C->N == N && C->E == E && C->device == dev &&
                   std::memcmp(C->conn.data(), conn, sizeof(uint32_t) * 2 * (size_t)E) == 0;
  if (!hit) {
    if (C->plan) { stereo_rd_plan_destroy(C->plan); C->plan = nullptr; }
    stereo_rd_plan *plan = nullptr;
    const int rc = stereo_rd_plan_create(N, E, conn, &plan, err, errcap);
    if (rc != 0) return rc;
    const int64_t H = grid_height_of(conn, N, E);
    if (H > 0 && N / H < INT32_MAX) {
      char e2[128] = {0};
      (void)stereo_rd_plan_set_grid(plan, (int)H, (int)(N / H), e2, sizeof(e2));   // a hint: results do not depend on it
    }
    C->plan = plan; C->N = N; C->E = E; C->device = dev;
    C->conn.assign(conn, conn + 2 * (size_t)E);
  }
  return rd_plan_solve_host(C->plan, opt, U0, U1, E00, E01, E10, E11, improve, labelling, energy, lower_bound, num_unlabelled,
                            err, errcap);
}

}  // namespace

extern "C" void stereo_rd_cache_clear(void) {
  RdPlanCache &C = rd_plan_cache();
  std::lock_guard<std::mutex> lock(C.mu);
  if (C.plan) { stereo_rd_plan_destroy(C.plan); C.plan = nullptr; }
  C.conn.clear(); C.conn.shrink_to_fit();
}


extern "C" int stereo_rd(const double *U0, const double *U1, const double *E00, const double *E01,
                         const double *E10, const double *E11, const uint32_t *conn, int64_t N, int64_t E,
                         int improve, double *labelling, double *energy, double *lower_bound,
                         double *num_unlabelled, char *err, size_t errcap) {
  if (!U0 || !U1 || !labelling || !energy || !lower_bound || !num_unlabelled || (E > 0 && (!E00 || !E01 || !E10 || !E11 || !conn)))
    return fail("stereo_rd: NULL argument", err, errcap);
  if (stereo_hip_device_count() < 1)
    return fail("stereo_rd: no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  // The gateway is called once per fusion move with the SAME connectivity (dispmap_super.m:61-84): the plan of the
  // last connectivity seen is kept (edge grouping, slot layout, device buffers), so that from the second move on a
  // call costs what stereo_rd_plan_solve costs -- the upload of the six term arrays and the solve -- instead of
  // rebuilding the graph on the host every time (54 -> 2 ms at 450 x 375).  STEREO_HIP_RD_CACHE=0: build per call.
  const QpboOptions opt = QpboOptions::from_env();
  if (E > 0 && N > 0 && opt.rd_cache)
    return rd_through_cached_plan(opt, U0, U1, E00, E01, E10, E11, conn, N, E, improve, labelling, energy, lower_bound,
                                  num_unlabelled, err, errcap);
  try {
    QpboSolver S;
    std::string berr;
    const bool verbose = opt.verbose;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    if (!build_problem(U0, U1, E00, E01, E10, E11, conn, N, E, S.P, berr)) return fail(berr, err, errcap);
    const double t1 = now();
    S.upload();
    const double t2 = now();
    S.maxflow(opt);
    const double t3 = now();
    if (verbose) std::fprintf(stderr, "[stereo_hip qpbo] build %.2f ms, upload %.2f ms, maxflow %.2f ms\n", t1 - t0, t2 - t1, t3 - t2);
    const int n = S.n;
    std::vector<int32_t> h(n);
    std::vector<double> snk(n);
    STEREO_HIP_CHECK(hipMemcpy(h.data(), S.g.h, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    STEREO_HIP_CHECK(hipMemcpy(snk.data(), S.d_snk.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    std::vector<int> label(N);
    double unl = 0;
    for (int64_t i = 0; i < N; ++i) {
      label[i] = label_from_heights(h[i], h[i + N], n, -1);
      if (label[i] < 0) unl += 1;
    }
    if (unl > 0) {
      std::vector<double> r(S.m);
      STEREO_HIP_CHECK(hipMemcpy(r.data(), S.d_r.p, sizeof(double) * S.m, hipMemcpyDeviceToHost));
      weak_persistencies(S.P, r, label);
      unl = 0;
      for (int64_t i = 0; i < N; ++i) if (label[i] < 0) unl += 1;
    }
    if (verbose)
      std::fprintf(stderr, "[stereo_hip qpbo] n=%d arcs=%d iterations=%lld global_relabels=%lld unlabelled=%g\n", S.n, S.m,
                   (long long)S.iterations, (long long)S.relabels, unl);
    *num_unlabelled = unl;  // rd_mex.cpp:83-88: counted before Improve
    // roof-dual bound: const + sum_i min(0, tr_i) + flow/2, flow = what reached the sink
    {
      double flow = 0, neg = 0;
      for (int v = 0; v < n; ++v) flow += S.snk0[v] - snk[v];
      for (int64_t i = 0; i < N; ++i) neg += S.P.tr[i] < 0 ? S.P.tr[i] : 0.0;
      *lower_bound = S.P.const0 + neg + flow / 2;
    }
    if (improve && unl > 0) {
      // QPBO::Improve() (QPBO_extra.cpp:1151-1233) from user labels 0: visit the nodes in a
      // rand() permutation (QPBO_extra.cpp:13-27); a node that is still not strongly labelled
      // is fixed to 0 by a large unary term and the flow is re-maximised incrementally.
      // only nodes without a strong label can ever need fixing; strong labels persist
      S.improve(opt, improve_permutation(N), h);
      for (int64_t i = 0; i < N; ++i) label[i] = label_from_heights(h[i], h[i + N], n, 0);  // QPBO_extra.cpp:1210-1219: ambiguous -> user label (0)
    }
    // energy of the labelling (unknown -> 0, QPBO.cpp:857), from the caller's own tables
    double en = 0;
    for (int64_t i = 0; i < N; ++i) { labelling[i] = label[i]; en += label[i] == 1 ? U1[i] : U0[i]; }
    for (int64_t e = 0; e < E; ++e) {
      const int xi = label[conn[2 * e]] == 1, xj = label[conn[2 * e + 1]] == 1;
      en += xi ? (xj ? E11[e] : E10[e]) : (xj ? E01[e] : E00[e]);
    }
    *energy = en;
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  } catch (const std::exception &e) {
    return fail(std::string("stereo_rd: ") + e.what(), err, errcap);
  }
}

// ------------------------------------------------------------------ plan API

struct stereo_rd_plan {
  int64_t N = 0, E = 0, npairs = 0;
  DevBuf<int32_t> d_pair_i, d_pair_j, d_pe_ptr, d_pe_edge, d_slots, d_slot_pair;
  DevBuf<uint32_t> d_conn;
  DevBuf<double> d_ci, d_cjs, d_konst, d_trv, d_terms, d_partial, d_in[6], d_snk0;
  DevBuf<int8_t> d_label, d_flab;
  DevBuf<int32_t> d_free, d_fids, d_fhead;   // unlabelled variables (unordered | sorted), heads of the free nodes' arcs
  DevBuf<uint8_t> d_fflag;
  QpboSolver S;
};

namespace {

double det_sum(const double *x, int64_t n, DevBuf<double> &partial) {
  if (n <= 0) return 0.0;
  const int64_t nb = (n + kQB * 8 - 1) / (kQB * 8);
  if (partial.n < (size_t)nb) partial.alloc(nb);
  hipLaunchKernelGGL(det_sum_kernel, dim3((unsigned)nb), dim3(kQB), 0, 0, x, n, partial.p);
  std::vector<double> h(nb);
  STEREO_HIP_CHECK(hipMemcpy(h.data(), partial.p, sizeof(double) * nb, hipMemcpyDeviceToHost));
  double s = 0;
  for (double v : h) s += v;  // fixed order
  return s;
}


// Several fixed-shape sums whose results the host only needs later: the kernels are queued as they become
// possible, one copy brings all block partials back (a synchronous copy per sum was eight host round trips per move).
struct DetSums {
  DevBuf<double> &buf;
  std::vector<std::pair<size_t, int64_t>> slots;   // (offset, #partials)
  std::vector<double> host;
  size_t used = 0;
  static int64_t blocks(int64_t n) { return n > 0 ? (n + kQB * 8 - 1) / (kQB * 8) : 0; }
  DetSums(DevBuf<double> &b, int64_t capacity) : buf(b) {
    if (buf.n < (size_t)std::max<int64_t>(capacity, 1)) buf.alloc((size_t)std::max<int64_t>(capacity, 1));
  }
  int queue(const double *x, int64_t n) {
    const int64_t nb = blocks(n);
    if (used + (size_t)nb > buf.n) throw HipError{"DetSums: capacity"};
    if (nb > 0) hipLaunchKernelGGL(det_sum_kernel, dim3((unsigned)nb), dim3(kQB), 0, 0, x, n, buf.p + used);
    slots.push_back({used, nb});
    used += (size_t)nb;
    return (int)slots.size() - 1;
  }
  void fetch() {
    host.resize(used);
    if (used) STEREO_HIP_CHECK(hipMemcpy(host.data(), buf.p, sizeof(double) * used, hipMemcpyDeviceToHost));
  }
  double get(int slot) const {
    double s = 0;
    for (int64_t k = 0; k < slots[slot].second; ++k) s += host[slots[slot].first + k];  // fixed order
    return s;
  }
};
}  // namespace

extern "C" int stereo_rd_plan_create(int64_t N, int64_t E, const uint32_t *conn, stereo_rd_plan **plan, char *err,
                                     size_t errcap) {
  if (!plan) return fail("stereo_rd_plan_create: plan is NULL", err, errcap);
  *plan = nullptr;
  if (N <= 0 || (E > 0 && !conn)) return fail("stereo_rd_plan_create: bad argument", err, errcap);
  if (2 * N >= INT32_MAX / 2 || E >= INT32_MAX / 4) return fail("stereo_rd: problem too large for 32-bit ids", err, errcap);
  if (stereo_hip_device_count() < 1)
    return fail("stereo_rd: no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  try {
    std::unique_ptr<stereo_rd_plan> P(new stereo_rd_plan);
    P->N = N; P->E = E;
    PairGroups G;
    std::string gerr;
    if (!group_pairs(conn, N, E, G, gerr)) return fail(gerr, err, errcap);
    const std::vector<int32_t> &pi = G.pi, &pj = G.pj, &pe_ptr = G.pe_ptr, &pe_edge = G.pe_edge;
    const int64_t np = G.npairs(), n = 2 * N, m = 4 * np;
    P->npairs = np;
    // slot layout: every pair owns one outgoing arc at i, j, i', j'; arcs grouped by tail in pair order
    std::vector<int32_t> aptr(n + 1, 0);
    for (int64_t k = 0; k < np; ++k) { ++aptr[pi[k] + 1]; ++aptr[pj[k] + 1]; ++aptr[pi[k] + N + 1]; ++aptr[pj[k] + N + 1]; }
    for (int64_t v = 0; v < n; ++v) aptr[v + 1] += aptr[v];
    std::vector<int32_t> fill(aptr.begin(), aptr.end() - 1), slots(4 * np), slot_pair(m, 0);
    for (int64_t k = 0; k < np; ++k) {
      const int32_t i = pi[k], j = pj[k];
      slots[4 * k] = fill[i]++; slots[4 * k + 1] = fill[j]++;
      slots[4 * k + 2] = fill[i + N]++; slots[4 * k + 3] = fill[j + N]++;
      slot_pair[slots[4 * k]] = (int32_t)(2 * k); slot_pair[slots[4 * k + 1]] = (int32_t)(2 * k + 1);
      slot_pair[slots[4 * k + 2]] = (int32_t)(2 * k); slot_pair[slots[4 * k + 3]] = (int32_t)(2 * k + 1);
    }
    P->d_pair_i.upload(pi.data(), np); P->d_pair_j.upload(pj.data(), np);
    P->d_pe_ptr.upload(pe_ptr.data(), pe_ptr.size()); P->d_pe_edge.upload(pe_edge.data(), E);
    P->d_slots.upload(slots.data(), slots.size()); P->d_slot_pair.upload(slot_pair.data(), slot_pair.size());
    P->d_conn.upload(conn, 2 * E);
    P->d_ci.alloc(np); P->d_cjs.alloc(np); P->d_konst.alloc(np); P->d_trv.alloc(N);
    P->d_terms.alloc(std::max<int64_t>(N + E, n)); P->d_label.alloc(N); P->d_snk0.alloc(n);
    QpboSolver &S = P->S;
    S.P.N = N; S.P.aptr = aptr;
    S.bind(N, aptr);   // (heads, reverse arcs, capacities and terminals are written by the kernels of every solve)
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    *plan = P.release();
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  } catch (const std::exception &e) {
    return fail(std::string("stereo_rd_plan_create: ") + e.what(), err, errcap);
  }
}

extern "C" void stereo_rd_plan_destroy(stereo_rd_plan *plan) { delete plan; }

// inputs: six DEVICE arrays (U0, U1 of length N; E00, E01, E10, E11 of length E)
static int rd_plan_solve_device(stereo_rd_plan *P, const QpboOptions &opt, const double *const in[6], int improve,
                                double *labelling, double *energy, double *lower_bound, double *num_unlabelled, char *err,
                                size_t errcap) {
  try {
    QpboSolver &S = P->S;
    const int64_t N = P->N, E = P->E, np = P->npairs;
    const int n = S.n;
    RdPlanDev d{};
    d.N = (int)N; d.npairs = (int)np; d.pair_i = P->d_pair_i.p; d.pair_j = P->d_pair_j.p;
    d.pe_ptr = P->d_pe_ptr.p; d.pe_edge = P->d_pe_edge.p; d.slots = P->d_slots.p; d.aptr = S.d_aptr.p;
    d.slot_pair = P->d_slot_pair.p;
    d.U0 = in[0]; d.U1 = in[1]; d.E00 = in[2]; d.E01 = in[3]; d.E10 = in[4]; d.E11 = in[5];
    d.head = S.d_head.p; d.rev = S.d_rev.p; d.r = S.d_r.p; d.ci = P->d_ci.p; d.cjs = P->d_cjs.p;
    d.konst = P->d_konst.p; d.ex = S.d_ex.p; d.snk = S.d_snk.p; d.trv = P->d_trv.p;
    // the two kernels may leave the sweep state of a previous move behind: restore the buffers
    S.g.h = S.d_h.p; S.g.h2 = S.d_h2.p;
    STEREO_HIP_CHECK(hipMemsetAsync(S.d_delta.p, 0, sizeof(double) * 2 * std::max(S.m, 1), 0));
    if (np > 0) hipLaunchKernelGGL(rd_pairs_kernel, dim3((unsigned)((np + kQB - 1) / kQB)), dim3(kQB), 0, 0, d);
    hipLaunchKernelGGL(rd_nodes_kernel, dim3((unsigned)((N + kQB - 1) / kQB)), dim3(kQB), 0, 0, d);
    STEREO_HIP_CHECK(hipMemcpyAsync(P->d_snk0.p, S.d_snk.p, sizeof(double) * n, hipMemcpyDeviceToDevice, 0));
    // constant of the normal form and sum_i min(0, tr_i): fixed-shape reductions, queued now and read back
    // together with the sums that follow the max-flow
    DetSums sums(P->d_partial, DetSums::blocks(np) + 2 * DetSums::blocks(N) + 2 * DetSums::blocks(n) + DetSums::blocks(N + E));
    const int s_konst = sums.queue(P->d_konst.p, np), s_u0 = sums.queue(in[0], N);
    const int s_neg = sums.queue(P->d_snk0.p, N);   // sum_i min(0, tr_i) = -(sink capacity of the unprimed half)
    S.iterations = 0; S.relabels = 0;
    const bool verbose = opt.verbose;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (verbose) STEREO_HIP_CHECK(hipDeviceSynchronize());
    const double tm0 = now();
    S.maxflow(opt);
    if (verbose) {
      STEREO_HIP_CHECK(hipDeviceSynchronize());
      std::fprintf(stderr, "[stereo_hip qpbo plan] maxflow %.3f ms\n", now() - tm0);
    }
    // what reached the sink, node by node (snk0 - snk is exact for a node whose capacity barely moved -- an
    // out-of-range plane makes unaries of 4e7, dispmap_ncc.m:245 -- where the difference of the two totals
    // loses everything below ulp(1e12): 1e-3 on example_ncc.m's first move)
    hipLaunchKernelGGL(rd_absorbed_kernel, dim3((unsigned)((n + kQB - 1) / kQB)), dim3(kQB), 0, 0, n, P->d_snk0.p, S.d_snk.p,
                       P->d_terms.p);
    const int s_flow = sums.queue(P->d_terms.p, n);   // (d_terms, max(N + E, 2 N) doubles, is free until the energy terms below)
    // labels on the device; the host only sees the number of unlabelled nodes
    if ((int64_t)P->d_label.n < N) P->d_label.alloc(N);
    STEREO_HIP_CHECK(hipMemsetAsync(S.d_cnt.p + 3, 0, sizeof(int32_t), 0));
    if ((int64_t)P->d_free.n < N) P->d_free.alloc(N);
    hipLaunchKernelGGL(rd_labels_kernel, dim3((unsigned)((N + kQB - 1) / kQB)), dim3(kQB), 0, 0, N, n, S.g.h,
                       P->d_label.p, S.d_cnt.p + 3, P->d_free.p);
    // the energy of the strong labels, on the bet that no node stays unlabelled (otherwise it is summed again below)
    hipLaunchKernelGGL(rd_energy_terms_kernel, dim3((unsigned)((N + E + kQB - 1) / kQB)), dim3(kQB), 0, 0, N, E,
                       P->d_conn.p, S.g.h, n, in[0], in[1], in[2], in[3], in[4], in[5], P->d_label.p, P->d_terms.p);
    const int s_energy = sums.queue(P->d_terms.p, N + E);
    sums.fetch();
    int32_t unl32 = 0;
    STEREO_HIP_CHECK(hipMemcpy(&unl32, S.d_cnt.p + 3, sizeof(unl32), hipMemcpyDeviceToHost));
    const double konst = sums.get(s_konst) + sums.get(s_u0), neg = -sums.get(s_neg);
    *lower_bound = konst + neg + sums.get(s_flow) / 2;
    double unl = unl32;
    if (unl > 0) {
      const double tw0 = now();
      std::vector<int32_t> h;
      const int maxdeg = S.max_degree;
      const bool compact = maxdeg >= 1 && maxdeg <= 16 && !opt.weak_full;
      if (compact) {
        // Weak persistency (QPBO_postprocessing.cpp:10-120) is a two-pass DFS over the FREE nodes only: their ids
        // come back, the arcs of exactly those nodes are gathered on the device, the pass runs on the host on that
        // small graph, and the new labels go back by id -- instead of the heights and the whole residual network.
        const int cnt = unl32;
        std::vector<int32_t> ids(cnt);
        STEREO_HIP_CHECK(hipMemcpy(ids.data(), P->d_free.p, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
        std::sort(ids.begin(), ids.end());
        const size_t na = (size_t)2 * cnt * maxdeg;
        if (P->d_fids.n < (size_t)cnt) P->d_fids.alloc((size_t)cnt + cnt / 2 + 64);
        if (P->d_fhead.n < na) { P->d_fhead.alloc(na + na / 2 + 64); P->d_fflag.alloc(na + na / 2 + 64); }
        if (P->d_flab.n < (size_t)cnt) P->d_flab.alloc((size_t)cnt + cnt / 2 + 64);
        STEREO_HIP_CHECK(hipMemcpyAsync(P->d_fids.p, ids.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice, 0));
        hipLaunchKernelGGL(rd_free_arcs_kernel, dim3((unsigned)((2 * cnt + kQB - 1) / kQB)), dim3(kQB), 0, 0, cnt, (int)N,
                           P->d_fids.p, S.d_aptr.p, S.d_head.p, S.d_rev.p, S.d_r.p, maxdeg, P->d_fhead.p, P->d_fflag.p);
        std::vector<int32_t> heads(na);
        std::vector<uint8_t> flags(na);
        STEREO_HIP_CHECK(hipMemcpy(heads.data(), P->d_fhead.p, sizeof(int32_t) * na, hipMemcpyDeviceToHost));
        STEREO_HIP_CHECK(hipMemcpy(flags.data(), P->d_fflag.p, na, hipMemcpyDeviceToHost));
        const double tw1 = now();
        std::vector<int8_t> lab;
        weak_persistencies_compact(cnt, (int)N, ids, maxdeg, heads, flags, lab);
        unl = 0;
        for (int t = 0; t < cnt; ++t) if (lab[t] < 0) unl += 1;
        STEREO_HIP_CHECK(hipMemcpyAsync(P->d_flab.p, lab.data(), cnt, hipMemcpyHostToDevice, 0));
        hipLaunchKernelGGL(rd_set_labels_kernel, dim3((unsigned)((cnt + kQB - 1) / kQB)), dim3(kQB), 0, 0, cnt, P->d_fids.p,
                           P->d_flab.p, P->d_label.p);
        STEREO_HIP_CHECK(hipStreamSynchronize(0));   // (the host vectors of the two asynchronous copies go out of scope)
        if (verbose) std::fprintf(stderr, "[stereo_hip qpbo plan] weak persistency: %d free variables, %.3f ms to fetch their arcs, %.3f ms on the host\n", cnt, tw1 - tw0, now() - tw1);
      } else {
        // (graphs with long arc lists: heights and the whole residual network go to the host)
        h.resize(n);
        STEREO_HIP_CHECK(hipMemcpy(h.data(), S.g.h, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        std::vector<int> label(N);
        for (int64_t i = 0; i < N; ++i) label[i] = label_from_heights(h[i], h[i + N], n, -1);
        S.P.head.resize(S.m); S.P.rev.resize(S.m);
        std::vector<double> r(S.m);
        STEREO_HIP_CHECK(hipMemcpy(S.P.head.data(), S.d_head.p, sizeof(int32_t) * S.m, hipMemcpyDeviceToHost));
        STEREO_HIP_CHECK(hipMemcpy(S.P.rev.data(), S.d_rev.p, sizeof(int32_t) * S.m, hipMemcpyDeviceToHost));
        STEREO_HIP_CHECK(hipMemcpy(r.data(), S.d_r.p, sizeof(double) * S.m, hipMemcpyDeviceToHost));
        const double tw1 = now();
        weak_persistencies(S.P, r, label);
        unl = 0;
        for (int64_t i = 0; i < N; ++i) if (label[i] < 0) unl += 1;
        std::vector<int8_t> l8(N);
        for (int64_t i = 0; i < N; ++i) l8[i] = (int8_t)label[i];
        P->d_label.upload(l8.data(), N);
        if (verbose) std::fprintf(stderr, "[stereo_hip qpbo plan] weak persistency: %.3f ms to fetch the residual network, %.3f ms on the host\n", tw1 - tw0, now() - tw1);
      }
      *num_unlabelled = unl;  // rd_mex.cpp:83-88: counted before Improve
      if (improve && unl > 0) {
        const double ti0 = now();
        const std::vector<int32_t> perm = improve_permutation(N);
        if (verbose) std::fprintf(stderr, "[stereo_hip qpbo plan] Improve: permutation %.3f ms\n", now() - ti0);
        S.improve(opt, perm, h);   // (returns the final heights)
        std::vector<int8_t> l8(N);
        for (int64_t i = 0; i < N; ++i) l8[i] = (int8_t)label_from_heights(h[i], h[i + N], n, 0);   // QPBO_extra.cpp:1210-1219: ambiguous -> user label (0)
        P->d_label.upload(l8.data(), N);
        if (verbose) std::fprintf(stderr, "[stereo_hip qpbo plan] Improve: %.3f ms\n", now() - ti0);
      }
    }
    *num_unlabelled = unl;
    if (verbose)
      std::fprintf(stderr, "[stereo_hip qpbo plan] n=%d arcs=%d iterations=%lld global_relabels=%lld unlabelled=%g\n", S.n,
                   S.m, (long long)S.iterations, (long long)S.relabels, unl);
    if (labelling) {
      std::vector<int8_t> l8(N);
      STEREO_HIP_CHECK(hipMemcpy(l8.data(), P->d_label.p, N, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < N; ++i) labelling[i] = l8[i];
    }
    if (unl32 > 0) {   // labels changed on the host (weak persistency, Improve): the energy of the final labelling
      hipLaunchKernelGGL(rd_energy_terms_kernel, dim3((unsigned)((N + E + kQB - 1) / kQB)), dim3(kQB), 0, 0, N, E,
                         P->d_conn.p, S.g.h, n, in[0], in[1], in[2], in[3], in[4], in[5], P->d_label.p, P->d_terms.p);
      *energy = det_sum(P->d_terms.p, N + E, P->d_partial);
    } else {
      *energy = sums.get(s_energy);
    }
    STEREO_HIP_CHECK(hipGetLastError());
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  } catch (const std::exception &e) {
    return fail(std::string("stereo_rd: ") + e.what(), err, errcap);
  }
}

extern "C" const int8_t *stereo_rd_plan_device_labels(stereo_rd_plan *P) { return P ? P->d_label.p : nullptr; }

extern "C" int stereo_rd_plan_set_grid(stereo_rd_plan *P, int H, int W, char *err, size_t errcap) {
  if (!P) return fail("stereo_rd_plan_set_grid: NULL plan", err, errcap);
  if (H < 1 || W < 1 || (int64_t)H * W != P->N) return fail("stereo_rd_plan_set_grid: H * W must equal N", err, errcap);
  try {
    P->S.set_tiling(P->N, H, W);
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

namespace {

// the six HOST arrays go to the plan's input buffers first
int rd_plan_solve_host(stereo_rd_plan *P, const QpboOptions &opt, const double *U0, const double *U1, const double *E00,
                       const double *E01, const double *E10, const double *E11, int improve, double *labelling,
                       double *energy, double *lower_bound, double *num_unlabelled, char *err, size_t errcap) {
  if (!P || !U0 || !U1 || !labelling || !energy || !lower_bound || !num_unlabelled ||
      (P->E > 0 && (!E00 || !E01 || !E10 || !E11)))
    return fail("stereo_rd_plan_solve: NULL argument", err, errcap);
  try {
    const double *src[6] = {U0, U1, E00, E01, E10, E11};
    const double *in[6];
    for (int k = 0; k < 6; ++k) {
      P->d_in[k].upload(src[k], k < 2 ? P->N : P->E);
      in[k] = P->d_in[k].p;
    }
    return rd_plan_solve_device(P, opt, in, improve, labelling, energy, lower_bound, num_unlabelled, err, errcap);
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

}  // namespace

extern "C" int stereo_rd_plan_solve(stereo_rd_plan *P, const double *U0, const double *U1, const double *E00,
                                    const double *E01, const double *E10, const double *E11, int improve,
                                    double *labelling, double *energy, double *lower_bound,
                                    double *num_unlabelled, char *err, size_t errcap) {
  return rd_plan_solve_host(P, QpboOptions::from_env(), U0, U1, E00, E01, E10, E11, improve, labelling, energy, lower_bound,
                            num_unlabelled, err, errcap);
}

extern "C" int stereo_rd_plan_solve_device(stereo_rd_plan *P, const double *d_U0, const double *d_U1,
                                           const double *d_E00, const double *d_E01, const double *d_E10,
                                           const double *d_E11, int improve, double *labelling, double *energy,
                                           double *lower_bound, double *num_unlabelled, char *err,
                                           size_t errcap) {
  if (!P || !d_U0 || !d_U1 || !energy || !lower_bound || !num_unlabelled)
    return fail("stereo_rd_plan_solve_device: NULL argument", err, errcap);
  const double *in[6] = {d_U0, d_U1, d_E00, d_E01, d_E10, d_E11};
  return rd_plan_solve_device(P, QpboOptions::from_env(), in, improve, labelling, energy, lower_bound, num_unlabelled, err, errcap);
}
