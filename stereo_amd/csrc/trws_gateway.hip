// ---- the gateway entry: what trws_mex reaches ------------------------------------------------------------
// A simultaneous fusion through trws.m:33 calls the gateway once per move with the SAME connectivity
// (dispmap_super.m:153-198: the neighbourhood of the object), and fronto-parallel proposals make every column
// of q and qprim one and the same vector (:177-183 evaluates each plane at every edge: [0 0 1 -d] gives d).
// So the gateway (i) keeps the plan of the last (kernel, K, N, E, connectivity, message mode, device) -- graph
// analysis, descriptors and device buffers survive the call -- and (ii) looks at q / qprim on the host before
// uploading anything: if all 2 E columns are bitwise one vector, that vector goes up as the plan's shared
// positions (8 K bytes instead of 16 K E) and the shared-position kernels run; results are the K x E form's bit
// for bit (tests/test_trws_gpu.py).  STEREO_HIP_TRWS_CACHE=0: a plan per call, K x E arrays always uploaded.
// File map: trws_plan.hip.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <thread>

#include "trws_plan.h"

using namespace stereo;

namespace {

// true iff every column of q and of qprim (K x E, column-major) equals q's first column bit for bit
bool columns_are_one_vector(const double *q, const double *qprim, int K, int64_t E) {
  if (E < 1) return false;
  const size_t row = sizeof(double) * (size_t)K;
  if (std::memcmp(q, qprim, row) != 0) return false;
  // a quick look at a few columns first: general planes differ on the first edge already
  for (int64_t e : {E / 2, E - 1})
    if (std::memcmp(q, q + (size_t)e * K, row) != 0 || std::memcmp(q, qprim + (size_t)e * K, row) != 0) return false;
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(nt ? nt : 1u, 16u));
  if ((size_t)E * K < (1u << 20)) nt = 1;
  std::vector<char> same(nt, 1);
  auto scan = [&](unsigned t) {
    const int64_t a = E * t / nt, b = E * (t + 1) / nt;
    for (int64_t e = a; e < b; ++e)
      if (std::memcmp(q, q + (size_t)e * K, row) != 0 || std::memcmp(q, qprim + (size_t)e * K, row) != 0) { same[t] = 0; return; }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(scan, t);
  scan(0);
  for (auto &x : th) x.join();
  for (char c : same) if (!c) return false;
  return true;
}

// beliefs: run with the plan's belief flag on and read min-marginals (K x N) / confidence (N), either may be NULL;
// otherwise the flag is off (a plan the min-marginal entry used before pays nothing)
int trws_solve_on(stereo_trws_plan *P, const double *unary, const double *q, const double *qprim, const double *alphas,
                  double tol, double maxiter, double max_relgap, bool look_for_shared, double *labelling, double *energy,
                  double *lower_bound, double *iterations, char *err, size_t errcap, bool beliefs = false,
                  double *min_marginals = nullptr, double *confidence = nullptr) {
  int rc;
  if (beliefs || P->keep_mm) {
    rc = stereo_trws_plan_keep_min_marginals(P, beliefs ? 1 : 0, err, errcap);
    if (rc) return rc;
  }
  if (look_for_shared && columns_are_one_vector(q, qprim, P->K, P->E))
    rc = stereo_trws_plan_upload(P, unary, nullptr, nullptr, q, alphas, tol, err, errcap);
  else
    rc = stereo_trws_plan_upload(P, unary, q, qprim, nullptr, alphas, tol, err, errcap);
  if (rc) return rc;
  // Minimize_TRW_S always runs at least one iteration (minimize.cpp:31,100-101)
  int itmax = (int)maxiter;  // trws_mex.cpp:125
  if (itmax < 1) itmax = 1;
  rc = stereo_trws_plan_iterate(P, itmax, max_relgap, nullptr, nullptr, nullptr, err, errcap);
  if (rc) return rc;
  rc = stereo_trws_plan_result(P, labelling, energy, lower_bound, iterations, err, errcap);
  if (rc || !beliefs || (!min_marginals && !confidence)) return rc;
  return stereo_trws_plan_min_marginals(P, min_marginals, confidence, nullptr, err, errcap);
}

// ---- the gateway on several devices (STEREO_HIP_GPUS = G): row strips of the image grid ---------------------------
// trws_mex hands over a graph, not an image; the image grid of dispmap_super.m:279-302 is recognised from it: nodes
// col * H + row (:281-282), every edge joins vertical (|a - b| == 1, same column) or horizontal (|a - b| == H)
// neighbours.  Band g of the rows goes to strip g; strip g runs on device g when the process sees at least G devices
// (peer access, stereo_trws_plan_connect), otherwise all strips share the current device as logical strips (one fused
// launch per sweep) -- the same kernels, the same hand-over protocol, the same bits.  Anything else (another graph, a
// label count the strip kernels do not take) stays on one device.
int64_t image_grid_height(int64_t N, int64_t E, const uint32_t *conn) {
  int64_t H = 0;
  for (int64_t e = 0; e < E; ++e) {
    const int64_t a = conn[2 * e], b = conn[2 * e + 1];
    const int64_t d = a > b ? a - b : b - a;
    if (d == 1) continue;
    if (H == 0) H = d;
    if (d != H) return 0;
  }
  if (H < 2 || N % H != 0) return 0;
  for (int64_t e = 0; e < E; ++e) {   // vertical edges stay inside a column
    const int64_t a = conn[2 * e], b = conn[2 * e + 1];
    if ((a > b ? a - b : b - a) == 1 && a / H != b / H) return 0;
  }
  return H;
}

// The terms of the bound and of the energy in the order ONE plan adds them (rank N - 1 down to 0: the node's own term, then
// one per message; rank 0 up: one per node), as runs of consecutive terms of one strip: a strip numbers its terms in that
// same order, so a run is as long as consecutive ranks stay with one owner (a band of rows: a few runs per image row at
// most).  Summed this way the gateway's two scalars are the single plan's to the last bit -- and with them the stop test
// and the iteration count (minimize.cpp:105).
struct TermRuns {
  std::vector<int32_t> strip;
  std::vector<int64_t> start, count;
  void add(int s, int64_t pos, int64_t n) {
    if (!strip.empty() && strip.back() == s && start.back() + count.back() == pos) { count.back() += n; return; }
    strip.push_back(s); start.push_back(pos); count.push_back(n);
  }
};

struct TrwsStripSet {
  std::vector<stereo_trws_plan *> plans;
  std::vector<int32_t> owner;
  TermRuns lb_runs, en_runs;
  bool one_device = true;
  ~TrwsStripSet() { for (stereo_trws_plan *P : plans) if (P) stereo_trws_plan_destroy(P); }
};

int strips_create(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn, int mode, int G, int64_t H, TrwsStripSet &S, char *err,
                  size_t errcap) {
  S.owner.resize(N);
  for (int64_t i = 0; i < N; ++i) S.owner[i] = (int32_t)std::min<int64_t>((i % H) * G / H, G - 1);
  const int ndev = stereo_hip_device_count();
  S.one_device = ndev < G;
  int home = 0;
  if (hipGetDevice(&home) != hipSuccess) return fail("stereo_trws: no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, home);
  const int per_strip = S.one_device ? std::max(2, cus / G) : 0;   // logical strips must all be resident together
  S.plans.assign(G, nullptr);
  int rc = 0;
  for (int g = 0; g < G && !rc; ++g) {
    if (!S.one_device && hipSetDevice(g) != hipSuccess) rc = fail("stereo_trws: hipSetDevice failed", err, errcap);
    if (!rc) rc = stereo_trws_plan_create_strip(kernel, K, N, E, conn, mode, g == 0 ? S.owner.data() : nullptr, G, g, per_strip,
                                                g ? S.plans[0] : nullptr, &S.plans[g], err, errcap);
  }
  (void)hipSetDevice(home);
  for (int g = 0; g < G && !rc; ++g) {
    if (g > 0) rc = stereo_trws_plan_connect(S.plans[g], 0, S.plans[g - 1], err, errcap);
    if (!rc && g + 1 < G) rc = stereo_trws_plan_connect(S.plans[g], 1, S.plans[g + 1], err, errcap);
  }
  if (!rc) {
    const TrwsGraph &g = *S.plans[0]->graph;
    for (int64_t r = N - 1; r >= 0; --r) {
      const int s = S.owner[g.order[r]];
      S.lb_runs.add(s, g.lb_pos_node[r], 1);
      for (int32_t k = g.bptr[r]; k < g.bptr[r + 1]; ++k) S.lb_runs.add(s, g.lb_pos_edge[g.bidx[k]], 1);
    }
    for (int64_t r = 0; r < N; ++r) S.en_runs.add(S.owner[g.order[r]], g.e_pos[r], 1);
  }
  return rc;
}

// The strips' belief rows put together at their node ids.  Logical strips: one grouped launch into arrays of the whole
// problem on the device; strips on devices of their own: each strip's own rows, scattered on the host.
int strips_min_marginals(TrwsStripSet &S, double *min_marginals, double *confidence, char *err, size_t errcap) {
  const int G = (int)S.plans.size();
  const stereo_trws_plan *P0 = S.plans[0];
  const size_t K = (size_t)P0->K;
  try {
    if (S.one_device) {
      DevBuf<double> d_mm, d_conf;
      if (min_marginals) d_mm.alloc((size_t)P0->N * K);
      if (confidence) d_conf.alloc((size_t)P0->N);
      if (int rc = stereo_trws_plans_min_marginals_device(S.plans.data(), G, d_mm.p, d_conf.p, nullptr, nullptr, err, errcap)) return rc;
      if (min_marginals) STEREO_HIP_CHECK(hipMemcpy(min_marginals, d_mm.p, sizeof(double) * (size_t)P0->N * K, hipMemcpyDeviceToHost));
      if (confidence) STEREO_HIP_CHECK(hipMemcpy(confidence, d_conf.p, sizeof(double) * (size_t)P0->N, hipMemcpyDeviceToHost));
      return 0;
    }
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
  std::vector<double> mm, conf;
  for (int g = 0; g < G; ++g) {
    const StripLayout &L = *S.plans[g]->layout;
    if (min_marginals) mm.resize((size_t)L.n_own * K);
    if (confidence) conf.resize((size_t)L.n_own);
    if (int rc = stereo_trws_plan_strip_min_marginals(S.plans[g], min_marginals ? mm.data() : nullptr, confidence ? conf.data() : nullptr,
                                                      nullptr, err, errcap)) return rc;
    for (int64_t j = 0; j < L.n_own; ++j) {
      if (min_marginals) std::memcpy(min_marginals + (size_t)L.nodes[j] * K, &mm[(size_t)j * K], sizeof(double) * K);
      if (confidence) confidence[L.nodes[j]] = conf[j];
    }
  }
  return 0;
}

// beliefs: as trws_solve_on -- every strip runs with its belief flag on and the rows are read afterwards
int strips_solve(TrwsStripSet &S, const double *unary, const double *q, const double *qprim, const double *alphas, double tol,
                 double maxiter, double max_relgap, double *labelling, double *energy, double *lower_bound, double *iterations, char *err,
                 size_t errcap, bool beliefs = false, double *min_marginals = nullptr, double *confidence = nullptr) {
  const int G = (int)S.plans.size();
  stereo_trws_plan *P0 = S.plans[0];
  for (int g = 0; g < G; ++g)
    if (beliefs || S.plans[g]->keep_mm)
      if (int rc = stereo_trws_plan_strip_keep_min_marginals(S.plans[g], beliefs ? 1 : 0, err, errcap)) return rc;
  const bool shared = columns_are_one_vector(q, qprim, P0->K, P0->E);
  for (int g = 0; g < G; ++g) {
    const int rc = shared ? stereo_trws_plan_upload(S.plans[g], unary, nullptr, nullptr, q, alphas, tol, err, errcap)
                          : stereo_trws_plan_upload(S.plans[g], unary, q, qprim, nullptr, alphas, tol, err, errcap);
    if (rc) return rc;
  }
  int itmax = (int)maxiter;  // trws_mex.cpp:125; Minimize_TRW_S always runs at least one iteration (minimize.cpp:31,100-101)
  if (itmax < 1) itmax = 1;
  double lb = 0, en = 0;
  int done = 0;
  for (int it = 0; it < itmax; ++it) {
    int rc = 0;
    if (S.one_device) rc = stereo_trws_plans_issue(S.plans.data(), G, nullptr, err, errcap);
    else for (int g = 0; g < G && !rc; ++g) rc = stereo_trws_plan_issue(S.plans[g], nullptr, err, errcap);
    if (rc) return rc;
    // every strip's terms are on the host behind its collect; they are added in the order one plan adds them (TermRuns)
    for (int g = 0; g < G; ++g)
      if ((rc = stereo_trws_plan_collect(S.plans[g], nullptr, nullptr, err, errcap)) != 0) return rc;
    lb = 0; en = 0;
    for (size_t k = 0; k < S.lb_runs.strip.size(); ++k) {
      const double *t = S.plans[S.lb_runs.strip[k]]->h_lb.p + S.lb_runs.start[k];
      for (int64_t i = 0; i < S.lb_runs.count[k]; ++i) lb += t[i];
    }
    for (size_t k = 0; k < S.en_runs.strip.size(); ++k) {
      const double *t = S.plans[S.en_runs.strip[k]]->h_en.p + S.en_runs.start[k];
      for (int64_t i = 0; i < S.en_runs.count[k]; ++i) en += t[i];
    }
    for (int g = 0; g < G; ++g) (void)stereo_trws_plan_commit(S.plans[g], lb, en, err, errcap);
    ++done;
    if ((en - lb) / en < max_relgap) break;  // minimize.cpp:105
  }
  std::vector<double> part((size_t)P0->N);
  for (int g = 0; g < G; ++g) {
    const int rc = stereo_trws_plan_result(S.plans[g], part.data(), nullptr, nullptr, nullptr, err, errcap);
    if (rc) return rc;
    for (int64_t i = 0; i < P0->N; ++i)
      if (S.owner[i] == g) labelling[i] = part[i];
  }
  *energy = en; *lower_bound = lb; *iterations = (double)done;
  if (!beliefs || (!min_marginals && !confidence)) return 0;
  return strips_min_marginals(S, min_marginals, confidence, err, errcap);
}

// how many strips the gateway should cut the problem into (1: the plain single-device plan)
int gateway_strips(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn, const double *q, const double *qprim, int mode, int64_t *H_out) {
  const char *ge = trws_switch(kSwGpus);
  const int G = ge ? std::atoi(ge) : 1;
  if (G < 2 || G > kMaxGroup || mode != STEREO_TRWS_MESSAGES_EXACT) return 1;
  // a label count some strip family takes on an image grid; where none takes q / qprim per edge (K > 128), only with
  // one shared positions vector
  TrwsPlanFacts f;
  f.kernel = kernel; f.K = K; f.fast_ok = true; f.strips = true;
  const TrwsInputFacts per_edge;
  const char *why = nullptr;
  if (trws_family(f, nullptr, &why) == TrwsFamily::None) return 1;
  if (trws_family(f, &per_edge, &why) == TrwsFamily::None && !columns_are_one_vector(q, qprim, K, E)) return 1;
  const int64_t H = image_grid_height(N, E, conn);
  if (H < 2 * G) return 1;
  *H_out = H;
  return G;
}

// The cache: the plan of the last problem, or its row strips (G > 1).  conn points at the caller's array in a key
// made for a lookup and at the entry's own copy in the key that is kept.
struct TrwsCacheKey {
  int kernel = 0, K = 0, mode = 0, device = -1, G = 0;
  int64_t N = 0, E = 0;
  std::string env;   // trws_env_key
  const uint32_t *conn = nullptr;
  bool operator==(const TrwsCacheKey &o) const {
    return kernel == o.kernel && K == o.K && mode == o.mode && device == o.device && G == o.G && N == o.N && E == o.E && env == o.env &&
           std::memcmp(conn, o.conn, sizeof(uint32_t) * 2 * (size_t)E) == 0;
  }
};

struct TrwsCache {
  std::mutex mu;
  stereo_trws_plan *plan = nullptr;
  TrwsStripSet *strips = nullptr;
  TrwsCacheKey key;
  std::vector<uint32_t> conn;
  void clear() {
    if (plan) { stereo_trws_plan_destroy(plan); plan = nullptr; }
    if (strips) { delete strips; strips = nullptr; }
  }
};

TrwsCache &trws_cache() {
  static TrwsCache *C = new TrwsCache;   // (never destroyed: the HIP runtime may be gone before static destructors run)
  return *C;
}

// A plan (S == nullptr) or a strip set for the key's problem.
int gateway_create(const TrwsCacheKey &k, int64_t gridH, stereo_trws_plan **P, TrwsStripSet *S, char *err, size_t errcap) {
  if (S) return strips_create(k.kernel, k.K, k.N, k.E, k.conn, k.mode, k.G, gridH, *S, err, errcap);
  return stereo_trws_plan_create(k.kernel, k.K, k.N, k.E, k.conn, k.mode, P, err, errcap);
}

thread_local int g_last_gateway_strips = 0;   // what the last stereo_trws call of this thread ran on (stereo_trws_gateway_strips)

// The gateway behind stereo_trws and stereo_trws_min_marginals.  beliefs: ONE plan (strips give the same bits) unless
// STEREO_HIP_TRWS_BELIEFS_STRIPS=1 asks for the strips of stereo_trws's rule; G is part of the cache key.
int trws_gateway(int kernel, const double *unary, const uint32_t *conn, const double *q, const double *qprim, const double *alphas,
                 double tol, double maxiter, double max_relgap, int K, int64_t N, int64_t E, double *labelling, double *energy,
                 double *lower_bound, double *iterations, bool beliefs, double *min_marginals, double *confidence, char *err,
                 size_t errcap) {
  if (kernel != 1 && kernel != 2) return fail("Unsupported kernel", err, errcap);  // trws_mex.cpp:162
  if (!unary || !conn || !q || !qprim || !alphas || !labelling || !energy || !lower_bound || !iterations)
    return fail("stereo_trws: NULL argument", err, errcap);
  TrwsCacheKey key;
  key.kernel = kernel; key.K = K; key.N = N; key.E = E; key.conn = conn;
  key.mode = STEREO_TRWS_MESSAGES_EXACT;
  if (const char *m = std::getenv("STEREO_HIP_TRWS_MESSAGES"))
    if (std::string(m) == "minplus") key.mode = STEREO_TRWS_MESSAGES_MINPLUS;
  const char *ce = std::getenv("STEREO_HIP_TRWS_CACHE");
  const bool cached = (!ce || std::atoi(ce) != 0) && E > 0 && N > 0;
  int64_t gridH = 0;
  bool shard = !beliefs;
  if (const char *bs = trws_switch(kSwBeliefsStrips)) shard = shard || std::atoi(bs) == 1;
  key.G = (E > 0 && N > 0 && shard) ? gateway_strips(kernel, K, N, E, conn, q, qprim, key.mode, &gridH) : 1;
  g_last_gateway_strips = key.G;
  auto solve = [&](stereo_trws_plan *P, TrwsStripSet *S, bool look_for_shared) {
    if (S) return strips_solve(*S, unary, q, qprim, alphas, tol, maxiter, max_relgap, labelling, energy, lower_bound, iterations, err, errcap,
                               beliefs, min_marginals, confidence);
    return trws_solve_on(P, unary, q, qprim, alphas, tol, maxiter, max_relgap, look_for_shared, labelling, energy, lower_bound,
                         iterations, err, errcap, beliefs, min_marginals, confidence);
  };
  if (!cached) {
    TrwsStripSet S;
    stereo_trws_plan *P = nullptr;
    int rc = gateway_create(key, gridH, &P, key.G > 1 ? &S : nullptr, err, errcap);
    // (above 512 labels only the shared positions vector is taken: look for it there)
    if (!rc) rc = solve(P, key.G > 1 ? &S : nullptr, K > kGenericMaxK);
    if (P) stereo_trws_plan_destroy(P);
    return rc;
  }
  TrwsCache &C = trws_cache();
  std::lock_guard<std::mutex> lock(C.mu);
  if (hipGetDevice(&key.device) != hipSuccess) return fail("stereo_trws: no HIP device available (the HIP path has no CPU fallback)", err, errcap);
  key.env = trws_env_key();
  if (!((C.plan || C.strips) && C.key == key)) {
    C.clear();
    std::unique_ptr<TrwsStripSet> S(key.G > 1 ? new TrwsStripSet : nullptr);
    const int rc = gateway_create(key, gridH, &C.plan, S.get(), err, errcap);
    if (rc) return rc;
    C.strips = S.release();
    C.conn.assign(conn, conn + 2 * (size_t)E);
    C.key = key; C.key.conn = C.conn.data();
  }
  const int rc = solve(C.plan, C.strips, true);
  if (rc) C.clear();   // never keep plans an error went through
  return rc;
}

}  // namespace

extern "C" {

int stereo_trws_gateway_strips(void) { return g_last_gateway_strips; }

void stereo_trws_cache_clear(void) {
  TrwsCache &C = trws_cache();
  std::lock_guard<std::mutex> lock(C.mu);
  C.clear();
  C.conn.clear(); C.conn.shrink_to_fit();
}

int stereo_trws(int kernel, const double *unary, const uint32_t *conn, const double *q,
                const double *qprim, const double *alphas, double tol, double maxiter,
                double max_relgap, int K, int64_t N, int64_t E, double *labelling, double *energy,
                double *lower_bound, double *iterations, char *err, size_t errcap) {
  return trws_gateway(kernel, unary, conn, q, qprim, alphas, tol, maxiter, max_relgap, K, N, E, labelling, energy, lower_bound,
                      iterations, false, nullptr, nullptr, err, errcap);
}

int stereo_trws_min_marginals(int kernel, const double *unary, const uint32_t *conn, const double *q,
                              const double *qprim, const double *alphas, double tol, double maxiter,
                              double max_relgap, int K, int64_t N, int64_t E, double *labelling, double *energy,
                              double *lower_bound, double *iterations, double *min_marginals, double *confidence,
                              char *err, size_t errcap) {
  return trws_gateway(kernel, unary, conn, q, qprim, alphas, tol, maxiter, max_relgap, K, N, E, labelling, energy, lower_bound,
                      iterations, true, min_marginals, confidence, err, errcap);
}

}  // extern "C"
