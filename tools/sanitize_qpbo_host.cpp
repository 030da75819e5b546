// Development / CI tool: the QPBO host code that makes no HIP call (stereo_amd/csrc/qpbo_graph.cpp, qpbo_rand.cpp:
// pair grouping, the doubled graph, weak persistency in both forms, the Improve permutation) under
// AddressSanitizer + UndefinedBehaviorSanitizer, checked against first principles:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude \
//       tools/sanitize_qpbo_host.cpp stereo_amd/csrc/qpbo_graph.cpp stereo_amd/csrc/qpbo_rand.cpp
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../stereo_amd/csrc/qpbo_host.h"

using namespace stereo;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return (uint32_t)((state >> 33) % n);
}
static bool chance(double p) { return rnd(1000000) < p * 1000000; }

static int fails = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- (a) weak persistency: full pass == compact pass == the strongly connected components of the free residual graph

// A doubled graph over the variable pairs `pairs` (repeats allowed), every pair sub- or supermodular at random, the
// four arcs of a pair in the order build_problem emits them (arc a and its reverse a ^ 1), grouped by tail.
static void doubled_graph(int N, const std::vector<std::pair<int, int>> &pairs, QpboProblem &P) {
  struct Arc { int tail, head; };
  std::vector<Arc> arcs;
  for (const auto &pr : pairs) {
    const int i = pr.first, j = pr.second, im = i + N, jm = j + N;
    if (rnd(2)) { arcs.push_back({i, j}); arcs.push_back({j, i}); arcs.push_back({jm, im}); arcs.push_back({im, jm}); }
    else { arcs.push_back({i, jm}); arcs.push_back({jm, i}); arcs.push_back({j, im}); arcs.push_back({im, j}); }
  }
  const int n = 2 * N, m = (int)arcs.size();
  P.N = N;
  P.aptr.assign(n + 1, 0);
  for (const Arc &a : arcs) ++P.aptr[a.tail + 1];
  for (int v = 0; v < n; ++v) P.aptr[v + 1] += P.aptr[v];
  std::vector<int32_t> fill(P.aptr.begin(), P.aptr.end() - 1), newid(m);
  for (int a = 0; a < m; ++a) newid[a] = fill[arcs[a].tail]++;
  P.head.assign(m, 0); P.rev.assign(m, 0);
  for (int a = 0; a < m; ++a) { P.head[newid[a]] = arcs[a].head; P.rev[newid[a]] = newid[a ^ 1]; }
}

static std::vector<std::pair<int, int>> grid_pairs(int H, int W) {
  std::vector<std::pair<int, int>> p;
  for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) p.push_back({x * H + r, x * H + r + 1});
  for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) p.push_back({x * H + r, (x + 1) * H + r});
  return p;
}

static int comparable_checked = 0, decided_total = 0;

// residual with probability p on every arc, 60 % of the variables free; returns the largest arc count of a node
static int check_weak(int N, const std::vector<std::pair<int, int>> &pairs, double p, const char *what) {
  QpboProblem P;
  doubled_graph(N, pairs, P);
  const int n = 2 * N, m = (int)P.head.size();
  std::vector<double> r(m);
  for (int a = 0; a < m; ++a) r[a] = chance(p) ? 1.0 + rnd(5) : 0.0;
  std::vector<int> label(N);
  std::vector<int32_t> ids;
  for (int i = 0; i < N; ++i) {
    label[i] = chance(0.6) ? -1 : (int)rnd(2);
    if (label[i] < 0) ids.push_back(i);
  }
  const int cnt = (int)ids.size();
  int maxdeg = 0;
  for (int v = 0; v < n; ++v) maxdeg = std::max(maxdeg, (int)(P.aptr[v + 1] - P.aptr[v]));
  // the full pass
  std::vector<int> full = label;
  weak_persistencies(P, r, full);
  for (int i = 0; i < N; ++i)
    if (label[i] >= 0) EXPECT(full[i] == label[i], "%s: a labelled variable changed", what);
  // the compact pass on what rd_free_arcs_kernel gathers
  std::vector<int32_t> heads((size_t)2 * cnt * std::max(maxdeg, 1), -1);
  std::vector<uint8_t> flags((size_t)2 * cnt * std::max(maxdeg, 1), 0);
  for (int t = 0; t < 2 * cnt; ++t) {
    const int v = t < cnt ? ids[t] : ids[t - cnt] + N;
    for (int k = 0; k < P.aptr[v + 1] - P.aptr[v]; ++k) {
      const int a = P.aptr[v] + k;
      heads[(size_t)t * maxdeg + k] = P.head[a];
      flags[(size_t)t * maxdeg + k] = (uint8_t)((r[a] > 0 ? 1 : 0) | (r[P.rev[a]] > 0 ? 2 : 0));
    }
  }
  std::vector<int8_t> lab;
  weak_persistencies_compact(cnt, N, ids, maxdeg, heads, flags, lab);
  EXPECT((int)lab.size() == cnt, "%s: compact pass returned %d labels for %d variables", what, (int)lab.size(), cnt);
  for (int t = 0; t < cnt && t < (int)lab.size(); ++t)
    EXPECT(lab[t] == full[ids[t]], "%s: variable %d: full %d, compact %d", what, ids[t], full[ids[t]], (int)lab[t]);
  // reachability among the free nodes by transitive closure
  std::vector<uint8_t> is_free(n, 0);
  for (int i : ids) is_free[i] = is_free[i + N] = 1;
  std::vector<std::vector<uint8_t>> reach(n, std::vector<uint8_t>(n, 0));
  for (int v = 0; v < n; ++v) {
    if (!is_free[v]) continue;
    reach[v][v] = 1;
    for (int a = P.aptr[v]; a < P.aptr[v + 1]; ++a)
      if (r[a] > 0 && is_free[P.head[a]]) reach[v][P.head[a]] = 1;
  }
  for (int k = 0; k < n; ++k)
    for (int u = 0; u < n; ++u)
      if (reach[u][k])
        for (int v = 0; v < n; ++v) reach[u][v] |= reach[k][v];
  for (int i : ids) {
    const bool to_mate = reach[i][i + N], from_mate = reach[i + N][i];
    EXPECT((full[i] >= 0) == !(to_mate && from_mate), "%s: variable %d decided %d, one component with its mate %d", what, i,
           full[i], (int)(to_mate && from_mate));
    decided_total += full[i] >= 0;
    if (to_mate != from_mate) {   // comparable components: the direction fixes the label
      ++comparable_checked;
      EXPECT(full[i] == (from_mate ? 0 : 1), "%s: variable %d: mate reaches it %d, it reaches the mate %d, label %d", what, i,
             (int)from_mate, (int)to_mate, full[i]);
    }
  }
  return maxdeg;
}

static void test_weak_persistency() {
  const int shapes[][2] = {{5, 6}, {1, 7}, {2, 2}};
  const double ps[] = {0.3, 0.5, 0.7};
  for (int rep = 0; rep < 60; ++rep)
    for (auto &s : shapes)
      for (double p : ps) {
        if (s[0] != 5 && rep >= 20) continue;   // (the small shapes: fewer draws)
        check_weak(s[0] * s[1], grid_pairs(s[0], s[1]), p, "grid");
      }
  int dense = 0;
  for (int rep = 0; rep < 12; ++rep) {   // random multigraphs, more than 16 arcs at some node
    const int N = 4 + (int)rnd(5);
    std::vector<std::pair<int, int>> pairs;
    for (int e = 0; e < 12 * N; ++e) {
      const int a = (int)rnd(N), b = (int)rnd(N);
      if (a != b) pairs.push_back({std::min(a, b), std::max(a, b)});
    }
    dense += check_weak(N, pairs, ps[rep % 3] * 0.3, "multigraph") > 16;
  }
  EXPECT(dense >= 6, "only %d multigraphs with more than 16 arcs at a node", dense);
  EXPECT(comparable_checked >= 100, "the direction check fired on %d variables only (%d decided)", comparable_checked, decided_total);
  std::printf("weak persistency: %d variables decided, direction checked on %d\n", decided_total, comparable_checked);
}

// ---- (b) pair grouping and the doubled graph

// E(x) of the caller's tables == const0 + sum_i tr_i x_i + 1/2 sum_arcs cap [x_tail = 0][x_head = 1], x_(i + N) = 1 - x_i
// (every term of the normal form appears on an arc and on its mirror)
static void check_normal_form(int N, const std::vector<uint32_t> &conn, const char *what) {
  const int E = (int)conn.size() / 2;
  std::vector<double> U0(N), U1(N), E00(E), E01(E), E10(E), E11(E);
  for (int i = 0; i < N; ++i) { U0[i] = rnd(20); U1[i] = rnd(20); }
  for (int e = 0; e < E; ++e) { E00[e] = rnd(20); E01[e] = rnd(20); E10[e] = rnd(20); E11[e] = rnd(20); }
  QpboProblem P;
  std::string err;
  const bool ok = build_problem(U0.data(), U1.data(), E00.data(), E01.data(), E10.data(), E11.data(), E ? conn.data() : nullptr, N, E, P, err);
  EXPECT(ok, "%s: build_problem: %s", what, err.c_str());
  if (!ok) return;
  const int n = 2 * N, m = (int)P.head.size();
  EXPECT((int)P.aptr.size() == n + 1 && P.aptr[n] == m && (int)P.tr.size() == n, "%s: sizes", what);
  std::vector<int> tail(m);
  for (int v = 0; v < n; ++v) for (int a = P.aptr[v]; a < P.aptr[v + 1]; ++a) tail[a] = v;
  for (int a = 0; a < m; ++a) {
    EXPECT(P.rev[P.rev[a]] == a && P.rev[a] != a, "%s: rev is not an involution at arc %d", what, a);
    EXPECT(P.head[P.rev[a]] == tail[a], "%s: the reverse of arc %d does not lead back", what, a);
    EXPECT(P.cap[a] >= 0, "%s: negative capacity", what);
  }
  for (int i = 0; i < N; ++i) EXPECT(P.tr[i + N] == -P.tr[i], "%s: mate terminal", what);
  for (int x = 0; x < (1 << N); ++x) {
    auto lab = [&](int v) { return v < N ? (x >> v) & 1 : 1 - ((x >> (v - N)) & 1); };
    double direct = 0, twice = 0;
    for (int i = 0; i < N; ++i) direct += lab(i) ? U1[i] : U0[i];
    for (int e = 0; e < E; ++e) {
      const int xi = lab(conn[2 * e]), xj = lab(conn[2 * e + 1]);
      direct += xi ? (xj ? E11[e] : E10[e]) : (xj ? E01[e] : E00[e]);
    }
    double normal = P.const0;
    for (int i = 0; i < N; ++i) normal += P.tr[i] * lab(i);
    for (int a = 0; a < m; ++a) twice += (!lab(tail[a]) && lab(P.head[a])) ? P.cap[a] : 0.0;
    EXPECT(direct == normal + twice / 2, "%s: labelling %d: energy %g, normal form %g", what, x, direct, normal + twice / 2);
  }
}

static void test_grouping_and_build() {
  // parallel, antiparallel and duplicated edges: pairs (0,1) <- e0, e1 (transposed), e2; (0,2) <- e5; (1,2) <- e3 (transposed), e4
  const std::vector<uint32_t> conn = {0, 1, 1, 0, 0, 1, 2, 1, 1, 2, 0, 2};
  PairGroups G;
  std::string err;
  EXPECT(group_pairs(conn.data(), 3, 6, G, err), "group_pairs: %s", err.c_str());
  EXPECT((G.pi == std::vector<int32_t>{0, 0, 1}) && (G.pj == std::vector<int32_t>{1, 2, 2}), "pair list");
  EXPECT((G.pe_ptr == std::vector<int32_t>{0, 3, 4, 6}), "edge ranges");
  EXPECT((G.pe_edge == std::vector<int32_t>{0, 3, 4, 10, 7, 8}), "edges of the pairs, input order, transposed bit");
  check_normal_form(3, conn, "merged edges");
  check_normal_form(4, {3, 0, 0, 3, 3, 0, 1, 2, 2, 1, 0, 1, 0, 1, 2, 3}, "merged edges, four variables");
  check_normal_form(4, {0, 1, 1, 2, 2, 3, 3, 0}, "simple cycle");
  check_normal_form(3, {}, "no edges");
  // E = 0
  EXPECT(group_pairs(nullptr, 5, 0, G, err) && G.npairs() == 0 && G.pe_ptr == std::vector<int32_t>{0} && G.pe_edge.empty(), "E = 0");
  // refusals
  const uint32_t out_of_range[4] = {0, 1, 1, 3}, self_loop[4] = {0, 1, 2, 2};
  EXPECT(!group_pairs(out_of_range, 3, 2, G, err) && err == "connectivity index out of range", "out of range: %s", err.c_str());
  EXPECT(!group_pairs(self_loop, 3, 2, G, err) && err == "stereo_rd: self loops are not supported", "self loop: %s", err.c_str());
  EXPECT(!group_pairs(nullptr, (int64_t)1 << 30, 0, G, err), "2 N beyond 32-bit ids");
  QpboProblem P;
  double u[3] = {0, 0, 0}, t[2] = {0, 0};
  EXPECT(!build_problem(u, u, t, t, t, t, self_loop, 3, 2, P, err), "build_problem accepted a self loop");
  EXPECT(!build_problem(u, u, t, t, t, t, out_of_range, 3, 2, P, err), "build_problem accepted an index out of range");
  EXPECT(!build_problem(u, u, t, t, t, t, nullptr, 0, 0, P, err), "build_problem accepted N = 0");
  // the grid hint
  std::vector<uint32_t> g;
  for (auto &pr : grid_pairs(5, 6)) { g.push_back(pr.first); g.push_back(pr.second); }
  EXPECT(grid_height_of(g.data(), 30, (int64_t)g.size() / 2) == 5, "grid hint");
  g[1] = 7;
  EXPECT(grid_height_of(g.data(), 30, (int64_t)g.size() / 2) == 0, "grid hint on a graph that is no grid");
}

// ---- (c) the Improve permutation: the plain rand() loop of QPBO_extra.cpp:13-27, the generator left where that loop leaves it

static void test_permutation() {
  for (int round = 0; round < 2; ++round)
    for (int64_t N : {0, 1, 2, 1000}) {
      srand(1234 + (unsigned)N);
      std::vector<int32_t> want((size_t)N);
      for (int64_t i = 0; i < N; ++i) want[i] = (int32_t)i;
      for (int64_t i = 0; i < N - 1; ++i) {
        int64_t j = i + (int64_t)((rand() / (1.0 + (double)RAND_MAX)) * (double)(N - i));
        if (j > N - 1) j = N - 1;
        std::swap(want[i], want[j]);
      }
      const int next_want = rand();
      srand(1234 + (unsigned)N);
      const std::vector<int32_t> got = improve_permutation(N);
      const int next_got = rand();
      EXPECT(got == want, "improve_permutation(%lld) differs from the rand() loop", (long long)N);
      EXPECT(next_got == next_want, "improve_permutation(%lld) leaves the generator elsewhere", (long long)N);
    }
}

int main() {
  test_weak_persistency();
  test_grouping_and_build();
  test_permutation();
  std::printf(fails ? "SANITIZE_QPBO_HOST_FAILED (%d)\n" : "SANITIZE_QPBO_HOST_OK\n", fails);
  return fails ? 1 : 0;
}
