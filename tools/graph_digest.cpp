// Development / CI tool: pins every bit of what the host-side graph analysis produces.  For a fixed set of graphs and
// options it builds a TrwsGraph and prints one line per case -- case id, "ok" or the error text, and a 64-bit FNV-1a
// digest over every field of the graph (vectors as length + bytes; with strips also every strip's layout and belief
// lists).  tests/test_graph_digest_cpu.py compares the lines with tests/golden/trws_graph_digests.txt, recorded before
// the analysis was split into stages; a restructuring of the analysis must leave every line as it is.
//   g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tools/graph_digest.cpp
//       stereo_amd/csrc/trws_graph*.cpp -lpthread           (one command line)
//   ./a.out > tests/golden/trws_graph_digests.txt      (re-record; only ever on a commit whose output is the truth)
// The fixture was recorded on commit 0ff1655 with this file and that commit's trws_graph.cpp as the only other source,
// the body of build() below replaced by the one statement
//   return stereo::build_trws_graph(N, E, conn, g, err, p.max_resident_runs, p.owner, p.nstrips, p.certainly_resident,
//                                   p.ordering, p.row_chunk, p.chunk_resident, p.row_chunk_backward);
// Two runs gave the same bytes.
//   ./a.out --time H W                                 (host time of the analysis on the H x W twin-edge grid)
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../stereo_amd/csrc/trws_graph.h"

namespace stereo {
std::string &last_error() {
  static thread_local std::string s;
  return s;
}
}  // namespace stereo

using stereo::TrwsGraph;

// what a case asks of build_trws_graph
struct Params {
  int64_t max_resident_runs = 0;
  const int32_t *owner = nullptr;
  int nstrips = 1;
  int64_t certainly_resident = 256;
  int ordering = 0;
  int64_t row_chunk = 0, chunk_resident = 0, row_chunk_backward = -1;
};

static bool build(int64_t N, int64_t E, const uint32_t *conn, const Params &p, TrwsGraph &g, std::string &err) {
  stereo::TrwsGraphOptions opt;
  opt.max_resident_runs = p.max_resident_runs; opt.owner = p.owner; opt.nstrips = p.nstrips;
  opt.certainly_resident = p.certainly_resident; opt.ordering = p.ordering; opt.row_chunk_forward = p.row_chunk;
  opt.chunk_resident = p.chunk_resident; opt.row_chunk_backward = p.row_chunk_backward;
  return stereo::build_trws_graph(N, E, conn, opt, g, err);
}

// ---- digest
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void *p, size_t n) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 0x100000001b3ull; }
  }
  template <class T> void pod(T v) { bytes(&v, sizeof(v)); }
  void flag(bool b) { pod<uint8_t>(b ? 1 : 0); }
  template <class T> void vec(const std::vector<T> &v) { pod<uint64_t>(v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};

static void hash_spec(Fnv &f, const TrwsGraph::Sweep::Spec &s) {
  f.flag(s.ok); f.pod(s.run); f.pod(s.c0); f.pod(s.c1); f.pod(s.seg_len); f.pod(s.nseg); f.pod(s.max_len);
  f.vec(s.run_ptr); f.vec(s.run_order); f.vec(s.kind);
}

static void hash_graph(Fnv &f, const TrwsGraph &g) {
  f.pod(g.N); f.pod(g.E); f.vec(g.tail); f.vec(g.head); f.vec(g.mdir); f.vec(g.order); f.vec(g.rank);
  f.vec(g.fptr); f.vec(g.fidx); f.vec(g.bptr); f.vec(g.bidx); f.vec(g.gamma);
  f.vec(g.level_ptr); f.vec(g.level_ranks); f.pod(g.max_level_nodes); f.vec(g.lb_pos_node); f.vec(g.lb_pos_edge); f.pod(g.lb_terms);
  f.vec(g.owner); f.pod<int32_t>(g.nstrips); f.vec(g.strip_lb_terms); f.vec(g.strip_nodes); f.vec(g.e_pos); f.flag(g.fast_ok);
  for (int d = 0; d < 2; ++d) {
    const TrwsGraph::Sweep &S = g.sweep[d];
    f.vec(S.run_ptr); f.vec(S.run_order); f.vec(S.dep_ptr); f.vec(S.dep_rank); f.vec(S.in_slot); f.vec(S.desc);
    f.vec(S.chain_rank); f.vec(S.chain_run_ptr); f.vec(S.chain_run_order); f.vec(S.run_strip); f.vec(S.chain_run_strip);
    hash_spec(f, S.spec);
    f.flag(S.chunked.ok); f.pod(S.chunked.chunk); f.vec(S.chunked.desc); f.vec(S.chunked.run_ptr); f.vec(S.chunked.run_order);
    hash_spec(f, S.chunked.spec);
  }
}

static void hash_strips(Fnv &f, const TrwsGraph &g) {
  for (int s = 0; s < g.nstrips; ++s) {
    stereo::StripLayout L;
    std::string err;
    const bool ok = stereo::build_strip_layout(g, s, L, err);
    f.flag(ok); f.bytes(err.data(), err.size());
    f.pod(L.n_own); f.vec(L.nodes); f.vec(L.edges);
    for (int d = 0; d < 2; ++d) { f.vec(L.desc[d]); f.vec(L.run_ptr[d]); f.flag(L.need_peer[d]); }
    stereo::StripBeliefLists B;
    err.clear();
    const bool okb = stereo::build_strip_belief_lists(g, s, L.nodes, L.edges, B, err);
    f.flag(okb); f.bytes(err.data(), err.size());
    f.vec(B.own); f.vec(B.fptr); f.vec(B.fidx); f.vec(B.bptr); f.vec(B.bidx);
  }
}

// ---- branch counts: the digest must keep reaching every stage of the analysis
static int64_t n_builds, n_fast, n_spec, n_chunked, n_chunked_spec, n_run_order, n_chain_order;

static void run_case(const std::string &id, int64_t N, const std::vector<uint32_t> &conn, const Params &p) {
  TrwsGraph g;
  std::string err;
  Fnv f;
  const int64_t E = (int64_t)conn.size() / 2;
  ++n_builds;
  if (!build(N, E, conn.data(), p, g, err)) {
    f.bytes(err.data(), err.size());
    std::printf("%s %s %016llx\n", id.c_str(), err.c_str(), (unsigned long long)f.h);
    return;
  }
  hash_graph(f, g);
  if (g.nstrips > 1 && g.fast_ok) hash_strips(f, g);
  n_fast += g.fast_ok;
  for (int d = 0; d < 2; ++d) {
    const TrwsGraph::Sweep &S = g.sweep[d];
    n_spec += S.spec.ok; n_chunked += S.chunked.ok; n_chunked_spec += S.chunked.ok && S.chunked.spec.ok;
    n_run_order += !S.run_order.empty(); n_chain_order += !S.chain_run_order.empty();
  }
  std::printf("%s ok %016llx\n", id.c_str(), (unsigned long long)f.h);
}

// ---- graphs
static uint64_t state;
static uint32_t rnd(uint32_t n) {
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return (uint32_t)((state >> 33) % n);
}

// 4-neighbourhood, node id = column * H + row; twin: every pair as two directed edges, else once (low id first)
static std::vector<uint32_t> grid(int H, int W, bool twin) {
  std::vector<uint32_t> c;
  auto add = [&](int a, int b) { c.push_back(a); c.push_back(b); };
  for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) add(x * H + r, x * H + r + 1);
  if (twin) for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) add(x * H + r + 1, x * H + r);
  for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) add(x * H + r, (x + 1) * H + r);
  if (twin) for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) add((x + 1) * H + r, x * H + r);
  return c;
}

static std::vector<uint32_t> flat(std::initializer_list<std::pair<int, int>> edges) {
  std::vector<uint32_t> c;
  for (auto &e : edges) { c.push_back(e.first); c.push_back(e.second); }
  return c;
}

static std::string tag(const char *fmt, ...) {
  char buf[128];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

static void grid_cases(const std::string &pre) {
  const int shapes[][2] = {{6, 8}, {1, 9}, {9, 1}, {2, 2}, {37, 5}, {5, 41}, {24, 31}, {40, 48}, {70, 90}};
  for (auto &s : shapes)
    for (int twin = 1; twin >= 0; --twin) {
      const int H = s[0], W = s[1];
      const int64_t N = (int64_t)H * W;
      const std::vector<uint32_t> conn = grid(H, W, twin);
      const std::string base = pre + tag("%c%dx%d", twin ? 't' : 's', H, W);
      for (int64_t mrr : {0, 4, 64})
        for (int64_t cr : {256, 2})
          for (int ordering : {0, 1}) {
            Params p; p.max_resident_runs = mrr; p.certainly_resident = cr; p.ordering = ordering;
            run_case(base + tag(".m%d.c%d.o%d", (int)mrr, (int)cr, ordering), N, conn, p);
          }
      for (int64_t chunk : {4, 8, 16})
        for (int64_t cres : {0, 2, 16})
          for (int64_t back : {-1, 0, 5}) {
            Params p; p.max_resident_runs = 256; p.row_chunk = chunk; p.chunk_resident = cres; p.row_chunk_backward = back;
            run_case(base + tag(".k%d.r%d.b%d", (int)chunk, (int)cres, (int)back), N, conn, p);
          }
      for (int G = 2; G <= 4 && G <= H; ++G) {
        std::vector<int32_t> owner(N);
        for (int64_t i = 0; i < N; ++i) owner[i] = (int32_t)(((i % H) * G) / H);
        for (int64_t mrr : {0, 4}) {
          Params p; p.max_resident_runs = mrr; p.owner = owner.data(); p.nstrips = G;
          run_case(base + tag(".G%d.m%d", G, (int)mrr), N, conn, p);
        }
      }
    }
}

static void random_cases(const std::string &pre) {
  state = 0x9E3779B97F4A7C15ull;
  for (int trial = 0; trial < 300; ++trial) {
    const int64_t N = 3 + rnd(60);
    const bool capped = trial % 3 != 2;   // at most 8 incident edges per node: the descriptor kernels' range
    std::vector<int> deg(N, 0);
    std::vector<uint32_t> conn;
    const int64_t want = 1 + rnd((uint32_t)(capped ? 2 * N : 3 * N));
    for (int64_t e = 0; e < want; ++e) {
      const uint32_t a = rnd((uint32_t)N), b = rnd((uint32_t)N);
      if (a == b || (capped && (deg[a] >= 8 || deg[b] >= 8))) continue;
      conn.push_back(a); conn.push_back(b); ++deg[a]; ++deg[b];
    }
    if (conn.empty()) { conn.push_back(0); conn.push_back(1); }
    Params p;
    p.max_resident_runs = (trial & 1) ? 3 : 0; p.certainly_resident = (trial & 2) ? 2 : 256; p.row_chunk = (trial & 4) ? 4 : 0;
    run_case(pre + tag("r%d", trial), N, conn, p);
  }
}

static void family_cases(const std::string &pre) {
  // tests/graph_families.py: DEADLOCK8, SPEC_DEADLOCK172, SPEC_DEADLOCK302
  run_case(pre + "deadlock8", 8, flat({{0, 1}, {0, 2}, {1, 3}, {2, 4}, {1, 5}, {5, 6}, {3, 7}, {5, 2}, {3, 5}, {6, 2}}), Params());
  {
    std::vector<uint32_t> c;
    for (int i = 0; i < 169; ++i) { c.push_back(i); c.push_back(i + 1); }
    for (auto &e : {std::pair<int, int>{170, 171}, {171, 8}, {10, 170}}) { c.push_back(e.first); c.push_back(e.second); }
    run_case(pre + "specdead172", 172, c, Params());
  }
  {
    std::vector<uint32_t> c;
    for (int i = 0; i < 297; ++i) { c.push_back(i); c.push_back(i + 1); }
    for (auto &e : {std::pair<int, int>{298, 299}, {229, 299}, {298, 231}, {301, 300}, {301, 227}, {300, 229}}) { c.push_back(e.first); c.push_back(e.second); }
    run_case(pre + "specdead302", 302, c, Params());
  }
  for (int64_t mrr : {0, 4}) {
    Params p; p.max_resident_runs = mrr;
    {   // ring, both directions of every pair
      const int n = 300;
      std::vector<uint32_t> c;
      for (int i = 0; i < n; ++i) { c.push_back(i); c.push_back((i + 1) % n); }
      for (int i = 0; i < n; ++i) { c.push_back((i + 1) % n); c.push_back(i); }
      run_case(pre + tag("ring.m%d", (int)mrr), n, c, p);
    }
    {   // the 14 x 19 grid under a random renumbering of its nodes
      const int H = 14, W = 19;
      std::vector<uint32_t> perm(H * W), c = grid(H, W, true);
      for (int i = 0; i < H * W; ++i) perm[i] = i;
      state = 0x2545F4914F6CDD1Dull;
      for (int i = H * W - 1; i > 0; --i) std::swap(perm[i], perm[rnd(i + 1)]);
      for (auto &v : c) v = perm[v];
      run_case(pre + tag("permgrid.m%d", (int)mrr), H * W, c, p);
    }
    {   // 8 x 9 grid numbered row by row
      const int H = 8, W = 9;
      std::vector<uint32_t> c = grid(H, W, true);
      for (auto &v : c) v = (v % H) * W + v / H;
      run_case(pre + tag("rowmajor.m%d", (int)mrr), H * W, c, p);
    }
  }
}

static void refusal_cases(const std::string &pre) {
  const std::vector<uint32_t> tri = flat({{0, 1}, {1, 2}, {2, 3}});
  const int32_t own_ok[4] = {0, 0, 1, 1}, own_bad[4] = {0, 0, 1, 5}, own_far[4] = {0, 0, 2, 2};
  Params p;
  run_case(pre + "x.empty", 0, tri, p);
  run_case(pre + "x.range", 3, tri, p);
  run_case(pre + "x.loop", 4, flat({{0, 1}, {2, 2}}), p);
  p.nstrips = 0; run_case(pre + "x.nstrips", 4, tri, p);
  p.nstrips = 2; run_case(pre + "x.noowner", 4, tri, p);
  p.owner = own_bad; run_case(pre + "x.owner", 4, tri, p);
  p.nstrips = 3; p.owner = own_far; run_case(pre + "x.far", 4, tri, p);
  p.nstrips = 2; p.owner = own_ok; run_case(pre + "x.fine", 4, tri, p);
}

static void print_counts(const char *what) {
  std::printf("counts %s builds %lld fast_ok %lld spec %lld chunked %lld chunked_spec %lld run_order %lld chain_run_order %lld\n",
              what, (long long)n_builds, (long long)n_fast, (long long)n_spec, (long long)n_chunked, (long long)n_chunked_spec,
              (long long)n_run_order, (long long)n_chain_order);
  n_builds = n_fast = n_spec = n_chunked = n_chunked_spec = n_run_order = n_chain_order = 0;
}

static void whole_set(const std::string &pre) {
  grid_cases(pre); random_cases(pre); family_cases(pre); refusal_cases(pre);
}

static int time_mode(int H, int W) {
  const std::vector<uint32_t> conn = grid(H, W, true);
  Params p; p.max_resident_runs = 256; p.row_chunk = 16;
  std::vector<double> ms;
  for (int i = 0; i < 5; ++i) {
    TrwsGraph g;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    if (!build((int64_t)H * W, (int64_t)conn.size() / 2, conn.data(), p, g, err)) { std::printf("%s\n", err.c_str()); return 1; }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  std::printf("%dx%d: median %.1f ms, range %.1f .. %.1f ms\n", H, W, ms[2], ms[0], ms[4]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--time")) return time_mode(std::atoi(argv[2]), std::atoi(argv[3]));
  unsetenv("STEREO_HIP_TRWS_SPEC_SEG");
  whole_set("");
  print_counts("seg16");
  setenv("STEREO_HIP_TRWS_SPEC_SEG", "4", 1);
  whole_set("4/");
  print_counts("seg4");
  return 0;
}
