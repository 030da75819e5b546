// Development / CI tool: the builder of the runner's chain records (stereo_amd/csrc/trws_runner_records.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the host, on the graphs of tests/test_runner_records_cpu.py: twin and
// single-edged grids, a chain that is no multiple of the segment length, a grid with tripled border pairs (more than
// four incoming rows), sub-row descriptor sets, every chain run of every graph (not only the one that is cut), and the
// degenerate ranges.  Nothing is loaded into Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Iinclude tools/sanitize_runner_records.cpp stereo_amd/csrc/trws_graph*.cpp
//       stereo_amd/csrc/trws_runner_records.cpp -lpthread                                            (one command line)
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../stereo_amd/csrc/trws_graph.h"
#include "../stereo_amd/csrc/trws_runner_records.h"

namespace stereo {
std::string &last_error() {
  static thread_local std::string s;
  return s;
}
}  // namespace stereo

using stereo::TrwsGraph;

static int fails = 0;

// 4-neighbourhood, node id = column * H + row; copies: 2 twin edges, 1 every pair once; border3: one more edge per border pair
static std::vector<uint32_t> grid(int H, int W, int copies, bool border3) {
  std::vector<uint32_t> c;
  auto add = [&](int a, int b) { c.push_back(a); c.push_back(b); };
  auto on_border = [&](int x, int r) { return x == 0 || x == W - 1 || r == 0 || r == H - 1; };
  for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) { add(x * H + r, x * H + r + 1); if (copies > 1) add(x * H + r + 1, x * H + r); }
  for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) { add(x * H + r, (x + 1) * H + r); if (copies > 1) add((x + 1) * H + r, x * H + r); }
  if (border3) {
    for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) if (on_border(x, r) && on_border(x, r + 1)) add(x * H + r, x * H + r + 1);
    for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) if (on_border(x, r) && on_border(x + 1, r)) add(x * H + r, (x + 1) * H + r);
  }
  return c;
}

static void check(const std::vector<int32_t> &desc, int32_t c0, int32_t c1, int32_t L, int32_t nseg, const char *what) {
  std::vector<int32_t> rec;
  stereo::build_runner_records(desc.data(), c0, c1, L, nseg, rec);
  const size_t n = c1 > c0 ? (size_t)(c1 - c0) : 0;
  bool ok = rec.size() == n * stereo::kRecWords;
  for (size_t j = 0; ok && j < n; ++j) {
    const int32_t *R = &rec[j * stereo::kRecWords];
    ok = R[15] == 0 && R[14] == desc[(size_t)(c0 + j) * TrwsGraph::kDescWords] && R[stereo::kRecKfirst] >= 0 && R[stereo::kRecKfirst] <= 30 &&
         (R[5] == 0 || (R[5] > 0 && R[5] < nseg)) && R[stereo::kRecStage] < 8 && R[stereo::kRecMsg] < 4 && R[stereo::kRecMsg + 1] < 4;
  }
  if (!ok) { std::printf("%s: records [%d, %d) seg %d x %d\n", what, c0, c1, L, nseg); ++fails; }
}

static void run(const char *what, int H, int W, int copies, bool border3, int seg, int64_t chunk_f, int64_t chunk_b, int64_t resident) {
  const std::vector<uint32_t> conn = grid(H, W, copies, border3);
  stereo::TrwsGraphOptions opt;
  opt.max_resident_runs = 256; opt.seg_len = seg; opt.row_chunk_forward = chunk_f; opt.row_chunk_backward = chunk_b; opt.chunk_resident = resident;
  TrwsGraph g;
  std::string err;
  if (!stereo::build_trws_graph((int64_t)H * W, (int64_t)conn.size() / 2, conn.data(), opt, g, err)) { std::printf("%s: %s\n", what, err.c_str()); ++fails; return; }
  if (!g.fast_ok) { std::printf("%s: no descriptors\n", what); ++fails; return; }
  for (int d = 0; d < 2; ++d) {
    const TrwsGraph::Sweep &S = g.sweep[d];
    const TrwsGraph::Sweep::Spec &s0 = g.sweep[0].spec;
    if (S.spec.ok) check(S.desc, S.spec.c0, S.spec.c1, s0.seg_len, s0.nseg, what);
    if (S.chunked.ok && S.chunked.spec.ok) check(S.chunked.desc, S.chunked.spec.c0, S.chunked.spec.c1, s0.seg_len, s0.nseg, what);
    // every run of the chain schedule, cut or not, and the degenerate ranges
    for (size_t k = 0; k + 1 < S.chain_run_ptr.size(); ++k) {
      const int32_t a = S.chain_run_ptr[k], b = S.chain_run_ptr[k + 1];
      check(S.desc, a, b, seg, (b - a) / seg, what);
      check(S.desc, a, b, 1, b - a, what);
    }
    check(S.desc, 0, 0, seg, 0, what);
    check(S.desc, 3, 3, 0, 0, what);
    check(S.desc, 0, 1, 0, 0, what);
    check(S.desc, 0, (int32_t)(S.desc.size() / TrwsGraph::kDescWords), 1 << 30, 1, what);
  }
}

int main() {
  run("12x9", 12, 9, 2, false, 4, 0, -1, 0);
  run("9x12", 9, 12, 2, false, 4, 0, -1, 0);
  run("30x40", 30, 40, 2, false, 16, 0, -1, 0);
  run("30x40 sub-rows", 30, 40, 2, false, 16, 12, 12, 2);
  run("30x40 sub-rows backward", 30, 40, 2, false, 16, 0, 12, 4);
  run("13x10", 13, 10, 2, false, 4, 0, -1, 0);
  run("single 30x40", 30, 40, 1, false, 16, 0, -1, 0);
  run("tripled border 14x19", 14, 19, 2, true, 4, 0, -1, 0);
  std::printf(fails ? "SANITIZE_RUNNER_RECORDS_FAILED\n" : "SANITIZE_RUNNER_RECORDS_OK\n");
  return fails ? 1 : 0;
}
