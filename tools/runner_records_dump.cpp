// Development / CI tool: the runner's chain records (stereo_amd/csrc/trws_runner_records.cpp) next to the descriptors
// they were made from, for tests/test_runner_records_cpu.py.  Nothing is loaded into Python.
//   g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tools/runner_records_dump.cpp
//       stereo_amd/csrc/trws_graph*.cpp stereo_amd/csrc/trws_runner_records.cpp -lpthread        (one command line)
//   ./a.out graph.txt seg_len row_chunk_forward row_chunk_backward chunk_resident [longest]
// graph.txt: N E, then E lines "tail head" (zero-based).  For every direction and every descriptor set the K <= 64
// runner can be launched on (the chain schedule's; the sub-row schedule's where it exists) one block:
//   set <direction> <sub> <c0> <c1> <seg_len> <nseg>
//   c1 - c0 lines of kDescWords descriptor words, then c1 - c0 lines of kRecWords record words
// with the segment geometry bound the way make_params binds it (seg_len and nseg of the forward chain schedule).
// `longest`: the records of the chain schedule's longest run in segments of seg_len, whether or not the graph keeps the
// speculative schedule (the builder is a function of the descriptors alone; a chain node with more than four incoming
// rows never gets that schedule, trws_graph_desc.cpp: runner_can_walk).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static void dump(int d, int sub, const std::vector<int32_t> &desc, const TrwsGraph::Sweep::Spec &sp, const TrwsGraph::Sweep::Spec &s0) {
  constexpr int DW = TrwsGraph::kDescWords;
  std::vector<int32_t> rec;
  stereo::build_runner_records(desc.data(), sp.c0, sp.c1, s0.seg_len, s0.nseg, rec);
  std::printf("set %d %d %d %d %d %d\n", d, sub, (int)sp.c0, (int)sp.c1, (int)s0.seg_len, (int)s0.nseg);
  for (int32_t i = sp.c0; i < sp.c1; ++i) {
    for (int k = 0; k < DW; ++k) std::printf("%d%c", (int)desc[(size_t)i * DW + k], k + 1 < DW ? ' ' : '\n');
  }
  for (int32_t i = 0; i < sp.c1 - sp.c0; ++i) {
    for (int k = 0; k < stereo::kRecWords; ++k) std::printf("%d%c", (int)rec[(size_t)i * stereo::kRecWords + k], k + 1 < stereo::kRecWords ? ' ' : '\n');
  }
}

int main(int argc, char **argv) {
  if (argc != 6 && argc != 7) { std::fprintf(stderr, "usage: %s graph.txt seg_len row_chunk_forward row_chunk_backward chunk_resident\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  long long N = 0, E = 0;
  if (!f || std::fscanf(f, "%lld %lld", &N, &E) != 2 || N < 1 || E < 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<uint32_t> conn(2 * (size_t)E);
  for (size_t i = 0; i < conn.size(); ++i) {
    unsigned v;
    if (std::fscanf(f, "%u", &v) != 1) { std::fprintf(stderr, "%s is short\n", argv[1]); return 2; }
    conn[i] = v;
  }
  std::fclose(f);
  stereo::TrwsGraphOptions opt;
  opt.max_resident_runs = 256;
  opt.seg_len = std::atoi(argv[2]);
  opt.row_chunk_forward = std::atoi(argv[3]); opt.row_chunk_backward = std::atoi(argv[4]); opt.chunk_resident = std::atoi(argv[5]);
  TrwsGraph g;
  std::string err;
  if (!stereo::build_trws_graph(N, E, conn.data(), opt, g, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  if (argc == 7) {
    if (!g.fast_ok || opt.seg_len < 1) { std::printf("none\n"); return 0; }
    for (int d = 0; d < 2; ++d) {
      const TrwsGraph::Sweep &S = g.sweep[d];
      TrwsGraph::Sweep::Spec sp;
      for (size_t k = 0; k + 1 < S.chain_run_ptr.size(); ++k)
        if (S.chain_run_ptr[k + 1] - S.chain_run_ptr[k] > sp.c1 - sp.c0) { sp.c0 = S.chain_run_ptr[k]; sp.c1 = S.chain_run_ptr[k + 1]; }
      sp.seg_len = opt.seg_len; sp.nseg = (sp.c1 - sp.c0) / opt.seg_len;
      dump(d, 0, S.desc, sp, sp);
    }
    return 0;
  }
  const TrwsGraph::Sweep::Spec &s0 = g.sweep[0].spec;
  if (!g.fast_ok || !s0.ok || !g.sweep[1].spec.ok) { std::printf("none\n"); return 0; }
  for (int d = 0; d < 2; ++d) {
    const TrwsGraph::Sweep &S = g.sweep[d];
    dump(d, 0, S.desc, S.spec, s0);
    if (S.chunked.ok && S.chunked.spec.ok) dump(d, 1, S.chunked.desc, S.chunked.spec, s0);
  }
  return 0;
}
