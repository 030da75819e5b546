// Development / CI tool (tests/test_strip_beliefs_cpu.py): the host-side builder of a strip's belief lists
// (stereo_amd/csrc/trws_graph*.cpp: build_strip_belief_lists behind stereo_trws_strip_belief_lists_host) under
// AddressSanitizer + UndefinedBehaviorSanitizer, over the CPU test's grids and strip counts, with arrays of exactly the
// sizes the entry reports.  Prints SANITIZE_STRIP_LISTS_OK.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Iinclude tools/sanitize_strip_lists.cpp stereo_amd/csrc/trws_graph*.cpp -lpthread
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/stereo_hip.h"

namespace stereo {
std::string &last_error() {
  static thread_local std::string s;
  return s;
}
}  // namespace stereo

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static std::vector<uint32_t> grid(int H, int W) {   // tests/helpers.py: grid_conn
  std::vector<uint32_t> c;
  for (int x = 0; x < W; ++x) for (int r = 0; r + 1 < H; ++r) { c.push_back(x * H + r); c.push_back(x * H + r + 1); }
  for (int x = 0; x + 1 < W; ++x) for (int r = 0; r < H; ++r) { c.push_back(x * H + r); c.push_back((x + 1) * H + r); }
  return c;
}

int main() {
  char err[512];
  const int shapes[][2] = {{9, 40}, {8, 6}, {5, 7}};
  for (auto &s : shapes) {
    const int H = s[0], W = s[1];
    const int64_t N = (int64_t)H * W;
    const std::vector<uint32_t> conn = grid(H, W);
    const int64_t E = (int64_t)conn.size() / 2;
    for (int G = 1; G <= 4; ++G) {
      std::vector<int32_t> owner(N);
      for (int64_t i = 0; i < N; ++i) owner[i] = (int32_t)(((i % H) * G) / H);
      int64_t own_total = 0, fwd_total = 0, bwd_total = 0;
      for (int g = 0; g < G; ++g) {
        int64_t n_own = -1, n_fwd = -1, n_bwd = -1;
        EXPECT(stereo_trws_strip_belief_lists_host(N, E, conn.data(), G > 1 ? owner.data() : nullptr, G, g, &n_own, &n_fwd, &n_bwd,
                                                   nullptr, nullptr, nullptr, nullptr, nullptr, err, sizeof(err)) == 0);
        if (n_own < 0) { std::printf("%dx%d G %d strip %d: %s\n", H, W, G, g, err); continue; }
        std::vector<int32_t> own(n_own), fptr(n_own + 1), fidx(n_fwd), bptr(n_own + 1), bidx(n_bwd);
        EXPECT(stereo_trws_strip_belief_lists_host(N, E, conn.data(), G > 1 ? owner.data() : nullptr, G, g, nullptr, nullptr, nullptr,
                                                   own.data(), fptr.data(), fidx.data(), bptr.data(), bidx.data(), err, sizeof(err)) == 0);
        EXPECT(fptr[0] == 0 && fptr[n_own] == n_fwd && bptr[0] == 0 && bptr[n_own] == n_bwd);
        for (int64_t j = 0; j < n_own; ++j) EXPECT(own[j] >= 0 && own[j] < n_own && fptr[j] <= fptr[j + 1] && bptr[j] <= bptr[j + 1]);
        // any single output alone
        EXPECT(stereo_trws_strip_belief_lists_host(N, E, conn.data(), G > 1 ? owner.data() : nullptr, G, g, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, fidx.data(), nullptr, nullptr, err, sizeof(err)) == 0);
        own_total += n_own; fwd_total += n_fwd; bwd_total += n_bwd;
      }
      // every node is some strip's own; every edge is on one forward and one backward list
      EXPECT(own_total == N && fwd_total == E && bwd_total == E);
    }
    // refusals touch nothing
    std::vector<int32_t> owner(N, 0);
    EXPECT(stereo_trws_strip_belief_lists_host(N, E, conn.data(), owner.data(), 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, err, sizeof(err)) != 0);
    EXPECT(stereo_trws_strip_belief_lists_host(N, E, conn.data(), nullptr, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, err, sizeof(err)) != 0);
    EXPECT(stereo_trws_strip_belief_lists_host(N, E, nullptr, owner.data(), 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, 0) != 0);
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("SANITIZE_STRIP_LISTS_OK\n");
  return 0;
}
