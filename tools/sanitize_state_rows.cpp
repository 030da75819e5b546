// Development / CI tool (tests/test_trws_state_cpu.py): the host-side rules of the TRW-S solver state
// (stereo_amd/csrc/trws_state.h behind stereo_trws_state_check and stereo_trws_strip_state_rows_host)
// under AddressSanitizer + UndefinedBehaviorSanitizer, with arrays of exactly the sizes the entries take.
// Prints SANITIZE_STATE_ROWS_OK.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Iinclude tools/sanitize_state_rows.cpp stereo_amd/csrc/trws_graph*.cpp -lpthread
#include <cstdint>
#include <cstdio>
#include <cstring>
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
  char why[256];
  const int shapes[][2] = {{6, 8}, {9, 40}, {5, 7}};
  for (auto &s : shapes) {
    const int H = s[0], W = s[1];
    const int64_t N = (int64_t)H * W;
    const std::vector<uint32_t> conn = grid(H, W);
    const int64_t E = (int64_t)conn.size() / 2;
    for (int G = 2; G <= 4; ++G) {
      std::vector<int32_t> owner(N);
      for (int64_t i = 0; i < N; ++i) owner[i] = (int32_t)(((i % H) * G) / H);
      for (int phase = 0; phase < 2; ++phase) {
        std::vector<int> count(E, 0);
        for (int g = 0; g < G; ++g) {
          std::vector<uint8_t> take(E, 7);
          EXPECT(stereo_trws_strip_state_rows_host(N, E, conn.data(), owner.data(), G, g, phase, take.data()) == 0);
          for (int64_t e = 0; e < E; ++e) { EXPECT(take[e] <= 1); count[e] += take[e]; }
        }
        for (int64_t e = 0; e < E; ++e) EXPECT(count[e] == 1);
      }
      // refusals touch nothing
      std::vector<uint8_t> take(E, 7);
      EXPECT(stereo_trws_strip_state_rows_host(N, E, conn.data(), owner.data(), G, G, 1, take.data()) != 0);
      EXPECT(stereo_trws_strip_state_rows_host(N, E, conn.data(), owner.data(), G, 0, 2, take.data()) != 0);
      EXPECT(stereo_trws_strip_state_rows_host(N, E, conn.data(), nullptr, G, 0, 1, take.data()) != 0);
      EXPECT(stereo_trws_strip_state_rows_host(N, E, conn.data(), owner.data(), G, 0, 1, nullptr) != 0);
      for (int64_t e = 0; e < E; ++e) EXPECT(take[e] == 7);
    }
    // the refusal rule: a header that fits, then one field at a time, with reason buffers of several sizes
    stereo_trws_state_header h;
    std::memset(&h, 0, sizeof(h));
    h.magic = STEREO_TRWS_STATE_MAGIC; h.version = STEREO_TRWS_STATE_VERSION; h.kernel = 1; h.K = 5; h.N = N; h.E = E;
    h.phase = 1; h.iterations = 3;
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, conn.data(), 0, why, sizeof(why)) != 0);   // (no key yet)
    EXPECT(std::strstr(why, "connectivity_key") != nullptr);
    // the key: FNV-1a over the words, restated
    uint64_t key = 0xcbf29ce484222325ull;
    for (uint32_t w : conn) { key ^= w; key *= 0x100000001b3ull; }
    h.connectivity_key = key;
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, conn.data(), 0, why, sizeof(why)) == 0 && why[0] == 0);
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, conn.data(), STEREO_TRWS_MESSAGES_MINPLUS, nullptr, 0) == 0);
    EXPECT(stereo_trws_state_check(&h, 2, 5, N, E, conn.data(), 0, why, sizeof(why)) != 0 && std::strstr(why, "kernel"));
    EXPECT(stereo_trws_state_check(&h, 1, 6, N, E, conn.data(), 0, why, 8) != 0 && std::strlen(why) == 7);
    EXPECT(stereo_trws_state_check(&h, 1, 5, N + 1, E, conn.data(), 0, why, 1) != 0 && why[0] == 0);
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E - 1, conn.data(), 0, nullptr, 0) != 0);
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, conn.data(), STEREO_TRWS_ORDER_INDEX, why, sizeof(why)) != 0 && std::strstr(why, "message_mode"));
    EXPECT(stereo_trws_state_check(nullptr, 1, 5, N, E, conn.data(), 0, why, sizeof(why)) != 0);
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, nullptr, 0, why, sizeof(why)) != 0);
    h.phase = 3;
    EXPECT(stereo_trws_state_check(&h, 1, 5, N, E, conn.data(), 0, why, sizeof(why)) != 0 && std::strstr(why, "phase"));
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("SANITIZE_STATE_ROWS_OK\n");
  return 0;
}
