// Development / CI tool (tests/test_band_carry_cpu.py): the host side of the carried messages --
// stereo_trws_state_receivers_host and the argument checks behind stereo_band_carry / stereo_band_carry_device
// (stereo_amd/csrc/carry_host.cpp) -- under AddressSanitizer + UndefinedBehaviorSanitizer, with arrays of exactly the
// sizes the entries take.  Prints SANITIZE_CARRY_OK.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Iinclude tools/sanitize_carry.cpp stereo_amd/csrc/carry_host.cpp \
//       stereo_amd/csrc/trws_graph*.cpp -lpthread
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/stereo_hip.h"
#include "../stereo_amd/csrc/carry_host.h"

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

static bool refused(const stereo::carry::Args &a, const char *names) {
  char why[200];
  why[0] = 0;
  const int rc = stereo::carry::check_args("carry", a, why, sizeof(why));
  return rc != 0 && std::strstr(why, names) != nullptr;
}

int main() {
  char why[256];
  const int shapes[][2] = {{6, 8}, {5, 7}, {1, 9}, {9, 1}, {1, 1}};
  for (auto &s : shapes) {
    const int H = s[0], W = s[1];
    const int64_t N = (int64_t)H * W;
    const std::vector<uint32_t> conn = grid(H, W);
    const int64_t E = (int64_t)conn.size() / 2;
    std::vector<int64_t> rank(N), tail(E), head(E);
    EXPECT(stereo_trws_analyze(N, E, conn.data(), rank.data(), tail.data(), head.data(), nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, why, sizeof(why)) == 0);
    for (int phase = 0; phase < 3; ++phase) {
      std::vector<int32_t> recv(E, -7);
      EXPECT(stereo_trws_state_receivers_host(N, E, conn.data(), 0, phase, recv.data(), why, sizeof(why)) == 0);
      for (int64_t e = 0; e < E; ++e) EXPECT(recv[e] == (phase == 0 ? tail[e] : head[e]));
      // node index order: the later endpoint is the larger id
      EXPECT(stereo_trws_state_receivers_host(N, E, conn.data(), STEREO_TRWS_ORDER_INDEX, phase, recv.data(), why, sizeof(why)) == 0);
      for (int64_t e = 0; e < E; ++e) {
        const uint32_t a = conn[2 * e], b = conn[2 * e + 1], lo = a < b ? a : b, hi = a < b ? b : a;
        EXPECT(recv[e] == (int32_t)(phase == 0 ? lo : hi));
      }
    }
    // refusals touch nothing
    std::vector<int32_t> recv(E, -7);
    EXPECT(stereo_trws_state_receivers_host(N, E, conn.data(), 0, 3, recv.data(), why, sizeof(why)) != 0 && std::strstr(why, "phase"));
    EXPECT(stereo_trws_state_receivers_host(N, E, conn.data(), 0, -1, recv.data(), why, 8) != 0 && std::strlen(why) <= 7);
    if (E > 0) {
      EXPECT(stereo_trws_state_receivers_host(N, E, nullptr, 0, 1, recv.data(), why, sizeof(why)) != 0 && std::strstr(why, "conn"));
      EXPECT(stereo_trws_state_receivers_host(N, E, conn.data(), 0, 1, nullptr, why, sizeof(why)) != 0 && std::strstr(why, "receiver"));
      EXPECT(stereo_trws_state_receivers_host(N - 1, E, conn.data(), 0, 1, recv.data(), nullptr, 0) != 0);
    }
    EXPECT(stereo_trws_state_receivers_host(-1, E, conn.data(), 0, 1, recv.data(), why, sizeof(why)) != 0);
    for (int64_t e = 0; e < E; ++e) EXPECT(recv[e] == -7);
  }

  // the argument checks, with vectors of exactly K entries
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<double> off_old = {-1.0, -0.25, 0.5}, off_new = {-0.5, 0.0, 0.125, 2.0}, M_old(5 * 3, 1.0), M_new(4 * 4, 0.0), shift(6, 0.0);
  std::vector<int32_t> src = {0, 1, -1, 4}, recv = {0, 5, 2, 3};
  int32_t bad = 0;
  stereo::carry::Args ok;
  ok.M_old = M_old.data(); ok.E_old = 5; ok.K_old = 3; ok.off_old = off_old.data(); ok.edge_src = src.data();
  ok.receiver_new = recv.data(); ok.N_new = 6; ok.shift = shift.data(); ok.stretch = 0.5; ok.gain = 2.0;
  ok.off_new = off_new.data(); ok.K_new = 4; ok.E_new = 4; ok.M_new = M_new.data(); ok.bad = &bad;
  EXPECT(stereo::carry::check_args("carry", ok, why, sizeof(why)) == 0);
  EXPECT(stereo::carry::check_args("carry", ok, nullptr, 0) == 0);
  stereo::carry::Args a;
  a = ok; a.M_old = nullptr; EXPECT(refused(a, "M_old"));
  a = ok; a.off_old = nullptr; EXPECT(refused(a, "off_old"));
  a = ok; a.off_new = nullptr; EXPECT(refused(a, "off_new"));
  a = ok; a.receiver_new = nullptr; EXPECT(refused(a, "receiver_new"));
  a = ok; a.shift = nullptr; EXPECT(refused(a, "shift"));
  a = ok; a.M_new = nullptr; EXPECT(refused(a, "M_new"));
  a = ok; a.K_old = 0; EXPECT(refused(a, "K_old"));
  a = ok; a.K_old = 4097; EXPECT(refused(a, "K_old"));
  a = ok; a.K_new = 0; EXPECT(refused(a, "K_new"));
  a = ok; a.K_new = 513; EXPECT(refused(a, "K_new"));
  a = ok; a.stretch = 0.0; EXPECT(refused(a, "stretch"));
  a = ok; a.stretch = nan; EXPECT(refused(a, "stretch"));
  a = ok; a.gain = -1.0; EXPECT(refused(a, "gain"));
  a = ok; a.gain = inf; EXPECT(refused(a, "gain"));
  a = ok; a.edge_src = nullptr; EXPECT(refused(a, "edge_src"));
  a = ok; a.edge_src = nullptr; a.E_old = 4; EXPECT(stereo::carry::check_args("carry", a, why, sizeof(why)) == 0);
  a = ok; a.M_new = M_old.data(); EXPECT(refused(a, "M_new"));
  a = ok; a.M_new = shift.data(); EXPECT(refused(a, "M_new"));
  a = ok; a.bad = recv.data(); EXPECT(refused(a, "bad"));
  a = ok; a.bad = M_new.data(); EXPECT(refused(a, "bad"));
  a = ok; a.device_form = true; EXPECT(refused(a, "d_off_old"));
  a = ok; a.device_form = true; a.d_off_old = off_old.data(); EXPECT(refused(a, "d_off_new"));
  a = ok; a.E_new = -1; EXPECT(refused(a, "E_new"));
  a = ok; a.E_old = (int64_t)1 << 31; EXPECT(refused(a, "E_old"));
  for (double v : {nan, inf, -1.0, -3.0, 0.5}) {
    std::vector<double> o = off_old;
    o[1] = v;
    a = ok; a.off_old = o.data();
    EXPECT(refused(a, "off_old"));
  }
  {
    std::vector<double> o = off_new;
    o[3] = o[2];
    a = ok; a.off_new = o.data();
    EXPECT(refused(a, "off_new"));
  }
  // short reason buffers
  a = ok; a.gain = 0.0;
  char small[6];
  EXPECT(stereo::carry::check_args("carry", a, small, sizeof(small)) != 0 && std::strlen(small) == 5);
  EXPECT(stereo::carry::check_args("carry", a, small, 1) != 0 && small[0] == 0);

  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("SANITIZE_CARRY_OK\n");
  return 0;
}
