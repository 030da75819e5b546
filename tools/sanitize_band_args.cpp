// Development tool: the argument checks of the band entries (stereo_amd/csrc/band.hip) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the host.  No device call is made: this program supplies
// stereo_hip_device_count() itself and answers 0, so a call whose arguments pass every check stops at "no HIP device".
// Arrays have exactly the sizes the entries take.  Prints SANITIZE_BAND_ARGS_OK.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Istereo_amd/csrc stereo_amd/csrc/band.hip \
//       tools/sanitize_band_args.cpp -o sanitize_band_args && ./sanitize_band_args
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../include/stereo_hip.h"

namespace stereo {
std::string &last_error() {
  static thread_local std::string s;
  return s;
}
}  // namespace stereo

extern "C" int stereo_hip_device_count(void) { return 0; }

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool says(const char *err, const char *what) { return std::strstr(err, what) != nullptr; }

int main() {
  const int H = 3, W = 4, D = 5, K = 3;
  const int64_t E = 2;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<double> ncc((size_t)H * W * D, 0.5), disp = {0, 1, 2, 3, 4}, base((size_t)H * W, 2.0), off = {-0.5, 0.0, 0.5};
  std::vector<uint32_t> conn = {0, 1, 1, 2};
  std::vector<double> unary((size_t)K * H * W), q((size_t)K * E), qp((size_t)K * E), refined((size_t)H * W);
  std::vector<int32_t> labels((size_t)H * W, 1);
  char err[256];
  auto inputs = [&](const double *o, int k) {
    err[0] = 0;
    return stereo_band_inputs(ncc.data(), H, W, D, 0, disp.data(), 1.0, base.data(), o, k, E, conn.data(), unary.data(), q.data(),
                              qp.data(), err, sizeof err);
  };
  auto apply = [&](const double *o, int k) {
    err[0] = 0;
    return stereo_band_apply(base.data(), H, W, labels.data(), o, k, refined.data(), err, sizeof err);
  };
  // a valid call passes every check and stops where the device would be looked for
  EXPECT(inputs(off.data(), K) != 0 && says(err, "no HIP device"));
  EXPECT(apply(off.data(), K) != 0 && says(err, "no HIP device"));
  // offsets: read to exactly K entries, never beyond
  for (int k : {1, 2, 512}) {
    std::vector<double> o((size_t)k);
    for (int i = 0; i < k; ++i) o[(size_t)i] = (double)i;                  // 0, 1, ..., k - 1: valid
    std::vector<double> u((size_t)k * H * W), a((size_t)k * E), b((size_t)k * E);
    err[0] = 0;
    EXPECT(stereo_band_inputs(ncc.data(), H, W, D, 1, disp.data(), 1.0, base.data(), o.data(), k, E, conn.data(), u.data(), a.data(),
                              b.data(), err, sizeof err) != 0 && says(err, "no HIP device"));
  }
  {
    std::vector<double> o(513);
    for (size_t i = 0; i < o.size(); ++i) o[i] = (double)i;
    EXPECT(inputs(o.data(), 513) != 0 && says(err, "1 .. 512"));
    EXPECT(inputs(o.data(), 0) != 0 && says(err, "1 .. 512"));
    EXPECT(apply(o.data(), -3) != 0 && says(err, "1 .. 512"));
  }
  { const double o[3] = {-1.0, nan, 0.0};  EXPECT(inputs(o, 3) != 0 && says(err, "not finite")); }
  { const double o[2] = {0.0, inf};        EXPECT(apply(o, 2) != 0 && says(err, "not finite")); }
  { const double o[3] = {0.0, 1.0, 1.0};   EXPECT(inputs(o, 3) != 0 && says(err, "strictly ascending")); }
  { const double o[2] = {1.0, 0.0};        EXPECT(apply(o, 2) != 0 && says(err, "strictly ascending")); }
  { const double o[2] = {0.25, 0.5};       EXPECT(inputs(o, 2) != 0 && says(err, "contain 0.0")); }
  EXPECT(inputs(nullptr, K) != 0 && says(err, "NULL"));
  // sizes, layout, NULL arrays
  err[0] = 0;
  EXPECT(stereo_band_inputs(ncc.data(), 0, W, D, 0, disp.data(), 1.0, base.data(), off.data(), K, E, conn.data(), unary.data(), q.data(),
                            qp.data(), err, sizeof err) != 0 && says(err, "H and W"));
  EXPECT(stereo_band_inputs(ncc.data(), 1 << 16, 1 << 15, D, 0, disp.data(), 1.0, base.data(), off.data(), K, E, conn.data(), unary.data(),
                            q.data(), qp.data(), err, sizeof err) != 0 && says(err, "2^31"));
  EXPECT(stereo_band_inputs(ncc.data(), H, W, 0, 0, disp.data(), 1.0, base.data(), off.data(), K, E, conn.data(), unary.data(), q.data(),
                            qp.data(), err, sizeof err) != 0 && says(err, "D must"));
  EXPECT(stereo_band_inputs(ncc.data(), H, W, D, 2, disp.data(), 1.0, base.data(), off.data(), K, E, conn.data(), unary.data(), q.data(),
                            qp.data(), err, sizeof err) != 0 && says(err, "layout"));
  EXPECT(stereo_band_inputs(ncc.data(), H, W, D, 0, disp.data(), 1.0, base.data(), off.data(), K, E, nullptr, unary.data(), q.data(),
                            qp.data(), err, sizeof err) != 0 && says(err, "NULL"));
  EXPECT(stereo_band_inputs(ncc.data(), H, W, D, 0, disp.data(), 1.0, base.data(), off.data(), K, 0, nullptr, unary.data(), nullptr,
                            nullptr, err, sizeof err) != 0 && says(err, "no HIP device"));       // E = 0 needs no edge arrays
  EXPECT(stereo_band_inputs_device(ncc.data(), H, W, D, 0, disp.data(), nullptr, 1.0, base.data(), off.data(), off.data(), K, E,
                                   conn.data(), unary.data(), q.data(), qp.data(), nullptr, nullptr, err, sizeof err) != 0 &&
         says(err, "d_disparities"));
  EXPECT(stereo_band_apply_device(base.data(), H, W, labels.data(), off.data(), nullptr, K, refined.data(), nullptr, nullptr, err,
                                  sizeof err) != 0 && says(err, "d_offsets"));
  // the host entries scan base, conn and labels to exactly their ends
  base[(size_t)H * W - 1] = nan;
  EXPECT(inputs(off.data(), K) != 0 && says(err, "row 2, column 3"));
  EXPECT(apply(off.data(), K) != 0 && says(err, "row 2, column 3"));
  base[(size_t)H * W - 1] = 2.0;
  conn[3] = (uint32_t)(H * W);
  EXPECT(inputs(off.data(), K) != 0 && says(err, "edge 1"));
  conn[3] = 2;
  labels[(size_t)H * W - 1] = K + 1;
  EXPECT(apply(off.data(), K) != 0 && says(err, "outside 1 .. 3"));
  labels[(size_t)H * W - 1] = 0;
  EXPECT(apply(off.data(), K) != 0 && says(err, "outside 1 .. 3"));
  // a short error buffer is filled, terminated and not overrun
  char tiny[8];
  std::memset(tiny, 'x', sizeof tiny);
  EXPECT(stereo_band_apply(base.data(), H, W, labels.data(), off.data(), K, refined.data(), tiny, sizeof tiny) != 0 && tiny[7] == 0);
  EXPECT(stereo_band_apply(base.data(), H, W, labels.data(), off.data(), K, refined.data(), nullptr, 0) != 0);
  EXPECT(stereo_band_max_offsets() == 512);
  if (failures) return 1;
  std::printf("SANITIZE_BAND_ARGS_OK\n");
  return 0;
}
