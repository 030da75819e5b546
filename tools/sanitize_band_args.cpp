// Development tool: the argument checks and scans of the four level builders (stereo_amd/csrc/band.hip, plane_band.hip,
// candidates.hip, plane_candidates.hip; the shared ones live in band_common.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the host.  No device call is made: this program supplies
// stereo_hip_device_count() itself and answers 0, so a call whose arguments pass every check stops at "no HIP device".
// Arrays have exactly the sizes the entries take.  Prints SANITIZE_BAND_ARGS_OK.
//   cd stereo_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -I../../include -I. \
//       band.hip plane_band.hip candidates.hip plane_candidates.hip ../../tools/sanitize_band_args.cpp \
//       -o sanitize_band_args && ./sanitize_band_args
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

// ---------------------------------------------------------------- candidates, plane bands, plane candidates
// One image, 3 x 4, for all of them; a call is made by a lambda that takes what the case varies.

static void check_candidates() {
  const int H = 3, W = 4, D = 5, N = H * W;
  const int64_t E = 2;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> ncc((size_t)N * D, 0.5), disp = {0, 1, 2, 3, 4}, base((size_t)N, 2.0);
  std::vector<uint32_t> conn = {0, 1, 1, 2};
  char err[256];
  // gather: Ko offsets 0 .. Ko - 1, M sources, T taps, every tap (tap, -tap); the table holds exactly (Ko + M T) N
  auto gather = [&](int Ko, int M, int T, int32_t tap, bool null_sources, double last_source) {
    std::vector<double> off((size_t)Ko), src((size_t)M * N, 1.0), cand((size_t)(Ko + M * T) * N);
    for (int i = 0; i < Ko; ++i) off[(size_t)i] = (double)i;
    std::vector<int32_t> taps((size_t)2 * T);
    for (int t = 0; t < T; ++t) { taps[(size_t)2 * t] = tap; taps[(size_t)2 * t + 1] = -tap; }
    if (!src.empty()) src.back() = last_source;
    err[0] = 0;
    return stereo_candidates_gather(base.data(), H, W, off.data(), Ko, null_sources ? nullptr : src.data(), M,
                                    null_sources ? nullptr : taps.data(), T, cand.data(), err, sizeof err);
  };
  EXPECT(gather(3, 2, 2, (1 << 15) - 1, false, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(3, 2, 2, 1 << 15, false, 1.0) != 0 && says(err, "tap 0 has |dy| or |dx| of 2^15 or more"));
  EXPECT(gather(3, 0, 2, 0, true, 1.0) != 0 && says(err, "no HIP device"));          // M * T == 0: no sources, no taps
  EXPECT(gather(3, 2, 0, 0, true, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(3, 1, 1, 0, true, 1.0) != 0 && says(err, "sources and taps must not be NULL"));
  EXPECT(gather(511, 1, 1, 0, false, 1.0) != 0 && says(err, "no HIP device"));        // K = 512
  EXPECT(gather(512, 1, 1, 0, false, 1.0) != 0 && says(err, "K = Ko + M * T must be 1 .. 512 (got 513)"));
  EXPECT(gather(3, 2, 2, 1, false, nan) != 0 && says(err, "source 1 is not finite at pixel (row 2, column 3)"));
  // inputs and apply: the table, conn and the labels are scanned to exactly their ends
  const int K = 3;
  std::vector<double> cand((size_t)K * N, 1.5), unary((size_t)K * N), q((size_t)K * E), qp((size_t)K * E), out((size_t)N);
  std::vector<int32_t> labels((size_t)N, 1);
  auto inputs = [&] {
    err[0] = 0;
    return stereo_candidates_inputs(ncc.data(), H, W, D, 0, disp.data(), 1.0, cand.data(), K, E, conn.data(), unary.data(), q.data(),
                                    qp.data(), err, sizeof err);
  };
  auto apply = [&] {
    err[0] = 0;
    return stereo_candidates_apply(cand.data(), H, W, K, labels.data(), out.data(), err, sizeof err);
  };
  EXPECT(inputs() != 0 && says(err, "no HIP device"));
  EXPECT(apply() != 0 && says(err, "no HIP device"));
  cand.back() = nan;
  EXPECT(inputs() != 0 && says(err, "cand is not finite at pixel (row 2, column 3), label 3"));
  EXPECT(apply() != 0 && says(err, "cand is not finite at pixel (row 2, column 3), label 3"));
  cand.back() = 1.5;
  conn[3] = (uint32_t)N;
  EXPECT(inputs() != 0 && says(err, "edge 1"));
  conn[3] = 2;
  labels.back() = K + 1;
  EXPECT(apply() != 0 && says(err, "label 4 at pixel 11 is outside 1 .. 3"));
  err[0] = 0;
  EXPECT(stereo_candidates_inputs(ncc.data(), H, W, D, 0, disp.data(), 1.0, cand.data(), 513, E, conn.data(), unary.data(), q.data(),
                                  qp.data(), err, sizeof err) != 0 && says(err, "K must be 1 .. 512 (got 513)"));
}

static void check_planes() {
  const int H = 3, W = 4, D = 5, C = 2, N = H * W, K = 3;
  const int64_t E = 2;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> ncc((size_t)N * D, 0.5), disp = {0, 1, 2, 3, 4}, im0((size_t)N * C, 0.25), im1((size_t)N * C, 0.5);
  std::vector<double> P2 = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, off = {-0.5, 0.0, 0.5};
  std::vector<uint32_t> conn = {0, 1, 1, 2};
  std::vector<double> unary((size_t)K * N), q((size_t)K * E), qp((size_t)K * E), out4((size_t)4 * N);
  std::vector<int32_t> labels((size_t)N, 1);
  char err[256];
  auto plane_array = [](size_t count) {
    std::vector<double> p(4 * count, 0.0);
    for (size_t i = 0; i < count; ++i) { p[4 * i + 2] = 1.0; p[4 * i + 3] = -2.0; }
    return p;
  };
  // the plane band: planes, conn and the labels are scanned to exactly their ends
  std::vector<double> planes = plane_array((size_t)N);
  auto band_ncc = [&] {
    err[0] = 0;
    return stereo_plane_band_inputs_ncc(ncc.data(), H, W, D, 0, disp.data(), 1.0, planes.data(), off.data(), K, E, conn.data(),
                                        unary.data(), q.data(), qp.data(), err, sizeof err);
  };
  auto band_gs = [&](double d_step) {
    err[0] = 0;
    return stereo_plane_band_inputs_globalstereo(im0.data(), im1.data(), H, W, C, P2.data(), 0.0, d_step, 30.0, planes.data(),
                                                 off.data(), K, E, conn.data(), unary.data(), q.data(), qp.data(), err, sizeof err);
  };
  auto band_apply = [&] {
    err[0] = 0;
    return stereo_plane_band_apply(planes.data(), N, labels.data(), off.data(), K, out4.data(), err, sizeof err);
  };
  EXPECT(band_ncc() != 0 && says(err, "no HIP device"));
  EXPECT(band_gs(1.0) != 0 && says(err, "no HIP device"));
  EXPECT(band_gs(0.0) != 0 && says(err, "d_step must not be 0"));
  EXPECT(band_apply() != 0 && says(err, "no HIP device"));
  planes.back() = inf;
  EXPECT(band_ncc() != 0 && says(err, "a plane is not finite at pixel (row 2, column 3)"));
  EXPECT(band_apply() != 0 && says(err, "a plane is not finite at pixel 11"));
  planes.back() = -2.0;
  planes[planes.size() - 2] = 0.0;
  EXPECT(band_gs(1.0) != 0 && says(err, "Infinite disparity (c == 0) at pixel (row 2, column 3)"));
  planes[planes.size() - 2] = 1.0;
  conn[3] = (uint32_t)N;
  EXPECT(band_ncc() != 0 && says(err, "edge 1"));
  EXPECT(band_gs(1.0) != 0 && says(err, "edge 1"));
  conn[3] = 2;
  labels.back() = 0;
  EXPECT(band_apply() != 0 && says(err, "label 0 at pixel 11 is outside 1 .. 3"));
  labels.back() = 1;
  // plane candidates, gather: the table holds exactly 4 (Ko + M T) N
  auto gather = [&](int Ko, int M, int T, int32_t tap, bool null_sources, double last_c) {
    std::vector<double> o((size_t)Ko), src = plane_array((size_t)M * N), pcand((size_t)4 * (Ko + M * T) * N);
    for (int i = 0; i < Ko; ++i) o[(size_t)i] = (double)i;
    std::vector<int32_t> taps((size_t)2 * T);
    for (int t = 0; t < T; ++t) { taps[(size_t)2 * t] = -tap; taps[(size_t)2 * t + 1] = tap; }
    if (!src.empty()) src[src.size() - 2] = last_c;
    err[0] = 0;
    return stereo_plane_candidates_gather(planes.data(), H, W, o.data(), Ko, null_sources ? nullptr : src.data(), M,
                                          null_sources ? nullptr : taps.data(), T, pcand.data(), err, sizeof err);
  };
  EXPECT(gather(3, 2, 2, (1 << 15) - 1, false, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(3, 2, 2, 1 << 15, false, 1.0) != 0 && says(err, "tap 0 has |dy| or |dx| of 2^15 or more"));
  EXPECT(gather(3, 0, 2, 0, true, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(3, 2, 0, 0, true, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(3, 1, 1, 0, true, 1.0) != 0 && says(err, "sources and taps must not be NULL"));
  EXPECT(gather(511, 1, 1, 0, false, 1.0) != 0 && says(err, "no HIP device"));
  EXPECT(gather(512, 1, 1, 0, false, 1.0) != 0 && says(err, "K = Ko + M * T must be 1 .. 512 (got 513)"));
  EXPECT(gather(3, 2, 2, 1, false, 0.0) != 0 && says(err, "Infinite disparity (c == 0) in source 1 at pixel (row 2, column 3)"));
  EXPECT(gather(3, 2, 2, 1, false, inf) != 0 && says(err, "source 1 is not finite at pixel (row 2, column 3)"));
  // plane candidates, inputs and apply: the table, conn and the labels are scanned to exactly their ends
  std::vector<double> pcand = plane_array((size_t)K * N);
  auto cand_ncc = [&] {
    err[0] = 0;
    return stereo_plane_candidates_inputs_ncc(ncc.data(), H, W, D, 1, disp.data(), 1.0, pcand.data(), K, E, conn.data(), unary.data(),
                                              q.data(), qp.data(), err, sizeof err);
  };
  auto cand_gs = [&] {
    err[0] = 0;
    return stereo_plane_candidates_inputs_globalstereo(im0.data(), im1.data(), H, W, C, P2.data(), 0.0, 1.0, 30.0, pcand.data(), K, E,
                                                       conn.data(), unary.data(), q.data(), qp.data(), err, sizeof err);
  };
  auto cand_apply = [&] {
    err[0] = 0;
    return stereo_plane_candidates_apply(pcand.data(), H, W, K, labels.data(), out4.data(), err, sizeof err);
  };
  EXPECT(cand_ncc() != 0 && says(err, "no HIP device"));
  EXPECT(cand_gs() != 0 && says(err, "no HIP device"));
  EXPECT(cand_apply() != 0 && says(err, "no HIP device"));
  pcand.back() = inf;
  EXPECT(cand_ncc() != 0 && says(err, "pcand is not finite at pixel (row 2, column 3), label 3"));
  EXPECT(cand_apply() != 0 && says(err, "pcand is not finite at pixel (row 2, column 3), label 3"));
  pcand.back() = -2.0;
  pcand[pcand.size() - 2] = 0.0;
  EXPECT(cand_gs() != 0 && says(err, "Infinite disparity (c == 0) in pcand at pixel (row 2, column 3), label 3"));
  pcand[pcand.size() - 2] = 1.0;
  conn[3] = (uint32_t)N;
  EXPECT(cand_ncc() != 0 && says(err, "edge 1"));
  EXPECT(cand_gs() != 0 && says(err, "edge 1"));
  conn[3] = 2;
  labels.back() = K + 1;
  EXPECT(cand_apply() != 0 && says(err, "label 4 at pixel 11 is outside 1 .. 3"));
  labels.back() = 1;
  // the device forms refuse a plane array that is not 16-byte aligned (the window of a buffer one double longer)
  auto misaligned = [](std::vector<double> &buf) { return ((uintptr_t)buf.data() & 15) != 0 ? buf.data() : buf.data() + 1; };
  std::vector<double> planes1 = plane_array((size_t)N + 1), pcand1 = plane_array((size_t)K * N + 1), out1((size_t)4 * N + 1);
  std::vector<double> src = plane_array((size_t)N), src1 = plane_array((size_t)N + 1), table((size_t)4 * 4 * N), table1((size_t)4 * 4 * N + 1);
  std::vector<int32_t> taps = {0, 1};
  auto gather_device = [&](const double *own, const double *sources, double *to) {
    err[0] = 0;
    return stereo_plane_candidates_gather_device(own, H, W, off.data(), off.data(), K, sources, 1, taps.data(), taps.data(), 1, to,
                                                 nullptr, nullptr, err, sizeof err);
  };
  EXPECT(gather_device(planes.data(), src.data(), table.data()) != 0 && says(err, "no HIP device"));
  EXPECT(gather_device(misaligned(planes1), src.data(), table.data()) != 0 && says(err, "planes must be 16-byte aligned"));
  EXPECT(gather_device(planes.data(), misaligned(src1), table.data()) != 0 && says(err, "sources must be 16-byte aligned"));
  EXPECT(gather_device(planes.data(), src.data(), misaligned(table1)) != 0 && says(err, "pcand must be 16-byte aligned"));
  err[0] = 0;
  EXPECT(stereo_plane_candidates_inputs_ncc_device(ncc.data(), H, W, D, 0, disp.data(), disp.data(), 1.0, misaligned(pcand1), K, E,
                                                   conn.data(), unary.data(), q.data(), qp.data(), nullptr, nullptr, err, sizeof err) != 0 &&
         says(err, "pcand must be 16-byte aligned"));
  EXPECT(stereo_plane_candidates_inputs_globalstereo_device(im0.data(), im1.data(), H, W, C, P2.data(), 0.0, 1.0, 30.0, misaligned(pcand1),
                                                            K, E, conn.data(), unary.data(), q.data(), qp.data(), nullptr, nullptr, err,
                                                            sizeof err) != 0 && says(err, "pcand must be 16-byte aligned"));
  EXPECT(stereo_plane_candidates_apply_device(misaligned(pcand1), H, W, K, labels.data(), out4.data(), nullptr, nullptr, err,
                                              sizeof err) != 0 && says(err, "pcand must be 16-byte aligned"));
  EXPECT(stereo_plane_candidates_apply_device(pcand.data(), H, W, K, labels.data(), misaligned(out1), nullptr, nullptr, err,
                                              sizeof err) != 0 && says(err, "out must be 16-byte aligned"));
  EXPECT(stereo_plane_candidates_apply_device(pcand.data(), H, W, K, labels.data(), out4.data(), nullptr, nullptr, err,
                                              sizeof err) != 0 && says(err, "no HIP device"));
}

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
  check_candidates();
  check_planes();
  if (failures) return 1;
  std::printf("SANITIZE_BAND_ARGS_OK\n");
  return 0;
}
