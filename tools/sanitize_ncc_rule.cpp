// Development / CI tool (tests/test_ncc_exact_cpu.py): the host rule that picks the NCC volume kernel and its launch
// geometry (stereo_amd/csrc/ncc_rule.cpp, stereo_ncc_volume_rule) under AddressSanitizer + UndefinedBehaviorSanitizer,
// with disparity vectors of exactly D entries, at the boundaries of the rule: D around the 64-label chunk (a last chunk
// of one label among them), chunk spans around what the staged segment holds, widths and heights around the tiles,
// vectors with a fraction, a negative value, a value equal to W and a NaN.  What a lanes answer promises the kernel is
// asserted on every call: the staged segments hold the columns (cols + span + 5 <= 96, cols + 5 <= 36) and the column
// chunks cover the image.  Prints SANITIZE_NCC_RULE_OK.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/sanitize_ncc_rule.cpp stereo_amd/csrc/ncc_rule.cpp
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/stereo_hip.h"

static int failures = 0;
static long calls = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

// D integer disparities below W whose 64-label chunks span `span` at most, the LAST chunk exactly (so a last chunk of
// one label spans 0 and the one before it `span`)
static std::vector<double> spanning(int D, int span) {
  std::vector<double> d(D);
  for (int i = 0; i < D; ++i) d[i] = (i % 64) % (span + 1);
  const int last = (D - 1) / 64 * 64;
  if (D - last > 1) d[D - 1] = span;
  else if (last > 0) d[last - 1] = span;
  return d;
}

static int ask(int H, int W, const std::vector<double> &d, int layout, int cus, int naive, int rowlanes) {
  int path = -1, cols = -1, chunks = -1, span = -1;
  char why[64];
  ++calls;
  EXPECT(stereo_ncc_volume_rule(H, W, d.data(), (int)d.size(), 2, layout, cus, naive, rowlanes, &path, &cols, &chunks, &span,
                                why, sizeof(why)) == 0 && why[0] == 0);
  EXPECT(path >= 0 && path <= 2);
  if (path == 2) {
    EXPECT(layout == 1 && !naive && !rowlanes);
    EXPECT(cols >= 8 && cols + 5 <= 36 && cols + span + 5 <= 96);
    EXPECT(chunks >= 1 && (long)chunks * cols >= W && (long)(chunks - 1) * cols < W);
  } else {
    EXPECT(cols == 0 && chunks == 0 && span == 0);
  }
  if (naive) EXPECT(path == 0);
  return path;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int cus : {1, 8, 256, 1024})
    for (int H : {1, 11, 12, 13, 24, 25})
      for (int D : {1, 63, 64, 65, 128, 129})
        for (int span : {0, 81, 82, 83, 84, 85}) {
          if (D == 1 && span > 0) continue;
          const std::vector<double> d = spanning(D, span);
          const double largest = *std::max_element(d.begin(), d.end());
          for (int W : {span + 1, span + 2, 97, 200, 9 * cus - 5, 62 * cus + 7}) {
            for (int layout = 0; layout < 2; ++layout)
              for (int sw = 0; sw < 4; ++sw) {
                const int path = ask(H, W, d, layout, cus, sw & 1, sw >> 1);
                if (!(sw & 1)) EXPECT(path == (largest >= W ? 0 : layout == 1 && !(sw >> 1) && span <= 83 ? 2 : 1));
              }
          }
        }
  // not an integer in [0, W): the per-tap kernel, wherever the value stands
  for (int D : {1, 64, 65})
    for (int at : {0, D - 1})
      for (double v : {0.5, -1.0, 40.0, nan}) {
        std::vector<double> d = spanning(D, 0);
        d[at] = v;
        EXPECT(ask(13, 40, d, 1, 256, 0, 0) == 0);
        EXPECT(ask(13, 41, d, 1, 256, 0, 0) == (v == 40.0 ? 2 : 0));
      }
  // another patch size: per tap
  {
    const std::vector<double> d = spanning(3, 2);
    int path = -1;
    EXPECT(stereo_ncc_volume_rule(9, 12, d.data(), 3, 1, 1, 256, 0, 0, &path, nullptr, nullptr, nullptr, nullptr, 0) == 0 && path == 0);
    // refusals write nothing but the reason, in a buffer of any size
    char small[6];
    path = -7;
    EXPECT(stereo_ncc_volume_rule(9, 12, nullptr, 3, 2, 1, 256, 0, 0, &path, nullptr, nullptr, nullptr, small, sizeof(small)) != 0);
    EXPECT(path == -7 && std::strlen(small) == 5);
    EXPECT(stereo_ncc_volume_rule(0, 12, d.data(), 3, 2, 1, 256, 0, 0, &path, nullptr, nullptr, nullptr, small, 1) != 0 && small[0] == 0);
    EXPECT(stereo_ncc_volume_rule(9, 12, d.data(), 0, 2, 1, 256, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != 0);
    EXPECT(stereo_ncc_volume_rule(9, 12, d.data(), 3, 2, 2, 256, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != 0);
    EXPECT(stereo_ncc_volume_rule(9, 12, d.data(), 3, 2, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != 0);
  }
  if (failures) { std::printf("%d failures in %ld calls\n", failures, calls); return 1; }
  std::printf("SANITIZE_NCC_RULE_OK (%ld calls)\n", calls);
  return 0;
}
