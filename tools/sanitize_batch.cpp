// Development tool (tests/test_trws_batch_cpu.py): the host-only part of the TRW-S batches -- the admission rule and
// the launch partition of stereo_amd/csrc/trws_batch.cpp -- built with -fsanitize=address,undefined and walked over
// every refusal, the member limit and a sweep of partitions.  Prints SANITIZE_BATCH_OK.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../stereo_amd/csrc/trws_batch.h"

using namespace stereo;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static TrwsBatchMember good() {
  TrwsBatchMember m;
  m.present = true; m.have_inputs = true; m.family = TrwsFamily::Pipe;
  return m;
}

int main() {
  std::string why;
  {
    std::vector<TrwsBatchMember> v(3, good());
    EXPECT(trws_batch_admit(v.data(), 3, &why) == -1);
    EXPECT(trws_batch_admit(v.data(), 0, &why) == 0 && why.find("1 .. 16") != std::string::npos);
    EXPECT(trws_batch_admit(nullptr, 2, &why) == 0);
    EXPECT(trws_batch_admit(v.data(), 3, nullptr) == -1);
  }
  {
    std::vector<TrwsBatchMember> v(kBatchMaxMembers, good());   // exactly the limit: nothing behind it is read
    EXPECT(trws_batch_admit(v.data(), kBatchMaxMembers, &why) == -1);
    EXPECT(trws_batch_admit(v.data(), kBatchMaxMembers + 1, &why) == kBatchMaxMembers && why.find("member 16") == 0);
  }
  struct Case { void (*spoil)(TrwsBatchMember &); const char *text; };
  const Case cases[] = {
      {[](TrwsBatchMember &m) { m.present = false; }, "NULL plan"},
      {[](TrwsBatchMember &m) { m.repeated = true; }, "already"},
      {[](TrwsBatchMember &m) { m.nstrips = 2; }, "row strip"},
      {[](TrwsBatchMember &m) { m.have_inputs = false; }, "no inputs"},
      {[](TrwsBatchMember &m) { m.family = TrwsFamily::Generic; }, "generic kernel family"},
      {[](TrwsBatchMember &m) { m.family = TrwsFamily::Large; }, "large kernel family"},
      {[](TrwsBatchMember &m) { m.family = TrwsFamily::None; }, "kernel family"},
      {[](TrwsBatchMember &m) { m.device = 3; }, "device 3"},
      {[](TrwsBatchMember &m) { m.family = TrwsFamily::Wide; }, "mixed instantiations"},
      {[](TrwsBatchMember &m) { m.kernel = 2; }, "smoothness kernel"},
      {[](TrwsBatchMember &m) { m.exact = false; }, "message mode"},
      {[](TrwsBatchMember &m) { m.shared = true; }, "kind of positions"},
  };
  for (const Case &c : cases)
    for (int at = 1; at < 4; ++at) {   // (member 0 is the one the others are compared with)
      std::vector<TrwsBatchMember> v(4, good());
      c.spoil(v[at]);
      const int bad = trws_batch_admit(v.data(), 4, &why);
      EXPECT(bad == at);
      EXPECT(why.find("member " + std::to_string(at) + " ") == 0 && why.find(c.text) != std::string::npos);
    }
  // partitions: shares start at 0, never shrink below one, the static form takes a prefix that fits
  for (int n = 1; n <= kBatchMaxMembers; ++n)
    for (int capacity : {1, 7, 256, 512, 100000})
      for (int scale : {0, 1, 37, 450, 5000}) {
        std::vector<int> blocks(n), first(n + 1, -1);
        int64_t sum = 0;
        for (int i = 0; i < n; ++i) { blocks[i] = scale * (1 + i % 3); sum += blocks[i] > 1 ? blocks[i] : 1; }
        EXPECT(trws_batch_partition(blocks.data(), n, capacity, true, first.data()) == n);
        EXPECT(first[0] == 0);
        for (int i = 0; i < n; ++i) EXPECT(first[i + 1] > first[i]);
        if (sum <= capacity) EXPECT(first[n] == sum);
        else EXPECT(first[n] <= capacity + n);
        std::vector<int> sfirst(n + 1, -1);
        const int take = trws_batch_partition(blocks.data(), n, capacity, false, sfirst.data());
        EXPECT(take >= 1 && take <= n && sfirst[0] == 0);
        for (int i = 0; i < take; ++i) EXPECT(sfirst[i + 1] - sfirst[i] == (blocks[i] > 1 ? blocks[i] : 1));
        EXPECT(take == 1 || sfirst[take] <= capacity);
        if (take < n) EXPECT(sfirst[take] + (blocks[take] > 1 ? blocks[take] : 1) > capacity);
      }
  if (failures) return 1;
  std::printf("SANITIZE_BATCH_OK\n");
  return 0;
}
