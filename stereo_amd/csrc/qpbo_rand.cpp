// The permutation of QPBO::Improve (QPBO_extra.cpp:13-27), drawn from libc rand() like the
// reference's.  Note for callers that seed rand() to reproduce the reference: the HIP runtime draws
// from the same generator during its one-time initialisation (measured), so initialise it first
// (stereo_hip_warm_up; the Python package does so when it loads the library).
// `count` values of rand(), in order, from the process-wide generator -- the same values and the same generator
// state afterwards as `count` calls of rand(), without glibc's lock per call (2.7 ms of a 3.0 ms permutation at
// 450 x 375; an Improve move pays it on the host).  POSIX semantics only: initstate() parks the generator on a
// scratch array and hands back the array it was running on, position included; random_r() runs on that array
// through a random_data of our own; parking that one writes the advanced position back; setstate() resumes.
// The first use checks itself against rand() on a saved copy of the state (nothing is consumed by the check) and
// falls back to rand() for good if anything differs.  STEREO_HIP_FAST_RAND=0: always rand().
// Threads: the park / resume window swaps the PROCESS-WIDE generator state, so every window of this
// library is serialised by rand_window_mutex() (two host threads running Improve moves would otherwise
// hand each other's park buffers around and leave the generator on a static array for good).  A
// foreign thread that calls rand() inside a window draws from the parked stream (seeded 1) instead of
// the process stream -- the same hazard class as any unsynchronised rand() user, documented in
// INTEGRATION.md.
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/stereo_hip.h"
#include "qpbo_host.h"

namespace stereo {
namespace {

std::mutex &rand_window_mutex() {
  static std::mutex m;
  return m;
}

// (callers hold rand_window_mutex())
bool draw_rand_fast(int32_t *out, int64_t count) {
  alignas(int32_t) static char park[256];
  alignas(int32_t) static char park_r[256];
  alignas(int32_t) static char scratch[256];
  char *old = initstate(1u, park, sizeof(park));
  if (!old) return false;
  struct random_data rd;
  std::memset(&rd, 0, sizeof(rd));
  bool ok = initstate_r(1u, scratch, sizeof(scratch), &rd) == 0 && setstate_r(old, &rd) == 0;
  if (ok) {
    for (int64_t i = 0; i < count; ++i) { int32_t v; random_r(&rd, &v); out[i] = v; }
    ok = initstate_r(1u, park_r, sizeof(park_r), &rd) == 0;   // (parks rd: the position goes back into `old`)
  }
  setstate(old);
  return ok;
}

// (callers hold rand_window_mutex())
bool fast_rand_usable() {
  static std::atomic<int> state{-1};   // -1 unknown, 0 no, 1 yes
  if (state.load() >= 0) return state.load() == 1;
  state.store(0);
  if (const char *e = std::getenv("STEREO_HIP_FAST_RAND")) if (std::atoi(e) == 0) return false;
  // a copy of the generator's state while it is parked, to undo what the check draws
  alignas(int32_t) static char park[256];
  static const size_t bytes_of_type[5] = {8, 32, 64, 128, 256};   // TYPE_0 .. TYPE_4 arrays incl. the info word
  char *old = initstate(1u, park, sizeof(park));
  if (!old) return false;
  int32_t info;
  std::memcpy(&info, old, sizeof(info));
  const int type = (int)(((info % 5) + 5) % 5);
  const size_t bytes = bytes_of_type[type];
  char saved[256];
  std::memcpy(saved, old, bytes);
  setstate(old);
  int32_t slow[8], fast[8];
  for (int i = 0; i < 8; ++i) slow[i] = rand();
  const int32_t slow_next = rand();
  auto restore = [&]() -> bool {
    char *cur = initstate(1u, park, sizeof(park));
    if (cur != old) { if (cur) setstate(cur); return false; }
    std::memcpy(old, saved, bytes);
    setstate(old);
    return true;
  };
  if (!restore()) return false;
  const bool drew = draw_rand_fast(fast, 8);
  const int32_t fast_next = rand();
  if (!restore()) return false;
  if (drew && std::memcmp(slow, fast, sizeof(slow)) == 0 && slow_next == fast_next) state.store(1);
  return state.load() == 1;
}

}  // namespace

std::vector<int32_t> improve_permutation(int64_t N) {
  std::vector<int32_t> perm((size_t)N);
  for (int64_t i = 0; i < N; ++i) perm[i] = (int32_t)i;
  if (N < 2) return perm;
  std::vector<int32_t> r((size_t)(N - 1));
  {
    std::lock_guard<std::mutex> window(rand_window_mutex());   // one permutation's draws are contiguous in the stream
    if (!(fast_rand_usable() && draw_rand_fast(r.data(), N - 1)))
      for (int64_t i = 0; i < N - 1; ++i) r[i] = rand();   // (draw_rand_fast either drew everything or nothing)
  }
  for (int64_t i = 0; i < N - 1; ++i) {
    int64_t j = i + (int64_t)((r[i] / (1.0 + (double)RAND_MAX)) * (double)(N - i));
    if (j > N - 1) j = N - 1;
    std::swap(perm[i], perm[j]);
  }
  return perm;
}

}  // namespace stereo

extern "C" int stereo_hip_improve_permutation(int64_t N, int32_t *out) {
  if (N < 0 || (N > 0 && !out)) return 1;
  const std::vector<int32_t> perm = stereo::improve_permutation(N);
  if (N > 0) std::memcpy(out, perm.data(), sizeof(int32_t) * (size_t)N);
  return 0;
}
