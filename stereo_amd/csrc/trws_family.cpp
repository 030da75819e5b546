// The kernel-family rule of the TRW-S plans (trws_family.h) and its C entry for tests.
#include "trws_family.h"

#include <cstring>

#include "../../include/stereo_hip.h"

namespace stereo {

namespace {
const char *const kKRange = "stereo_trws: K must be in [1, 512] (up to 4096 with one strictly ascending positions vector shared by every edge)";
const char *const kStripGraph = "stereo_trws: row strips need a graph the pipelined kernels take (<= 8 edges per node, <= 4 dependencies in other runs, a chain schedule that provably terminates)";
const char *const kStripLabels = "stereo_trws: row strips need a graph and label count the pipelined kernels take "
                                 "(<= 8 edges per node; K <= 64, or K <= 128 with per-edge positions, or K <= 256 with shared ascending positions)";
const char *const kStripInputs = "stereo_trws: row strips with these inputs would need the generic kernel, which has no strip support "
                                 "(K > 128 or the MINPLUS mode need shared strictly ascending positions)";
constexpr unsigned bit(TrwsFamily f) { return 1u << (int)f; }
}  // namespace

unsigned trws_families_possible(const TrwsPlanFacts &f, const char **why) {
  if (f.K < 1 || f.K > kFamilyLargeMaxK) { *why = kKRange; return 0; }
  if (f.strips && !f.fast_ok) { *why = kStripGraph; return 0; }
  unsigned m = 0;
  if (f.fast_ok && f.fast_switch) {
    if (f.K <= kFamilyPipeMaxK && f.exact) m |= bit(TrwsFamily::Pipe);
    if (f.K > kFamilyPipeMaxK && f.K <= kFamilyPipe2MaxK && f.exact) m |= bit(TrwsFamily::Pipe2);
    // (kernel 1 in either message mode -- MINPLUS runs it lean --, kernel 2 with exact messages)
    if (f.K > kFamilyPipeMaxK && f.K <= kFamilyWideMaxK && (f.kernel == 1 || f.exact)) m |= bit(TrwsFamily::Wide);
  }
  if (f.strips) {
    // a strip walks the chain schedule with one of the descriptor-driven kernels
    if (!m) *why = kStripLabels;
    return m;
  }
  return f.K > kFamilyGenericMaxK ? bit(TrwsFamily::Large) : m | bit(TrwsFamily::Generic);
}

TrwsFamily trws_family(const TrwsPlanFacts &f, const TrwsInputFacts *in, const char **why) {
  const unsigned m = trws_families_possible(f, why);
  if (!m) return TrwsFamily::None;
  const bool ascending = in && in->shared && in->ascending;
  if (possible(m, TrwsFamily::Large)) {
    if (in && !ascending) { *why = kKRange; return TrwsFamily::None; }
    return TrwsFamily::Large;
  }
  if (possible(m, TrwsFamily::Wide) && ascending && in->lambda >= 0) return TrwsFamily::Wide;
  if (possible(m, TrwsFamily::Pipe2)) return TrwsFamily::Pipe2;
  if (possible(m, TrwsFamily::Pipe)) return TrwsFamily::Pipe;
  if (in && f.strips) { *why = kStripInputs; return TrwsFamily::None; }
  return TrwsFamily::Generic;
}

}  // namespace stereo

extern "C" int stereo_trws_family_rule(int kernel, int K, int message_mode, int fast_ok, int fast_switch, int strips,
                                       int positions, double lambda, char *err, size_t errcap) {
  using namespace stereo;
  TrwsPlanFacts f;
  f.kernel = kernel; f.K = K; f.exact = message_mode == STEREO_TRWS_MESSAGES_EXACT;
  f.fast_ok = fast_ok != 0; f.fast_switch = fast_switch != 0; f.strips = strips != 0;
  TrwsInputFacts in;
  in.shared = positions >= 1; in.ascending = positions == 2; in.lambda = lambda;
  const char *why = "";
  const TrwsFamily fam = trws_family(f, positions < 0 ? nullptr : &in, &why);
  if (err && errcap) {
    std::strncpy(err, fam == TrwsFamily::None ? why : "", errcap - 1);
    err[errcap - 1] = 0;
  }
  return (int)fam;
}
