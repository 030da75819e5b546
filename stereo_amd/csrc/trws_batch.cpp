// Admission rule and launch partition of the TRW-S batches (trws_batch.h).
#include "trws_batch.h"

#include <algorithm>
#include <cstdint>

namespace stereo {

namespace {
const char *family_name(TrwsFamily f) {
  switch (f) {
    case TrwsFamily::Generic: return "generic";
    case TrwsFamily::Pipe: return "K <= 64";
    case TrwsFamily::Wide: return "wide";
    case TrwsFamily::Pipe2: return "K <= 128";
    case TrwsFamily::Large: return "large";
    default: return "no";
  }
}
int refuse(int i, const std::string &what, std::string *why) {
  if (why) *why = "member " + std::to_string(i) + " " + what;
  return i;
}
}  // namespace

int trws_batch_admit(const TrwsBatchMember *m, int n, std::string *why) {
  if (!m || n < 1) {
    if (why) *why = "a batch needs 1 .. " + std::to_string(kBatchMaxMembers) + " plans";
    return 0;
  }
  if (n > kBatchMaxMembers)
    return refuse(kBatchMaxMembers, "does not fit: a batch holds at most " + std::to_string(kBatchMaxMembers) + " plans", why);
  for (int i = 0; i < n; ++i) {
    const TrwsBatchMember &a = m[i], &a0 = m[0];
    if (!a.present) return refuse(i, "is a NULL plan", why);
    if (a.repeated) return refuse(i, "is in the batch already (a plan can be a member once)", why);
    if (a.nstrips != 1) return refuse(i, "is a row strip (strips iterate through stereo_trws_plans_issue)", why);
    if (!a.have_inputs) return refuse(i, "has no inputs uploaded/bound", why);
    if (!pipelined(a.family))
      return refuse(i, std::string("runs the ") + family_name(a.family) + " kernel family: batches run on the pipelined kernels only "
                    "(K <= 64; K <= 128 with per-edge positions; K <= 256 with shared ascending positions)", why);
    if (a.device != a0.device)
      return refuse(i, "lives on device " + std::to_string(a.device) + ", member 0 on device " + std::to_string(a0.device) +
                    " (a batch runs on one device)", why);
    if (a.family != a0.family || a.kernel != a0.kernel || a.exact != a0.exact || a.shared != a0.shared) {
      const char *what = a.family != a0.family ? "kernel family" : a.kernel != a0.kernel ? "smoothness kernel"
                         : a.exact != a0.exact ? "message mode" : "kind of positions (shared or per edge)";
      return refuse(i, std::string("differs from member 0 in its ") + what + ": mixed instantiations (one launch runs one sweep kernel)", why);
    }
  }
  return -1;
}

int trws_batch_partition(const int *blocks, int n, int capacity, bool floating, int *first) {
  capacity = std::max(capacity, 1);
  first[0] = 0;
  if (!floating) {
    int take = 0;
    while (take < n && (take == 0 || first[take] + std::max(blocks[take], 1) <= capacity)) {
      first[take + 1] = first[take] + std::max(blocks[take], 1);
      ++take;
    }
    return take;
  }
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) sum += std::max(blocks[i], 1);
  for (int i = 0; i < n; ++i) {
    int64_t share = std::max(blocks[i], 1);
    if (sum > capacity) share = std::max<int64_t>(1, share * capacity / sum);
    first[i + 1] = first[i] + (int)share;
  }
  return n;
}

}  // namespace stereo
