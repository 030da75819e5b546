// Batches of independent TRW-S plans (stereo_trws_batch_*): which plans may share the launches of a
// sweep, and how the workgroups of one launch are divided among them (host only, no HIP).
//
// A batch is a group launch (GroupArgs, trws_dev.h) of whole problems instead of strips: every member is an ordinary
// plan that keeps its own inputs, messages, labels, bound, energy and iteration count, and computes bit for bit what
// it computes alone.  The group kernels are instantiated on the smoothness kernel, the message mode and the kind of
// positions, and one launch runs one kernel: the members of a batch agree on those and on the kernel family.
#pragma once

#include <string>

#include "trws_family.h"

namespace stereo {

constexpr int kBatchMaxMembers = 16;   // what GroupArgs holds (kMaxGroup, trws_dev.h)
// K <= 64 members that each have more runs than the device keeps workgroups resident share a launch from this many
// on; below, they take their own launches in turn (measured on 450 x 375 x 60: 0.74 x at 2, 0.98 x at 4, 1.15 x at 8)
constexpr int kBatchLargeMin = 8;

// what stereo_trws_batch_create (and every stereo_trws_batch_iterate: an upload may have changed it) looks at
struct TrwsBatchMember {
  bool present = false;      // not a NULL pointer
  bool repeated = false;     // the same plan as an earlier member
  int nstrips = 1;
  bool have_inputs = false;
  TrwsFamily family = TrwsFamily::None;
  int kernel = 1;
  bool exact = true;         // message mode
  bool shared = false;       // one shared positions vector instead of q / qprim per edge
  int device = 0;
};

// -1: the batch is accepted.  Otherwise the index of the first member that cannot be in it (0 where n itself is out of
// range, kBatchMaxMembers where there are too many) and the refusal, which names that member, in *why.
int trws_batch_admit(const TrwsBatchMember *m, int n, std::string *why);

// The workgroups of ONE sweep launch: member i's are first[i] .. first[i + 1] - 1 (its share: where they start; the
// floating kernel lets them move on afterwards).  blocks[i]: what member i launches alone; capacity: workgroups that
// stay resident together.  Returns how many of the n members this launch takes, at least one:
//   floating (trws_pipe_batch_kernel)   all of them; shares shrink in proportion, to one at least, when the sum
//                                       exceeds the capacity (a workgroup that runs out of tickets serves the others)
//   static (the group kernels)          the longest prefix whose sum fits, the rest goes into the next launch
int trws_batch_partition(const int *blocks, int n, int capacity, bool floating, int *first);

}  // namespace stereo
