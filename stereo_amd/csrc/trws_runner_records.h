// Host-made records of the speculative schedule's runner.  Everything a loader of the runner
// derives from the descriptors of a chain position and the one behind it, the position itself and the segment
// geometry is a function of the graph alone: it is worked out here, once per bound descriptor set, and a loader wave
// fetches the result with one per-lane load (trws_spec.h: run_loader).  Nothing of K, the weights or any uploaded data
// is in a record.  Plain C++, no HIP.
#pragma once
#include <cstdint>
#include <vector>

namespace stereo {

constexpr int kRecWords = 64;   // 32-bit words per chain position: one word per lane of a loader wave
// words 0-15: the staged words of the node as the message and label waves read them (trws_spec.h: kRsNt ...), with
//             word 2 = messages to compute when the two rows to the next node are twins (0: none goes there, else 1),
//             words 9-12 = -1 (label of an incoming row: the node in front) and word 15 = 0 (the tag is the loader's)
// words 16-23: edge whose weight goes to double j of the staged node (alpha of the two messages, 0 for gamma's place,
//             alpha of incoming rows 0-4); a lane of these loads its own weight
constexpr int kRecAlphaEdge = 16;
constexpr int kRecKfirst = 24;   // rows 0 .. kfirst - 1 of the node's list make the prefix sum
constexpr int kRecNout = 25;     // the node's own (outgoing) rows, loaded in front of the foreign flags
constexpr int kRecNdep = 26;     // foreign dependencies
constexpr int kRecRank = 27;     // the node's rank (for the give-up report of the wait)
constexpr int kRecFetch = 28;    // bit k: row k is loaded behind the flags
constexpr int kRecLabels = 29;   // bit k: ... and the label at its other end, which goes to staged word 9 + k - n_out
constexpr int kRecGamma = 30;    // 30, 31: the 64 bits of gamma = 1.0 / max(n_out, n_in, 1)
constexpr int kRecEdge = 32;     // 32-39: row / weight index of list slot k (the descriptor's words 4-11)
constexpr int kRecOther = 40;    // 40-47: label index of list slot k (the descriptor's words 32-39)
constexpr int kRecStage = 48;    // 48-50: list slot whose row goes to staged row S 0 / 1 / 2 (-1: none)
constexpr int kRecMsg = 51;      // 51, 52: list slot (0-3) whose row is the old row M 0 / 1 of the messages (-1: none)
constexpr int kRecTwin = 53;     // 0: one message at most; 1: two unless the weights agree; 2: ... and the old rows
constexpr int kRecS0 = 54;       // 54, 55: s0, s1 as the descriptors give them (slots in the outgoing list, -1: none)
constexpr int kRecDep = 56;      // 56-59: ranks of the foreign dependencies (the descriptor's words 20-23)
constexpr int kRecNin = 60;
// words 61-63: 0

// Records of the positions c0 .. c1 - 1 of one direction's bound descriptor array `desc` (TrwsGraph::kDescWords words
// per schedule position: the chain schedule's, or the sub-row schedule's), for segments of seg_len visits of which at
// most nseg exist.  out: (c1 - c0) * kRecWords words, position c0 first.
void build_runner_records(const int32_t *desc, int32_t c0, int32_t c1, int32_t seg_len, int32_t nseg, std::vector<int32_t> &out);

}  // namespace stereo
