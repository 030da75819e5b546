// Which sweep kernel family runs a TRW-S plan: the one place that decides it (host only, no HIP).
//
// Precedence Large > Wide > Pipe2 > Pipe > Generic (DESIGN.md 4.8 has the rule as a table):
//   Large    512 < K <= 4096; needs one shared positions vector, finite and strictly ascending
//   Wide     64 < K <= 256, linear kernel in either message mode or quadratic with exact messages;
//            needs the same of the positions and lambda >= 0
//   Pipe2    64 < K <= 128, exact messages, any positions
//   Pipe     K <= 64, exact messages, any positions
//   Generic  everything else up to 512 labels; no row strips
// Wide, Pipe2 and Pipe are the pipelined families: they need a graph the descriptors can express
// (TrwsGraph::fast_ok) and STEREO_HIP_TRWS_FAST not 0.
#pragma once

namespace stereo {

// the values ARE what stereo_trws_plan_path returns
enum class TrwsFamily : int { None = 0, Generic = 1, Pipe = 2, Wide = 3, Pipe2 = 4, Large = 5 };

constexpr int kFamilyPipeMaxK = 64, kFamilyPipe2MaxK = 128, kFamilyWideMaxK = 256, kFamilyGenericMaxK = 512,
              kFamilyLargeMaxK = 4096;

// The descriptor-driven families: they walk the chain schedule (trws_graph.h), take row strips and have a group launch.
constexpr bool pipelined(TrwsFamily f) { return f == TrwsFamily::Pipe || f == TrwsFamily::Pipe2 || f == TrwsFamily::Wide; }

// what is known when a plan is created
struct TrwsPlanFacts {
  int kernel = 1;          // smoothness kernel: 1 linear, 2 quadratic
  int K = 0;
  bool exact = true;       // STEREO_TRWS_MESSAGES_EXACT (false: the MINPLUS mode)
  bool fast_ok = false;    // TrwsGraph::fast_ok
  bool fast_switch = true; // STEREO_HIP_TRWS_FAST is not 0
  bool strips = false;     // the plan is a row strip
};

// what an upload or bind adds
struct TrwsInputFacts {
  bool shared = false;     // one positions vector instead of q / qprim per edge
  bool ascending = false;  // ... finite and strictly ascending
  double lambda = 0;
};

// The families a plan with these facts may still run, as a mask of 1 << family, or 0 and the refusal in *why.
unsigned trws_families_possible(const TrwsPlanFacts &f, const char **why);
constexpr bool possible(unsigned families, TrwsFamily f) { return (families >> (int)f) & 1u; }

// The family that runs, or None and the refusal in *why.  in == nullptr (no inputs yet): the family the plan runs
// unless its inputs select a better one; nothing that depends on the inputs is refused.
TrwsFamily trws_family(const TrwsPlanFacts &f, const TrwsInputFacts *in, const char **why);

}  // namespace stereo
