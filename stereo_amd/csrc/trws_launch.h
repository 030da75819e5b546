// Host-side launchers of the TRW-S sweep kernel families (one translation unit each).
// what: 0 = forward sweep, 1 = backward sweep, 2 = forward sweep + primal pass of the previous
// iteration, 3 = primal pass only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "common.h"
#include "trws_dev.h"

namespace stereo {

// The four sweep variants (BACKWARD, PRIMAL, UPDATE) in `what` order: X(BW, PR, UP, ...) once per variant.  A family
// file builds its table of kernel addresses from this list exactly once -- one row of four per (smoothness kernel,
// shared positions or message mode, plain / group / speculative entry) --, its *_set_attributes walks the table and its
// launch_* index it, so the kernels that are launched and the kernels that got their LDS size are the same by
// construction.
#define TRWS_SWEEP_VARIANTS(X, ...) \
  X(false, false, true, __VA_ARGS__) X(true, false, true, __VA_ARGS__) X(false, true, true, __VA_ARGS__) X(false, true, false, __VA_ARGS__)
typedef const void *SweepRow[4];

// every kernel of `rows` may use `bytes` of dynamic LDS (above 64 KB a kernel without this fails at launch)
inline void set_max_dynamic_lds(const SweepRow *rows, int nrows, int bytes) {
  for (int r = 0; r < nrows; ++r)
    for (const void *k : rows[r]) STEREO_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}
// launches row[what] with (arg, epoch); arg: DevParams, or GroupArgs for the group kernels
template <class Arg>
inline void launch_sweep(const SweepRow &row, int what, int blocks, int threads, size_t lds, hipStream_t s, const Arg &arg, int epoch) {
  void *args[] = {(void *)&arg, (void *)&epoch};
  STEREO_HIP_CHECK(hipLaunchKernel(row[what >= 0 && what < 3 ? what : 3], dim3(blocks), dim3(threads), args, lds, s));
  STEREO_HIP_CHECK(hipGetLastError());
}

size_t generic_lds_bytes(int Kp);
void generic_set_attributes(int lds);
void launch_generic(int kernel, int mode, int what, int blocks, size_t lds, hipStream_t s, const DevParams &p, int epoch);

size_t large_lds_bytes(int Kp);
size_t large_scratch_doubles(int Kp);
void large_set_attributes(int lds);
void launch_large(int kernel, int mode, int what, int blocks, size_t lds, hipStream_t s, const DevParams &p, int epoch);

size_t pipe_lds_bytes();
int pipe_threads();
void pipe_set_attributes();
void launch_pipe(int kernel, bool shared, int what, int blocks, hipStream_t s, const DevParams &p, int epoch);
void launch_pipe_group(int kernel, bool shared, int what, int blocks, hipStream_t s, const GroupArgs &ga, int epoch);
// independent problems in one launch, workgroups that move between them (stereo_trws_batch_*); how many of its
// workgroups a compute unit holds at once
void launch_pipe_batch(int kernel, bool shared, int what, int blocks, hipStream_t s, const BatchArgs &ba, int epoch);
int pipe_batch_resident_per_cu(int kernel, bool shared);

size_t pipe2_lds_bytes();
void pipe2_set_attributes();
void launch_pipe2(int kernel, bool shared, int what, int blocks, hipStream_t s, const DevParams &p, int epoch);
void launch_pipe2_group(int kernel, bool shared, int what, int blocks, hipStream_t s, const GroupArgs &ga, int epoch);

size_t wide_lds_bytes();
void wide_set_attributes();
void launch_wide(int kernel, int what, int blocks, hipStream_t s, const DevParams &p, int epoch);
void launch_wide_group(int kernel, int what, int blocks, hipStream_t s, const GroupArgs &ga, int epoch);

// node beliefs after a run (trws_beliefs.hip): phase 1 between the backward sweep and the fused forward
// sweep of an iteration, phase 2 on request after the run; K x N label-fastest rows in node-id order
void launch_beliefs_accum(const double *unary, const double *msg, const int32_t *order, const int32_t *fptr,
                          const int32_t *fidx, int K, int64_t N, double *out, hipStream_t s);
void launch_beliefs_finish(const double *part, const double *msg, const int32_t *order, const int32_t *bptr,
                           const int32_t *bidx, int K, int64_t N, double *mm, double *conf, int32_t *argmin,
                           hipStream_t s);
// phase 2 of a strip with its rows written at map[local node id] (local -> global) in arrays of the whole problem
void launch_beliefs_finish_map(const double *part, const double *msg, const int32_t *order, const int32_t *bptr,
                               const int32_t *bidx, const int64_t *map, int K, int64_t N, double *mm, double *conf,
                               int32_t *argmin, hipStream_t s);
// Either phase for several plans in ONE launch (the logical strips of a device, the members of a batch): a table of
// blocks in device memory, workgroup b works for plan m with first[m] <= b < first[m + 1] (beliefs_workgroups each).
// Phase 1: in = unary, ptr / idx = firstForward lists, out = partial sums.  Phase 2: in = partial sums, ptr / idx =
// firstBackward lists, map = local -> global node ids or NULL; one output set for all plans.
struct BeliefBlock {
  const double *in, *msg;
  const int32_t *order, *ptr, *idx;
  const int64_t *map;
  double *out;
  int64_t n;
  int K, lg;
};
struct BeliefGroupArgs {
  const BeliefBlock *pp;
  int n;
  int first[kMaxGroup + 1];
};
int beliefs_lanes_log2(int K);
int beliefs_workgroups(int64_t N, int K);
void launch_beliefs_accum_group(const BeliefGroupArgs &ga, hipStream_t s);
void launch_beliefs_finish_group(const BeliefGroupArgs &ga, double *mm, double *conf, int32_t *argmin, hipStream_t s);

}  // namespace stereo
