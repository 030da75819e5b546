// TRW-S node beliefs after a run: min-marginals, confidence, argmin.
//
// No reference counterpart as an output; the values are what MRFEnergy's forward pass of the iteration
// after the last one forms at each node (cpp/trw-s/minimize.cpp:38-46):
//   Di = D_i + sum_{e in firstForward(i)} m_e + sum_{e in firstBackward(i)} m_e
// One message state at rest never holds every node's incoming messages (each edge stores one message,
// its direction flips every sweep), so the sum is taken in two phases:
//   trws_beliefs_accum_kernel   between the backward sweep of iteration t and the fused forward sweep of
//                               t + 1: P_i = D_i + firstForward messages (they point into i right then)
//   trws_beliefs_finish_kernel  after the run: Di = P_i + firstBackward messages (the forward messages of
//                               t + 1), then Di - min Di, the second-smallest entry of that and the first
//                               argmin (lexicographic (value, index) minimum as trws_dev.h's wave_argmin)
// Every sum is the reference's sequence of fp64 adds in list order (-ffp-contract=off).
//
// Mapping: a group of G lanes per node, G = the power of two >= K up to 64, so a wave holds 64 / G nodes
// (K = 15: four nodes, 120-byte rows); above 64 labels one wave per node with a strided label loop.
// Nodes are taken in rank order (the lists are per rank), rows are written in node-id order, label
// fastest (MATLAB's K x N).  Both kernels stream: phase 1 moves 8 K (2 N + E) bytes, phase 2
// 8 K (2 N + E) + 12 N.
//
// Row strips and batches: a strip runs the same two phases over its OWN nodes -- `order` holds their strip-local ids
// in rank order, the lists strip-local edge ids in the global list order (trws_graph.h: StripBeliefLists), unary,
// messages and the partial sums are the strip's own arrays -- and phase 2 may put the rows back at global node ids
// through the strip's local -> global table.  Several plans that iterate together (the logical strips of a device,
// the members of a batch) share ONE launch per phase: the *_group_kernel forms take a table of per-plan blocks in
// device memory and map a workgroup to (plan, rank slice) by a prefix over the plans' workgroup counts; the plans
// may differ in K and in the lane grouping.  Per node the arithmetic is the single plan's, add for add.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "trws_launch.h"

namespace stereo {
namespace {

constexpr int kBelWave = 64;
constexpr int kBelBlock = 256;

__device__ __forceinline__ int64_t belief_rank(unsigned block, int lg) {
  const int lane = threadIdx.x & (kBelWave - 1);
  const int64_t wave = (int64_t)block * (kBelBlock / kBelWave) + threadIdx.x / kBelWave;
  return wave * (kBelWave >> lg) + (lane >> lg);
}

// phase 1 for the node of rank r (block: the workgroup's index among those of its plan)
__device__ __forceinline__ void beliefs_accum(unsigned block, const double *__restrict__ unary, const double *__restrict__ msg,
                                              const int32_t *__restrict__ order, const int32_t *__restrict__ fptr,
                                              const int32_t *__restrict__ fidx, int K, int64_t N, int lg,
                                              double *__restrict__ out) {
  const int64_t r = belief_rank(block, lg);
  if (r >= N) return;
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const size_t row = (size_t)order[r] * K;
  const int i0 = fptr[r], i1 = fptr[r + 1];
  for (int k = sub; k < K; k += G) {
    double acc = unary[row + k];
    for (int i = i0; i < i1; ++i) acc += msg[(size_t)fidx[i] * K + k];
    out[row + k] = acc;
  }
}

// phase 2; map: the output rows' node ids (a strip's local -> global table), NULL: the ids of `order`
__device__ __forceinline__ void beliefs_finish(unsigned block, const double *__restrict__ part, const double *__restrict__ msg,
                                               const int32_t *__restrict__ order, const int32_t *__restrict__ bptr,
                                               const int32_t *__restrict__ bidx, const int64_t *__restrict__ map, int K,
                                               int64_t N, int lg, double *mm, double *conf, int32_t *argmin) {
  const int64_t r = belief_rank(block, lg);
  if (r >= N) return;
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const int node = order[r];
  const size_t row = (size_t)node * K;
  const int64_t to = map ? map[node] : (int64_t)node;
  const size_t orow = (size_t)to * K;
  const int i0 = bptr[r], i1 = bptr[r + 1];
  // per lane: smallest value, its (first) label, second-smallest value
  double m1 = __builtin_huge_val(), m2 = __builtin_huge_val();
  int a1 = 0x7fffffff;
  double own = 0;
  for (int k = sub; k < K; k += G) {
    double d = part[row + k];
    for (int i = i0; i < i1; ++i) d += msg[(size_t)bidx[i] * K + k];
    if (d < m1) { m2 = m1; m1 = d; a1 = k; }
    else if (d < m2) m2 = d;
    own = d;
    if (mm && K > G) mm[orow + k] = d;   // (several labels per lane: normalised in a second pass)
  }
  // across the group (G lanes, aligned: the xor partners stay inside it)
  for (int off = G >> 1; off > 0; off >>= 1) {
    const double o1 = __shfl_xor(m1, off, kBelWave), o2 = __shfl_xor(m2, off, kBelWave);
    const int oa = __shfl_xor(a1, off, kBelWave);
    if (o1 < m1 || (o1 == m1 && oa < a1)) { m2 = m1 < o2 ? m1 : o2; m1 = o1; a1 = oa; }
    else m2 = m2 < o1 ? m2 : o1;
  }
  if (mm) {
    if (K <= G) { if (sub < K) mm[orow + sub] = own - m1; }
    else for (int k = sub; k < K; k += G) mm[orow + k] = mm[orow + k] - m1;
  }
  if (sub == 0) {
    if (conf) conf[to] = K == 1 ? __builtin_huge_val() : m2 - m1;
    if (argmin) argmin[to] = a1;
  }
}

// the plan a workgroup of a grouped launch works for
__device__ __forceinline__ int belief_member(const BeliefGroupArgs &ga) {
  int m = 0;
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i) m = (i < ga.n && (int)blockIdx.x >= ga.first[i]) ? i : m;  // static indices only
  return m;
}

}  // namespace

__global__ __launch_bounds__(kBelBlock) void trws_beliefs_accum_kernel(const double *__restrict__ unary,
                                                                       const double *__restrict__ msg,
                                                                       const int32_t *__restrict__ order,
                                                                       const int32_t *__restrict__ fptr,
                                                                       const int32_t *__restrict__ fidx, int K,
                                                                       int64_t N, int lg, double *__restrict__ out) {
  beliefs_accum(blockIdx.x, unary, msg, order, fptr, fidx, K, N, lg, out);
}

__global__ __launch_bounds__(kBelBlock) void trws_beliefs_finish_kernel(const double *__restrict__ part,
                                                                        const double *__restrict__ msg,
                                                                        const int32_t *__restrict__ order,
                                                                        const int32_t *__restrict__ bptr,
                                                                        const int32_t *__restrict__ bidx, int K,
                                                                        int64_t N, int lg, double *mm, double *conf,
                                                                        int32_t *argmin) {
  // (beliefs_finish without a map, kept as its own text: through the shared body the compiler allocates this kernel's
  //  registers differently, and the single plan's kernels stay instruction for instruction what they were)
  const int64_t r = belief_rank(blockIdx.x, lg);
  if (r >= N) return;
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const int node = order[r];
  const size_t row = (size_t)node * K;
  const int i0 = bptr[r], i1 = bptr[r + 1];
  double m1 = __builtin_huge_val(), m2 = __builtin_huge_val();
  int a1 = 0x7fffffff;
  double own = 0;
  for (int k = sub; k < K; k += G) {
    double d = part[row + k];
    for (int i = i0; i < i1; ++i) d += msg[(size_t)bidx[i] * K + k];
    if (d < m1) { m2 = m1; m1 = d; a1 = k; }
    else if (d < m2) m2 = d;
    own = d;
    if (mm && K > G) mm[row + k] = d;
  }
  for (int off = G >> 1; off > 0; off >>= 1) {
    const double o1 = __shfl_xor(m1, off, kBelWave), o2 = __shfl_xor(m2, off, kBelWave);
    const int oa = __shfl_xor(a1, off, kBelWave);
    if (o1 < m1 || (o1 == m1 && oa < a1)) { m2 = m1 < o2 ? m1 : o2; m1 = o1; a1 = oa; }
    else m2 = m2 < o1 ? m2 : o1;
  }
  if (mm) {
    if (K <= G) { if (sub < K) mm[row + sub] = own - m1; }
    else for (int k = sub; k < K; k += G) mm[row + k] = mm[row + k] - m1;
  }
  if (sub == 0) {
    if (conf) conf[node] = K == 1 ? __builtin_huge_val() : m2 - m1;
    if (argmin) argmin[node] = a1;
  }
}

// ... of one plan with its rows put at the node ids of `map` (a strip read into arrays of the whole problem)
__global__ __launch_bounds__(kBelBlock) void trws_beliefs_finish_map_kernel(const double *__restrict__ part,
                                                                            const double *__restrict__ msg,
                                                                            const int32_t *__restrict__ order,
                                                                            const int32_t *__restrict__ bptr,
                                                                            const int32_t *__restrict__ bidx,
                                                                            const int64_t *__restrict__ map, int K, int64_t N,
                                                                            int lg, double *mm, double *conf, int32_t *argmin) {
  beliefs_finish(blockIdx.x, part, msg, order, bptr, bidx, map, K, N, lg, mm, conf, argmin);
}

// Several plans in one launch.  Phase 1: block.in = unary, block.ptr / idx = the firstForward lists, block.out = the
// plan's partial sums.
__global__ __launch_bounds__(kBelBlock) void trws_beliefs_accum_group_kernel(BeliefGroupArgs ga) {
  const int m = belief_member(ga);
  const BeliefBlock &b = ga.pp[m];
  beliefs_accum(blockIdx.x - (unsigned)ga.first[m], b.in, b.msg, b.order, b.ptr, b.idx, b.K, b.n, b.lg, b.out);
}

// Phase 2: block.in = the partial sums, block.ptr / idx = the firstBackward lists, block.map = local -> global node
// ids; every plan's rows go into the one mm / conf / argmin set (strips of one problem: disjoint own nodes).
__global__ __launch_bounds__(kBelBlock) void trws_beliefs_finish_group_kernel(BeliefGroupArgs ga, double *mm, double *conf,
                                                                              int32_t *argmin) {
  const int m = belief_member(ga);
  const BeliefBlock &b = ga.pp[m];
  beliefs_finish(blockIdx.x - (unsigned)ga.first[m], b.in, b.msg, b.order, b.ptr, b.idx, b.map, b.K, b.n, b.lg, mm, conf, argmin);
}

namespace {
int lanes_log2(int K) {
  int lg = 0;
  while ((1 << lg) < K && lg < 6) ++lg;
  return lg;
}
unsigned belief_blocks(int64_t N, int lg) {
  const int64_t per_block = (int64_t)(kBelBlock / kBelWave) * (kBelWave >> lg);
  return (unsigned)((N + per_block - 1) / per_block);
}
}  // namespace

void launch_beliefs_accum(const double *unary, const double *msg, const int32_t *order, const int32_t *fptr,
                          const int32_t *fidx, int K, int64_t N, double *out, hipStream_t s) {
  if (N <= 0) return;
  const int lg = lanes_log2(K);
  hipLaunchKernelGGL(trws_beliefs_accum_kernel, dim3(belief_blocks(N, lg)), dim3(kBelBlock), 0, s, unary, msg, order,
                     fptr, fidx, K, N, lg, out);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_beliefs_finish(const double *part, const double *msg, const int32_t *order, const int32_t *bptr,
                           const int32_t *bidx, int K, int64_t N, double *mm, double *conf, int32_t *argmin,
                           hipStream_t s) {
  if (N <= 0) return;
  const int lg = lanes_log2(K);
  hipLaunchKernelGGL(trws_beliefs_finish_kernel, dim3(belief_blocks(N, lg)), dim3(kBelBlock), 0, s, part, msg, order,
                     bptr, bidx, K, N, lg, mm, conf, argmin);
  STEREO_HIP_CHECK(hipGetLastError());
}

int beliefs_lanes_log2(int K) { return lanes_log2(K); }
int beliefs_workgroups(int64_t N, int K) { return N > 0 ? (int)belief_blocks(N, lanes_log2(K)) : 0; }

void launch_beliefs_finish_map(const double *part, const double *msg, const int32_t *order, const int32_t *bptr,
                               const int32_t *bidx, const int64_t *map, int K, int64_t N, double *mm, double *conf,
                               int32_t *argmin, hipStream_t s) {
  if (N <= 0) return;
  const int lg = lanes_log2(K);
  hipLaunchKernelGGL(trws_beliefs_finish_map_kernel, dim3(belief_blocks(N, lg)), dim3(kBelBlock), 0, s, part, msg, order,
                     bptr, bidx, map, K, N, lg, mm, conf, argmin);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_beliefs_accum_group(const BeliefGroupArgs &ga, hipStream_t s) {
  if (ga.first[ga.n] <= 0) return;
  hipLaunchKernelGGL(trws_beliefs_accum_group_kernel, dim3((unsigned)ga.first[ga.n]), dim3(kBelBlock), 0, s, ga);
  STEREO_HIP_CHECK(hipGetLastError());
}

void launch_beliefs_finish_group(const BeliefGroupArgs &ga, double *mm, double *conf, int32_t *argmin, hipStream_t s) {
  if (ga.first[ga.n] <= 0) return;
  hipLaunchKernelGGL(trws_beliefs_finish_group_kernel, dim3((unsigned)ga.first[ga.n]), dim3(kBelBlock), 0, s, ga, mm, conf, argmin);
  STEREO_HIP_CHECK(hipGetLastError());
}

}  // namespace stereo
