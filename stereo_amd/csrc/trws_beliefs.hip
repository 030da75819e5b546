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
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "trws_launch.h"

namespace stereo {
namespace {

constexpr int kBelWave = 64;
constexpr int kBelBlock = 256;

__device__ __forceinline__ int64_t belief_rank(int lg) {
  const int lane = threadIdx.x & (kBelWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kBelBlock / kBelWave) + threadIdx.x / kBelWave;
  return wave * (kBelWave >> lg) + (lane >> lg);
}

}  // namespace

__global__ __launch_bounds__(kBelBlock) void trws_beliefs_accum_kernel(const double *__restrict__ unary,
                                                                       const double *__restrict__ msg,
                                                                       const int32_t *__restrict__ order,
                                                                       const int32_t *__restrict__ fptr,
                                                                       const int32_t *__restrict__ fidx, int K,
                                                                       int64_t N, int lg, double *__restrict__ out) {
  const int64_t r = belief_rank(lg);
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

__global__ __launch_bounds__(kBelBlock) void trws_beliefs_finish_kernel(const double *__restrict__ part,
                                                                        const double *__restrict__ msg,
                                                                        const int32_t *__restrict__ order,
                                                                        const int32_t *__restrict__ bptr,
                                                                        const int32_t *__restrict__ bidx, int K,
                                                                        int64_t N, int lg, double *mm, double *conf,
                                                                        int32_t *argmin) {
  const int64_t r = belief_rank(lg);
  if (r >= N) return;
  const int G = 1 << lg;
  const int sub = threadIdx.x & (G - 1);
  const int node = order[r];
  const size_t row = (size_t)node * K;
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
    if (mm && K > G) mm[row + k] = d;   // (several labels per lane: normalised in a second pass)
  }
  // across the group (G lanes, aligned: the xor partners stay inside it)
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

}  // namespace stereo
