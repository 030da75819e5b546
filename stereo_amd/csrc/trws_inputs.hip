// TRW-S plan inputs: the sort permutations of the positions (in the order the reference's gateway hands them to the
// message code) and the analysis of one shared positions vector.  File map: trws_plan.hip.
#include <algorithm>
#include <cmath>
#include <limits>
#include <thread>
#include <utility>

#include "trws_plan.h"

namespace stereo {

namespace {

// Ascending sort permutation of each K-vector (ties: lower index first), one
// wave per vector, bitonic network in LDS.  Replaces the per-edge std::sort of
// trws_mex.cpp:84-119 (which re-sorts after every push_back).
__global__ __launch_bounds__(kWave) void argsort_kernel(const double *vals, uint16_t *perm, int K,
                                                        int P, int64_t count) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double *v = lds;
  int *id = (int *)(lds + P);
  const int lane = threadIdx.x;
  for (int64_t a = blockIdx.x; a < count; a += gridDim.x) {
    const double *src = vals + (size_t)a * K;
    for (int i = lane; i < P; i += kWave) {
      v[i] = i < K ? src[i] : __builtin_huge_val();
      id[i] = i < K ? i : (0x10000 + i);
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < P / 2; t += kWave) {
          const int lo = (t / stride) * (stride * 2) + (t % stride);
          const int hi = lo + stride;
          const bool up = ((lo & size) == 0);
          const double a0 = v[lo], a1 = v[hi];
          const int i0 = id[lo], i1 = id[hi];
          const bool gt = (a0 > a1) || (a0 == a1 && i0 > i1);
          if (gt == up) { v[lo] = a1; v[hi] = a0; id[lo] = i1; id[hi] = i0; }
        }
        __syncthreads();
      }
    }
    uint16_t *dstp = perm + (size_t)a * K;
    for (int i = lane; i < K; i += kWave) dstp[i] = (uint16_t)id[i];
    __syncthreads();
  }
}

// Rows whose ascending order holds two equal values (the order of equal positions needs the
// reference gateway's own sort sequence, see gateway_order below); one thread per row.
__global__ __launch_bounds__(kBlock) void equal_values_kernel(const double *vals, const uint16_t *perm, int K,
                                                             int64_t count, uint8_t *flag) {
  const int64_t a = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (a >= count) return;
  const double *v = vals + (size_t)a * K;
  const uint16_t *pm = perm + (size_t)a * K;
  bool eq = false;
  double prev = v[pm[0]];
  for (int k = 1; k < K; ++k) { const double x = v[pm[k]]; eq = eq || x == prev; prev = x; }
  flag[a] = eq ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(const double *vals, const int64_t *rows, int64_t n, int K,
                                                            double *out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < n * K) out[t] = vals[(size_t)rows[t / K] * K + t % K];
}
__global__ __launch_bounds__(kBlock) void scatter_perm_kernel(const uint16_t *in, const int64_t *rows, int64_t n, int K,
                                                             uint16_t *perm) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < n * K) perm[(size_t)rows[t / K] * K + t % K] = in[t];
}

}  // namespace

void run_argsort(const double *vals, uint16_t *perm, int K, int64_t count, hipStream_t s) {
  int Pw = 2;
  while (Pw < K) Pw <<= 1;
  const size_t lds = (size_t)Pw * (sizeof(double) + sizeof(int));
  const int64_t grid = std::min<int64_t>(count, 256 * 32);
  hipLaunchKernelGGL(argsort_kernel, dim3((unsigned)grid), dim3(kWave), lds, s, vals, perm, K, Pw, count);
  STEREO_HIP_CHECK(hipGetLastError());
}

// The order in which the reference's gateway hands EQUAL positions to the message code.
// trws_mex.cpp:84-97 pushes one (value, index) pair at a time and calls std::sort on the whole
// vector after every push, comparing values only (:16-20).  std::sort is not stable: up to 16
// elements it is an insertion sort (equal values stay in index order -- what argsort_kernel
// produces), beyond that its introsort may swap equal values.  Equal positions are no corner
// case: simultaneous_fusion appends the current assignment as a label (dispmap_super.m:158), so
// wherever a proposal's plane is the current plane two labels coincide exactly.  For such vectors
// the same sequence of calls is made here, with the std::sort of the toolchain in use -- what a
// reference built with that toolchain does.
static void gateway_order(const double *v, int K, uint16_t *perm) {
  typedef std::pair<double, int> Pair;
  struct Cmp {
    bool operator()(const Pair &a, const Pair &b) const { return a.first < b.first; }
  };
  std::vector<Pair> pr;
  pr.reserve(K);
  for (int j = 0; j < K; ++j) {
    pr.push_back(Pair(v[j], j));
    std::sort(pr.begin(), pr.end(), Cmp());
  }
  for (int j = 0; j < K; ++j) perm[j] = (uint16_t)pr[j].second;
}

// After argsort_kernel: rows with equal values get the gateway's order (K > 16 only, see above).
void fix_equal_positions(const double *d_vals, uint16_t *d_perm, int K, int64_t count) {
  if (K <= 16 || count <= 0) return;
  DevBuf<uint8_t> d_flag;
  d_flag.alloc(count);
  hipLaunchKernelGGL(equal_values_kernel, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, 0, d_vals,
                     d_perm, K, count, d_flag.p);
  STEREO_HIP_CHECK(hipGetLastError());
  std::vector<uint8_t> flag(count);
  STEREO_HIP_CHECK(hipMemcpy(flag.data(), d_flag.p, count, hipMemcpyDeviceToHost));
  std::vector<int64_t> rows;
  for (int64_t a = 0; a < count; ++a)
    if (flag[a]) rows.push_back(a);
  const int64_t n = (int64_t)rows.size();
  if (n == 0) return;
  DevBuf<int64_t> d_rows;
  DevBuf<double> d_g;
  DevBuf<uint16_t> d_p;
  d_rows.upload(rows.data(), n);
  d_g.alloc((size_t)n * K); d_p.alloc((size_t)n * K);
  const unsigned gb = (unsigned)(((int64_t)n * K + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(gb), dim3(kBlock), 0, 0, d_vals, d_rows.p, n, K, d_g.p);
  STEREO_HIP_CHECK(hipGetLastError());
  std::vector<double> g((size_t)n * K);
  STEREO_HIP_CHECK(hipMemcpy(g.data(), d_g.p, sizeof(double) * n * K, hipMemcpyDeviceToHost));
  std::vector<uint16_t> pm((size_t)n * K);
  const int64_t T = std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency() / 2, 64, n / 256 + 1}));
  std::vector<std::thread> pool;
  auto work = [&](int64_t a, int64_t b) { for (int64_t i = a; i < b; ++i) gateway_order(&g[(size_t)i * K], K, &pm[(size_t)i * K]); };
  for (int64_t t = 1; t < T; ++t) pool.emplace_back(work, n * t / T, n * (t + 1) / T);
  work(0, n / T);
  for (auto &th : pool) th.join();
  STEREO_HIP_CHECK(hipMemcpy(d_p.p, pm.data(), sizeof(uint16_t) * n * K, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(scatter_perm_kernel, dim3(gb), dim3(kBlock), 0, 0, d_p.p, d_rows.p, n, K, d_perm);
  STEREO_HIP_CHECK(hipGetLastError());
  STEREO_HIP_CHECK(hipDeviceSynchronize());
}

void gather_rows(const double *d_full, const int64_t *d_rows, int64_t n, int width, double *d_out) {
  const unsigned gb = (unsigned)((n * width + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(gb), dim3(kBlock), 0, 0, d_full, d_rows, n, width, d_out);
  STEREO_HIP_CHECK(hipGetLastError());
}

void sort_positions(stereo_trws_plan *P) {
  if (P->pos) {
    P->d_perm_pos.alloc(P->K);
    run_argsort(P->pos, P->d_perm_pos.p, P->K, 1, nullptr);
    fix_equal_positions(P->pos, P->d_perm_pos.p, P->K, 1);
    P->d_perm_q.release(); P->d_perm_qp.release();
  } else {
    P->d_perm_q.alloc((size_t)P->El * P->K);
    P->d_perm_qp.alloc((size_t)P->El * P->K);
    run_argsort(P->q, P->d_perm_q.p, P->K, P->El, nullptr);
    run_argsort(P->qprim, P->d_perm_qp.p, P->K, P->El, nullptr);
    fix_equal_positions(P->q, P->d_perm_q.p, P->K, P->El);
    fix_equal_positions(P->qprim, P->d_perm_qp.p, P->K, P->El);
  }
  STEREO_HIP_CHECK(hipDeviceSynchronize());
}

bool positions_ascend(const double *d_pos, int K, std::vector<double> &hp) {
  hp.resize(K);
  STEREO_HIP_CHECK(hipMemcpy(hp.data(), d_pos, sizeof(double) * K, hipMemcpyDeviceToHost));
  bool asc = std::isfinite(hp[0]);
  for (int k = 1; k < K && asc; ++k) asc = std::isfinite(hp[k]) && hp[k] > hp[k - 1];
  return asc;
}

// truncation window in index steps (windowed min-plus of the pipelined kernel's flat-h path; the wide-label kernel
// requires it)
void analyse_window(stereo_trws_plan *P, const std::vector<double> &hp) {
  // a source farther than lambda from a destination (squared distance for kernel 2)
  // costs >= vTrunc, so min-plus only needs the sources within +-window indices
  int w = 0;
  for (int k = 0, lo = 0; k < P->K; ++k) {
    for (;; ++lo) {
      const double d = hp[k] - hp[lo];
      if ((P->kernel == 1 ? d : d * d) <= (P->kernel == 1 ? P->lambda : P->lambda * (1 + 1e-9))) break;
    }
    w = std::max(w, k - lo);
  }
  P->window = w;
  P->pos_ascending = true;
  // exact arithmetic progression inside the window?  (then alpha |t - q| = alpha |d step| bit for bit)
  P->uniform_step = 0;
  if (w <= 16 && P->K > 1) {
    const double step = hp[1] - hp[0];
    bool uni = step > 0;
    for (int d = 1; d <= w && uni; ++d)
      for (int k = 0; k + d < P->K && uni; ++k) uni = (hp[k + d] - hp[k]) == (double)d * step;
    if (uni) P->uniform_step = step;
    // the runner of the speculative schedule (trws_spec.h) walks the window in groups of four entries: the
    // spacing must hold for those too, and what lies beyond the window must cost >= vTrunc as an index distance
    const int wr = (w + 3) & ~3;
    bool spw = uni && P->kernel == 1;
    for (int d = w + 1; d <= wr && spw; ++d) {
      spw = (double)d * step > P->lambda;
      for (int k = 0; k + d < P->K && spw; ++k) spw = (hp[k + d] - hp[k]) == (double)d * step;
    }
    P->spec_window = spw;
  }
}

}  // namespace stereo
