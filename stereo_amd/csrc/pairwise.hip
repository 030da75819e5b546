// Pairwise-term and TRW-S position kernels (MI355X / gfx950) + their C ABI.
//
// Device versions of the MATLAB array math that feeds the two solvers:
//   dispmap_super.m:318-328   plane -> disparity
//   dispmap_super.m:226-262   truncated |p-q|^k pairwise terms (E00, E01, E10, E11)
//   dispmap_super.m:177-183   q / qprim of K proposals for TRW-S
// Independent per edge: one thread each, coalesced along the edge index.  HBM-bound streaming kernels; no
// contraction (-ffp-contract=off) so that + - * / match numpy.
#include "ncc_sample.h"
#include "terms_host.h"

namespace stereo {
namespace {

__device__ __forceinline__ double pair_term(int kernel, double w, double p, double q, double tol) {
  const double d = p - q;
  const double v = kernel == 1 ? fabs(d) : d * d;
  return w * (v < tol ? v : tol);
}

__global__ __launch_bounds__(kTB) void pairwise_terms_kernel(int kernel, int64_t E, const uint32_t *conn,
                                                            const double *points, const double *cur,
                                                            const double *prop, const double *w, double tol,
                                                            double d_min, double d_step, double *E00,
                                                            double *E01, double *E10, double *E11) {
  const int64_t e = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (e >= E) return;
  const uint32_t i1 = conn[2 * e], i2 = conn[2 * e + 1];
  const double x = points[2 * (size_t)i2], y = points[2 * (size_t)i2 + 1];
  double q = plane_disp(cur + 4 * (size_t)i2, x, y), qp = plane_disp(cur + 4 * (size_t)i1, x, y);
  if (d_step != 0) { q = (q - d_min) / d_step; qp = (qp - d_min) / d_step; }
  const double we = w[e];
  E00[e] = pair_term(kernel, we, q, qp, tol);
  if (prop) {
    double nq = plane_disp(prop + 4 * (size_t)i2, x, y), nqp = plane_disp(prop + 4 * (size_t)i1, x, y);
    if (d_step != 0) { nq = (nq - d_min) / d_step; nqp = (nqp - d_min) / d_step; }
    E11[e] = pair_term(kernel, we, nq, nqp, tol);
    E10[e] = pair_term(kernel, we, q, nqp, tol);   // dispmap_super.m:256
    E01[e] = pair_term(kernel, we, nq, qp, tol);   // dispmap_super.m:259
  }
}

__global__ __launch_bounds__(kTB) void trws_positions_kernel(int64_t E, int K, int64_t N, const uint32_t *conn,
                                                            const double *points, const double *props,
                                                            double d_min, double d_step, double *q,
                                                            double *qprim) {
  const int64_t t = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (t >= E * K) return;
  const int64_t e = t / K;
  const int k = (int)(t % K);
  const uint32_t i1 = conn[2 * e], i2 = conn[2 * e + 1];
  const double x = points[2 * (size_t)i2], y = points[2 * (size_t)i2 + 1];
  const double *P = props + (size_t)k * 4 * N;
  double a = plane_disp(P + 4 * (size_t)i2, x, y), b = plane_disp(P + 4 * (size_t)i1, x, y);
  if (d_step != 0) { a = (a - d_min) / d_step; b = (b - d_min) / d_step; }
  q[t] = a;       // K x E column major: label fastest
  qprim[t] = b;
}

}  // namespace

void launch_pairwise_terms(int kernel, int64_t E, const uint32_t *conn, const double *points, const double *cur,
                           const double *prop, const double *w, double tol, double d_min, double d_step, double *E00,
                           double *E01, double *E10, double *E11) {
  hipLaunchKernelGGL(pairwise_terms_kernel, dim3(blocks(E)), dim3(kTB), 0, 0, kernel, E, conn, points, cur, prop, w, tol,
                     d_min, d_step, E00, E01, E10, E11);
}

void launch_trws_positions(int64_t E, int K, int64_t N, const uint32_t *conn, const double *points, const double *props,
                           double d_min, double d_step, double *q, double *qprim) {
  hipLaunchKernelGGL(trws_positions_kernel, dim3(blocks(E * K)), dim3(kTB), 0, 0, E, K, N, conn, points, props, d_min,
                     d_step, q, qprim);
}

}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_pairwise_terms(int kernel, int64_t N, int64_t E, const uint32_t *conn, const double *points,
                          const double *assignment, const double *proposal, const double *weights, double tol,
                          double d_min, double d_step, double *E00, double *E01, double *E10, double *E11,
                          char *err, size_t errcap) {
  if (kernel != 1 && kernel != 2) return fail("Unkown kernel type", err, errcap);  // dispmap_super.m:233
  if (!conn || !points || !assignment || !weights || !E00 || (proposal && (!E01 || !E10 || !E11)))
    return fail("stereo_pairwise_terms: NULL argument", err, errcap);
  return guarded_sync("stereo_pairwise_terms", err, errcap, [&] {
    check_planes(assignment, N);
    if (proposal) check_planes(proposal, N);
    DevBuf<uint32_t> dc; DevBuf<double> dp, da, dpr, dw, o0, o1, o2, o3;
    dc.upload(conn, 2 * E); dp.upload(points, 2 * N); da.upload(assignment, 4 * N); dw.upload(weights, E);
    if (proposal) dpr.upload(proposal, 4 * N);
    o0.alloc(E); o1.alloc(E); o2.alloc(E); o3.alloc(E);
    launch_pairwise_terms(kernel, E, dc.p, dp.p, da.p, proposal ? dpr.p : nullptr, dw.p, tol, d_min, d_step, o0.p, o1.p,
                          o2.p, o3.p);
    download(E00, o0, E);
    if (proposal) { download(E01, o1, E); download(E10, o2, E); download(E11, o3, E); }
  });
}

int stereo_trws_positions(int64_t N, int64_t E, int K, const uint32_t *conn, const double *points,
                          const double *proposals, double d_min, double d_step, double *q, double *qprim,
                          char *err, size_t errcap) {
  if (!conn || !points || !proposals || !q || !qprim || K < 1)
    return fail("stereo_trws_positions: bad argument", err, errcap);
  return guarded_sync("stereo_trws_positions", err, errcap, [&] {
    check_planes(proposals, N * K);
    DevBuf<uint32_t> dc; DevBuf<double> dp, dpr, oq, oqp;
    dc.upload(conn, 2 * E); dp.upload(points, 2 * N); dpr.upload(proposals, (size_t)4 * N * K);
    oq.alloc((size_t)E * K); oqp.alloc((size_t)E * K);
    launch_trws_positions(E, K, N, dc.p, dp.p, dpr.p, d_min, d_step, oq.p, oqp.p);
    download(q, oq, (size_t)E * K); download(qprim, oqp, (size_t)E * K);
  });
}

}  // extern "C"
