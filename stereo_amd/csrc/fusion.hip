// The device-resident fusion context (MI355X / gfx950): stereo_fusion_* of the C ABI.
//
// The dispmap object of the reference kept in HBM, a move uploads its proposal and returns scalars:
//   dispmap_super.m:57-84     binary_fusion
//   dispmap_super.m:85-152    binary_fuse_until_convergence
//   dispmap_super.m:153-198   simultaneous_fusion
//   dispmap_super.m:263-274   update_energy
//   dispmap_ncc.m:48-92       proposals: local plane fits
// The pairwise terms, the TRW-S positions and the unaries are the kernels of pairwise.hip and unary.hip, reached
// through their launchers (terms_host.h); the kernels here are the ones only the context runs.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "terms_host.h"

namespace stereo {
namespace {

// ---- device-resident fusion moves (stereo_fusion_*) -----------------------------------------
// dispmap_super.m:78-82: assignment(:, labelling == 1) = proposal(:, labelling == 1); the cached
// unary of the current assignment follows (the unary is a per-pixel function of the pixel's plane).
__global__ __launch_bounds__(kTB) void fusion_scatter_kernel(int64_t N, const int8_t *label, const double *prop,
                                                            const double *U1, double *cur, double *Ucur) {
  const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (i >= N || label[i] != 1) return;
  cur[4 * i] = prop[4 * i]; cur[4 * i + 1] = prop[4 * i + 1];
  cur[4 * i + 2] = prop[4 * i + 2]; cur[4 * i + 3] = prop[4 * i + 3];
  Ucur[i] = U1[i];
}

// unary of proposal k into the K x N (label fastest) layout TRW-S consumes
__global__ __launch_bounds__(kTB) void fusion_interleave_kernel(int64_t N, int K, int k, const double *Uk,
                                                               double *unary) {
  const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (i < N) unary[i * K + k] = Uk[i];
}

// dispmap_super.m:189-195: every pixel takes the plane of the proposal TRW-S chose for it;
// its unary follows from the K x N table
__global__ __launch_bounds__(kTB) void fusion_select_kernel(int64_t N, int K, const int32_t *label,
                                                           const double *props, const double *unary,
                                                           double *cur, double *Ucur) {
  const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (i >= N) return;
  const int k = label[i];
  const double *P = props + (size_t)k * 4 * N + 4 * i;
  cur[4 * i] = P[0]; cur[4 * i + 1] = P[1]; cur[4 * i + 2] = P[2]; cur[4 * i + 3] = P[3];
  Ucur[i] = unary[i * K + k];
}

// fixed-shape reduction (same tree for every run): partial[b] = sum of a 2048-element chunk
__global__ __launch_bounds__(kTB) void fusion_sum_kernel(const double *x, int64_t n, double *partial) {
  __shared__ double sh[kTB];
  const int64_t base = (int64_t)blockIdx.x * (kTB * 8);
  double acc = 0;
  for (int k = 0; k < 8; ++k) {
    const int64_t i = base + (int64_t)k * kTB + threadIdx.x;
    if (i < n) acc += x[i];
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s2 = kTB / 2; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) sh[threadIdx.x] += sh[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// ---- proposals built on the device --------------------------------------------
// A proposal of the reference's examples is never an arbitrary 4 x N array: it is one plane for
// every pixel (example_ncc.m:24-41: plane fits and fronto-parallel planes, repmat'ed,
// dispmap_ncc.m:65) or one plane per image segment (dispmap_globalstereo.m:154-192 SegPln).  Built
// from a 4 x S table (+ an N-vector of segment ids) in HBM, so a move uploads 32 S bytes, not 32 N.
__global__ __launch_bounds__(kTB) void proposal_from_planes_kernel(int64_t N, const double *planes, int S,
                                                                  const int32_t *segments, double *prop) {
  const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (i >= N) return;
  int sgm = segments ? segments[i] : 0;
  sgm = sgm < 0 ? 0 : sgm >= S ? S - 1 : sgm;
  prop[4 * i] = planes[4 * sgm]; prop[4 * i + 1] = planes[4 * sgm + 1];
  prop[4 * i + 2] = planes[4 * sgm + 2]; prop[4 * i + 3] = planes[4 * sgm + 3];
}

// dispmap_ncc.m:48-92 generate_new_plane_RANSAC + fit_plane_to_points: the plane through the
// winner-takes-all disparities of the pixels within radius r of (x, y) (1-based, x = column): total
// least squares (kernel 2) or 20 rounds of iteratively reweighted least squares (kernel 1).  The
// reference takes V(:, end) of svd(w .* cost): the eigenvector of the smallest eigenvalue of
// sum_i w_i^2 c_i c_i' -- found here by cyclic Jacobi rotations of that 3 x 3 matrix (MATLAB's svd
// is outside the reference tree: agreement with a LAPACK SVD to ~1e-9, not bit for bit; the sign
// of the vector cancels in p / p(3)).  At most (2r+1)^2 points: one thread does the arithmetic in
// the reference's order (pixels in column-major order), the rest of the wave idles.
constexpr int kFitMax = 1024;
// One workgroup per fit: blockIdx.x picks the centre (xy = [x_0 y_0 x_1 y_1 ...], 1-based pixel
// coordinates) and the output slot -- the whole lattice of example_ncc.m:24-32 is one launch.
__global__ __launch_bounds__(64) void fit_plane_kernel(const double *best, int H, int W, const double *xy, double r,
                                                      int kernel, double *out_all /* (4 + count) per fit */) {
  __shared__ double px[kFitMax], py[kFitMax], pz[kFitMax], wt[kFitMax];
  if (threadIdx.x != 0) return;
  const double x = xy[2 * blockIdx.x], y = xy[2 * blockIdx.x + 1];
  double *out = out_all + 5 * (size_t)blockIdx.x;
  int n = 0;
  const int c0 = (int)fmax(1.0, floor(x - r)), c1 = (int)fmin((double)W, ceil(x + r));
  const int r0 = (int)fmax(1.0, floor(y - r)), r1 = (int)fmin((double)H, ceil(y + r));
  for (int c = c0; c <= c1; ++c)
    for (int rr = r0; rr <= r1; ++rr) {
      const double dx = (double)c - x, dy = (double)rr - y;
      if (sqrt(dx * dx + dy * dy) < r && n < kFitMax) {
        px[n] = c; py[n] = rr; pz[n] = best[(size_t)(c - 1) * H + (rr - 1)]; wt[n] = 1.0; ++n;
      }
    }
  out[4] = n;
  if (n < 3) { out[0] = 0; out[1] = 0; out[2] = 1; out[3] = 0; return; }
  double cx = 0, cy = 0, cz = 0;
  for (int i = 0; i < n; ++i) { cx += px[i]; cy += py[i]; cz += pz[i]; }
  cx /= n; cy /= n; cz /= n;
  double v[3] = {0, 0, 1};
  const int rounds = kernel == 1 ? 20 : 1;
  for (int it = 0; it < rounds; ++it) {
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int i = 0; i < n; ++i) {
      const double w = wt[i], a = -(px[i] - cx) * w, b = -(py[i] - cy) * w, c = -(pz[i] - cz) * w;
      A[0][0] += a * a; A[0][1] += a * b; A[0][2] += a * c; A[1][1] += b * b; A[1][2] += b * c; A[2][2] += c * c;
    }
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
      const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
      if (off < 1e-300) break;
      for (int pp = 0; pp < 2; ++pp)
        for (int q = pp + 1; q < 3; ++q) {
          if (A[pp][q] == 0) continue;
          const double theta = (A[q][q] - A[pp][pp]) / (2 * A[pp][q]);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
          const double cs = 1 / sqrt(t * t + 1), sn = t * cs;
          for (int k = 0; k < 3; ++k) {  // A <- A J
            const double akp = A[k][pp], akq = A[k][q];
            A[k][pp] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq;
          }
          for (int k = 0; k < 3; ++k) {  // A <- J' A
            const double apk = A[pp][k], aqk = A[q][k];
            A[pp][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk;
          }
          for (int k = 0; k < 3; ++k) {
            const double vkp = V[k][pp], vkq = V[k][q];
            V[k][pp] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq;
          }
        }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    v[0] = V[0][m]; v[1] = V[1][m]; v[2] = V[2][m];
    if (kernel == 1)
      for (int i = 0; i < n; ++i)  // w = sqrt(abs(cost * V(:, end)))
        wt[i] = sqrt(fabs(-(px[i] - cx) * v[0] + -(py[i] - cy) * v[1] + -(pz[i] - cz) * v[2]));
  }
  const double p4 = -(v[0] * cx + v[1] * cy + v[2] * cz);
  out[0] = v[0] / v[2]; out[1] = v[1] / v[2]; out[2] = v[2] / v[2]; out[3] = p4 / v[2];
}

}  // namespace
}  // namespace stereo

using namespace stereo;

// ---------------------------------------------------------------- fusion context

struct stereo_fusion {
  int H = 0, W = 0, kernel = 1;
  int64_t N = 0, E = 0;
  double tol = 0, d_min = 0, d_step = 0;
  DevBuf<uint32_t> conn;
  DevBuf<double> points, weights, cur, prop, Ucur, U1, E00, E01, E10, E11, partial;
  DevBuf<uint8_t> take;
  stereo_rd_plan *rd = nullptr;
  stereo_trws_plan *trws = nullptr;  // simultaneous fusion: plan of the last label count
  int trws_K = 0;
  bool trws_mm = false;              // its node beliefs are kept (stereo_fusion_keep_min_marginals)
  DevBuf<double> props, unaryK, qK, qpK;
  DevBuf<int32_t> labels;
  std::vector<uint32_t> h_conn;
  std::vector<int32_t> h_label;
  // unary source: 1 = NCC volume (dispmap_ncc.m), 2 = photo-consistency (dispmap_globalstereo.m)
  int unary_kind = 0;
  DevBuf<double> ncc, disparities, im0, im1, P2;
  int D = 0, C = 0;
  double unary_weight = 0, dmin = 0, dmax = 0, col_thresh = 0;
  bool ascending = false;  // strictly ascending disparities: the sampler bisects instead of scanning
  DevBuf<double> best, plane_tab, fit_out;   // proposals built on the device: WTA disparities, 4 x S planes
  DevBuf<int32_t> segments;
  bool have_best = false, have_segments = false;
  bool have_assignment = false;
  double energy = 0;
  std::vector<double> h_lab;
  std::vector<uint8_t> h_take;
  ~stereo_fusion() {
    if (rd) stereo_rd_plan_destroy(rd);
    if (trws) stereo_trws_plan_destroy(trws);
  }
};

namespace {

// blocks of fusion_sum_kernel over n elements (0 for none)
int64_t sum_blocks(int64_t n) { return n > 0 ? (n + kTB * 8 - 1) / (kTB * 8) : 0; }

// block partials of x[0 .. n) into `partial` (sum_blocks(n) doubles); the caller copies back and adds them in order
void launch_partials(const double *x, int64_t n, double *partial) {
  if (const int64_t nb = sum_blocks(n)) hipLaunchKernelGGL(fusion_sum_kernel, dim3((unsigned)nb), dim3(kTB), 0, 0, x, n, partial);
}

void fusion_unary(stereo_fusion *F, const double *d_planes, double *d_out) {
  if (F->unary_kind == 1) {
    launch_ncc_unary(F->ncc.p, F->H, F->W, F->D, 0, F->disparities.p, F->dmin, F->dmax, F->unary_weight, d_planes, d_out,
                     F->ascending ? 1 : 0);
  } else if (F->unary_kind == 2) {
    launch_globalstereo_unary(F->im0.p, F->im1.p, F->H, F->W, F->C, F->P2.p, F->d_min, F->d_step, F->col_thresh, d_planes,
                              d_out);
  } else {
    throw std::runtime_error("Overload unary_cost");  // dispmap_super.m:200-203
  }
}

// dispmap_super.m:263-274 update_energy on the resident assignment
void fusion_update_energy(stereo_fusion *F) {
  launch_pairwise_terms(F->kernel, F->E, F->conn.p, F->points.p, F->cur.p, nullptr, F->weights.p, F->tol, F->d_min,
                        F->d_step, F->E00.p, F->E01.p, F->E10.p, F->E11.p);
  // both sums with one copy back: the unary's block partials, then the edges', each added in block order
  const int64_t nbN = sum_blocks(F->N), nbE = sum_blocks(F->E);
  if ((int64_t)F->partial.n < nbN + nbE) F->partial.alloc((size_t)(nbN + nbE));
  launch_partials(F->Ucur.p, F->N, F->partial.p);
  launch_partials(F->E00.p, F->E, F->partial.p + nbN);
  std::vector<double> h((size_t)(nbN + nbE));
  if (!h.empty()) STEREO_HIP_CHECK(hipMemcpy(h.data(), F->partial.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  double tu = 0, te = 0;
  for (int64_t i = 0; i < nbN; ++i) tu += h[i];
  for (int64_t i = 0; i < nbE; ++i) te += h[nbN + i];
  F->energy = tu + te;
}

}  // namespace

extern "C" {

int stereo_fusion_create(int H, int W, int kernel, double tol, int64_t E, const uint32_t *conn,
                         const double *weights, double d_min, double d_step, stereo_fusion **ctx, char *err,
                         size_t errcap) {
  if (!ctx) return fail("stereo_fusion_create: ctx is NULL", err, errcap);
  *ctx = nullptr;
  if (kernel != 1 && kernel != 2) return fail("Unkown kernel type", err, errcap);  // dispmap_super.m:233
  if (H < 1 || W < 1 || E < 0 || (E > 0 && (!conn || !weights))) return fail("stereo_fusion_create: bad argument", err, errcap);
  std::unique_ptr<stereo_fusion> F(new stereo_fusion);
  const int rc = guarded_sync("stereo_fusion_create", err, errcap, [&] {
    F->H = H; F->W = W; F->kernel = kernel; F->tol = tol; F->E = E; F->N = (int64_t)H * W;
    F->d_min = d_min; F->d_step = d_step;
    const int64_t N = F->N;
    std::vector<double> pts(2 * N);
    for (int64_t i = 0; i < N; ++i) { pts[2 * i] = (double)(i / H + 1); pts[2 * i + 1] = (double)(i % H + 1); }  // :275-278
    F->conn.upload(conn, 2 * E); F->weights.upload(weights, E); F->points.upload(pts.data(), 2 * N);
    F->h_conn.assign(conn, conn + 2 * E);
    F->cur.alloc(4 * N); F->prop.alloc(4 * N); F->Ucur.alloc(N); F->U1.alloc(N); F->take.alloc(N);
    F->E00.alloc(std::max<int64_t>(E, 1)); F->E01.alloc(std::max<int64_t>(E, 1));
    F->E10.alloc(std::max<int64_t>(E, 1)); F->E11.alloc(std::max<int64_t>(E, 1));
    F->h_lab.resize(N); F->h_take.resize(N);
    char e2[256] = {0};
    if (stereo_rd_plan_create(N, E, conn, &F->rd, e2, sizeof(e2)) != 0) throw std::runtime_error(e2);
    if (stereo_rd_plan_set_grid(F->rd, H, W, e2, sizeof(e2)) != 0) throw std::runtime_error(e2);
  });
  if (rc == 0) *ctx = F.release();
  return rc;
}

void stereo_fusion_destroy(stereo_fusion *ctx) { delete ctx; }

int stereo_fusion_unary_ncc(stereo_fusion *F, const double *ncc, int D, const double *disparities,
                            double unary_weight, char *err, size_t errcap) {
  if (!F || !ncc || !disparities || D < 1) return fail("stereo_fusion_unary_ncc: bad argument", err, errcap);
  return guarded_sync("stereo_fusion_unary_ncc", err, errcap, [&] {
    F->ncc.upload(ncc, (size_t)F->N * D); F->disparities.upload(disparities, D);
    F->D = D; F->unary_weight = unary_weight; F->unary_kind = 1;
    F->ascending = strictly_ascending(disparities, D);
    F->have_best = false;
    disparity_range(disparities, D, F->dmin, F->dmax);
    F->have_assignment = false;
  });
}

int stereo_fusion_unary_globalstereo(stereo_fusion *F, const double *im0, const double *im1, int C,
                                     const double *P2, double col_thresh, char *err, size_t errcap) {
  if (!F || !im0 || !im1 || !P2 || C < 1) return fail("stereo_fusion_unary_globalstereo: bad argument", err, errcap);
  return guarded_sync("stereo_fusion_unary_globalstereo", err, errcap, [&] {
    F->im0.upload(im0, (size_t)F->N * C); F->im1.upload(im1, (size_t)F->N * C); F->P2.upload(P2, 12);
    F->C = C; F->col_thresh = col_thresh; F->unary_kind = 2;
    F->have_assignment = false;
  });
}

int stereo_fusion_set_assignment(stereo_fusion *F, const double *assignment, double *energy, char *err,
                                 size_t errcap) {
  if (!F || !assignment) return fail("stereo_fusion_set_assignment: bad argument", err, errcap);
  return guarded_sync("stereo_fusion_set_assignment", err, errcap, [&] {
    check_planes(assignment, F->N);
    F->cur.upload(assignment, 4 * F->N);
    fusion_unary(F, F->cur.p, F->Ucur.p);
    fusion_update_energy(F);
    F->have_assignment = true;
    if (energy) *energy = F->energy;
  });
}

int stereo_fusion_get_assignment(stereo_fusion *F, double *assignment, double *energy, char *err, size_t errcap) {
  if (!F) return fail("stereo_fusion_get_assignment: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  return guarded_sync("stereo_fusion_get_assignment", err, errcap, [&] {
    if (assignment) download(assignment, F->cur, 4 * F->N);
    if (energy) *energy = F->energy;
  });
}

// the 4 x S plane table (+ segment ids) of a proposal -> 4 x N on the device
static void fusion_build_proposal(stereo_fusion *F, const double *planes, int S, const int32_t *segments, double *d_prop) {
  check_planes(planes, S);
  if (S > 1 && !segments && !F->have_segments) throw std::runtime_error("stereo_fusion: more than one plane needs segment ids");
  if (segments) { F->segments.upload(segments, F->N); F->have_segments = true; }
  F->plane_tab.upload(planes, (size_t)4 * S);
  hipLaunchKernelGGL(proposal_from_planes_kernel, dim3(blocks(F->N)), dim3(kTB), 0, 0, F->N, F->plane_tab.p, S,
                     S > 1 ? F->segments.p : (const int32_t *)nullptr, d_prop);
}

// one binary fusion move with the proposal already in F->prop
static void fusion_binary_core(stereo_fusion *F, int improve, double *energy, double *rd_energy, double *lower_bound,
                               double *num_unlabelled, double t_start) {
  const int64_t N = F->N, E = F->E;
  const bool verbose = std::getenv("STEREO_HIP_FUSION_VERBOSE") != nullptr;
  double t[6];
  t[0] = t_start;
  launch_pairwise_terms(F->kernel, E, F->conn.p, F->points.p, F->cur.p, F->prop.p, F->weights.p, F->tol, F->d_min, F->d_step,
                        F->E00.p, F->E01.p, F->E10.p, F->E11.p);
  fusion_unary(F, F->prop.p, F->U1.p);
  if (verbose) STEREO_HIP_CHECK(hipDeviceSynchronize());
  t[1] = wall_ms();
  double e = 0, lb = 0, unl = 0;
  char e2[256] = {0};
  if (stereo_rd_plan_solve_device(F->rd, F->Ucur.p, F->U1.p, F->E00.p, F->E01.p, F->E10.p, F->E11.p, improve,
                                  nullptr, &e, &lb, &unl, e2, sizeof(e2)) != 0)  // labels stay on the device
    throw std::runtime_error(e2);
  t[2] = wall_ms();
  hipLaunchKernelGGL(fusion_scatter_kernel, dim3(blocks(N)), dim3(kTB), 0, 0, N, stereo_rd_plan_device_labels(F->rd),
                     F->prop.p, F->U1.p, F->cur.p, F->Ucur.p);
  if (verbose) STEREO_HIP_CHECK(hipDeviceSynchronize());
  t[3] = wall_ms();
  fusion_update_energy(F);
  t[4] = wall_ms();
  if (verbose)
    std::fprintf(stderr, "[stereo_hip fusion] upload+terms %.2f ms, qpbo %.2f ms, scatter %.2f ms, energy %.2f ms\n",
                 t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3]);
  if (energy) *energy = F->energy;
  if (rd_energy) *rd_energy = e;
  if (lower_bound) *lower_bound = lb;
  if (num_unlabelled) *num_unlabelled = unl;
}

int stereo_fusion_binary(stereo_fusion *F, const double *proposal, int improve, double *energy,
                         double *rd_energy, double *lower_bound, double *num_unlabelled, char *err,
                         size_t errcap) {
  if (!F || !proposal) return fail("stereo_fusion_binary: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  return guarded_sync("stereo_fusion_binary", err, errcap, [&] {
    const double t0 = wall_ms();
    check_planes(proposal, F->N);
    F->prop.upload(proposal, 4 * F->N);
    fusion_binary_core(F, improve, energy, rd_energy, lower_bound, num_unlabelled, t0);
  });
}

int stereo_fusion_binary_planes(stereo_fusion *F, const double *planes, int S, const int32_t *segments, int improve,
                                double *energy, double *rd_energy, double *lower_bound, double *num_unlabelled,
                                char *err, size_t errcap) {
  if (!F || !planes || S < 1) return fail("stereo_fusion_binary_planes: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  return guarded_sync("stereo_fusion_binary_planes", err, errcap, [&] {
    const double t0 = wall_ms();
    fusion_build_proposal(F, planes, S, segments, F->prop.p);
    fusion_binary_core(F, improve, energy, rd_energy, lower_bound, num_unlabelled, t0);
  });
}

// binary_fuse_until_convergence (dispmap_super.m:85-152) as ONE call: the n proposals go to the device
// once (4 x N x n arrays, or a 4 x n table of single planes that are expanded there), the revisit
// schedule `ids` (1-based, what the reference builds from 1:n and its randi draws, with its
// `ids([diff(ids) == 0]) = 0` filter already applied by the caller) is walked here with the reference's
// loop -- the loop variable bumped inside the body, the exact `~=` on consecutive energies, the
// `visited` bookkeeping -- and every move runs on the resident state; nothing of size N crosses PCIe
// between moves and no interpreter sits between them.  energies: E(1) = energy before the first move,
// then one entry per move (at most cap; n_energies = length(E) = what the reference returns).
int stereo_fusion_fuse_until_convergence(stereo_fusion *F, const double *proposals, const double *planes, int n,
                                         const int64_t *ids, int64_t n_ids, int64_t maxiter, int improve,
                                         double *n_energies, double *energies, int64_t cap, char *err, size_t errcap) {
  if (!F || (!proposals && !planes) || n < 1 || !ids || n_ids < 0 || maxiter < 0)
    return fail("stereo_fusion_fuse_until_convergence: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  for (int64_t i = 0; i < n_ids; ++i)
    if (ids[i] < 1 || ids[i] > n) return fail("stereo_fusion_fuse_until_convergence: proposal id out of range", err, errcap);
  return guarded_sync("stereo_fusion_fuse_until_convergence", err, errcap, [&] {
    const int64_t N = F->N;
    // Where a move's proposal comes from: a single plane is expanded on the device when its move comes
    // (32 bytes of input, no storage); 4 x N arrays stay resident for the whole schedule only while all
    // n of them fit a budget (STEREO_HIP_FUSION_RESIDENT_MB, default 4096 MB and never more than a quarter
    // of the free device memory) -- beyond that each move uploads its own proposal from the caller's
    // buffer, as the per-move entry point does (a 3000 x 2000 image is 192 MB per proposal: a schedule
    // over a few dozen proposals must not need tens of GB up front).
    DevBuf<double> all;
    bool resident = false;
    if (proposals) {
      check_planes(proposals, N * n);
      size_t budget = (size_t)4096 << 20, free_b = 0, total_b = 0;
      if (const char *mb = std::getenv("STEREO_HIP_FUSION_RESIDENT_MB")) budget = (size_t)std::max(0L, std::atol(mb)) << 20;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 4);
      const size_t need = sizeof(double) * 4 * (size_t)N * (size_t)n;
      resident = need <= budget;
      if (resident) {
        all.alloc((size_t)4 * N * n);
        STEREO_HIP_CHECK(hipMemcpy(all.p, proposals, need, hipMemcpyHostToDevice));
      }
    } else {
      check_planes(planes, n);
    }
    std::vector<double> E(1, F->energy);
    std::vector<char> visited((size_t)n, 0);
    for (int64_t it = 1; it <= maxiter; ++it) {
      const int64_t it1 = it + 1;                    // iter = iter + 1 inside the for body (dispmap_super.m:108)
      if (it1 > n_ids) break;
      const int64_t pid = ids[it1 - 1];
      if (visited[pid - 1]) continue;
      if (!proposals) fusion_build_proposal(F, planes + 4 * (pid - 1), 1, nullptr, F->prop.p);
      else if (resident) STEREO_HIP_CHECK(hipMemcpyAsync(F->prop.p, all.p + (size_t)4 * N * (pid - 1), sizeof(double) * 4 * N, hipMemcpyDeviceToDevice, 0));
      else F->prop.upload(proposals + (size_t)4 * N * (pid - 1), 4 * N);
      fusion_binary_core(F, improve, nullptr, nullptr, nullptr, nullptr, wall_ms());
      E.push_back(F->energy);
      if (E[E.size() - 2] != E.back()) std::fill(visited.begin(), visited.end(), 0);   // E(end-1) ~= E(end)
      else visited[pid - 1] = 1;
      if (std::all_of(visited.begin(), visited.end(), [](char v) { return v != 0; })) break;
    }
    if (n_energies) *n_energies = (double)E.size();
    if (energies) for (int64_t i = 0; i < cap && i < (int64_t)E.size(); ++i) energies[i] = E[i];
  });
}

int stereo_fusion_fit_planes(stereo_fusion *F, const double *xs, const double *ys, int n, double r, double *planes,
                             double *npoints, char *err, size_t errcap) {
  if (!F || !planes || !xs || !ys || n < 1) return fail("stereo_fusion_fit_planes: bad argument", err, errcap);
  if (F->unary_kind != 1) return fail("stereo_fusion_fit_planes: needs the NCC volume (dispmap_ncc)", err, errcap);
  if (!(r > 0) || (2 * r + 3) * (2 * r + 3) > kFitMax) return fail("stereo_fusion_fit_planes: radius out of range", err, errcap);
  return guarded_sync("stereo_fusion_fit_planes", err, errcap, [&] {
    if (!F->have_best) {  // best_disp_from_ncc (dispmap_ncc.m:208-221), once per volume
      F->best.alloc(F->N);
      launch_ncc_best_disp(F->ncc.p, F->H, F->W, F->D, 0, F->disparities.p, F->best.p);
      F->have_best = true;
    }
    std::vector<double> xy(2 * (size_t)n), h(5 * (size_t)n);
    for (int i = 0; i < n; ++i) { xy[2 * i] = xs[i]; xy[2 * i + 1] = ys[i]; }
    DevBuf<double> d_xy;
    d_xy.upload(xy.data(), xy.size());
    if (F->fit_out.n < h.size()) F->fit_out.alloc(h.size());
    hipLaunchKernelGGL(fit_plane_kernel, dim3((unsigned)n), dim3(64), 0, 0, F->best.p, F->H, F->W, d_xy.p, r, F->kernel, F->fit_out.p);
    STEREO_HIP_CHECK(hipMemcpy(h.data(), F->fit_out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 4; ++k) planes[4 * i + k] = h[5 * i + k];
      if (npoints) npoints[i] = h[5 * i + 4];
    }
  });
}

int stereo_fusion_fit_plane(stereo_fusion *F, double x, double y, double r, double *plane, double *npoints, char *err,
                            size_t errcap) {
  return stereo_fusion_fit_planes(F, &x, &y, 1, r, plane, npoints, err, errcap);
}

// proposals: 4 x N x K host array, or NULL with plane_tab = 4 x K (one plane per proposal, built on the device)
static int fusion_simultaneous_impl(stereo_fusion *F, const double *proposals, const double *plane_tab, int K,
                                    double maxiter, double max_relgap, double *energy, double *trws_energy,
                                    double *lower_bound, double *iterations, char *err, size_t errcap) {
  return guarded_sync("stereo_fusion_simultaneous", err, errcap, [&] {
    const int64_t N = F->N, E = F->E;
    const int Kt = K + 1;  // proposals{end+1} = self.assignment (dispmap_super.m:160)
    const bool verbose = std::getenv("STEREO_HIP_FUSION_VERBOSE") != nullptr;
    const double t0 = wall_ms();
    if (proposals) check_planes(proposals, N * K); else check_planes(plane_tab, K);
    char e2[256] = {0};
    if (!F->trws || F->trws_K != Kt) {
      if (F->trws) { stereo_trws_plan_destroy(F->trws); F->trws = nullptr; }
      if (stereo_trws_plan_create(F->kernel, Kt, N, E, F->h_conn.data(), STEREO_TRWS_MESSAGES_EXACT, &F->trws, e2,
                                  sizeof(e2)) != 0)
        throw std::runtime_error(e2);
      F->trws_K = Kt;
      F->props.alloc((size_t)4 * N * Kt); F->unaryK.alloc((size_t)N * Kt);
      F->qK.alloc((size_t)std::max<int64_t>(E, 1) * Kt); F->qpK.alloc((size_t)std::max<int64_t>(E, 1) * Kt);
      F->labels.alloc(N); F->h_label.resize(N);
    }
    if (proposals) {
      STEREO_HIP_CHECK(hipMemcpy(F->props.p, proposals, sizeof(double) * 4 * N * K, hipMemcpyHostToDevice));
    } else {
      F->plane_tab.upload(plane_tab, (size_t)4 * K);
      for (int k = 0; k < K; ++k)
        hipLaunchKernelGGL(proposal_from_planes_kernel, dim3(blocks(N)), dim3(kTB), 0, 0, N, F->plane_tab.p + 4 * k, 1,
                           (const int32_t *)nullptr, F->props.p + (size_t)k * 4 * N);
    }
    STEREO_HIP_CHECK(hipMemcpy(F->props.p + (size_t)4 * N * K, F->cur.p, sizeof(double) * 4 * N, hipMemcpyDeviceToDevice));
    // unary (K x N, dispmap_super.m:164-172) and positions (:177-183) on the device
    for (int k = 0; k < Kt; ++k) {
      if (k < K) fusion_unary(F, F->props.p + (size_t)k * 4 * N, F->U1.p);
      hipLaunchKernelGGL(fusion_interleave_kernel, dim3(blocks(N)), dim3(kTB), 0, 0, N, Kt, k,
                         k < K ? F->U1.p : F->Ucur.p, F->unaryK.p);
    }
    if (E > 0)
      launch_trws_positions(E, Kt, N, F->conn.p, F->points.p, F->props.p, F->d_min, F->d_step, F->qK.p, F->qpK.p);
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    const double t1 = wall_ms();
    if (stereo_trws_plan_bind_device(F->trws, F->unaryK.p, F->qK.p, F->qpK.p, nullptr, F->weights.p, F->tol, e2,
                                     sizeof(e2)) != 0 ||
        stereo_trws_plan_reset(F->trws, e2, sizeof(e2)) != 0 ||
        stereo_trws_plan_keep_min_marginals(F->trws, F->trws_mm ? 1 : 0, e2, sizeof(e2)) != 0)
      throw std::runtime_error(e2);
    const double t2 = wall_ms();
    // Minimize_TRW_S runs at least one iteration and stops at iter >= iterMax (minimize.cpp:100-112)
    int iters = maxiter >= 1 ? (maxiter > 2e9 ? 2000000000 : (int)maxiter) : 1;
    int done = 0, stopped = 0;
    if (stereo_trws_plan_iterate(F->trws, iters, max_relgap, nullptr, &done, &stopped, e2, sizeof(e2)) != 0)
      throw std::runtime_error(e2);
    const double t3 = wall_ms();
    double te = 0, tlb = 0, tit = 0;
    if (stereo_trws_plan_result(F->trws, F->h_lab.data(), &te, &tlb, &tit, e2, sizeof(e2)) != 0)
      throw std::runtime_error(e2);
    for (int64_t i = 0; i < N; ++i) F->h_label[i] = (int32_t)F->h_lab[i] - 1;
    F->labels.upload(F->h_label.data(), N);
    hipLaunchKernelGGL(fusion_select_kernel, dim3(blocks(N)), dim3(kTB), 0, 0, N, Kt, F->labels.p, F->props.p,
                       F->unaryK.p, F->cur.p, F->Ucur.p);
    fusion_update_energy(F);
    if (energy) *energy = F->energy;
    if (verbose) {
      int64_t serial = 0;
      (void)stereo_trws_plan_counters(F->trws, &serial, 1);
      std::fprintf(stderr, "[stereo_hip fusion] simultaneous K=%d: plan + unary + positions %.1f ms, bind (argsort) %.1f ms, %d iterations %.1f ms (path %d, %lld serial-envelope messages), scatter + energy %.1f ms\n",
                   Kt, t1 - t0, t2 - t1, done, t3 - t2, stereo_trws_plan_path(F->trws), (long long)serial, wall_ms() - t3);
    }
    if (trws_energy) *trws_energy = te;
    if (lower_bound) *lower_bound = tlb;
    if (iterations) *iterations = tit;
  });
}

int stereo_fusion_simultaneous(stereo_fusion *F, const double *proposals, int K, double maxiter,
                               double max_relgap, double *energy, double *trws_energy, double *lower_bound,
                               double *iterations, char *err, size_t errcap) {
  if (!F || !proposals || K < 1) return fail("stereo_fusion_simultaneous: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  return fusion_simultaneous_impl(F, proposals, nullptr, K, maxiter, max_relgap, energy, trws_energy, lower_bound,
                                  iterations, err, errcap);
}

int stereo_fusion_keep_min_marginals(stereo_fusion *F, int on, char *err, size_t errcap) {
  if (!F) return fail("stereo_fusion_keep_min_marginals: NULL context", err, errcap);
  F->trws_mm = on != 0;
  return 0;
}

int stereo_fusion_trws_min_marginals(stereo_fusion *F, double *min_marginals, double *confidence, int32_t *argmin, char *err,
                                     size_t errcap) {
  if (!F) return fail("stereo_fusion_trws_min_marginals: NULL context", err, errcap);
  if (!F->trws || !F->trws_mm)
    return fail("stereo_fusion_trws_min_marginals: no simultaneous fusion has run with stereo_fusion_keep_min_marginals on",
                err, errcap);
  return stereo_trws_plan_min_marginals(F->trws, min_marginals, confidence, argmin, err, errcap);
}

int stereo_fusion_simultaneous_planes(stereo_fusion *F, const double *planes, int K, double maxiter, double max_relgap,
                                      double *energy, double *trws_energy, double *lower_bound, double *iterations,
                                      char *err, size_t errcap) {
  if (!F || !planes || K < 1) return fail("stereo_fusion_simultaneous_planes: bad argument", err, errcap);
  if (!F->have_assignment) return fail("stereo_fusion: no assignment set", err, errcap);
  return fusion_simultaneous_impl(F, nullptr, planes, K, maxiter, max_relgap, energy, trws_energy, lower_bound,
                                  iterations, err, errcap);
}

}  // extern "C"
