// The NCC cost volume (MI355X / gfx950) + its C ABI.
//
// Device version of
//   dispmap_ncc.m:116-198     5x5xRGB normalised cross-correlation volume
// One per-tap kernel for any patch and any disparities, and the staged kernels for integer disparities; which one
// runs, and on what grid, is decided by ncc_rule.h.  No contraction (-ffp-contract=off) so that + - * / match numpy.
#include <cstdlib>

#include "ncc_geometry.h"
#include "ncc_rule.h"
#include "terms_host.h"

namespace stereo {
namespace {

// ---- NCC volume -----------------------------------------------------------

struct NccParams {
  int H, W, D, r;
  const double *im0, *im1;  // H x W x 3 column major
  const double *disp;       // D
  double *out;
  int layout;               // 0: H x W x D (MATLAB), 1: D x N label fastest
};

// right image shifted by d (dispmap_ncc.m:145-154), zero outside the filled columns
__device__ __forceinline__ double shifted(const NccParams &p, int row, int col, int ch, double d, int c0, int n,
                                          double step) {
  if (row < 0 || row >= p.H || col < 0 || col >= p.W) return 0.0;  // conv2 'same' zero padding
  if (col + 1 < c0) return 0.0;
  const int i = col + 1 - c0;
  const double X = n > 1 ? 1.0 + i * step : 1.0;  // linspace(1, W-d, n)
  int x0 = (int)floor(X);
  if (x0 < 1) x0 = 1;
  if (p.W > 1 && x0 > p.W - 1) x0 = p.W - 1;
  const double t = X - x0;
  const double *plane = p.im1 + (size_t)ch * p.H * p.W;
  const double left = plane[(size_t)(x0 - 1) * p.H + row];
  if (t == 0) return left;
  const int xr = x0 < p.W - 1 ? x0 : p.W - 1;
  const double right = plane[(size_t)xr * p.H + row];
  return left * (1 - t) + right * t;
}

__device__ __forceinline__ double ref_px(const NccParams &p, int row, int col, int ch) {
  if (row < 0 || row >= p.H || col < 0 || col >= p.W) return 0.0;
  return p.im0[(size_t)ch * p.H * p.W + (size_t)col * p.H + row];
}

__global__ __launch_bounds__(kTB) void ncc_volume_kernel(NccParams p) {
  const int64_t t = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t Npx = (int64_t)p.H * p.W;
  if (t >= Npx * p.D) return;
  const int di = (int)(t / Npx);
  const int64_t px = t % Npx;
  const int row = (int)(px % p.H), col = (int)(px / p.H);
  const double d = p.disp[di];
  const int c0 = (int)ceil(d + 1);
  const int n = p.W - c0 + 1;
  const double step = n > 1 ? ((p.W - d) - 1.0) / (n - 1) : 0.0;
  const int r = p.r;
  const double npatch = (double)((2 * r + 1) * (2 * r + 1));
  const double mscale = 1.0 / npatch / 3.0;
  double bL[3] = {0, 0, 0}, bT[3] = {0, 0, 0}, bLL[3] = {0, 0, 0}, bTT[3] = {0, 0, 0}, bLT[3] = {0, 0, 0};
  for (int dx = -r; dx <= r; ++dx)
    for (int dy = -r; dy <= r; ++dy)
      for (int ch = 0; ch < 3; ++ch) {
        const double L = ref_px(p, row + dy, col + dx, ch);
        const double T = shifted(p, row + dy, col + dx, ch, d, c0, n, step);
        bL[ch] += L; bT[ch] += T; bLL[ch] += L * L; bTT[ch] += T * T; bLT[ch] += L * T;
      }
  const double meanL = (bL[0] * mscale + bL[1] * mscale) + bL[2] * mscale;
  const double meanT = (bT[0] * mscale + bT[1] * mscale) + bT[2] * mscale;
  const double t1L = (bLL[0] + bLL[1]) + bLL[2];
  const double t2L = (meanL * bL[0] + meanL * bL[1]) + meanL * bL[2];
  const double varL = t1L - 2 * t2L + npatch * 3 * meanL * meanL;
  const double u1 = (bTT[0] + bTT[1]) + bTT[2];
  const double u2 = (meanT * bT[0] + meanT * bT[1]) + meanT * bT[2];
  const double varT = u1 - 2 * u2 + npatch * 3 * meanT * meanT;
  const double c1 = (bLT[0] + bLT[1]) + bLT[2];
  const double c2 = (meanL * bT[0] + meanL * bT[1]) + meanL * bT[2];
  const double c3 = (meanT * bL[0] + meanT * bL[1]) + meanT * bL[2];
  const double num = c1 - c2 - c3 + npatch * 3 * meanT * meanL;
  // sqrt of a negative variance is imaginary in MATLAB; real(num/normL/normT) follows
  // (dispmap_ncc.m:141,171,188-192): one imaginary norm -> 0, both -> -num/(sL*sT)
  double val;
  const double sL = sqrt(fabs(varL)), sT = sqrt(fabs(varT));
  if (varL >= 0 && varT >= 0) val = num / sL / sT;
  else if (varL < 0 && varT < 0) val = -(num / sL / sT);
  else val = 0.0;
  if (!isfinite(val)) val = 0.0;
  const int cmask = (int)floor(d + 1 + 0.5);  // bnd_im(:, round(d+1):end) = 1, MATLAB round()
  if (col + 1 < cmask) val = 0.0;
  if (p.layout == 0) p.out[(size_t)di * Npx + px] = val;
  else p.out[(size_t)px * p.D + di] = val;
}

// ---- NCC volume, integer disparities: staged statistics + separable cross term ---------------
// With an integer disparity d the shifted image of dispmap_ncc.m:145-154 is a pure shift,
// imtr(row, col) = im1(row, col - d) (zero for col < d), so the d-independent box sums of im1 and
// im1^2 serve every slice: box5(imtr)(row, col) = box5(im1)(row, col - d) wherever the 5 x 5 window
// stays inside the image horizontally (the last `r` columns differ: conv2's zero padding cuts the
// window of imtr at column W, the one of im1 only at column W + d; they are summed directly).  One
// pre-pass per image stores per pixel the three per-channel box sums, the mean and the variance term
// (ncc_stats_kernel: 25 taps x 3 channels in the order of ncc_volume_kernel, d-independent).  What is
// left per (pixel, d) is the cross term sum_window sum_ch im0 * imtr -- a sliding-window sum with no
// contraction index shared between outputs (no MFMA) -- computed separably: lane = image row, a wave
// walks along the columns for one disparity with the five column products of the window in
// registers, the vertical five-tap sum comes from the neighbouring lanes (DPP wave shifts).  All
// image and statistics reads are coalesced 512-byte rows served by L2; the volume is written once,
// coalesced in both layouts (the label-fastest layout through an 8-disparity LDS transpose: 64-byte runs).
// Association: products (c0 + c1) + c2, then columns left to right, then rows top to bottom; the
// per-channel 25-tap order of the reference's conv2 is NOT kept for the cross term (agreement with
// the NumPy restatement to 1e-12 is the bar, tests/test_terms_gpu.py).
// (tile constants kNccRows / kNccWaves / kNccCols: ncc_geometry.h)

struct NccFast {
  int H, W, D;
  const double *im0, *im1;
  const double *st0, *st1;   // [5][N]: box sums of the three channels, mean, signed reciprocal norm
  const double *disp;
  double *out;
  int layout;
};

__global__ __launch_bounds__(kTB) void ncc_stats_kernel(const double *im, int H, int W, int r, double *st, double *stT = nullptr) {
  const int64_t px = (int64_t)blockIdx.x * kTB + threadIdx.x;
  const int64_t Npx = (int64_t)H * W;
  if (px >= Npx) return;
  const int row = (int)(px % H), col = (int)(px / H);
  const double npatch = (double)((2 * r + 1) * (2 * r + 1));
  const double mscale = 1.0 / npatch / 3.0;
  double b[3] = {0, 0, 0}, bb[3] = {0, 0, 0};
  for (int dx = -r; dx <= r; ++dx)
    for (int dy = -r; dy <= r; ++dy)
      for (int ch = 0; ch < 3; ++ch) {
        const int rr = row + dy, cc = col + dx;
        const double v = (rr < 0 || rr >= H || cc < 0 || cc >= W) ? 0.0 : im[(size_t)ch * Npx + (size_t)cc * H + rr];
        b[ch] += v; bb[ch] += v * v;
      }
  const double mean = (b[0] * mscale + b[1] * mscale) + b[2] * mscale;
  const double t1 = (bb[0] + bb[1]) + bb[2];
  const double t2 = (mean * b[0] + mean * b[1]) + mean * b[2];
  const double var = t1 - 2 * t2 + npatch * 3 * mean * mean;
  // the norm with the sign of the variance term: sqrt of a negative one is imaginary in MATLAB
  // (dispmap_ncc.m:141,171), which the cross kernel resolves from the two signs
  // (stored as the RECIPROCAL: the volume kernels multiply by it instead of dividing twice per output --
  //  a third of their instructions; the quotient moves by an ulp or two, the 1e-12 agreement with the
  //  NumPy restatement is unaffected.  A zero norm gives +-inf and, as with the division, a non-finite
  //  value that becomes 0, dispmap_ncc.m:190)
  const double rnorm = 1.0 / sqrt(fabs(var));
  if (st) {    // column-major planes (ncc_cross_kernel); the label-fastest path only wants the row-major ones
    st[px] = b[0]; st[Npx + px] = b[1]; st[2 * Npx + px] = b[2]; st[3 * Npx + px] = mean;
    st[4 * Npx + px] = var < 0 ? -rnorm : rnorm;
  }
  if (stT) {   // the same five planes row-major, for ncc_lane_kernel
    const int64_t t = (int64_t)row * W + col;
    stT[t] = b[0]; stT[Npx + t] = b[1]; stT[2 * Npx + t] = b[2]; stT[3 * Npx + t] = mean;
    stT[4 * Npx + t] = var < 0 ? -rnorm : rnorm;
  }
}

struct NccCol {  // what one step of the column walk reads: loaded one step ahead
  double l0, l1, l2, r0, r1, r2;          // the two pixels of the product two columns ahead
  double bL0, bL1, bL2, meanL, nL;        // statistics of im0 at (row, c)
  double bT0, bT1, bT2, meanT, nT;        // statistics of im1 at (row, c - d)
};

__device__ __forceinline__ void ncc_load(const NccFast &p, int64_t Npx, int row_c, int c, int d, NccCol &o) {
  // unconditional, clamped addresses (masked by the caller): every load of a step is in flight together
  const int H = p.H, W = p.W;
  int cp = c + 2; cp = cp < 0 ? 0 : cp > W - 1 ? W - 1 : cp;
  int cr = c + 2 - d; cr = cr < 0 ? 0 : cr > W - 1 ? W - 1 : cr;
  const size_t a = (size_t)cp * H + row_c, b = (size_t)cr * H + row_c;
  o.l0 = p.im0[a]; o.l1 = p.im0[Npx + a]; o.l2 = p.im0[2 * Npx + a];
  o.r0 = p.im1[b]; o.r1 = p.im1[Npx + b]; o.r2 = p.im1[2 * Npx + b];
  int cs = c < 0 ? 0 : c > W - 1 ? W - 1 : c;
  int ct = c - d; ct = ct < 0 ? 0 : ct > W - 1 ? W - 1 : ct;
  const size_t sa = (size_t)cs * H + row_c, sb = (size_t)ct * H + row_c;
  o.bL0 = p.st0[sa]; o.bL1 = p.st0[Npx + sa]; o.bL2 = p.st0[2 * Npx + sa]; o.meanL = p.st0[3 * Npx + sa]; o.nL = p.st0[4 * Npx + sa];
  o.bT0 = p.st1[sb]; o.bT1 = p.st1[Npx + sb]; o.bT2 = p.st1[2 * Npx + sb]; o.meanT = p.st1[3 * Npx + sb]; o.nT = p.st1[4 * Npx + sb];
}

// Statistics of the shifted image where the 5 x 5 window leaves the image on the right: its columns
// >= W are zero for imtr but not for im1, so the pre-pass planes do not apply (last two columns only).
// Out of line (arguments and result by value, in registers): inlined, its 75 unrolled taps cost the
// column walk a hundred VGPRs and half of its occupancy.
struct NccStat { double b0, b1, b2, mean, nrm; };
__device__ __attribute__((noinline)) NccStat ncc_right_border(const double *im1, int H, int W, int64_t Npx, int row, int c, int d) {
  double b0 = 0, b1 = 0, b2 = 0, q0 = 0, q1 = 0, q2 = 0;
#pragma unroll 1
  for (int dx = -2; dx <= 2; ++dx)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int rr = row + dy, cc = c + dx;
      const bool in = !(rr < 0 || rr >= H || cc < 0 || cc >= W || cc - d < 0);
      const size_t a = in ? (size_t)(cc - d) * H + rr : 0;
      const double v0 = in ? im1[a] : 0.0, v1 = in ? im1[Npx + a] : 0.0, v2 = in ? im1[2 * Npx + a] : 0.0;
      b0 += v0; q0 += v0 * v0; b1 += v1; q1 += v1 * v1; b2 += v2; q2 += v2 * v2;
    }
  const double mscale = 1.0 / 25.0 / 3.0;
  NccStat o;
  o.b0 = b0; o.b1 = b1; o.b2 = b2;
  o.mean = (b0 * mscale + b1 * mscale) + b2 * mscale;
  const double u1 = (q0 + q1) + q2;
  const double u2 = (o.mean * b0 + o.mean * b1) + o.mean * b2;
  const double varT = u1 - 2 * u2 + 75.0 * o.mean * o.mean;
  const double nn = 1.0 / sqrt(fabs(varT));   // signed reciprocal, as in the statistics planes
  o.nrm = varT < 0 ? -nn : nn;
  return o;
}

// value of the lane above (UP) / below in the wave of 64; the lane that falls off the end reads 0
// (DPP wave_shr:1 / wave_shl:1, bound_ctrl: one VALU move per half instead of a trip through LDS)
template <bool UP>
__device__ __forceinline__ double lane_neighbour(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, UP ? 0x138 : 0x130, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, UP ? 0x138 : 0x130, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kNccWaves * 64, 2) void ncc_cross_kernel(NccFast p) {
  __shared__ double tr[2][kNccRows][kNccWaves + 1];  // label-fastest transpose, double buffered
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = p.H, W = p.W;
  const int64_t Npx = (int64_t)H * W;
  const int row0 = blockIdx.x * kNccRows, row = row0 - 2 + lane;
  const int di = blockIdx.y * kNccWaves + wave;
  const bool dvalid = di < p.D;
  const int d = dvalid ? (int)p.disp[di] : 0;
  const int c_begin = blockIdx.z * kNccCols, c_end = c_begin + kNccCols < W ? c_begin + kNccCols : W;
  const bool rvalid = row >= 0 && row < H;
  const int row_c = row < 0 ? 0 : row > H - 1 ? H - 1 : row;
  const bool outlane = lane >= 2 && lane < 2 + kNccRows && row < H;
  const double npatch3 = 75.0;
  auto product = [&](int c, const NccCol &v) -> double {  // sum over the channels of im0(row, c) * imtr(row, c)
    const double pr = (v.l0 * v.r0 + v.l1 * v.r1) + v.l2 * v.r2;
    return (rvalid && dvalid && c >= 0 && c < W && c - d >= 0) ? pr : 0.0;
  };
  NccCol cur, nxt;
  double P0, P1, P2, P3;
  ncc_load(p, Npx, row_c, c_begin - 4, d, cur); P0 = product(c_begin - 2, cur);
  ncc_load(p, Npx, row_c, c_begin - 3, d, cur); P1 = product(c_begin - 1, cur);
  ncc_load(p, Npx, row_c, c_begin - 2, d, cur); P2 = product(c_begin, cur);
  ncc_load(p, Npx, row_c, c_begin - 1, d, cur); P3 = product(c_begin + 1, cur);
  ncc_load(p, Npx, row_c, c_begin, d, cur);
#pragma unroll 1
  for (int c = c_begin; c < c_end; ++c) {
    ncc_load(p, Npx, row_c, c + 1, d, nxt);  // the next step's loads travel while this one computes
    const double P4 = product(c + 2, cur);
    const double h = (((P0 + P1) + P2) + P3) + P4;
    const double hm1 = lane_neighbour<true>(h), hp1 = lane_neighbour<false>(h);      // rows - 1, + 1
    const double hm2 = lane_neighbour<true>(hm1), hp2 = lane_neighbour<false>(hp1);  // rows - 2, + 2
    const double c1 = (((hm2 + hm1) + h) + hp1) + hp2;
    P0 = P1; P1 = P2; P2 = P3; P3 = P4;
    double val = 0.0;
    const bool live = outlane && dvalid && c >= d;  // columns left of round(d + 1) are masked (dispmap_ncc.m:190-191)
    double bT0 = cur.bT0, bT1 = cur.bT1, bT2 = cur.bT2, meanT = cur.meanT, nT = cur.nT;
    if (c + 2 >= W && live) {
      const NccStat o = ncc_right_border(p.im1, H, W, Npx, row, c, d);
      bT0 = o.b0; bT1 = o.b1; bT2 = o.b2; meanT = o.mean; nT = o.nrm;
    }
    {
      const double c2 = (cur.meanL * bT0 + cur.meanL * bT1) + cur.meanL * bT2;
      const double c3 = (meanT * cur.bL0 + meanT * cur.bL1) + meanT * cur.bL2;
      const double num = c1 - c2 - c3 + npatch3 * meanT * cur.meanL;
      const double q = num * fabs(cur.nL) * fabs(nT);
      // real(num / normL / normT) with imaginary norms for negative variance terms (dispmap_ncc.m:188-192)
      const bool negL = cur.nL < 0, negT = nT < 0;
      val = negL == negT ? (negL ? -q : q) : 0.0;
      if (!isfinite(val) || !live) val = 0.0;
    }
    if (p.layout == 0) {
      if (outlane && dvalid) p.out[((size_t)di * W + c) * H + row] = val;
    } else {
      double (*buf)[kNccWaves + 1] = tr[(c - c_begin) & 1];
      if (lane >= 2 && lane < 2 + kNccRows) buf[lane - 2][wave] = val;
      __syncthreads();
      const int t = threadIdx.x;
      if (t < kNccRows * kNccWaves) {
        const int rr = t / kNccWaves, ww = t % kNccWaves;
        const int orow = row0 + rr, odi = blockIdx.y * kNccWaves + ww;
        if (orow < H && odi < p.D) p.out[((size_t)c * H + orow) * p.D + odi] = buf[rr][ww];
      }
    }
    cur = nxt;
  }
}

// ---- NCC volume, label-fastest layout: lane = disparity (round 3) ------------------------------
// ncc_cross_kernel above has lane = image row, which writes the MATLAB layout (H x W x D) in full rows
// but reaches the label-fastest layout TRW-S reads only through an LDS transpose with one workgroup
// barrier per column and 64-byte runs, re-fetching both images for every group of eight disparities
// (round 2: 151 us for 89 MB, 6 % of the write roofline, 3.8 x the algorithmic traffic).  Here a lane
// is a disparity: pixel (r, c) of the volume is ONE coalesced store of D doubles, the right image and
// its statistics are read as im1(r, c - d) from row-major copies (consecutive lanes, consecutive
// addresses), the left image and its statistics are the same for every lane (scalar loads), and both
// images are read once per 12-row tile for ALL disparities.  A workgroup is 16 waves = 16 image rows
// (12 output rows + the 2 + 2 rows the 5 x 5 window needs); a wave walks along its row keeping the
// window's five column products in registers, posts the horizontal sum in LDS and the 12 output waves
// add the five rows -- the same association as ncc_cross_kernel (products (c0 + c1) + c2, columns
// left to right, rows top to bottom), so both kernels give the same bits.
// (kNlWaves, kNlRows: ncc_geometry.h)

struct NccLane {
  int H, W, D;
  const double *im1;          // MATLAB layout (right-border statistics)
  const double *i0T, *i1T;    // [3][H][W]: row-major copies of the two images
  const double *s0T, *s1T;    // [5][H][W]: row-major statistics (ncc_stats_kernel)
  const double *disp;
  double *out;                // [W][H][D]
  int cols;                   // columns per workgroup
};

// row-major copy of an H x W x 3 image (MATLAB layout: [ch][col][row])
__global__ __launch_bounds__(kTB) void ncc_transpose_kernel(const double *im, int H, int W, double *out) {
  __shared__ double tile[16][17];
  const int64_t Npx = (int64_t)H * W;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int r0 = blockIdx.x * 16, c0 = blockIdx.y * 16, ch = blockIdx.z;
  if (r0 + tx < H && c0 + ty < W) tile[ty][tx] = im[(size_t)ch * Npx + (size_t)(c0 + ty) * H + r0 + tx];
  __syncthreads();
  if (r0 + ty < H && c0 + tx < W) out[(size_t)ch * Npx + (size_t)(r0 + ty) * W + c0 + tx] = tile[tx][ty];
}

// LDS of ncc_lane_kernel: per wave (= image row) the row segments it reads, staged once per workgroup --
// every load of a workgroup is in flight together, and the column walk itself touches LDS only:
//   seg1 [8][kNlSeg1]: im1 (3 channels) and its statistics (5 planes) at columns seg_c0 + x
//   seg0 [8][kNlSeg0]: im0 and its statistics at columns c_begin - 2 + x
// (kNlSeg1 = 96, kNlSeg0 = 36: ncc_geometry.h)
constexpr int kNlImDoubles = 3 * (kNlSeg1 + kNlSeg0);   // per wave: the two images' row segments
constexpr int kNlStDoubles = 5 * (kNlSeg1 + kNlSeg0);   // per OUTPUT wave: their statistics
constexpr int kNlLdsDoubles = kNlWaves * kNlImDoubles + kNlRows * kNlStDoubles + 4 * kNlWaves * 64;   // + two pairs of horizontal sums

__global__ __launch_bounds__(kNlWaves * 64) void ncc_lane_kernel(NccLane p) {
  extern __shared__ __attribute__((aligned(16))) double nl_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double *seg1 = nl_lds + wave * kNlImDoubles, *seg0 = seg1 + 3 * kNlSeg1;                 // images: [3][kNlSeg1], [3][kNlSeg0]
  const int ow = wave >= 2 && wave < 2 + kNlRows ? wave - 2 : 0;
  double *sts1 = nl_lds + kNlWaves * kNlImDoubles + ow * kNlStDoubles, *sts0 = sts1 + 5 * kNlSeg1;  // statistics: [5][..]
  double (*hbuf)[kNlWaves][64] = (double (*)[kNlWaves][64])(nl_lds + kNlWaves * kNlImDoubles + kNlRows * kNlStDoubles);   // [4][16][64]
  const int H = p.H, W = p.W;
  const int64_t Npx = (int64_t)H * W;
  const int row = blockIdx.x * kNlRows - 2 + wave;
  const int di = blockIdx.y * 64 + lane;
  const bool dvalid = di < p.D;
  const int d = dvalid ? (int)p.disp[di] : (int)p.disp[blockIdx.y * 64];
  // smallest / largest disparity of this 64-label chunk (the host checked that the segment holds the span)
  int dmin = d, dmax = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(dmin, o, 64), b2 = __shfl_xor(dmax, o, 64);
    dmin = a < dmin ? a : dmin; dmax = b2 > dmax ? b2 : dmax;
  }
  const int c_begin = blockIdx.z * p.cols, c_end = c_begin + p.cols < W ? c_begin + p.cols : W;
  const bool rvalid = row >= 0 && row < H;
  const int row_c = row < 0 ? 0 : row > H - 1 ? H - 1 : row;
  const size_t rowoff = (size_t)row_c * W;
  const bool outw = wave >= 2 && wave < 2 + kNlRows && row < H;   // (uniform) this wave writes a row of the volume
  const int seg_c0 = c_begin - 2 - dmax, seg0_c0 = c_begin - 2;
  // ---- stage the row segments (clamped columns: what lies outside the image is masked below)
  {
    double v1[8][2], v0[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double *src1 = (k < 3 ? p.i1T + (size_t)k * Npx : p.s1T + (size_t)(k - 3) * Npx) + rowoff;
      const double *src0 = (k < 3 ? p.i0T + (size_t)k * Npx : p.s0T + (size_t)(k - 3) * Npx) + rowoff;
      // (image planes: zero outside the image and in rows outside it, so that the products need no
      //  mask in the loop -- the shifted image is zero-filled, conv2 pads with zeros)
      const bool need = k < 3 || outw;   // (uniform) statistics only where a row of the volume is written
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        const int gg = seg_c0 + lane + 64 * hlf, g = gg < 0 ? 0 : gg > W - 1 ? W - 1 : gg;
        const double v = need ? src1[g] : 0.0;
        v1[k][hlf] = (k < 3 && (gg < 0 || gg > W - 1 || !rvalid)) ? 0.0 : v;
      }
      const int gg0 = seg0_c0 + lane, g0 = gg0 < 0 ? 0 : gg0 > W - 1 ? W - 1 : gg0;
      const double v = need ? src0[g0] : 0.0;
      v0[k] = (k < 3 && (gg0 < 0 || gg0 > W - 1 || !rvalid)) ? 0.0 : v;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k >= 3 && !outw) continue;
      double *d1 = k < 3 ? seg1 + k * kNlSeg1 : sts1 + (k - 3) * kNlSeg1;
      double *d0 = k < 3 ? seg0 + k * kNlSeg0 : sts0 + (k - 3) * kNlSeg0;
      d1[lane] = v1[k][0];
      if (lane + 64 < kNlSeg1) d1[lane + 64] = v1[k][1];
      if (lane < kNlSeg0) d0[lane] = v0[k];
    }
  }
  __syncthreads();
  const double npatch3 = 75.0;
  // sum over the channels of im0(row, c) * imtr(row, c), c = column of the product (indices are inside the
  // segments by construction; columns outside the image hold zeros)
  const double *s1d = seg1 - d - seg_c0;   // this lane's view of seg1: s1d[c] = plane 0 at column c - d
  const double *s0c = seg0 - seg0_c0;
  const double *t1d = sts1 - d - seg_c0, *t0c = sts0 - seg0_c0;   // the same views of the statistics
  auto product = [&](int c) -> double {
    const double l0 = s0c[c], l1 = s0c[kNlSeg0 + c], l2 = s0c[2 * kNlSeg0 + c];
    const double r0 = s1d[c], r1 = s1d[kNlSeg1 + c], r2 = s1d[2 * kNlSeg1 + c];
    return (l0 * r0 + l1 * r1) + l2 * r2;
  };
  double P0 = product(c_begin - 2), P1 = product(c_begin - 1), P2 = product(c_begin), P3 = product(c_begin + 1);
  // two columns per workgroup barrier (the horizontal sums of both are posted first)
  double *outp = p.out + ((size_t)c_begin * H + (row_c)) * p.D + di;   // this lane's element of pixel (row, c_begin)
  const size_t ostep = (size_t)H * p.D;
  auto emit = [&](int c, double h, const double (*hb)[64], double *dst) {
    const double hm2 = hb[wave - 2][lane], hm1 = hb[wave - 1][lane], hp1 = hb[wave + 1][lane], hp2 = hb[wave + 2][lane];
    const double bL0 = t0c[c], bL1 = t0c[kNlSeg0 + c], bL2 = t0c[2 * kNlSeg0 + c];
    const double meanL = t0c[3 * kNlSeg0 + c], nL = t0c[4 * kNlSeg0 + c];
    double bT0 = t1d[c], bT1 = t1d[kNlSeg1 + c], bT2 = t1d[2 * kNlSeg1 + c];
    double meanT = t1d[3 * kNlSeg1 + c], nT = t1d[4 * kNlSeg1 + c];
    const double c1 = (((hm2 + hm1) + h) + hp1) + hp2;
    const bool live = dvalid && c >= d;  // columns left of round(d + 1) are masked (dispmap_ncc.m:190-191)
    if (c + 2 >= W && live) {
      const NccStat o = ncc_right_border(p.im1, H, W, Npx, row, c, d);
      bT0 = o.b0; bT1 = o.b1; bT2 = o.b2; meanT = o.mean; nT = o.nrm;
    }
    const double c2 = (meanL * bT0 + meanL * bT1) + meanL * bT2;
    const double c3 = (meanT * bL0 + meanT * bL1) + meanT * bL2;
    const double num = c1 - c2 - c3 + npatch3 * meanT * meanL;
    const double q = num * fabs(nL) * fabs(nT);
    // real(num / normL / normT) with imaginary norms for negative variance terms (dispmap_ncc.m:188-192)
    const bool negL = nL < 0, negT = nT < 0;
    double val = negL == negT ? (negL ? -q : q) : 0.0;
    if (!isfinite(val) || !live) val = 0.0;
    if (dvalid) *dst = val;
  };
  int parity = 0;
#pragma unroll 1
  for (int c = c_begin; c < c_end; c += 2, parity ^= 1) {
    const double Pa = product(c + 2), Pb = product(c + 3);
    const double ha = (((P0 + P1) + P2) + P3) + Pa;
    const double hb2 = (((P1 + P2) + P3) + Pa) + Pb;
    P0 = P2; P1 = P3; P2 = Pa; P3 = Pb;
    double (*hA)[64] = hbuf[2 * parity], (*hB)[64] = hbuf[2 * parity + 1];
    hA[wave][lane] = ha; hB[wave][lane] = hb2;
    __syncthreads();   // (double buffered: the other pair is written by the next step, after every wave has read this one)
    if (outw) {
      emit(c, ha, hA, outp);
      if (c + 1 < c_end) emit(c + 1, hb2, hB, outp + ostep);
    }
    outp += 2 * ostep;
  }
}

// ---- the three paths: allocations and launches only (ncc_rule.h decides between them) ---------

void run_per_tap(const NccParams &p) {
  hipLaunchKernelGGL(ncc_volume_kernel, dim3(blocks((int64_t)p.H * p.W * p.D)), dim3(kTB), 0, 0, p);
}

// label-fastest volume: lane = disparity (ncc_lane_kernel) over row-major copies of images and statistics
void run_lanes(const NccParams &p, const NccChoice &c, int dev) {
  const int H = p.H, W = p.W, D = p.D;
  const size_t npx = (size_t)H * W;
  // (row-major staging copies only, in stream-ordered scratch: released behind the kernel without a
  //  device-wide synchronisation; the column-major statistics are the other path's)
  StreamBuf<double> s0T, s1T, i0T, i1T;
  s0T.alloc(5 * npx); s1T.alloc(5 * npx); i0T.alloc(3 * npx); i1T.alloc(3 * npx);
  const dim3 tg((H + 15) / 16, (W + 15) / 16, 3);
  hipLaunchKernelGGL(ncc_transpose_kernel, tg, dim3(kTB), 0, 0, p.im0, H, W, i0T.p);
  hipLaunchKernelGGL(ncc_transpose_kernel, tg, dim3(kTB), 0, 0, p.im1, H, W, i1T.p);
  hipLaunchKernelGGL(ncc_stats_kernel, dim3(blocks(npx)), dim3(kTB), 0, 0, p.im0, H, W, p.r, (double *)nullptr, s0T.p);
  hipLaunchKernelGGL(ncc_stats_kernel, dim3(blocks(npx)), dim3(kTB), 0, 0, p.im1, H, W, p.r, (double *)nullptr, s1T.p);
  const int rt = (H + kNlRows - 1) / kNlRows, dc = (D + 63) / 64;
  NccLane f{H, W, D, p.im1, i0T.p, i1T.p, s0T.p, s1T.p, p.disp, p.out, c.cols};
  const size_t lds = sizeof(double) * kNlLdsDoubles;
  static thread_local int lds_set_on = -1;   // the attribute is per device: set once per device and thread
  if (lds_set_on != dev) {
    STEREO_HIP_CHECK(hipFuncSetAttribute((const void *)ncc_lane_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set_on = dev;
  }
  hipLaunchKernelGGL(ncc_lane_kernel, dim3(rt, dc, c.chunks), dim3(kNlWaves * 64), lds, 0, f);
  STEREO_HIP_CHECK(hipGetLastError());
  // (the staging buffers are freed in stream order behind the kernel)
}

void run_cross(const NccParams &p) {
  const int H = p.H, W = p.W, D = p.D;
  const size_t npx = (size_t)H * W;
  DevBuf<double> st0, st1;
  st0.alloc(5 * npx); st1.alloc(5 * npx);
  hipLaunchKernelGGL(ncc_stats_kernel, dim3(blocks(npx)), dim3(kTB), 0, 0, p.im0, H, W, p.r, st0.p, (double *)nullptr);
  hipLaunchKernelGGL(ncc_stats_kernel, dim3(blocks(npx)), dim3(kTB), 0, 0, p.im1, H, W, p.r, st1.p, (double *)nullptr);
  NccFast f{H, W, D, p.im0, p.im1, st0.p, st1.p, p.disp, p.out, p.layout};
  const dim3 grid((H + kNccRows - 1) / kNccRows, (D + kNccWaves - 1) / kNccWaves, (W + kNccCols - 1) / kNccCols);
  hipLaunchKernelGGL(ncc_cross_kernel, grid, dim3(kNccWaves * 64), 0, 0, f);
  STEREO_HIP_CHECK(hipGetLastError());
  STEREO_HIP_CHECK(hipDeviceSynchronize());  // st0 / st1 are released on return
}

// NCC volume on the device: the staged kernels when every disparity is an integer in [0, W) and the
// patch is 5 x 5 (what dispmap_ncc.m:24 always asks for), the per-tap kernel otherwise.
void launch_ncc_volume(const double *d_im0, const double *d_im1, int H, int W, const double *h_disp,
                       const double *d_disp, int D, int patchsize, int layout, double *d_out) {
  int cus = 256, dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const NccChoice c = ncc_rule(H, W, h_disp, D, patchsize, layout, cus, std::getenv("STEREO_HIP_NCC_NAIVE") != nullptr,
                               std::getenv("STEREO_HIP_NCC_ROWLANES") != nullptr);
  const NccParams p{H, W, D, patchsize, d_im0, d_im1, d_disp, d_out, layout};
  switch (c.path) {
    case NccPath::PerTap: run_per_tap(p); break;
    case NccPath::Cross: run_cross(p); break;
    case NccPath::Lanes: run_lanes(p, c, dev); break;
  }
}

}  // namespace
}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_ncc_volume(const double *im0, const double *im1, int H, int W, const double *disparities, int D,
                      int patchsize, int layout, double *ncc, char *err, size_t errcap) {
  if (!im0 || !im1 || !disparities || !ncc || H < 1 || W < 1 || D < 1 || patchsize < 0 || (layout != 0 && layout != 1))
    return fail("stereo_ncc_volume: bad argument", err, errcap);
  return guarded_sync("stereo_ncc_volume", err, errcap, [&] {
    const size_t npx = (size_t)H * W;
    DevBuf<double> d0, d1, dd, out;
    d0.upload(im0, npx * 3); d1.upload(im1, npx * 3); dd.upload(disparities, D); out.alloc(npx * D);
    launch_ncc_volume(d0.p, d1.p, H, W, disparities, dd.p, D, patchsize, layout, out.p);
    download(ncc, out, npx * D);
  });
}

}  // extern "C"
