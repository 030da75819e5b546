// The speculative schedule of the long serial run (trws_graph.h: Sweep::Spec) for trws_wide_kernel:
// 64 < K <= 256 labels on shared uniformly spaced positions, linear kernel, even K.  Same protocol as trws_spec.h has for
// trws_pipe_kernel -- a RUNNER walks the cut run computing nothing but the recurrence that makes it serial, the segments
// recompute every visit with the certified routine side by side and commit in order after comparing what they started
// from with what the segment in front really handed over: a wrong row of the runner's costs a second walk, never a bit --
// with the runner's roles laid out for four chunks of 64 labels:
//   waves 0-3   messages: wave w holds labels 64 w .. 64 w + 63, one per lane.  Di from the staged prefix sum and the
//               row(s) node i - 1 handed over (in the wave's registers), H = gamma Di - m into a table in LDS, the four
//               waves meet once per message (arrival words in LDS; twice in the backward sweep, where Di loses its
//               minimum first), then windowed min-plus over +-8 table entries: ~110 instructions per wave and visit
//               where a visit of the certified routine is ~700 on its longest wave;
//   wave 4      labels of the primal pass, four per lane (the primal wave's operations);
//   waves 5-10  loaders: wave l stages the nodes i = l (mod 6) into ring slot l: descriptor, foreign flags, unary and
//               message rows, prefix sum in list order;
//   wave 11     publisher: at every cut the rows / label of the node in front go to p.spec_rows / p.spec_x, drained, then
//               the segment's flag done[N + s].
// The runner's LDS OVERLAYS the visit loops' (it is called at kernel entry, before they set anything up).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trws_dev.h"
#include "trws_spec.h"

#define WRLI(v, i) __builtin_amdgcn_readlane((v), (i))

namespace stereo {
namespace {

constexpr int kWrSlots = 6, kWrLoaders = 6, kWrMsg = 4;
constexpr int kWrK = 256;   // row stride (labels)
// a staged node: the slot layout of trws_spec.h in rows of kWrK doubles
constexpr int kWrRowP = 0, kWrRowS = kWrK, kWrRowM = 4 * kWrK, kWrRowTH = 6 * kWrK, kWrRowOUT = 7 * kWrK, kWrSc = 11 * kWrK;
constexpr int kWrSlotDoubles = kWrSc + 16;
constexpr int kWrTab = kWrSlots * kWrSlotDoubles;   // 2 tables of 16 + 256 + 16 doubles: H with +inf on both sides
constexpr int kWrTabDoubles = kWrK + 32;
constexpr int kWrPm = kWrTab + 2 * kWrTabDoubles;   // partial minima of the four waves: [2 tables][4] for min H, [2][4] for min Di
constexpr int kWrPub = kWrPm + 16;                  // 2 x (2 rows): what the publisher stores
constexpr int kWrWords = kWrPub + 4 * kWrK;         // 64 ints
constexpr int kWrPos = kWrWords + 32 + 32;          // (behind the words and the 64 words where lanes that have nothing to say store) the positions
constexpr int kWrDoubles = kWrPos + kWrK;
// words beyond trws_spec.h's: arrival of the four message waves: 40-43 | nodes consumed by message wave w: 48-51
constexpr int kWwArrive = 40, kWwConsM = 48;
constexpr int kWrAbortInt = 2 * (kWrWords + 31);   // (the last double of the words)

// ---- waves 0-3: the message recurrence, 64 labels each -----------------------------------------------------------------
struct WrNodeM {
  int sw;
  double sd, P, S0, S1, S2, M0, M1;
};
__device__ __forceinline__ void wr_request_m(const double *sl, int lane, int k, WrNodeM &n) {
  n.sw = ((const int *)(sl + kWrSc))[lane & 15];
  asm volatile("" ::: "memory");   // (LDS serves a wave's requests in order: rows behind a tag that was found are the node's)
  n.sd = sl[kWrSc + 8 + (lane & 7)];
  n.P = sl[kWrRowP + k]; n.S0 = sl[kWrRowS + k]; n.S1 = sl[kWrRowS + kWrK + k]; n.S2 = sl[kWrRowS + 2 * kWrK + k];
  n.M0 = sl[kWrRowM + k]; n.M1 = sl[kWrRowM + kWrK + k];
}
struct WrArgsM {
  int K, c0, c1;
  double lambda, step;
  int32_t *abort_flag;
  long long spin_ticks;
  unsigned long long *stat;
};

// The four waves meet: everybody's table entries and partial minimum are written, then read.  `seq` counts the meetings.
__device__ __forceinline__ bool wr_meet(int *rw, int wv, int lane, int seq, int *abort_word, const WrArgsM &a, int dir) {
  const long long t0_ = a.stat ? (long long)wall_clock64() : 0;
  SPEC_RELEASE();
  if (lane == 0) lds_store(rw + kWwArrive + wv, seq);
  const bool ok = run_wait_n<4>(rw + kWwArrive, seq, abort_word, a.abort_flag, a.spin_ticks);
  if (a.stat && wv == 0 && lane == 0) atomicAdd(a.stat + 16 + dir, (unsigned long long)((long long)wall_clock64() - t0_));
  return ok;
}

template <bool BACKWARD, int G>
__device__ __forceinline__ void wr_messages_g(const WrArgsM &a, double *rb, int lane, int wv, int *abort_word) {
  const double inf = __builtin_huge_val();
  const int k = wv * kWave + lane;   // this lane's label
  const bool act = k < a.K;
  int *rw = (int *)(rb + kWrWords);
  int *cons_word = lane == 0 ? rw + kWwConsM + wv : (int *)(rb + kWrWords + 32) + lane;   // (dummy words behind)
  double ad[4 * G];   // alpha |d step| of the window's index distances, for the weight seen last
#pragma unroll
  for (int d = 0; d < 4 * G; ++d) ad[d] = 0;
  double alpha_have = 0;
  double A0 = 0, A1 = 0;
  WrNodeM cur, nxt;
  wr_request_m(rb, lane, k, cur);
  nxt = cur;
  int slot_off = 0, seq = 0, tsel = 0, nsel = 0;
  for (int i = a.c0; i < a.c1; ++i) {
    if (__builtin_amdgcn_readlane(cur.sw, kRsTag) != i + 1) {   // (not there yet when it was asked for)
      const long long t0_ = (long long)wall_clock64();
      if (!__builtin_amdgcn_readfirstlane((int)run_wait((const int *)(rb + slot_off + kWrSc) + kRsTag, i + 1, abort_word, a.abort_flag, a.spin_ticks))) return;
      wr_request_m(rb + slot_off, lane, k, cur);
      if (a.stat && wv == 0 && lane == 0) { atomicAdd(a.stat + 3 + 2 * (BACKWARD ? 1 : 0), 1ull); atomicAdd(a.stat + 4 + 2 * (BACKWARD ? 1 : 0), (unsigned long long)((long long)wall_clock64() - t0_)); }
    }
    const int sw = cur.sw;
    const int key = __builtin_amdgcn_readlane(sw, kRsKinds), nmsg = __builtin_amdgcn_readlane(sw, kRsNmsg), cut = __builtin_amdgcn_readlane(sw, kRsCut);
    double Di = cur.P;
    // the tail of the node's list from the first handed-over row on, in list order (the order of the reference's additions)
    if (key == 0x20098) { Di += A0; Di += A1; }
    else if (key == 0x30908) { Di += A0; Di += cur.S0; Di += A1; }
    else if (key == 0x30098) { Di += A0; Di += A1; Di += cur.S0; }
    else if (key == 0x41908) { Di += A0; Di += cur.S0; Di += A1; Di += cur.S1; }
    else {
      const int nt = key >> 16;
      for (int t = 0; t < nt; ++t) {
        const int kd = (key >> (4 * t)) & 15;
        if (kd == 8) Di += A0; else if (kd == 9) Di += A1; else if (kd == 0) Di += cur.S0; else if (kd == 1) Di += cur.S1; else Di += cur.S2;
      }
    }
    const double sd = cur.sd, mold0 = cur.M0, mold1 = cur.M1;
    // this node's words and rows are in registers: its place in the ring is free for this wave, the next node's are asked for
    lds_store(cons_word, i + 1 - a.c0);
    slot_off += kWrSlotDoubles;
    if (slot_off == kWrSlots * kWrSlotDoubles) slot_off = 0;
    if (i + 1 < a.c1) wr_request_m(rb + slot_off, lane, k, nxt);
    double *pm = rb + kWrPm;
    if (BACKWARD) {   // minimize.cpp:79-83: the node's own lower-bound term leaves Di
      const double part = wave_min_dpp(act ? Di : inf);
      if (lane == 0) pm[8 + 4 * nsel + wv] = part;
      if (!wr_meet(rw, wv, lane, ++seq, abort_word, a, BACKWARD ? 1 : 0)) return;
      Di -= min_raw(min_raw(pm[8 + 4 * nsel], pm[8 + 4 * nsel + 1]), min_raw(pm[8 + 4 * nsel + 2], pm[8 + 4 * nsel + 3]));
      nsel ^= 1;   // (two sets of partial minima in turn, like the tables: nobody writes what a wave one meeting behind still reads)
    }
    const double gamma = readlane_f64(sd, 2);
    double R0 = 0, R1 = 0;
    for (int m = 0; m < nmsg; ++m) {
      const double alpha = readlane_f64(sd, m);
      const double h = gamma * Di - (m == 0 ? mold0 : mold1);   // (labels beyond K: the loader staged -inf as their old message: h = +inf)
      double out = 0;   // (alpha == 0: typeStereoLinear.h:390-396, a constant row, normalised)
      if (alpha != 0) {
        double *tabl = rb + kWrTab + tsel * kWrTabDoubles + 16 + k;
        *tabl = h;
        const double part = wave_min_dpp(h);
        if (lane == 0) pm[4 * tsel + wv] = part;
        if (__builtin_expect(alpha != alpha_have, 0)) {
#pragma unroll
          for (int d = 0; d < 4 * G; ++d) ad[d] = alpha * ((double)(d + 1) * a.step);
          alpha_have = alpha;
        }
        if (!wr_meet(rw, wv, lane, ++seq, abort_word, a, BACKWARD ? 1 : 0)) return;
        const double hmin = min_raw(min_raw(pm[4 * tsel], pm[4 * tsel + 1]), min_raw(pm[4 * tsel + 2], pm[4 * tsel + 3]));
        const double vtrunc = hmin + alpha * a.lambda;
        double lo[4 * G], hi[4 * G];
#pragma unroll
        for (int d = 0; d < 4 * G; ++d) { lo[d] = tabl[-(d + 1)]; hi[d] = tabl[d + 1]; }
        double ma = h, mb = vtrunc;   // (two chains)
#pragma unroll
        for (int d = 0; d < 4 * G; ++d) { ma = min_raw(ma, lo[d] + ad[d]); mb = min_raw(mb, hi[d] + ad[d]); }
        out = min_raw(ma, mb) - hmin;
        tsel ^= 1;   // (the other table next: a wave two meetings ahead of a reader cannot exist)
      }
      if (m == 0) R0 = out; else R1 = out;
    }
    A0 = R0; A1 = nmsg == 2 ? R1 : R0;
    if (cut) {
      // the rows the segment behind this node starts from: to the publisher
      const int ps = cut & 1;
      if (__builtin_amdgcn_readfirstlane(lds_load(rw + kSwFree)) < cut - 2 &&
          !__builtin_amdgcn_readfirstlane((int)run_wait(rw + kSwFree, cut - 2, abort_word, a.abort_flag, a.spin_ticks))) return;
      double *pb = rb + kWrPub + ps * 2 * kWrK;
      pb[k] = A0; pb[kWrK + k] = A1;
      if (wv == 0 && lane == 0) lds_store(rw + kSwKinds + ps, __builtin_amdgcn_readlane(sw, kRsPubKinds));
      SPEC_RELEASE();
      if (lane == 0) lds_store(rw + kSwPubM + 4 * ps + wv, cut);
    }
    cur = nxt;
  }
}

template <bool BACKWARD>
__device__ __attribute__((noinline)) void wr_messages(const DevParams *pp, int wv_) {
  extern __shared__ __attribute__((aligned(16))) double wr_lds[];
  constexpr int D = BACKWARD ? 1 : 0;
  WrArgsM a;
  a.K = uniform_value(pp->K); a.c0 = uniform_value(pp->spec_c0[D]); a.c1 = uniform_value(pp->spec_c1[D]);
  a.lambda = uniform_value(pp->lambda); a.step = uniform_value(pp->uniform_step);
  a.abort_flag = uniform_value(pp->abort_flag); a.spin_ticks = uniform_value(pp->spin_ticks); a.stat = uniform_value(pp->timeline) ? uniform_value(pp->spec_stat) : nullptr;   // (development counters: with STEREO_HIP_TRWS_TIMELINE only)
  const int window = uniform_value(pp->window);
  int *abort_word = (int *)wr_lds + kWrAbortInt;
  const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(wv_);
  if (window <= 4) wr_messages_g<BACKWARD, 1>(a, wr_lds, lane, wv, abort_word);
  else wr_messages_g<BACKWARD, 2>(a, wr_lds, lane, wv, abort_word);
}

// ---- wave 4: the labels of the primal pass (minimize.cpp:223-264, as the primal wave of a visit computes them) ------
template <bool BACKWARD>
__device__ __attribute__((noinline)) void wr_labels(const DevParams *pp_) {
  extern __shared__ __attribute__((aligned(16))) double wr_lds[];
  const DevParams p = uniform_params(pp_);
  double *rb = wr_lds;
  int *abort_word = (int *)wr_lds + kWrAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  const int c0 = p.spec_c0[BACKWARD ? 1 : 0], c1 = p.spec_c1[BACKWARD ? 1 : 0];
  const double inf = __builtin_huge_val();
  const int K = p.K;
  int *rw = (int *)(rb + kWrWords);
  double posk[4];
  bool act[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { act[c] = c * kWave + lane < K; posk[c] = act[c] ? p.pos[c * kWave + lane] : 0.0; }
  const double lambda = p.lambda;
  int xprev = 0;
  for (int i = c0; i < c1; ++i) {
    const double *sl = rb + ((i - c0) % kWrSlots) * kWrSlotDoubles;
    {
      const long long t0_ = (p.timeline && p.spec_stat) ? (long long)wall_clock64() : 0;
      if (!run_wait_i<false>((const int *)(sl + kWrSc) + kRsTag, i + 1, abort_word, p.abort_flag, p.spin_ticks)) return;
      if (p.timeline && p.spec_stat && lane == 0) atomicAdd(p.spec_stat + 18, (unsigned long long)((long long)wall_clock64() - t0_));
    }
    const int sw = ((const int *)(sl + kWrSc))[lane & 15];
    const double sd = sl[kWrSc + 8 + (lane & 7)];
    const int nout = __builtin_amdgcn_readlane(sw, kRsNout), nin = __builtin_amdgcn_readlane(sw, kRsNin), md = __builtin_amdgcn_readlane(sw, kRsMd),
              cut = __builtin_amdgcn_readlane(sw, kRsCut);
    double db[4], o[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      db[c] = act[c] ? sl[kWrRowTH + c * kWave + lane] : 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j][c] = sl[kWrRowOUT + j * kWrK + c * kWave + lane];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) lds_store(rw + kSwConsP, i + 1 - c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nin) {
        const int src = __builtin_amdgcn_readlane(sw, kRsSrc + j);
        const int ks = src < 0 ? xprev : src;
        const double pks = rb[kWrPos + ks];
        const double aj = readlane_f64(sd, 3 + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double d = ((md >> j) & 1) == 0 ? pks - posk[c] : posk[c] - pks;
          db[c] += aj * min_raw(fabs(d), lambda);
        }
      }
    }
    double di[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      di[c] = db[c];
      if (nout > 0) di[c] += o[0][c];
      if (nout > 1) di[c] += o[1][c];
      if (nout > 2) di[c] += o[2][c];
      if (nout > 3) di[c] += o[3][c];
      di[c] = act[c] ? di[c] : inf;
    }
    const double vbest = wave_min_dpp(min_raw(min_raw(di[0], di[1]), min_raw(di[2], di[3])));
    int bi = 0;
    bool found = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned long long hit = __builtin_amdgcn_ballot_w64(di[c] == vbest);
      if (!found && hit) { bi = c * kWave + __builtin_ctzll(hit); found = true; }
    }
    xprev = bi;
    if (cut) {
      const int ps = cut & 1;
      if (!run_wait(rw + kSwFree, cut - 2, abort_word, p.abort_flag, p.spin_ticks)) return;
      if (lane == 0) { rw[kSwLabel + ps] = xprev; rw[kSwNode + ps] = __builtin_amdgcn_readlane(sw, kRsNode); }
      SPEC_RELEASE();
      if (lane == 0) lds_store(rw + kSwPubP + ps, cut);
    }
  }
}

// ---- waves 5-10: staging -------------------------------------------------------------------------------------------------
template <bool BACKWARD, bool PRIMAL, bool UPDATE>
__device__ __attribute__((noinline)) void wr_loader(const DevParams *pp_, int epoch_, int lw_) {
  extern __shared__ __attribute__((aligned(16))) double wr_lds[];
  const DevParams p = uniform_params(pp_);
  double *rb = wr_lds;
  int *abort_word = (int *)wr_lds + kWrAbortInt;
  const int lane = threadIdx.x & (kWave - 1);
  const int epoch = __builtin_amdgcn_readfirstlane(epoch_), lw = __builtin_amdgcn_readfirstlane(lw_);
  constexpr int D = BACKWARD ? 1 : 0;
  const int c0 = p.spec_c0[D], c1 = p.spec_c1[D];
  constexpr int DW = TrwsGraph::kDescWords;
  const int32_t *desc = p.desc[D];
  const int K = p.K;
  int *rw = (int *)(rb + kWrWords);
  const int L = p.spec_len, nseg = p.spec_nseg;
  double *sl = rb + lw * kWrSlotDoubles;   // (six loaders, six slots: node i lives in slot i mod 6 = this wave's)
  // The node's own data -- unary row and its (up to four) outgoing rows, which nobody writes before the segment that holds
  // the node walks it -- is requested ONE TURN AHEAD (this wave's next node, six positions on) and waits in registers
  // while the current node is staged: a loader's turn used to be one memory round trip longer than the six visits it has.
  // (no load below is conditional on the lane: a label index beyond K reads label K - 1 again -- rows of such labels are
  //  never looked at --, so that the requests of a node go out back to back instead of one exec-mask region each)
  bool ok[4];
  int lk[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { ok[c] = c * kWave + lane < K; lk[c] = ok[c] ? c * kWave + lane : K - 1; }
  double theta_n[4] = {0, 0, 0, 0}, own_n[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) own_n[k][c] = 0;
#define WR_REQUEST_OWN(W)                                                                                                        \
  do {                                                                                                                         \
    const int nout_ = WRLI((W), 2) & 15;                                                                                       \
    const double *ua_ = p.unary + (size_t)((unsigned long long)(unsigned)WRLI((W), 0) * (unsigned long long)(unsigned)K);      \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) theta_n[c] = ua_[lk[c]];                                                     \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                            \
      if (k < nout_) {                                                                                                         \
        const double *mb_ = p.msg + (size_t)((unsigned long long)(unsigned)WRLI((W), 4 + k) * (unsigned long long)(unsigned)K); \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) own_n[k][c] = mb_[lk[c]];                                                \
      }                                                                                                                        \
    }                                                                                                                          \
  } while (0)
  int w2 = 0, wn2 = 0;
  if (c0 + lw < c1) { w2 = desc[(size_t)(c0 + lw) * DW + lane]; wn2 = c0 + lw + 1 < c1 ? desc[(size_t)(c0 + lw + 1) * DW + lane] : 0; WR_REQUEST_OWN(w2); }
  for (int i = c0 + lw; i < c1; i += kWrLoaders) {
    const long long tl0_ = (p.timeline && p.spec_stat && lw == 0) ? (long long)wall_clock64() : 0;
    const int w = w2, wn = wn2;
    double theta[4], r[8][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      theta[c] = theta_n[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k][c] = own_n[k][c];
#pragma unroll
      for (int k = 4; k < 8; ++k) r[k][c] = 0;
    }
    if (i + kWrLoaders < c1) {
      w2 = desc[(size_t)(i + kWrLoaders) * DW + lane];
      wn2 = i + kWrLoaders + 1 < c1 ? desc[(size_t)(i + kWrLoaders + 1) * DW + lane] : 0;
      WR_REQUEST_OWN(w2);
    }
    const int f = WRLI(w, 2), fn = WRLI(wn, 2);
    const int nout = f & 15, nin = (f >> 4) & 15, ndep = (f >> 8) & 15, md = (f >> 16) & 255, ntot = nout + nin;
    const int noutn = fn & 15, ntotn = noutn + ((fn >> 4) & 15);
    const int j8 = lane & 7;
    const int slw = __shfl(w, 12 + j8, kWave), sln = __shfl(wn, 12 + j8, kWave);
    // rows the node in front hands over (this node's and, for the messages to compute here, the next node's)
    const int fr = i > c0 ? (int)(__builtin_amdgcn_ballot_w64(lane < 8 && lane >= nout && lane < ntot && slw >= 0) & 255ull) : 0;
    const int frn = i + 1 < c1 ? (int)(__builtin_amdgcn_ballot_w64(lane < 8 && lane >= noutn && lane < ntotn && sln >= 0) & 255ull) : 0;
    const int kfirst = fr ? __builtin_ctz(fr) : ntot;
    int s0 = -1, s1 = -1;   // slots, in this node's outgoing list, of the (up to two distinct) messages the next node takes from it
    {
      int rest = frn;
      while (rest) {
        const int k = __builtin_ctz(rest);
        rest &= rest - 1;
        const int s = __builtin_amdgcn_readlane(wn, 12 + k);
        if (s0 < 0 || s0 == s) s0 = s; else s1 = s;
      }
    }
    int p0s = -1;
    if (fr) p0s = __builtin_amdgcn_readlane(w, 12 + kfirst);
    int kinds = 0, nt = 0, nstaged = 0, stage_of[4] = {-1, -1, -1, -1};
    for (int k = kfirst; k < ntot; ++k) {
      int kd;
      if ((fr >> k) & 1) kd = __builtin_amdgcn_readlane(w, 12 + k) == p0s ? 8 : 9;
      else { kd = nstaged; if (nstaged < 4) stage_of[nstaged] = k; ++nstaged; }
      kinds |= kd << (4 * nt);
      ++nt;
    }
    int cut = 0, pubkinds = 0;
    if (i + 1 < c1 && (i + 1 - c0) % L == 0 && (i + 1 - c0) / L < nseg) {
      cut = (i + 1 - c0) / L;
      for (int k = noutn; k < ntotn; ++k)
        if ((frn >> k) & 1) pubkinds |= (__builtin_amdgcn_readlane(wn, 12 + k) == s0 ? 8 : 9) << (4 * k);
    }
    // the node's own data (nobody writes it before the segment that holds the node walks it)
    const int fm = WRLI(w, kDescFetch) & 255;
    const double av = p.alpha[__shfl(w, 4 + j8, kWave)];
#pragma unroll
    for (int k = 4; k < 8; ++k) {   // (own rows five to eight: no node of a cut run has them; fetched here for completeness)
      if (k < nout) {
        const double *mb = p.msg + (size_t)((unsigned long long)(unsigned)WRLI(w, 4 + k) * (unsigned long long)(unsigned)K);
#pragma unroll
        for (int c = 0; c < 4; ++c) r[k][c] = mb[lk[c]];
      }
    }
    // foreign dependencies (everything but the node in front), then their rows and labels
    if (ndep > 0) wait_for_dependencies_w(p, ndep, __shfl(w, 20 + (lane & 3), kWave), WRLI(w, 1), epoch, lane, abort_word);
    if (lds_load(abort_word)) return;
    int src = -1;   // lane k < nin: the label the k-th incoming row's pairwise term takes (-1: the node in front)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k >= nout && k < ntot && ((fm >> k) & 1) && !((fr >> k) & 1)) {
        if (UPDATE) {
          const double *mb = p.msg + (size_t)((unsigned long long)(unsigned)WRLI(w, 4 + k) * (unsigned long long)(unsigned)K);
#pragma unroll
          for (int c = 0; c < 4; ++c) r[k][c] = ld_sc1(mb + lk[c]);
        }
        if (PRIMAL) { const int xv = ld_sc1(p.x + WRLI(w, 32 + k)); if (lane == k - nout) src = xv; }
      }
    }
    // the ring slot: all recurrences have taken the node that had it into their registers
    const int need = i - c0 - kWrSlots + 1;
    const long long tl1_ = (p.timeline && p.spec_stat && lw == 0) ? (long long)wall_clock64() : 0;
    if (UPDATE && need > 0 && !run_wait_n<4>(rw + kWwConsM, need, abort_word, p.abort_flag, p.spin_ticks)) return;
    if (PRIMAL && need > 0 && !run_wait_i<false>(rw + kSwConsP, need, abort_word, p.abort_flag, p.spin_ticks)) return;
    const long long tl2_ = (p.timeline && p.spec_stat && lw == 0) ? (long long)wall_clock64() : 0;
    // (a row picked by a uniform index: one scalar branch tree per row instead of a select per candidate and chunk)
#define WR_GET(KSEL, DST)                                                                         \
    do {                                                                                          \
      switch (KSEL) {                                                                             \
        case 0: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[0][c]; break;            \
        case 1: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[1][c]; break;            \
        case 2: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[2][c]; break;            \
        case 3: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[3][c]; break;            \
        case 4: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[4][c]; break;            \
        case 5: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[5][c]; break;            \
        case 6: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[6][c]; break;            \
        default: _Pragma("unroll") for (int c = 0; c < 4; ++c) DST[c] = r[7][c]; break;           \
      }                                                                                           \
    } while (0)
    double m0[4] = {0, 0, 0, 0}, m1[4] = {0, 0, 0, 0};
    if (UPDATE) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double P = theta[c];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < kfirst) P += r[k][c];
        sl[kWrRowP + c * kWave + lane] = P;
      }
      for (int t = 0; t < 3; ++t) {   // (staged rows of the tail: none on an ordinary node of the run)
        if (t < nstaged) {
          double v[4];
          WR_GET(stage_of[t], v);
#pragma unroll
          for (int c = 0; c < 4; ++c) sl[kWrRowS + t * kWrK + c * kWave + lane] = v[c];
        }
      }
      if (s0 >= 0) {   // (labels beyond K: -inf, which makes the recurrence's H = gamma Di - m = +inf there)
        WR_GET(s0, m0);
#pragma unroll
        for (int c = 0; c < 4; ++c) sl[kWrRowM + c * kWave + lane] = ok[c] ? m0[c] : -__builtin_huge_val();
      }
      if (s1 >= 0) {
        WR_GET(s1, m1);
#pragma unroll
        for (int c = 0; c < 4; ++c) sl[kWrRowM + kWrK + c * kWave + lane] = ok[c] ? m1[c] : -__builtin_huge_val();
      }
    }
    if (PRIMAL) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kk = c * kWave + lane;
        sl[kWrRowTH + kk] = theta[c];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nout) sl[kWrRowOUT + k * kWrK + kk] = r[k][c];
      }
    }
    // the two messages to the next node are ONE message if weights and old rows agree (positions are shared)
    int nmsg = s0 < 0 ? 0 : 1;
    if (UPDATE && s1 >= 0) {
      bool differ = false;
#pragma unroll
      for (int c = 0; c < 4; ++c) differ = differ | (ok[c] & (__double_as_longlong(m0[c]) != __double_as_longlong(m1[c])));
      const bool same = WRLI(__double2hiint(av), s0) == WRLI(__double2hiint(av), s1) && WRLI(__double2loint(av), s0) == WRLI(__double2loint(av), s1) && !UNI(differ);
      nmsg = same ? 1 : 2;
    }
#undef WR_GET
    {
      int word = 0;
      word = lane == kRsNt ? nt : lane == kRsKinds ? (kinds | (nt << 16)) : lane == kRsNmsg ? nmsg : lane == kRsCut ? cut
           : lane == kRsPubKinds ? pubkinds : lane == kRsNout ? nout : lane == kRsNin ? nin : lane == kRsMd ? (md >> nout) : lane == kRsNode ? WRLI(w, 0) : 0;
      const int srck = __shfl(src, lane - kRsSrc, kWave);
      if (lane >= kRsSrc && lane < kRsSrc + 4) word = srck;
      if (lane < kRsTag) ((int *)(sl + kWrSc))[lane] = word;
      const double a0 = readlane_f64(av, s0 < 0 ? 0 : s0), a1 = readlane_f64(av, s1 < 0 ? (s0 < 0 ? 0 : s0) : s1);
      const double ain = __shfl(av, nout + (lane - 3 < 0 ? 0 : lane - 3), kWave);
      const double g = (double)1 / (double)(nout > nin ? nout : nin > 0 ? nin : 1);
      if (lane < 8) sl[kWrSc + 8 + lane] = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? g : ain;
    }
    SPEC_RELEASE();
    if (lane == 0) lds_store((int *)(sl + kWrSc) + kRsTag, i + 1);
    if (p.timeline && p.spec_stat && lw == 0 && lane == 0) {
      const long long tl3_ = (long long)wall_clock64();
      atomicAdd(p.spec_stat + 21 + D, (unsigned long long)(tl1_ - tl0_)); atomicAdd(p.spec_stat + 19 + D, (unsigned long long)(tl2_ - tl1_));
      atomicAdd(p.spec_stat + 23 + D, (unsigned long long)(tl3_ - tl2_));
    }
  }
#undef WR_REQUEST_OWN
}

// the wide runner's layout and roles for chain_runner (trws_spec.h): waves 0-3 messages, wave 4 labels, waves 5-10
// loaders, wave 11 publisher; the positions go to LDS first
struct WideRunner {
  static constexpr int C = 4, kBase = 0, kAbortInt = kWrAbortInt, kSlots = kWrSlots, kSlotDoubles = kWrSlotDoubles, kSc = kWrSc,
                       kTab = kWrTab, kTabs = 2, kPub = kWrPub, kWords = kWrWords, kMsgWaves = kWrMsg, kLoaders = kWrLoaders;
  static constexpr bool kOverlay = true;
  static __device__ __forceinline__ void prepare(const DevParams &p, double *rb, int tid) {
    for (int k = tid; k < kWrK; k += (int)blockDim.x) rb[kWrPos + k] = k < p.K ? p.pos[k] : 0.0;
  }
  template <bool BACKWARD>
  static __device__ __forceinline__ void messages(const DevParams *pp, int wave) { wr_messages<BACKWARD>(pp, wave); }
  template <bool BACKWARD>
  static __device__ __forceinline__ void labels(const DevParams *pp) { wr_labels<BACKWARD>(pp); }
  template <bool BACKWARD, bool PRIMAL, bool UPDATE>
  static __device__ __forceinline__ void loader(const DevParams *pp, int epoch, int lw) { wr_loader<BACKWARD, PRIMAL, UPDATE>(pp, epoch, lw); }
};
static_assert(kWrTabDoubles == kWrK + 32, "chain_runner's table stride");

}  // namespace
}  // namespace stereo
