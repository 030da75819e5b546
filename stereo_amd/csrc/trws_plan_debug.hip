// TRW-S plan diagnostics: the timeline and profiler printouts, the development aids of the C ABI and the
// single-message entry stereo_trws_messages.  File map: trws_plan.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "trws_plan.h"

namespace stereo {

namespace {

// ---- single message updates (diagnostic entry point stereo_trws_messages) ------------------
// One wave per message through message_regs -- the routine the pipelined sweep kernel computes
// its messages with (certified fast path, second look, serial construction), table in LDS as
// there -- so that the certificate can be attacked with hand-placed near-tangent cones.
template <int KERNEL, bool SHAREDPOS>
__global__ __launch_bounds__(kWave) void trws_messages_kernel(DevParams p, int K, int64_t M, const double *Di,
                                                             const double *gamma, const double *msg_in,
                                                             const double *qsrc, const double *qdst,
                                                             const double *alpha, const uint16_t *perm, int window,
                                                             double *msg_out, double *vmin, int32_t *serial,
                                                             unsigned long long *counters) {
  __shared__ __attribute__((aligned(16))) double tab[kPipeTab];
  const int lane = threadIdx.x;
  const bool act = lane < K;
  if (lane < 2 * kPipePad) {
    double *e = tab + 4 * (lane < kPipePad ? lane : kWave + lane);
    e[0] = __builtin_huge_val(); e[1] = 0; e[2] = 0; e[3] = 0;
  }
  __syncthreads();
  for (int64_t m = blockIdx.x; m < M; m += gridDim.x) {
    const size_t o = (size_t)m * K + lane;
    const double h = act ? gamma[m] * Di[o] - msg_in[o] : __builtin_huge_val();
    const double qs = act ? qsrc[o] : 0.0, qt = act ? qdst[o] : 0.0;
    p.fallbacks = counters + blockIdx.x;  // (one counter per workgroup: its messages run one after the other)
    unsigned long long before = 0;
    if (lane == 0) before = *p.fallbacks;
    before = __shfl(before, 0, kWave);
    double out = 0;
    const double v = message_regs<KERNEL, SHAREDPOS>(p, K, alpha[m], h, qs, qt, perm + (size_t)m * K, out, lane,
                                                     tab + 4 * kPipePad, window);
    __threadfence();
    if (act) msg_out[o] = out;
    if (lane == 0) { vmin[m] = v; serial[m] = (int32_t)(*p.fallbacks - before); }
  }
}

}  // namespace

void print_timeline(const stereo_trws_plan *plan) {
  const bool chain = pipelined(plan->family);
  const bool spec = spec_active(plan);
  // (the stride of make_params: the runs the plan's own launches walk)
  const bool sub = own_sub_rows(plan, 0) || own_sub_rows(plan, 1);
  auto own_runs = [&](int d) {
    return own_sub_rows(plan, d) ? plan->graph->sweep[d].chunked.run_ptr.size() - 1 : plan->graph->sweep[d].chain_run_ptr.size() - 1;
  };
  const size_t R = spec ? std::max(own_spec(plan, 0).kind.size(), own_spec(plan, 1).kind.size())
                        : sub ? std::max(own_runs(0), own_runs(1))
                        : (chain ? plan->graph->sweep[0].chain_run_ptr.size() : plan->graph->sweep[0].run_ptr.size()) - 1;
  std::vector<unsigned long long> t(4 * (R + 1) + 8);
  if (hipMemcpy(t.data(), plan->d_timeline.p, sizeof(unsigned long long) * (4 * R + 4), hipMemcpyDeviceToHost) == hipSuccess) {
    // (STEREO_HIP_TRWS_TIMELINE=first, trws_plan.hip: launch_persistent -- direction 0's run stamps are the first forward
    //  launch's, but the runner stamps through the plan's own parameter block, in every launch: its line would set the
    //  first launch's segments against the last launch's runner)
    const char *tl = std::getenv("STEREO_HIP_TRWS_TIMELINE");
    const bool first = tl && std::strcmp(tl, "first") == 0;
    if (first)
      std::fprintf(stderr, "[stereo_hip timeline] dir 0: the plan's FIRST forward launch (no primal pass); its runner line is left out (the runner's "
                           "stamps are the last launch's)\n");
    if (spec)
      for (int d = first ? 1 : 0; d < 2; ++d) {
        const auto &sp = own_spec(plan, d);
        const unsigned long long t0 = t[(2 * R + d) * 2];
        std::fprintf(stderr, "[stereo_hip timeline] dir %d speculative: runner %.0f us; segments (us since the runner started, start..commit): ", d,
                     (t[(2 * R + d) * 2 + 1] - t0) / 100.0);
        for (int q = 0; q < sp.nseg; q += std::max(1, sp.nseg / 8))
          std::fprintf(stderr, "seg%d[%.0f..%.0f] ", q, ((double)t[((size_t)d * R + sp.run + q) * 2] - (double)t0) / 100.0,
                       ((double)t[((size_t)d * R + sp.run + q) * 2 + 1] - (double)t0) / 100.0);
        std::fprintf(stderr, "last[..%.0f]\n", ((double)t[((size_t)d * R + sp.run + sp.nseg - 1) * 2 + 1] - (double)t0) / 100.0);
      }
    // sub-row runs: the whole rows once more (runs of the chain schedule, its numbers) -- first start .. last end of a row's pieces
    for (int d = 0; d < 2; ++d) {
      if (!own_sub_rows(plan, d)) continue;
      const TrwsGraph::Sweep &S = plan->graph->sweep[d];
      const std::vector<int32_t> &rp = spec ? S.chunked.spec.run_ptr : S.chunked.run_ptr;
      const size_t RW = S.chain_run_ptr.size() - 1, step = (RW + (spec ? S.spec.nseg - 1 : 0)) / 12 + 1;
      const unsigned long long t0 = t[(size_t)d * R * 2];
      std::fprintf(stderr, "[stereo_hip timeline] dir %d whole rows (us since run 0 start): ", d);
      for (size_t k = 8; k < RW; k += step) {
        double lo = 1e300, hi = -1e300;
        for (size_t j = 0; j + 1 < rp.size(); ++j)
          if (rp[j] >= S.chain_run_ptr[k] && rp[j] < S.chain_run_ptr[k + 1]) {
            lo = std::min(lo, ((double)t[(d * R + j) * 2] - (double)t0) / 100.0);
            hi = std::max(hi, ((double)t[(d * R + j) * 2 + 1] - (double)t0) / 100.0);
          }
        std::fprintf(stderr, "row%zu[%.0f..%.0f] ", k, lo, hi);
      }
      std::fprintf(stderr, "\n");
    }
    for (int d = 0; d < 2; ++d) {
      const unsigned long long t0 = t[(size_t)d * R * 2];
      std::fprintf(stderr, "[stereo_hip timeline] dir %d (us since run 0 start): ", d);
      for (size_t r = 0; r < R; r += (r < 8 ? 1 : R / 12 + 1))
        std::fprintf(stderr, "run%zu[%.0f..%.0f] ", r, (t[(d * R + r) * 2] - t0) / 100.0, (t[(d * R + r) * 2 + 1] - t0) / 100.0);
      std::fprintf(stderr, "last[%.0f..%.0f]\n", (t[(d * R + R - 1) * 2] - t0) / 100.0, (t[(d * R + R - 1) * 2 + 1] - t0) / 100.0);
    }
  }
}

void print_profile(const stereo_trws_plan *plan) {
  const bool wide = plan->family == TrwsFamily::Wide;
  unsigned long long v[64];
  if (hipMemcpy(v, plan->d_prof.p, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) {
    if (!wide)
      std::fprintf(stderr, "[stereo_hip prof] cycles: p0 %llu p1 %llu p2 %llu p3 %llu p4 %llu | p5 %llu steps %llu\n",
                   v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
    if (!wide && v[6]) {
      std::fprintf(stderr, "[stereo_hip prof] cycles from barrier to barrier arrival per visit, per wave:");
      for (int i = 0; i < 12; ++i) std::fprintf(stderr, " %.0f", (double)v[32 + i] / v[6]);
      std::fprintf(stderr, "\n");
      if (v[48] | v[49] | v[50])  // -DSTEREO_HIP_VISIT_PROFILE
        std::fprintf(stderr, "[stereo_hip prof] wave 0 per visit: stage words %.0f | Di %.0f | H, positions %.0f | message %.0f | "
                             "hand-over %.0f | barrier %.0f\n", (double)v[48] / v[6], (double)v[49] / v[6], (double)v[50] / v[6],
                     (double)v[51] / v[6], (double)v[52] / v[6], (double)v[53] / v[6]);
      if ((v[48] | v[49] | v[50]) && v[19] && v[22])
        std::fprintf(stderr, "[stereo_hip prof] loader (steady state, per visit): until it polls %.0f | flags %.0f | fetch + stage %.0f; "
                             "storer: until the drain %.0f | drain %.0f\n", (double)v[16] / v[19], (double)v[17] / v[19],
                     (double)v[18] / v[19], (double)v[20] / v[22], (double)v[21] / v[22]);
      if (v[48] | v[49] | v[50])
        std::fprintf(stderr, "[stereo_hip prof] of the message: reduction + table %.0f | pair loop / flat path %.0f | margins + second look "
                             "%.0f | serial construction + walk %.0f | minimum %.0f\n", (double)v[56] / v[6], (double)v[57] / v[6],
                     (double)v[58] / v[6], (double)v[59] / v[6], (double)v[60] / v[6]);
    }
    if (!wide && (v[56] | v[57] | v[58] | v[59]) && !(v[48] | v[49] | v[50]))
      std::fprintf(stderr, "[stereo_hip prof messages] useful sources per message: <= 8: %llu, <= 16: %llu, <= 32: %llu, more (flat path): %llu\n", v[56], v[57], v[58], v[59]);
    if (!wide && v[9])
      std::fprintf(stderr, "[stereo_hip prof messages] certified attempt %.0f cycles x %llu | second look %.0f x %llu | "
                           "serial construction %.0f x %llu | walk %.0f x %llu\n",
                   (double)v[8] / v[9], v[9], v[11] ? (double)v[10] / v[11] : 0.0, v[11], v[13] ? (double)v[12] / v[13] : 0.0,
                   v[13], v[15] ? (double)v[14] / v[15] : 0.0, v[15]);
    if (!wide && v[17])
      std::fprintf(stderr, "[stereo_hip prof closed form] thresholds %.0f cycles | rows %.0f | scan + fixed point %.0f | slots + fill %.0f | "
                           "x %llu, extra rounds %.2f (%.2f with late tests), pushed %.1f, rows computed %.1f, top-segment check failed %llu, "
                           "up-front tests %.0f cycles, rounds %.0f cycles\n",
                   (double)v[16] / v[17], v[19] ? (double)v[18] / v[19] : 0.0, v[21] ? (double)v[20] / v[21] : 0.0,
                   v[23] ? (double)v[22] / v[23] : 0.0, v[17], v[21] ? (double)v[24] / v[21] : 0.0, v[21] ? (double)v[28] / v[21] : 0.0,
                   v[21] ? (double)v[26] / v[21] : 0.0, v[21] ? (double)v[27] / v[21] : 0.0, v[25],
                   v[21] ? (double)v[29] / v[21] : 0.0, v[21] ? (double)v[30] / v[21] : 0.0);
    if (wide && v[22]) {
      std::fprintf(stderr, "[stereo_hip prof wide] cycles per visit of wave 0:");
      for (int i = 0; i < 16; ++i) std::fprintf(stderr, " [%d] %.0f", i, (double)v[i] / v[22]);
      std::fprintf(stderr, " | loader A %.0f B %.0f storer %.0f primal %.0f | hw barrier wait %.0f | visits %llu\n",
                   (double)v[16] / v[22], (double)v[17] / v[22], (double)v[18] / v[22], (double)v[19] / v[22],
                   (double)v[21] / v[22], v[22]);
      std::fprintf(stderr, "[stereo_hip prof wide] cycles from barrier to barrier arrival, per wave:");
      for (int i = 0; i < 16; ++i) std::fprintf(stderr, " %.0f", (double)v[32 + i] / v[22]);
      if (v[28] | v[29])
        std::fprintf(stderr, "\n[stereo_hip prof wide] loader B: request inside the node's own visit %.0f cycles x %llu | staging (incl. wait for "
                             "parked loads) %.0f per visit | request two visits ahead %.0f x %llu",
                     v[28] ? (double)v[24] / v[28] : 0.0, v[28], (double)v[25] / v[22], v[29] ? (double)v[26] / v[29] : 0.0, v[29]);
      std::fprintf(stderr, "\n[stereo_hip prof wide] visits with more than 8000 cycles to the barrier, per wave:");
      for (int i = 0; i < 12; ++i) std::fprintf(stderr, " %llu", v[48 + i]);
      std::fprintf(stderr, "\n");
    }
  }
}

}  // namespace stereo

using namespace stereo;

extern "C" {

int stereo_trws_plan_debug_flags(stereo_trws_plan *P, int32_t *done, int32_t *ctl) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return 1;
  if (done && P->layout) {  // per global rank, like a plan of the whole problem (0 where the strip holds nothing)
    std::vector<int32_t> f(P->Nl);
    if (hipMemcpy(f.data(), P->d_done.p, sizeof(int32_t) * P->Nl, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    std::fill(done, done + P->N, 0);
    for (int64_t i = 0; i < P->Nl; ++i) done[P->graph->rank[P->layout->nodes[i]]] = f[i];
  } else
  if (done && hipMemcpy(done, P->d_done.p, sizeof(int32_t) * P->N, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (ctl && hipMemcpy(ctl, P->d_ctl.p, sizeof(int32_t) * 2, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return 0;
}

// Development aids: the lower-bound terms of the last backward sweep in the order the host sums them (rank N - 1 down to
// 0: the node's own term, then one per message it sent), and the message rows as they lie in HBM (E x K, edge-major).
int stereo_trws_plan_debug_terms(stereo_trws_plan *P, double *lb_terms, int64_t cap, int64_t *n_lb) {
  if (!P) return 1;
  if (n_lb) *n_lb = P->n_lb;
  if (lb_terms) std::memcpy(lb_terms, P->h_lb.p, sizeof(double) * (size_t)std::min<int64_t>(cap, P->n_lb));
  return 0;
}
int stereo_trws_plan_debug_messages(stereo_trws_plan *P, double *out, int64_t count) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P || !out) return 1;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  const int64_t n = std::min<int64_t>(count, (int64_t)P->d_msg.n);
  return hipMemcpy(out, P->d_msg.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}

int stereo_trws_plan_stats(stereo_trws_plan *P, double *sweep_ms, int64_t *sweep_launches, int reset) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return 1;
  if (sweep_ms) *sweep_ms = P->sweep_ms;
  if (sweep_launches) *sweep_launches = P->sweep_launches;
  if (reset) { P->sweep_ms = 0; P->sweep_launches = 0; }
  P->time_sweeps = true;
  return 0;
}

int stereo_trws_plan_counters(stereo_trws_plan *P, int64_t *serial_messages, int reset) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P) return 1;
  unsigned long long v = 0;
  if (P->bwd_pending) {
    // a backward sweep no iteration has taken yet (trws_plan.h) does not show: the count from before it; a reset leaves
    // the device with what that sweep adds
    v = P->h_held.p[0];
    if (reset) {
      unsigned long long now = 0;
      if (hipStreamSynchronize(P->issue_stream) != hipSuccess) return 1;
      if (hipMemcpy(&now, P->d_fallbacks.p, sizeof(now), hipMemcpyDeviceToHost) != hipSuccess) return 1;
      now -= v;
      if (hipMemcpy(P->d_fallbacks.p, &now, sizeof(now), hipMemcpyHostToDevice) != hipSuccess) return 1;
      P->h_held.p[0] = 0;
    }
    if (serial_messages) *serial_messages = (int64_t)v;
    return 0;
  }
  if (hipMemcpy(&v, P->d_fallbacks.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (serial_messages) *serial_messages = (int64_t)v;
  if (reset && hipMemset(P->d_fallbacks.p, 0, sizeof(v)) != hipSuccess) return 1;
  return 0;
}

int stereo_trws_plan_spec_stats(stereo_trws_plan *P, int64_t out[4]) {
  DeviceScope device_scope_(P ? P->device : -1);
  if (!P || !out) return 1;
  out[0] = spec_active(P) ? 1 : 0; out[1] = out[2] = out[3] = 0;
  if (P->d_spec_stat.p) {
    unsigned long long v[32] = {0};
    if (hipMemcpy(v, P->d_spec_stat.p, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (P->bwd_pending) std::memcpy(v, P->h_held.p + 1, sizeof(v));   // (as they read before the sweep no iteration has taken yet)
    if (std::getenv("STEREO_HIP_TRWS_TIMELINE"))
      std::fprintf(stderr, "[stereo_hip spec] last sweeps, roles done after (us): forward messages %.0f labels %.0f last loader %.0f publisher %.0f | backward messages %.0f "
                           "last loader %.0f publisher %.0f\n", v[8] / 100.0, v[9] / 100.0, v[10] / 100.0, v[11] / 100.0, v[12] / 100.0, v[14] / 100.0, v[15] / 100.0);
    if (false && v[8] && v[2])   // (-DSTEREO_HIP_RUNNER_PROFILE)
      std::fprintf(stderr, "[stereo_hip spec] message recurrence, cycles per visit: loop top %.0f | node in registers (incl. waits) %.0f | Di, next node asked for %.0f | "
                           "H, table, min H %.0f | window + row %.0f | publish, turn %.0f\n", (double)v[13] / v[2], (double)v[8] / v[2], (double)v[9] / v[2],
                   (double)v[10] / v[2], (double)v[11] / v[2], (double)v[12] / v[2]);
    out[1] = (int64_t)v[0]; out[2] = (int64_t)v[1]; out[3] = (int64_t)v[2];
    if (std::getenv("STEREO_HIP_TRWS_TIMELINE") && (v[16] || v[17]))   // (development, wide runner: where its roles wait, us in all)
      std::fprintf(stderr, "[stereo_hip spec] wide runner, us in all launches: meetings of the message waves forward %.0f backward %.0f | label wave waiting for its node %.0f | "
                           "loader 0: until the slot wait forward %.0f backward %.0f, slot wait %.0f / %.0f, staging %.0f / %.0f\n", v[16] / 100.0, v[17] / 100.0, v[18] / 100.0,
                   v[21] / 100.0, v[22] / 100.0, v[19] / 100.0, v[20] / 100.0, v[23] / 100.0, v[24] / 100.0);
    if (std::getenv("STEREO_HIP_TRWS_TIMELINE"))   // (development: how often, and for how long, the message recurrence found its next node not staged yet)
      std::fprintf(stderr, "[stereo_hip spec] runner visits %llu; the message recurrence found its node not staged yet: forward sweeps %llu times, %.1f us in all; "
                           "backward %llu times, %.1f us (incl. the wait for the rows in front of the chain)\n", v[2], v[3], (double)v[4] / 100.0, v[5], (double)v[6] / 100.0);
  }
  return 0;
}

int stereo_trws_messages(int kernel, int K, int64_t M, const double *Di, const double *gamma, const double *msg_in,
                         const double *q_source, const double *q_dest, const double *alpha, double lambda,
                         int certificate, int window, const double *shared_positions, double *msg_out,
                         double *vmin, int32_t *used_serial, char *err, size_t errcap) {
  if (kernel != 1 && kernel != 2) return fail("Unsupported kernel", err, errcap);
  if (K < 1 || K > kWave || M < 1) return fail("stereo_trws_messages: K must be in [1, 64], M >= 1", err, errcap);
  if (!Di || !gamma || !msg_in || !q_source || !q_dest || !alpha || !msg_out || !vmin)
    return fail("stereo_trws_messages: NULL argument", err, errcap);
  if (stereo_hip_device_count() < 1) return fail("stereo_trws_messages: no HIP device available", err, errcap);
  try {
    const size_t MK = (size_t)M * K;
    DevBuf<double> dD, dg, dm, dqs, dqd, da, dout, dv;
    DevBuf<uint16_t> dperm;
    DevBuf<int32_t> dser;
    DevBuf<unsigned long long> dfb;
    dD.upload(Di, MK); dg.upload(gamma, M); dm.upload(msg_in, MK); dqs.upload(q_source, MK); dqd.upload(q_dest, MK);
    da.upload(alpha, M); dout.alloc(MK); dv.alloc(M); dperm.alloc(MK); dser.alloc(M); dfb.alloc(4096);
    STEREO_HIP_CHECK(hipMemset(dfb.p, 0, sizeof(unsigned long long) * 4096));
    run_argsort(dqs.p, dperm.p, K, M, nullptr);
    fix_equal_positions(dqs.p, dperm.p, K, M);
    DevParams p{};
    p.K = K; p.Kp = (K + 1) & ~1; p.kernel = kernel; p.lambda = lambda; p.certificate = certificate ? 1 : 0;
    p.fallbacks = dfb.p;
    if (shared_positions) { p.pos_first = shared_positions[0]; p.pos_last = shared_positions[K - 1]; }
    // shared_positions: every message's q_source and q_dest ARE this vector (the caller's promise, as the
    // sweep kernels have it with fronto-parallel labels); strictly ascending ones take the compacted
    // certified loop of message_regs<.., true>
    bool shared_asc = false;
    if (shared_positions) {
      p.pos_gap = std::numeric_limits<double>::infinity();
      for (int k = 1; k < K; ++k) p.pos_gap = std::min(p.pos_gap, shared_positions[k] - shared_positions[k - 1]);
      shared_asc = K > 1 && p.pos_gap > 0 && std::isfinite(shared_positions[0]) && std::isfinite(shared_positions[K - 1]);
      if (!shared_asc && kernel == 1) p.pos_gap = 0;
    }
    if (const char *dbg = std::getenv("STEREO_HIP_TRWS_DEBUG")) p.debug = std::atoi(dbg);
    const unsigned grid = (unsigned)std::min<int64_t>(M, 4096);
#define STEREO_MSG_LAUNCH(KER, SH)                                                                                              \
    hipLaunchKernelGGL((trws_messages_kernel<KER, SH>), dim3(grid), dim3(kWave), 0, 0, p, K, M, dD.p, dg.p, dm.p, dqs.p, dqd.p, \
                       da.p, dperm.p, shared_positions ? window : -1, dout.p, dv.p, dser.p, dfb.p)
    if (kernel == 1) { if (shared_asc) STEREO_MSG_LAUNCH(1, true); else STEREO_MSG_LAUNCH(1, false); }
    else STEREO_MSG_LAUNCH(2, false);
#undef STEREO_MSG_LAUNCH
    STEREO_HIP_CHECK(hipGetLastError());
    STEREO_HIP_CHECK(hipDeviceSynchronize());
    STEREO_HIP_CHECK(hipMemcpy(msg_out, dout.p, sizeof(double) * MK, hipMemcpyDeviceToHost));
    STEREO_HIP_CHECK(hipMemcpy(vmin, dv.p, sizeof(double) * M, hipMemcpyDeviceToHost));
    if (used_serial) STEREO_HIP_CHECK(hipMemcpy(used_serial, dser.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost));
    return 0;
  } catch (const HipError &e) {
    return fail(e.msg, err, errcap);
  }
}

}  // extern "C"
