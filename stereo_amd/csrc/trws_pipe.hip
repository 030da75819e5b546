// TRW-S pipelined sweep kernel for K <= 64 (both smoothness kernels): role-specialised waves, one
// barrier per visit, every role's visit loop a function of its own (pipe_compute, pipe_loader_b, pipe_loader_a,
// pipe_storer, pipe_primal) that the kernel body (pipe_body) calls once per run.  Part of libstereo_hip.so; overview in
// DESIGN.md 4.1, the run and visit frame in trws_visit.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stereo_hip.h"
#include "common.h"
#include "trws_dev.h"
#include "trws_launch.h"
#include "trws_spec.h"
#include "trws_visit.h"

namespace stereo {
namespace {

#define RLI(v, i) __builtin_amdgcn_readlane((v), (i))

// ---- tagged-granule hand-over (kDescGran, DevParams::gran): a message entry travels as two 8-byte
// granules {high half, epoch} {low half, epoch}, ONE aligned 16-byte write-through store per lane; the consumer re-reads
// them until every tag is the sweep's epoch -- the data is the flag, no drain, no flag store, no second round trip.
// Inline assembly because the loads must be repeated: the compiler takes the buffer-load builtins for loads of
// unchanging memory and keeps a single one out of the spin loop, and volatile loads wait for each other one by one.
typedef unsigned int gran4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void publish_granules(unsigned long long *a, double v, int epoch) {
  const gran4 d = {(unsigned)__double2hiint(v), (unsigned)epoch, (unsigned)__double2loint(v), (unsigned)epoch};
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(a), "v"(d) : "memory");
}
__device__ __forceinline__ void load_granules2(const unsigned long long *a, const unsigned long long *b, gran4 &x, gran4 &y) {
  asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %3, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(x), "=&v"(y) : "v"(a), "v"(b) : "memory");
}
__device__ __forceinline__ void load_granules2x(const unsigned long long *a, const unsigned long long *b, const unsigned long long *c,
                                                gran4 &x, gran4 &y, unsigned long long &z) {
  asm volatile("global_load_dwordx4 %0, %3, off sc0 sc1\n\tglobal_load_dwordx4 %1, %4, off sc0 sc1\n\t"
               "global_load_dwordx2 %2, %5, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(x), "=&v"(y), "=&v"(z) : "v"(a), "v"(b), "v"(c) : "memory");
}
__device__ __forceinline__ void load_granule_x(const unsigned long long *c, unsigned long long &z) {
  asm volatile("global_load_dwordx2 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(z) : "v"(c) : "memory");
}
__device__ __forceinline__ bool granules_tagged(gran4 x, unsigned epoch) { return x.y == epoch && x.w == epoch; }
__device__ __forceinline__ double granules_value(gran4 x) { return __hiloint2double((int)x.x, (int)x.z); }
// development switch 262144 (tests): a hashed quarter of the nodes publishes a few microseconds late -- consumers
// find old tags and sweep again; nothing is skipped or changed
__device__ __forceinline__ void granule_delay(const DevParams &p, int node) {
  if (!(p.debug & 262144) || (((unsigned)node * 2654435761u) >> 30) != 0) return;
  const long long t0 = (long long)wall_clock64();
  while ((long long)wall_clock64() - t0 < 400) __builtin_amdgcn_s_sleep(2);
}

// ---- pipelined persistent sweep (K <= 64): role-specialised waves ---------------------
// Same dataflow schedule and arithmetic as trws_persistent_kernel, but the global-memory traffic
// of a visit is taken off the critical path by dedicated waves of the workgroup:
//   waves 0-7  compute: read the staged node from LDS, form Di, compute outgoing message
//              `wave` in registers, hand it over in LDS
//   wave 8     loader:  while node i is computed, decodes the descriptor of node i+1, waits
//              for its foreign completion flags, fetches unary / messages / weights /
//              positions / neighbour labels and stages them in LDS
//   wave 9     storer:  while node i is computed, writes node i-1's new messages and scalars
//              to HBM (write-through), drains, raises node i-1's completion flag
//   wave 10    loader A: the node's OWN data (unary row, last sweep's outgoing rows, weights), requested two
//              visits ahead -- nothing there waits for a flag -- and the prefix of Di summed once per node
//   wave 11    primal:  labelling + energy term of node i (previous iteration's primal pass)
// One s_barrier per visit.  The compute waves issue no vector-memory instruction outside the serial
// fallback's counter (and the granule publish behind a finished message), so no load or store latency is
// exposed on the chain of dependent visits.  That holds only while nothing the message routine keeps live
// across its loops has its address taken by an out-of-line routine: such a variable lives in the wave's
// private segment, which IS vector memory (message_regs, trws_dev.h: m1).
// SPEC: the instantiation that knows the speculative schedule (trws_graph.h: Sweep::Spec; trws_spec.h) -- a kernel of its
// own, launched only when a plan's sweeps use it: everything it adds (the runner's ticket, a segment's first visit,
// the held-back flags, the rows kept for a second walk, the commit) costs the visit loops registers, and the plain
// schedule's kernels stay what they were.
// BATCH: the body as trws_pipe_batch_kernel calls it, once per member of a batch (below): the one thing it adds is a mark
// in ctl[2] -- the speculative kernel's verdict word, unused here -- once the workgroup holds a run of this member.
//
// ROLES: every role's visit loop is a real (noinline) function with a register allocation of its own, as the runner's
// roles are (trws_spec.h).  In one function with the ticket loop, the commit, the profile epilogue and a by-value
// parameter block of some seventy fields, the allocator spilled ~180 scalars into VGPR lanes by live ranges it cannot
// weigh, and 55-70 v_readlane / v_writelane per visit sat on the finishing compute wave.
// A role reads the parameter block from its copy in global memory -- through the constant address space and a uniform
// address: scalar loads, as a kernel reads its arguments --, takes the run's values as arguments (they arrive in vector
// registers and are declared uniform), addresses LDS through the dynamic allocation's own symbol, pinned, and hands back
// what the kernel body needs of it: the busy cycles of the development profile, what the wave keeps from run to run
// (the compute waves' look_streak) and whether it left through the abort word.  A spill in the caller is paid once per
// run of hundreds of visits.
struct PipeRoleResult {
  unsigned long long busy;
  int carry;
  int aborted;
};
__device__ __forceinline__ PipeRoleResult pipe_role_result(unsigned long long busy, int carry, int aborted) {
  PipeRoleResult r;
  r.busy = busy; r.carry = carry; r.aborted = aborted;
  return r;
}
// The parameter block as a role reads it: field by field from the constant address space at a uniform address -- every
// load a scalar load, and a field the role does not use no load at all.  (EVERY field is named: one left out would read
// as zero -- the copy is value-initialised -- in the roles and nowhere else.  Not a whole-struct copy: C++ cannot copy
// a struct out of address space 4 (the copy constructor takes a generic reference), and the copy through a generic
// pointer, left to the compiler to trace back to the constant address space, came out as flat loads into vector
// registers, which the scalar constraints of the visit frame refuse.  trws_spec.h: uniform_params is the other such list.)
typedef const __attribute__((address_space(4))) DevParams pipe_const_params;
__device__ __forceinline__ DevParams pipe_role_params(const DevParams *pp_) {
  static_assert(sizeof(DevParams) == 632, "a field was added to DevParams: name it below");
  pipe_const_params *c = (pipe_const_params *)uniform_value(pp_);
  DevParams q{};
#define F(f) q.f = c->f;
#define F2(f) q.f[0] = c->f[0]; q.f[1] = c->f[1];
  F(K) F(Kp) F(kernel) F(lambda) F(unary) F(msg) F(q) F(qprim) F(pos) F(perm_q) F(perm_qp) F(perm_pos) F(alpha) F(mdir) F(tail) F(order)
  F(fptr) F(fidx) F(bptr) F(bidx) F(gamma) F(lb_pos_node) F(lb_pos_edge) F(lbterms) F(eterms) F(x)
  F2(run_ptr) F2(run_order) F2(nruns) F2(dep_ptr) F2(dep_rank) F2(in_slot)
  F(done) F(ticket) F(abort_flag) F(spin_ticks) F(n_own) F(N) F(fallbacks) F(certificate) F(lean) F(prof) F2(desc) F(prof_run)
  F(large_scratch) F(debug) F(timeline) F(window) F(uniform_step) F(win_ok) F(pos_gap) F(pos_first) F(pos_last) F2(ntickets)
  F2(spec_kind) F2(spec_c0) F2(spec_c1) F(spec_len) F(spec_nseg) F(spec_max_len) F(spec_rows) F(spec_x) F(spec_undo) F(spec_stat)
  F(tl_stride) F(self) F(peer_msg0) F(peer_msg1) F(peer_done0) F(peer_done1) F(peer_x0) F(peer_x1) F(gran) F(xgran) F2(run_rec)
#undef F2
#undef F
  return q;
}

// A visit is bound by the instructions the CU's four SIMDs issue for all twelve waves (~4400 per visit
// before round 4, 45 % of them scalar), so the service waves are written branch-poor: no exec-mask region
// per row -- a lane beyond the last label works on label K - 1 again (loads read an element that exists,
// stores repeat lane K - 1's value at lane K - 1's address), a row the node does not have is skipped by
// ONE scalar branch on a uniform count or on a mask the host put into the descriptor (word 55: which
// incoming rows come from global memory), row addresses are one unsigned 32 x 32 -> 64 multiply and one
// shift-add on a per-lane base, and values one lane needs from another lane's descriptor word come by
// ds_bpermute instead of chains of eight compares and selects.
#define PIPE_ROW(BASE, E) ((BASE) + (size_t)((unsigned long long)(unsigned)(E) * (unsigned long long)(unsigned)Kv))
#ifdef STEREO_HIP_VISIT_PROFILE
#define VSTAMP(i) do { const long long n_ = (long long)__builtin_readcyclecounter(); vacc[i] += (unsigned long long)(n_ - vmark); vmark = n_; } while (0)
#define PIPE_VISIT_MARK long long vmark = (long long)__builtin_readcyclecounter();
// (the stamps of the profile flavour are a role's own: it adds them up where the kernel body adds the busy cycles)
#define PIPE_ROLE_STAMPS unsigned long long vacc[6] = {0, 0, 0, 0, 0, 0}, macc[5] = {0, 0, 0, 0, 0}, lacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PIPE_ROLE_STAMPS_OUT \
  if (p.prof && lane == 0 && (p.prof_run < 0 || run == p.prof_run)) { \
    if (wave == 0) for (int i = 0; i < 6; ++i) atomicAdd(p.prof + 48 + i, vacc[i]); \
    if (wave == 0) for (int i = 0; i < 5; ++i) atomicAdd(p.prof + 56 + i, macc[i]); \
    if (wave == kPipeCompute) for (int i = 0; i < 4; ++i) atomicAdd(p.prof + 16 + i, lacc[i]); \
    if (wave == kPipeCompute + 1) for (int i = 4; i < 7; ++i) atomicAdd(p.prof + 16 + i, lacc[i]); \
  }
#else
#define VSTAMP(i) do { } while (0)
#define PIPE_VISIT_MARK
#define PIPE_ROLE_STAMPS
#define PIPE_ROLE_STAMPS_OUT
#endif
#define PIPE_LOAD8(DST, PTR) DST = *(PTR)   /* plain loads: the compiler keeps them in flight across the barrier and waits at the first use */
#define PIPE_REQUEST_OWN(W)                                                                          \
    do {                                                                                             \
      const int rf_ = RLI((W), 2);                                                                   \
      const int rnout = rf_ & 15, rtot = rnout + ((rf_ >> 4) & 15);                                  \
      { const double *a_ = PIPE_ROW(p.unary + lkv, RLI((W), 0)); PIPE_LOAD8(rdk, a_); }                   \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                \
        if (j < rnout && (UPDATE || PRIMAL)) { const double *a_ = PIPE_ROW((p.msg + lkv), RLI((W), 4 + j)); PIPE_LOAD8(rmv[j], a_); } \
        if (!SHARED && j < rtot) {                                                                   \
          const double *a_ = PIPE_ROW(p.q + lkv, RLI((W), 4 + j)), *b_ = PIPE_ROW(p.qprim + lkv, RLI((W), 4 + j)); \
          PIPE_LOAD8(rqv[j], a_); PIPE_LOAD8(rqpv[j], b_);                                           \
        }                                                                                            \
      }                                                                                              \
      rav = p.alpha[__shfl((W), 4 + (lane & 7), kWave)];  /* lane j: weight of the node's edge j (words of absent edges hold 0) */ \
    } while (0)

// What every role is called with, and how it sets itself up: the parameter block, the run's values as uniform values,
// the LDS carve of pipe_body (the one statement of the layout is there; kPipeLdsDoubles checks it), the names the visit
// frame uses.  prof_on_: the kernel body's verdict on the development profile (switches 2 / 4: one direction only).
#define PIPE_ROLE_PARAMS const DevParams *pp_, int epoch_, int p0_, int p1_, int run_, int seg_, int spec_in_, int second_walk_, int prof_on_
#define PIPE_ROLE_ENTER                                                                                    \
  extern __shared__ __attribute__((aligned(16))) double pipe_lds[];                                        \
  DevParams p = pipe_role_params(pp_);                                                                     \
  if (!__builtin_amdgcn_readfirstlane(prof_on_)) p.prof = nullptr;                                         \
  const int epoch = __builtin_amdgcn_readfirstlane(epoch_), p0 = __builtin_amdgcn_readfirstlane(p0_),      \
            p1 = __builtin_amdgcn_readfirstlane(p1_), run = __builtin_amdgcn_readfirstlane(run_),          \
            seg = __builtin_amdgcn_readfirstlane(seg_), second_walk = __builtin_amdgcn_readfirstlane(second_walk_); \
  const bool spec_in = __builtin_amdgcn_readfirstlane(spec_in_) != 0;                                      \
  double *lds = pinned_lds(pipe_lds);                                                                      \
  double *stage0 = lds, *hand = lds + 2 * kStageDoubles, *scal = hand + 4 * 8 * kWave;                     \
  double *hqtab = scal + 2 * kScalDoubles;                                                                 \
  int *ctl = (int *)(lds + kPipeCtlOff), *dring = ctl + 4;                                                 \
  double *zrow = (double *)(dring + 3 * kWave), *gtab = zrow + kWave;                                      \
  constexpr int D = BACKWARD ? 1 : 0, DW = TrwsGraph::kDescWords;                                          \
  const int32_t *desc = p.desc[D];                                                                         \
  const int K = p.K;                                                                                       \
  const double inf = __builtin_huge_val();                                                                 \
  const int tid = threadIdx.x, lane = tid & (kWave - 1);                                                   \
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);                                            \
  const bool act = lane < K;                                                                               \
  unsigned long long busy = 0;                                                                             \
  PIPE_ROLE_STAMPS                                                                                         \
  (void)epoch; (void)run; (void)seg; (void)second_walk; (void)spec_in; (void)hqtab; (void)dring; (void)zrow; (void)gtab; \
  (void)desc; (void)inf; (void)wave; (void)act; (void)DW;
#define PIPE_ROLE_LEAVE(CARRY) \
  PIPE_ROLE_STAMPS_OUT \
  return pipe_role_result(busy, (CARRY), 0);

// every role walks the run in its own loop (trws_visit.h): four ring slots, the abort word looked at before the barrier
#define PIPE_VISITS_BEGIN \
    TRWS_VISITS_BEGIN(TRWS_BUSY_OPEN PIPE_VISIT_MARK, stage0, kStageDoubles, TRWS_RING4(hand, kWave), scal, TRWS_ABORT_LOOK(ctl) TRWS_OPAQUE_K)
#define PIPE_VISITS_END \
    TRWS_VISITS_END(TRWS_BUSY_CLOSE VSTAMP(4);, TRWS_ABORT_LEAVE_WITH(aborted_, , pipe_role_result(0, 0, 1)), __syncthreads(), VSTAMP(5);)

// ---- compute (waves 0-7).  look_streak_: failed second looks in a row of this wave (message_regs), kept from run to
// run by the kernel body; posk, perm_shared: the lane's position and its place in the source order, read once per launch.
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC>
__device__ __attribute__((noinline)) PipeRoleResult pipe_compute(PIPE_ROLE_PARAMS, int look_streak_, double posk, int perm_shared) {
    PIPE_ROLE_ENTER
    int look_streak = __builtin_amdgcn_readfirstlane(look_streak_);
#ifdef STEREO_HIP_VISIT_PROFILE
    // wave 0's message stamps.  The array's address is made a value first: selected as it stands (wave == 0 ? macc : nullptr)
    // in a function with a frame, this toolchain puts the s_add that forms the frame address between the compare and its
    // s_cselect, the add overwrites SCC, and every wave gets the null pointer (seen in this flavour's assembly; the stamps read 0).
    unsigned long long *macc_w0 = macc;
    asm volatile("" : "+s"(macc_w0));
    if (wave != 0) macc_w0 = nullptr;
#endif
    {
    PIPE_VISITS_BEGIN
      {
        // ------------------------------------------------------------ compute
        if (UPDATE && have_node) {
          const int *sti = (const int *)(st + kStI);
          const int f = __builtin_amdgcn_readfirstlane(sti[2]);
          const int nout = f & 15, nin = (f >> 4) & 15, md = (f >> 16) & 255;
          const int myrow = sti[72 + (lane & 7)];  // LDS offsets (doubles) of the node's incoming message rows, from the loader
          const unsigned twins = SHARED ? (unsigned)__builtin_amdgcn_readfirstlane(sti[kDescTwin]) : 0x76543210u;
          // lanes 0-7: the edge ids of the node's messages, lane 8: the granule word -- one LDS read in flight with the
          // ones above, so that publishing behind the message waits for no LDS round trip (it used to wait for three)
          const int gword = sti[lane == 8 ? kDescGran : 4 + (lane & 7)];
          const int gpub = p.gran ? (RLI(gword, 8) >> 8) & 255 : 0;   // messages published as granules
          VSTAMP(0);
          if (wave < nout || (BACKWARD && wave == 0)) {  // waves without a message stay out of the way
          // the prefix of Di in list order -- the unary row and the outgoing rows, last sweep's messages -- is
          // loader A's sum, staged once per node (a lane beyond K holds a value nobody uses)
          double Di = st[kStP + lane];
          // (this wave's own old message is one of the prefix's rows; it is read from its stage row)
          const double mown = st[kStM + (wave < nout ? wave : 0) * kWave + lane];
          const int partner = wave < nout ? (int)((twins >> (4 * wave)) & 15u) : wave;
          const int twin_mask = (SHARED && KERNEL == 1) ? __builtin_amdgcn_readfirstlane((int)st[kStA + 9]) : 0;   // (loader A's verdict)
          const double alpha_me = st[kStA + (wave < nout ? wave : 0)];
          // (the tail -- list positions nout .. nout + 3, the incoming rows of an ordinary node -- is requested
          //  together and added in list order; a position the node does not have is the zero row -- x + 0.0 == x --,
          //  so nothing here branches on the node's degree and the reads share one LDS latency instead of paying
          //  one each; a node with more than four incoming rows -- border chain, row ends, off-grid graphs --
          //  takes one uniform branch for positions nout + 4 ..)
          {
            double rowv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) rowv[j] = lds[__builtin_amdgcn_readlane(myrow, j) + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) Di += rowv[j];
            if (nin > 4) {
#pragma unroll
              for (int j = 0; j < 4; ++j) rowv[j] = lds[__builtin_amdgcn_readlane(myrow, 4 + j) + lane];
#pragma unroll
              for (int j = 0; j < 4; ++j) Di += rowv[j];
            }
          }
          double node_vmin = 0;
          if (BACKWARD) {
            node_vmin = wave_min_dpp(act ? Di : inf);
            Di -= node_vmin;
            if (tid == 0) sc[8] = node_vmin;
          }
          VSTAMP(1);
          {
            const int j = wave;  // one compute wave per outgoing message
            if (j < nout) {
              const double gamma = st[kStG];  // (double)1 / (double)max(n_out, n_in), MRFEnergy.cpp:207-228
              const double h = act ? gamma * Di - mown : inf;
              const bool src_is_qprim = ((BACKWARD ? 1 : 0) == ((md >> j) & 1));
              double qsrc = posk, qdst = posk;
              const uint16_t *perm = p.perm_pos;
              if (!SHARED) {
                const double a_ = act ? st[kStQ + j * kWave + lane] : 0.0;
                const double b_ = act ? st[kStQP + j * kWave + lane] : 0.0;
                qsrc = src_is_qprim ? b_ : a_;
                qdst = src_is_qprim ? a_ : b_;
                const int e = __builtin_amdgcn_readfirstlane(sti[4 + j]);
                perm = (src_is_qprim ? p.perm_qp : p.perm_q) + (size_t)e * Kv;
              }
              const double alpha = alpha_me;
              // a twin -- the node's other message to the same neighbour -- with the same weight and the same old
              // message is the same message: one wave finishes it, the other takes half of its loop (CoopPart)
              CoopPart cp;
              if (SHARED && KERNEL == 1 && ((twin_mask >> j) & 1)) {
                const int helper = j > partner ? j : partner;
                cp.word = 1 | (j > partner ? 2 : 0) | (helper << 4) | (((pos + 1) & 0x7fffff) << 8);
                cp.lds = lds;
              }
              VSTAMP(2);
              double newm = 0;
              const double v = message_regs<KERNEL, SHARED>(p, Kv, alpha, h, qsrc, qdst, perm, newm, lane,
                                                    hqtab + wave * kPipeTab + 4 * kPipePad, (SHARED && p.win_ok) ? p.window : -1, &look_streak
#ifdef STEREO_HIP_VISIT_PROFILE
                                                    , macc_w0
#else
                                                    , nullptr
#endif
                                                    , perm_shared, cp);
              VSTAMP(3);
              if (!cp.part()) {
                hcur[j * kWave + lane] = newm;   // (lanes beyond K fill the row's padding)
                if (BACKWARD && lane == 0) sc[j] = v;
                if (cp.active()) {
                  hcur[partner * kWave + lane] = newm;
                  if (BACKWARD && lane == 0) sc[partner] = v;
                }
                // final: to the consumer in another run as granules now, not behind the storer's flag one visit later
                // (lanes < K only: the granules of a lane beyond K are nobody's)
                const int gmine = gpub & ((1 << j) | (cp.active() ? 1 << partner : 0));
                if (gmine) {
                  if (p.debug & 262144) granule_delay(p, __builtin_amdgcn_readfirstlane(sti[0]));   // (the node's number is read only when asked for: an LDS round trip)
                  if ((gmine >> j) & 1)
                    if (act) publish_granules(p.gran + 2 * ((size_t)(unsigned)RLI(gword, j) * (unsigned)Kv + lane), newm, epoch);
                  if ((gmine >> partner) & 1 && partner != j)
                    if (act) publish_granules(p.gran + 2 * ((size_t)(unsigned)RLI(gword, partner) * (unsigned)Kv + lane), newm, epoch);
                }
              }
            }
          }
          }
        }
      }
    PIPE_VISITS_END
    }
    PIPE_ROLE_LEAVE(look_streak)
}

// ---- loader B (wave 8): stage node pos + 1 -- what comes from other runs, behind flags or as granules
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC>
__device__ __attribute__((noinline)) PipeRoleResult pipe_loader_b(PIPE_ROLE_PARAMS) {
    PIPE_ROLE_ENTER
    int wnext = desc[(size_t)p0 * DW + lane];   // raw descriptor word of the node after next (prefetched)
    {
    PIPE_VISITS_BEGIN
      {
        // ------------------------------------------------------------ loader: stage node pos + 1
        if (pos + 1 >= p0 && pos + 1 < p1) {
          const int w = wnext;
          if (pos + 2 < p1) wnext = desc[(size_t)(pos + 2) * DW + lane];
          int *stni = (int *)(stn + kStI);
          // (first visit of a speculative segment: the rows of the node in front come from the runner, behind the
          //  segment's flag -- to everybody else in the workgroup they look like rows of another run)
          //  (a second walk takes the same rows from the messages themselves: the segment in front has committed)
          const bool sfirst = SPEC && seg > 0 && pos + 1 == p0;
          stni[lane] = (sfirst && lane >= 12 && lane < 20 && w >= 0) ? -1 : w;
          dring[((pos + 1) % 3) * kWave + lane] = w;
          const int f = RLI(w, 2);
          const int nout = f & 15, ntot = nout + ((f >> 4) & 15);
          int ndep = (f >> 8) & 15;
          int fm = RLI(w, kDescFetch) & 255;   // incoming rows that come from global memory (behind flags)
          const int gw = p.gran ? RLI(w, kDescGran) : 0;
          const int gm = gw & 255;             // ... of them those that come as granules instead
          fm &= ~gm;
          const int j8 = lane & 7;
          int sl = __shfl(w, 12 + j8, kWave);  // lane j: hand-over slot of the node's edge j, label source
          const int xn = __shfl(w, 32 + j8, kWave);
          int smask = 0, deprank = __shfl(w, 20 + (lane & 3), kWave);
          if (sfirst) {
            smask = (int)(__builtin_amdgcn_ballot_w64(lane < 8 && lane >= nout && lane < ntot && sl >= 0) & 255ull);
            fm |= smask;
            sl = -1;
            deprank = lane == ndep ? p.N + seg : deprank;
            ++ndep;
          }
          {
            // where the compute waves find the tail of Di at visit pos + 1 -- entry k: list position nout + k, the
            // node's k-th incoming row; the outgoing rows are in loader A's prefix --: a message handed
            // over inside the run sits in the ring of the last two visits, everything else in this
            // stage, a position the node does not have is the zero row -- decided once here instead of by
            // every compute wave in scalar code
            const int q8 = (nout + j8) & 7;
            const int slq = sfirst ? -1 : __shfl(w, 12 + q8, kWave);
            const int row = nout + j8 >= ntot ? (int)(zrow - lds)
                          : slq < 0 ? (int)(stn - lds) + kStM + q8 * kWave
                          : slq >= 8 ? (int)(hand - lds) + ((pos - 1) & 3) * 8 * kWave + (slq - 8) * kWave
                                     : (int)(hand - lds) + (pos & 3) * 8 * kWave + slq * kWave;
            if (lane < 8) stni[72 + lane] = row;
          }
          // (everything that does not depend on other workgroups -- unary, previous-sweep messages,
          //  positions, weights -- is loader A's, below, two visits ahead)
          // the completion flags of the foreign neighbours, then their data
          // (all flags are polled together: lane j watches dependency j)
          // (the rows that come from global memory -- two per foreign dependency, four on an ordinary row or
          //  chain node, up to eight where a node hangs on four other runs -- are the set bits of the mask, walked
          //  four at a time: row number and edge id of the k-th one are scalars; the addresses of the first four are
          //  formed BEFORE the wait, so that behind the flags nothing but the loads themselves is left)
          double mv[4];
          const double *fa[4];
          int jr[4];
          int mrest = UPDATE ? fm : 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            jr[k] = mrest ? __builtin_ctz(mrest) : -1;
            mrest &= mrest - 1;
            const int jk = jr[k] >= 0 ? jr[k] : 0;
            fa[k] = (SPEC && spec_in && ((smask >> jk) & 1)) ? PIPE_ROW((p.spec_rows + lkv), seg * 8 + jk)
                                                 : PIPE_ROW((p.msg + lkv), __builtin_amdgcn_readlane(w, 4 + jk));
          }
          // (the label of the node in front of a speculative segment: the runner's, kept apart from p.x -- what the commit
          //  compares must be what was read here)
          const int32_t *xa = (SPEC && spec_in && ((smask >> j8) & 1)) ? p.spec_x + seg : p.x + xn;
#ifdef STEREO_HIP_VISIT_PROFILE
          const long long lb0 = (long long)__builtin_readcyclecounter();
#endif
          const unsigned watch = gm ? (unsigned)(gw >> 16) & 15u : ~0u;   // (granule rows: their producers' flags are not waited for)
          if (ndep > 0 && watch) wait_for_dependencies_w(p, ndep, deprank, RLI(w, 1), epoch, lane, ctl + 1, watch);
#ifdef STEREO_HIP_VISIT_PROFILE
          const long long lb1 = (long long)__builtin_readcyclecounter();
#endif
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (jr[k] >= 0) mv[k] = ld_sc1(fa[k]);
          int pxv = 0;
          if (PRIMAL && ((fm >> j8) & 1)) pxv = ld_sc1(xa);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (jr[k] >= 0) stn[kStM + jr[k] * kWave + lane] = mv[k];
          while (mrest) {   // rows five to eight (rare)
            const int jx = __builtin_ctz(mrest);
            mrest &= mrest - 1;
            stn[kStM + jx * kWave + lane] = ld_sc1((SPEC && spec_in && ((smask >> jx) & 1)) ? PIPE_ROW((p.spec_rows + lkv), seg * 8 + jx)
                                                                                : PIPE_ROW((p.msg + lkv), __builtin_amdgcn_readlane(w, 4 + jx)));
          }
          if (gm) {
            // rows (and labels) of other runs' nodes that arrive as granules: re-read until every tag is this sweep's
            // epoch -- bounded by the wall clock like the flag wait, and a give-up aborts the workgroup the same way
            int gr = gm;
            const int g0 = __builtin_ctz(gr);
            int gj[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { gj[k] = gr ? __builtin_ctz(gr) : g0; gr &= gr - 1; }
            const bool more = __builtin_popcount(gm) > 2;
            const unsigned long long *ga[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) ga[k] = p.gran + 2 * ((size_t)(unsigned)RLI(w, 4 + gj[k]) * (unsigned)Kv + lkv);
            const unsigned long long *xg = p.xgran + xn;
            const bool want_x = PRIMAL && lane < 8 && ((gm >> lane) & 1);
            const unsigned ep = (unsigned)epoch;
            gran4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
            unsigned long long xv = 0;
            int spins = 0;
            long long t0 = 0;
            for (;;) {
              bool ok = true;
              if (UPDATE) {
                if (PRIMAL) load_granules2x(ga[0], ga[1], xg, a0, a1, xv);
                else load_granules2(ga[0], ga[1], a0, a1);
                ok = granules_tagged(a0, ep) && granules_tagged(a1, ep);
                if (more) { load_granules2(ga[2], ga[3], a2, a3); ok = ok && granules_tagged(a2, ep) && granules_tagged(a3, ep); }
              } else {
                load_granule_x(xg, xv);
              }
              if (want_x) ok = ok && (unsigned)(xv >> 32) == ep;
              if (!UNI(!ok)) break;
              if (!keep_waiting(p, spins, t0, false)) {
                if (lane == 0) {
                  report_give_up(p, RLI(w, 1), RLI(w, 20 + __builtin_ctz(~(gw >> 16) | 16)), (int)a0.y, epoch);
                  ctl[1] = 1;
                }
                break;
              }
            }
            if (UPDATE) {
              stn[kStM + gj[0] * kWave + lane] = granules_value(a0);
              stn[kStM + gj[1] * kWave + lane] = granules_value(a1);
              if (more) { stn[kStM + gj[2] * kWave + lane] = granules_value(a2); stn[kStM + gj[3] * kWave + lane] = granules_value(a3); }
            }
            if (want_x) pxv = (int)(unsigned)xv;
          }
          if (lane < 8) stni[64 + lane] = pxv;
#ifdef STEREO_HIP_VISIT_PROFILE
          if (pos > p0 + 3) {  // steady state only: the first visits of a run wait for the wavefront to arrive
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            const long long lb2 = (long long)__builtin_readcyclecounter();
            lacc[0] += (unsigned long long)(lb0 - vmark); lacc[1] += (unsigned long long)(lb1 - lb0);
            lacc[2] += (unsigned long long)(lb2 - lb1); lacc[3] += 1;
          }
#endif
        }
      }
    PIPE_VISITS_END
    }
    PIPE_ROLE_LEAVE(0)
}

// ---- loader A (wave 10): own data of node pos + 1, two visits deep -- descriptors of the next three nodes and the
// parked requests
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC>
__device__ __attribute__((noinline)) PipeRoleResult pipe_loader_a(PIPE_ROLE_PARAMS) {
    PIPE_ROLE_ENTER
    int wa1 = 0, wa2 = 0, wa3 = 0;
    double rdk = 0, rmv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rqv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rqpv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rav = 0;
    wa1 = desc[(size_t)p0 * DW + lane];
    if (p0 + 1 < p1) wa2 = desc[(size_t)(p0 + 1) * DW + lane];
    if (p0 + 2 < p1) wa3 = desc[(size_t)(p0 + 2) * DW + lane];
    { const int Kv = K, lkv = lane < K ? lane : K - 1; PIPE_REQUEST_OWN(wa1); }
    {
    PIPE_VISITS_BEGIN
      {
        // ------------------------------------------------------------ loader A: own data of node pos + 1
        // The registers hold what was requested during visit pos - 1 (its HBM latency lies behind a
        // whole visit, not inside one -- on the serial chains of the reference's node order the visit
        // was as long as this loader's round trip); it goes to the stage, then node pos + 2's requests
        // go out and stay in flight across the barrier (plain loads: the compiler waits at their first use,
        // which is in the next visit).
        if (pos + 1 >= p0 && pos + 1 < p1) {
          const int f = RLI(wa1, 2);
          const int nout = f & 15, nin = (f >> 4) & 15;
          stn[kStD + lane] = rdk;
          // (the prefix of Di in list order, ((D + m_0) + m_1) + ..: the association the compute waves used to form, each
          //  by itself, from the rows written here -- those stay for the primal wave, the waves' own rows and the twin verdict)
          double pk = rdk;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j < nout) { stn[kStM + j * kWave + lane] = rmv[j]; if (UPDATE) pk += rmv[j]; }
            if (!SHARED && j < nout + nin) { stn[kStQ + j * kWave + lane] = rqv[j]; stn[kStQP + j * kWave + lane] = rqpv[j]; }
          }
          if (UPDATE) stn[kStP + lane] = pk;
          if (SPEC && UPDATE && seg >= 0 && !second_walk) {
            // a speculative segment keeps the rows its visits overwrite: a second walk starts from them (below)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nout) st_sc1(PIPE_ROW(p.spec_undo + lkv, (seg * p.spec_max_len + (pos + 1 - p0)) * 4 + j), rmv[j]);
          }
          if (lane < 8) stn[kStA + lane] = rav;
          if (lane == 0) stn[kStG] = gtab[nout > nin ? nout : nin];
          if (SHARED && KERNEL == 1 && UPDATE) {
            // Which outgoing messages have a twin that IS the same message (word 56 names the candidates; equal weights,
            // bitwise equal old rows -- this wave holds them in registers -- and shared positions make it so): decided
            // here, off the compute waves' path, for ordinary nodes (up to four outgoing messages); bit j of the mask.
            const unsigned tw = (unsigned)RLI(wa1, kDescTwin);
            int mask = 0;
            if (nout <= 4 && !(p.debug & 8192)) {   // (development switch 8192: no twins)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int k = j + 1; k < 4; ++k) {
                  if (k < nout && (int)((tw >> (4 * j)) & 15u) == k) {
                    const bool same = !UNI(act && rmv[j] != rmv[k]) && RLI(__double2hiint(rav), j) == RLI(__double2hiint(rav), k) &&
                                      RLI(__double2loint(rav), j) == RLI(__double2loint(rav), k);
                    if (same) mask |= (1 << j) | (1 << k);
                  }
                }
              }
            }
            if (lane == 0) stn[kStA + 9] = (double)mask;
          }
          int wa4 = 0;
          if (pos + 4 < p1) wa4 = desc[(size_t)(pos + 4) * DW + lane];  // three nodes ahead: waited for at the top of the next visit
          wa1 = wa2; wa2 = wa3; wa3 = wa4;
          if (pos + 2 < p1) PIPE_REQUEST_OWN(wa1);
        }
      }
    PIPE_VISITS_END
    }
    PIPE_ROLE_LEAVE(0)
}

// ---- storer (wave 9): node pos - 1.  sw: node pos's descriptor word (per lane), fetched during visit pos and used right
// behind the barrier that ends it
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC>
__device__ __attribute__((noinline)) PipeRoleResult pipe_storer(PIPE_ROLE_PARAMS) {
    PIPE_ROLE_ENTER
    int sw = 0;
    {
    PIPE_VISITS_BEGIN
      {
        // ------------------------------------------------------------ storer: node pos - 1
        // The node's descriptor word is in a register since the previous visit (below) and nothing but the
        // fields the stores need is read from it, each row address being a scalar multiply and a shift-add:
        // the flag a row below waits for used to rise ~3 k cycles into this visit, 2.2 k of them the
        // decoding of all 55 descriptor fields and an exec-mask region per row.
        if (pos - 1 >= p0) {
          const double *scp = scal + ((pos + 1) & 1) * kScalDoubles;  // parity of pos - 1
          const int s_nout = RLI(sw, 2) & 15;
          const int s_remote = RLI(sw, kDescRemote), s_pn0 = RLI(sw, kDescPeerNode), s_pn1 = RLI(sw, kDescPeerNode + 1);
          if (UPDATE) {
            if (s_remote & 255) {   // strips: some rows go to a neighbour's array, under the neighbour's edge numbers
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                if (j < s_nout) {
                  double *mb = ((s_remote >> j) & 1) ? (((s_remote >> (8 + j)) & 1) ? p.peer_msg1 : p.peer_msg0) : p.msg;
                  const int ej = ((s_remote >> j) & 1) ? RLI(sw, kDescPeerEdge + j) : RLI(sw, 4 + j);
                  st_sc1(PIPE_ROW(mb + lkv, ej), hprev[j * kWave + lkv]);
                }
              }
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (j < s_nout) st_sc1(PIPE_ROW((p.msg + lkv), RLI(sw, 4 + j)), hprev[j * kWave + lkv]);
            }
            if (BACKWARD) {
              const int s_lbe = __shfl(sw, 24 + (lane & 7), kWave);   // lane j: position of message j's lower-bound term
              if (lane < s_nout) p.lbterms[s_lbe] = scp[lane];
              if (lane == 0) p.lbterms[RLI(sw, 3)] = scp[8];
            }
          }
          if (PRIMAL && lane == 0) {
            const int xi = ((const int *)(scp + 10))[0];
            st_sc1(p.x + RLI(sw, 0), xi);
            if (s_remote & (1 << 16)) st_sc1(p.peer_x0 + s_pn0, xi);
            if (s_remote & (1 << 17)) st_sc1(p.peer_x1 + s_pn1, xi);
            p.eterms[RLI(sw, kDescEpos)] = scp[9];
          }
          const int s_rank = RLI(sw, 1);
#ifdef STEREO_HIP_VISIT_PROFILE
          const long long sb0 = (long long)__builtin_readcyclecounter();
#endif
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef STEREO_HIP_VISIT_PROFILE
          if (pos > p0 + 3) {
            const long long sb1 = (long long)__builtin_readcyclecounter();
            lacc[4] += (unsigned long long)(sb0 - vmark); lacc[5] += (unsigned long long)(sb1 - sb0); lacc[6] += 1;
          }
#endif
          if (lane == 0) {
            if (!(SPEC && seg >= 0)) st_sc1(p.done + s_rank, epoch);   // (a speculative segment raises its flags when it commits)
            if (s_remote & (1 << 16)) st_sc1(p.peer_done0 + s_pn0, epoch);
            if (s_remote & (1 << 17)) st_sc1(p.peer_done1 + s_pn1, epoch);
          }
        }
        if (have_node) {
          // node pos's descriptor (it reached dring during visit pos - 1)
          sw = dring[(pos % 3) * kWave + lane];
        }
      }
    PIPE_VISITS_END
    }
    PIPE_ROLE_LEAVE(0)
}

// ---- primal (wave 11): labelling + energy term of node pos.  xprev, xprev2: labels of the previous two nodes of the run
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC>
__device__ __attribute__((noinline)) PipeRoleResult pipe_primal(PIPE_ROLE_PARAMS, double posk) {
    PIPE_ROLE_ENTER
    int xprev = 0, xprev2 = 0;
    {
    PIPE_VISITS_BEGIN
      {
        // ------------------------------------------------------------ primal of node pos
        if (PRIMAL && have_node) {
          const int *sti = (const int *)(st + kStI);
          const int f = __builtin_amdgcn_readfirstlane(sti[2]);
          const int nout = f & 15, nin = (f >> 4) & 15, md = (f >> 16) & 255, ntot = nout + nin;
          double db = act ? st[kStD + lane] : 0.0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j >= nout && j < ntot) {
              const int sl = __builtin_amdgcn_readfirstlane(sti[12 + j]);
              const int ks = sl >= 8 ? xprev2 : sl >= 0 ? xprev : __builtin_amdgcn_readfirstlane(sti[64 + j]);
              const int mdj = (md >> j) & 1;
              double d;
              if (SHARED) {
                const double pks = readlane_f64(posk, ks);
                d = mdj == 0 ? pks - posk : posk - pks;
              } else {
                const double qvj = act ? st[kStQ + j * kWave + lane] : 0.0;
                const double qpj = act ? st[kStQP + j * kWave + lane] : 0.0;
                d = mdj == 0 ? readlane_f64(qpj, ks) - qvj : qpj - readlane_f64(qvj, ks);
              }
              const double v = KERNEL == 1 ? fabs(d) : d * d;
              db += st[kStA + j] * min_raw(v, p.lambda);  // (v, lambda >= 0: the value of v < lambda ? v : lambda)
            }
          }
          double di = db;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (j < nout) di += st[kStM + j * kWave + lane];
          // first minimum (AddColumn's vectorMin): the minimum by a plain reduction, then the lowest lane that has it
          const double dim = act ? di : inf;
          const double vbest = wave_min_dpp(dim);
          const int bi = __builtin_ctzll(__builtin_amdgcn_ballot_w64(dim == vbest));
          xprev2 = xprev; xprev = bi;
          const double eb = readlane_f64(db, bi);
          if (lane == 0) { sc[9] = eb; ((int *)(sc + 10))[0] = bi; }
          if (p.gran && ((__builtin_amdgcn_readfirstlane(sti[kDescGran]) >> 20) & 1)) {   // the label, for consumers in other runs
            const int node = __builtin_amdgcn_readfirstlane(sti[0]);
            granule_delay(p, node);
            if (lane == 0) __hip_atomic_store(p.xgran + node, ((unsigned long long)(unsigned)epoch << 32) | (unsigned)bi, __ATOMIC_RELAXED, STEREO_HANDOVER_SCOPE);
          }
        }
      }
    PIPE_VISITS_END
    }
    PIPE_ROLE_LEAVE(0)
}
#undef PIPE_VISITS_BEGIN
#undef PIPE_VISITS_END
#undef PIPE_ROLE_LEAVE
#undef PIPE_ROLE_ENTER
#undef PIPE_ROLE_STAMPS_OUT
#undef PIPE_ROLE_STAMPS

// ---- the kernel body: LDS tables, the ticket loop, the roles by wave, the commit of a speculative segment, the
// development stamps.  pp: the block `p` was copied from, in global memory -- what the roles, the runner and the commit
// read (a plan's own launches: p.self; a group's or a batch's: the strip's / member's entry of the launch's table).
// TWO copies of the block, then: the ticket loop, the timeline and the stamps work from `p`, the roles from *pp.  What a
// launch edits in its by-value copy only (trws_plan.hip: the timeline pointer cleared for STEREO_HIP_TRWS_TIMELINE=first)
// the roles do not see; that is right only for fields no role reads, and `timeline` is the one such edit today.
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED, bool SPEC = false, bool BATCH = false>
__device__ __forceinline__ void pipe_body(DevParams p, const DevParams *pp, int epoch) {
  static_assert(!SPEC || (SHARED && KERNEL == 1), "the speculative schedule exists for shared positions and the linear kernel");
  static_assert(!(SPEC && BATCH), "batches keep the plain chain schedule");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double *stage0 = lds;                                   // 2 stages
  double *hand = lds + 2 * kStageDoubles;                 // ring of 4 x 8 x 64: the last visits' new messages
  double *scal = hand + 4 * 8 * kWave;                    // 2 x kScalDoubles
  double *hqtab = scal + 2 * kScalDoubles;                // per compute wave: 64 x (h, q, u, v)
  int *ctl = (int *)(hqtab + kPipeCompute * kPipeTab);    // [0] run, [1] abort
  int *dring = ctl + 4;                                   // the last three descriptors (the storer's comes from here, not from HBM)
  double *zrow = (double *)(dring + 3 * kWave);           // 64 zeros: where the Di loop finds the message rows a node does not have
  double *gtab = zrow + kWave;                            // gtab[k] = (double)1 / (double)k, k = 1 .. 8 (MRFEnergy.cpp:207-228), divided once
  double *xchg = gtab + 16;                               // per compute wave (as helper): partial minima and match counts of a shared message
  int *xflag = (int *)(xchg + kPipeCompute * kPipeXchg);  // ... and the flag behind them (CoopPart, trws_dev.h)
  (void)stage0;
  constexpr int D = BACKWARD ? 1 : 0;
  // The runner of the speculative schedule holds ticket 0 of either direction, and the workgroup that draws it calls
  // it HERE, before anything else: at this point only the kernel arguments are live.
  bool have_ticket = false;
  if (SPEC) {
    if (threadIdx.x == 0) { ctl[1] = 0; ctl[2] = 0; ctl[3] = 0; }
    if (draw_first_ticket<D>(p, ctl) == -1) chain_runner<PipeRunner, BACKWARD, PRIMAL, UPDATE>(pp, epoch);
    else have_ticket = true;
  }
  const int K = p.K;
  const double inf = __builtin_huge_val();
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const bool act = lane < K;
  // (per lane, read once per launch and handed to the roles as vector arguments)
  const double posk = (SHARED && act) ? p.pos[lane] : 0.0;
  int look_streak = 0;  // failed second looks in a row (this compute wave): see message_regs
  const int perm_shared = (SHARED && wave < kPipeCompute) ? (act ? (int)p.perm_pos[lane] : lane) : -1;  // source order by position, once
  if (!SPEC && tid == 0) { ctl[1] = 0; ctl[2] = 0; ctl[3] = 0; }
  if (tid < kWave) zrow[tid] = 0.0;
  if (tid < 16) gtab[tid] = (double)1 / (double)(tid > 0 ? tid : 1);
  if (tid < kPipeCompute) xflag[tid] = 0;
  if (wave < kPipeCompute && lane < 2 * kPipePad) {
    // padding of the source tables (entries -16 .. -1 and 64 .. 79): never overwritten afterwards
    double *e = hqtab + wave * kPipeTab + 4 * (lane < kPipePad ? lane : kWave + lane);
    e[0] = inf; e[1] = 0; e[2] = 0; e[3] = 0;
  }
  // development switches 2 / 4: profile backward / forward sweeps only
  const int prof_on = (p.prof != nullptr && !((p.debug & 2) && !BACKWARD) && !((p.debug & 4) && BACKWARD)) ? 1 : 0;

  for (;;) {
    // (ctl[3]: the workgroup walks the speculative segment it holds a second time -- no new ticket)
    TRWS_DRAW_TICKET(ctl, SPEC && (ctl[3] || have_ticket))
    have_ticket = false;
    // (the helpers' exchange flags show schedule positions: a second walk of a speculative segment visits the SAME
    //  positions again, and a flag left by the first walk would pass for the helper's word of the second -- the
    //  finishing wave would merge the first walk's partial minima, which are those of almost the same message.)
    //  (development switch 131072: flags left as they are)
    TRWS_RUN_ENTER(SPEC, ctl, if (tid < kPipeCompute && !(p.debug & 131072)) xflag[tid] = 0;)
    TRWS_SPEC_SEGMENT
    if (BATCH && tid == 0) ctl[2] = 1;
    if (p.timeline && tid == 0) p.timeline[((size_t)D * p.tl_stride + run) * 2] = wall_clock64();
    // every role walks the run in a function of its own (above); a wave is in one role for the whole launch
#define PIPE_ROLE(NAME) NAME<KERNEL, BACKWARD, PRIMAL, UPDATE, SHARED, SPEC>
#define PIPE_ROLE_ARGS pp, epoch, p0, p1, run, seg, spec_in ? 1 : 0, second_walk, prof_on
    PipeRoleResult r;
    if (wave < kPipeCompute) r = PIPE_ROLE(pipe_compute)(PIPE_ROLE_ARGS, look_streak, posk, perm_shared);
    else if (wave == kPipeCompute) r = PIPE_ROLE(pipe_loader_b)(PIPE_ROLE_ARGS);
    else if (wave == kPipeCompute + 2) r = PIPE_ROLE(pipe_loader_a)(PIPE_ROLE_ARGS);
    else if (wave == kPipeCompute + 1) r = PIPE_ROLE(pipe_storer)(PIPE_ROLE_ARGS);
    else r = PIPE_ROLE(pipe_primal)(PIPE_ROLE_ARGS, posk);
#undef PIPE_ROLE_ARGS
#undef PIPE_ROLE
    if (__builtin_amdgcn_readfirstlane(r.aborted)) return;   // (the abort word: the wave leaves the kernel, trws_visit.h)
    look_streak = r.carry;
    if (SPEC && seg >= 0) {
      const int verdict = spec_commit<1, kPipeWaves, 2, BACKWARD, PRIMAL, UPDATE>(pp, epoch, p0, p1, seg, spec_in ? 1 : 0, 2 * kPipeCtlOff);
      if (verdict == 2) return;
      if (verdict == 1) continue;   // (ctl[3] is set: the same run once more)
    }
    if (p.timeline && tid == 0) p.timeline[((size_t)D * p.tl_stride + run) * 2 + 1] = wall_clock64();
    if (prof_on && lane == 0 && (p.prof_run < 0 || run == p.prof_run)) {
      // busy cycles before the barrier per role: compute (wave 0), loader, storer, primal; steps
      const int slot = wave == 0 ? 0 : wave == kPipeCompute ? 1 : wave == kPipeCompute + 1 ? 2 : wave == kPipeCompute + 3 ? 3 : -1;
      if (slot >= 0) atomicAdd(p.prof + slot, r.busy);
      atomicAdd(p.prof + 32 + wave, r.busy);  // every wave: cycles from barrier to barrier arrival
      if (wave == 0) atomicAdd(p.prof + 6, (unsigned long long)(p1 - p0));
    }
  }
}

template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED>
__global__ __launch_bounds__(kPipeThreads) void trws_pipe_kernel(DevParams p, int epoch) {
  pipe_body<KERNEL, BACKWARD, PRIMAL, UPDATE, SHARED>(p, p.self, epoch);
}

template <bool BACKWARD, bool PRIMAL, bool UPDATE>
__global__ __launch_bounds__(kPipeThreads) void trws_pipe_spec_kernel(DevParams p, int epoch) {
  pipe_body<1, BACKWARD, PRIMAL, UPDATE, true, true>(p, p.self, epoch);
}

template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED>
__global__ __launch_bounds__(kPipeThreads) void trws_pipe_group_kernel(GroupArgs ga, int epoch) {
  const DevParams *pp = ga.pp + group_strip(ga);   // the strip's block
  pipe_body<KERNEL, BACKWARD, PRIMAL, UPDATE, SHARED>(*pp, pp, epoch);
}

// Independent problems in one launch (stereo_trws_batch_*): the member frame of trws_visit.h around the
// body.  A workgroup starts at the member its block index names (the host's shares, as for strips), walks that member's
// runs until its tickets are used up, and moves on to the next member, round the table once.  Everything the body keeps
// per problem -- the parameter block in scalar registers, positions and permutation per lane, the LDS tables -- is set
// up again by the body itself at every call: a member is entered exactly as a launch of its own enters it.  A member
// whose sweep gave up (ctl[1]) ends the workgroup: the host reports that member, and nothing is started behind a fault.
template <int KERNEL, bool BACKWARD, bool PRIMAL, bool UPDATE, bool SHARED>
__global__ __launch_bounds__(kPipeThreads) void trws_pipe_batch_kernel(BatchArgs ba, int epoch) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int *ctl = (int *)(lds + kPipeCtlOff);
  int *state = (int *)(lds + kPipeLdsDoubles);   // (behind the body's LDS: pipe_batch_lds_bytes)
  TRWS_MEMBERS_BEGIN(ba, group_strip(ba.g), state)
    pipe_body<KERNEL, BACKWARD, PRIMAL, UPDATE, SHARED, false, true>(ba.g.pp[member], ba.g.pp + member, epoch);   // (the member's block in the table)
  TRWS_MEMBERS_END(ba, ctl, state)
}

#undef PIPE_REQUEST_OWN
#undef PIPE_LOAD8
#undef VSTAMP
#undef PIPE_VISIT_MARK
#undef PIPE_ROW
#undef RLI

}  // namespace

size_t pipe_lds_bytes() {
  static_assert(kPipeLdsDoubles == 2 * kStageDoubles + 4 * 8 * kWave + 2 * kScalDoubles + kPipeCompute * kPipeTab + 2 + 3 * kWave / 2 + kWave + 16 +
                                   kPipeCompute * kPipeXchg + kPipeCompute / 2, "LDS layout of pipe_body");
  return sizeof(double) * kPipeLdsDoubles;
}
static size_t pipe_batch_lds_bytes() { return sizeof(double) * (kPipeLdsDoubles + 2); }   // ... with the member frame's state behind
size_t pipe_spec_lds_bytes() { return sizeof(double) * (kRunBase + kRunDoubles + kRunDummy); }   // ... with the runner's ring behind
int pipe_threads() { return kPipeThreads; }

// rows: [smoothness kernel 1 | 2][per-edge | shared positions][plain | group], then the speculative schedule's kernel;
// the batch kernels in a table of their own: [smoothness kernel 1 | 2][per-edge | shared positions]
#define PIPE_ENTRY(BW, PR, UP, NAME, KER, SH) (const void *)NAME<KER, BW, PR, UP, SH>,
#define PIPE_SPEC_ENTRY(BW, PR, UP, ...) (const void *)trws_pipe_spec_kernel<BW, PR, UP>,
#define PIPE_ROWS(KER, SH) {TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_kernel, KER, SH)}, {TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_group_kernel, KER, SH)}
constexpr int kPipeSpecRow = 8;
static const SweepRow kPipeKernels[kPipeSpecRow + 1] = {PIPE_ROWS(1, false), PIPE_ROWS(1, true), PIPE_ROWS(2, false), PIPE_ROWS(2, true),
                                                        {TRWS_SWEEP_VARIANTS(PIPE_SPEC_ENTRY)}};
static const SweepRow kPipeBatchKernels[4] = {{TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_batch_kernel, 1, false)}, {TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_batch_kernel, 1, true)},
                                              {TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_batch_kernel, 2, false)}, {TRWS_SWEEP_VARIANTS(PIPE_ENTRY, trws_pipe_batch_kernel, 2, true)}};
#undef PIPE_ROWS
#undef PIPE_SPEC_ENTRY
#undef PIPE_ENTRY
static int pipe_row(int kernel, bool shared, bool group) { return ((kernel == 1 ? 0 : 1) * 2 + (shared ? 1 : 0)) * 2 + (group ? 1 : 0); }

void pipe_set_attributes() {
  set_max_dynamic_lds(kPipeKernels, kPipeSpecRow, (int)pipe_lds_bytes());
  set_max_dynamic_lds(kPipeKernels + kPipeSpecRow, 1, (int)pipe_spec_lds_bytes());
  set_max_dynamic_lds(kPipeBatchKernels, 4, (int)pipe_batch_lds_bytes());
}

void launch_pipe(int kernel, bool shared, int what, int blocks, hipStream_t s, const DevParams &p, int epoch) {
  // the speculative schedule's kernel (the runner's LDS lies behind the visits')
  if (p.spec_kind[0] != nullptr && p.spec_kind[1] != nullptr && kernel == 1 && shared)
    return launch_sweep(kPipeKernels[kPipeSpecRow], what, blocks, kPipeThreads, pipe_spec_lds_bytes(), s, p, epoch);
  launch_sweep(kPipeKernels[pipe_row(kernel, shared, false)], what, blocks, kPipeThreads, pipe_lds_bytes(), s, p, epoch);
}
void launch_pipe_group(int kernel, bool shared, int what, int blocks, hipStream_t s, const GroupArgs &ga, int epoch) {
  // (strips keep the plain chain schedule)
  launch_sweep(kPipeKernels[pipe_row(kernel, shared, true)], what, blocks, kPipeThreads, pipe_lds_bytes(), s, ga, epoch);
}
void launch_pipe_batch(int kernel, bool shared, int what, int blocks, hipStream_t s, const BatchArgs &ba, int epoch) {
  launch_sweep(kPipeBatchKernels[pipe_row(kernel, shared, false) / 2], what, blocks, kPipeThreads, pipe_batch_lds_bytes(), s, ba, epoch);
}
int pipe_batch_resident_per_cu(int kernel, bool shared) {
  // (the backward sweep's kernel: the variants of a row differ by a few registers at most, and a share that is
  //  not resident at once only starts later -- tickets are drawn by workgroups that run)
  int per_cu = 0;
  STEREO_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kPipeBatchKernels[pipe_row(kernel, shared, false) / 2][1], kPipeThreads,
                                                                 pipe_batch_lds_bytes()));
  return per_cu > 0 ? per_cu : 1;
}

}  // namespace stereo
