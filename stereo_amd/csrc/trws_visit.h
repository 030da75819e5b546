// The run and visit frame of the pipelined TRW-S sweep kernels (trws_pipe.hip, trws_pipe2.hip, trws_wide.hip): how a
// workgroup draws a run, and how each of its roles walks positions p0 - 1 .. p1 of that run with one barrier per visit.
//
// Everything here is a MACRO, on purpose.  These kernels sit at the scalar-register limit: the same statements moved
// into a __forceinline__ function change the register allocation of every kernel (pipe2's epilogue as a function: 76 ->
// 84 spilled SGPRs on the backward sweep).  Textual sharing leaves the device assembly as it was, line for line, and
// that is how a change to these files is checked: tools/isa_compare.py on the saved assembly of the parent and of the
// change, every kernel `same`.
//
// The macros use the names of the bodies they expand in: p, tid, wave, D, SPEC, have_ticket (run frame); p0, p1 (visit
// frame).  They declare run, second_walk, p0, p1, seg, spec_in, and per visit pos, st, stn, hcur, hprev, sc, have_node.
#pragma once

#include "trws_dev.h"

// ---- the run frame: the head of the body of a kernel's `for (;;)` over runs ------------------------------------------
// One lane draws the next ticket into CTL[0] unless the workgroup HOLDS a run already (the speculative kernels: the
// first ticket, drawn before the visit loops exist, or CTL[3] -- the workgroup walks the speculative segment it holds a
// second time).
#define TRWS_DRAW_TICKET(CTL, HOLDS) \
    if (tid == 0 && !(HOLDS)) (CTL)[0] = next_run<D>(p);
// Everybody reads the run behind a barrier; CLEAR (statements, may be empty) runs between the two barriers, where every
// wave is behind the last visit's barrier and nothing is being published or collected.  SPEC_: whether this kernel
// knows the speculative schedule (run -1 is the runner's ticket, served before the loop).  Leaves the loop over runs
// when the tickets are used up.
#define TRWS_RUN_ENTER(SPEC_, CTL, CLEAR) \
    __syncthreads(); \
    const int run = __builtin_amdgcn_readfirstlane((CTL)[0]); \
    const int second_walk = (SPEC_) ? __builtin_amdgcn_readfirstlane((CTL)[3]) : 0; \
    (void)second_walk; \
    CLEAR \
    __syncthreads(); \
    if ((SPEC_) && tid == 0) (CTL)[3] = 0; \
    if (run >= p.nruns[D]) break; \
    if ((SPEC_) && run < 0) continue;   /* (the runner's ticket is ticket 0: drawn and served above) */ \
    const int p0 = p.run_ptr[D][run], p1 = p.run_ptr[D][run + 1];
// A segment of the speculative schedule (trws_graph.h: Sweep::Spec): its first visit takes what the node in front hands
// over from the runner's rows (spec_in; a second walk takes the same rows from the messages themselves: the segment in
// front has committed), its completion flags wait for the commit below the visit loops.  seg = -1: an ordinary run.
#define TRWS_SPEC_SEGMENT \
    const int seg = (SPEC && p.spec_kind[D]) ? __builtin_amdgcn_readfirstlane(p.spec_kind[D][run]) - 1 : -1; \
    const bool spec_in = SPEC && seg > 0 && !second_walk; \
    (void)spec_in;

// ---- the member frame: one level above the run frame (trws_pipe_batch_kernel; stereo_trws_batch_*) ------
// A launch that serves several INDEPENDENT problems from one table of parameter blocks.  The ticket draw gets one more
// level: a workgroup draws the tickets of the member HOME names until none is left (the run frame's own exit), then those
// of the next member of the table, once round.  It enters a member only through that member's ticket counter, so inside
// every member tickets are still handed out in schedule order to workgroups that run -- what every wait relies on.
// Between BEGIN and END stands the call of the kernel body with the member's parameter block, `member` its index:
// the body reads the block from the table and sets up everything it keeps per problem anew.  CTL: the body's control
// words; [1] != 0: a wait gave up -- the workgroup ends, wave by wave, as it does in a launch of one problem (no barrier
// behind a body that some waves have left early); [2]: the body held a run of this member.  BA.ctl[0] counts the
// workgroups that held runs of more than one member.  STATE: three ints of LDS behind the body's own -- what the frame
// keeps across a body lives there, not in registers the visit loops would have to spill.
#define TRWS_MEMBERS_BEGIN(BA, HOME, STATE) \
    if (threadIdx.x == 0) { (STATE)[0] = (HOME); (STATE)[1] = 0; (STATE)[2] = 0; }   /* member, members visited, members served */ \
    __syncthreads(); \
    for (;;) { \
      const int member = __builtin_amdgcn_readfirstlane((STATE)[0]);
#define TRWS_MEMBERS_END(BA, CTL, STATE) \
      if (__hip_atomic_load((CTL) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return; \
      __syncthreads(); \
      if (threadIdx.x == 0) { \
        (STATE)[2] += (CTL)[2]; \
        (STATE)[1] += 1; \
        (STATE)[0] = (STATE)[0] + 1 < (BA).g.n ? (STATE)[0] + 1 : 0; \
      } \
      __syncthreads(); \
      if (__builtin_amdgcn_readfirstlane((STATE)[1]) >= (BA).g.n) break; \
    } \
    if (threadIdx.x == 0 && (STATE)[2] > 1) atomicAdd((BA).ctl, 1ull);

// ---- the visit frame -------------------------------------------------------------------------------------------------
// Every role walks the run in its own loop -- the same visits, the same barrier at the end of each: the hardware barrier
// counts arrivals, whichever s_barrier instruction a wave arrives at -- so that what one role keeps across visits (the
// loaders' parked requests and descriptor words, the primal wave's labels) and the kernel parameters it uses are live in
// ITS loop only: in one loop for all roles the function sat at the scalar-register limit, ~300 scalars spilled into VGPR
// lanes, and every edit anywhere moved spill code onto the compute waves' path.  A role is
//     <FAMILY>_VISITS_BEGIN  ... the role's work at position pos ...  <FAMILY>_VISITS_END
// where each family composes its pair from the pieces below.  A wave without work still walks every visit and reaches
// every barrier: BEGIN directly followed by END.
//
// TRWS_VISITS_BEGIN(OPEN, STAGE0, STAGE, RING, SCAL, LOOK): visit pos works on node pos, staged in st (stn: node
// pos + 1, being staged; two stages of STAGE doubles at STAGE0), hands messages over in hcur (RING: one of the two
// rings below), leaves its scalars in sc (two blocks at SCAL); positions p0 - 1 and p1 have no node (have_node) -- the
// loaders run one visit ahead, the storer one behind.  OPEN and LOOK: the family's profile stamps and early abort look.
#define TRWS_VISITS_BEGIN(OPEN, STAGE0, STAGE, RING, SCAL, LOOK) \
    for (int pos = p0 - 1; pos <= p1; ++pos) { \
      OPEN \
      double *st = (STAGE0) + (pos & 1) * (STAGE);          /* node `pos` */ \
      double *stn = (STAGE0) + ((pos + 1) & 1) * (STAGE);   /* node `pos + 1` */ \
      RING \
      double *sc = (SCAL) + (pos & 1) * kScalDoubles; \
      const bool have_node = pos >= p0 && pos < p1; \
      LOOK \
      (void)st; (void)stn; (void)hcur; (void)hprev; (void)sc; (void)have_node;
// the hand-over ring: the last visits' new messages, 8 rows of ROW doubles per visit -- four slots, or three with hprev2
#define TRWS_RING4(HAND, ROW) \
      double *hcur = (HAND) + (pos & 3) * 8 * (ROW), *hprev = (HAND) + ((pos - 1) & 3) * 8 * (ROW);
#define TRWS_RING3(HAND, ROW) \
      const int hb = ((pos % 3) + 3) % 3, hb1 = (((pos - 1) % 3) + 3) % 3, hb2 = (((pos - 2) % 3) + 3) % 3; \
      double *hcur = (HAND) + hb * 8 * (ROW), *hprev = (HAND) + hb1 * 8 * (ROW), *hprev2 = (HAND) + hb2 * 8 * (ROW); \
      (void)hprev2;
// The workgroup's abort word (CTL[1]: a loader's wait gave up during the PREVIOUS visit; bounded spin, the host reports
// it) is requested at the top of the visit and looked at in FRONT of the barrier that ends it: read behind that
// barrier, its LDS round trip was the first thing on every wave's path into the next visit.  (trws_pipe2.hip still
// reads it behind the barrier: TRWS_ABORT_LEAVE(ctl[1], ...) as the LATE part of its END.)
#define TRWS_ABORT_LOOK(CTL) \
      const int aborted_ = __hip_atomic_load((CTL) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#define TRWS_ABORT_LEAVE(COND, REPORT) \
      if (COND) { \
        REPORT \
        return; \
      }
// (the same where the visit loop stands in a role function of its own -- trws_pipe.hip --: the role hands VALUE back, and
//  the kernel body that called it leaves the kernel)
#define TRWS_ABORT_LEAVE_WITH(COND, REPORT, VALUE) \
      if (COND) { \
        REPORT \
        return VALUE; \
      }
// Opaque copies of the label count, renewed every visit: what is derived from them -- per-lane row bases, the
// label-count tests of the envelope code, ... -- is recomputed where it is used, one instruction each; left visible as
// loop invariants, the compiler hoists dozens of such values out of the visit loop and keeps them in spilled
// registers, scalar ones in VGPR lanes, vector ones in scratch memory.
#define TRWS_OPAQUE_K \
      int Kv = K; \
      asm volatile("" : "+s"(Kv)); \
      const int lkv = lane < Kv ? lane : Kv - 1; \
      (void)lkv;
// development profile (STEREO_HIP_TRWS_PROF): this wave's cycles from barrier to barrier arrival, summed in `busy`
#define TRWS_BUSY_OPEN \
      const long long tstart = p.prof ? (long long)__builtin_readcyclecounter() : 0;
#define TRWS_BUSY_CLOSE \
      if (p.prof) busy += (unsigned long long)((long long)__builtin_readcyclecounter() - tstart);
// TRWS_VISITS_END(CLOSE, EARLY, BARRIER, LATE): the family's closing stamps, the abort leave in front of the barrier
// (or nothing), the barrier, what follows it (a stamp, or pipe2's late abort leave).
#define TRWS_VISITS_END(CLOSE, EARLY, BARRIER, LATE) \
      CLOSE \
      EARLY \
      BARRIER; \
      LATE \
    }
