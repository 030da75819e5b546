// Host-side graph analysis for the TRW-S path (product code, C++).
//
// Produces, for an arbitrary directed edge list, exactly the node order, edge
// orientation and per-node forward/backward edge lists that the reference
// builds in MRFEnergy::AddEdge (cpp/trw-s/MRFEnergy.cpp:83-111),
// SetAutomaticOrdering (cpp/trw-s/ordering.cpp:7-157) and
// CompleteGraphConstruction (cpp/trw-s/MRFEnergy.cpp:137-229), plus the
// dependency levels of that order that the level-synchronous HIP sweeps run on.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stereo {

struct TrwsGraph {
  int64_t N = 0, E = 0;
  // per edge, after orientation: tail has the lower rank
  std::vector<int32_t> tail, head;
  std::vector<uint8_t> mdir;  // Swap() parity (typeStereoLinear.h:318-321)
  // node order
  std::vector<int32_t> order;  // order[r] = node id
  std::vector<int32_t> rank;   // rank[node]
  // per RANK r: forward / backward edge ids in the reference's list order (CSR)
  std::vector<int32_t> fptr, fidx, bptr, bidx;
  std::vector<double> gamma;  // per rank: 1/max(nFwd,nBwd) (treeProbabilities.cpp:24-45)
  // dependency levels of the forward sweep (longest path over backward edges)
  std::vector<int32_t> level_ptr;    // size L+1
  std::vector<int32_t> level_ranks;  // ranks grouped by level, ascending rank inside
  int64_t max_level_nodes = 0;
  // position of every lower-bound term in the reference's summation order
  // (minimize.cpp:67-95: node minimum, then one term per backward edge, nodes
  // visited in descending rank); energy terms are simply indexed by rank.
  std::vector<int32_t> lb_pos_node;  // per rank
  std::vector<int32_t> lb_pos_edge;  // per edge
  int64_t lb_terms = 0;

  // Row strips (multi-GPU): owner[node] = strip that visits the node; empty = one strip.  Strips
  // form a chain: every edge joins nodes of the same strip or of strips g, g+1.  With strips the
  // positions above are STRIP-LOCAL (every strip sums its own terms, in the reference's order
  // restricted to its nodes; the partial sums are combined in strip order), runs never cross a
  // strip boundary, and the descriptors say which outgoing messages / flags / labels go to the
  // neighbouring strip's memory.
  std::vector<int32_t> owner;            // per NODE
  int nstrips = 1;
  std::vector<int64_t> strip_lb_terms;   // per strip
  std::vector<int64_t> strip_nodes;      // per strip
  std::vector<int32_t> e_pos;            // per rank: position of the node's energy term in its strip

  // Schedule of the persistent dataflow sweeps.  Processing position p is rank p
  // in the forward sweep and rank N-1-p in the backward sweep.  A "run" is a
  // maximal stretch of consecutive positions in which every node has its
  // predecessor among its incoming neighbours (a grid row, the border chain):
  // one workgroup walks a run sequentially, hands the messages for the next
  // node over in LDS and waits on completion flags only for `dep_rank`.
  struct Sweep {
    std::vector<int32_t> run_ptr;   // R+1 offsets into processing positions
    // order in which workgroups pick runs up (ticket -> run); empty = 0, 1, 2, ...
    std::vector<int32_t> run_order;
    std::vector<int32_t> dep_ptr;   // N+1, indexed by rank
    std::vector<int32_t> dep_rank;  // ranks whose flag must be set first
    // aligned with the node's INCOMING list (bidx forward / fidx backward):
    // slot of that edge in the predecessor's outgoing list, or -1
    std::vector<int8_t> in_slot;
    // Packed per-position descriptors for the fast kernels (kDescWords int32 each,
    // layout below: kDescNode ...); empty unless fast_ok.  They are laid out in the order of
    // the CHAIN schedule below, which is what the descriptor-driven kernels walk.
    std::vector<int32_t> desc;
    // Chain schedule of the fast kernels: a run is a path of the dependency DAG (every node
    // hangs on the node visited just before it), not necessarily a stretch of consecutive
    // ranks -- the reference order interleaves the ranks of the last two grid rows, which a
    // rank-contiguous run would walk as ONE serial chain of 2W visits.  chain_rank maps a
    // schedule position to the rank visited there; chain_run_ptr / chain_run_order are the
    // counterparts of run_ptr / run_order over schedule positions.
    std::vector<int32_t> chain_rank, chain_run_ptr, chain_run_order;
    // strip that owns each run of the rank-contiguous / chain schedule (empty with one strip)
    std::vector<int32_t> run_strip, chain_run_strip;
    // Speculative schedule.  The image grid's border chain is ONE run of 2(H+W)-4 strictly
    // serial visits during most of which nothing else can run.  What makes it serial is a single row per
    // visit -- the message a node hands to the next one -- and that row is plain min-plus of the previous
    // one whenever the certificate holds.  So the run is cut into segments of `seg_len` visits; a RUNNER
    // (one wave of one workgroup) walks the whole run computing nothing but that recurrence, uncertified,
    // and leaves the row at every cut; the segments -- ordinary runs, every visit exact and certified --
    // start from the runner's rows side by side on as many workgroups, hold their completion flags back,
    // and COMMIT in order: a segment compares the rows it started from with what the segment in front
    // really produced (bit for bit) and walks its visits a second time if they differ.  By induction every
    // committed value is the sequential sweep's.  The schedule below is the chain schedule with that one
    // run replaced by a runner ticket + its segments; descriptors are shared (the kernel treats the first
    // visit of a segment differently, nothing in the descriptor says so).
    struct Spec {
      bool ok = false;
      int32_t run = -1;                  // the run of the chain schedule that is cut
      int32_t c0 = 0, c1 = 0;            // its schedule positions
      int32_t seg_len = 0, nseg = 0, max_len = 0;
      std::vector<int32_t> run_ptr;      // CSR over schedule positions, the cut run as nseg runs
      std::vector<int32_t> run_order;    // ticket -> run; -1: the runner's ticket (ticket 0)
      std::vector<int32_t> kind;         // per run: 0, or 1 + segment index
    } spec;
    // Sub-row runs: the chain schedule with every ordinary run longer than `chunk` positions cut into
    // consecutive runs of at most that many, so that a workgroup is held for a piece of a grid row and not for the
    // whole of it.  Same positions (chain_rank), other runs, tickets and descriptors: a piece's first node waits for the
    // last node of the piece in front like for any other foreign node.  The speculative schedule's cut run stays whole;
    // `spec` is that schedule over these runs.  Built on request for one direction at a time (TrwsGraphOptions:
    // row_chunk_forward / row_chunk_backward), kept only where the checks of the chain schedule hold on it.
    struct Chunked {
      bool ok = false;
      int32_t chunk = 0;
      std::vector<int32_t> desc, run_ptr, run_order;   // as desc / chain_run_ptr / chain_run_order (run_order: never empty)
      Spec spec;
    } chunked;
  } sweep[2];
  static constexpr int kDescWords = 64;
  // every node has <= 8 incident edges and <= 4 foreign dependencies per direction, and the loader protocol
  // terminates on both chain schedules (trws_graph_desc.cpp); false: the generic kernel takes the graph
  bool fast_ok = false;
  static constexpr int kMaxSlots = 8;
};

// What build_trws_graph is asked for besides the connectivity.  Everything that changes the result is a member, so a
// cache of graphs (trws_plan_create.hip) compares keys with the one operator== below and cannot miss an option.
struct TrwsGraphOptions {
  // > 0: if a sweep has more runs than that, cut runs in front of nodes that wait long for a foreign node and
  // dispense them in dependency-level order (trws_graph.cpp: contiguous_runs, trws_graph_schedule.cpp: chain_runs)
  int64_t max_resident_runs = 0;
  const int32_t *owner = nullptr;     // N entries, values 0 .. nstrips-1, or nullptr: see TrwsGraph::owner
  int nstrips = 1;
  int64_t certainly_resident = 256;   // workgroups sure to be resident whatever the kernel's LDS use (the CU count)
  // 0 = SetAutomaticOrdering (ordering.cpp:7-157, what the gateway calls, trws_mex.cpp:121);
  // 1 = node index order, MRFEnergy's order when SetAutomaticOrdering is not called (nodes in the
  // order they were added, MRFEnergy.cpp:37-76).  On the image grid: H + W - 1 anti-diagonal levels,
  // no serial border chain.  Another valid TRW-S schedule, not the gateway's results.
  int ordering = 0;
  // row_chunk_forward > 0: also build Sweep::chunked with runs of at most that many positions, in every direction that
  // has more runs than chunk_resident workgroups (those certain to be resident in the launch that will walk them);
  // row_chunk_backward >= 0: the backward sweep's own length (0: whole rows there).
  int64_t row_chunk_forward = 0, row_chunk_backward = -1, chunk_resident = 0;
  // visits per segment of the speculative schedule; 0: spec_segment_length(), read once per build
  int seg_len = 0;
};
// (owner is compared by the one who keeps the arrays: by content, not by address)
inline bool operator==(const TrwsGraphOptions &a, const TrwsGraphOptions &b) {
  return a.max_resident_runs == b.max_resident_runs && a.nstrips == b.nstrips && a.certainly_resident == b.certainly_resident &&
         a.ordering == b.ordering && a.row_chunk_forward == b.row_chunk_forward && a.row_chunk_backward == b.row_chunk_backward &&
         a.chunk_resident == b.chunk_resident && a.seg_len == b.seg_len;
}

// conn: 2 x E zero-based (column major: conn[2e] = tail, conn[2e+1] = head).
// Returns false and sets `err` on invalid input.
bool build_trws_graph(int64_t N, int64_t E, const uint32_t *conn, const TrwsGraphOptions &opt, TrwsGraph &g, std::string &err);
// visits per segment of the speculative schedule (STEREO_HIP_TRWS_SPEC_SEG, default 16)
int spec_segment_length();

// ticket -> run of a schedule's ticket order (run_order, chain_run_order, Chunked::run_order): empty = 0, 1, 2, ...
inline int32_t run_of_ticket(const std::vector<int32_t> &order, int64_t t) { return order.empty() ? (int32_t)t : order[(size_t)t]; }

// The descriptor of one visit: kDescWords int32, decoded on the device by decode_desc (trws_dev.h: NodeDesc).
//   word 0: node id            word 1: rank (the index of the node's completion flag)
//   word 2: counts, see desc_pack            word 3: position of the node's lower-bound term (lb_pos_node)
//   words 4-11:  edge ids, the n_out outgoing ones first, then the n_in incoming ones (k below: index in this list)
//   words 12-19: per edge k: slot of an incoming edge in the outgoing list of the node visited one (0..7) or two
//                (8..15) steps earlier in the same run, which hands the row over in LDS; -1: none
//   words 20-23: ranks of the foreign dependencies (completion flags waited for)
//   words 24-31: per outgoing edge k: position of its lower-bound term (lb_pos_edge)
//   words 32-39: per incoming edge k: the node at its other end (its label feeds the primal)
//   word 40: completion flags are raised in the middle of the next visit (1) or lazily at the run's end (0)
//   words 41, 42: words 12-19 once more, one byte each (0xff = none), for the compute waves
constexpr int kDescNode = 0, kDescRank = 1, kDescCounts = 2, kDescLbNode = 3, kDescEdge = 4, kDescSlot = 12, kDescDep = 20,
              kDescLbEdge = 24, kDescOther = 32, kDescEager = 40, kDescSlotBytes = 41;
constexpr int kMaxDeps = 4;   // foreign dependencies a descriptor holds
// word 2: n_out | n_in << 4 | dependencies << 8 | bit 12 (a loader may wait for the node's dependencies two visits
// ahead, trws_graph_desc.cpp: describe_visit) | Swap() parity of edge k << (16 + k)
inline int32_t desc_pack(int nout, int nin, int ndep, bool ahead, uint32_t mdir) {
  return (int32_t)((uint32_t)nout | ((uint32_t)nin << 4) | ((uint32_t)ndep << 8) | ((uint32_t)ahead << 12) | (mdir << 16));
}
inline int desc_nout(const int32_t *D) { return D[kDescCounts] & 15; }
inline int desc_nin(const int32_t *D) { return (D[kDescCounts] >> 4) & 15; }
inline int desc_ndep(const int32_t *D) { return (D[kDescCounts] >> 8) & 15; }
inline bool desc_ahead(const int32_t *D) { return (D[kDescCounts] >> 12) & 1; }
inline uint32_t desc_mdir(const int32_t *D) { return ((uint32_t)D[kDescCounts] >> 16) & 255; }

// Descriptor words added for strips
//   word 43: bits 0-7 outgoing message k goes to the neighbouring strip; bits 8-15 which one
//            (0 = previous strip, 1 = next strip); bit 16 / 17: flag (+ label) also raised in the
//            previous / next strip's memory
//   word 44: TrwsGraph::e_pos of the node
constexpr int kDescRemote = 43, kDescEpos = 44;
//   words 45-52: with strip-local storage, the id of outgoing edge k in the neighbouring strip's
//            numbering (valid where bit k of word 43 is set)
//   words 53, 54: the node's id in the previous / next strip's numbering (bits 16 / 17 of word 43)
constexpr int kDescPeerEdge = 45, kDescPeerNode = 53;
//   word 55: bits 0-7: edge k of the node's list (k >= n_out: an incoming edge) brings its message from GLOBAL memory --
//            the other end was not visited one or two steps earlier in the same run, so a loader fetches the row (and
//            that node's label) behind the node's completion flag
constexpr int kDescFetch = 55;
//   word 56: nibble k: the outgoing message that goes to the same neighbour as outgoing message k (k itself: none)
constexpr int kDescTwin = 56;
//   word 57: the tagged-granule hand-over between two ordinary runs (trws_pipe.hip) --
//            bits 0-7:   incoming row k (a bit of word 55) arrives as granules in slot "edge id of row k" of the
//                        granule array, not behind the other end's completion flag
//            bits 8-15:  outgoing message k is published as granules as soon as it is final
//            bit 20:     the node publishes its label as a granule (primal sweeps; set with any bit 8-15)
//            bits 16-19: which of the dependencies (words 20-23) are still waited for by their flags, with
//                        granules on (the others only feed rows of bits 0-7)
//            Marked only where both ends are ordinary runs of the same sweep (no segment of the speculative
//            schedule, not its runner, no strips) and the producer's run draws the earlier ticket; 0 elsewhere.
constexpr int kDescGran = 57;

// Strip-local storage.  A strip keeps arrays only for what it touches: its own nodes, the nodes
// one edge away (whose flags it waits on and whose labels its primal pass reads), and the edges
// with an own endpoint.  Local ids: own nodes in ascending global id, then the halo nodes in
// ascending global id; edges in ascending global id.  A flag is indexed by the local NODE id.
// The descriptors of the strip's own visits are renumbered accordingly and laid out run after
// run in ticket order, so the kernels see an ordinary single-strip problem of the local size
// plus the peer ids of words 45-54.
struct StripLayout {
  int64_t n_own = 0;
  std::vector<int32_t> nodes, edges;  // local id -> global id
  std::vector<int32_t> desc[2], run_ptr[2];
  bool need_peer[2] = {false, false};
};
bool build_strip_layout(const TrwsGraph &g, int strip, StripLayout &out, std::string &err);

// What the two belief kernels (trws_beliefs.hip) walk on a strip: its own nodes in rank order as
// strip-local ids, and per such node the firstForward / firstBackward lists as strip-local edge ids in the GLOBAL
// list order (a belief is a sequence of fp64 adds in that order).  Every listed edge has an own endpoint, so it
// has a local id.  nodes / edges: the strip's local -> global ids (StripLayout); one strip (g.nstrips == 1, no
// owner table): the whole problem's lists, ids unchanged.
struct StripBeliefLists {
  std::vector<int32_t> own, fptr, fidx, bptr, bidx;
};
bool build_strip_belief_lists(const TrwsGraph &g, int strip, const std::vector<int32_t> &nodes, const std::vector<int32_t> &edges,
                              StripBeliefLists &out, std::string &err);

}  // namespace stereo
