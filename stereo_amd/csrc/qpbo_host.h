// QPBO roof duality, host side without any HIP call: neighbour-pair grouping, the doubled graph built on the
// host, weak persistency, labels from heights, the grid hint, the Improve permutation.  Compiles with a plain
// C++ compiler (tools/sanitize_qpbo_host.cpp runs it under the sanitizers).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stereo {

// Parallel and antiparallel edges of one neighbour pair, merged: key (lo, hi), the edges of a pair in input order.
struct PairGroups {
  std::vector<int32_t> pi, pj;   // per pair: i < j
  std::vector<int32_t> pe_ptr;   // npairs + 1: the edges of pair k are pe_edge[pe_ptr[k] .. pe_ptr[k + 1])
  std::vector<int32_t> pe_edge;  // edge id * 2 + transposed bit (the edge runs hi -> lo)
  int64_t npairs() const { return (int64_t)pi.size(); }
};

// false with `err` set: ids that do not fit 32 bits, an index out of range, a self loop
bool group_pairs(const uint32_t *conn, int64_t N, int64_t E, PairGroups &G, std::string &err);

struct QpboProblem {
  int64_t N = 0;
  std::vector<int32_t> aptr, head;  // doubled graph, arcs grouped by tail; reverse of a is rev[a]
  std::vector<int32_t> rev;
  std::vector<double> cap, tr;      // initial residuals, terminal capacities (2N)
  std::vector<uint8_t> pair_super;  // per pair
  double const0 = 0;                // constant of the normal form: sum E0 + sum_sub A + sum_super B
};

// Builds the doubled graph.  Arcs are sorted by tail so that the kernels can use `a` both
// as CSR position and as arc id; the reverse arc is found through `rev`.
bool build_problem(const double *U0, const double *U1, const double *E00, const double *E01, const double *E10,
                   const double *E11, const uint32_t *conn, int64_t N, int64_t E, QpboProblem &P, std::string &err);

// strong persistency (QPBO.cpp:840-844; what_segment: 1 iff in the sink tree): x_i = 1 iff i reaches the sink,
// 0 iff its mate does, `ambiguous` if both or neither
inline int label_from_heights(int hi, int hm, int n, int ambiguous) {
  const int li = hi < n ? 1 : 0, lm = hm < n ? 1 : 0;
  return li == lm ? ambiguous : li;
}

// Kosaraju pass of QPBO_postprocessing.cpp:10-120 on the unlabelled nodes and their mates, over the residual
// network `r` of P: label[i] < 0 becomes 0 or 1 where i and its mate lie in different components.
void weak_persistencies(const QpboProblem &P, const std::vector<double> &r, std::vector<int> &label);

// The same pass on the free subgraph alone (rd_free_arcs_kernel): local node t < cnt is variable ids[t] (ascending),
// t >= cnt its mate; `maxdeg` arc slots per node in the order of the arc lists, head -1 = no arc, flag bit 0 / 1 =
// residual capacity on the arc / on its reverse.  lab[t]: new label of variable ids[t], the same as the full pass gives.
void weak_persistencies_compact(int cnt, int N, const std::vector<int32_t> &ids, int maxdeg, const std::vector<int32_t> &heads,
                                const std::vector<uint8_t> &flags, std::vector<int8_t> &lab);

// H if the edges are exactly those of a 4-connected H x W image numbered col * H + row (any order, either
// direction, no edge across a column end), else 0: the work-partition hint of stereo_rd_plan_set_grid.
int64_t grid_height_of(const uint32_t *conn, int64_t N, int64_t E);

// The permutation of QPBO::Improve (QPBO_extra.cpp:13-27), drawn from libc rand() (qpbo_rand.cpp)
std::vector<int32_t> improve_permutation(int64_t N);

}  // namespace stereo
