// QPBO roof duality, host-side graph code (no HIP call): pair grouping, the doubled graph, weak persistency,
// the grid hint.  See qpbo_maxflow.hip for the construction and the references into QPBO v1.3.
#include "qpbo_host.h"

#include <algorithm>
#include <numeric>

namespace stereo {

bool group_pairs(const uint32_t *conn, int64_t N, int64_t E, PairGroups &G, std::string &err) {
  if (2 * N >= INT32_MAX / 2 || E >= INT32_MAX / 4) { err = "stereo_rd: problem too large for 32-bit ids"; return false; }
  for (int64_t e = 0; e < E; ++e) {
    const uint32_t a = conn[2 * e], b = conn[2 * e + 1];
    if (a >= (uint64_t)N || b >= (uint64_t)N) { err = "connectivity index out of range"; return false; }
    if (a == b) { err = "stereo_rd: self loops are not supported"; return false; }
  }
  // merge parallel / antiparallel edges: key (lo, hi), the edges of a pair stay in input order
  std::vector<int64_t> order(E);
  std::iota(order.begin(), order.end(), 0);
  auto key = [&](int64_t e) {
    const uint32_t a = conn[2 * e], b = conn[2 * e + 1];
    return ((uint64_t)std::min(a, b) << 32) | std::max(a, b);
  };
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
  G.pi.clear(); G.pj.clear(); G.pe_ptr.clear();
  G.pe_edge.assign(E, 0);
  for (int64_t k = 0; k < E; ++k) {
    const int64_t e = order[k];
    const uint32_t a = conn[2 * e], b = conn[2 * e + 1];
    const int32_t lo = (int32_t)std::min(a, b), hi = (int32_t)std::max(a, b);
    if (G.pi.empty() || G.pi.back() != lo || G.pj.back() != hi) { G.pi.push_back(lo); G.pj.push_back(hi); G.pe_ptr.push_back((int32_t)k); }
    G.pe_edge[k] = (int32_t)(e * 2 + ((int32_t)a == lo ? 0 : 1));
  }
  G.pe_ptr.push_back((int32_t)E);
  return true;
}

namespace {

// QPBO.h:760-807
inline void compute_weights(double A, double B, double C, double D, double &ci, double &cj, double &cij,
                            double &cji) {
  ci = D - A;
  B -= A;
  C -= D;
  if (B < 0) { ci += -B; cj = B; cji = B + C; cij = 0; }
  else if (C < 0) { ci += C; cj = -C; cij = B + C; cji = 0; }
  else { cj = 0; cij = B; cji = C; }
}

}  // namespace

bool build_problem(const double *U0, const double *U1, const double *E00, const double *E01,
                   const double *E10, const double *E11, const uint32_t *conn, int64_t N, int64_t E,
                   QpboProblem &P, std::string &err) {
  if (N <= 0) { err = "stereo_rd: no nodes"; return false; }
  PairGroups G;
  if (!group_pairs(conn, N, E, G, err)) return false;
  P.N = N;
  const int64_t n = 2 * N, np = G.npairs();
  P.tr.assign(n, 0.0);
  P.pair_super.assign(np, 0);
  double const0 = 0;
  std::vector<int32_t> deg(n + 1, 0);
  struct ArcTmp { int32_t tail, head; double cap; };
  std::vector<ArcTmp> arcs;
  arcs.reserve(4 * np);
  for (int64_t k = 0; k < np; ++k) {
    // the pair's tables oriented lo -> hi, summed in input order
    double A = 0, B = 0, C = 0, D = 0;
    for (int32_t q = G.pe_ptr[k]; q < G.pe_ptr[k + 1]; ++q) {
      const int64_t e = G.pe_edge[q] >> 1;
      // first index of the table = label of conn(0,e) (rd_mex.cpp:59)
      if (G.pe_edge[q] & 1) { A += E00[e]; B += E10[e]; C += E01[e]; D += E11[e]; }
      else { A += E00[e]; B += E01[e]; C += E10[e]; D += E11[e]; }
    }
    double ci, cj, cij, cji;
    const int32_t i = G.pi[k], j = G.pj[k], im = i + (int32_t)N, jm = j + (int32_t)N;
    if (B + C >= A + D) {  // QPBO.cpp:434
      compute_weights(A, B, C, D, ci, cj, cij, cji);
      const0 += A;  // constant of the normal form
      P.tr[i] += ci; P.tr[j] += cj;
      arcs.push_back({i, j, cij}); arcs.push_back({j, i, cji});
      arcs.push_back({jm, im, cij}); arcs.push_back({im, jm, cji});
    } else {
      P.pair_super[k] = 1;
      compute_weights(B, A, D, C, ci, cj, cij, cji);
      // normal form of phi(x_i, y) = theta(x_i, 1 - y): constant theta(0,1), and the unary
      // cj * y = cj - cj * x_j contributes cj to the constant as well
      const0 += B + cj;
      P.tr[i] += ci; P.tr[j] -= cj;
      arcs.push_back({i, jm, cij}); arcs.push_back({jm, i, cji});
      arcs.push_back({j, im, cij}); arcs.push_back({im, j, cji});
    }
  }
  for (int64_t u = 0; u < N; ++u) {
    P.tr[u] += U1[u] - U0[u];  // QPBO.h:615-624
    const0 += U0[u];
  }
  for (int64_t u = 0; u < N; ++u) P.tr[u + N] = -P.tr[u];  // QPBO.cpp:689
  P.const0 = const0;
  // group arcs by tail (counting sort), remember where each arc's reverse lands
  const int64_t m = (int64_t)arcs.size();
  for (const ArcTmp &a : arcs) ++deg[a.tail + 1];
  P.aptr.assign(n + 1, 0);
  for (int64_t v = 0; v < n; ++v) P.aptr[v + 1] = P.aptr[v] + deg[v + 1];
  std::vector<int32_t> fill(P.aptr.begin(), P.aptr.end() - 1), newid(m);
  for (int64_t a = 0; a < m; ++a) newid[a] = fill[arcs[a].tail]++;
  P.head.resize(m); P.cap.resize(m); P.rev.resize(m);
  for (int64_t a = 0; a < m; ++a) {
    P.head[newid[a]] = arcs[a].head;
    P.cap[newid[a]] = arcs[a].cap;
    P.rev[newid[a]] = newid[a ^ 1];
  }
  return true;
}

namespace {

// The two DFS passes of the weak persistency (Kosaraju) over an "arc view" of M nodes:
//   V.arcs(t)     number of arc slots of node t
//   V.head(t, k)  head of t's k-th arc, or -1 (no arc there / a head outside the view)
//   V.fwd(t, k), V.bwd(t, k)   residual capacity on that arc / on its reverse
// Nodes with fixed[t] are not visited.  Returns the component number of every free node (from 1, in the order the
// second pass meets them; 0 for fixed nodes).  The component numbering among INCOMPARABLE components follows
// the node and arc order of the view, not the reference's linked-list order (those labels are an artefact of DFS
// order there too): both views below present the free nodes and their arcs in the same order.
template <class View>
std::vector<int32_t> free_components(const View &V, int64_t M, const std::vector<uint8_t> &fixed) {
  std::vector<int32_t> region(M, 0), parent(M, 0), cursor(M, 0);
  std::vector<uint8_t> seen(fixed);
  for (int64_t t = 0; t < M; ++t)
    if (!fixed[t]) region[t] = -1;
  std::vector<int32_t> stack;  // finish order
  for (int64_t s = 0; s < M; ++s) {
    if (seen[s]) continue;
    int32_t i = (int32_t)s;
    seen[i] = 1; parent[i] = i; cursor[i] = 0;
    for (;;) {
      if (cursor[i] == V.arcs(i)) {
        stack.push_back(i);
        if (parent[i] == i) break;
        i = parent[i];
        ++cursor[i];
        continue;
      }
      const int32_t j = V.head(i, cursor[i]);
      if (j < 0 || !V.fwd(i, cursor[i]) || seen[j]) { ++cursor[i]; continue; }
      seen[j] = 1; parent[j] = i; i = j; cursor[i] = 0;
    }
  }
  int component = 0;
  for (int64_t k = (int64_t)stack.size() - 1; k >= 0; --k) {
    int32_t i = stack[k];
    if (region[i] > 0) continue;
    region[i] = ++component; parent[i] = i; cursor[i] = 0;
    for (;;) {
      if (cursor[i] == V.arcs(i)) {
        if (parent[i] == i) break;
        i = parent[i];
        ++cursor[i];
        continue;
      }
      const int32_t j = V.head(i, cursor[i]);
      if (j < 0 || !V.bwd(i, cursor[i]) || region[j] >= 0) { ++cursor[i]; continue; }
      parent[j] = i; i = j; cursor[i] = 0; region[i] = component;
    }
  }
  return region;
}

// x = 0 if the node's component comes after its mate's, 1 if before, else still unlabelled
inline int weak_label(int32_t region_node, int32_t region_mate) {
  return region_node > region_mate ? 0 : (region_node < region_mate ? 1 : -1);
}

// the CSR residual network: every node of the doubled graph, the labelled ones fixed
struct CsrArcView {
  const QpboProblem &P;
  const std::vector<double> &r;
  int32_t arcs(int32_t t) const { return P.aptr[t + 1] - P.aptr[t]; }
  int32_t head(int32_t t, int32_t k) const { return P.head[P.aptr[t] + k]; }
  bool fwd(int32_t t, int32_t k) const { return r[P.aptr[t] + k] > 0; }
  bool bwd(int32_t t, int32_t k) const { return r[P.rev[P.aptr[t] + k]] > 0; }
};

// the gathered free subgraph: `maxdeg` slots per local node, heads already mapped to local ids
struct GatheredArcView {
  int32_t maxdeg;
  const std::vector<int32_t> &loc;
  const std::vector<uint8_t> &flags;
  int32_t arcs(int32_t) const { return maxdeg; }
  int32_t head(int32_t t, int32_t k) const { return loc[(size_t)t * maxdeg + k]; }
  bool fwd(int32_t t, int32_t k) const { return flags[(size_t)t * maxdeg + k] & 1; }
  bool bwd(int32_t t, int32_t k) const { return flags[(size_t)t * maxdeg + k] & 2; }
};

}  // namespace

void weak_persistencies(const QpboProblem &P, const std::vector<double> &r, std::vector<int> &label) {
  const int64_t N = P.N, n = 2 * N;
  std::vector<uint8_t> fixed(n, 1);
  bool any = false;
  for (int64_t i = 0; i < N; ++i)
    if (label[i] < 0) { fixed[i] = fixed[i + N] = 0; any = true; }
  if (!any) return;
  const std::vector<int32_t> region = free_components(CsrArcView{P, r}, n, fixed);
  for (int64_t i = 0; i < N; ++i)
    if (label[i] < 0) label[i] = weak_label(region[i], region[i + N]);
}

void weak_persistencies_compact(int cnt, int N, const std::vector<int32_t> &ids, int maxdeg,
                                const std::vector<int32_t> &heads, const std::vector<uint8_t> &flags,
                                std::vector<int8_t> &lab) {
  const int M = 2 * cnt;
  std::vector<int32_t> loc((size_t)M * maxdeg, -1);   // local index of every arc's head, -1: not free / no arc
  for (int t = 0; t < M; ++t)
    for (int k = 0; k < maxdeg; ++k) {
      const int32_t w = heads[(size_t)t * maxdeg + k];
      if (w < 0) continue;
      const int32_t var = w >= N ? w - N : w;
      const auto it = std::lower_bound(ids.begin(), ids.end(), var);
      if (it != ids.end() && *it == var) loc[(size_t)t * maxdeg + k] = (int32_t)(it - ids.begin()) + (w >= N ? cnt : 0);
    }
  const std::vector<int32_t> region = free_components(GatheredArcView{maxdeg, loc, flags}, M, std::vector<uint8_t>(M, 0));
  lab.assign(cnt, -1);
  for (int t = 0; t < cnt; ++t) lab[t] = (int8_t)weak_label(region[t], region[t + cnt]);
}

int64_t grid_height_of(const uint32_t *conn, int64_t N, int64_t E) {
  int64_t H = 0;
  for (int64_t e = 0; e < E; ++e) {
    const int64_t a = conn[2 * e], b = conn[2 * e + 1], d = a < b ? b - a : a - b;
    if (d == 1) continue;
    if (H == 0) H = d;
    if (d != H) return 0;
  }
  if (H < 2 || N % H != 0) return 0;
  for (int64_t e = 0; e < E; ++e) {
    const int64_t a = conn[2 * e], b = conn[2 * e + 1], lo = a < b ? a : b, d = a < b ? b - a : a - b;
    if (d == 1 && lo % H == H - 1) return 0;
  }
  return H;
}

}  // namespace stereo
