// Strip-local storage and belief lists of the TRW-S path.  See trws_graph.h.
#include "trws_graph.h"

namespace stereo {
namespace {
// local ids of strip s: node_l / edge_l are -1 where the strip holds nothing
void strip_ids(const TrwsGraph &g, int s, std::vector<int32_t> &node_l, std::vector<int32_t> &edge_l,
               std::vector<int32_t> *nodes, std::vector<int32_t> *edges, int64_t *n_own) {
  const int64_t N = (int64_t)g.owner.size(), E = (int64_t)g.tail.size();
  node_l.assign(N, -1); edge_l.assign(E, -1);
  std::vector<uint8_t> halo(N, 0);
  int32_t el = 0;
  for (int64_t e = 0; e < E; ++e) {
    const bool a = g.owner[g.tail[e]] == s, b = g.owner[g.head[e]] == s;
    if (!a && !b) continue;
    edge_l[e] = el++;
    if (edges) edges->push_back((int32_t)e);
    if (!a) halo[g.tail[e]] = 1;
    if (!b) halo[g.head[e]] = 1;
  }
  int32_t nl = 0;
  for (int64_t i = 0; i < N; ++i)
    if (g.owner[i] == s) { node_l[i] = nl++; if (nodes) nodes->push_back((int32_t)i); }
  if (n_own) *n_own = nl;
  for (int64_t i = 0; i < N; ++i)
    if (halo[i]) { node_l[i] = nl++; if (nodes) nodes->push_back((int32_t)i); }
}
}  // namespace

bool build_strip_layout(const TrwsGraph &g, int strip, StripLayout &out, std::string &err) {
  constexpr int W = TrwsGraph::kDescWords;
  out = StripLayout();
  std::vector<int32_t> node_l, edge_l, node_p[2], edge_p[2];
  strip_ids(g, strip, node_l, edge_l, &out.nodes, &out.edges, &out.n_own);
  if (strip > 0) strip_ids(g, strip - 1, node_p[0], edge_p[0], nullptr, nullptr, nullptr);
  if (strip + 1 < g.nstrips) strip_ids(g, strip + 1, node_p[1], edge_p[1], nullptr, nullptr, nullptr);
  bool sound = true;
  for (int d = 0; d < 2; ++d) {
    const TrwsGraph::Sweep &S = g.sweep[d];
    const int64_t R = (int64_t)S.chain_run_ptr.size() - 1;
    out.run_ptr[d].assign(1, 0);
    for (int64_t t = 0; t < R; ++t) {
      const int32_t run = run_of_ticket(S.chain_run_order, t);
      if (S.chain_run_strip[run] != strip) continue;
      for (int64_t q = S.chain_run_ptr[run]; q < S.chain_run_ptr[run + 1]; ++q) {
        const int32_t *G = &S.desc[(size_t)q * W];
        const size_t at = out.desc[d].size();
        out.desc[d].insert(out.desc[d].end(), G, G + W);
        int32_t *D = &out.desc[d][at];
        const int nout = desc_nout(G), nin = desc_nin(G), nd = desc_ndep(G);
        const uint32_t rem = (uint32_t)G[kDescRemote];
        D[kDescNode] = node_l[G[kDescNode]];
        D[kDescRank] = D[kDescNode];  // the flag of a node sits at its local node id
        for (int k = 0; k < 8; ++k) {
          if (k < nout + nin) D[kDescEdge + k] = edge_l[G[kDescEdge + k]];
          if (k >= nout && k < nout + nin) D[kDescOther + k] = node_l[G[kDescOther + k]];
          if (k < nout && ((rem >> k) & 1)) D[kDescPeerEdge + k] = edge_p[(rem >> (8 + k)) & 1][G[kDescEdge + k]];
        }
        for (int k = 0; k < nd && k < kMaxDeps; ++k) D[kDescDep + k] = node_l[g.order[G[kDescDep + k]]];
        if (rem & (1u << 16)) { D[kDescPeerNode] = node_p[0][G[kDescNode]]; out.need_peer[0] = true; }
        if (rem & (1u << 17)) { D[kDescPeerNode + 1] = node_p[1][G[kDescNode]]; out.need_peer[1] = true; }
        // every id the strip's kernels will use must be one the strip stores
        for (int k = 0; k < W; ++k)
          if ((k == kDescNode || k == kDescRank || (k >= kDescEdge && k < kDescEdge + nout + nin) || (k >= kDescDep && k < kDescDep + nd) ||
               (k >= kDescOther + nout && k < kDescOther + nout + nin) || k >= kDescPeerEdge) && D[k] < 0) sound = false;
      }
      out.run_ptr[d].push_back((int32_t)(out.desc[d].size() / W));
    }
  }
  if (!sound) err = "stereo_trws: a strip refers to a node or edge outside its halo (strips must be consecutive in the visiting order)";
  return sound;
}

bool build_strip_belief_lists(const TrwsGraph &g, int strip, const std::vector<int32_t> &nodes, const std::vector<int32_t> &edges,
                              StripBeliefLists &out, std::string &err) {
  out = StripBeliefLists();
  const bool whole = g.nstrips <= 1 || g.owner.empty();
  std::vector<int32_t> node_l, edge_l;
  if (!whole) {
    node_l.assign((size_t)g.N, -1); edge_l.assign((size_t)g.E, -1);
    for (size_t i = 0; i < nodes.size(); ++i) node_l[nodes[i]] = (int32_t)i;
    for (size_t e = 0; e < edges.size(); ++e) edge_l[edges[e]] = (int32_t)e;
  }
  out.fptr.assign(1, 0); out.bptr.assign(1, 0);
  bool sound = true;
  for (int64_t r = 0; r < g.N; ++r) {
    const int32_t node = g.order[r];
    if (!whole && g.owner[node] != strip) continue;
    const int32_t nl = whole ? node : node_l[node];
    if (nl < 0) sound = false;
    out.own.push_back(nl);
    for (int32_t k = g.fptr[r]; k < g.fptr[r + 1]; ++k) {
      const int32_t el = whole ? g.fidx[k] : edge_l[g.fidx[k]];
      if (el < 0) sound = false;
      out.fidx.push_back(el);
    }
    for (int32_t k = g.bptr[r]; k < g.bptr[r + 1]; ++k) {
      const int32_t el = whole ? g.bidx[k] : edge_l[g.bidx[k]];
      if (el < 0) sound = false;
      out.bidx.push_back(el);
    }
    out.fptr.push_back((int32_t)out.fidx.size());
    out.bptr.push_back((int32_t)out.bidx.size());
  }
  if (!sound) err = "stereo_trws: a strip's belief lists name a node or edge the strip does not store";
  return sound;
}

}  // namespace stereo
