// The runner's chain records (trws_runner_records.h): the derivation the loaders of trws_spec.h made on the device on
// every sweep until round 12, written once on the host.
#include "trws_runner_records.h"

#include <cstring>

#include "trws_graph.h"

namespace stereo {

void build_runner_records(const int32_t *desc, int32_t c0, int32_t c1, int32_t seg_len, int32_t nseg, std::vector<int32_t> &out) {
  constexpr int DW = TrwsGraph::kDescWords;
  out.assign(c1 > c0 ? (size_t)(c1 - c0) * kRecWords : 0, 0);
  const int32_t none[DW] = {};
  for (int32_t i = c0; i < c1; ++i) {
    const int32_t *w = desc + (size_t)i * DW, *wn = i + 1 < c1 ? desc + (size_t)(i + 1) * DW : none;
    int32_t *R = out.data() + (size_t)(i - c0) * kRecWords;
    const uint32_t f = (uint32_t)w[kDescCounts], fn = (uint32_t)wn[kDescCounts];
    const int nout = f & 15, nin = (f >> 4) & 15, ndep = (f >> 8) & 15, md = (f >> 16) & 255, ntot = nout + nin;
    const int noutn = fn & 15, ntotn = noutn + ((fn >> 4) & 15);
    // rows the node in front hands over (this node's and, for the messages to compute here, the next node's)
    uint32_t fr = 0, frn = 0;
    for (int k = 0; k < 8; ++k) {
      if (i > c0 && k >= nout && k < ntot && w[kDescSlot + k] >= 0) fr |= 1u << k;
      if (i + 1 < c1 && k >= noutn && k < ntotn && wn[kDescSlot + k] >= 0) frn |= 1u << k;
    }
    const int kfirst = fr ? __builtin_ctz(fr) : ntot;
    // slots, in this node's outgoing list, of the (up to two distinct) messages the next node takes from it
    int s0 = -1, s1 = -1;
    for (int k = 0; k < 8; ++k) {
      if (!((frn >> k) & 1)) continue;
      const int s = wn[kDescSlot + k];
      if (s0 < 0 || s0 == s) s0 = s; else s1 = s;
    }
    // the tail of the list from the first handed-over row on: 8 / 9 first / second distinct handed-over row, else the
    // staged row's number
    const int p0s = fr ? w[kDescSlot + kfirst] : -1;
    uint32_t kinds = 0;
    int nt = 0, nstaged = 0, stage_of[3] = {-1, -1, -1};
    for (int k = kfirst; k < ntot && k < 8; ++k) {
      int kd;
      if ((fr >> k) & 1) kd = w[kDescSlot + k] == p0s ? 8 : 9;
      else { kd = nstaged; if (nstaged < 3) stage_of[nstaged] = k; ++nstaged; }
      kinds |= (uint32_t)kd << (4 * nt);
      ++nt;
    }
    // cut behind this node?
    int cut = 0;
    uint32_t pubkinds = 0;
    if (i + 1 < c1 && seg_len > 0 && (i + 1 - c0) % seg_len == 0 && (i + 1 - c0) / seg_len < nseg) {
      cut = (i + 1 - c0) / seg_len;
      for (int k = noutn; k < ntotn && k < 8; ++k)
        if ((frn >> k) & 1) pubkinds |= (uint32_t)(wn[kDescSlot + k] == s0 ? 8 : 9) << (4 * k);
    }
    // the staged words (trws_spec.h: kRsNt = 0, kRsKinds, kRsNmsg, kRsCut = 5, kRsPubKinds, kRsNout, kRsNin, kRsSrc = 9 .. 12,
    // kRsMd = 13, kRsNode = 14)
    R[0] = nt; R[1] = (int32_t)(kinds | ((uint32_t)nt << 16)); R[2] = s0 < 0 ? 0 : 1; R[5] = cut; R[6] = (int32_t)pubkinds;
    R[7] = nout; R[8] = nin; R[9] = R[10] = R[11] = R[12] = -1; R[13] = md >> nout; R[14] = w[kDescNode];
    // whose weight goes where among the staged doubles
    const int a0 = s0 < 0 ? 0 : s0, a1 = s1 < 0 ? a0 : s1;
    R[kRecAlphaEdge] = w[kDescEdge + (a0 & 7)]; R[kRecAlphaEdge + 1] = w[kDescEdge + (a1 & 7)]; R[kRecAlphaEdge + 2] = 0;
    for (int j = 3; j < 8; ++j) R[kRecAlphaEdge + j] = w[kDescEdge + ((nout + j - 3) & 7)];
    R[kRecKfirst] = kfirst; R[kRecNout] = nout; R[kRecNdep] = ndep; R[kRecRank] = w[kDescRank];
    uint32_t fetch = 0, labels = 0;
    const uint32_t fm = (uint32_t)w[kDescFetch] & 255u;
    for (int k = nout; k < ntot && k < 8; ++k)
      if (((fm >> k) & 1) && !((fr >> k) & 1)) { fetch |= 1u << k; if (k - nout < 4) labels |= 1u << k; }
    R[kRecFetch] = (int32_t)fetch; R[kRecLabels] = (int32_t)labels;
    const double gamma = (double)1 / (double)(nout > nin ? nout : nin > 0 ? nin : 1);   // (MRFEnergy.cpp:207-228)
    std::memcpy(R + kRecGamma, &gamma, 8);
    for (int k = 0; k < 8; ++k) { R[kRecEdge + k] = w[kDescEdge + k]; R[kRecOther + k] = w[kDescOther + k]; }
    for (int j = 0; j < 3; ++j) R[kRecStage + j] = stage_of[j];
    const int m0 = s0 >= 0 && s0 < 4 ? s0 : -1, m1 = s1 >= 0 && s1 < 4 ? s1 : -1;
    R[kRecMsg] = m0; R[kRecMsg + 1] = m1;
    R[kRecTwin] = s1 < 0 ? 0 : (m0 >= 0 && m1 >= 0) ? 2 : 1;
    R[kRecS0] = s0; R[kRecS0 + 1] = s1;
    for (int k = 0; k < kMaxDeps; ++k) R[kRecDep + k] = w[kDescDep + k];
    R[kRecNin] = nin;
  }
}

}  // namespace stereo
