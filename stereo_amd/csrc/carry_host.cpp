// Host side of the message transfer (carry_host.h): argument checks, and the receiving end of every edge's message
// row in a solver state.  No device call.
#include "carry_host.h"

#include <cmath>
#include <string>

#include "../../include/stereo_hip.h"
#include "common.h"
#include "trws_graph.h"

namespace stereo {
namespace carry {

namespace {
int check_ascending(const std::string &what, const char *name, const double *v, int K, int kmax, char *err, size_t errcap) {
  const std::string n(name);
  if (K < 1 || K > kmax)
    return fail(what + ": K_" + n.substr(4) + " must be 1 .. " + std::to_string(kmax) + " (got " + std::to_string(K) + ")", err, errcap);
  if (!v) return fail(what + ": " + n + " must not be NULL", err, errcap);
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(v[k])) return fail(what + ": " + n + "[" + std::to_string(k) + "] is not finite", err, errcap);
    if (k > 0 && !(v[k] > v[k - 1]))
      return fail(what + ": " + n + " must be strictly ascending (" + n + "[" + std::to_string(k) + "] <= " + n + "[" + std::to_string(k - 1) + "])", err, errcap);
  }
  return 0;
}
}  // namespace

int check_args(const char *entry, const Args &a, char *err, size_t errcap) {
  const std::string what(entry);
  constexpr int64_t kMaxEdges = (int64_t)1 << 31;
  if (a.E_old < 0 || a.E_old >= kMaxEdges) return fail(what + ": E_old must be 0 .. 2^31 - 1", err, errcap);
  if (a.E_new < 0 || a.E_new >= kMaxEdges) return fail(what + ": E_new must be 0 .. 2^31 - 1", err, errcap);
  if (a.N_new < 0 || a.N_new >= kMaxEdges) return fail(what + ": N_new must be 0 .. 2^31 - 1", err, errcap);
  if (int rc = check_ascending(what, "off_old", a.off_old, a.K_old, kMaxOldLabels, err, errcap)) return rc;
  if (int rc = check_ascending(what, "off_new", a.off_new, a.K_new, kMaxNewLabels, err, errcap)) return rc;
  if (!std::isfinite(a.stretch) || !(a.stretch > 0.0)) return fail(what + ": stretch must be finite and positive", err, errcap);
  if (!std::isfinite(a.gain) || !(a.gain > 0.0)) return fail(what + ": gain must be finite and positive", err, errcap);
  if (!a.edge_src && a.E_old != a.E_new)
    return fail(what + ": edge_src must be given where E_old != E_new (" + std::to_string(a.E_old) + " and " + std::to_string(a.E_new) + ")", err, errcap);
  if (a.E_old > 0 && !a.M_old) return fail(what + ": M_old must not be NULL", err, errcap);
  if (a.E_new > 0 && !a.receiver_new) return fail(what + ": receiver_new must not be NULL", err, errcap);
  if (a.E_new > 0 && !a.M_new) return fail(what + ": M_new must not be NULL", err, errcap);
  if (a.N_new > 0 && !a.shift) return fail(what + ": shift must not be NULL", err, errcap);
  if (a.device_form && !a.d_off_old) return fail(what + ": d_off_old must not be NULL", err, errcap);
  if (a.device_form && !a.d_off_new) return fail(what + ": d_off_new must not be NULL", err, errcap);
  const void *inputs[] = {a.M_old, a.off_old, a.edge_src, a.receiver_new, a.shift, a.off_new, a.d_off_old, a.d_off_new};
  for (const void *in : inputs) {
    if (in && a.M_new && in == (const void *)a.M_new) return fail(what + ": M_new must not be one of the inputs", err, errcap);
    if (in && a.bad && in == a.bad) return fail(what + ": bad must not be one of the inputs", err, errcap);
  }
  if (a.bad && a.bad == (const void *)a.M_new) return fail(what + ": bad must not be M_new", err, errcap);
  return 0;
}

}  // namespace carry
}  // namespace stereo

extern "C" int stereo_trws_state_receivers_host(int64_t N, int64_t E, const uint32_t *conn, int message_mode, int phase,
                                                int32_t *receiver, char *err, size_t errcap) {
  const std::string what = "stereo_trws_state_receivers_host";
  if (N < 0 || N >= ((int64_t)1 << 31)) return stereo::fail(what + ": N must be 0 .. 2^31 - 1", err, errcap);
  if (E < 0) return stereo::fail(what + ": E must not be negative", err, errcap);
  if (phase < 0 || phase > 2) return stereo::fail(what + ": phase must be 0, 1 or 2", err, errcap);
  if (E > 0 && !conn) return stereo::fail(what + ": conn must not be NULL", err, errcap);
  if (E > 0 && !receiver) return stereo::fail(what + ": receiver must not be NULL", err, errcap);
  for (int64_t e = 0; e < 2 * E; ++e)
    if ((int64_t)conn[e] >= N) return stereo::fail(what + ": conn names a node outside 0 .. N - 1 (edge " + std::to_string(e / 2) + ")", err, errcap);
  try {
    stereo::TrwsGraphOptions opt;
    opt.ordering = (message_mode & STEREO_TRWS_ORDER_INDEX) ? 1 : 0;
    stereo::TrwsGraph g;
    std::string gerr;
    if (!stereo::build_trws_graph(N, E, conn, opt, g, gerr)) return stereo::fail(what + ": " + gerr, err, errcap);
    for (int64_t e = 0; e < E; ++e) receiver[e] = (int32_t)(phase == 0 ? g.tail[e] : g.head[e]);
    return 0;
  } catch (const std::exception &e) {
    return stereo::fail(what + ": " + e.what(), err, errcap);
  }
}
