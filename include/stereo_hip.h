/* stereo_hip.h -- C ABI of libstereo_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the 3D-label stereo energy-minimisation path of
 * johannesu/stereo.  Every entry point replaces one reference interface; the
 * citation says which (paths relative to the reference tree).  Plain pointers
 * and sizes only; all functions return 0 on success, non-zero on failure,
 * never throw and never exit().  On failure a message is copied into `err`
 * (if errcap > 0) and is also available from stereo_hip_last_error().
 *
 * Array conventions are MATLAB's at the mex boundary: column-major, i.e. a
 * K x N matrix is N consecutive K-vectors (label fastest).  `conn` is the
 * 2 x E uint32 connectivity, ZERO based as passed to the mex gateways
 * (rd.m:21 / trws.m:33 subtract 1 before the call).
 */
#ifndef STEREO_HIP_H_
#define STEREO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point is added or a signature changes; the Python binding refuses a
 * library that reports another version (a stale libstereo_hip.so).  3: stereo_hip_device_cus, plan
 * entry points select their plan's device, wall-clock bound on cross-workgroup waits.  4: stereo_fusion_fit_planes,
 * stereo_fusion_fuse_until_convergence.  5: stereo_segpln_wta, stereo_segpln_planes.  6: stereo_segment_* (the segmenters
 * behind dispmap_globalstereo), stereo_trws_plan_debug_terms / _messages, stereo_segpln_planes_batch.  7: TRW-S takes
 * up to 4096 labels with one shared strictly ascending positions vector (stereo_trws_plan_path 5).  8: stereo_trws_batch_*
 * (independent plans that share one launch per sweep).  10: stereo_trws_plans_state_* (solver state: save / load),
 * stereo_trws_state_check, stereo_trws_strip_state_rows_host.  11: stereo_lr_check / stereo_lr_fill (left-right
 * consistency).  12: stereo_band_inputs / stereo_band_apply (band refinement around a solved disparity map).
 * 13: stereo_plane_band_inputs_ncc / _globalstereo / stereo_plane_band_apply (band refinement around a solved plane map).
 * 14: stereo_pyramid_reduce / stereo_pyramid_expand (image pyramid: box reduction, map expansion).
 * 15: stereo_band_carry / stereo_band_carry_device (messages carried from one band level or pyramid scale to the
 * next), stereo_trws_state_receivers_host.  16: stereo_pyramid_reduce_volume / _device (image pyramid: a coarser
 * level's NCC volume as the block mean of the finer one).  17: stereo_candidates_gather / _inputs / _apply (candidate
 * bands: per-pixel label sets propagated from neighbours).  18: stereo_plane_candidates_gather / _inputs_ncc /
 * _inputs_globalstereo / _apply (plane candidates: per-pixel plane sets propagated from neighbours).
 * 19: stereo_pyramid_expand_planes / _device (a plane map carried to the next finer scale as planes),
 * stereo_planes_fit_local / _device (the per-pixel local plane fit).  20: stereo_scanline_aggregate / _device.
 * 21: stereo_scanline_edges_* (scanline aggregation on per-edge positions and weights).
 * 22: stereo_contrast_edge_weights / stereo_contrast_step_weights (smoothness weights from an image),
 * stereo_scanline_aggregate_weighted / _device (scanline aggregation with a weight per pixel and direction).
 * Still 22: stereo_map_filter_max_radius / stereo_map_weighted_median / _device (map filter) -- three added symbols and
 * no changed signature; tests/test_scanline_weighted_cpu.py pins 22, and the binding that needs them
 * (stereo_amd/mapfilter.py) refuses a library without them by name. */
#define STEREO_HIP_ABI_VERSION 22

/* ---- library ---------------------------------------------------------- */

int stereo_hip_abi_version(void);
/* Number of visible HIP devices (0 if none / runtime failure). */
int stereo_hip_device_count(void);
/* Selects the device used by subsequent calls of this thread (default 0).  A plan stays on the
 * device that was current when it was created: every plan entry point makes that device current for
 * its own duration. */
int stereo_hip_set_device(int device);
/* Compute units of the current device (0 without a device): the number of workgroups of a persistent
 * sweep launch that are certain to be resident together. */
int stereo_hip_device_cus(void);
/* Creates the HIP context of the current device and launches one empty kernel, so that the
 * runtime's one-time initialisation happens now.  Optional; it matters to callers that seed libc
 * rand() for QPBO Improve (QPBO_extra.cpp:13-27 draws its permutation from it): the runtime
 * consumes rand() values during that initialisation.  Returns 0, or non-zero without a device. */
int stereo_hip_warm_up(void);

/* Test hook (host only, no device needed): the node permutation QPBO::Improve walks
 * (QPBO_extra.cpp:13-27, :1224-1232), drawn from libc rand() exactly as the reference draws it --
 * N - 1 values consumed, the generator left where N - 1 calls of rand() leave it.  out: N int32. */
int stereo_hip_improve_permutation(int64_t N, int32_t *out);
/* Last error message of the calling thread ("" if none). */
const char *stereo_hip_last_error(void);

/* ---- TRW-S simultaneous fusion ---------------------------------------- *
 * Replaces cpp/trws_mex.cpp:149-164 mexFunction -> solve_mrf<T> (:27-147):
 *   [labelling, energy, lower_bound, iterations] =
 *       trws_mex(kernel, unary, connectivity-1, q, qprim, alphas, tol, options)
 * kernel      1 = truncated linear  (TypeStereoLinear),
 *             2 = truncated quadratic (TypeStereoQuadratic); anything else fails
 *             with "Unsupported kernel" (trws_mex.cpp:162).
 * unary       K x N   q, qprim  K x E   alphas  E   tol = lambda (trws_mex.cpp:37)
 * K           1 .. 512 with any q / qprim; 513 .. 4096 when every column of q and qprim is one and
 *             the same finite, strictly ascending vector; anything else fails with "K must be in ...".
 * maxiter, max_relgap: the two fields of the options struct (trws_mex.cpp:40-41;
 *             defaults 1000 and 0 are applied by the caller / gateway).
 * labelling   N doubles, ONE based (trws_mex.cpp:137).
 */
/* Repeated calls with the same (kernel, K, connectivity) -- one per simultaneous_fusion of an object,
 * dispmap_super.m:153-198 -- reuse the plan of the last problem seen: graph analysis, descriptors and
 * device buffers are kept, a call costs the upload of its inputs, the iterations and the labels back.
 * If every column of q and qprim is bitwise the same vector (fronto-parallel proposals, :177-183) only
 * that vector is uploaded and the shared-position kernels run; same bits as the K x E form.
 * STEREO_HIP_TRWS_CACHE=0: a fresh plan per call and the K x E arrays always.  The cached plan keeps its
 * device memory (messages: 8 K E bytes) until the next different problem or stereo_trws_cache_clear(). */
int stereo_trws(int kernel, const double *unary, const uint32_t *conn, const double *q,
                const double *qprim, const double *alphas, double tol, double maxiter,
                double max_relgap, int K, int64_t N, int64_t E, double *labelling,
                double *energy, double *lower_bound, double *iterations, char *err,
                size_t errcap);
void stereo_trws_cache_clear(void);
/* Same solve, plus each node's min-marginals and confidence (definition: stereo_trws_plan_keep_min_marginals).
 * No reference counterpart (trws_mex returns four outputs; mex/trws_minmarginals_mex.cpp is the six-output gateway).
 * min_marginals K x N, confidence N; either may be NULL.  Labels, energy, bound and iterations are stereo_trws's bits.
 * ONE plan by default, also with STEREO_HIP_GPUS >= 2 (strips give the same bits): cached strips of the same problem
 * are replaced by a single plan.  With STEREO_HIP_TRWS_BELIEFS_STRIPS=1 as well the call is sharded by stereo_trws's
 * rule (stereo_trws_gateway_strips): every strip keeps the beliefs of its own nodes and the rows are put together at
 * their node ids -- the same bits again, with messages and beliefs divided among the strips.  The flag is a runtime
 * setting of the cached plan(s): a later plain stereo_trws call on them runs with the flag off and pays nothing.
 * Extra device memory 8 K N bytes (over all strips). */
int stereo_trws_min_marginals(int kernel, const double *unary, const uint32_t *conn, const double *q,
                              const double *qprim, const double *alphas, double tol, double maxiter,
                              double max_relgap, int K, int64_t N, int64_t E, double *labelling,
                              double *energy, double *lower_bound, double *iterations,
                              double *min_marginals, double *confidence, char *err, size_t errcap);


/* Device-resident form of the same solver: graph analysis (SetAutomaticOrdering,
 * ordering.cpp:7-157; CompleteGraphConstruction, MRFEnergy.cpp:137-229) is done
 * once per connectivity, inputs live in HBM across calls, iterations can be
 * issued without host round trips.  Used by the mex gateway for repeated
 * simultaneous_fusion calls on one image (dispmap_super.m:153-198) and by
 * bench.py (inputs resident before the timed region).
 */
typedef struct stereo_trws_plan stereo_trws_plan;

/* flags */
#define STEREO_TRWS_MESSAGES_EXACT 0   /* reference lower-envelope semantics (default) */
#define STEREO_TRWS_MESSAGES_MINPLUS 1 /* plain min-plus messages, no certificate / envelope construction:
                                         the reference's bits unless a message's certificate would have
                                         failed (exact or near ties), the brute-force O(K^2) result always.
                                         With 64 < K <= 256 and shared ascending positions it is a branch of
                                         trws_wide_kernel (1.4x the exact messages at 3000x2000x256) */
/* OR-ed into message_mode: visit the nodes in index order -- MRFEnergy's order when the gateway
 * does NOT call SetAutomaticOrdering (trws_mex.cpp:121; nodes keep the order of AddNode,
 * MRFEnergy.cpp:37-76).  On an image grid the dependency DAG then has H + W - 1 anti-diagonal
 * levels and no serial border chain (the gateway's order: ~2 (H + W)): a faster, equally valid
 * TRW-S schedule whose labels / energies are NOT the gateway's.  Explicit opt-in only. */
#define STEREO_TRWS_ORDER_INDEX 0x100

/* K in [1, 4096]; above 512 the plan takes only a shared positions vector that is finite and strictly
 * ascending (upload / bind_device fail with "K must be in ..." otherwise). */
int stereo_trws_plan_create(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn,
                            int message_mode, stereo_trws_plan **plan, char *err,
                            size_t errcap);
void stereo_trws_plan_destroy(stereo_trws_plan *plan);

/* Host -> HBM upload of the per-call inputs (same meaning as stereo_trws).
 * q == NULL && qprim == NULL selects "shared positions": every edge uses the
 * K-vector `positions` for both q(:,e) and qprim(:,e) (fronto-parallel labels,
 * dispmap_super.m:177-183 with planes [0 0 1 -d]); nothing K x E is stored. */
int stereo_trws_plan_upload(stereo_trws_plan *plan, const double *unary, const double *q,
                            const double *qprim, const double *positions,
                            const double *alphas, double tol, char *err, size_t errcap);
/* Same, but the arrays are already DEVICE pointers (e.g. torch tensors, or the
 * output of the cost-volume kernels); they are borrowed, not copied. */
int stereo_trws_plan_bind_device(stereo_trws_plan *plan, const double *d_unary,
                                 const double *d_q, const double *d_qprim,
                                 const double *d_positions, const double *d_alphas,
                                 double tol, char *err, size_t errcap);
/* Both calls start a NEW minimisation: if the plan has iterated before, they imply
 * stereo_trws_plan_reset (an iterate call runs the forward sweep of the following iteration ahead
 * of time, so messages computed from the old inputs cannot be continued with new ones).  To go on
 * from messages that exist -- a saved run, a warm start with other unaries -- upload or bind first,
 * then load a solver state (stereo_trws_plans_state_load below). */

/* Zero all messages (MRFEnergy.cpp:115-133) and the iteration counter. */
int stereo_trws_plan_reset(stereo_trws_plan *plan, char *err, size_t errcap);
/* Runs up to `iters` further iterations of Minimize_TRW_S (minimize.cpp:31-113):
 * forward sweep, backward sweep (+ lower bound), primal labelling + energy, stop
 * test `(E-LB)/E < max_relgap`.  Returns in *done_iters the number executed in
 * this call, *stopped != 0 if the relative-gap test fired.  `stream` is a
 * hipStream_t (NULL = default stream); the call returns after the last
 * iteration's scalars have reached the host. */
int stereo_trws_plan_iterate(stereo_trws_plan *plan, int iters, double max_relgap,
                             void *stream, int *done_iters, int *stopped, char *err,
                             size_t errcap);
/* Result of the most recent iteration (minimize.cpp:104: the LAST primal, not the
 * best).  labelling: N doubles, one based; may be NULL. */
int stereo_trws_plan_result(stereo_trws_plan *plan, double *labelling, double *energy,
                            double *lower_bound, double *iterations, char *err,
                            size_t errcap);
/* Diagnostics: graph analysis results (all may be NULL). rank: N int64;
 * levels: number of dependency levels of the node order. */
int stereo_trws_plan_info(stereo_trws_plan *plan, int64_t *rank, int64_t *levels,
                          int64_t *max_level_nodes, char *err, size_t errcap);
/* Timing hooks for bench.py: total device time (ms, hipEvent on the plan's
 * stream) and launch count of the sweep kernels since the last reset_stats. */
int stereo_trws_plan_stats(stereo_trws_plan *plan, double *sweep_ms, int64_t *sweep_launches,
                           int reset);

/* Diagnostics: number of message updates (since the last reset) for which the fast
 * min-plus path could not certify equality with the reference's serial envelope
 * construction and the serial construction was run instead. */
int stereo_trws_plan_counters(stereo_trws_plan *plan, int64_t *serial_messages, int reset);

/* The speculative schedule of the long serial run (the image grid's border chain): a runner computes the
 * run's recurrence ahead with plain min-plus, segments of the run recompute every visit with the certified routine side
 * by side, compare what they started from with what the segment in front produced, and walk again if it differs --
 * results are the sequential sweep's either way.  out[0] = 1 if the plan's next sweeps use it (graph, kernel family,
 * positions permitting; STEREO_HIP_TRWS_SPEC=0 turns it off at plan creation), out[1] = segments walked twice,
 * out[2] = segments committed, out[3] = visits of the runner, since the plan was created.  No reference counterpart. */
int stereo_trws_plan_spec_stats(stereo_trws_plan *plan, int64_t out[4]);

/* Diagnostics / test hook: M independent message updates Edge::UpdateMessage
 * (typeStereoLinear.h:329-487, typeStereoQuadratic.h:329-501) on the device, one wavefront per
 * message, through the very routine the pipelined sweep kernel uses (certified min-plus fast
 * path, second look, serial lower-envelope construction).  Row m of the M x K arrays (K <= 64):
 * H = gamma[m] * Di - msg_in (:383-387), source positions q_source, destination positions q_dest
 * (the caller has resolved dir == m_dir, :343-357).  certificate = 0 forces the serial
 * construction.  shared_positions != NULL tells the routine that every row uses these K strictly
 * ascending positions for sources and destinations (`window` = index distance beyond which a
 * source costs >= vTrunc, or -1).  used_serial[m] (may be NULL) = 1 if the serial construction ran. */
int stereo_trws_messages(int kernel, int K, int64_t M, const double *Di, const double *gamma,
                         const double *msg_in, const double *q_source, const double *q_dest,
                         const double *alpha, double lambda, int certificate, int window,
                         const double *shared_positions, double *msg_out, double *vmin,
                         int32_t *used_serial, char *err, size_t errcap);

/* Diagnostics: which sweep implementation the plan's current inputs select.
 * 1 generic persistent kernel, 2 pipelined kernel (K <= 64),
 * 3 wide pipelined kernel (64 < K <= 256, shared strictly ascending positions),
 * 4 two-labels-per-lane pipelined kernel (64 < K <= 128, linear kernel, any positions),
 * 5 large-label kernel (512 < K <= 4096, shared strictly ascending positions, any graph, both modes).
 * All give identical results.  Negative on a NULL plan. */
int stereo_trws_plan_path(stereo_trws_plan *plan);

/* ---- node beliefs: min-marginals, confidence, argmin ------------------------------ *
 * No reference counterpart as an output.  After a run whose last finished iteration is t (the iterations
 * reported), the belief of node i is the Di that MRFEnergy's forward pass of iteration t + 1 forms at i
 * (minimize.cpp:38-46): D_i + the messages of firstForward(i) + those of firstBackward(i), in list order --
 * the vector the plan's fused launch used to send i's forward messages.  One message state at rest never
 * holds all of them (each edge stores one message and its direction flips every sweep), so with the flag on
 * every iteration runs one extra kernel between the backward sweep and the fused forward sweep
 * (P_i = D_i + firstForward messages; 8 K N bytes of device memory, about 8 K (2 N + E) bytes of traffic),
 * and the read adds the firstBackward messages.  Bit-identical to t iterations of minimize.cpp plus one forward
 * pass on the CPU.  Flag off (the default): no extra launch, no extra memory.  A strip plan refuses this entry and
 * takes stereo_trws_plan_strip_keep_min_marginals (below).  on = 0 frees the buffer.  Fails cleanly if the buffer
 * cannot be allocated. */
int stereo_trws_plan_keep_min_marginals(stereo_trws_plan *plan, int on, char *err, size_t errcap);
/* Outputs of the last run, node-id order: min_marginals K x N (label fastest) = Di - min Di; confidence N = the
 * second-smallest entry of that vector (+Inf when K = 1); argmin N = the first minimum, 0-based (the primal's tie
 * rule).  Any of the three may be NULL.  Fails if no iteration has run with the flag on since it was set, after a
 * reset, upload or bind (they start a new minimisation), while an issued iteration has not been collected, and on
 * strip plans (their entry: stereo_trws_plan_strip_min_marginals).  Reading twice without iterating gives the same
 * bits.  Host arrays: */
int stereo_trws_plan_min_marginals(stereo_trws_plan *plan, double *min_marginals, double *confidence,
                                   int32_t *argmin, char *err, size_t errcap);
/* ... or device arrays of the caller (e.g. torch tensors), written on `stream` (hipStream_t, NULL = default)
 * without waiting for it. */
int stereo_trws_plan_min_marginals_device(stereo_trws_plan *plan, double *d_min_marginals,
                                          double *d_confidence, int32_t *d_argmin, void *stream,
                                          char *err, size_t errcap);

/* ---- row strips: one image tiled across the GPUs of a node ------------------------------ *
 * No reference counterpart (the reference is one serial sweep, minimize.cpp:36-95); what is
 * sharded is exactly that sweep under the order of ordering.cpp:42-152, and the labels are the
 * ones a single plan returns, bit for bit.  `owner[i]` names the strip that visits node i; strips
 * form a chain (an edge joins nodes of one strip or of strips g, g+1) -- for an image, bands of
 * rows.  One plan per strip, normally one process and one GPU each.  A strip stores only what
 * it touches -- its own nodes, the nodes one edge away (halo) and the edges with an own endpoint,
 * under strip-local ids -- so the messages and unaries of a large problem are divided among the
 * GPUs (1/G each plus a boundary row).  A boundary node's new messages, its completion flag and
 * its label are written by the visiting workgroup straight into the neighbouring strip's arrays,
 * at the neighbour's ids (peer stores over xGMI + flag; nothing is staged through the host and
 * there is no collective on the data path).  stereo_trws_plan_upload / _bind_device still take
 * the arrays of the WHOLE problem and keep the strip's rows (a gather into arrays owned by the
 * plan, so the full ones may be freed afterwards); stereo_trws_plan_bind_device_strip takes
 * arrays that are strip-local already, in the order stereo_trws_plan_strip_layout reports.
 * stereo_trws_plan_result fills the labels of the strip's nodes (1 elsewhere).  Energy and lower bound come back as per-strip
 * partial sums (each in the reference's summation order restricted to the strip); the caller adds
 * them in strip order -- the only cross-strip reduction, two doubles per iteration -- so they
 * agree with the single-plan values to rounding (1e-12 relative), not bit for bit.
 *
 * max_workgroups > 0 caps the strip's launch (strips that share one GPU must all be resident
 * together).  share_analysis_with: another strip's plan of the same problem in this process
 * (owner may then be NULL), so the host-side analysis is done once. */
int stereo_trws_plan_create_strip(int kernel, int K, int64_t N, int64_t E, const uint32_t *conn,
                                  int message_mode, const int32_t *owner, int nstrips, int strip,
                                  int max_workgroups, stereo_trws_plan *share_analysis_with,
                                  stereo_trws_plan **plan, char *err, size_t errcap);
/* Neighbour in the same process (which: 0 = strip - 1, 1 = strip + 1); enables peer access if the
 * two plans live on different devices. */
int stereo_trws_plan_connect(stereo_trws_plan *plan, int which, stereo_trws_plan *peer, char *err,
                             size_t errcap);
/* Neighbour in another process: export writes STEREO_TRWS_IPC_BYTES bytes of HIP IPC handles
 * (messages, flags, labels) that the neighbour passes to ipc_connect after exchanging them over
 * any channel (bench.py: torch.distributed all_gather). */
#define STEREO_TRWS_IPC_BYTES 256
int stereo_trws_plan_ipc_export(stereo_trws_plan *plan, void *handles, size_t cap, char *err,
                                size_t errcap);
int stereo_trws_plan_ipc_connect(stereo_trws_plan *plan, int which, const void *handles, char *err,
                                 size_t errcap);
/* One iteration of a strip in three steps, so that all strips of a process can be in flight
 * together and the caller can reduce the partial sums across processes:
 *   issue   launches forward sweep (first iteration only), backward sweep and the primal pass
 *           fused with the next forward sweep, without waiting (stream NULL = the plan's own);
 *   collect waits and returns this strip's partial lower bound and energy;
 *   commit  records the reduced totals (what stereo_trws_plan_result reports) and counts the
 *           iteration.  The stop test (E-LB)/E < max_relgap of minimize.cpp:105 is the caller's. */
int stereo_trws_plan_issue(stereo_trws_plan *plan, void *stream, char *err, size_t errcap);
/* The same for n <= 16 strips that share ONE device (logical strips; a process that owns several
 * bands): each sweep is a single launch whose workgroups are divided among the strips, so all of
 * them are resident together (separate launches on separate streams may be serialised by the
 * runtime, and strips wait for each other in both directions).  Collect / commit per plan. */
int stereo_trws_plans_issue(stereo_trws_plan *const *plans, int n, void *stream, char *err, size_t errcap);
int stereo_trws_plan_collect(stereo_trws_plan *plan, double *lower_bound_part, double *energy_part,
                             char *err, size_t errcap);
int stereo_trws_plan_commit(stereo_trws_plan *plan, double lower_bound, double energy, char *err,
                            size_t errcap);
/* ---- batches: independent problems that share one launch per sweep ----
 * A sweep of one problem is bound by the dependency chain of its node order and leaves most of the device idle; a batch
 * runs the sweeps of n <= 16 plans in one launch each, so that the idle compute units work on the other problems.
 * Members are ordinary plans and stay the caller's: each keeps its own inputs, messages, labels, energy, bound and
 * iteration count, results come from stereo_trws_plan_result per member, and every member computes bit for bit what
 * stereo_trws_plan_iterate computes for it alone (its bound and energy are summed per member, in the single plan's
 * order).  A member may be iterated alone between batch calls; it must outlive the batch's last call.
 *
 * create accepts plans that are whole problems (not strips) with inputs uploaded or bound, all on one device, all in
 * one pipelined kernel family (stereo_trws_plan_path 2, 3 or 4), with the same smoothness kernel, message mode and kind
 * of positions (one shared vector, or q / qprim per edge): one launch runs one sweep kernel.  K, the graph and its size
 * may differ.  Everything else -- the generic or large family, mixed instantiations, a strip, a member without inputs
 * or on another device, the same plan twice, n < 1 or n > 16 -- is refused with a message that names the offending
 * member ("member <index> ...") and the reason; the plans are left as they were.  The rule is applied again by every
 * iterate (an upload can move a plan to another family).
 *
 * K <= 64 (path 2): the launch's workgroups start on one member each and move on to the next member that has runs
 * left when theirs has none, so members of unequal size share the device.  Paths 3 and 4 run one workgroup per compute
 * unit: the launch's grid is divided statically, and a batch whose shares do not fit the device together is split into
 * consecutive launches.  Shared launches keep the plain chain schedule: the speculative border-chain schedule of a
 * single plan (stereo_trws_plan_spec_stats) is OFF inside them, like in a strip group; results do not depend on it.
 * Where a shared launch is measured to lose against the plans iterated in turn -- one active member; fewer than 8
 * members on path 2 that each have more runs than the device keeps workgroups resident -- iterate gives
 * every member its own launches, one after the other, exactly as stereo_trws_plan_iterate does: same bits, same
 * contract, and out[1] of stereo_trws_batch_stats does not count them.
 * Node beliefs: the members with stereo_trws_plan_keep_min_marginals on get their phase 1 in every batch iteration -- one
 * launch for all of them -- between the backward and the fused launch as in stereo_trws_plan_iterate, and stereo_trws_plan_min_marginals after a
 * batch iteration returns what it returns after the same iterations alone.
 * A batch runs on the default (NULL) stream: the members' inputs must be complete there (bound arrays written on
 * another stream need a synchronisation first).  Sweep timing (stereo_trws_plan_stats) is not defined for batch
 * iterations: the launches belong to all members at once. */
typedef struct stereo_trws_batch stereo_trws_batch;
int stereo_trws_batch_create(stereo_trws_plan *const *plans, int n, stereo_trws_batch **out, char *err, size_t errcap);
/* Frees the batch; the members are not touched. */
void stereo_trws_batch_destroy(stereo_trws_batch *batch);
/* Up to `iters` iterations of every member.  max_relgap applies PER MEMBER exactly as in stereo_trws_plan_iterate: a
 * member whose (E - LB) / E falls below it stops and keeps its state, the others go on, the launches that follow leave
 * it out, and it stays out of this batch's later calls until stereo_trws_batch_reset.  done_iters[i] (n entries, may be
 * NULL): iterations member i ran in this call.  If a member's sweep gives up waiting, every member's iteration is
 * collected first and the error names the member. */
int stereo_trws_batch_iterate(stereo_trws_batch *batch, int iters, double max_relgap, int32_t *done_iters, char *err,
                              size_t errcap);
/* stereo_trws_plan_reset of every member; stopped members take part again; the batch's counters restart. */
int stereo_trws_batch_reset(stereo_trws_batch *batch, char *err, size_t errcap);
/* Diagnostics since creation / the last reset: out[0] workgroups that held runs of more than one member (read from the
 * batch's control words on the device; 0 on paths 3 and 4), out[1] sweep launches issued (a split batch counts each
 * part), out[2] 1 if the speculative schedule runs inside this batch (always 0), out[3] workgroups one launch keeps
 * resident together. */
int stereo_trws_batch_stats(stereo_trws_batch *batch, int64_t out[4]);
/* What a strip stores.  nodes (n_nodes entries): global id of local node i -- the n_own own nodes
 * in ascending order, then the halo; edges (n_edges): global id of local edge e, ascending.  Any
 * output may be NULL (ask for the counts first).  A plan of the whole problem reports identity. */
int stereo_trws_plan_strip_layout(stereo_trws_plan *plan, int64_t *n_nodes, int64_t *n_own,
                                  int64_t *n_edges, int32_t *nodes, int32_t *edges);
/* stereo_trws_plan_bind_device with strip-local arrays: d_unary K x n_nodes, d_alphas n_edges,
 * d_q / d_qprim K x n_edges (or shared d_positions), rows in the order of strip_layout.  The
 * arrays stay the caller's. */
int stereo_trws_plan_bind_device_strip(stereo_trws_plan *plan, const double *d_unary,
                                       const double *d_q, const double *d_qprim,
                                       const double *d_positions, const double *d_alphas,
                                       double tol, char *err, size_t errcap);
/* The same without a device: what strip `strip` of the problem stores, and the descriptors of its
 * own visits in sweep `direction` (0 forward, 1 backward) after renumbering -- n_visits x 64 words,
 * layout in stereo_amd/csrc/trws_graph.h (words 0 node, 4-11 edges, 20-23 dependencies, 32-39
 * neighbours, 43 remote bits, 45-52 / 53-54 the neighbour strips' ids).  Sizes first (arrays
 * NULL), then the arrays.  For tests of the multi-GPU decomposition on a host without GPUs. */
int stereo_trws_strip_layout_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner,
                                  int nstrips, int strip, int direction, int64_t *n_nodes,
                                  int64_t *n_own, int64_t *n_edges, int64_t *n_visits, int32_t *nodes,
                                  int32_t *edges, int32_t *desc, char *err, size_t errcap);
/* Node beliefs on strips.  A strip keeps the beliefs of its OWN nodes: 8 K n_own bytes, one extra
 * kernel per iteration between the strip's backward and its fused launch -- every message row the two phases read for
 * an own node is in the strip's own copy when they read it, so the strips exchange nothing for this.  Strips that
 * iterate through stereo_trws_plans_issue share one such launch per iteration, as do the members of a batch.
 * On a plan of the whole problem the call is stereo_trws_plan_keep_min_marginals.  on = 0 frees the buffers.
 * Turn it on on every strip between iterations (collective where the strips are processes). */
int stereo_trws_plan_strip_keep_min_marginals(stereo_trws_plan *plan, int on, char *err, size_t errcap);
/* The strip's own rows after its iteration was collected, host arrays: min_marginals K x n_own, confidence n_own,
 * argmin n_own (0-based), own nodes in the order of stereo_trws_plan_strip_layout (row j belongs to node nodes[j]).
 * Any output may be NULL.  Fails like stereo_trws_plan_min_marginals: flag off, no iteration since it was set or since
 * a reset / upload / bind, an issued iteration not yet collected. */
int stereo_trws_plan_strip_min_marginals(stereo_trws_plan *plan, double *min_marginals, double *confidence,
                                         int32_t *argmin, char *err, size_t errcap);
/* n <= 16 strips of one problem that share ONE device, read in one launch into device arrays of the WHOLE problem
 * (d_min_marginals K x N, d_confidence N, d_argmin N, any may be NULL) on `stream`, without waiting for it: every own
 * node's row is written at its global id; nodes of strips that are not named keep what the arrays held. */
int stereo_trws_plans_min_marginals_device(stereo_trws_plan *const *plans, int n, double *d_min_marginals,
                                           double *d_confidence, int32_t *d_argmin, void *stream, char *err,
                                           size_t errcap);
/* Host only (no device): the lists the belief kernels walk on strip `strip` -- own (n_own entries): its own nodes in
 * rank order as strip-local ids; fptr / bptr (n_own + 1) and fidx / bidx (n_fwd / n_bwd): per such node the
 * firstForward / firstBackward edges as strip-local ids, in the list order of stereo_trws_analyze.  Sizes first
 * (arrays NULL), then the arrays.  nstrips == 1: the whole problem (owner may be NULL). */
int stereo_trws_strip_belief_lists_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner,
                                        int nstrips, int strip, int64_t *n_own, int64_t *n_fwd, int64_t *n_bwd,
                                        int32_t *own, int32_t *fptr, int32_t *fidx, int32_t *bptr, int32_t *bidx,
                                        char *err, size_t errcap);
/* ---- solver state: save and restore; resume, re-shard, warm start ---------------- *
 * No reference counterpart (MRFEnergy keeps its messages inside the object).  A state is what a minimisation has
 * computed, in the CALLER's layout, so that it can leave the plan that ran it and enter another one -- a fresh plan in
 * another process, row strips instead of one plan or back, another kernel family, a batch member: this header, the
 * messages (E x K doubles: MATLAB's K x E, label fastest, the caller's edge order) and the labels (N int32, zero based,
 * node-id order: what stereo_trws_plan_result reports minus one).  Inputs (unary, q, qprim, positions, alphas, tol),
 * sweep statistics, counters and node beliefs are not part of it.
 *   phase 0  the messages stand as after a backward sweep.  What a fresh or reset plan saves (zero messages,
 *            iterations 0), and the door for foreign messages.
 *   phase 1  the forward sweep of iteration `iterations` + 1 has run: where every iterate call leaves a plan.
 *   phase 2  the backward sweep of that iteration has run as well and no iteration has taken it (an iterate call that
 *            stopped on max_relgap before its last iteration); its bound, summed in the single plan's order, is
 *            lower_bound_next.  Single plans only.
 * Every kernel family, strips and batches promise identical results, so a run that goes on from a loaded state equals
 * the uninterrupted run bit for bit (strips: labels and messages; their energy and bound are sums of partial sums as
 * always).  Exact and min-plus message modes may differ between save and load: no bit promise across them. */
#define STEREO_TRWS_STATE_MAGIC 0x53575254u /* "TRWS" */
#define STEREO_TRWS_STATE_VERSION 1
typedef struct stereo_trws_state_header {
  uint32_t magic, version;
  int32_t kernel, K;
  int64_t N, E;
  int32_t message_mode;       /* as given to stereo_trws_plan_create, STEREO_TRWS_ORDER_INDEX included */
  int32_t phase;              /* 0, 1, 2 */
  uint64_t connectivity_key;  /* FNV-1a (64 bit) over the 2 x E uint32 words of the connectivity */
  int64_t iterations;
  double energy, lower_bound, lower_bound_next;
} stereo_trws_state_header;
/* n == 1 and a plan of the whole problem: that plan.  Otherwise plans[0 .. n) are ALL the strips of one problem, each
 * once, in one state (same iteration count, nothing issued and uncollected).
 * save waits for the plans' streams, reads, and leaves every plan exactly as it was (a pending sweep and the counters
 * held for it included).  messages / labels: host arrays, E x K doubles and N int32.  From strips every edge row is
 * taken from the one strip whose copy is valid (stereo_trws_strip_state_rows_host), every label from its owner. */
int stereo_trws_plans_state_save(stereo_trws_plan *const *plans, int n, stereo_trws_state_header *header,
                                 double *messages, int32_t *labels, char *err, size_t errcap);
/* load = stereo_trws_plan_reset (a pending sweep is discarded as there), then messages, labels, iteration count,
 * energy and bound are the state's and the plan continues as the saved one would have: stereo_trws_plan_result returns
 * what it returned there, the first launch of the next iterate is the backward sweep (phase 1) or the fused launch
 * (phase 2).  The plans need their inputs first ("upload or bind first, then load": an upload wipes the state).
 * Refused, naming the field: another magic, version, kernel, K, N, E or connectivity, a differing
 * STEREO_TRWS_ORDER_INDEX bit, phase 2 into strips.  Node beliefs (stereo_trws_plan_keep_min_marginals) cannot be
 * rebuilt from a state: they are readable again after one iteration.  Every strip takes every row it stores. */
int stereo_trws_plans_state_load(stereo_trws_plan *const *plans, int n, const stereo_trws_state_header *header,
                                 const double *messages, const int32_t *labels, char *err, size_t errcap);
/* The same with DEVICE arrays of the caller (e.g. torch tensors) on the plans' device; the header stays on the host.
 * save: the copies / the gather are enqueued on `stream` (hipStream_t, NULL = default) behind the plans' own work and
 * not waited for.  load: the plans' state is reset first (synchronously), the copies / the scatter run on `stream`,
 * and the call returns when they are done. */
int stereo_trws_plans_state_save_device(stereo_trws_plan *const *plans, int n, stereo_trws_state_header *header,
                                        double *d_messages, int32_t *d_labels, void *stream, char *err, size_t errcap);
int stereo_trws_plans_state_load_device(stereo_trws_plan *const *plans, int n, const stereo_trws_state_header *header,
                                        const double *d_messages, const int32_t *d_labels, void *stream, char *err,
                                        size_t errcap);
/* One plan of a whole problem: the group entries with n == 1. */
int stereo_trws_plan_state_save(stereo_trws_plan *plan, stereo_trws_state_header *header, double *messages,
                                int32_t *labels, char *err, size_t errcap);
int stereo_trws_plan_state_load(stereo_trws_plan *plan, const stereo_trws_state_header *header, const double *messages,
                                const int32_t *labels, char *err, size_t errcap);
/* Host only (no device).  The refusal rule of load: 0 if a plan created with (kernel, K, N, E, conn, message_mode)
 * takes the state, else nonzero with the reason -- which names the field -- in why. */
int stereo_trws_state_check(const stereo_trws_state_header *header, int kernel, int K, int64_t N, int64_t E,
                            const uint32_t *conn, int message_mode, char *why, size_t cap);
/* Host only: take[e] = 1 for the global edge rows strip `strip` is authoritative for in `phase` (0 or 1).  A strip
 * stores a row for every edge with an own endpoint, but a visit writes a cross-strip message only into the copy of
 * the strip that owns the RECEIVING end: at rest in phase 1 the valid copy of an edge is with the owner of its endpoint
 * later in the node order, in phase 0 with the owner of the earlier one.  Over the strips every edge is taken once.
 * Nonzero on a bad argument (the reason: stereo_hip_last_error). */
int stereo_trws_strip_state_rows_host(int64_t N, int64_t E, const uint32_t *conn, const int32_t *owner, int nstrips,
                                      int strip, int phase, uint8_t *take);
/* Diagnostics (any output may be NULL). */
int stereo_trws_plan_strip_info(stereo_trws_plan *plan, int *nstrips, int *strip, int64_t *own_nodes,
                                int64_t *runs_forward, int64_t *runs_backward, int *needs_previous,
                                int *needs_next);
/* Development aid: completion flags (N, by rank: epoch of the last completed visit) and
 * [ticket, abort] of the plan's last launch. */
int stereo_trws_plan_debug_flags(stereo_trws_plan *plan, int32_t *done, int32_t *ctl);
/* Development aids: the lower-bound terms of the plan's last backward sweep in the order the host sums them (rank N - 1
 * down to 0: the node's own term, minimize.cpp:79-83, then one per message it sent, :85-91), and the message rows as
 * they lie in HBM (E x K doubles, edge-major).  No reference counterpart. */
int stereo_trws_plan_debug_terms(stereo_trws_plan *plan, double *lb_terms, int64_t cap, int64_t *n_lb);
int stereo_trws_plan_debug_messages(stereo_trws_plan *plan, double *out, int64_t count);
/* Development aid, host only (no device): the rule that picks a plan's sweep kernel family.  Facts of the
 * plan: kernel, K, message_mode, fast_ok (the graph suits the pipelined kernels), fast_switch (STEREO_HIP_TRWS_FAST is
 * not 0), strips (the plan is a row strip).  Facts of its inputs: positions = 0 q / qprim per edge, 1 one shared vector
 * that is not finite and strictly ascending, 2 one that is, -1 no inputs yet; lambda.  Returns what stereo_trws_plan_path
 * would, or 0 with the refusal the plan gives in err. */
int stereo_trws_family_rule(int kernel, int K, int message_mode, int fast_ok, int fast_switch, int strips,
                            int positions, double lambda, char *err, size_t errcap);
/* Development aid, host only (no device): the rule that picks the kernel of stereo_ncc_volume and its launch geometry
 * (stereo_amd/csrc/ncc_rule.h).  Facts: H, W, the D host disparities, patchsize, layout, cus (the device's compute-unit
 * count), naive (STEREO_HIP_NCC_NAIVE is set), rowlanes (STEREO_HIP_NCC_ROWLANES is set).  *path = 0 ncc_volume_kernel
 * (per tap), 1 ncc_cross_kernel, 2 ncc_lane_kernel; for path 2 *cols = columns per workgroup, *chunks = column chunks
 * of the grid and *span = the largest max - min over the 64-label chunks of the disparities, all 0 for the other paths.
 * Any output may be NULL.  Returns 0, or 1 with the reason in err for an argument stereo_ncc_volume refuses. */
int stereo_ncc_volume_rule(int H, int W, const double *disparities, int D, int patchsize, int layout, int cus, int naive,
                           int rowlanes, int *path, int *cols, int *chunks, int *span, char *err, size_t errcap);
/* The gateway on several devices.  With STEREO_HIP_GPUS=G (2 .. 16) in the environment stereo_trws -- what trws_mex
 * reaches, cpp/trws_mex.cpp:149-164 -- cuts the problem into G row strips when the graph is the image grid of
 * dispmap_super.m:279-302 (nodes col * H + row, 4-neighbourhood, H >= 2 G; K <= 128, or <= 256 with one positions vector
 * in every column of q and qprim): strip g on device g when the process sees G devices (peer access over xGMI), all
 * strips on the current device otherwise (logical strips, one fused launch per sweep).  Same labels, energy, bound and
 * iteration count as on one device.  stereo_trws_min_marginals follows the same rule only with
 * STEREO_HIP_TRWS_BELIEFS_STRIPS=1 set as well.  This call tells how many strips the calling thread's last stereo_trws /
 * stereo_trws_min_marginals ran on (1: the single-device plan).  No reference counterpart. */
int stereo_trws_gateway_strips(void);

/* Host only (no device): the speculative schedule of the graph's one long serial run, if it has one (DESIGN.md 4.5;
 * stereo_trws_plan_spec_stats).  info[0..5] = exists, the run of stereo_trws_schedule that is cut, its first schedule
 * position, one past its last, visits per segment, segments.  The arrays (may be NULL) describe the schedule with that
 * run replaced by its segments: run_ptr (*nruns + 1 schedule positions), kind (*nruns: 0, or 1 + segment index),
 * ticket_run (*nruns + 1 tickets; -1 = the runner's ticket, the first).  No reference counterpart. */
int stereo_trws_spec_schedule(int64_t N, int64_t E, const uint32_t *connectivity0, int direction, int64_t *info,
                              int64_t *nruns, int64_t *run_ptr, int64_t *kind, int64_t *ticket_run, char *err,
                              size_t errcap);

/* Host only (no device): the descriptors of the descriptor-driven kernels' chain schedule, N x 64 int32 in schedule
 * order (stereo_trws_schedule's positions; layout in trws_graph.h).  No reference counterpart. */
int stereo_trws_descriptors_host(int64_t N, int64_t E, const uint32_t *connectivity0, int direction, int32_t *desc,
                                 char *err, size_t errcap);

/* stereo_trws_schedule with strips: additionally run_strip (N provided, *nruns used) = strip of
 * every run, remote (N, by rank) = descriptor word 43 (bits 0-7: outgoing message k is written
 * to a neighbour, 8-15: which one, 16 / 17: flag and label also raised at strip - 1 / + 1). */
int stereo_trws_schedule_strips(int64_t N, int64_t E, const uint32_t *conn, int64_t max_resident_runs,
                                int direction, const int32_t *owner, int nstrips, int64_t *rank_at,
                                int64_t *run_ptr, int64_t *nruns, int64_t *ticket_run,
                                int64_t *pred_rank, int64_t *dep_ptr, int64_t *dep_rank,
                                int64_t *run_strip, int64_t *remote, char *err, size_t errcap);

/* Host-only graph analysis behind stereo_trws_plan_create (no device needed):
 * node order of SetAutomaticOrdering (ordering.cpp:7-157), edge orientation and
 * per-node forward/backward edge lists of CompleteGraphConstruction
 * (MRFEnergy.cpp:137-229), and the dependency level of every node.
 * rank: N; tail, head: E (after orientation); mdir: E (Swap parity);
 * fwd_ptr, bwd_ptr: N+1 CSR offsets indexed by NODE ID; fwd_idx, bwd_idx: E
 * edge ids in list order; level: N (indexed by node id).  Any output may be NULL. */
int stereo_trws_analyze(int64_t N, int64_t E, const uint32_t *conn, int64_t *rank,
                        int64_t *tail, int64_t *head, int32_t *mdir, int64_t *fwd_ptr,
                        int64_t *fwd_idx, int64_t *bwd_ptr, int64_t *bwd_idx, int64_t *level,
                        char *err, size_t errcap);

/* Host-only inspection of the dataflow schedule the descriptor-driven sweep kernels walk
 * (trws_graph.h "chain schedule"; no reference counterpart -- the reference is serial,
 * minimize.cpp:36-95).  direction 0 = forward sweep, 1 = backward.  max_resident_runs as
 * passed by stereo_trws_plan_create (0 = unlimited).  Outputs (any may be NULL):
 * rank_at (N): rank visited at schedule position p; run_ptr (N+1 entries provided, *nruns+1
 * used): offsets of the runs in schedule positions; ticket_run (N provided, *nruns used):
 * run picked up with ticket t; pred_rank (N, by rank): rank visited just before in the same
 * run whose messages are handed over in LDS, or -1; dep_ptr (N+1) / dep_rank (4N provided):
 * foreign ranks a node waits for (completion flags).  Returns non-zero if the graph is not
 * eligible for those kernels. */
int stereo_trws_schedule(int64_t N, int64_t E, const uint32_t *conn, int64_t max_resident_runs,
                         int direction, int64_t *rank_at, int64_t *run_ptr, int64_t *nruns,
                         int64_t *ticket_run, int64_t *pred_rank, int64_t *dep_ptr,
                         int64_t *dep_rank, char *err, size_t errcap);

/* ---- QPBO roof-duality binary fusion ---------------------------------- *
 * Replaces cpp/rd_mex.cpp:14-100 mexFunction:
 *   [labelling, energy, lower_bound, num_unlabelled] =
 *       rd_mex(U0, U1, E00, E01, E10, E11, connectivity-1, options)
 * U0,U1 N; E00..E11 E; improve = options.improve (rd_mex.cpp:34, default false).
 * labelling N doubles in {-1,0,1}; num_unlabelled is counted BEFORE Improve
 * (rd_mex.cpp:83-88).
 */
/* Repeated calls with the same connectivity (a fusion schedule: one call per proposal) reuse the plan of
 * the last connectivity seen -- from the second call on a move costs the upload of the six term arrays
 * and the solve (3.7 ms at 450 x 375 instead of 56 ms; STEREO_HIP_RD_CACHE=0 rebuilds per call). */
int stereo_rd(const double *U0, const double *U1, const double *E00, const double *E01,
              const double *E10, const double *E11, const uint32_t *conn, int64_t N,
              int64_t E, int improve, double *labelling, double *energy,
              double *lower_bound, double *num_unlabelled, char *err, size_t errcap);
/* Frees the plan stereo_rd keeps for the last connectivity (its device buffers stay allocated until
 * the next different problem otherwise). */
void stereo_rd_cache_clear(void);

/* Device-resident form of stereo_rd for repeated fusion moves on one connectivity
 * (dispmap_super.m:61-84 is called once per proposal): edge grouping, the doubled-graph
 * slot layout and all device buffers are set up once; a move uploads (or binds) the six term
 * arrays, rebuilds capacities on the device and solves. */
typedef struct stereo_rd_plan stereo_rd_plan;
int stereo_rd_plan_create(int64_t N, int64_t E, const uint32_t *conn, stereo_rd_plan **plan, char *err,
                          size_t errcap);
void stereo_rd_plan_destroy(stereo_rd_plan *plan);
/* Device pointer to the labels of the last solve: N int8 in {-1, 0, 1} (valid until the next solve). */
const int8_t *stereo_rd_plan_device_labels(stereo_rd_plan *plan);
/* Optional hint: the N nodes are the pixels of an H x W image numbered col*H + row
 * (dispmap_super.m:281-282).  Only the internal work partition changes (image patches instead of
 * index ranges per workgroup: fewer grid-wide barriers), never a result. */
int stereo_rd_plan_set_grid(stereo_rd_plan *plan, int H, int W, char *err, size_t errcap);
int stereo_rd_plan_solve(stereo_rd_plan *plan, const double *U0, const double *U1, const double *E00,
                         const double *E01, const double *E10, const double *E11, int improve,
                         double *labelling, double *energy, double *lower_bound,
                         double *num_unlabelled, char *err, size_t errcap);
/* the same with the six term arrays already in HBM (e.g. written by the term-builder kernels);
 * labelling may be NULL: the labels then stay on the device (stereo_rd_plan_device_labels) */
int stereo_rd_plan_solve_device(stereo_rd_plan *plan, const double *d_U0, const double *d_U1,
                                const double *d_E00, const double *d_E01, const double *d_E10,
                                const double *d_E11, int improve, double *labelling, double *energy,
                                double *lower_bound, double *num_unlabelled, char *err, size_t errcap);

/* ---- term builders and cost volume ------------------------------------- *
 * Device versions of the MATLAB array math between the images and the two
 * solvers.  Pixels are numbered column-major, id = col*H + row (dispmap_super.m:281-282);
 * points(:,id) = [col+1; row+1] (:275-278); planes are 4-vectors [a b c d],
 * disparity = -(a*x + b*y + d)/c (:318-328).  d_step != 0 applies the
 * dispmap_globalstereo rescaling (d - d_min)/d_step (dispmap_globalstereo.m:336-345).
 */

/* dispmap_super.m:236-262 all_pairwise_costs (+ :226-235 pairwise_cost).
 * conn 2 x E zero based [ind1; ind2]; points 2 x N; assignment / proposal 4 x N;
 * proposal == NULL computes E00 only (update_energy, :263-274).  Planes with c == 0
 * fail with "Infinite disparity" (:323-325). */
int stereo_pairwise_terms(int kernel, int64_t N, int64_t E, const uint32_t *conn, const double *points,
                          const double *assignment, const double *proposal, const double *weights,
                          double tol, double d_min, double d_step, double *E00, double *E01,
                          double *E10, double *E11, char *err, size_t errcap);

/* dispmap_super.m:177-183: q(k,e), qprim(k,e) of K proposals (4 x N x K) -> K x E each. */
int stereo_trws_positions(int64_t N, int64_t E, int K, const uint32_t *conn, const double *points,
                          const double *proposals, double d_min, double d_step, double *q,
                          double *qprim, char *err, size_t errcap);

/* dispmap_ncc.m:116-198 compute_ncc.  im0 = reference image, im1 = the image that is
 * shifted; both H x W x 3 column major doubles.  layout 0: H x W x D (MATLAB, self.ncc);
 * layout 1: D x (H*W), label fastest -- what TRW-S consumes as `unary` after
 * unary_weight*(1 - ncc). */
int stereo_ncc_volume(const double *im0, const double *im1, int H, int W, const double *disparities,
                      int D, int patchsize, int layout, double *ncc, char *err, size_t errcap);

/* dispmap_ncc.m:107-115 unary_cost = unary_weight*(1 - sample_ncc_from_disp(...)) (:222-276). */
int stereo_ncc_unary(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                     double unary_weight, const double *assignment, double *U, char *err,
                     size_t errcap);

/* dispmap_ncc.m:208-221 best_disp_from_ncc (winner takes all + parabola vertex), H x W. */
int stereo_ncc_best_disp(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                         double *best, char *err, size_t errcap);

/* dispmap_globalstereo.m:355-375 unary_cost with ephoto (:405) and the 'linear' branch of
 * vgg_interp2 (imrender/vgg/vgg_interp2.cxx:245-322, oobv = -1000).  P2 = self.P(:,:,2),
 * 4 x 3 column major (already permuted, :43). */
int stereo_globalstereo_unary(const double *im0, const double *im1, int H, int W, int C,
                              const double *P2, double d_min, double d_step, double col_thresh,
                              const double *assignment, double *U, char *err, size_t errcap);

/* ---- left-right consistency: cross-check, occlusion map, fill ------------------------ *
 * No reference counterpart (the reference's maps are single-view).  A disparity map is H x W doubles,
 * column major as stereo_ncc_best_disp writes it: element (y, x) at y + H*x, zero based.  A pixel at
 * column x of the map's own view with disparity d matches column x - direction*d of the other view
 * (dispmap_ncc.m:143-154 is direction = +1, the left-referenced map; -1 is the right-referenced one).
 *
 * Refused with a message: direction other than +1 / -1, tol negative or NaN, H or W below 1,
 * H*W >= 2^31 (columns and sources are int32), NULL for a required array.  H = 1 and W = 1 are valid.
 * The arguments are checked before the device is looked for. */

/* status (int32) and residual (double, may be NULL) per pixel of d_ref:
 *   d = d_ref(y, x) not finite                                  -> status 4, residual NaN
 *   xi = floor(x - direction*d + 0.5) outside 0 .. W - 1         -> status 3 (out of view), residual NaN
 *   dr = d_other(y, xi) not finite                              -> status 4, residual NaN
 *   residual = d - dr;  |residual| <= tol                       -> status 0 (consistent)
 *                       residual < 0                            -> status 1 (occluded: the other view sees
 *                                                                  something nearer there)
 *                       residual > 0                            -> status 2 (mismatch)
 * The nearest column, ties to the higher index; no interpolation of d_other.  Every operation is exact in
 * IEEE double, so the outputs are those of the same lines written in any language, bit for bit. */
int stereo_lr_check(const double *d_ref, const double *d_other, int H, int W, int direction,
                    double tol, int32_t *status, double *residual, char *err, size_t errcap);
/* Row by row: a pixel with status 0 keeps its disparity, source = x.  Any other pixel takes the nearest
 * status-0 pixel of its row at a lower column (l) and at a higher column (r): the one with the smaller
 * disparity (the background) -- r only if its disparity is strictly smaller, l otherwise or if r does not
 * exist -- and source (int32, may be NULL) is that column.  A row without a status-0 pixel: NaN, source -1.
 * Not in place: filled == d_ref and source == status are refused (filled and source hold intermediate values
 * while the inputs are still being read); the four arrays must not overlap. */
int stereo_lr_fill(const double *d_ref, const int32_t *status, int H, int W,
                   double *filled, int32_t *source, char *err, size_t errcap);
/* The same on device arrays of the caller (e.g. torch tensors), launched on `stream` (hipStream_t,
 * NULL = default) without waiting for it. */
int stereo_lr_check_device(const double *d_ref, const double *d_other, int H, int W, int direction,
                           double tol, int32_t *status, double *residual, void *stream, char *err,
                           size_t errcap);
int stereo_lr_fill_device(const double *d_ref, const int32_t *status, int H, int W,
                          double *filled, int32_t *source, void *stream, char *err, size_t errcap);
/* The fill kernel splits a row into `chunks` contiguous column ranges, one wave each (1 .. 16; the results
 * do not depend on it).  stereo_lr_fill_chunks: the number the entries above use;
 * stereo_lr_fill_device_chunks: stereo_lr_fill_device with another one (timing, tests). */
int stereo_lr_fill_chunks(void);
int stereo_lr_fill_device_chunks(const double *d_ref, const int32_t *status, int H, int W,
                                 double *filled, int32_t *source, int chunks, void *stream, char *err,
                                 size_t errcap);

/* ---- band refinement around a solved disparity map ---------------------------------- *
 * No reference counterpart as a call; the problem it builds is the reference's own energy restricted to
 * fronto-parallel per-pixel labels.  From a disparity map `base` (H x W doubles, column major, N = H*W) and a
 * strictly ascending vector `offsets` (K doubles, one of them 0.0), label k at pixel i means disparity
 * base_i + offsets_k.  Unary and positions of label k are exactly what stereo_ncc_unary and
 * stereo_trws_positions give for the proposal whose plane at pixel i is [0, 0, 1, -(base_i + offsets_k)];
 * the plane -> disparity rule (dispmap_super.m:318-328) gives base_i + offsets_k for that plane exactly
 * (with the plane's sign of zero: -0 where the sum is 0).
 *
 * In:  ncc          the NCC volume, layout 0 (H x W x D) or 1 (D x N, label fastest), D slices at `disparities`
 *                   (ascending or not: both branches of the sampler's nearest-slice search), and unary_weight
 *      conn         2 x E zero based, edge e = (i1, i2) = (conn[2e], conn[2e + 1])
 * Out: unary        K x N, label fastest: unary(k, i) = unary_weight * (1 - sample(base_i + offsets_k)), with the
 *                   sampler's rules (dispmap_ncc.m:222-249): ties go to the larger slice index, t2 == 1 or t2 == D
 *                   gives the end slice, a disparity outside [min, max] of `disparities` gives -1e6.  A band label
 *                   that leaves the volume's range therefore costs unary_weight * (1 + 1e6), as the same plane does
 *                   in dispmap_ncc.  Nothing is clamped.
 *      q, qprim     K x E, label fastest: q(k, e) = base_{i2} + offsets_k, qprim(k, e) = base_{i1} + offsets_k
 *                   (the order stereo_trws_positions writes).  E = 0: conn, q and qprim may be NULL.
 * stereo_band_apply: refined_i = base_i + offsets_{label_i - 1}, labels int32 and one based as
 * stereo_trws_plan_result returns them: one addition.
 *
 * Everything is fp64 without FMA contraction and runs the code of stereo_ncc_unary (csrc/ncc_sample.h), so the
 * outputs equal those of K calls of stereo_ncc_unary and one of stereo_trws_positions bit for bit.
 *
 * Refused with a message, before the device is looked for: offsets not finite, not strictly ascending or
 * without 0.0; K < 1 or K > 512 (stereo_band_max_offsets); layout other than 0 / 1; D, H or W below 1;
 * H*W >= 2^31; NULL for a required array.  The host entries also refuse a base entry that is not finite (the
 * message names the pixel), a conn entry outside 0 .. N - 1 and, in apply, a label outside 1 .. K. */
int stereo_band_max_offsets(void);
int stereo_band_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                       double unary_weight, const double *base, const double *offsets, int K, int64_t E,
                       const uint32_t *conn, double *unary, double *q, double *qprim, char *err,
                       size_t errcap);
int stereo_band_apply(const double *base, int H, int W, const int32_t *labels, const double *offsets,
                      int K, double *refined, char *err, size_t errcap);
/* The same on device arrays of the caller (ncc, base, conn, labels and every output), launched on `stream`
 * (hipStream_t, NULL = default) without waiting for it.  The two short vectors are passed twice: `disparities` and
 * `offsets` on the host (they are checked, and min / max / order of the slices come from them) and
 * `d_disparities` / `d_offsets`, the same values in device memory, which the kernels read -- so the entries
 * copy nothing.  `bad` (device int32, may be NULL) is set to zero on `stream` and then incremented once per
 * pixel whose base is not finite (inputs) or whose label is outside 1 .. K (apply: that pixel's refined value
 * is NaN).  The outputs of an offending pixel are unspecified but written.  An edge that names a pixel outside
 * 0 .. N - 1 reads nothing; its positions are NaN. */
int stereo_band_inputs_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                              const double *d_disparities, double unary_weight, const double *base,
                              const double *offsets, const double *d_offsets, int K, int64_t E,
                              const uint32_t *conn, double *unary, double *q, double *qprim, int32_t *bad,
                              void *stream, char *err, size_t errcap);
int stereo_band_apply_device(const double *base, int H, int W, const int32_t *labels, const double *offsets,
                             const double *d_offsets, int K, double *refined, int32_t *bad, void *stream,
                             char *err, size_t errcap);

/* ---- candidate bands: per-pixel label sets propagated from neighbours ------------------ *
 * No reference counterpart as a call; the problem is the reference's own energy restricted to K fronto-parallel
 * labels per pixel, as the band's is, but label k at pixel i means an arbitrary per-pixel disparity cand[k, i], not
 * base_i plus a shared offset.  A pixel whose base is wrong by more than a band's half-width has no band label that
 * is right; if a neighbour at one of the taps, or another map such as the volume's winner-take-all map, is right
 * there, the candidate set holds the right value.
 *
 * The candidate table `cand` is K x N doubles, label fastest (element (k, i) at k + K*i), pixels column major
 * (pixel (y, x) is i = y + H*x, zero based), N = H*W.
 *
 * stereo_candidates_gather builds a table from
 *      base         H x W doubles, column major
 *      offsets      Ko >= 1 doubles under the band's rules: finite, strictly ascending, containing 0.0
 *      sources      M >= 0 maps, H x W doubles each, one after the other (source m starts at sources + m*N)
 *      taps         T >= 0 pairs of int32, (dy_t, dx_t) at taps[2t], taps[2t + 1], |dy|, |dx| < 2^15
 * as
 *      cand[k, i]                      = base_i + offsets_k                                        for k < Ko
 *      cand[Ko + m*T + t, (y, x)]      = src_m[clamp(y + dy_t, 0, H - 1), clamp(x + dx_t, 0, W - 1)]
 * (the value is copied, nothing is added), K = Ko + M*T, 1 <= K <= stereo_band_max_offsets().  Duplicates are allowed
 * and are not removed -- the tap (0, 0), taps clamped at a border, neighbours with equal values: TRW-S's first-minimum
 * rule decides among equal labels, and the applied value is the same either way.  With M*T == 0 sources and taps may
 * be NULL and the table is the band's.
 *
 * stereo_candidates_inputs takes a table (this one or any other the caller brings), not the recipe.  Label k at
 * pixel i is the plane [0, 0, 1, -cand[k, i]]; unary and positions are exactly what stereo_ncc_unary and
 * stereo_trws_positions give for those K proposals, byte for byte:
 *      unary        K x N, label fastest: unary(k, i) = unary_weight * (1 - sample(cand[k, i])) with every rule of the
 *                   sampler as listed for stereo_band_inputs; a candidate outside the volume's range costs
 *                   unary_weight * (1 + 1e6).  Nothing is clamped.
 *      q, qprim     K x E, label fastest: q(k, e) = cand[k, i2], qprim(k, e) = cand[k, i1] for edge e = (i1, i2) =
 *                   (conn[2e], conn[2e + 1]), through the plane -> disparity rule (dispmap_super.m:318-328), which
 *                   gives the candidate itself with the plane's sign of zero (-0 for a candidate of 0).  E = 0: conn, q
 *                   and qprim may be NULL.
 * stereo_candidates_apply: out_i = cand[label_i - 1, i], labels int32 and one based; the value is copied.
 *
 * Everything is fp64 without FMA contraction and runs the code of stereo_ncc_unary (csrc/ncc_sample.h).
 *
 * Refused with a message, before the device is looked for: the band's refusals (offsets not finite, not strictly
 * ascending or without 0.0; Ko < 1; layout other than 0 / 1; D, H or W below 1; H*W >= 2^31; NULL for a required
 * array); K outside 1 .. stereo_band_max_offsets(); M < 0 or T < 0; M*T > 0 with NULL sources or taps; |dy| or
 * |dx| >= 2^15.  The host entries also refuse a base, source or candidate value that is not finite (the message names
 * the pixel, and for a candidate the label), a conn entry outside 0 .. N - 1 and, in apply, a label outside 1 .. K. */
int stereo_candidates_gather(const double *base, int H, int W, const double *offsets, int Ko, const double *sources,
                             int M, const int32_t *taps, int T, double *cand, char *err, size_t errcap);
int stereo_candidates_inputs(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                             double unary_weight, const double *cand, int K, int64_t E, const uint32_t *conn,
                             double *unary, double *q, double *qprim, char *err, size_t errcap);
int stereo_candidates_apply(const double *cand, int H, int W, int K, const int32_t *labels, double *out, char *err,
                            size_t errcap);
/* The same on device arrays of the caller (base, sources, cand, ncc, conn, labels and every output), launched on
 * `stream` (hipStream_t, NULL = default) without waiting for it, with the conventions of stereo_band_inputs_device:
 * the short vectors are passed twice, on the host (`offsets`, `taps`, `disparities`: checked) and on the device
 * (`d_offsets`, `d_taps`, `d_disparities`: read by the kernels), so the entries copy nothing.  `bad` (device int32,
 * may be NULL) is set to zero on `stream` and then incremented once per offending pixel: in gather a pixel at which
 * the base or one of the sources is not finite, in inputs a pixel with a candidate that is not finite, in apply a pixel
 * whose label is outside 1 .. K (its value is NaN).  The outputs of an offending pixel are unspecified but written.
 * An edge that names a pixel outside 0 .. N - 1 reads nothing of that pixel; its positions are NaN. */
int stereo_candidates_gather_device(const double *base, int H, int W, const double *offsets, const double *d_offsets,
                                    int Ko, const double *sources, int M, const int32_t *taps, const int32_t *d_taps,
                                    int T, double *cand, int32_t *bad, void *stream, char *err, size_t errcap);
int stereo_candidates_inputs_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                    const double *d_disparities, double unary_weight, const double *cand, int K,
                                    int64_t E, const uint32_t *conn, double *unary, double *q, double *qprim,
                                    int32_t *bad, void *stream, char *err, size_t errcap);
int stereo_candidates_apply_device(const double *cand, int H, int W, int K, const int32_t *labels, double *out,
                                   int32_t *bad, void *stream, char *err, size_t errcap);

/* ---- plane candidates: per-pixel plane sets propagated from neighbours ----------------- *
 * No reference counterpart as a call; the problem is the reference's own energy restricted to K planes per pixel.
 * Label k at pixel i means an arbitrary per-pixel PLANE pcand[:, k, i], not the fronto-parallel plane
 * [0, 0, 1, -cand[k, i]] of the candidate bands above and not only pixel i's own plane moved along the disparity
 * axis as in the plane band below.  A plane is a function on the whole image, so a plane copied from a neighbour is
 * that neighbour's surface extended to this pixel: on a slanted surface the copy is right where a copied disparity
 * is wrong by slope times tap distance.
 *
 * The plane candidate table `pcand` is 4 x K x N doubles: component j of label k at pixel i at j + 4*(k + K*i),
 * pixels column major (pixel (y, x) is i = y + H*x, zero based), N = H*W, 1 <= K <= stereo_band_max_offsets().
 *
 * stereo_plane_candidates_gather builds a table from
 *      planes       4 x N doubles, column major: the current assignment [a b c d] per pixel
 *      offsets      Ko >= 1 doubles under the band's rules: finite, strictly ascending, containing 0.0
 *      sources      M >= 0 plane maps, 4 x N doubles each, one after the other (source m starts at sources + 4*m*N)
 *      taps         T >= 0 pairs of int32, (dy_t, dx_t) at taps[2t], taps[2t + 1], |dy|, |dx| < 2^15
 * as
 *      pcand[:, k, i]                  = [a_i, b_i, c_i, d_i - c_i * offsets_k]                     for k < Ko
 *      pcand[:, Ko + m*T + t, (y, x)]  = src_m[:, clamp(y + dy_t, 0, H - 1) + H * clamp(x + dx_t, 0, W - 1)]
 * The first is the plane band's label (one fp64 multiplication, one fp64 subtraction, no contraction); in the second
 * the four doubles are copied and nothing is re-anchored.  K = Ko + M*T.  Duplicates are allowed and are not removed,
 * as for stereo_candidates_gather.  With M*T == 0 sources and taps may be NULL and the table is the plane band's.
 *
 * stereo_plane_candidates_inputs_ncc / _globalstereo take a table (this one or any other the caller brings), not the
 * recipe, and give exactly what the library's existing entries give for the K proposals P_k = pcand[:, k, :], byte
 * for byte:
 *      unary        K x N, label fastest: unary(k, i) is what stereo_ncc_unary (_ncc) or stereo_globalstereo_unary
 *                   (_globalstereo) gives for proposal k at pixel i, whose point is [i / H + 1, i % H + 1], formed in
 *                   the kernel (csrc/ncc_sample.h, csrc/gs_sample.h: one copy of each sampler).
 *      q, qprim     K x E, label fastest: for e = (i1, i2) = (conn[2e], conn[2e + 1]), q(k, e) = plane pcand[:, k, i2]
 *                   at the point of i2 and qprim(k, e) = plane pcand[:, k, i1] at the point of i2, through the
 *                   plane -> disparity rule (dispmap_super.m:318-328), with d_min = d_step = 0 for _ncc and the
 *                   (v - d_min) / d_step rescaling for _globalstereo: what stereo_trws_positions writes.  E = 0: conn,
 *                   q and qprim may be NULL.
 * stereo_plane_candidates_apply: out[:, i] = pcand[:, label_i - 1, i], 4 x N, labels int32 and one based; the values
 * are copied.
 *
 * Everything is fp64 without FMA contraction.
 *
 * Refused with a message, before the device is looked for: the band's refusals (offsets not finite, not strictly
 * ascending or without 0.0; Ko < 1; layout other than 0 / 1; D, H, W or C below 1; H*W >= 2^31; NULL for a required
 * array; d_step == 0 for _globalstereo); K outside 1 .. stereo_band_max_offsets(); M < 0 or T < 0; M*T > 0 with NULL
 * sources or taps; |dy| or |dx| >= 2^15; E < 0.  The host entries also refuse a plane -- of `planes`, of a source or
 * of the table -- with a component that is not finite or with c == 0 ("Infinite disparity", dispmap_super.m:323-325);
 * the message names the pixel and, for a table entry, the label.  They refuse a conn entry outside 0 .. N - 1 and,
 * in apply, a label outside 1 .. K. */
int stereo_plane_candidates_gather(const double *planes, int H, int W, const double *offsets, int Ko,
                                   const double *sources, int M, const int32_t *taps, int T, double *pcand, char *err,
                                   size_t errcap);
int stereo_plane_candidates_inputs_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                       double unary_weight, const double *pcand, int K, int64_t E,
                                       const uint32_t *conn, double *unary, double *q, double *qprim, char *err,
                                       size_t errcap);
int stereo_plane_candidates_inputs_globalstereo(const double *im0, const double *im1, int H, int W, int C,
                                                const double *P2, double d_min, double d_step, double col_thresh,
                                                const double *pcand, int K, int64_t E, const uint32_t *conn,
                                                double *unary, double *q, double *qprim, char *err, size_t errcap);
int stereo_plane_candidates_apply(const double *pcand, int H, int W, int K, const int32_t *labels, double *out,
                                  char *err, size_t errcap);
/* The same on device arrays of the caller (planes, sources, pcand, ncc / im0 / im1, conn, labels and every output),
 * launched on `stream` (hipStream_t, NULL = default) without waiting for it, with the conventions of
 * stereo_candidates_*_device and stereo_plane_band_*_device: the short vectors are passed twice, on the host
 * (`offsets`, `taps`, `disparities`: checked) and on the device (`d_offsets`, `d_taps`, `d_disparities`: read by the
 * kernels), so the entries copy nothing; P2 is 12 host doubles and travels as a kernel argument.  A plane moves as two
 * 16-byte accesses: planes, sources, pcand and out must be 16-byte aligned (refused otherwise).  `bad` (device
 * int32, may be NULL) is set to zero on `stream` and then incremented once per offending pixel: in gather a pixel at
 * which the own plane or a source's plane AT THAT PIXEL has a component that is not finite or c == 0, in inputs a pixel
 * with such a candidate, in apply a pixel whose label is outside 1 .. K (its four outputs are NaN).  The outputs of
 * an offending pixel are unspecified but written.  An edge that names a pixel outside 0 .. N - 1 reads nothing of
 * that pixel; its positions are NaN. */
int stereo_plane_candidates_gather_device(const double *planes, int H, int W, const double *offsets,
                                          const double *d_offsets, int Ko, const double *sources, int M,
                                          const int32_t *taps, const int32_t *d_taps, int T, double *pcand,
                                          int32_t *bad, void *stream, char *err, size_t errcap);
int stereo_plane_candidates_inputs_ncc_device(const double *ncc, int H, int W, int D, int layout,
                                              const double *disparities, const double *d_disparities,
                                              double unary_weight, const double *pcand, int K, int64_t E,
                                              const uint32_t *conn, double *unary, double *q, double *qprim,
                                              int32_t *bad, void *stream, char *err, size_t errcap);
int stereo_plane_candidates_inputs_globalstereo_device(const double *im0, const double *im1, int H, int W, int C,
                                                       const double *P2, double d_min, double d_step,
                                                       double col_thresh, const double *pcand, int K, int64_t E,
                                                       const uint32_t *conn, double *unary, double *q, double *qprim,
                                                       int32_t *bad, void *stream, char *err, size_t errcap);
int stereo_plane_candidates_apply_device(const double *pcand, int H, int W, int K, const int32_t *labels, double *out,
                                         int32_t *bad, void *stream, char *err, size_t errcap);

/* ---- messages carried from one band level or pyramid scale to the next --------------- *
 * No reference counterpart.  A chain of band problems solves every level around the map the level before produced;
 * this operator turns the messages that level left (M_old: E_old x K_old doubles, label fastest, a solver state's
 * layout) into messages on the next level's label grid (M_new: E_new x K_new), so that the next level starts from
 * them instead of from zero.  Any message array is a valid reparametrisation: a level that starts from carried
 * messages still reports a true lower bound, only its speed depends on them.
 *
 * A message row is a function on the labels of its RECEIVING node (stereo_trws_state_receivers_host).  Old label i
 * of a node lies at off_old[i] on that node's offset axis, new label j of node r at shift[r] + stretch * off_new[j]
 * on the old axis of the node r inherits from.  For every new edge e, in fp64 without contraction, in this order:
 *   s = edge_src ? edge_src[e] : e;  r = receiver_new[e];  t = shift[r]
 *   s < 0 or t not finite: the row is all zeros.  Otherwise for j = 0 .. K_new - 1:
 *     u = t + stretch * off_new[j]                                  (the multiply first)
 *     u <= off_old[0]:          v_j = M_old[s][0]
 *     u >= off_old[K_old - 1]:  v_j = M_old[s][K_old - 1]           (flat outside the old range, as a truncated
 *                                                                    pairwise term makes messages there)
 *     else, i the largest index with off_old[i] <= u and w = (u - off_old[i]) / (off_old[i + 1] - off_old[i]):
 *                               v_j = M_old[s][i] + w * (M_old[s][i + 1] - M_old[s][i])
 *   m = min_j v_j, the first minimum (strict <, so a NaN never wins);  M_new[e][j] = gain * (v_j - m)
 * An edge_src entry >= E_old or a receiver_new entry outside 0 .. N_new - 1 reads nothing: its row is zero and it
 * counts once in `bad`.
 *
 * off_old: K_old doubles, strictly ascending, need not contain 0 (1 <= K_old <= 4096: a full-range solve with shared
 * positions may be the source, its disparities the offsets).  off_new: K_new doubles, strictly ascending,
 * 1 <= K_new <= stereo_band_max_offsets().  shift: N_new doubles.  edge_src, receiver_new: E_new int32; edge_src may
 * be NULL (s = e), then E_old == E_new is required.  E_old, E_new < 2^31.
 *
 * Refused with a message that names the argument, before the device is looked for: a NULL required array; a K out of
 * range; offsets not finite or not strictly ascending; stretch or gain not finite or not positive; E_old != E_new
 * without edge_src; an output (M_new, bad) that is also an input.
 *
 * stereo_band_carry: host arrays in and out, the count of offending edges in *bad (may be NULL).
 * stereo_band_carry_device: device arrays of the caller, launched on `stream` (hipStream_t, NULL = default) without
 * waiting for it; the offsets are passed twice as in stereo_band_inputs_device (host: checked; device: read by the
 * kernel); `bad` (device int32, may be NULL) is set to zero on `stream` first. */
int stereo_band_carry(const double *M_old, int64_t E_old, int K_old, const double *off_old, const int32_t *edge_src,
                      const int32_t *receiver_new, int64_t N_new, const double *shift, double stretch, double gain,
                      const double *off_new, int K_new, int64_t E_new, double *M_new, int64_t *bad, char *err,
                      size_t errcap);
int stereo_band_carry_device(const double *M_old, int64_t E_old, int K_old, const double *off_old,
                             const double *d_off_old, const int32_t *edge_src, const int32_t *receiver_new,
                             int64_t N_new, const double *shift, double stretch, double gain, const double *off_new,
                             const double *d_off_new, int K_new, int64_t E_new, double *M_new, int32_t *bad,
                             void *stream, char *err, size_t errcap);
/* Host only (no device): receiver[e] = the node on whose labels the message row of edge e is indexed in a solver
 * state of `phase` of a plan created with (N, E, conn, message_mode): the endpoint LATER in the
 * plan's node order in phases 1 and 2 (`head` of stereo_trws_analyze), the EARLIER one (`tail`) in phase 0.
 * STEREO_TRWS_ORDER_INDEX in message_mode is honoured. */
int stereo_trws_state_receivers_host(int64_t N, int64_t E, const uint32_t *conn, int message_mode, int phase,
                                     int32_t *receiver, char *err, size_t errcap);

/* ---- band refinement around a solved plane map ----------------------------------------- *
 * No reference counterpart as a call; the problem it builds is the reference's own energy restricted to K
 * per-pixel labels.  From `planes` (4 x N column major, N = H*W: an object's assignment [a b c d] per pixel) and a
 * strictly ascending vector `offsets` (K doubles, one of them 0.0, in the planes' own disparity units), label k
 * at pixel i means pixel i's own plane moved by offsets_k along the disparity axis:
 *     [a_i, b_i, c_i, d_i - c_i * offsets_k]      (one fp64 multiplication, one fp64 subtraction, no contraction)
 * In exact arithmetic its disparity at any point is plane i's disparity plus offsets_k; two pixels on one slanted
 * plane keep q == qprim for every label, which the fronto-parallel band above gives up.
 *
 * Everything else is the library's existing code on those K proposals: unary(k, i) is what stereo_ncc_unary
 * (_ncc) or stereo_globalstereo_unary (_globalstereo) gives for proposal k; q(k, e), qprim(k, e) for
 * e = (i1, i2) = (conn[2e], conn[2e + 1]) are what stereo_trws_positions gives -- q the shifted plane of i2 at the
 * point of i2, qprim the shifted plane of i1 at the point of i2 -- with d_min = d_step = 0 for _ncc and the
 * (v - d_min) / d_step rescaling for _globalstereo.  A pixel's point is [id / H + 1, id % H + 1], formed in the
 * kernel.  unary is K x N, q and qprim are K x E, label fastest; E = 0: conn, q and qprim may be NULL.  The outputs
 * equal those of K calls of the unary entry and one of stereo_trws_positions bit for bit (csrc/ncc_sample.h,
 * csrc/gs_sample.h: one copy of each sampler).
 * stereo_plane_band_apply: refined_i = [a_i, b_i, c_i, d_i - c_i * offsets_{label_i - 1}], 4 x N, labels int32 and
 * one based as stereo_trws_plan_result returns them.
 *
 * Refused with a message, before the device is looked for: the offset rules of the band above and K outside
 * 1 .. stereo_band_max_offsets(); layout other than 0 / 1; D, H, W or C below 1 (apply: N below 1); H*W >= 2^31
 * (apply: N >= 2^31); NULL for a required array; d_step == 0 for _globalstereo.  The host entries also refuse a plane
 * with c == 0 ("Infinite disparity", dispmap_super.m:323-325) or a component that is not finite, a conn entry
 * outside 0 .. N - 1 and, in apply, a label outside 1 .. K; the message names the pixel. */
int stereo_plane_band_inputs_ncc(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                 double unary_weight, const double *planes, const double *offsets, int K,
                                 int64_t E, const uint32_t *conn, double *unary, double *q, double *qprim,
                                 char *err, size_t errcap);
int stereo_plane_band_inputs_globalstereo(const double *im0, const double *im1, int H, int W, int C,
                                          const double *P2, double d_min, double d_step, double col_thresh,
                                          const double *planes, const double *offsets, int K, int64_t E,
                                          const uint32_t *conn, double *unary, double *q, double *qprim,
                                          char *err, size_t errcap);
int stereo_plane_band_apply(const double *planes, int64_t N, const int32_t *labels, const double *offsets,
                            int K, double *refined, char *err, size_t errcap);
/* The same on device arrays of the caller (ncc / im0 / im1, planes, conn, labels and every output), launched on
 * `stream` (hipStream_t, NULL = default) without waiting for it, with the conventions of stereo_band_inputs_device:
 * the short vectors are passed twice, on the host (checked) and in device memory (read by the kernels); P2 is
 * 12 host doubles and travels as a kernel argument.  `bad` (device int32, may be NULL) is set to zero on `stream`
 * and then incremented once per pixel whose plane has c == 0 or a component that is not finite (inputs) or, in
 * apply, such a plane or a label outside 1 .. K: that pixel's refined plane is four NaN.  The outputs of an
 * offending pixel are unspecified but written.  An edge that names a pixel outside 0 .. N - 1 reads nothing; its
 * positions are NaN. */
int stereo_plane_band_inputs_ncc_device(const double *ncc, int H, int W, int D, int layout,
                                        const double *disparities, const double *d_disparities,
                                        double unary_weight, const double *planes, const double *offsets,
                                        const double *d_offsets, int K, int64_t E, const uint32_t *conn,
                                        double *unary, double *q, double *qprim, int32_t *bad, void *stream,
                                        char *err, size_t errcap);
int stereo_plane_band_inputs_globalstereo_device(const double *im0, const double *im1, int H, int W, int C,
                                                 const double *P2, double d_min, double d_step,
                                                 double col_thresh, const double *planes, const double *offsets,
                                                 const double *d_offsets, int K, int64_t E, const uint32_t *conn,
                                                 double *unary, double *q, double *qprim, int32_t *bad,
                                                 void *stream, char *err, size_t errcap);
int stereo_plane_band_apply_device(const double *planes, int64_t N, const int32_t *labels, const double *offsets,
                                   const double *d_offsets, int K, double *refined, int32_t *bad, void *stream,
                                   char *err, size_t errcap);

/* ---- image pyramid: box reduction and map expansion ---------------------------------- *
 * No reference counterpart.  An image is H x W x C doubles and a map H x W doubles, column major: element
 * (y, x, c) at y + H*(x + W*c), zero based.  The coarse size of H x W is Hc = (H + 1) / 2, Wc = (W + 1) / 2.
 * Everything is fp64 without FMA contraction in the order written here, so the outputs are those of the same
 * lines in any language, bit for bit.
 *
 * stereo_pyramid_reduce: out (Hc x Wc x C):
 *     out(yc, xc, c) = 0.25 * (((a00 + a10) + a01) + a11),  a_ij = im(min(2 yc + i, H - 1), min(2 xc + j, W - 1), c)
 * (i the row offset, j the column offset): the 2 x 2 box, the last row / column replicated at an odd size.  A coarse
 * pixel covers the fine columns 2 xc and 2 xc + 1 in both views of a rectified pair, so a fine disparity d is d / 2
 * at the coarse scale, without an offset.
 *
 * stereo_pyramid_expand: out (H x W) and source (int32, H x W, may be NULL) from d_coarse (Hc x Wc).  For the fine
 * pixel (y, x): parent (yc, xc) = (y >> 1, x >> 1); ny = yc + 1 for an odd y, yc - 1 for an even one, clamped to
 * 0 .. Hc - 1; nx the same from x and Wc.  Candidates, in this order: 0 (yc, xc), 1 (ny, xc), 2 (yc, nx), 3 (ny, nx):
 * the coarse pixels of the fine pixel's bilinear footprint under the box reduction.
 *   mode 0 (nearest): out = 2 * d_coarse(candidate 0) whatever that value is, source = 0; im_fine and im_coarse are
 *     not read and may be NULL.
 *   mode 1 (guided by the view's own image, im_fine H x W x C and im_coarse Hc x Wc x C): a candidate whose
 *     disparity is not finite is skipped; a remaining candidate's distance is ((e0*e0 + e1*e1) + ...) over the
 *     channels in order, e_c = im_fine(y, x, c) - im_coarse(candidate, c); the first remaining candidate is the best
 *     until a later one has a strictly smaller distance (ties and NaN distances keep the earlier one);
 *     out = 2 * d_coarse(best), source = its number.  No candidate remains: out = NaN, source = -1.
 * The map is never interpolated.
 *
 * Refused with a message, before the device is looked for: H, W or C below 1; H*W >= 2^31; NULL for a required
 * array; Hc, Wc that are not the coarse size of H, W; a mode other than 0 / 1; an output that is an input (out ==
 * im, out or source == d_coarse / im_fine / im_coarse, source == out). */
int stereo_pyramid_reduce(const double *im, int H, int W, int C, double *out, char *err, size_t errcap);
int stereo_pyramid_expand(const double *d_coarse, int Hc, int Wc, int H, int W, int mode,
                          const double *im_fine, const double *im_coarse, int C, double *out,
                          int32_t *source, char *err, size_t errcap);
/* The same on device arrays of the caller, launched on `stream` (hipStream_t, NULL = default) without waiting
 * for it. */
int stereo_pyramid_reduce_device(const double *im, int H, int W, int C, double *out, void *stream, char *err,
                                 size_t errcap);
int stereo_pyramid_expand_device(const double *d_coarse, int Hc, int Wc, int H, int W, int mode,
                                 const double *im_fine, const double *im_coarse, int C, double *out,
                                 int32_t *source, void *stream, char *err, size_t errcap);

/* ---- plane pyramid: a plane map to the next finer scale, and the local plane fit ------- *
 * No reference counterpart.  A plane map is 4 x N doubles, column major: component j of pixel (y, x) at
 * j + 4*(y + H*x), zero based; a plane [a b c d] has the disparity -((a*X + b*Y) + d) / c at the 1-based point
 * (X, Y) = (x + 1, y + 1) (dispmap_super.m:318-328).  A plane is VALID when its four components are finite and
 * c != 0.  fp64 without FMA contraction in the order written here: bit for bit the same lines in any language.
 *
 * stereo_pyramid_expand_planes: out (4 x N, N = H*W) and source (int32, H x W, may be NULL) from p_coarse (4 x Nc,
 * Nc = Hc*Wc).  The size rule, the candidates 0 .. 3 of a fine pixel and the guided choice are stereo_pyramid_expand's
 * (one copy in the library), with "the candidate's plane is valid" in the place of "its disparity is finite":
 *   mode 0 (nearest): candidate 0 and source = 0; out is four NaN if that plane is not valid.
 *   mode 1 (guided): among the valid candidates, the first one whose squared colour distance no later one undercuts;
 *     none valid: out is four NaN, source = -1.
 * The chosen plane [a b c d] is written as
 *     [a, b, c, (2.0*d + 0.5*a) + 0.5*b]
 * The fine pixel x (zero based) sits at the coarse zero-based coordinate (x + 0.5) / 2 - 0.5, that is at the 1-based
 * coarse X_c = (X_f + 0.5) / 2 for the 1-based fine X_f, and one coarse disparity unit is two fine ones: the fine
 * plane's disparity at every fine point is twice the coarse plane's at that point's coarse coordinate (exactly, for
 * dyadic planes).  The transform is applied uniformly: also at the replicated last row or column of an odd size, where
 * the box reduction's footprint is one fine pixel wide and the coarse pixel's centre strictly lies half a fine pixel
 * further in.  A fronto-parallel [0 0 1 -v] becomes [0 0 1 -2v], the value stereo_pyramid_expand gives; for v == 0 the
 * two additions leave d = +0.0 where negating the expanded map gives -0.0 (equal values, another sign bit).
 * Refused with a message, before the device is looked for: stereo_pyramid_expand's refusals; any overlap of out with
 * p_coarse or an image, or of source with out or p_coarse; in the device form a p_coarse or out that is not 16-byte
 * aligned (a plane moves as two 16-byte accesses).
 *
 * stereo_planes_fit_local: out (4 x N) from planes (4 x N), radius r in 1 .. 8 and tau >= 0 (+inf allowed) in the
 * planes' own disparity units.  z_n is plane n's disparity at its own pixel, by the rule above with s = a*X + b*Y,
 * z = -(s + d) / c; NaN for a plane that is not valid.  For the pixel i = (y, x) with a valid plane, over the taps
 * n = (y + dy, x + dx) inside the image, dx = -r .. r ascending in the outer loop and dy = -r .. r ascending in the
 * inner one, with e = z_n - z_i, those with |e| <= tau (a NaN fails) are accumulated, each sum as S = S + term:
 *     n += 1   Sx += dx   Sy += dy   Sxx += dx*dx   Sxy += dx*dy   Syy += dy*dy   Sz += e   Sxz += dx*e   Syz += dy*e
 * (The six sums without e are whole numbers below 2^15: exact in fp64 whatever the order, so an implementation may
 * keep them as integers and convert them once; the order matters for Sz, Sxz and Syz only.)
 * Then the normal equations of e ~ alpha*dx + beta*dy + gamma are solved by cofactors:
 *     c00 = Syy*n - Sy*Sy     c01 = Sxy*n - Sy*Sx     c02 = Sxy*Sy - Syy*Sx
 *     det = (Sxx*c00 - Sxy*c01) + Sx*c02
 *     c11 = Sxx*n - Sx*Sx     c12 = Sxx*Sy - Sxy*Sx   c22 = Sxx*Syy - Sxy*Sxy
 *     alpha = ((c00*Sxz - c01*Syz) + c02*Sz) / det
 *     beta  = ((c11*Syz - c01*Sxz) - c12*Sz) / det
 *     gamma = ((c02*Sxz - c12*Syz) + c22*Sz) / det
 * unless n < 3 or det > 0 does not hold: then alpha = beta = gamma = 0, the pixel's own fronto-parallel plane (so it
 * is everywhere in an image one pixel wide or high, whose taps are collinear: det = 0).  The output is
 *     [-alpha, -beta, 1, -(((z_i + gamma) - alpha*X) - beta*Y)]
 * A pixel whose own plane is not valid keeps it, copied, and is counted in `bad`.  The fit sees only z: a slanted
 * plane map and the fronto-parallel planes of the same surface give the same output.
 * `bad`: in the host form a host int32 (may be NULL) that receives the count; in the device form a device int32 (may
 * be NULL), set to zero on `stream` and then incremented once per such pixel, as in stereo_plane_band_*_device.
 * Refused with a message, before the device is looked for: NULL planes or out; H or W below 1; H*W >= 2^31; a radius
 * outside 1 .. 8; a tau that is negative or NaN; out overlapping planes; in the device form planes or out not
 * 16-byte aligned. */
int stereo_pyramid_expand_planes(const double *p_coarse, int Hc, int Wc, int H, int W, int mode,
                                 const double *im_fine, const double *im_coarse, int C, double *out,
                                 int32_t *source, char *err, size_t errcap);
int stereo_planes_fit_local(const double *planes, int H, int W, int radius, double tau, double *out, int32_t *bad,
                            char *err, size_t errcap);
/* The same on device arrays of the caller, launched on `stream` (hipStream_t, NULL = default) without waiting
 * for it. */
int stereo_pyramid_expand_planes_device(const double *p_coarse, int Hc, int Wc, int H, int W, int mode,
                                        const double *im_fine, const double *im_coarse, int C, double *out,
                                        int32_t *source, void *stream, char *err, size_t errcap);
int stereo_planes_fit_local_device(const double *planes, int H, int W, int radius, double tau, double *out,
                                   int32_t *bad, void *stream, char *err, size_t errcap);

/* ---- image pyramid: a level's volume as the block mean of the finer volume ------------ *
 * No reference counterpart.  `ncc` is an NCC volume of H x W pixels and D slices at `disparities`, layout 0
 * (H x W x D, element (y, x, k) at y + H*(x + W*k)) or 1 (D x N, element (y, x, k) at k + D*(y + H*x)), as
 * elsewhere.  Hc = (H + 1) / 2, Wc = (W + 1) / 2.  v(y, x, j) is the NCC sampler's value (dispmap_ncc.m:222-249,
 * as stereo_ncc_unary evaluates it before the weighting) at pixel (y, x) and disparity sample_at[j]: the nearest
 * slice with ties to the larger index, the parabola through it and its two neighbours, the slice itself at the first
 * and the last one, -1e6 outside [min, max] of `disparities`.  Then
 *     out(yc, xc, j) = 0.25 * (((v00 + v10) + v01) + v11),  v_ik = v(min(2 yc + i, H - 1), min(2 xc + k, W - 1), j)
 * (i the row offset, k the column offset): stereo_pyramid_reduce's order and replication.  `out` has the input's
 * layout with the sizes Hc, Wc, Kc: layout 0 (yc, xc, j) at yc + Hc*(xc + Wc*j), layout 1 at j + Kc*(yc + Hc*xc).
 * fp64 without FMA contraction in the order written here: bit for bit the same lines in any language.
 * With sample_at = 2 * (the coarser level's slices), clipped to the finer range, a coarse pixel's value is the mean
 * over its fine pixels at the doubled disparity, so unary_weight * (1 - out) is the mean of their unaries: the level
 * model's unary half.
 *
 * Refused with a message, before the device is looked for: H, W, D or Kc below 1; H*W >= 2^31; Hc*Wc*Kc or H*W*D
 * >= 2^63 / 8; a layout other than 0 / 1; NULL for a required array; a value of `disparities` or `sample_at` that
 * is not finite; out == ncc. */
int stereo_pyramid_reduce_volume(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                 const double *sample_at, int Kc, double *out, char *err, size_t errcap);
/* The same on device arrays of the caller, launched on `stream` (hipStream_t, NULL = default) without waiting for
 * it.  The two short vectors are passed twice, as stereo_band_inputs_device takes its own: on the host
 * (`disparities`, `sample_at`: checked; min, max and the order of the slices are taken from them) and in device
 * memory (`d_disparities`, `d_sample_at`: the same values, which the kernels read). */
int stereo_pyramid_reduce_volume_device(const double *ncc, int H, int W, int D, int layout, const double *disparities,
                                        const double *d_disparities, const double *sample_at,
                                        const double *d_sample_at, int Kc, double *out, void *stream, char *err,
                                        size_t errcap);

/* ---- scanline aggregation: directional chain min-marginals --------------------------- *
 * No reference counterpart.  `unary` is D x N, label fastest (element (k, p) at k + D*p: layout 1, what TRW-S
 * consumes), N = H*W, pixel id p = y + H*x.  `positions`: D doubles, finite, in any order (repeats allowed).
 * kernel 1: v(d) = d, kernel 2: v(d) = d*d.  `directions`: R pairs (dy, dx), dy, dx in {-1, 0, 1}, not both 0,
 * 1 <= R <= 8, duplicates allowed; `weights`: one w_r >= 0 per direction.
 *     V_r[k, l] = w_r * min(v(|pos_k - pos_l|), tol)       (the product last, every operation rounded once)
 * For direction r the predecessor of pixel (y, x) is (y - dy, x - dx):
 *     L_r(p, k) = U(p, k)                                           where the predecessor is outside the image,
 *     L_r(p, k) = U(p, k) + min_l (L_r(p - r, l) + V_r[k, l])       otherwise.
 * The minimum over l is NOT subtracted: L_r(p, k) is the exact minimum energy, under the model's own pairwise term
 * w_r * min(v(|pos_a - pos_b|), tol), of the half chain that runs along direction r from the image border to p and
 * ends with x_p = k; L_r + L_-r - U is the min-marginal of the whole scanline.
 *     S = (((L_1 + L_2) + L_3) + ...)      in list order, D x N
 *     labels[p]     = the first minimum of S(p, .), ONE based
 *     map[p]        = positions[labels[p] - 1], H x W column major
 *     confidence[p] = the second-smallest entry of S(p, .) - min S(p, .): 0 where the minimum occurs twice, +Inf at
 *                     D = 1 (the rule of stereo_trws_plan_keep_min_marginals)
 * fp64 without FMA contraction.  Every candidate L + V is one add, U + min is one add, and a minimum of finite
 * doubles does not depend on the order it is taken in: for finite inputs the results are these lines' bits.
 *
 * Refused with a message, before the device is looked for: H or W below 1; H*W >= 2^31; D outside 1 ..
 * stereo_scanline_max_labels() (256); kernel other than 1 / 2; tol negative or NaN; R outside 1 .. 8; a direction
 * outside the set above; a weight that is negative or not finite; NULL for a required array; S == unary; and in
 * stereo_scanline_aggregate, whose arrays are on the host, a value of `unary` or `positions` that is not finite.
 * H = 1, W = 1 and D = 1 are valid.  S, map and confidence may be NULL there. */
int stereo_scanline_max_labels(void);
int stereo_scanline_aggregate(const double *unary, int H, int W, int D, const double *positions, int kernel, double tol,
                              const int32_t *directions, const double *weights, int R, double *S, int32_t *labels,
                              double *map, double *confidence, char *err, size_t errcap);
/* The same on device arrays of the caller (`unary`, `positions`, `S`, `labels`, `map`, `confidence`), launched on
 * `stream` (hipStream_t, NULL = default) without waiting for it: one launch per direction and one for the reduction.
 * `directions` and `weights` stay HOST arrays: they are the launches' parameters (at most 8 pairs and 8 doubles),
 * checked as above and not read after the call returns.  S is required: it is the workspace the directions add into,
 * and the output.  map and confidence may be NULL.  The inputs must be finite; for other values the call promises
 * only labels in 1 .. D and no access outside its arrays. */
int stereo_scanline_aggregate_device(const double *unary, int H, int W, int D, const double *positions, int kernel,
                                     double tol, const int32_t *directions, const double *weights, int R, double *S,
                                     int32_t *labels, double *map, double *confidence, void *stream, char *err,
                                     size_t errcap);

/* ---- scanline aggregation on per-edge positions ----------------------------------------- *
 * The same dynamic programme on the general model a TRW-S plan is bound to.  No reference counterpart.
 * Inputs: `unary` K x N, label fastest, N = H*W, pixel id p = y + H*x; `conn` 2 x E, zero based; `q` and `qprim`
 * K x E, label fastest; `alphas` E doubles, finite and >= 0; kernel 1: v(d) = d, kernel 2: v(d) = d*d; tol >= 0;
 * 1 <= K <= stereo_scanline_edges_max_labels() (64).
 * Edge cost, for e = (i1, i2) = (conn[2e], conn[2e+1]):
 *     c_e(x_i1, x_i2) = alphas_e * min(v(|qprim(x_i1, e) - q(x_i2, e)|), tol)   (the product last, every operation
 *                                                                                rounded once)
 * Graph: every edge joins two 4-neighbours of the H x W grid; a neighbour pair carries at most one edge in each
 * orientation (none, one or two edges); edges come in any order.  An edge that is a self-loop, out of range, not
 * between 4-neighbours (the last row of one column and the first of the next are no neighbours), or a second edge in
 * an occupied slot is refused.
 * Edge table: `table`, 4*N int32, two slots for each of two axes per pixel p.  Axis 0 is the pair (p - 1, p) in a
 * column, axis 1 the pair (p - H, p) in a row.  Slot 0 is the id of the edge oriented from the smaller pixel id to the
 * larger, slot 1 the reverse; -1 where the edge is absent or the neighbour lies outside the image.
 *     table[slot + 2*(axis + 2*p)]
 * Step table, for pixel p with label k and its predecessor p' with label l:
 *     T[k, l] = c_a(.) + c_b(.)        a, b the two slots of the pair, each with its arguments in its own orientation;
 *                                      an absent slot contributes +0.0 (two non-negative terms: any order)
 * Recurrence: `directions` are R pairs (dy, dx) out of (0, 1), (0, -1), (1, 0), (-1, 0), 1 <= R <= 8, duplicates
 * allowed; the model has no diagonal edges, so a diagonal is refused.  There are no per-direction weights: `alphas`
 * are the weights.  The predecessor of (y, x) is (y - dy, x - dx):
 *     L_r(p, k) = U(p, k)                                         where p' is outside the image,
 *     L_r(p, k) = U(p, k) + min_l (L_r(p', l) + T[k, l])          otherwise.
 * The minimum is not subtracted.  A pair without any edge has T = 0: the chain is not cut, L is still the half
 * chain's exact minimum energy.
 *     S = ((L_1 + L_2) + ...)    in list order, K x N
 *     labels[p]     = the first minimum of S(p, .), ONE based
 *     confidence[p] = the second-smallest entry of S(p, .) - min S(p, .): 0 at a tie, +Inf at K = 1
 * There is no map: positions are per edge, the caller applies the labels as a level does.
 * Every candidate L + T is one add, U + min is one add, T is one add of two products, a minimum of finite doubles is
 * order-free: for finite inputs S, labels and confidence are these lines' bits (fp64 without FMA contraction).
 *
 * Refused with a message, before the device is looked for: H or W below 1; H*W >= 2^31; K outside 1 .. 64; kernel
 * other than 1 / 2; tol negative or NaN; R outside 1 .. 8; a direction outside the four; E < 0 or E >= 2^31; NULL for
 * a required array (E = 0 allows NULL conn, q, qprim, alphas; every T is then 0 and S(p, .) is R * U(p, .) plus one
 * constant per pixel, the minima of the pixels before p along each direction); S == unary. */
int stereo_scanline_edges_max_labels(void);
/* The edge table of `conn` on the host, no device needed: `table` (4*H*W int32) is written.  The message names the
 * first offending edge. */
int stereo_scanline_edges_table(const uint32_t *conn, int64_t E, int H, int W, int32_t *table, char *err,
                                size_t errcap);
/* The same on device arrays, launched on `stream` without waiting for it: `table` is filled with -1, `bad` (one
 * int32) zeroed, then one thread per edge writes its slot; an invalid edge, or one whose slot is taken, adds one to
 * `bad` and writes nothing. */
int stereo_scanline_edges_table_device(const uint32_t *conn, int64_t E, int H, int W, int32_t *table, int32_t *bad,
                                       void *stream, char *err, size_t errcap);
/* On host arrays.  Builds the table itself (an invalid `conn` is refused with the table's message) and also refuses
 * a value of `unary`, `q` or `qprim` that is not finite and an alpha that is negative or not finite.  S and
 * confidence may be NULL. */
int stereo_scanline_edges_aggregate(int kernel, const double *unary, int H, int W, int K, int64_t E,
                                    const uint32_t *conn, const double *q, const double *qprim, const double *alphas,
                                    double tol, const int32_t *directions, int R, double *S, int32_t *labels,
                                    double *confidence, char *err, size_t errcap);
/* The same on device arrays of the caller with the table made before (stereo_scanline_edges_table_device, `bad` 0),
 * launched on `stream` without waiting for it: one launch per direction and one for the reduction.  `directions`
 * stays a HOST array.  S is required (the workspace the directions add into, and the output); confidence may be
 * NULL.  The inputs must be finite; for other values the call promises only labels in 1 .. K and no access outside
 * its arrays, as long as the table's entries are -1 or edge ids below E. */
int stereo_scanline_edges_aggregate_device(int kernel, const double *unary, int H, int W, int K, int64_t E,
                                           const int32_t *table, const double *q, const double *qprim,
                                           const double *alphas, double tol, const int32_t *directions, int R,
                                           double *S, int32_t *labels, double *confidence, void *stream, char *err,
                                           size_t errcap);
/* The N unary terms unary[labels_p - 1, p], then the E edge terms c_e(labels_i1, labels_i2) of a labelling, into
 * `terms` (N + E doubles on the device), each with the definition's operations; the level's model energy is their sum.
 * `bad` (one int32, zeroed on the stream first) counts labels outside 1 .. K; a term such a label, or an endpoint
 * outside 0 .. N-1, takes part in is written as 0.  Refused: N < 1 or N >= 2^31, K outside 1 .. 64, kernel, tol and
 * E as above, NULL for a required array (E = 0 allows NULL conn, q, qprim, alphas). */
int stereo_scanline_edges_energy_device(int kernel, const double *unary, int K, int64_t N, int64_t E,
                                        const uint32_t *conn, const double *q, const double *qprim,
                                        const double *alphas, double tol, const int32_t *labels, double *terms,
                                        int32_t *bad, void *stream, char *err, size_t errcap);

/* ---- image-guided smoothness: contrast weights and weighted scanlines ------------------ *
 * No reference counterpart.  An image is H x W x C doubles, column major, as stereo_pyramid_reduce takes it: element
 * (y, x, c) at y + H*(x + W*c), C >= 1, finite; N = H*W, pixel id p = y + H*x.
 * Contrast of two pixels a, b:
 *     g(a, b) = max_c |im(a, c) - im(b, c)|        (one subtraction per channel; the maximum of finite doubles does
 *                                                   not depend on its order: g is symmetric and bit-defined)
 * Ramp rho(g) with the parameters w_high >= 0, w_low >= 0, 0 <= g0 <= g1, all finite, tested in this order:
 *     g <= g0             ->  w_high
 *     otherwise g >= g1   ->  w_low
 *     otherwise           ->  w_high + (w_low - w_high) * ((g - g0) / (g1 - g0))
 * Every operation is rounded once, nothing is contracted, there is no exp: the same bits in any language (the
 * expression order of tests/contrast_restate.py is the definition).  g0 == g1 is a step, a two-level rule like
 * col_thresh; w_low > w_high is not refused.  rho is finite and >= 0.
 *
 * stereo_contrast_edge_weights: alphas[e] = rho(g(conn[2e], conn[2e+1])) for the E edges of `conn` (2 x E, zero
 * based), any graph on the image's pixels.  One thread per edge.  The host form refuses an endpoint outside
 * 0 .. N-1, naming the edge, and an image value that is not finite.  The device form takes `bad` (one int32 on the
 * device, zeroed on the stream first, as in stereo_scanline_edges_table_device): an edge with an endpoint outside
 * 0 .. N-1, or whose contrast is not finite, writes 0.0 and adds one to `bad`.
 *
 * stereo_contrast_step_weights: wstep, R x N doubles, element (r, p) at p + N*r, for the R directions (dy, dx) of
 * `directions` (a HOST array in both forms; the 8 of stereo_scanline_aggregate, 1 <= R <= 8), one launch for all R:
 *     wstep[r, p] = rho(g(p, p - r))     where the predecessor (y - dy, x - dx) is inside the image,
 *     wstep[r, p] = 0.0                  where it is not.
 * The host form refuses an image value that is not finite; in the device form the image must be finite.
 * For an axis direction wstep[r, p] is the alphas of the grid edge between p and its predecessor, in either
 * orientation: the aggregation below and a TRW-S plan uploaded with those alphas then speak about one energy.
 *
 * Refused with a message, before the device is looked for: H, W or C below 1; H*W >= 2^31; E < 0; NULL for a
 * required array (conn may be NULL at E = 0); a parameter that is negative or not finite, or g0 > g1; R outside
 * 1 .. 8 or a direction outside the 8; an output that is an input (alphas == im or conn, wstep == im). */
typedef struct stereo_contrast_params {
  double w_high, w_low, g0, g1;
} stereo_contrast_params;
int stereo_contrast_edge_weights(const double *im, int H, int W, int C, const uint32_t *conn, int64_t E,
                                 const stereo_contrast_params *params, double *alphas, char *err, size_t errcap);
int stereo_contrast_step_weights(const double *im, int H, int W, int C, const int32_t *directions, int R,
                                 const stereo_contrast_params *params, double *wstep, char *err, size_t errcap);
/* The same on device arrays of the caller (`im`, `conn`, `alphas`, `bad`, `wstep`), launched on `stream`
 * (hipStream_t, NULL = default) without waiting for it. */
int stereo_contrast_edge_weights_device(const double *im, int H, int W, int C, const uint32_t *conn, int64_t E,
                                        const stereo_contrast_params *params, double *alphas, int32_t *bad,
                                        void *stream, char *err, size_t errcap);
int stereo_contrast_step_weights_device(const double *im, int H, int W, int C, const int32_t *directions, int R,
                                        const stereo_contrast_params *params, double *wstep, void *stream, char *err,
                                        size_t errcap);

/* stereo_scanline_aggregate_weighted: stereo_scanline_aggregate with `step_weights` (R x N doubles, element (r, p) at
 * p + N*r, finite and >= 0) in the place of the one weight per direction.  Everything else is that entry's, with
 *     L_r(p, k) = U(p, k)                                                                    no predecessor,
 *     L_r(p, k) = U(p, k) + min_l (L_r(p - r, l) + wstep[r, p] * min(v(|pos_k - pos_l|), tol))     otherwise
 * (the product last, the minimum not subtracted): the step INTO p along direction r weighs wstep[r, p].  S, labels,
 * map and confidence are defined as there.  An entry of `step_weights` at a pixel without a predecessor is not read.
 * A step weight of exactly 0 is legal and gives L = U + min_l L(p - r, l).  With wstep[r, .] constant = w_r the
 * results are stereo_scanline_aggregate's bits.
 * Refused: stereo_scanline_aggregate's refusals (step_weights in the place of weights); S == step_weights; and in
 * the host form an entry of `step_weights` that is read and is negative or not finite.  The device form promises for
 * such values, as for other non-finite inputs, only labels in 1 .. D and no access outside its arrays. */
int stereo_scanline_aggregate_weighted(const double *unary, int H, int W, int D, const double *positions, int kernel,
                                       double tol, const int32_t *directions, const double *step_weights, int R,
                                       double *S, int32_t *labels, double *map, double *confidence, char *err,
                                       size_t errcap);
/* On device arrays of the caller (`step_weights` too; `directions` stays a HOST array), as
 * stereo_scanline_aggregate_device. */
int stereo_scanline_aggregate_weighted_device(const double *unary, int H, int W, int D, const double *positions,
                                              int kernel, double tol, const int32_t *directions,
                                              const double *step_weights, int R, double *S, int32_t *labels,
                                              double *map, double *confidence, void *stream, char *err,
                                              size_t errcap);

/* ---- map filter: image-guided weighted median of a disparity map ------------------------ *
 * No reference counterpart.  d: H x W doubles, column major, (y, x) at y + H*x, pixel id p = y + H*x, N = H*W < 2^31.
 * radius r, 1 <= r <= stereo_map_filter_max_radius() (4).  Optional: `im`, H x W x C finite doubles as in the section
 * above, with `params` (both or neither); `pixel_weight`, N doubles, finite and >= 0; `targets`, N int32, a pixel is
 * a target where its entry is not 0 (NULL: every pixel is).
 *
 * Taps of p = (y, x): the window positions (y + dy, x + dx), dx = -r .. r outer, dy = -r .. r inner: TAP ORDER.
 * A tap q is valid if it lies inside the image and d(q) is finite.  Its weight is
 *     w_q = rho(g(p, q)) * pixel_weight(q)            (g and rho as above; without im the first factor is 1.0 and not
 *                                                      multiplied, without pixel_weight there is no second factor;
 *                                                      with both ONE product, rounded once; the centre is a tap)
 * At a target p, with every sum formed by rounded additions in tap order, starting from 0.0:
 *     total   = sum of w_q over the valid taps
 *     W_le(v) = sum of (d(q) <= v ? w_q : 0.0) over the valid taps
 *     total > 0 false:  out(p) = d(p) (its bits), source(p) = p, and the pixel is counted in `kept`;
 *     otherwise:        v* = the smallest d(q) among the valid taps with 2 * W_le(d(q)) >= total,
 *                       source(p) = the id of the first tap in tap order that is valid, has w_q > 0 and d(q) == v*,
 *                       out(p) = d(source(p)) (that tap's bits: it says which zero where -0.0 == +0.0 tie).
 * Rounded addition is monotone, so W_le is monotone in v and the largest value qualifies (its sum is total's own): v* is
 * the lower weighted median; it is the value of a positive-weight tap (the sum rose at v*), and it does not depend on the
 * order in which candidates are examined.  At a pixel that is not a target out(p) = d(p), bit for bit whatever it is, and
 * source(p) = p.  `kept` (one int32) = the number of targets with total > 0 false.
 * A 4 x N plane map is filtered by taking, per pixel, the plane of source(p).
 *
 * One launch: a kernel per radius and per guided / weighted combination, one thread per pixel, a workgroup's tile of d
 * (and, a channel at a time, of im, then of pixel_weight) with its r-wide halo in LDS; (2r+1)^4 compare-select-add steps
 * per target.  `source` may be NULL in both forms.  The device form zeroes `kept` on the stream first; the image and
 * pixel_weight must there be finite (and >= 0): for other values it promises only no access outside its arrays.
 * Refused with a message, before the device is looked for: H or W below 1; H*W >= 2^31; a radius outside the range;
 * NULL d, out or kept; im without params or params without im; C < 1 with an image; the ramp's parameter rule above;
 * out, source or kept equal to an input or to each other; and in the host form an image value that is not finite or
 * a pixel weight that is negative or not finite, naming the first. */
int stereo_map_filter_max_radius(void);
int stereo_map_weighted_median(const double *d, int H, int W, int radius, const double *im, int C,
                               const stereo_contrast_params *params, const double *pixel_weight,
                               const int32_t *targets, double *out, int32_t *source, int32_t *kept, char *err,
                               size_t errcap);
/* The same on device arrays of the caller, launched on `stream` (hipStream_t, NULL = default) without waiting. */
int stereo_map_weighted_median_device(const double *d, int H, int W, int radius, const double *im, int C,
                                      const stereo_contrast_params *params, const double *pixel_weight,
                                      const int32_t *targets, double *out, int32_t *source, int32_t *kept,
                                      void *stream, char *err, size_t errcap);

/* ---- device-resident fusion moves --------------------------------------- *
 * The state of one dispmap object kept in HBM across moves: connectivity, weights, points,
 * the current assignment (dispmap_super.m properties :5-24), its unary and the unary source of
 * the subclass.  A binary fusion move (dispmap_super.m:61-84 binary_fusion followed by
 * :263-274 update_energy) then uploads only the proposal (4 x N) and returns four scalars:
 * pairwise terms, both unaries, QPBO (stereo_rd_plan), the scatter of the accepted planes and
 * the new energy all run on the device.  d_step != 0: dispmap_globalstereo rescaling. */
typedef struct stereo_fusion stereo_fusion;
int stereo_fusion_create(int H, int W, int kernel, double tol, int64_t E, const uint32_t *conn,
                         const double *weights, double d_min, double d_step, stereo_fusion **ctx,
                         char *err, size_t errcap);
void stereo_fusion_destroy(stereo_fusion *ctx);
/* unary source: dispmap_ncc.m:107-115 (ncc: H x W x D, MATLAB layout) ... */
int stereo_fusion_unary_ncc(stereo_fusion *ctx, const double *ncc, int D, const double *disparities,
                            double unary_weight, char *err, size_t errcap);
/* ... or dispmap_globalstereo.m:355-375 (images H x W x C, P2 4 x 3 as in stereo_globalstereo_unary) */
int stereo_fusion_unary_globalstereo(stereo_fusion *ctx, const double *im0, const double *im1, int C,
                                     const double *P2, double col_thresh, char *err, size_t errcap);
/* set.assignment + update_energy (dispmap_super.m:57-60, :263-274); energy may be NULL */
int stereo_fusion_set_assignment(stereo_fusion *ctx, const double *assignment, double *energy, char *err,
                                 size_t errcap);
/* current assignment (4 x N, may be NULL) and stored energy (may be NULL) */
int stereo_fusion_get_assignment(stereo_fusion *ctx, double *assignment, double *energy, char *err,
                                 size_t errcap);
/* one binary fusion move; energy = stored energy after the move, the other three are the outputs
 * of rd.m for this move (any may be NULL) */
int stereo_fusion_binary(stereo_fusion *ctx, const double *proposal, int improve, double *energy,
                         double *rd_energy, double *lower_bound, double *num_unlabelled, char *err,
                         size_t errcap);
/* Proposals built on the device.  The proposals of the reference's examples are one
 * plane for every pixel (example_ncc.m:24-41: plane fits and fronto-parallel planes, repmat'ed at
 * dispmap_ncc.m:65) or one plane per image segment (dispmap_globalstereo.m:154-192): `planes` is
 * 4 x S, `segments` N ids in [0, S) (may be NULL when S == 1, or to reuse the ids of the last call).
 * Same move as stereo_fusion_binary; 32 S bytes cross PCIe instead of 32 N. */
int stereo_fusion_binary_planes(stereo_fusion *ctx, const double *planes, int S, const int32_t *segments,
                                int improve, double *energy, double *rd_energy, double *lower_bound,
                                double *num_unlabelled, char *err, size_t errcap);
/* dispmap_ncc.m:48-92 generate_new_plane_RANSAC / fit_plane_to_points on the device: plane [a b 1 d]
 * through the winner-takes-all disparities (:208-221) within radius r of pixel (x, y) (one based,
 * x = column); kernel 1: 20 rounds of IRLS, kernel 2: total least squares.  The reference's
 * svd(...) V(:, end) is computed as the smallest eigenvector of the 3 x 3 normal matrix (MATLAB's svd
 * lies outside the reference tree: agreement to rounding, not bit for bit).  npoints (may be NULL):
 * pixels inside the radius. */
int stereo_fusion_fit_plane(stereo_fusion *ctx, double x, double y, double r, double *plane,
                            double *npoints, char *err, size_t errcap);
/* binary_fuse_until_convergence (dispmap_super.m:85-152) in one call on the resident state: n
 * proposals (either `proposals`, 4 x N x n column major, or `planes`, 4 x n single planes built on the
 * device; the other NULL), the 1-based revisit schedule `ids` exactly as the reference's loop indexes
 * it (ids(iter + 1) in trip iter; the caller concatenates 1:n with its random draws and applies the
 * reference's diff filter), at most `maxiter` trips.  n_energies = length(E), what the reference
 * returns; energies (cap entries, may be NULL) = E itself. */
int stereo_fusion_fuse_until_convergence(stereo_fusion *ctx, const double *proposals, const double *planes, int n,
                                         const int64_t *ids, int64_t n_ids, int64_t maxiter, int improve,
                                         double *n_energies, double *energies, int64_t cap, char *err, size_t errcap);
/* The same fit for n centres in ONE launch (xs, ys: 1-based pixel coordinates; planes: 4 x n column
 * major; npoints: n or NULL) -- the lattice `for x = 10:50:W, for y = 10:50:H` of example_ncc.m:24-32. */
int stereo_fusion_fit_planes(stereo_fusion *ctx, const double *xs, const double *ys, int n, double r,
                             double *planes, double *npoints, char *err, size_t errcap);
/* stereo_fusion_simultaneous with K single-plane proposals (planes 4 x K) built on the device */
int stereo_fusion_simultaneous_planes(stereo_fusion *ctx, const double *planes, int K, double maxiter,
                                      double max_relgap, double *energy, double *trws_energy,
                                      double *lower_bound, double *iterations, char *err, size_t errcap);
/* one simultaneous fusion (dispmap_super.m:153-198): the K proposals (4 x N x K) and the current
 * assignment (appended as label K+1, :160) compete per pixel; unary K x N, q / qprim K x E, TRW-S
 * (stereo_trws_plan, options maxiter / max_relgap as in trws.m) and the scatter of the winning
 * planes run on the device.  energy = stored energy afterwards; the other three are trws.m's. */
int stereo_fusion_simultaneous(stereo_fusion *ctx, const double *proposals, int K, double maxiter,
                               double max_relgap, double *energy, double *trws_energy,
                               double *lower_bound, double *iterations, char *err, size_t errcap);
/* Node beliefs of the simultaneous fusion's TRW-S run (stereo_trws_plan_keep_min_marginals; no reference
 * counterpart).  keep: applies to the plan the context creates for stereo_fusion_simultaneous / _planes from the
 * next call on.  Read after such a call: min_marginals (K+1) x N, confidence N, argmin N (0-based), any may be
 * NULL; rows in the label order TRW-S saw: the proposals in order, then the current assignment
 * (dispmap_super.m:158-160). */
int stereo_fusion_keep_min_marginals(stereo_fusion *ctx, int on, char *err, size_t errcap);
int stereo_fusion_trws_min_marginals(stereo_fusion *ctx, double *min_marginals, double *confidence,
                                     int32_t *argmin, char *err, size_t errcap);

/* ---- SegPln proposals (dispmap_globalstereo.m:60-201) -------------------------------------
 * The winner-takes-all disparity map by window matching (:72-113): for every image and every disparity of
 * `disps` (the class's self.disps: descending, :49) the reference image's pixels are projected, the image is
 * sampled bilinearly (vgg_interp2, oobv -1000), ephoto of the colour difference (:405) is averaged over the
 * (2 window + 1)^2 box ('valid') and summed over the images; normalised score, first maximum, disparities with
 * a score below min_corr (0.07, :112) set to 0, mirrored back to H x W.  images: n_images blocks of H x W x C
 * doubles (MATLAB layout), the first one the reference image; P: 3 x 4 x n_images column major (the argument
 * of the class constructor, :67).  wta: H x W column major. */
int stereo_segpln_wta(const double *images, int n_images, int H, int W, int C, const double *P, const double *disps,
                      int nd, double col_thresh, int window, double min_corr, double *wta, char *err, size_t errcap);
/* One proposal of segpln (:140-197) from a segmentation the CALLER supplies (labels 1 .. S, 0 = none; the
 * mean-shift / Felzenszwalb segmenters of :124-137 are out of scope): per segment the LO-RANSAC of :417-450
 * (threshold rt = 0.1 at :163, at most max_samples = 500 trials, confidence 0.95) over the world coordinates
 * [x y 1] / d, then the least-squares plane of the inliers; proposal (4 x N) = [N1 N2 1 N3] on the segment's
 * pixels, [0 0 1 0] where nothing was fitted, NaN / Inf -> 1e-100.  The reference draws its triples with
 * randperm; here trial t of segment s takes the three distinct indices splitmix64(seed, s, t, attempt) mod n
 * (oracle/terms.py:segpln_sample -- the draw is an input of the parity test), the 3 x 3 systems are solved by
 * Cramer's rule and the least-squares planes through the normal equations in a fixed summation order (MATLAB's
 * mldivide is outside the reference tree; oracle/terms.py:segpln_planes is the definition, matched bit for
 * bit).  planes (3 x S) / inliers (S) may be NULL; so may proposal when planes is given (the caller expands the planes
 * over the segments itself, or hands planes + segments to stereo_fusion_binary_planes). */
int stereo_segpln_planes(const double *wta, const int32_t *segments, int H, int W, double rt, uint64_t seed,
                         int max_samples, double *proposal, int S, double *planes, int32_t *inliers, char *err,
                         size_t errcap);

/* The same for M maps in one call (segpln fits fourteen, dispmap_globalstereo.m:122-197): segments[m], seeds[m], S[m],
 * proposals[m] (or NULL), planes[m] (or NULL), inliers[m] (or NULL) are map m's arguments of stereo_segpln_planes and
 * the results are those of M such calls, bit for bit -- the segments of all maps run side by side on the device (one
 * launch per workgroup size; pixels grouped and proposals delivered on helper threads), which is what the call is for. */
int stereo_segpln_planes_batch(const double *wta, const int32_t *const *segments, int M, int H, int W, double rt,
                               const uint64_t *seeds, int max_samples, double *const *proposals, const int *S,
                               double *const *planes, int32_t *const *inliers, char *err, size_t errcap);


/* ---- Image segmentation: what dispmap_globalstereo takes its edge weights (:391-403) and the maps of
 * its 14 SegPln proposals (:121-134) from.  A: H x W x 3 uint8, MATLAB column-major; out: H x W uint32, column-major.
 *
 * stereo_segment_ms = vgg_segment_ms(A, h_s, h_r, min_sz) (imrender/vgg/vgg_segment_ms.cxx:18-87 ->
 * msImageProcessor::Segment(sigmaS, sigmaR, minRegion, HIGH_SPEEDUP), seg_ms/msImageProcessor.cpp:703-808): mean-shift
 * filter in LUV (one thread per pixel on the device), then on the host connected components of the filtered image,
 * transitive closure of the region graph and pruning of regions below min_sz pixels; labels from 1 in the reference's
 * numbering.  The scalars are cast as the gateway casts them ((int) h_s, (float) h_r, (int) min_sz).  The optional
 * fifth gateway argument (a weight map, :55-68) has no caller in the reference and is not offered.  The reference reads
 * its speed-up threshold uninitialised (msImageProcessor.h:796); this entry point computes what the reference's own
 * build and the fixtures made with it compute: the upper half of a stack address taken for a float, 4.59e-41 -- in
 * effect "the colours are equal" (csrc/segment_host.h: kSpeedThreshold).
 *
 * stereo_segment_gb = vgg_segment_gb(A, sigma, k, min_sz, compress) (imrender/vgg/vgg_segment_gb.cxx:21-87 ->
 * seg_gb/segment-image.h:181-247): Gaussian smoothing and the weights of the 8-neighbourhood's edges on the device,
 * edges sorted by weight (std::sort, as in the reference: the order of equal weights is the library's), Kruskal with
 * the threshold k / size, components below min_sz joined; the labels are the union-find roots, or -- compress != 0 --
 * 1, 2, ... by first appearance in column-major order.  The library never writes its last row and column: they stay 0
 * (compressed: the label value 0 gets).
 *
 * The staged entry points are the same computation cut at the device / host boundaries: _ms_luv (host: RGB -> LUV,
 * L x 3 floats, pixel y * W + x); _ms_own (device: every pixel's own mode, same layout, and `events`, L bytes: 1 where
 * another pixel's colour came within the reference's speed-up threshold of the pixel's trajectory -- in flat regions);
 * _ms_finish (host: the pixels with events walked again in scan order with the reference's basin-of-attraction
 * bookkeeping, msImageProcessor.cpp:4015-4022,4085-4127,4256-4270 -> the reference's filtered image; *walked = how many);
 * _ms_filter = _ms_own + _ms_finish; _ms_regions (host: labels from a filtered image); _gb_weights (device: 4 floats per
 * pixel y * W + x: to (x+1,y), (x,y+1), (x+1,y+1), (x+1,y-1); 0 where the edge leaves the image), _gb_regions (host).
 * The host stages need no device. */
int stereo_segment_ms(const uint8_t *A, int H, int W, double h_s, double h_r, double min_sz, uint32_t *out, char *err,
                      size_t errcap);
int stereo_segment_gb(const uint8_t *A, int H, int W, double sigma, double k, double min_sz, int compress, uint32_t *out,
                      char *err, size_t errcap);
int stereo_segment_ms_luv(const uint8_t *A, int H, int W, float *luv, char *err, size_t errcap);
int stereo_segment_ms_own(const uint8_t *A, int H, int W, double h_s, double h_r, float *own, uint8_t *events, char *err,
                          size_t errcap);
int stereo_segment_ms_finish(const uint8_t *A, int H, int W, double h_s, double h_r, const float *own, const uint8_t *events,
                             float *filtered, int64_t *walked, char *err, size_t errcap);
int stereo_segment_ms_filter(const uint8_t *A, int H, int W, double h_s, double h_r, float *filtered, char *err,
                             size_t errcap);
int stereo_segment_ms_regions(const float *filtered, int H, int W, double h_r, double min_sz, uint32_t *out, char *err,
                              size_t errcap);
int stereo_segment_gb_weights(const uint8_t *A, int H, int W, double sigma, float *weights, char *err, size_t errcap);
int stereo_segment_gb_regions(const float *weights, int H, int W, double k, double min_sz, int compress, uint32_t *out,
                              char *err, size_t errcap);

#ifdef __cplusplus
}
#endif
#endif /* STEREO_HIP_H_ */
