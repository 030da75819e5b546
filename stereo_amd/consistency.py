"""Left-right consistency (no reference counterpart): the cross-check of two disparity
maps, the occlusion map it gives, the per-row fill, and ``solve_pair_ncc``, which solves both views of a
pair in one TRW-S batch and checks each map against the other.

Maps are H x W float64 arrays (any memory order on the host; the device forms take column-major
storage, element (y, x) at y + H*x).  ``direction`` +1: the map is referenced on the left image, a pixel
at column x with disparity d matches column x - d of the other view; -1: the right-referenced map.
Status values: 0 consistent, 1 occluded, 2 mismatch, 3 out of view, 4 not finite.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from . import terms as T
from ._lib import StereoHipError
from .trws import TrwsBatch, TrwsPlan

CONSISTENT, OCCLUDED, MISMATCH, OUT_OF_VIEW, NOT_FINITE = range(5)


def fill_chunks():
    """Column ranges (waves) the fill kernel splits a row into (stereo_lr_fill_chunks)."""
    return int(_lib.lib().stereo_lr_fill_chunks())


def _map(a, what, dtype=np.float64):
    a = np.asarray(a)
    if a.ndim != 2:
        raise StereoHipError("%s must be an H x W array" % what)
    return np.asfortranarray(a, dtype=dtype)


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def lr_check(d_ref, d_other, direction, tol, want_residual=True):
    """stereo_lr_check -> (status H x W int32, residual H x W float64 or None)."""
    d_ref, d_other = _map(d_ref, "d_ref"), _map(d_other, "d_other")
    if d_ref.shape != d_other.shape:
        raise StereoHipError("lr_check: the two maps must have the same size")
    H, W = d_ref.shape
    status = np.zeros((H, W), np.int32, order="F")
    residual = np.zeros((H, W), order="F") if want_residual else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_lr_check(_p(d_ref), _p(d_other), C.c_int(H), C.c_int(W), C.c_int(int(direction)),
                                    C.c_double(float(tol)), _p(status, C.c_int32), _p(residual), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return status, residual


def lr_fill(d_ref, status, want_source=True):
    """stereo_lr_fill -> (filled H x W float64, source H x W int32 or None)."""
    d_ref, status = _map(d_ref, "d_ref"), _map(status, "status", np.int32)
    if d_ref.shape != status.shape:
        raise StereoHipError("lr_fill: status must have the map's size")
    H, W = d_ref.shape
    filled = np.zeros((H, W), order="F")
    source = np.zeros((H, W), np.int32, order="F") if want_source else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_lr_fill(_p(d_ref), _p(status, C.c_int32), C.c_int(H), C.c_int(W), _p(filled),
                                   _p(source, C.c_int32), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return filled, source


def _device_map(t, what, dtype, shape=None):
    """A torch tensor that stores an H x W map column major: shape (W, H), contiguous, on the current device."""
    import torch
    want = torch.float64 if dtype is np.float64 else torch.int32
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != want or not t.is_cuda or not t.is_contiguous():
        raise StereoHipError("%s must be a contiguous (W, H) %s tensor on the device (column-major H x W)" % (what, want))
    if t.device.index != torch.cuda.current_device():
        raise StereoHipError("%s must be on the current device" % what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise StereoHipError("%s must have the map's size" % what)
    return t


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return int(getattr(stream, "cuda_stream", stream))


def lr_check_device(d_ref, d_other, direction, tol, status=None, residual=None, stream=None, want_residual=True):
    """stereo_lr_check_device on torch tensors of the current device.  A map is a contiguous (W, H) tensor: the
    column-major storage of H x W (``torch.from_numpy(m.T.copy())``, ``t.T`` on the way back).  Launched on `stream`
    (a torch stream or a raw handle; default: torch's current stream) without waiting for it.  `status` / `residual`:
    tensors to write into; made here otherwise.  -> (status, residual or None)."""
    import torch
    d_ref = _device_map(d_ref, "d_ref", np.float64)
    d_other = _device_map(d_other, "d_other", np.float64, d_ref.shape)
    W, H = d_ref.shape
    status = torch.empty((W, H), dtype=torch.int32, device=d_ref.device) if status is None else _device_map(status, "status", np.int32, d_ref.shape)
    if residual is None and want_residual:
        residual = torch.empty((W, H), dtype=torch.float64, device=d_ref.device)
    elif residual is not None:
        residual = _device_map(residual, "residual", np.float64, d_ref.shape)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_lr_check_device(vp(d_ref), vp(d_other), C.c_int(H), C.c_int(W), C.c_int(int(direction)),
                                           C.c_double(float(tol)), vp(status), vp(residual), C.c_void_p(_stream(stream)),
                                           err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return status, residual


def lr_fill_device(d_ref, status, filled=None, source=None, stream=None, want_source=True, chunks=None):
    """stereo_lr_fill_device on torch tensors, as lr_check_device takes them.  `chunks`: another number of column ranges
    than fill_chunks() (stereo_lr_fill_device_chunks; the results do not depend on it).  -> (filled, source or None)."""
    import torch
    d_ref = _device_map(d_ref, "d_ref", np.float64)
    status = _device_map(status, "status", np.int32, d_ref.shape)
    W, H = d_ref.shape
    filled = torch.empty((W, H), dtype=torch.float64, device=d_ref.device) if filled is None else _device_map(filled, "filled", np.float64, d_ref.shape)
    if source is None and want_source:
        source = torch.empty((W, H), dtype=torch.int32, device=d_ref.device)
    elif source is not None:
        source = _device_map(source, "source", np.int32, d_ref.shape)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    err = _lib.errbuf()
    L = _lib.lib()
    if chunks is None:
        rc = L.stereo_lr_fill_device(vp(d_ref), vp(status), C.c_int(H), C.c_int(W), vp(filled), vp(source),
                                     C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    else:
        rc = L.stereo_lr_fill_device_chunks(vp(d_ref), vp(status), C.c_int(H), C.c_int(W), vp(filled), vp(source),
                                            C.c_int(int(chunks)), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return filled, source


# ---------------------------------------------------------------- both views of a pair

def flip_volume(vol, H, W):
    """A D x (H*W) label-fastest volume with its columns x -> W - 1 - x."""
    D = vol.shape[0]
    return np.asfortranarray(vol.reshape((D, H, W), order="F")[:, :, ::-1].reshape((D, H * W), order="F"))


def pair_volumes(images, disparities):
    """The two D x N NCC volumes of a pair: the left-referenced one as dispmap_ncc builds it, the right-referenced one
    by the mirror: the same volume function on the horizontally flipped images in swapped order, flipped
    back."""
    im0, im1 = (np.asarray(im, dtype=np.float64) for im in images[:2])
    H, W = im0.shape[:2]
    left = T.ncc_volume(im0, im1, disparities, 2, layout=1)
    right = flip_volume(T.ncc_volume(im1[:, ::-1], im0[:, ::-1], disparities, 2, layout=1), H, W)
    return left, right


def pair_unaries(images, disparities, unary_weight, volumes=None):
    """The two D x N unary volumes unary_weight * (1 - ncc) of a pair, from pair_volumes."""
    left, right = pair_volumes(images, disparities) if volumes is None else volumes
    return unary_weight * (1.0 - left), unary_weight * (1.0 - right)


def occlusion_aware_unary(unary, status):
    """`unary` (D x N) with the columns of the occluded pixels (status 1) zeroed: the data term says nothing there."""
    u = np.array(unary, dtype=np.float64, order="F")
    u[:, np.asarray(status).T.reshape(-1) == OCCLUDED] = 0.0
    return u


class ViewResult:
    """One view of solve_pair_ncc: `labels` (N, one based), `dispmap`, `status`, `residual`, `filled`, `source`
    (H x W), and per pass `energy`, `lower_bound`, `iterations` (lists: the first solve, then the refine pass, then one
    entry per band level).  After band levels `labels` are the last level's band labels and `dispmap`, `status`,
    `residual`, `filled` and `source` those of the last level's refined map; `maps` keeps the map of every pass and
    `paths` the kernel family that ran it (TrwsPlan.path()).  A pyramid level that starts from an expanded map
     keeps that map and the expansion's candidate numbers as `expanded` and `expand_source`.  `carried`
    has one entry per pass: the pass started from the previous stage's messages.  With post_filter=
     `filtered` and `filter_source` are the filter's output on `filled` and its source pixel ids (H x W);
    None otherwise."""

    def __init__(self):
        self.labels = self.dispmap = self.status = self.residual = self.filled = self.source = None
        self.expanded = self.expand_source = None
        self.filtered = self.filter_source = None       # post_filter=: the filter on `filled`
        self.energy, self.lower_bound, self.iterations, self.maps, self.paths, self.carried = [], [], [], [], [], []


class PairResult:
    """solve_pair_ncc's result: `left` and `right` (ViewResult) and `times` (seconds per stage); with carry, `stages`:
    per view what the last pass leaves for a stage after it (carry.Stage, or None)."""

    def __init__(self):
        self.left, self.right = ViewResult(), ViewResult()
        self.times = {}
        self.stages = [None, None]

    @property
    def views(self):
        return self.left, self.right


def filter_views(out, post_filter, images):
    """post_filter (a mapfilter.MedianFilter, or None: nothing is done) on each view's `filled` map with the view's
    status and, where the filter has a contrast, the view's own image (`images`: the pair, left first) -> view.filtered,
    view.filter_source.  Nothing else of the view is touched: later stages start from the unfiltered maps."""
    if post_filter is None:
        return
    from . import mapfilter
    if not isinstance(post_filter, mapfilter.MedianFilter):
        raise StereoHipError("post_filter: a mapfilter.MedianFilter is needed (got %r)" % (post_filter,))
    if post_filter.contrast is not None and images is None:
        raise StereoHipError("post_filter: a filter with a contrast needs the pair's images")
    for i, view in enumerate(out.views):
        view.filtered, view.filter_source, _ = post_filter.apply(view.filled, view.status,
                                                                 None if images is None else images[i])


def collect_views(out, plans, to_map, check_tol, stage, post_filter=None, images=None):
    """One pass of a pair solve into `out` (PairResult): per view the plan's labels, energy, bound, iterations and
    kernel family, the map `to_map(view index, labels)`; then each map checked against the other and filled; with
    post_filter the filled maps filtered (filter_views; `images`: the pair, the guides)."""
    t = time.perf_counter()
    for i, (plan, view) in enumerate(zip(plans, out.views)):
        view.labels, en, lb, it = plan.result()
        view.energy.append(en); view.lower_bound.append(lb); view.iterations.append(it)
        view.paths.append(plan.path())
        view.dispmap = to_map(i, view.labels)
        view.maps.append(view.dispmap)
    for view, other, direction in ((out.left, out.right, 1), (out.right, out.left, -1)):
        view.status, view.residual = lr_check(view.dispmap, other.dispmap, direction, check_tol)
        view.filled, view.source = lr_fill(view.dispmap, view.status)
    filter_views(out, post_filter, images)
    out.times[stage] = time.perf_counter() - t


def run_band_levels(out, problems, band_levels, band_plans, kernel, conn, tol, maxiter, max_relgap, check_tol,
                    zero_occluded=False, carry=False, stages=None, scales=False, name="band", solver="trws", post_filter=None,
                    images=None):
    """The band passes of a pair solve: for every vector of offsets both views (`problems`: one band.BandProblem each,
    standing around the view's current map) build their band problem on the device and run up to `maxiter` iterations
    as a two-member TrwsBatch; the labels are applied, the refined maps checked with `check_tol` and filled
    (collect_views).  band_plans: {K: [plan, plan]}, filled here, closed by the caller.  zero_occluded: the unary
    columns of the pixels the preceding check found occluded are zeroed.
    The problems are driven by the protocol of band.run_levels (labels_of, build, leave, apply, carry_from), so they may
    as well be candidates.CandidateProblem: a level is then a candidate level, not a vector of offsets,
    carry must be off, and `name`, the prefix of the passes' entries in out.times, tells the two kinds apart.
    carry: every level after the first starts from the view's previous level's messages; the members
    take them as batch members take any state.  stages: per view the carry.Stage the FIRST level starts from (None:
    from zero) -- a solve on this grid, or with scales=True on the grid one box reduction coarser.  out.stages: per
    view the Stage of the last level (with carry).
    solver="scanline" (DESIGN.md 6.11): no plan is made and band_plans stays as it is; each view's level is aggregated in
    turn on the current stream (scanline.solve_level) and collected as a plan's result is: the labels' model energy,
    bound NaN, iterations 0, path 0.  carry and stages are refused.
    post_filter, images: passed to every level's collect_views."""
    import torch
    from . import band
    if band.check_solver(solver, carry, stages) == "scanline":
        from . import scanline
        for level, offsets in enumerate(band_levels):
            t0 = time.perf_counter()
            solved = []
            for prob, view in zip(problems, out.views):
                occluded = torch.from_numpy(view.status.T.reshape(-1) == OCCLUDED).cuda() if zero_occluded else None
                solved.append(scanline.solve_level(prob, offsets, kernel, tol, zero_columns=occluded))
                view.carried.append(False)
            out.times["%s_%d" % (name, level + 1)] = time.perf_counter() - t0
            collect_views(out, solved, lambda i, labels: problems[i].apply(labels), check_tol,
                          "%s_%d_check_fill" % (name, level + 1), post_filter, images)
        return
    N = problems[0].N
    previous = [prob.carry_from(st, scales) for prob, st in zip(problems, stages)] if stages is not None else [None, None]
    for level, offsets in enumerate(band_levels):
        t0 = time.perf_counter()
        Kb = problems[0].labels_of(offsets)
        if Kb not in band_plans:
            band_plans[Kb] = [TrwsPlan(int(kernel), Kb, N, conn) for _ in range(2)]
        for prob, plan, view, prev in zip(problems, band_plans[Kb], out.views, previous):
            occluded = torch.from_numpy(view.status.T.reshape(-1) == OCCLUDED).cuda() if zero_occluded else None
            prob.build(offsets, plan, tol, zero_columns=occluded, carry=prev)
            view.carried.append(prev is not None)
        with TrwsBatch(band_plans[Kb]) as batch:
            batch.iterate(maxiter, max_relgap)
        if carry:
            out.stages = [prob.leave(plan) for prob, plan in zip(problems, band_plans[Kb])]
        out.times["%s_%d" % (name, level + 1)] = time.perf_counter() - t0
        collect_views(out, band_plans[Kb], lambda i, labels: problems[i].apply(labels), check_tol,
                      "%s_%d_check_fill" % (name, level + 1), post_filter, images)
        previous = [prob.carry_from(st) for prob, st in zip(problems, out.stages)] if carry else [None, None]


def solve_pair_ncc(images, disparities, kernel, unary_weight, tol, maxiter, max_relgap, check_tol=1.0, refine_iters=0,
                   band_levels=None, smooth_weight=None, carry=False, volumes=None, contrast=None, post_filter=None):
    """Both views of a rectified pair: two NCC unary volumes, two TRW-S plans on the image grid with the shared
    positions `disparities`, iterated as one TrwsBatch; labels to maps; each map checked against the other and filled.
    refine_iters > 0: per view, the solver state is saved, the unary columns of the occluded pixels are zeroed and
    uploaded (which resets the plan), the state is loaded -- the warm start with other unaries of DESIGN.md 4.10 --
    and the batch runs refine_iters more iterations; then check and fill again.
    band_levels: a sequence of offset vectors.  After the passes above, for every level both views build
    the band problem around their map on the device, from their own volume, and run up to `maxiter` iterations as a
    two-member TrwsBatch; the refined maps are checked with check_tol and filled.  With refine_iters > 0 the unary
    columns of the pixels the preceding check found occluded are zeroed in the band as well.
    smooth_weight: the weight of every edge (default 1; DESIGN.md 6.4: a pyramid level's model).
    contrast: a contrast.Contrast in the place of smooth_weight -- giving both is refused.  Each view's
    edge weights are contrast.edge_weights of its own image on the image grid; the full-range plan, the occlusion-aware
    re-solve and the band levels of a view are uploaded with them.
    carry=True: the first band level starts from the full-range solve's messages (its disparities are the old offsets,
    the old base is zero), every later one from the level before it; the result's `stages` keeps what
    the last pass leaves.  The full-range passes themselves are what they are without it.
    volumes: the two D x N NCC volumes (left, right) to take in place of pair_volumes(images, disparities) -- a pyramid
    level's block volumes.
    post_filter: a mapfilter.MedianFilter.  After every check and fill of the solve, band levels
    included, each view's `filled` map is filtered, guided by the view's own image where the filter has a contrast,
    into `filtered` / `filter_source`.  Every other field, and what later passes start from, is what it is without."""
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    if len(images) != 2:
        raise StereoHipError("solve_pair_ncc: images must be the two views of a pair, left first (got %d)" % len(images))
    shapes = [np.shape(im) for im in images]
    if shapes[0] != shapes[1] or len(shapes[0]) != 3 or shapes[0][2] != 3:
        raise StereoHipError("solve_pair_ncc: the two images must be H x W x 3 arrays of one size (got %s and %s)" % tuple(shapes))
    if disparities.size < 1:
        raise StereoHipError("solve_pair_ncc: no disparities")
    H, W = shapes[0][:2]
    K, N = disparities.shape[0], H * W
    out = PairResult()
    clock = time.perf_counter
    t0 = clock()
    if band_levels is not None:
        from . import band
        band_levels = band.check_levels(band_levels)
    if volumes is None:
        volumes = pair_volumes(images, disparities)
    else:
        volumes = [np.asarray(v, dtype=np.float64) for v in volumes]
        if len(volumes) != 2 or any(v.shape != (K, N) for v in volumes):
            raise StereoHipError("solve_pair_ncc: volumes must be the two D x N volumes of the pair (%d x %d)" % (K, N))
    unaries = pair_unaries(images, disparities, unary_weight, volumes)
    out.times["volumes"] = clock() - t0
    conn = T.construct_neighborhood(H, W)
    if contrast is not None and smooth_weight is not None:
        raise StereoHipError("solve_pair_ncc: smooth_weight or contrast, not both")
    if contrast is None:
        alphas = [np.ones(conn.shape[1]) * (1.0 if smooth_weight is None else float(smooth_weight))] * 2     # per view
    else:
        from . import contrast as contrast_mod
        alphas = [contrast_mod.edge_weights(im, conn, contrast) for im in images]
    plans = [TrwsPlan(int(kernel), K, N, conn) for _ in range(2)]
    band_plans = {}
    by_index = lambda i, labels: disparities[labels.astype(np.int64) - 1].reshape(W, H).T

    try:
        t0 = clock()
        for plan, unary, a in zip(plans, unaries, alphas):
            plan.upload(unary, a, tol, positions=disparities)
        with TrwsBatch(plans) as batch:
            batch.iterate(maxiter, max_relgap)
        out.times["solve"] = clock() - t0
        collect_views(out, plans, by_index, check_tol, "check_fill", post_filter, images)
        for view in out.views:
            view.carried.append(False)
        if refine_iters > 0:
            t0 = clock()
            for plan, unary, view, a in zip(plans, unaries, out.views, alphas):
                state = plan.save_state()
                plan.upload(occlusion_aware_unary(unary, view.status), a, tol, positions=disparities)
                plan.load_state(state)
            with TrwsBatch(plans) as batch:   # a fresh batch: a member that max_relgap stopped takes part again
                batch.iterate(refine_iters, max_relgap)
            out.times["refine"] = clock() - t0
            collect_views(out, plans, by_index, check_tol, "refine_check_fill", post_filter, images)
            for view in out.views:
                view.carried.append(False)
        if carry:
            from . import carry as carry_mod
            out.stages = [carry_mod.full_range_stage(plan, disparities, conn, (H, W)) for plan in plans]
        if band_levels is not None:
            problems = [band.BandProblem(vol, disparities, unary_weight, view.dispmap, conn, a, layout=1)
                        for vol, view, a in zip(volumes, out.views, alphas)]
            run_band_levels(out, problems, band_levels, band_plans, kernel, conn, tol, maxiter, max_relgap, check_tol,
                            zero_occluded=refine_iters > 0, carry=carry, stages=out.stages if carry else None,
                            post_filter=post_filter, images=images)
    finally:
        for plan in plans + [p for pair in band_plans.values() for p in pair]:
            plan.close()
    return out
