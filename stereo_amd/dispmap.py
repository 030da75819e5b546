"""Host-side mirror of the reference's problem classes (dispmap_super.m,
dispmap_ncc.m, dispmap_globalstereo.m): same method names, argument meaning and
error behaviour, every array operation and both solvers running on the GPU through
the C ABI.  Planes are 4 x N arrays, images H x W x C doubles.

The proposal generators (local plane fits, segpln) and the two segmenters behind
dispmap_globalstereo (stereo_amd/segment.py) run through the same library; figures are
not mirrored.
"""
import numpy as np

from . import terms as T
from ._lib import StereoHipError
from .fusion import FusionContext, PlaneProposal
from .rd import RdPlan, rd  # noqa: F401
from .trws import trws


class dispmap_super:
    """dispmap_super.m.  Subclasses provide unary_cost()."""

    # True on the object dispmap_ncc.mirrored() returns: it is referenced on the second image and works,
    # internally, on the horizontally flipped pair; the maps that go in and out are in the un-flipped coordinates
    _mirrored = False

    def __init__(self, images, kernel):
        self.images = [np.asarray(im, dtype=np.float64) for im in images]
        self.sz = self.images[0].shape[:2]
        self.maxiter = 1000          # dispmap_super.m:9
        self.host_stack_budget_bytes = 8 << 30   # binary_fuse_until_convergence: largest 4 x N x n host array built for the native call
        self._max_relgap = 1e-4      # dispmap_super.m:10
        self._improve = False        # dispmap_super.m:13
        self._assignment = None
        self.stored_energy = np.inf
        self._kernel = kernel
        self.neighborhood = T.construct_neighborhood(*self.sz)          # zero based 2 x E
        self.points = T.get_points(*self.sz)
        self._smooth_weights = np.ones(self.neighborhood.shape[1])      # dispmap_super.m:35
        self.d_min, self.d_step = 0.0, 0.0                              # rescaling only in globalstereo
        self._rd_plan = None                                            # device-resident QPBO, built lazily
        self._ctx = None              # device-resident object state (stereo_fusion_*), built lazily
        self._ctx_has_assignment = False   # the context holds the current assignment
        self._host_stale = False           # ... and the host copy is older than the context's

    @property
    def smooth_weights(self):
        return self._smooth_weights

    @smooth_weights.setter
    def smooth_weights(self, w):
        self._smooth_weights = np.asarray(w, np.float64).reshape(-1)
        if getattr(self, "_ctx", None) is not None:
            self._invalidate_ctx()

    # ---- properties with the reference's setters (dispmap_super.m:39-56)
    @property
    def max_relgap(self):
        return self._max_relgap

    @max_relgap.setter
    def max_relgap(self, v):
        if v < 0:
            raise StereoHipError("Maximum relative gap must be non-negative")
        self._max_relgap = v

    @property
    def improve(self):
        return self._improve

    @improve.setter
    def improve(self, v):
        self._improve = bool(v)

    @property
    def assignment(self):
        if self._host_stale:          # moves ran on the device: fetch the planes on demand
            self._assignment, _ = self._ctx.get_assignment()
            self._host_stale = False
        return self._assignment

    @assignment.setter
    def assignment(self, a):
        self._assignment = np.asfortranarray(a, dtype=np.float64)
        self._host_stale = False
        self._ctx_has_assignment = False
        self.update_energy()

    # ---- device-resident state
    def _attach_unary(self, ctx):
        """Subclasses hand their unary source to the context; False = no device unary."""
        return False

    def _invalidate_ctx(self):
        """A parameter the context has baked in (tol, weights, kernel, unary source) changed."""
        if self._host_stale:
            self._assignment, _ = self._ctx.get_assignment()
            self._host_stale = False
        self._ctx = None
        self._ctx_has_assignment = False

    def _context(self):
        if self._ctx is None:
            ctx = FusionContext(self.sz[0], self.sz[1], self._kernel, self.tol, self.neighborhood,
                                self.smooth_weights, self.d_min, self.d_step)
            if not self._attach_unary(ctx):
                return None
            self._ctx = ctx
            self._ctx_has_assignment = False
        return self._ctx

    @property
    def smoothness_kernel(self):
        return self._kernel

    @smoothness_kernel.setter
    def smoothness_kernel(self, k):
        self._kernel = k
        self._invalidate_ctx()
        self.update_energy()

    def energy(self):
        return self.stored_energy

    # ---- terms
    def unary_cost(self, assignment):
        raise StereoHipError("Overload unary_cost")

    def disparitymap_from_assignment(self, assignment, points=None):
        pts = self.points if points is None else points
        if np.any(assignment[2] == 0):
            raise StereoHipError("Infinite disparity")
        d = -((assignment[0] * pts[0] + assignment[1] * pts[1]) + assignment[3]) / assignment[2]
        if self.d_step != 0:
            d = (d - self.d_min) / self.d_step
        return d

    def all_pairwise_costs(self, assignment, proposal=None):
        return T.pairwise_terms(self._kernel, self.neighborhood, self.points, assignment, proposal,
                                self.smooth_weights, self.tol, self.d_min, self.d_step)

    def update_energy(self):
        """dispmap_super.m:263-274"""
        if self._assignment is None or not hasattr(self, "tol"):
            self.stored_energy = np.inf
            return
        ctx = self._context()
        if ctx is not None:           # unary, E00 and both sums on the device
            self.stored_energy = ctx.set_assignment(self.assignment)
            self._ctx_has_assignment = True
            return
        U = self.unary_cost(self._assignment)
        P = self.all_pairwise_costs(self._assignment)
        self.stored_energy = float(np.sum(U) + np.sum(P))

    # ---- moves
    def binary_fusion(self, proposal):
        """dispmap_super.m:61-84.  `proposal`: 4 x N planes as in the reference, or a PlaneProposal
        (plane table, built into the 4 x N array on the device)."""
        if isinstance(proposal, PlaneProposal):
            ctx = self._context()
            if ctx is None:
                proposal = proposal.expand(self.sz[0] * self.sz[1])
            else:
                if not self._ctx_has_assignment:
                    ctx.set_assignment(self._assignment)
                    self._ctx_has_assignment = True
                self.stored_energy, e, lb, num_unlabelled = ctx.binary_planes(proposal, self._improve)
                self._host_stale = True
                return e, lb, num_unlabelled
        proposal = np.asfortranarray(proposal, dtype=np.float64)
        if proposal.shape != self._assignment.shape:
            raise StereoHipError("Binary fusion: Proposals is of wrong size")
        ctx = self._context()
        if ctx is not None:
            # device-resident move: only the proposal goes up, four scalars come back
            if not self._ctx_has_assignment:
                ctx.set_assignment(self._assignment)
                self._ctx_has_assignment = True
            self.stored_energy, e, lb, num_unlabelled = ctx.binary(proposal, self._improve)
            self._host_stale = True
            return e, lb, num_unlabelled
        E00, E01, E10, E11 = self.all_pairwise_costs(self._assignment, proposal)
        U0 = self.unary_cost(self._assignment)
        U1 = self.unary_cost(proposal)
        if self._rd_plan is None:      # same solver as rd(...), graph layout kept across moves
            self._rd_plan = RdPlan(self.sz[0] * self.sz[1], self.neighborhood, grid=self.sz)
        labelling, e, lb, num_unlabelled = self._rd_plan.solve(U0, U1, E00, E01, E10, E11, self._improve)
        a = self._assignment.copy(order="F")
        take = labelling == 1
        a[:, take] = proposal[:, take]
        self.assignment = a
        return e, lb, num_unlabelled

    def binary_fuse_until_convergence(self, proposal_cell, rng=None, device_loop=True):
        """dispmap_super.m:85-152, including its quirks (the loop variable is bumped inside the
        body, so ids(2) is fused first).  `rng` supplies the random revisit order (MATLAB's
        randi stream cannot be reproduced): a numpy Generator or an explicit id list.
        device_loop: run the schedule natively on the resident state (one call); False keeps the loop
        here, one binary_fusion call per move (the same moves, the same energies)."""
        if not isinstance(proposal_cell, (list, tuple)):
            raise StereoHipError("Input proposals should be given in cell array.")
        n = len(proposal_cell)
        number_of_random_ids = self.maxiter * 5
        if rng is None or isinstance(rng, np.random.Generator):
            rng = rng or np.random.default_rng()
            rand_ids = rng.integers(1, n + 1, number_of_random_ids)
        else:
            rand_ids = np.asarray(rng, dtype=np.int64)
        ids = np.concatenate([np.arange(1, n + 1), rand_ids])
        ids[:-1][np.diff(ids) == 0] = 0         # ids([diff(ids) == 0]) = 0 zeroes the FIRST of a repeated pair
        ids = ids[(ids >= 1) & (ids <= n)]
        # (a subclass with its own binary_fusion keeps the loop below, which calls it)
        native = device_loop and type(self).binary_fusion is dispmap_super.binary_fusion and hasattr(self, "tol")
        single = n > 0 and all(isinstance(p, PlaneProposal) and p.segments is None for p in proposal_cell)
        if native and not single and 32.0 * self.sz[0] * self.sz[1] * n > self.host_stack_budget_bytes:
            native = False   # the native call takes ONE contiguous 4 x N x n host array: beyond the budget keep the
                             # loop here, one proposal uploaded per move (the same moves, the same energies)
        ctx = self._context() if native else None
        if ctx is not None and n > 0:
            # the whole schedule in one native call on the resident state (stereo_fusion_fuse_until_convergence):
            # same loop, same exact energy comparisons, no interpreter and no PCIe traffic between moves
            N = self.sz[0] * self.sz[1]
            if not self._ctx_has_assignment:
                ctx.set_assignment(self._assignment)
                self._ctx_has_assignment = True
            props = None
            if not single:
                props = [p.expand(N) if isinstance(p, PlaneProposal) else np.asfortranarray(p, dtype=np.float64) for p in proposal_cell]
                for p in props:
                    if p.shape != (4, N):
                        raise StereoHipError("Binary fusion: Proposals is of wrong size")
            try:
                if single:
                    E = ctx.fuse_until_convergence(ids, self.maxiter, planes=np.concatenate([p.planes for p in proposal_cell], axis=1),
                                                   improve=self._improve)
                else:
                    E = ctx.fuse_until_convergence(ids, self.maxiter, proposals=props, improve=self._improve)
            except Exception:
                # a schedule that fails half way (a solver bound, out of memory) has already moved the RESIDENT
                # assignment and energy: the host copies are stale from here on, and the stored energy is whatever
                # the context holds now -- the object stays consistent with the device, then the error goes up
                self._host_stale = True
                try:
                    self.stored_energy = float(ctx.get_assignment()[1])
                except Exception:
                    self._ctx_has_assignment = False     # not even that: re-upload the host assignment before the next move
                    self._host_stale = False
                raise
            self.stored_energy = float(E[-1])
            self._host_stale = True
            self.fusion_energies = [float(e) for e in E]
            return len(E)
        E = [self.energy()]
        visited = np.zeros(n, dtype=bool)
        for it in range(1, self.maxiter + 1):
            if it > number_of_random_ids:
                ids = np.concatenate([ids, ids])
            it1 = it + 1                          # iter = iter + 1 inside the for body
            if it1 > len(ids):
                break
            pid = ids[it1 - 1]
            if visited[pid - 1]:
                continue
            self.binary_fusion(proposal_cell[pid - 1])
            E.append(self.energy())
            if E[-2] != E[-1]:
                visited[:] = False
            else:
                visited[pid - 1] = True
            if visited.all():
                break
        self.fusion_energies = [float(e) for e in E]
        return len(E)

    def simultaneous_fusion(self, proposal_cell, confidence=False):
        """dispmap_super.m:153-198.  confidence=True also sets self.min_marginals ((K+1) x N: the proposals in order,
        then the current assignment) and self.confidence (H x W, the reshape of current_dispmap) from the TRW-S run's
        node beliefs; the device-resident and the stateless path give the same values."""
        if not isinstance(proposal_cell, (list, tuple)):
            raise StereoHipError("Input proposals should be given in cell array.")
        ctx = self._context()
        N = self.sz[0] * self.sz[1]
        single = len(proposal_cell) > 0 and all(isinstance(p, PlaneProposal) and p.segments is None for p in proposal_cell)
        if not single:
            proposal_cell = [p.expand(N) if isinstance(p, PlaneProposal) else p for p in proposal_cell]
        for p in proposal_cell:
            if np.shape(p) != (4, N) and not isinstance(p, PlaneProposal):
                raise StereoHipError("Simultaneous fusion: Proposals is of wrong size")
        # (an empty cell: the reference appends the current assignment and runs trws with that one
        #  label, dispmap_super.m:158 -- the stateless path below does the same)
        if ctx is not None and len(proposal_cell) > 0:
            # device-resident: proposals go up, unary / positions / TRW-S / scatter stay in HBM
            if not self._ctx_has_assignment:
                ctx.set_assignment(self._assignment)
                self._ctx_has_assignment = True
            ctx.keep_min_marginals(confidence)
            if single:   # K planes instead of K x 4 x N doubles
                tab = np.concatenate([p.planes for p in proposal_cell], axis=1)
                self.stored_energy, e, lb, iterations = ctx.simultaneous_planes(tab, self.maxiter, self._max_relgap)
            else:
                self.stored_energy, e, lb, iterations = ctx.simultaneous(proposal_cell, self.maxiter, self._max_relgap)
            self._host_stale = True
            if confidence:
                mm, conf, _ = ctx.trws_min_marginals()
                self._set_confidence(mm, conf)
            return e, lb, iterations
        props = [np.asfortranarray(p, dtype=np.float64) for p in proposal_cell] + [self.assignment]
        unary = np.stack([self.unary_cost(p) for p in props], axis=0)             # K x N
        q, qprim = T.trws_positions(self.neighborhood, self.points, props, self.d_min, self.d_step)
        out = trws(np.int32(self._kernel), unary, self.neighborhood + 1, q, qprim, self.smooth_weights.reshape(-1),
                   self.tol, {"maxiter": self.maxiter, "max_relgap": self._max_relgap}, min_marginals=confidence)
        L, e, lb, iterations = out[:4]
        if confidence:
            self._set_confidence(out[4], out[5])
        a = np.zeros_like(props[0])
        for i, p in enumerate(props):
            a[:, L == i + 1] = p[:, L == i + 1]
        self.assignment = a
        return e, lb, iterations

    def _set_confidence(self, mm, conf):
        self.min_marginals = mm
        self.confidence = np.asarray(conf).reshape(self.sz[1], self.sz[0]).T

    def _unflip(self, m):
        """An H x W map between the object's internal columns and the image's own (the same operation both ways)."""
        return m[:, ::-1] if self._mirrored else m

    def current_dispmap(self):
        return self._unflip(self.disparitymap_from_assignment(self.assignment).reshape(self.sz[1], self.sz[0]).T)

    def set_disparity(self, disp):
        a = np.zeros((4, self.sz[0] * self.sz[1]))
        a[2] = 1
        a[3] = -self._unflip(np.asarray(disp, np.float64)).T.reshape(-1)   # column-major (:)
        self.assignment = a

    def cross_check(self, other, tol=1.0, fill=True):
        """Left-right consistency of this object's map against the other view's (no reference
        counterpart): stereo_lr_check of self.current_dispmap() against other.current_dispmap(), direction +1 unless
        self is a mirrored object, then stereo_lr_fill.  Sets and returns self.consistency (H x W int32: 0 consistent,
        1 occluded, 2 mismatch, 3 out of view, 4 not finite) and self.filled_dispmap (None without `fill`); the
        residuals and the fill's source columns are kept as self.consistency_residual / self.filled_source."""
        from . import consistency
        for obj in (self, other):
            if not getattr(obj, "_row_shift_views", False):
                raise StereoHipError("cross_check: %s reaches its second view through a projection, not a row shift; "
                                     "the left-right check is defined for dispmap_ncc" % type(obj).__name__)
        if tuple(self.sz) != tuple(other.sz):
            raise StereoHipError("cross_check: the two objects' sizes differ (%d x %d and %d x %d)" % (self.sz + other.sz))
        d = self.current_dispmap()
        self.consistency, self.consistency_residual = consistency.lr_check(d, other.current_dispmap(),
                                                                           -1 if self._mirrored else 1, tol)
        self.filled_dispmap, self.filled_source = consistency.lr_fill(d, self.consistency) if fill else (None, None)
        return self.consistency, self.filled_dispmap

    def filter_map(self, post_filter):
        """The map filter (no reference counterpart) on the map a preceding cross_check(fill=True) left:
        post_filter (a mapfilter.MedianFilter) on self.filled_dispmap with self.consistency and, where the filter has a
        contrast, the object's reference image -- for a mirrored object the flipped one it holds, un-flipped to the
        columns current_dispmap() and the filled map speak in.  Sets self.filtered_dispmap and self.filtered_source (pixel
        ids in those columns) and returns the map."""
        from . import mapfilter
        if not getattr(self, "_row_shift_views", False):
            raise StereoHipError("filter_map: %s reaches its second view through a projection, not a row shift; the "
                                 "left-right check it follows is defined for dispmap_ncc" % type(self).__name__)
        if not isinstance(post_filter, mapfilter.MedianFilter):
            raise StereoHipError("filter_map: a mapfilter.MedianFilter is needed (got %r)" % (post_filter,))
        if getattr(self, "filled_dispmap", None) is None:
            raise StereoHipError("filter_map: there is no filled map; call cross_check(other, fill=True) first")
        self.filtered_dispmap, self.filtered_source, _ = post_filter.apply(self.filled_dispmap, self.consistency,
                                                                           self._unflip(self.images[0]))
        return self.filtered_dispmap

    def refine_band(self, levels, maxiter=None, carry=False, solver="trws"):
        raise StereoHipError("refine_band: %s does not take its unary from the NCC sampler; band refinement is defined "
                             "for dispmap_ncc" % type(self).__name__)

    def refine_candidates(self, levels, maxiter=None, solver="trws"):
        raise StereoHipError("refine_candidates: %s does not take its unary from the NCC sampler; candidate bands are "
                             "defined for dispmap_ncc" % type(self).__name__)

    def solve_pyramid(self, levels, bands=None, maxiter=None, expand="guided", carry="none", unary="images", propagate=None):
        raise StereoHipError("solve_pyramid: %s reaches its second view through a projection, and its refinement is the "
                             "plane band; the image pyramid is defined for dispmap_ncc" % type(self).__name__)

    def solve_plane_pyramid(self, levels, bands=None, maxiter=None, expand="guided", carry="none", unary="images", propagate=None):
        raise StereoHipError("solve_plane_pyramid: %s reaches its second view through a projection; the plane pyramid is "
                             "defined for dispmap_ncc" % type(self).__name__)

    def _plane_band_source(self):
        """The hook of refine_plane_band: (the object's unary source, the factor from the units of `levels` to the
        planes' disparity units or None for 'as they are')."""
        raise StereoHipError("refine_plane_band: %s names no unary source" % type(self).__name__)

    def refine_plane_band(self, levels, maxiter=None, carry=False, solver="trws"):
        """Sub-pixel refinement that keeps each pixel's plane (no reference counterpart): for every
        vector of offsets in `levels` (strictly ascending, containing 0) TRW-S chooses per pixel among the pixel's own
        plane moved by an offset along the disparity axis, [a b c d - c offset], with this object's unary, kernel,
        tolerance, smoothness weights, rescaling and max_relgap, up to `maxiter` (default self.maxiter) iterations per
        level.  The levels are in the units of the object's smoothness term: disparities for dispmap_ncc, the rescaled
        units in which disp_thresh lives for dispmap_globalstereo.  carry=True: every level after the first starts from
        the previous level's messages.  solver="scanline": every level is one scanline aggregation on its
        inputs, not a TRW-S solve (no carry).  The result goes in through the assignment setter;
        returns plane_band.refine_plane_band's PlaneBandResult (planes in the object's internal columns)."""
        from . import plane_band
        levels = plane_band.check_levels(levels)
        source, unit = self._plane_band_source()
        if unit is not None:
            levels = [l * unit for l in levels]
        out = plane_band.refine_plane_band(source, self.assignment, self._kernel, self.tol, levels,
                                           self.maxiter if maxiter is None else maxiter, self._max_relgap,
                                           alphas=self.smooth_weights, conn=self.neighborhood, d_min=self.d_min,
                                           d_step=self.d_step, carry=carry, solver=solver)
        self.assignment = out.planes
        return out

    def _plane_candidate_level(self, level):
        """The hook of refine_plane_candidates: a level as the caller wrote it -> the level in the object's internal
        columns, with the source forms of the class resolved to 4 x N planes."""
        return level

    def refine_plane_candidates(self, levels, maxiter=None, solver="trws"):
        """Plane propagation around the current assignment (no reference counterpart): for every
        plane-candidate level in `levels` -- dict(offsets=, taps=, sources=), a source being 'base' (the current planes)
        or 4 x N planes -- TRW-S chooses per pixel among the pixel's own plane moved by an offset along the disparity
        axis and the sources' planes at the taps, copied unchanged (a neighbour's surface extended to this pixel), with
        this object's unary, kernel, tolerance, smoothness weights, rescaling and max_relgap, up to `maxiter` (default
        self.maxiter) iterations per level.  The offsets are in the units of refine_plane_band's levels.  4 x N sources
        are in the object's internal columns, as `assignment` is.  solver="scanline": every level is one scanline
        aggregation on its inputs.  The result goes in through the assignment setter;
        returns plane_candidates.refine_plane_candidates's PlaneBandResult (planes in the object's internal columns)."""
        from . import plane_candidates
        if isinstance(levels, dict):
            levels = [levels]
        levels = plane_candidates.check_levels([self._plane_candidate_level(l) for l in levels])
        source, unit = self._plane_band_source()
        if unit is not None:
            levels = [dict(l, offsets=l["offsets"] * unit) for l in levels]
        out = plane_candidates.refine_plane_candidates(source, self.assignment, self._kernel, self.tol, levels,
                                                       self.maxiter if maxiter is None else maxiter, self._max_relgap,
                                                       alphas=self.smooth_weights, conn=self.neighborhood, d_min=self.d_min,
                                                       d_step=self.d_step, solver=solver)
        self.assignment = out.planes
        return out


class dispmap_ncc(dispmap_super):
    """dispmap_ncc.m"""

    _row_shift_views = True    # the second view is the first one shifted along the rows: cross_check applies

    def __init__(self, images, disparities, kernel, unary_weight, tol):
        super().__init__(images, kernel)
        self.disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
        self._unary_weight = unary_weight
        self._tol = tol
        self.ncc = T.ncc_volume(self.images[0], self.images[1], self.disparities, 2)   # compute_ncc(self, 2)
        self.init_solution()

    @property
    def tol(self):
        return self._tol

    @tol.setter
    def tol(self, v):
        if v < 0:
            raise StereoHipError("Tolerance weight must be positive")
        self._tol = v
        self._invalidate_ctx()
        self.update_energy()

    @property
    def unary_weight(self):
        return self._unary_weight

    @unary_weight.setter
    def unary_weight(self, v):
        if v < 0:
            raise StereoHipError("Unary weight must be positive")
        self._unary_weight = v
        self._invalidate_ctx()
        self.update_energy()

    def unary_cost(self, assignment):
        return T.ncc_unary(self.ncc, self.disparities, self._unary_weight, assignment)

    def _attach_unary(self, ctx):
        ctx.unary_ncc(self.ncc, self.disparities, self._unary_weight)
        return True

    def _best_disp(self):
        return T.ncc_best_disp(self.ncc, self.disparities)      # internal columns

    def best_disp_from_ncc(self):
        return self._unflip(self._best_disp())

    def init_solution(self):
        self.set_disparity(self.best_disp_from_ncc())

    restart = init_solution

    def mirrored(self):
        """A new dispmap_ncc referenced on the SECOND image, with the same disparities, kernel, unary weight and
        tolerance (a definition, not a reference behaviour).  compute_ncc shifts one way only
        (dispmap_ncc.m:146-149 assumes d >= 0), so the right-referenced volume is the same volume function on the
        horizontally flipped images in swapped order, flipped back -- a mirrored conv2(..., 'same') window.  The object
        works on the flipped pair throughout (images, ncc, planes and proposals are in flipped columns);
        current_dispmap(), best_disp_from_ncc(), unary_volume() and set_disparity() speak in the un-flipped
        coordinates of the right image, where a pixel at column x with disparity d matches column x + d of the left."""
        m = dispmap_ncc([self.images[1][:, ::-1], self.images[0][:, ::-1]], self.disparities, self._kernel,
                        self._unary_weight, self._tol)
        m._mirrored = not self._mirrored      # (the mirror of a mirror is the first view again)
        return m

    def unary_volume(self):
        """H x W x D: unary_weight * (1 - ncc), the unary of every fronto-parallel label, in the image's own columns."""
        return self._unary_weight * (1.0 - (self.ncc[:, ::-1] if self._mirrored else self.ncc))

    def set_contrast(self, c):
        """Image-guided smoothness (no reference counterpart): smooth_weights become
        contrast.edge_weights(reference image, neighborhood, c) -- the object's own reference image, which for a mirrored
        object is the flipped one its neighborhood indexes.  Everything that reads smooth_weights follows; the pyramids
        refuse such an object as they refuse any smooth_weights other than 1."""
        from . import contrast
        self.smooth_weights = contrast.edge_weights(self.images[0], self.neighborhood, c)

    def aggregate_scanlines(self, directions=None, weights=None, contrast=None):
        """Scanline aggregation of this object's unary volume (no reference counterpart) with its
        disparities, kernel and tolerance: scanline.aggregate on unary_volume(), in the image's own columns (so is a
        direction's dx), along `directions` (default scanline.DIRECTIONS_8) with one weight per direction (default 1).
        contrast: a contrast.Contrast in the place of `weights` (both: refused) -- the weighted aggregation (DESIGN.md
        6.12) with the step weights of the reference image in its own columns.
        Nothing is stored in the object.  -> scanline.ScanlineResult with the summed volume (D x N)."""
        from . import scanline
        vol = self.unary_volume()
        H, W, D = vol.shape
        unary = np.asfortranarray(vol.transpose(2, 1, 0).reshape(D, W * H))
        directions = scanline.DIRECTIONS_8 if directions is None else directions
        if contrast is not None:
            from . import contrast as contrast_mod
            if weights is not None:
                raise StereoHipError("aggregate_scanlines: weights or contrast, not both")
            image = self.images[0][:, ::-1] if self._mirrored else self.images[0]
            wstep = contrast_mod.step_weights(image, directions, contrast)
            return scanline.aggregate_weighted(unary, (H, W), self.disparities, self._kernel, self._tol, wstep, directions,
                                               want_volume=True)
        return scanline.aggregate(unary, (H, W), self.disparities, self._kernel, self._tol, directions, weights,
                                  want_volume=True)

    def refine_band(self, levels, maxiter=None, carry=False, solver="trws"):
        """Sub-pixel refinement of the current map (no reference counterpart): for every vector of offsets in
        `levels` (strictly ascending, containing 0) TRW-S chooses per pixel among current disparity + offset, with this
        object's volume, unary weight, kernel, tolerance, smoothness weights and max_relgap, up to `maxiter` (default
        self.maxiter) iterations per level.  carry=True: every level after the first starts from the previous level's
        messages.  solver="scanline": every level is one scanline aggregation on its inputs, not a TRW-S
        solve (no carry).  The result goes in through set_disparity; returns band.refine_band's
        BandResult (its maps are in the object's internal columns: flipped for a mirrored object)."""
        from . import band
        base = self.disparitymap_from_assignment(self.assignment).reshape(self.sz[1], self.sz[0]).T    # internal columns
        out = band.refine_band(self.ncc, self.disparities, self._unary_weight, base, self._kernel, self._tol, levels,
                               self.maxiter if maxiter is None else maxiter, self._max_relgap, alphas=self.smooth_weights,
                               conn=self.neighborhood, carry=carry, solver=solver)
        self.set_disparity(self._unflip(out.dispmap))
        return out

    def refine_candidates(self, levels, maxiter=None, solver="trws"):
        """Propagation around the current map (no reference counterpart): for every candidate level in
        `levels` -- dict(offsets=, taps=, sources=), a source being 'base' (the current map), 'wta' (this volume's
        best_disp_from_ncc map) or an H x W map in the coordinates current_dispmap() speaks -- TRW-S chooses per pixel
        among current disparity + offset and the sources' values at the taps, with this object's volume, unary weight,
        kernel, tolerance, smoothness weights and max_relgap, up to `maxiter` (default self.maxiter) iterations per
        level.  solver="scanline": every level is one scanline aggregation on its inputs.
        The result goes in through set_disparity; returns candidates.refine_candidates's BandResult (its maps
        are in the object's internal columns: flipped for a mirrored object; the caller's maps and the taps' dx are
        in the image's own columns and are flipped on the way in)."""
        from . import candidates
        levels = candidates.check_levels(levels)
        if self._mirrored:        # maps of the caller are in un-flipped columns, the object works in flipped ones
            levels = [dict(l, sources=[s if isinstance(s, str) else np.asarray(s)[:, ::-1] for s in l["sources"]],
                           taps=l["taps"] * np.array([1, -1], np.int32)) for l in levels]
        base = self.disparitymap_from_assignment(self.assignment).reshape(self.sz[1], self.sz[0]).T    # internal columns
        out = candidates.refine_candidates(self.ncc, self.disparities, self._unary_weight, base, self._kernel, self._tol, levels,
                                           self.maxiter if maxiter is None else maxiter, self._max_relgap,
                                           alphas=self.smooth_weights, conn=self.neighborhood, solver=solver)
        self.set_disparity(self._unflip(out.dispmap))
        return out

    def solve_pyramid(self, levels, bands=None, maxiter=None, expand="guided", carry="none", unary="images", propagate=None):
        """The map from the image pyramid (no reference counterpart): this view solved at the scale
        2^levels with the level model of this object's kernel, unary weight and tolerance, carried up one scale at a time
        (`expand`: 'guided' by the reference image, or 'nearest') and refined at every finer level l by the band levels
        bands[l] (default one band, [-2 .. 2]); `maxiter` (default self.maxiter) is a scalar or one value per scale, level
        0 first; max_relgap is the object's.  A level's edges all weigh s^(k - 1): an object with other smooth_weights
        is refused.  A mirrored object works in its own flipped columns.  carry: 'none', 'levels' or 'scales'
        (pyramid.check_carry).  unary: 'images' (a level's volume is the NCC of the reduced images) or
        'blocks' (the block means of this object's own volume; nothing is recomputed).  propagate: per
        level 0 .. levels - 1 a list of candidate levels that run before the level's bands.  The result
        goes in through set_disparity;
        returns pyramid.solve_view_ncc_pyramid's ViewPyramidResult (maps in the object's internal columns)."""
        from . import pyramid
        unary = pyramid.check_unary(unary)
        if not np.all(self.smooth_weights == 1.0):
            raise StereoHipError("solve_pyramid: the level model gives every edge one weight; smooth_weights other than 1 "
                                 "do not carry to another scale")
        out = pyramid.solve_view_ncc_pyramid(self.images, self.disparities, self._kernel, self._unary_weight, self._tol,
                                             levels, self.maxiter if maxiter is None else maxiter, self._max_relgap,
                                             bands=bands, expand=expand, carry=carry, unary=unary,
                                             volume=self.ncc if unary == "blocks" else None, propagate=propagate)
        self.set_disparity(self._unflip(out.dispmap))
        return out

    def solve_plane_pyramid(self, levels, bands=None, maxiter=None, expand="guided", carry="none", unary="images", propagate=None):
        """The assignment from the plane pyramid (no reference counterpart): solve_pyramid's coarsest
        solve and level model, but what goes from scale to scale is a plane map (pyramid.expand_planes), and every finer
        level l runs the plane-candidate levels propagate[l] (sources 'base', plane_candidates.Fit(...), 'wta' and
        4 x N_l planes in the object's internal columns; None: no candidate pass) and then the plane bands bands[l], so
        a slant found or fitted at one scale survives to the next.  The arguments are solve_pyramid's, with carry 'none'
        or 'levels'; an object with smooth_weights other than 1 is refused as there.  A mirrored object works in its own
        flipped columns: the taps' dx are flipped on the way in.  The result goes in through the assignment setter;
        returns pyramid.solve_view_ncc_plane_pyramid's ViewPlanePyramidResult (planes in the object's internal columns)."""
        from . import pyramid
        from .candidates import _taps
        unary = pyramid.check_unary(unary)
        if not np.all(self.smooth_weights == 1.0):
            raise StereoHipError("solve_plane_pyramid: the level model gives every edge one weight; smooth_weights other "
                                 "than 1 do not carry to another scale")
        propagate = pyramid.check_plane_propagate(propagate, pyramid.check_plan(levels, 1, bands, expand)[0])
        if self._mirrored and propagate is not None:      # (checked above: lists of level dicts)
            propagate = [[dict(c, taps=_taps(c["taps"]) * np.array([1, -1], np.int32)) if "taps" in c else c for c in passes]
                         for passes in propagate]
        out = pyramid.solve_view_ncc_plane_pyramid(self.images, self.disparities, self._kernel, self._unary_weight, self._tol,
                                                   levels, self.maxiter if maxiter is None else maxiter, self._max_relgap,
                                                   bands=bands, expand=expand, carry=carry, unary=unary,
                                                   volume=self.ncc if unary == "blocks" else None, propagate=propagate)
        self.assignment = out.planes
        return out

    def _plane_band_source(self):
        from . import plane_band
        return plane_band.NccSource(self.ncc, self.disparities, self._unary_weight), None

    def _plane_candidate_level(self, level):
        """dispmap_ncc takes two more source forms: 'wta' -- the fronto-parallel planes of this volume's best_disp_from_ncc
        map; where that map is not finite the pixel's own plane stands in -- and an H x W map in the coordinates
        current_dispmap() speaks, taken as fronto-parallel planes.  A mirrored object flips such a map and the taps' dx on
        the way in; 4 x N sources are in the object's internal (flipped) columns, as `assignment` is, and pass unchanged."""
        from . import plane_candidates
        from .candidates import _taps
        if not isinstance(level, dict) or "sources" not in level:
            return level
        sources = level["sources"]
        if isinstance(sources, (str, np.ndarray, plane_candidates.OrOwn)):
            sources = [sources]
        N = self.sz[0] * self.sz[1]
        out = []
        for s in sources:
            if isinstance(s, str) and s == "wta":
                s = plane_candidates.OrOwn(plane_candidates.fronto(self._best_disp()))      # internal columns
            elif not isinstance(s, (str, plane_candidates.OrOwn)) and np.shape(s) == tuple(self.sz) and np.shape(s) != (4, N):
                s = plane_candidates.fronto(self._unflip(np.asarray(s, np.float64)))
            out.append(s)
        level = dict(level, sources=out)
        if self._mirrored and "taps" in level:
            level["taps"] = _taps(level["taps"]) * np.array([1, -1], np.int32)
        return level

    # ---- proposals (dispmap_ncc.m:48-92).  Host side: a few dozen points and 3 x 3 SVDs per
    # proposal; MATLAB's svd is outside the reference tree, so this mirrors the arithmetic with
    # numpy's (parity unpinned -- proposals are inputs of the parity-tested path, not outputs).
    def generate_new_plane_RANSAC(self, x, y, r, on_device=False):
        """dispmap_ncc.m:48-66: plane fitted to the winner-takes-all disparities within radius r
        of pixel (x, y) (1-based, x = column), repeated for every pixel.  on_device: the fit runs in
        the device-resident context (stereo_fusion_fit_plane) and a PlaneProposal comes back instead
        of the 4 x N array -- nothing of size N crosses PCIe for the proposal or the move."""
        if on_device:
            ctx = self._context()
            if ctx is not None:
                plane, _ = ctx.fit_plane(x, y, r)
                return PlaneProposal(plane)
        pts = self.points
        best = np.asarray(self._best_disp()).T.reshape(-1)      # column-major pixel order
        ids = np.sqrt((pts[0] - x) ** 2 + (pts[1] - y) ** 2) < r
        p = self.fit_plane_to_points(np.vstack([pts[:, ids], best[ids]]))
        return np.asfortranarray(np.repeat(p.reshape(4, 1), self.sz[0] * self.sz[1], axis=1))

    def generate_plane_lattice(self, radius=5, first=10, step=50, on_device=True):
        """The proposal lattice of example_ncc.m:24-32: `for x = first:step:W, for y = first:step:H`, one
        local plane fit (generate_new_plane_RANSAC) per point, in that order.  on_device: ALL fits in one
        launch (stereo_fusion_fit_planes), PlaneProposals come back; otherwise the host fits, 4 x N arrays."""
        xs = [x for x in range(first, self.sz[1] + 1, step) for _ in range(first, self.sz[0] + 1, step)]
        ys = [y for _ in range(first, self.sz[1] + 1, step) for y in range(first, self.sz[0] + 1, step)]
        if on_device:
            ctx = self._context()
            if ctx is not None and xs:
                planes, _ = ctx.fit_planes(xs, ys, radius)
                return [PlaneProposal(planes[:, i]) for i in range(planes.shape[1])]
        return [self.generate_new_plane_RANSAC(x, y, radius) for x, y in zip(xs, ys)]

    def fit_plane_to_points(self, points):
        """dispmap_ncc.m:67-92: total least squares (kernel 2) or 20 rounds of iteratively
        reweighted least squares (kernel 1) through the SVD of the centred points."""
        points = np.asarray(points, np.float64)
        c = points.mean(axis=1, keepdims=True)
        cost = -(points - c).T                                             # n x 3
        p = np.zeros(4)
        if self._kernel == 1:
            w = np.ones((cost.shape[0], 1))
            for _ in range(20):
                v = np.linalg.svd(w * cost, full_matrices=False)[2][-1]
                p[:3] = v
                w = np.sqrt(np.abs(cost @ v)).reshape(-1, 1)
        elif self._kernel == 2:
            p[:3] = np.linalg.svd(cost, full_matrices=False)[2][-1]
        p[3] = -(p[:3] @ points[:3].mean(axis=1))
        return p / p[2]


class dispmap_globalstereo(dispmap_super):
    """dispmap_globalstereo.m with the constants of ojw_default_options('cvpr08')
    (imrender/ojw/ojw_default_options.m:58-80) as defaults.  As in preprocess() (:377-403) the edge weights come
    from the mean-shift segmentation of the reference image, vgg_segment_ms(Rorig, seg_params) with seg_params =
    [4 5 0] (ojw_default_options.m:68; stereo_amd/segment.py); `segment` (H x W labels) or `smooth_weights`
    replace it for a caller who has them."""

    def __init__(self, images, P, disp_range, disparity_factor, options=None, segment=None,
                 smooth_weights=None, start_disparity=None, rng=None):
        opt = dict(smoothness_kernel=1, disp_thresh=0.02, col_thresh=30.0, lambda_l=9.0, lambda_h=108.0,
                   connect=4, improve=1, seg_params=(4, 5, 0))
        opt.update(options or {})
        super().__init__(images, opt["smoothness_kernel"])
        self.options = opt
        P = np.asarray(P, dtype=np.float64)
        if np.max(np.abs(P[:, :, 0].T.reshape(-1)[[0, 1, 2, 3, 4, 5, 8]] - np.array([1, 0, 0, 0, 1, 0, 1.0]))) > 1e-12:
            raise StereoHipError("First image must be reference image")
        self.P2 = np.asfortranarray(P[:, :, 1].T)          # self.P = permute(P, [2 1 3]); a = 2
        self._P = np.array(P[:, :, :len(self.images)], dtype=np.float64)   # the constructor's 3 x 4 x n (segpln projects with it, :67)
        # MATLAB colon lo*f : hi*f (dispmap_globalstereo.m:48): lo*f + (0 : floor(hi*f - lo*f)), also
        # for a fractional span (np.arange(lo*f, hi*f + 1) would append one element then)
        lo_f, hi_f = disp_range[0] * disparity_factor, disp_range[1] * disparity_factor
        disps = (lo_f + np.arange(np.floor(hi_f - lo_f + 1e-10) + 1))[::-1]
        self.disps = disps                                 # sorted descending (:49)
        self.d_min = float(disps[-1])
        self.d_step = float(disps[0] - self.d_min)
        self._tol = opt["disp_thresh"]
        self._improve = opt["improve"] > 0
        nin = len(self.images)
        if smooth_weights is None and segment is None:
            from . import segment as _segment                                         # :378-392
            sp = opt["seg_params"]
            segment = _segment.vgg_segment_ms(_segment.to_uint8(self.images[0]), sp[0], sp[1], sp[2])
        self.segment = None if segment is None else np.asarray(segment)
        if smooth_weights is not None:
            self.smooth_weights = np.asarray(smooth_weights, np.float64).reshape(-1)
        elif segment is not None:
            seg = np.asarray(segment).T.reshape(-1)
            same = seg[self.neighborhood[0]] == seg[self.neighborhood[1]]
            ew = same * opt["lambda_h"] + (~same) * opt["lambda_l"]                   # :400-402
            self.smooth_weights = ew * (nin / ((opt["connect"] == 8) + 1))            # :403
        if self._kernel == 2:                                                          # :410-413
            self.smooth_weights = self.smooth_weights / self._tol
            self._tol = self._tol ** 2
        H, W = self.sz
        if start_disparity is None:
            rng = rng or np.random.default_rng()
            start_disparity = rng.random((H, W)) * self.d_step + self.d_min          # :56
        self.start_disparity = np.asarray(start_disparity, np.float64)
        self.init_solution()

    @property
    def tol(self):
        return self._tol

    @tol.setter
    def tol(self, v):
        if v < 0:
            raise StereoHipError("Tolerance weight must be positive")
        self._tol = v
        self._invalidate_ctx()
        self.update_energy()

    def unary_cost(self, assignment):
        return T.globalstereo_unary(self.images[0], self.images[1], self.P2, self.d_min, self.d_step,
                                    self.options["col_thresh"], assignment)

    def _attach_unary(self, ctx):
        ctx.unary_globalstereo(self.images[0], self.images[1], self.P2, self.options["col_thresh"])
        return True

    def init_solution(self):
        self.set_disparity(self.start_disparity)

    def _plane_band_source(self):
        from . import plane_band
        return plane_band.GlobalstereoSource(self.images[0], self.images[1], self.P2, self.options["col_thresh"]), self.d_step

    # ---- proposals (dispmap_globalstereo.m:60-201)
    def segpln_wta(self):
        """The winner-takes-all disparity map of segpln (:72-113), computed on the device once per object."""
        if getattr(self, "_segpln_wta", None) is None:
            self._segpln_wta = T.segpln_wta(self.images, self._P, self.disps, col_thresh=self.options["col_thresh"],
                                            window=self.options.get("window", 2))
        return self._segpln_wta

    def segpln_segments(self):
        """The 14 segmentation maps of segpln (:116-134), H x W x 14, once per object."""
        if getattr(self, "_segpln_maps", None) is None:
            from . import segment as _segment
            self._segpln_maps = _segment.segpln_segments(self.images[0])
        return self._segpln_maps

    def segpln(self, segment_maps=None, seed=0):
        """dispmap_globalstereo.m:60-201: one piecewise-planar proposal (4 x N) per segmentation map -- 14 of them,
        on mean-shift / Felzenszwalb segmentations at the scales `mults` (:122-137; segpln_segments above), or on
        the maps the caller passes (H x W labels 1 .. S, 0 = no segment).  Window matching, LO-RANSAC and the
        plane fits run on the device (stereo_segpln_wta / stereo_segpln_planes); `seed` stands for MATLAB's
        random stream (map b uses seed + b)."""
        if segment_maps is None:
            maps = self.segpln_segments()
            segment_maps = [maps[:, :, b] for b in range(maps.shape[2])]
        wta = self.segpln_wta()
        return [out[0] for out in T.segpln_planes_batch(wta, list(segment_maps), [int(seed) + b for b in range(len(segment_maps))])]

    restart = init_solution
