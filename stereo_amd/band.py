"""Band refinement around a solved disparity map (the definition: include/stereo_hip.h).

From a map ``base`` (H x W) and a strictly ascending vector ``offsets`` that contains 0.0, the TRW-S problem whose
label k at pixel i means disparity ``base_i + offsets_k``: ``unary`` (K x N) from the NCC volume by the reference's
sampler, ``q`` / ``qprim`` (K x E) as stereo_trws_positions gives them for the planes ``[0 0 1 -(base + offsets_k)]``.
``refine_band`` builds these on the device, solves them level by level and applies the labels.

This module is also the one home of what the four level builders (band, plane_band, candidates, plane_candidates)
share: the host-array helpers, the helpers of the device wrappers (``_out`` ... ``_raise_bad``), the per-level result
lists (``LevelsResult``) and the level loop (``run_levels``) with the protocol a problem class offers it.

Host forms take NumPy arrays in MATLAB shapes (volume H x W x D for layout 0, D x N for layout 1; conn 2 x E zero
based).  Device forms take torch tensors of the current device: a map is a contiguous (W, H) tensor (the column-major
storage of H x W, as lr_check_device takes it), the volume, ``unary``, ``q`` and ``qprim`` are flat float64 tensors in
storage order, ``conn`` a flat int32 tensor of 2 E entries.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import carry as carry_mod
from . import terms as T
from ._lib import StereoHipError
from .consistency import _device_map, _map, _p, _stream
from .trws import TrwsPlan


def max_offsets():
    return int(_lib.lib().stereo_band_max_offsets())


def _vec(a, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 1:
        raise StereoHipError("%s must be a vector" % what)
    return np.ascontiguousarray(a)


def _volume(ncc, layout, H, W):
    """The volume in the storage order the C entry reads, and D."""
    ncc = np.asarray(ncc, dtype=np.float64)
    if layout == 0:
        if ncc.ndim == 2 and (H, W) == ncc.shape:
            ncc = ncc[:, :, None]
        if ncc.ndim != 3 or ncc.shape[:2] != (H, W):
            raise StereoHipError("band: a layout 0 volume must be H x W x D with the map's H and W")
        return np.asfortranarray(ncc), ncc.shape[2]
    if layout == 1:
        if ncc.ndim != 2 or ncc.shape[1] != H * W:
            raise StereoHipError("band: a layout 1 volume must be D x (H*W) with the map's H and W")
        return np.asfortranarray(ncc), ncc.shape[0]
    return np.asfortranarray(ncc), (ncc.shape[2] if ncc.ndim == 3 else ncc.shape[0])   # (the library refuses the layout)


def _conn(conn):
    c = np.asarray(conn)
    if c.ndim != 2 or c.shape[0] != 2:
        raise StereoHipError("connectivity must be 2 x E")
    return np.asfortranarray(c, dtype=np.uint32)


def band_inputs(ncc, disparities, unary_weight, base, offsets, conn, layout=0):
    """stereo_band_inputs -> (unary K x N, q K x E, qprim K x E), Fortran order."""
    base = _map(base, "base")
    H, W = base.shape
    vol, D = _volume(ncc, layout, H, W)
    disparities, offsets, conn = _vec(disparities, "disparities"), _vec(offsets, "offsets"), _conn(conn)
    if disparities.shape[0] != D:
        raise StereoHipError("band_inputs: %d disparities for a volume of %d slices" % (disparities.shape[0], D))
    K, E, N = offsets.shape[0], conn.shape[1], H * W
    unary = np.zeros((K, N), order="F")
    q, qprim = np.zeros((K, E), order="F"), np.zeros((K, E), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_inputs(_p(vol), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)), _p(disparities),
                                       C.c_double(float(unary_weight)), _p(base), _p(offsets), C.c_int(K), C.c_int64(E),
                                       _p(conn, C.c_uint32), _p(unary), _p(q), _p(qprim), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return unary, q, qprim


def _labels(labels, shape):
    lab = np.asarray(labels)
    if lab.ndim == 1 and lab.shape[0] == shape[0] * shape[1]:     # plan.result(): N values, column-major pixel order
        lab = lab.reshape(shape[1], shape[0]).T
    if lab.shape != tuple(shape):
        raise StereoHipError("band_apply: labels must be N values or an H x W array of the map's size")
    if not np.array_equal(lab, np.rint(lab)):
        raise StereoHipError("band_apply: labels must be whole numbers")
    return np.asfortranarray(lab, dtype=np.int32)


def band_apply(base, labels, offsets):
    """stereo_band_apply -> H x W: base + offsets[labels - 1].  `labels`: one based, N values as plan.result() returns
    them or H x W."""
    base = _map(base, "base")
    H, W = base.shape
    offsets = _vec(offsets, "offsets")
    lab = _labels(labels, (H, W))
    refined = np.zeros((H, W), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_apply(_p(base), C.c_int(H), C.c_int(W), _p(lab, C.c_int32), _p(offsets),
                                      C.c_int(offsets.shape[0]), _p(refined), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return refined


# ---------------------------------------------------------------- device forms

def _flat(t, what, dtype, n=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise StereoHipError("%s must be a contiguous %s tensor on the device" % (what, dtype))
    if t.device.index != torch.cuda.current_device():
        raise StereoHipError("%s must be on the current device" % what)
    if n is not None and t.numel() != n:
        raise StereoHipError("%s must hold %d elements (got %d)" % (what, n, t.numel()))
    return t


def to_device_vector(v):
    """A short host vector as a float64 tensor on the current device (what the device forms read as d_offsets)."""
    import torch
    return torch.from_numpy(np.array(v, dtype=np.float64)).cuda()


def _vp(t):
    """A tensor's address as the C entries take it: NULL for no tensor and for an empty one."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _out(t, what, n, dev, new=None):
    """An output of a device wrapper: `t` validated (n float64 elements), or a new tensor on `dev` (of shape `new`
    where that is not n)."""
    import torch
    return torch.empty(n if new is None else new, dtype=torch.float64, device=dev) if t is None else _flat(t, what, torch.float64, n)


def _bad(bad, dev):
    """The int32 counter a kernel adds its offending pixels to."""
    import torch
    return torch.zeros(1, dtype=torch.int32, device=dev) if bad is None else _flat(bad, "bad", torch.int32, 1)


def _edges(conn):
    """A flat int32 tensor of 2 E entries -> (conn, E)."""
    import torch
    conn = _flat(conn, "conn", torch.int32)
    if conn.numel() % 2:
        raise StereoHipError("conn must hold 2 E entries")
    return conn, conn.numel() // 2


def _device_vectors(stream, *vectors):
    """Short host vectors (float64 or int32) on the device.  Each of `vectors` is (host array, its device copy or None,
    the copy's name): a copy given is validated, one that is missing is made here.  If one was made and `stream` is
    given, torch's current stream is synchronized once: the copies ran on it, the kernels will not."""
    import torch
    made_here = any(d is None for _, d, _ in vectors)
    out = [torch.from_numpy(np.array(v).reshape(-1)).cuda() if d is None
           else _flat(d, what, torch.float64 if v.dtype == np.float64 else torch.int32, v.size) for v, d, what in vectors]
    if made_here and stream is not None:
        torch.cuda.current_stream().synchronize()
    return out


def _raise_bad(bad, check, message, *more):
    """check=True: reads the counter back (this waits for the stream) and raises `message % (count, *more)` if it is
    not zero."""
    if check:
        n = int(bad.item())
        if n:
            raise StereoHipError(message % ((n,) + more))


def _device_labels(labels):
    """plan.result()'s labels as the flat int32 tensor the apply entries read."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)).cuda()


def band_inputs_device(ncc, disparities, unary_weight, base, offsets, conn, layout=0, unary=None, q=None, qprim=None,
                       bad=None, stream=None, d_disparities=None, d_offsets=None, check=True):
    """stereo_band_inputs_device on torch tensors (module docstring), launched on `stream` (a torch stream or a raw
    handle; default: torch's current stream).  `disparities` and `offsets` are host vectors; `d_disparities` /
    `d_offsets`: their device copies, made here when not given.  check=True reads the count of pixels whose base is not
    finite back (this waits for the stream) and raises; check=False leaves it in `bad` and does not wait.
    -> (unary, q, qprim, bad): flat tensors K*N, K*E, K*E and the int32 counter."""
    import torch
    base = _device_map(base, "base", np.float64)
    W, H = base.shape
    disparities, offsets = _vec(disparities, "disparities"), _vec(offsets, "offsets")
    D, K, N = disparities.shape[0], offsets.shape[0], H * W
    ncc = _flat(ncc, "ncc", torch.float64, N * D)
    conn, E = _edges(conn)
    dev = base.device
    d_disparities, d_offsets = _device_vectors(stream, (disparities, d_disparities, "d_disparities"), (offsets, d_offsets, "d_offsets"))
    unary, q, qprim = _out(unary, "unary", K * N, dev), _out(q, "q", K * E, dev), _out(qprim, "qprim", K * E, dev)
    bad = _bad(bad, dev)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_inputs_device(_vp(ncc), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)), _p(disparities),
                                              _vp(d_disparities), C.c_double(float(unary_weight)), _vp(base), _p(offsets),
                                              _vp(d_offsets), C.c_int(K), C.c_int64(E), _vp(conn), _vp(unary), _vp(q), _vp(qprim),
                                              _vp(bad), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "band_inputs_device: base is not finite at %d pixel(s)")
    return unary, q, qprim, bad


def band_apply_device(base, labels, offsets, refined=None, bad=None, stream=None, d_offsets=None, check=True):
    """stereo_band_apply_device: `base` a (W, H) float64 map tensor, `labels` a (W, H) or flat int32 tensor, one based.
    check=True reads the count of labels outside 1 .. K back and raises.  -> (refined (W, H), bad)."""
    import torch
    base = _device_map(base, "base", np.float64)
    W, H = base.shape
    offsets = _vec(offsets, "offsets")
    K = offsets.shape[0]
    labels = _flat(labels, "labels", torch.int32, H * W)
    d_offsets, = _device_vectors(stream, (offsets, d_offsets, "d_offsets"))
    refined = torch.empty((W, H), dtype=torch.float64, device=base.device) if refined is None else _device_map(refined, "refined", np.float64, base.shape)
    bad = _bad(bad, base.device)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_apply_device(_vp(base), C.c_int(H), C.c_int(W), _vp(labels), _p(offsets), _vp(d_offsets),
                                             C.c_int(K), _vp(refined), _vp(bad), C.c_void_p(_stream(stream)), err,
                                             C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "band_apply_device: %d label(s) outside 1 .. %d", K)
    return refined, bad


# ---------------------------------------------------------------- levels

def check_levels(levels):
    """`levels` as a list of float64 vectors; at least one."""
    levels = [_vec(l, "a level's offsets") for l in levels]
    if not levels:
        raise StereoHipError("refine_band: levels must hold at least one vector of offsets")
    return levels


class LevelsResult:
    """What every refine_* keeps per level: `maps` (what apply() returned), `energy`, `lower_bound`, `iterations`,
    `labels` (N, one based), `paths` (the kernel family that ran, TrwsPlan.path()) and `carried` (the level started from
    the previous level's messages)."""

    def __init__(self):
        self.maps, self.labels = [], []
        self.energy, self.lower_bound, self.iterations, self.paths, self.carried = [], [], [], [], []


class BandResult(LevelsResult):
    """refine_band's result: LevelsResult's lists, `dispmap` (H x W, the last level's refined map) and `stage` (with
    carry: the carry.Stage the last level leaves)."""

    def __init__(self):
        super().__init__()
        self.dispmap = self.stage = None


SOLVERS = ("trws", "scanline")


def check_solver(solver, carry=False, start=None):
    """`solver` of a level loop: "trws", or "scanline" (DESIGN.md 6.11), which has no messages to carry."""
    if solver not in SOLVERS:
        raise StereoHipError("solver must be 'trws' or 'scanline' (got %r)" % (solver,))
    if solver == "scanline" and (carry or start is not None):
        raise StereoHipError("solver='scanline' has no messages to carry: carry and a carried start need solver='trws'")
    return solver


def run_levels(prob, levels, out, kernel, tol, maxiter, max_relgap, carry=False, start=None, solver="trws"):
    """The level loop of refine_band, refine_plane_band, refine_candidates and refine_plane_candidates.  For each of the
    checked `levels`: a TrwsPlan(kernel, K, N, conn) -- one per distinct K, made here and closed here -- is bound to the
    level's inputs, iterated up to `maxiter` times (`max_relgap` as in trws) and read, `out`'s (LevelsResult) lists
    grow by one entry, and the labels are applied.  carry=True: a level starts from what the one before it left;
    start: the carry.Carry the first level starts from.  -> what the last level left (None without carry).

    The protocol of `prob` (BandProblem, PlaneBandProblem and the two candidate problems derived from them):
    N, conn; labels_of(level) -> K, before the level is built; build(level, plan, tol, carry=) binds the level's inputs
    to `plan`, which starts from the carry.Carry `carry` if that is not None; leave(plan, labels) -> what the solved
    level leaves for the next one, taken before apply() (a plan is reused for equal K and the next bind wipes it);
    apply(labels) moves the problem on and returns the new map for the host; carry_from(left) -> the Carry into the
    next build from what leave() gave, taken after apply() (None for None).

    solver="scanline" (DESIGN.md 6.11): no TrwsPlan is made.  build(level, None, tol) leaves the level's inputs bound
    to nothing and the level is one scanline aggregation over the four axis directions on them (scanline.solve_level:
    K <= 64, `prob.conn` a grid's, its edge table built once and kept on the problem).  out.energy gets the labels'
    model energy, lower_bound NaN, iterations 0, paths 0 and carried False; carry and start are refused."""
    if check_solver(solver, carry, start) == "scanline":
        from . import scanline
        for level in levels:
            labels, en, lb, it = scanline.solve_level(prob, level, kernel, tol).result()
            out.carried.append(False); out.paths.append(0)
            out.labels.append(labels); out.energy.append(en); out.lower_bound.append(lb); out.iterations.append(it)
            out.maps.append(prob.apply(labels))
        return None
    plans, previous, left = {}, start, None
    try:
        for level in levels:
            K = prob.labels_of(level)
            if K not in plans:
                plans[K] = TrwsPlan(int(kernel), K, prob.N, prob.conn)
            plan = plans[K]
            prob.build(level, plan, tol, carry=previous)
            out.carried.append(previous is not None)
            plan.iterate(maxiter, max_relgap)
            labels, en, lb, it = plan.result()
            out.paths.append(plan.path())
            out.labels.append(labels); out.energy.append(en); out.lower_bound.append(lb); out.iterations.append(it)
            left = prob.leave(plan, labels) if carry else None
            out.maps.append(prob.apply(labels))
            previous = prob.carry_from(left)
    finally:
        for plan in plans.values():
            plan.close()
    return left


def bind_inputs(prob, plan, tol):
    """The inputs a build() has just made (prob.d_unary, d_q, d_qprim; torch's current stream has to finish them first)
    bound to `plan` with the problem's smoothness weights.  plan None: the inputs stay as they are, bound to nothing
    (a level that another solver takes from the problem's tensors)."""
    import torch
    if plan is None:
        return
    torch.cuda.current_stream().synchronize()
    plan.bind_device(prob.d_unary.data_ptr(), prob.d_alphas.data_ptr(), tol, d_q=prob.d_q.data_ptr(),
                     d_qprim=prob.d_qprim.data_ptr(), keepalive=[prob.d_unary, prob.d_q, prob.d_qprim, prob.d_alphas])


class BandProblem:
    """One view's band problems on the device: the volume, the connectivity and the smoothness weights go up once;
    build() makes a level's inputs from the current base and binds them to `plan`, apply() moves the base on.  (The
    protocol the level loops drive it by: run_levels.)"""

    def __init__(self, ncc, disparities, unary_weight, base, conn, alphas=None, layout=0):
        import torch
        _lib.require_device()
        base = _map(base, "base")
        self.H, self.W = base.shape
        vol, D = _volume(ncc, layout, self.H, self.W)
        self.disparities = _vec(disparities, "disparities")
        if self.disparities.shape[0] != D:
            raise StereoHipError("refine_band: %d disparities for a volume of %d slices" % (self.disparities.shape[0], D))
        self.layout, self.unary_weight = int(layout), float(unary_weight)
        self.conn = _conn(conn)
        self.N, self.E = self.H * self.W, self.conn.shape[1]
        alphas = np.ones(self.E) if alphas is None else np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).reshape(-1))
        if alphas.shape[0] != self.E:
            raise StereoHipError("refine_band: alphas must hold one weight per edge")
        self.d_ncc = torch.from_numpy(vol.reshape(-1, order="F")).cuda()
        self.d_disparities = to_device_vector(self.disparities)
        self.d_conn = torch.from_numpy(self.conn.reshape(-1, order="F").view(np.int32)).cuda()
        self.d_alphas = torch.from_numpy(alphas).cuda()
        self.d_base = torch.from_numpy(np.ascontiguousarray(base.T)).cuda()
        self.offsets = self.d_offsets = self.d_unary = self.d_q = self.d_qprim = None
        self.d_receiver = self.h_receiver = self.d_built_base = None

    def receiver(self):
        """The receiving node of every edge's message row in a plan at rest (phase 1), on the device: what the transfer
        of carried messages indexes `shift` with.  Worked out once (plans of this problem use the default node order)."""
        import torch
        if self.d_receiver is None:
            self.d_receiver = torch.from_numpy(self.receiver_host()).cuda()
        return self.d_receiver

    def receiver_host(self):
        if self.h_receiver is None:
            self.h_receiver = carry_mod.receivers(self.N, self.conn, 1)
        return self.h_receiver

    @staticmethod
    def labels_of(level):
        """K of the level `level` (here: a vector of offsets), before it is built."""
        return level.shape[0]

    def build(self, offsets, plan=None, tol=0.0, zero_columns=None, carry=None):
        """The inputs of the level `offsets` around the current base, bound to `plan` (None: to nothing).  zero_columns: a bool tensor (N,),
        pixels whose unary column is set to zero.  carry: a carry.Carry of the previous stage (whose messages were saved
        BEFORE this call: a plan is reused for equal K and the bind wipes it); the plan then starts from the transferred
        messages as a state of phase 1 with 0 iterations, not from zero."""
        self.offsets = _vec(offsets, "offsets")
        self.d_offsets = to_device_vector(self.offsets)
        self.d_built_base = self.d_base
        self.d_unary, self.d_q, self.d_qprim, _ = band_inputs_device(
            self.d_ncc, self.disparities, self.unary_weight, self.d_base, self.offsets, self.d_conn, self.layout,
            d_disparities=self.d_disparities, d_offsets=self.d_offsets)
        if zero_columns is not None:
            self.d_unary.view(self.N, -1)[zero_columns] = 0.0
        bind_inputs(self, plan, tol)
        if carry is not None:
            carry_mod.load_carried(plan, carry, self.offsets, self.receiver(), self.N, self.d_offsets)

    def stage(self, plan):
        """What the level built last leaves for the stage after it (carry.Stage): `plan`'s messages, saved on the device
        now (the next build may bind the same plan, which wipes it), the level's offsets and the base they were measured
        from.  To be called before or after apply().  None where the plan's state cannot be carried."""
        d_m = carry_mod.save_messages(plan, self.N)
        if d_m is None:
            return None
        return carry_mod.Stage(d_m, self.offsets, self.d_built_base.reshape(-1), self.conn, self.receiver_host(), (self.H, self.W))

    def leave(self, plan, labels=None):
        """What the solved level leaves for the next one: its stage()."""
        return self.stage(plan)

    def carry_from(self, stage, scales=False):
        """The carry.Carry from `stage` into the next level around the current base (None without a stage).  The shift
        is taken on the device from the two bases, so a base filled or otherwise edited in between is handled as well.
        scales=True: the stage is the scale above (one box reduction coarser)."""
        return carry_mod.carry_between(stage, self.d_base.reshape(-1), self.conn, self.receiver_host(), (self.H, self.W), scales)

    def apply(self, labels):
        """The base moved by the labels of the level built last -> the new base on the host, H x W."""
        self.d_base, _ = band_apply_device(self.d_base, _device_labels(labels), self.offsets, d_offsets=self.d_offsets)
        return self.d_base.cpu().numpy().T


def refine_band(ncc, disparities, unary_weight, base, kernel, tol, levels, maxiter, max_relgap, alphas=None, layout=0,
                conn=None, carry=False, carry_start=None, solver="trws"):
    """Refines the map `base` level by level: for each vector of offsets in `levels` the band problem around the current
    map is built on the device (stereo_band_inputs_device), bound to a TrwsPlan(kernel, K, N, conn) -- one plan per
    distinct K -- iterated up to `maxiter` times (`max_relgap` as in trws) and applied (stereo_band_apply_device); the
    refined map is the next level's base.  The volume goes to the device once; nothing K x N or K x E touches the host.
    conn: 2 x E zero based, default the image grid (construct_neighborhood).  carry=True: every level after the first
    starts from the previous level's messages, moved onto its own offsets, not from zero; the last
    level's carry.Stage is then kept as the result's `stage`.  carry_start: (a carry.Stage, scales) the first level
    starts from -- a solve on this grid, or with scales=True on the grid one box reduction coarser.  solver: "trws", or
    "scanline" -- every level one scanline aggregation on its inputs (run_levels; no carry).  -> BandResult."""
    check_solver(solver, carry, carry_start)
    levels = check_levels(levels)
    base = _map(base, "base")
    H, W = base.shape
    conn = T.construct_neighborhood(H, W) if conn is None else conn
    prob = BandProblem(ncc, disparities, unary_weight, base, conn, alphas, layout)
    out = BandResult()
    start = prob.carry_from(carry_start[0], carry_start[1]) if carry_start is not None else None
    out.stage = run_levels(prob, levels, out, kernel, tol, maxiter, max_relgap, carry, start, solver)
    out.dispmap = out.maps[-1]
    return out
