"""Plane candidates: per-pixel plane sets propagated from neighbours (the definition:
include/stereo_hip.h).

A plane candidate table ``pcand`` (4 x K x N: component, label, pixel; pixels column major) says what label k means at
pixel i: a plane ``[a b c d]`` of its own.  ``gather`` builds one from the planes of an assignment (4 x N), the band's
``offsets`` (strictly ascending, containing 0.0), M source plane maps (4 x N each) and T taps ``(dy, dx)``: the pixel's
own plane moved by ``offsets_k`` along the disparity axis, then for every source and tap the source's plane at the
clamped neighbour, copied unchanged -- a plane is a function on the whole image, so the copy is the neighbour's surface
extended to this pixel.  ``plane_candidates_inputs`` makes the TRW-S problem of any table -- ``unary`` (K x N) from a
unary source of plane_band.py (``NccSource`` or ``GlobalstereoSource``), ``q`` / ``qprim`` (K x E) as
stereo_trws_positions gives them for the K proposals ``pcand[:, k, :]`` -- and ``plane_candidates_apply`` reads the planes
a labelling selects.  ``refine_plane_candidates`` builds these on the device, solves them level by level and applies the
labels.

Host forms take NumPy arrays in MATLAB shapes (planes 4 x N, a table 4 x K x N, conn 2 x E zero based).  Device forms
take torch tensors of the current device, as in plane_band.py: ``planes`` and ``out`` are contiguous float64 tensors of
4 N elements (shape (N, 4)), M sources one contiguous (M, N, 4) tensor, a table a flat float64 tensor of 4 K N elements.
The helpers of the wrappers and the level loop are band.py's, the checks of a level candidates.py's.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import candidates
from . import plane_band
from . import terms as T
from ._lib import StereoHipError
from .band import (_bad, _conn, _device_labels, _edges, _flat, _out, _raise_bad, _vec, _vp, bind_inputs, check_solver, run_levels,
                   to_device_vector)
from .candidates import _device_vectors_of_gather, _taps
from .consistency import _map, _p, _stream
from .plane_band import PlaneBandProblem, PlaneBandResult, _planes, _rescale, _source


class OrOwn:
    """A source (4 x N planes) whose planes that are not finite stand for 'the pixel's own plane': they are replaced by
    the current assignment's when a level is built (dispmap_ncc's 'wta' source, whose map has holes where the volume
    has NaN slices)."""

    def __init__(self, planes):
        self.planes = np.asfortranarray(np.asarray(planes, dtype=np.float64))
        if self.planes.ndim != 2 or self.planes.shape[0] != 4:
            raise StereoHipError("plane candidates: a source must be 4 x N planes")


def fronto(m):
    """An H x W map -> the 4 x N fronto-parallel planes [0, 0, 1, -v], pixels column major."""
    m = _map(m, "a map")
    out = np.zeros((4, m.size), order="F")
    out[2] = 1.0
    out[3] = -m.reshape(-1, order="F")
    return out


class Fit:
    """A source that is made when a level is built: the local plane fit (fit_local_device) of the
    problem's CURRENT planes, so a second level fits the first level's result.  `radius`: 1 .. 8 pixels; `tau`: the
    largest |difference| to the pixel's own disparity a tap may have to take part, in the planes' raw disparity units
    (not the rescaled ones of dispmap_globalstereo's smoothness term); +inf takes every tap.  Geometric only: it reads
    no unary, so every plane-candidate level takes it."""

    def __init__(self, radius=2, tau=1.0):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_FIT_RADIUS:
            raise StereoHipError("plane candidates: Fit's radius must be a whole number 1 .. %d (got %r)" % (MAX_FIT_RADIUS, radius))
        if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or not float(tau) >= 0.0:
            raise StereoHipError("plane candidates: Fit's tau must be a number >= 0 (got %r)" % (tau,))
        self.radius, self.tau = int(radius), float(tau)

    def __repr__(self):
        return "Fit(radius=%d, tau=%r)" % (self.radius, self.tau)


MAX_FIT_RADIUS = 8


def _shape(shape):
    H, W = (int(v) for v in shape)
    return H, W


def fit_local(planes, shape, radius=2, tau=1.0):
    """stereo_planes_fit_local for an image of `shape` = (H, W): every pixel's plane replaced by the least-squares plane
    through the disparities its neighbours' planes have at their own pixels, |dx|, |dy| <= radius, of which those within
    `tau` of the pixel's own take part (the planes' own disparity units).  -> (out 4 x N, Fortran order, bad): `bad`
    counts the pixels whose own plane has c == 0 or a component that is not finite; they keep their plane."""
    H, W = _shape(shape)
    planes = _planes(planes, H * W)
    out = np.zeros((4, max(H * W, 1)), order="F")
    bad = C.c_int32(0)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_planes_fit_local(_p(planes), C.c_int(H), C.c_int(W), C.c_int(int(radius)), C.c_double(float(tau)),
                                            _p(out), C.byref(bad), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, int(bad.value)


def _table(pcand, N):
    pcand = np.asarray(pcand, dtype=np.float64)
    if pcand.ndim != 3 or pcand.shape[0] != 4 or pcand.shape[2] != N:
        raise StereoHipError("pcand must be 4 x K x (H*W)")
    return np.asfortranarray(pcand)


def _host_sources(sources, N):
    """M x (4 N) float64, C order: source m in the storage order of 4 x N column major."""
    out = np.zeros((len(sources), 4 * N))
    for m, s in enumerate(sources):
        s = np.asarray(s, dtype=np.float64)
        if s.ndim != 2 or s.shape != (4, N):
            raise StereoHipError("a source must be 4 x N planes of the image's size")
        out[m] = s.reshape(-1, order="F")
    return out


def gather(planes, offsets, shape, sources=(), taps=()):
    """stereo_plane_candidates_gather for an image of `shape` = (H, W): `planes` 4 x N, `sources` a list of 4 x N plane
    maps -> pcand, 4 x K x N (Fortran order), K = len(offsets) + len(sources) * len(taps)."""
    H, W = _shape(shape)
    N = H * W
    planes = _planes(planes, N)
    offsets, taps = _vec(offsets, "offsets"), _taps(taps)
    src = _host_sources(list(sources), N)
    Ko, M, Tn = offsets.shape[0], src.shape[0], taps.shape[0]
    K = Ko + M * Tn
    pcand = np.zeros((4, max(K, 1), max(N, 1)), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_candidates_gather(_p(planes), C.c_int(H), C.c_int(W), _p(offsets), C.c_int(Ko),
                                                   _p(src) if M * Tn else None, C.c_int(M),
                                                   _p(taps, C.c_int32) if M * Tn else None, C.c_int(Tn), _p(pcand), err,
                                                   C.c_size_t(len(err)))
    _lib.check(rc, err)
    return pcand


def _check_source_shape(source, H, W, what):
    if (source.H, source.W) != (H, W):
        raise StereoHipError("%s: the unary source is %d x %d, the table's image %d x %d" % (what, source.H, source.W, H, W))


def plane_candidates_inputs(source, pcand, shape, conn, d_min=0.0, d_step=0.0):
    """stereo_plane_candidates_inputs_ncc / _globalstereo for the table `pcand` (4 x K x N) of an image of `shape` =
    (H, W); `source` a plane_band.NccSource or GlobalstereoSource -> (unary K x N, q K x E, qprim K x E), Fortran order."""
    source = _source(source)
    d_min, d_step = _rescale(source, d_min, d_step)
    H, W = _shape(shape)
    _check_source_shape(source, H, W, "plane_candidates_inputs")
    N = H * W
    pcand, conn = _table(pcand, N), _conn(conn)
    K, E = pcand.shape[1], conn.shape[1]
    unary = np.zeros((K, N), order="F")
    q, qprim = np.zeros((K, E), order="F"), np.zeros((K, E), order="F")
    err = _lib.errbuf()
    tail = (_p(pcand), C.c_int(K), C.c_int64(E), _p(conn, C.c_uint32), _p(unary), _p(q), _p(qprim), err, C.c_size_t(len(err)))
    if source.kind == "ncc":
        rc = _lib.lib().stereo_plane_candidates_inputs_ncc(_p(source.vol), C.c_int(H), C.c_int(W), C.c_int(source.D),
                                                           C.c_int(source.layout), _p(source.disparities),
                                                           C.c_double(source.unary_weight), *tail)
    else:
        rc = _lib.lib().stereo_plane_candidates_inputs_globalstereo(_p(source.im0), _p(source.im1), C.c_int(H), C.c_int(W),
                                                                    C.c_int(source.C), _p(source.P2), C.c_double(d_min),
                                                                    C.c_double(d_step), C.c_double(source.col_thresh), *tail)
    _lib.check(rc, err)
    return unary, q, qprim


def plane_candidates_apply(pcand, labels, shape):
    """stereo_plane_candidates_apply -> 4 x N: pcand[:, labels - 1, pixel].  `labels`: N values, one based, as
    plan.result() returns them."""
    H, W = _shape(shape)
    N = H * W
    pcand = _table(pcand, N)
    lab = plane_band._labels(labels, N)
    out = np.zeros((4, N), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_candidates_apply(_p(pcand), C.c_int(H), C.c_int(W), C.c_int(pcand.shape[1]),
                                                  _p(lab, C.c_int32), _p(out), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out


# ---------------------------------------------------------------- device forms

def _device_table(pcand, N):
    import torch
    pcand = _flat(pcand, "pcand", torch.float64)
    if N < 1 or pcand.numel() == 0 or pcand.numel() % (4 * N):
        raise StereoHipError("pcand must hold 4 * K * H * W elements")
    return pcand, pcand.numel() // (4 * N)


def gather_device(planes, offsets, shape, sources=None, taps=(), pcand=None, bad=None, stream=None, d_offsets=None,
                  d_taps=None, check=True):
    """stereo_plane_candidates_gather_device: `planes` a float64 tensor of 4 N elements, `sources` None or a contiguous
    (M, N, 4) tensor, `offsets` and `taps` host arrays (`d_offsets` / `d_taps`: their device copies, made here when not
    given).  check=True reads the count of pixels at which the own plane or a source's plane is not finite or has c == 0
    back (this waits for the stream) and raises; check=False leaves it in `bad`.
    -> (pcand: flat tensor of 4*K*N elements, bad)."""
    import torch
    H, W = _shape(shape)
    N = H * W
    planes = _flat(planes, "planes", torch.float64, 4 * N)
    offsets, taps = _vec(offsets, "offsets"), _taps(taps)
    Ko, Tn = offsets.shape[0], taps.shape[0]
    M = 0
    if sources is not None:
        if not isinstance(sources, torch.Tensor) or sources.dim() != 3 or sources.shape[1] * sources.shape[2] != 4 * N:
            raise StereoHipError("sources must be a contiguous (M, N, 4) float64 tensor on the device")
        M = sources.shape[0]
        sources = _flat(sources, "sources", torch.float64, M * 4 * N)
    K = Ko + M * Tn
    dev = planes.device
    d_offsets, d_taps = _device_vectors_of_gather(stream, offsets, d_offsets, taps, d_taps, M * Tn)
    pcand, bad = _out(pcand, "pcand", 4 * K * N, dev, new=4 * max(K, 1) * N), _bad(bad, dev)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_candidates_gather_device(
        _vp(planes), C.c_int(H), C.c_int(W), _p(offsets), _vp(d_offsets), C.c_int(Ko), _vp(sources) if M * Tn else None,
        C.c_int(M), _p(taps, C.c_int32) if M * Tn else None, _vp(d_taps) if M * Tn else None, C.c_int(Tn), _vp(pcand),
        _vp(bad), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "gather_device: the own plane or a source's plane has c == 0 or a component that is not finite at %d pixel(s)")
    return pcand, bad


def plane_candidates_inputs_device(source, pcand, shape, conn, d_min=0.0, d_step=0.0, unary=None, q=None, qprim=None,
                                   bad=None, stream=None, check=True):
    """stereo_plane_candidates_inputs_*_device on torch tensors: `pcand` a flat float64 tensor of 4*K*N elements for an
    image of `shape` = (H, W); the rest as plane_band.plane_band_inputs_device.  check=True reads the count of pixels
    with a candidate that has c == 0 or is not finite back and raises.
    -> (unary, q, qprim, bad): flat tensors K*N, K*E, K*E and the int32 counter."""
    import torch
    source = _source(source)
    d_min, d_step = _rescale(source, d_min, d_step)
    H, W = _shape(shape)
    _check_source_shape(source, H, W, "plane_candidates_inputs_device")
    N = H * W
    pcand, K = _device_table(pcand, N)
    conn, E = _edges(conn)
    dev = pcand.device
    fresh = source.device()
    if stream is not None:
        torch.cuda.current_stream().synchronize()         # (the source's copies ran on torch's current stream)
    unary, q, qprim = _out(unary, "unary", K * N, dev), _out(q, "q", K * E, dev), _out(qprim, "qprim", K * E, dev)
    bad = _bad(bad, dev)
    err = _lib.errbuf()
    tail = (_vp(pcand), C.c_int(K), C.c_int64(E), _vp(conn), _vp(unary), _vp(q), _vp(qprim), _vp(bad),
            C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    if source.kind == "ncc":
        rc = _lib.lib().stereo_plane_candidates_inputs_ncc_device(
            _vp(fresh.d_vol), C.c_int(H), C.c_int(W), C.c_int(source.D), C.c_int(source.layout), _p(source.disparities),
            _vp(fresh.d_disparities), C.c_double(source.unary_weight), *tail)
    else:
        rc = _lib.lib().stereo_plane_candidates_inputs_globalstereo_device(
            _vp(fresh.d_im0), _vp(fresh.d_im1), C.c_int(H), C.c_int(W), C.c_int(source.C), _p(source.P2), C.c_double(d_min),
            C.c_double(d_step), C.c_double(source.col_thresh), *tail)
    _lib.check(rc, err)
    _raise_bad(bad, check, "plane_candidates_inputs_device: a candidate has c == 0 or a component that is not finite at %d pixel(s)")
    return unary, q, qprim, bad


def plane_candidates_apply_device(pcand, labels, shape, out=None, bad=None, stream=None, check=True):
    """stereo_plane_candidates_apply_device: `pcand` a flat float64 tensor of 4*K*N elements, `labels` a flat int32
    tensor, one based.  check=True reads the count of labels outside 1 .. K back and raises.  -> (out (N, 4), bad)."""
    import torch
    H, W = _shape(shape)
    N = H * W
    pcand, K = _device_table(pcand, N)
    labels = _flat(labels, "labels", torch.int32, N)
    out, bad = _out(out, "out", 4 * N, pcand.device, new=(N, 4)), _bad(bad, pcand.device)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_candidates_apply_device(_vp(pcand), C.c_int(H), C.c_int(W), C.c_int(K), _vp(labels), _vp(out),
                                                         _vp(bad), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "plane_candidates_apply_device: %d label(s) outside 1 .. %d", K)
    return out, bad


def fit_local_device(planes, shape, radius=2, tau=1.0, out=None, bad=None, stream=None, check=False):
    """stereo_planes_fit_local_device: `planes` a contiguous float64 tensor of 4 N elements, launched on `stream` (a
    torch stream or a raw handle; default: torch's current stream).  check=True reads the count of pixels whose own plane
    has c == 0 or is not finite back (this waits for the stream) and raises; check=False (the default: such a pixel keeps
    its plane, which is a defined result) leaves it in `bad` and does not wait.  -> (out (N, 4), bad)."""
    import torch
    H, W = _shape(shape)
    N = H * W
    planes = _flat(planes, "planes", torch.float64, 4 * N)
    out, bad = _out(out, "out", 4 * N, planes.device, new=(N, 4)), _bad(bad, planes.device)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_planes_fit_local_device(_vp(planes), C.c_int(H), C.c_int(W), C.c_int(int(radius)),
                                                   C.c_double(float(tau)), _vp(out), _vp(bad), C.c_void_p(_stream(stream)), err,
                                                   C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "fit_local_device: %d plane(s) with c == 0 or a component that is not finite")
    return out, bad


# ---------------------------------------------------------------- levels

def _check_source(s):
    if isinstance(s, str):
        if s != "base":
            raise StereoHipError("plane candidates: a source is 'base' or 4 x N planes, or a Fit (got %r)" % (s,))
    elif not isinstance(s, (OrOwn, Fit)) and (np.ndim(s) != 2 or np.shape(s)[0] != 4):
        raise StereoHipError("plane candidates: a source is 'base' or 4 x N planes, or a Fit")


_HOW = dict(check_source=_check_source, prefix="plane candidates", single=(str, np.ndarray, OrOwn, Fit))


def check_level(level):
    """A plane-candidate level as dict(offsets: float64 vector, taps: T x 2 int32, sources: list of 'base' / Fit / 4 x N
    plane arrays / OrOwn), checked as candidates.check_level checks a candidate level."""
    return candidates.check_level(level, **_HOW)


def check_levels(levels):
    """`levels` as a list of checked plane-candidate levels (check_level); at least one."""
    return candidates.check_levels(levels, **_HOW)


class PlaneCandidateProblem(PlaneBandProblem):
    """One object's plane-candidate problems on the device, with PlaneBandProblem's interface: the source's data, the
    connectivity and the smoothness weights go up once; build() gathers a level's table around the current planes, makes
    its inputs and binds them to `plan`; apply() reads the table and moves the planes on.  A level's labels have no
    common offset grid, so it neither takes nor leaves carried messages: leave() and carry_from() give None."""

    def __init__(self, source, planes, conn, alphas=None, d_min=0.0, d_step=0.0):
        super().__init__(source, planes, conn, alphas, d_min, d_step)
        self.shape = (self.source.H, self.source.W)
        self.d_pcand = None

    labels_of = staticmethod(candidates.labels_of)

    def _source_tensor(self, level):
        import torch
        maps = []
        for s in level["sources"]:
            if isinstance(s, str):
                maps.append(self.d_planes.view(self.N, 4))
                continue
            if isinstance(s, Fit):             # (made now, from the planes the levels before this one left)
                maps.append(fit_local_device(self.d_planes, self.shape, s.radius, s.tau)[0].view(self.N, 4))
                continue
            fill = isinstance(s, OrOwn)
            s = _planes(s.planes if fill else s, self.N)
            t = torch.from_numpy(np.array(s.T, order="C")).cuda()              # (N, 4)
            if fill:
                t = torch.where(torch.isfinite(t).all(dim=1, keepdim=True), t, self.d_planes.view(self.N, 4))
            maps.append(t)
        return torch.stack(maps).contiguous() if maps and level["taps"].shape[0] else None

    def build(self, level, plan=None, tol=0.0, carry=None):
        """The inputs of the plane-candidate level `level` (check_level's dict) around the current planes, bound to
        `plan` (None: to nothing).  carry must be None."""
        if carry is not None:
            raise StereoHipError("plane candidates: a plane-candidate level does not take carried messages")
        self.offsets = level["offsets"]
        self.d_offsets = to_device_vector(self.offsets)
        self.d_pcand, _ = gather_device(self.d_planes, self.offsets, self.shape, self._source_tensor(level), level["taps"],
                                        d_offsets=self.d_offsets)
        self.d_unary, self.d_q, self.d_qprim, _ = plane_candidates_inputs_device(
            self.source, self.d_pcand, self.shape, self.d_conn, self.d_min, self.d_step)
        bind_inputs(self, plan, tol)

    def leave(self, plan, labels):
        return None

    def carry_from(self, left, scales=False):
        return None

    def apply(self, labels):
        """The planes the labels of the level built last select -> the new planes on the host, 4 x N."""
        self.d_planes, _ = plane_candidates_apply_device(self.d_pcand, _device_labels(labels), self.shape)
        return np.asfortranarray(self.d_planes.cpu().numpy().T)


def refine_plane_candidates(source, planes, kernel, tol, levels, maxiter, max_relgap, alphas=None, conn=None, d_min=0.0,
                            d_step=0.0, solver="trws"):
    """Refines the plane map `planes` (4 x N) level by level: for each plane-candidate level in `levels` --
    dict(offsets=, taps=, sources=), a source being 'base' (the current planes) or 4 x N planes -- the table is gathered
    around the current planes on the device, its problem built (stereo_plane_candidates_inputs_*_device), bound to a
    TrwsPlan(kernel, K, N, conn) -- one plan per distinct K -- iterated up to `maxiter` times (`max_relgap` as in trws)
    and applied; the selected planes are the next level's.  The source's data goes to the device once; nothing K x N or
    K x E touches the host.  conn: 2 x E zero based, default the image grid; d_min / d_step: the rescaling of the
    positions and of the globalstereo unary.  Every level starts from zero messages.
    solver: "trws", or "scanline" -- every level one scanline aggregation on its inputs (band.run_levels).
    -> plane_band.PlaneBandResult (`carried` all False)."""
    check_solver(solver)
    levels = check_levels(levels)
    source = _source(source)
    conn = T.construct_neighborhood(source.H, source.W) if conn is None else conn
    prob = PlaneCandidateProblem(source, planes, conn, alphas, d_min, d_step)
    out = PlaneBandResult()
    run_levels(prob, levels, out, kernel, tol, maxiter, max_relgap, solver=solver)
    out.planes = out.plane_maps[-1]
    return out
