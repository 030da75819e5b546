"""Band refinement around a solved plane map (the definition: include/stereo_hip.h).

From ``planes`` (4 x N, an object's assignment in its internal columns) and a strictly ascending vector ``offsets``
that contains 0.0, the TRW-S problem whose label k at pixel i means pixel i's own plane moved by ``offsets_k`` along
the disparity axis, ``[a_i, b_i, c_i, d_i - c_i offsets_k]``: ``unary`` (K x N) from a unary source -- the NCC sampler
(``NccSource``) or the photo-consistency term of dispmap_globalstereo (``GlobalstereoSource``) -- and ``q`` / ``qprim``
(K x E) as stereo_trws_positions gives them for those K proposals.  ``refine_plane_band`` builds these on the device,
solves them level by level and applies the labels; a slanted surface keeps its slant.

Host forms take NumPy arrays in MATLAB shapes (planes 4 x N, conn 2 x E zero based).  Device forms take torch tensors of
the current device: ``planes`` and ``refined`` are contiguous float64 tensors of 4 N elements in the storage order of
4 x N column major (shape (N, 4)), ``unary``, ``q`` and ``qprim`` flat float64 tensors in storage order, ``conn`` a flat
int32 tensor of 2 E entries, ``labels`` a flat int32 tensor.  ``offsets`` are in the planes' own disparity units.
The helpers of the wrappers, the level loop and the protocol PlaneBandProblem offers it are band.py's.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import carry as carry_mod
from . import terms as T
from ._lib import StereoHipError
from .band import (LevelsResult, _bad, _conn, _device_labels, _device_vectors, _edges, _flat, _out, _raise_bad, _vec, _volume,
                   _vp, bind_inputs, check_levels, check_solver, run_levels, to_device_vector)
from .consistency import _p, _stream


class NccSource:
    """The unary of dispmap_ncc: `ncc` H x W x D (layout 0) or D x N label fastest (layout 1, with shape=(H, W)), its
    slice positions `disparities` and the unary weight."""
    kind = "ncc"

    def __init__(self, ncc, disparities, unary_weight, layout=0, shape=None):
        ncc = np.asarray(ncc, dtype=np.float64)
        if shape is None:
            if layout != 0 or ncc.ndim != 3:
                raise StereoHipError("NccSource: shape=(H, W) is needed unless the volume is H x W x D (layout 0)")
            shape = ncc.shape[:2]
        self.H, self.W = int(shape[0]), int(shape[1])
        self.vol, self.D = _volume(ncc, layout, self.H, self.W)
        self.disparities = _vec(disparities, "disparities")
        if self.disparities.shape[0] != self.D:
            raise StereoHipError("NccSource: %d disparities for a volume of %d slices" % (self.disparities.shape[0], self.D))
        self.layout, self.unary_weight = int(layout), float(unary_weight)
        self.d_vol = self.d_disparities = None

    def device(self):
        """The volume and the slice positions on the current device (sent once)."""
        if self.d_vol is None:
            self.d_vol = _send(self.vol)
            self.d_disparities = to_device_vector(self.disparities)
        return self


class GlobalstereoSource:
    """The unary of dispmap_globalstereo: the reference image `im0`, the second image `im1` (H x W x C), P2 =
    self.P(:,:,2) (4 x 3) and col_thresh.  The rescaling (d_min, d_step) is the call's."""
    kind = "globalstereo"

    def __init__(self, im0, im1, P2, col_thresh):
        im0, im1 = np.asarray(im0, dtype=np.float64), np.asarray(im1, dtype=np.float64)
        if im0.ndim == 2:
            im0 = im0[:, :, None]
        if im1.ndim == 2:
            im1 = im1[:, :, None]
        if im0.ndim != 3 or im0.shape != im1.shape:
            raise StereoHipError("GlobalstereoSource: the two images must be H x W x C of one size")
        self.H, self.W, self.C = im0.shape
        self.im0, self.im1 = np.asfortranarray(im0), np.asfortranarray(im1)
        P2 = np.asarray(P2, dtype=np.float64)
        if P2.shape != (4, 3):
            raise StereoHipError("GlobalstereoSource: P2 must be 4 x 3")
        self.P2 = np.ascontiguousarray(P2.reshape(-1, order="F"))
        self.col_thresh = float(col_thresh)
        self.d_im0 = self.d_im1 = None

    def device(self):
        if self.d_im0 is None:
            self.d_im0 = _send(self.im0)
            self.d_im1 = _send(self.im1)
        return self


def _send(a):
    """A host array's storage as a flat tensor on the current device."""
    import torch
    flat = a.reshape(-1, order="F")
    return torch.from_numpy(flat if flat.flags.writeable else flat.copy()).cuda()     # (torch wants a writable source)


def _source(source):
    if getattr(source, "kind", None) not in ("ncc", "globalstereo"):
        raise StereoHipError("plane band: the unary source must be an NccSource or a GlobalstereoSource")
    return source


def _rescale(source, d_min, d_step):
    if source.kind == "ncc" and (float(d_min) != 0.0 or float(d_step) != 0.0):
        raise StereoHipError("plane band: the NCC source has no rescaling (d_min and d_step must be 0)")
    return float(d_min), float(d_step)


def _planes(planes, N=None):
    p = np.asarray(planes, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] != 4 or (N is not None and p.shape[1] != N):
        raise StereoHipError("plane band: planes must be 4 x N%s" % ("" if N is None else " with N = H * W = %d" % N))
    return np.asfortranarray(p)


def plane_band_inputs(source, planes, offsets, conn, d_min=0.0, d_step=0.0):
    """stereo_plane_band_inputs_ncc / _globalstereo -> (unary K x N, q K x E, qprim K x E), Fortran order."""
    source = _source(source)
    d_min, d_step = _rescale(source, d_min, d_step)
    H, W = source.H, source.W
    N = H * W
    planes, offsets, conn = _planes(planes, N), _vec(offsets, "offsets"), _conn(conn)
    K, E = offsets.shape[0], conn.shape[1]
    unary = np.zeros((K, N), order="F")
    q, qprim = np.zeros((K, E), order="F"), np.zeros((K, E), order="F")
    err = _lib.errbuf()
    tail = (_p(planes), _p(offsets), C.c_int(K), C.c_int64(E), _p(conn, C.c_uint32), _p(unary), _p(q), _p(qprim), err,
            C.c_size_t(len(err)))
    if source.kind == "ncc":
        rc = _lib.lib().stereo_plane_band_inputs_ncc(_p(source.vol), C.c_int(H), C.c_int(W), C.c_int(source.D),
                                                     C.c_int(source.layout), _p(source.disparities),
                                                     C.c_double(source.unary_weight), *tail)
    else:
        rc = _lib.lib().stereo_plane_band_inputs_globalstereo(_p(source.im0), _p(source.im1), C.c_int(H), C.c_int(W),
                                                              C.c_int(source.C), _p(source.P2), C.c_double(d_min),
                                                              C.c_double(d_step), C.c_double(source.col_thresh), *tail)
    _lib.check(rc, err)
    return unary, q, qprim


def _labels(labels, N):
    lab = np.asarray(labels).reshape(-1)
    if lab.shape[0] != N:
        raise StereoHipError("plane_band_apply: labels must hold one value per plane")
    if not np.array_equal(lab, np.rint(lab)):
        raise StereoHipError("plane_band_apply: labels must be whole numbers")
    return np.ascontiguousarray(lab, dtype=np.int32)


def plane_band_apply(planes, labels, offsets):
    """stereo_plane_band_apply -> 4 x N: [a, b, c, d - c offsets[labels - 1]].  `labels`: N values, one based, as
    plan.result() returns them."""
    planes = _planes(planes)
    N = planes.shape[1]
    offsets = _vec(offsets, "offsets")
    lab = _labels(labels, N)
    refined = np.zeros((4, N), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_band_apply(_p(planes), C.c_int64(N), _p(lab, C.c_int32), _p(offsets),
                                            C.c_int(offsets.shape[0]), _p(refined), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return refined


# ---------------------------------------------------------------- device forms

def plane_band_inputs_device(source, planes, offsets, conn, d_min=0.0, d_step=0.0, unary=None, q=None, qprim=None, bad=None,
                             stream=None, d_offsets=None, check=True):
    """stereo_plane_band_inputs_*_device on torch tensors (module docstring), launched on `stream` (a torch stream or a
    raw handle; default: torch's current stream).  `source`: an NccSource or GlobalstereoSource; its data is sent to the
    device once (source.device()).  check=True reads the count of pixels whose plane has c == 0 or is not finite back
    (this waits for the stream) and raises; check=False leaves it in `bad` and does not wait.
    -> (unary, q, qprim, bad): flat tensors K*N, K*E, K*E and the int32 counter."""
    import torch
    source = _source(source)
    d_min, d_step = _rescale(source, d_min, d_step)
    H, W = source.H, source.W
    N = H * W
    planes = _flat(planes, "planes", torch.float64, 4 * N)
    offsets = _vec(offsets, "offsets")
    K = offsets.shape[0]
    conn, E = _edges(conn)
    dev = planes.device
    fresh = source.device()
    if stream is not None:
        torch.cuda.current_stream().synchronize()         # (the source's copies ran on torch's current stream)
    d_offsets, = _device_vectors(stream, (offsets, d_offsets, "d_offsets"))
    unary, q, qprim = _out(unary, "unary", K * N, dev), _out(q, "q", K * E, dev), _out(qprim, "qprim", K * E, dev)
    bad = _bad(bad, dev)
    err = _lib.errbuf()
    tail = (_vp(planes), _p(offsets), _vp(d_offsets), C.c_int(K), C.c_int64(E), _vp(conn), _vp(unary), _vp(q), _vp(qprim), _vp(bad),
            C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    if source.kind == "ncc":
        rc = _lib.lib().stereo_plane_band_inputs_ncc_device(_vp(fresh.d_vol), C.c_int(H), C.c_int(W), C.c_int(source.D),
                                                            C.c_int(source.layout), _p(source.disparities),
                                                            _vp(fresh.d_disparities), C.c_double(source.unary_weight), *tail)
    else:
        rc = _lib.lib().stereo_plane_band_inputs_globalstereo_device(_vp(fresh.d_im0), _vp(fresh.d_im1), C.c_int(H), C.c_int(W),
                                                                     C.c_int(source.C), _p(source.P2), C.c_double(d_min),
                                                                     C.c_double(d_step), C.c_double(source.col_thresh), *tail)
    _lib.check(rc, err)
    _raise_bad(bad, check, "plane_band_inputs_device: %d plane(s) with c == 0 or a component that is not finite")
    return unary, q, qprim, bad


def plane_band_apply_device(planes, labels, offsets, refined=None, bad=None, stream=None, d_offsets=None, check=True):
    """stereo_plane_band_apply_device: `planes` 4 N float64, `labels` N int32, one based.  check=True reads the count of
    offending pixels (a label outside 1 .. K, a plane with c == 0 or not finite) back and raises.  -> (refined, bad)."""
    import torch
    planes = _flat(planes, "planes", torch.float64)
    if planes.numel() % 4 or planes.numel() == 0:
        raise StereoHipError("planes must hold 4 N elements")
    N = planes.numel() // 4
    offsets = _vec(offsets, "offsets")
    K = offsets.shape[0]
    labels = _flat(labels, "labels", torch.int32, N)
    d_offsets, = _device_vectors(stream, (offsets, d_offsets, "d_offsets"))
    refined, bad = _out(refined, "refined", 4 * N, planes.device, new=(N, 4)), _bad(bad, planes.device)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_plane_band_apply_device(_vp(planes), C.c_int64(N), _vp(labels), _p(offsets), _vp(d_offsets), C.c_int(K),
                                                   _vp(refined), _vp(bad), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "plane_band_apply_device: %d pixel(s) with a label outside 1 .. %d or a plane without a disparity", K)
    return refined, bad


# ---------------------------------------------------------------- levels

class PlaneBandResult(LevelsResult):
    """refine_plane_band's result: band.LevelsResult's lists, of which `maps` is known as `plane_maps` here (4 x N per
    level), and `planes` (4 x N, the last level's refined planes)."""

    def __init__(self):
        super().__init__()
        self.planes, self.plane_maps = None, self.maps


class PlaneBandProblem:
    """One object's plane-band problems on the device: the source's data, the connectivity and the smoothness weights go
    up once; build() makes a level's inputs from the current planes and binds them to `plan`, apply() moves the planes on.
    (The protocol the level loop drives it by: band.run_levels.)"""

    def __init__(self, source, planes, conn, alphas=None, d_min=0.0, d_step=0.0):
        import torch
        _lib.require_device()
        self.source = _source(source)
        self.d_min, self.d_step = _rescale(source, d_min, d_step)
        self.N = source.H * source.W
        planes = _planes(planes, self.N)
        self.conn = _conn(conn)
        self.E = self.conn.shape[1]
        alphas = np.ones(self.E) if alphas is None else np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).reshape(-1))
        if alphas.shape[0] != self.E:
            raise StereoHipError("refine_plane_band: alphas must hold one weight per edge")
        source.device()
        self.d_conn = torch.from_numpy(self.conn.reshape(-1, order="F").view(np.int32)).cuda()
        self.d_alphas = torch.from_numpy(alphas).cuda()
        self.d_planes = torch.from_numpy(np.array(planes.T, order="C")).cuda()       # (N, 4): 4 x N column major, a copy
        self.offsets = self.d_offsets = self.d_unary = self.d_q = self.d_qprim = self.d_receiver = None

    def receiver(self):
        """The receiving node of every edge's message row in a plan at rest (phase 1), on the device (carry.receivers)."""
        import torch
        if self.d_receiver is None:
            self.d_receiver = torch.from_numpy(carry_mod.receivers(self.N, self.conn, 1)).cuda()
        return self.d_receiver

    @staticmethod
    def labels_of(level):
        """K of the level `level` (here: a vector of offsets), before it is built."""
        return level.shape[0]

    def leave(self, plan, labels):
        """What the level built last (solved by `plan` with `labels`, one based) leaves for the next one: the carry.Carry
        into it, whatever its offsets; to be called before the next build.  A plane moved along the disparity axis moves
        its own pixel's disparity by exactly that offset, so the new level's offset 0 at pixel r lies at
        offsets[labels_r - 1] on the old axis.  None where the plan's state cannot be carried."""
        import torch
        d_m = carry_mod.save_messages(plan, self.N)
        if d_m is None:
            return None
        index = torch.from_numpy(np.asarray(labels).reshape(-1).astype(np.int64) - 1).cuda()
        return carry_mod.Carry(d_m, self.offsets, self.d_offsets[index].contiguous())

    def carry_from(self, left, scales=False):
        """The Carry into the next build from what leave() gave: that itself (it does not depend on the planes)."""
        return left

    def build(self, offsets, plan=None, tol=0.0, carry=None):
        """The inputs of the level `offsets` around the current planes, bound to `plan` (None: to nothing).  carry: a carry.Carry of the
        previous level; the plan then starts from the transferred messages, not from zero."""
        self.offsets = _vec(offsets, "offsets")
        self.d_offsets = to_device_vector(self.offsets)
        self.d_unary, self.d_q, self.d_qprim, _ = plane_band_inputs_device(
            self.source, self.d_planes, self.offsets, self.d_conn, self.d_min, self.d_step, d_offsets=self.d_offsets)
        bind_inputs(self, plan, tol)
        if carry is not None:
            carry_mod.load_carried(plan, carry, self.offsets, self.receiver(), self.N, self.d_offsets)

    def apply(self, labels):
        """The planes moved by the labels of the level built last -> the new planes on the host, 4 x N."""
        self.d_planes, _ = plane_band_apply_device(self.d_planes, _device_labels(labels), self.offsets, d_offsets=self.d_offsets)
        return np.asfortranarray(self.d_planes.cpu().numpy().T)


def refine_plane_band(source, planes, kernel, tol, levels, maxiter, max_relgap, alphas=None, conn=None, d_min=0.0, d_step=0.0,
                      carry=False, solver="trws"):
    """Refines the plane map `planes` (4 x N) level by level: for each vector of offsets in `levels` (the planes' own
    disparity units) the plane-band problem around the current planes is built on the device
    (stereo_plane_band_inputs_*_device), bound to a TrwsPlan(kernel, K, N, conn) -- one plan per distinct K -- iterated up
    to `maxiter` times (`max_relgap` as in trws) and applied (stereo_plane_band_apply_device); the refined planes are
    the next level's.  The source's data goes to the device once; nothing K x N or K x E touches the host.  conn: 2 x E
    zero based, default the image grid (construct_neighborhood); d_min / d_step: the rescaling of the positions and of
    the globalstereo unary.  carry=True: every level after the first starts from the previous level's messages, moved
    onto its own offsets, not from zero.  solver: "trws", or "scanline" -- every level one scanline
    aggregation on its inputs (band.run_levels; no carry).  -> PlaneBandResult."""
    check_solver(solver, carry)
    levels = check_levels(levels)
    source = _source(source)
    conn = T.construct_neighborhood(source.H, source.W) if conn is None else conn
    prob = PlaneBandProblem(source, planes, conn, alphas, d_min, d_step)
    out = PlaneBandResult()
    run_levels(prob, levels, out, kernel, tol, maxiter, max_relgap, carry, solver=solver)
    out.planes = out.plane_maps[-1]
    return out
