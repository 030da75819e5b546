"""Image-guided smoothness weights (no reference counterpart; the definition: include/stereo_hip.h):
the contrast of two pixels, g = max_c |im(a, c) - im(b, c)|, through a piecewise linear ramp -- w_high up to g0, w_low
from g1 on, a straight line between -- as the `alphas` of any edge list on the image's pixels and as the R x N step
weights of scanline directions (scanline.aggregate_weighted).

An image is H x W x C (or H x W), pixel id = col * H + row.  Host forms take NumPy arrays; device forms take torch
tensors of the current device: the image as a flat contiguous float64 tensor of H * W * C elements in column-major
order (image_to_device makes one), `conn` as a flat int32 tensor of 2 E entries, as the level builders keep it.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import band
from ._lib import StereoHipError
from .consistency import _p, _stream


class _Params(C.Structure):
    _fields_ = [("w_high", C.c_double), ("w_low", C.c_double), ("g0", C.c_double), ("g1", C.c_double)]


class Contrast:
    """The ramp's parameters: weight `w_high` where the contrast is at most `g0`, `w_low` where it is at least `g1`,
    linear between.  g0 == g1 is a step; w_low > w_high is allowed.  The library checks the values."""

    def __init__(self, w_high, w_low, g0, g1):
        self.w_high, self.w_low, self.g0, self.g1 = float(w_high), float(w_low), float(g0), float(g1)

    def _c(self):
        return _Params(self.w_high, self.w_low, self.g0, self.g1)

    def __repr__(self):
        return "Contrast(w_high=%r, w_low=%r, g0=%r, g1=%r)" % (self.w_high, self.w_low, self.g0, self.g1)


def _check(c):
    if not isinstance(c, Contrast):
        raise StereoHipError("contrast: a Contrast is needed (got %r)" % (c,))
    return c._c()


def _image(image):
    """-> (column-major float64 array H x W x C, H, W, C)"""
    im = np.asarray(image, dtype=np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    if im.ndim != 3:
        raise StereoHipError("contrast: an image is H x W x C or H x W (got shape %s)" % (im.shape,))
    return (np.asfortranarray(im),) + im.shape


def _shape3(shape):
    shape = tuple(int(v) for v in shape)
    return shape if len(shape) == 3 else shape + (1,)


def _directions(directions):
    try:
        d = np.array([[int(v) for v in pair] for pair in directions], dtype=np.int32).reshape(-1, 2)
    except (TypeError, ValueError):
        raise StereoHipError("contrast: directions must be a sequence of (dy, dx) pairs")
    return np.ascontiguousarray(d.reshape(-1)), d.shape[0]


def image_to_device(image):
    """An H x W x C image as the flat column-major float64 tensor the device forms read."""
    import torch
    im, H, W, Cn = _image(image)
    return torch.from_numpy(im.reshape(-1, order="F").copy()).cuda()


def edge_weights(image, conn, c):
    """stereo_contrast_edge_weights: `conn` 2 x E zero based, any graph on the image's pixels -> E alphas."""
    im, H, W, Cn = _image(image)
    conn = band._conn(conn)
    E = conn.shape[1]
    alphas = np.zeros(max(E, 1))
    par = _check(c)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_contrast_edge_weights(_p(im), C.c_int(H), C.c_int(W), C.c_int(Cn), _p(conn, C.c_uint32), C.c_int64(E),
                                                 C.byref(par), _p(alphas), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return alphas[:E]


def edge_weights_device(d_image, shape, d_conn, c, alphas=None, bad=None, stream=None, check=True):
    """stereo_contrast_edge_weights_device: `d_image` flat, `shape` = (H, W[, C]), `d_conn` flat int32 of 2 E entries.
    check=True reads the count of edges with an endpoint outside the image (or a contrast that is not finite) back --
    this waits for the stream -- and raises; the host form names the edge.  -> (alphas: E float64 tensor, bad)."""
    import torch
    from .scanline import _counter
    H, W, Cn = _shape3(shape)
    d_image = band._flat(d_image, "image", torch.float64, max(H, 0) * max(W, 0) * max(Cn, 0))
    d_conn, E = band._edges(d_conn)
    alphas = band._out(alphas, "alphas", E, d_image.device)
    bad = _counter(bad, d_image.device, stream)
    par = _check(c)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_contrast_edge_weights_device(band._vp(d_image), C.c_int(H), C.c_int(W), C.c_int(Cn), band._vp(d_conn),
                                                        C.c_int64(E), C.byref(par), C.c_void_p(alphas.data_ptr()), band._vp(bad),
                                                        C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    band._raise_bad(bad, check, "edge_weights_device: %d edge(s) with an endpoint outside the %d x %d image or a contrast that "
                    "is not finite (contrast.edge_weights names the first)", H, W)
    return alphas, bad


def step_weights(image, directions, c):
    """stereo_contrast_step_weights: -> R x N array; row r holds, per pixel, the weight of the step into it along
    directions[r], 0.0 where the pixel has no predecessor."""
    im, H, W, Cn = _image(image)
    d, R = _directions(directions)
    wstep = np.zeros((max(R, 1), max(H * W, 1)))
    par = _check(c)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_contrast_step_weights(_p(im), C.c_int(H), C.c_int(W), C.c_int(Cn), _p(d, C.c_int32), C.c_int(R),
                                                 C.byref(par), _p(wstep), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return wstep[:R, :H * W]


def step_weights_device(d_image, shape, directions, c, wstep=None, stream=None):
    """stereo_contrast_step_weights_device, launched on `stream` without waiting for it.  -> flat float64 tensor of
    R * N elements, element (r, p) at p + N * r: what scanline.aggregate_weighted_device reads."""
    import torch
    H, W, Cn = _shape3(shape)
    d_image = band._flat(d_image, "image", torch.float64, max(H, 0) * max(W, 0) * max(Cn, 0))
    d, R = _directions(directions)
    wstep = band._out(wstep, "wstep", R * max(H, 0) * max(W, 0), d_image.device)
    par = _check(c)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_contrast_step_weights_device(band._vp(d_image), C.c_int(H), C.c_int(W), C.c_int(Cn), _p(d, C.c_int32),
                                                        C.c_int(R), C.byref(par), band._vp(wstep), C.c_void_p(_stream(stream)),
                                                        err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return wstep
