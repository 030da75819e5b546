"""Map filter (no reference counterpart; the definition: include/stereo_hip.h): the image-guided
weighted median of a disparity map over a (2 r + 1)^2 window, r = 1 .. max_radius(), with the pixel every output value
came from -- the finishing step after the left-right check and the per-row fill (consistency.lr_check / lr_fill), whose
status says which pixels may vote (``pixel_weight``) and which are rewritten (``targets``).

Host forms take H x W NumPy arrays (any memory order) and an H x W x C (or H x W) image.  Device forms take torch
tensors of the current device in column-major storage, as contrast.step_weights_device does: the map, `pixel_weight`
(float64) and `targets` (int32) as contiguous tensors of H * W elements (flat, or (W, H) as consistency's device forms
keep a map), the image flat (contrast.image_to_device), and `shape` = (H, W[, C]).  Pixel id = col * H + row.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import band
from ._lib import StereoHipError
from .consistency import _map, _p, _stream
from .contrast import _check, _image, _shape3

_ENTRIES = ("stereo_map_filter_max_radius", "stereo_map_weighted_median", "stereo_map_weighted_median_device")


def _library():
    L = _lib.lib()
    for name in _ENTRIES:
        if not hasattr(L, name):
            raise StereoHipError("%s does not export %s: rebuild it with stereo_amd/csrc/build.sh" % (_lib.LIB_PATH, name))
    return L


def max_radius():
    """The largest window radius (stereo_map_filter_max_radius)."""
    return int(_library().stereo_map_filter_max_radius())


def _guide(image, contrast, what):
    if (image is None) != (contrast is None):
        raise StereoHipError("%s: image and contrast are given together, or neither" % what)
    return None if contrast is None else _check(contrast)


def weighted_median(dispmap, radius, image=None, contrast=None, pixel_weight=None, targets=None, want_source=True):
    """stereo_map_weighted_median.  `image` with `contrast` (a contrast.Contrast): the guide; `pixel_weight`: H x W,
    finite and >= 0; `targets`: H x W, a pixel is filtered where the entry is not 0 (None: everywhere).
    -> (out H x W float64, source H x W int32 of pixel ids or None, kept: the targets whose window had no weight and
    that kept their value)."""
    d = _map(dispmap, "dispmap")
    H, W = d.shape
    par = _guide(image, contrast, "weighted_median")
    im, Cn = None, 0
    if image is not None:
        im, Hi, Wi, Cn = _image(image)
        if (Hi, Wi) != (H, W):
            raise StereoHipError("weighted_median: the image must have the map's size (%d x %d, got %d x %d)" % (H, W, Hi, Wi))
    pw = tg = None
    if pixel_weight is not None:
        pw = _map(pixel_weight, "pixel_weight")
    if targets is not None:
        tg = _map(np.asarray(targets) != 0, "targets", np.int32)
    for a, what in ((pw, "pixel_weight"), (tg, "targets")):
        if a is not None and a.shape != (H, W):
            raise StereoHipError("weighted_median: %s must have the map's size" % what)
    out = np.zeros((H, W), order="F")
    source = np.zeros((H, W), np.int32, order="F") if want_source else None
    kept = C.c_int32(0)
    err = _lib.errbuf()
    rc = _library().stereo_map_weighted_median(_p(d), C.c_int(H), C.c_int(W), C.c_int(int(radius)), _p(im), C.c_int(Cn),
                                               C.byref(par) if par is not None else None, _p(pw), _p(tg, C.c_int32), _p(out),
                                               _p(source, C.c_int32), C.byref(kept), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source, int(kept.value)


def weighted_median_device(d_map, shape, radius, d_image=None, contrast=None, pixel_weight=None, targets=None, out=None,
                           source=None, kept=None, stream=None, want_source=True):
    """stereo_map_weighted_median_device (module docstring), launched on `stream` (a torch stream or a raw handle;
    default: torch's current stream) without waiting for it.  `out`, `source`, `kept`: tensors to write into, made here
    otherwise (in the map's shape; `kept` one int32, zeroed by the entry on the stream).
    -> (out, source or None, kept: the int32 tensor -- reading it waits)."""
    import torch
    from .scanline import _counter
    H, W, Cn = _shape3(shape)
    n = max(H, 0) * max(W, 0)
    d_map = band._flat(d_map, "d_map", torch.float64, n)
    par = _guide(d_image, contrast, "weighted_median_device")
    if d_image is not None:
        d_image = band._flat(d_image, "image", torch.float64, n * max(Cn, 0))
    if pixel_weight is not None:
        pixel_weight = band._flat(pixel_weight, "pixel_weight", torch.float64, n)
    if targets is not None:
        targets = band._flat(targets, "targets", torch.int32, n)
    out = torch.empty_like(d_map) if out is None else band._flat(out, "out", torch.float64, n)
    if source is None and want_source:
        source = torch.empty(d_map.shape, dtype=torch.int32, device=d_map.device)
    elif source is not None:
        source = band._flat(source, "source", torch.int32, n)
    kept = _counter(kept, d_map.device, stream)
    err = _lib.errbuf()
    rc = _library().stereo_map_weighted_median_device(band._vp(d_map), C.c_int(H), C.c_int(W), C.c_int(int(radius)),
                                                      band._vp(d_image), C.c_int(Cn if d_image is not None else 0),
                                                      C.byref(par) if par is not None else None, band._vp(pixel_weight),
                                                      band._vp(targets), band._vp(out), band._vp(source), band._vp(kept),
                                                      C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source, kept


def take_planes(planes, source):
    """A 4 x N plane map (columns in pixel-id order) gathered at `source` (H x W or N pixel ids, as weighted_median
    returns them): the plane map that goes with the filtered disparity map."""
    planes = np.asarray(planes)
    src = np.asarray(source)
    src = (src.T if src.ndim == 2 else src).reshape(-1)            # (pixel id = col * H + row)
    if planes.ndim != 2 or planes.shape[1] != src.size:
        raise StereoHipError("take_planes: planes must be 4 x N with N the source map's size")
    if src.size and (src.min() < 0 or src.max() >= src.size):
        raise StereoHipError("take_planes: a source outside 0 .. N - 1")
    return np.asfortranarray(planes[:, src])


class MedianFilter:
    """The settings of a post filter on a checked and filled map: the window `radius`; `contrast` (a contrast.Contrast)
    to guide it by the view's image, or None; sources="consistent": only pixels the check found consistent vote
    (pixel_weight = status == 0), "all": every pixel does; targets="filled": only the other pixels are rewritten
    (targets = status != 0), "all": every pixel is."""

    def __init__(self, radius, contrast=None, sources="consistent", targets="filled"):
        if sources not in ("consistent", "all") or targets not in ("filled", "all"):
            raise StereoHipError("MedianFilter: sources is 'consistent' or 'all', targets 'filled' or 'all' (got %r, %r)"
                                 % (sources, targets))
        if contrast is not None:
            _check(contrast)
        self.radius, self.contrast, self.sources, self.targets = int(radius), contrast, sources, targets

    def masks(self, status):
        """-> (pixel_weight H x W float64 or None, targets H x W int32 or None) from a status map."""
        status = np.asarray(status)
        pw = (status == 0).astype(np.float64) if self.sources == "consistent" else None
        tg = (status != 0).astype(np.int32) if self.targets == "filled" else None
        return pw, tg

    def apply(self, dispmap, status, image=None):
        """The filter on `dispmap` (a view's `filled`) with the view's `status` and, with a contrast, its `image`.
        -> weighted_median's (out, source, kept)."""
        if self.contrast is not None and image is None:
            raise StereoHipError("MedianFilter: a filter with a contrast needs the view's image")
        pw, tg = self.masks(status)
        guided = self.contrast is not None
        return weighted_median(dispmap, self.radius, image if guided else None, self.contrast, pw, tg)

    def __repr__(self):
        return "MedianFilter(radius=%r, contrast=%r, sources=%r, targets=%r)" % (self.radius, self.contrast, self.sources,
                                                                                 self.targets)
