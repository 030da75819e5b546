"""Image pyramid (no reference counterpart; the definitions: include/stereo_hip.h): the 2 x 2 box
reduction of an image, the expansion of a coarse disparity map to the next finer scale, the model of a pyramid level
and ``solve_pair_ncc_pyramid``: the pair solved at the coarsest scale, the maps carried up one scale at a time, band
levels at every finer scale.  ``reduce_volume`` / ``level_volumes`` make a coarser
level's NCC volume as the 2 x 2 block mean of the finer one (``unary="blocks"``) where the default takes the NCC of the
reduced images.  ``propagate=`` runs candidate levels (candidates.py) before a level's bands.
``expand_planes`` carries a plane map to the next finer scale as planes, and ``solve_view_ncc_plane_pyramid`` is the
one-view pyramid on them: plane-candidate levels and plane bands at every finer scale.

Host forms take NumPy arrays: an image H x W x C (or H x W), a map H x W, any memory order.  Device forms take torch
tensors of the current device in column-major storage: a map is a contiguous (W, H) tensor as lr_check_device takes
it, an image a contiguous (C, W, H) tensor (``torch.from_numpy(np.ascontiguousarray(im.transpose(2, 1, 0)))``).
"""
import ctypes as C
import math
import time

import numpy as np

from . import _lib
from . import band
from . import carry as carry_mod
from . import consistency
from . import terms as T
from ._lib import StereoHipError
from .consistency import _device_map, _map, _p, _stream
from .trws import TrwsPlan

MODES = {"nearest": 0, "guided": 1}
MAX_LEVELS = 5
DEFAULT_BAND = (-2.0, -1.0, 0.0, 1.0, 2.0)


def coarse_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def _image(im, what):
    im = np.asarray(im, dtype=np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    if im.ndim != 3:
        raise StereoHipError("%s must be an H x W x C array" % what)
    return np.asfortranarray(im)


def _mode(mode):
    if mode in MODES:
        return MODES[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool):
        return int(mode)        # (the library refuses a number other than 0 / 1)
    raise StereoHipError("expand must be 'nearest' or 'guided' (got %r)" % (mode,))


def reduce(im):
    """stereo_pyramid_reduce -> the (H + 1) // 2 x (W + 1) // 2 x C image (H x W in, H x W out)."""
    flat = np.ndim(im) == 2
    im = _image(im, "im")
    H, W, Cn = im.shape
    Hc, Wc = coarse_size(H, W)
    out = np.zeros((max(Hc, 0), max(Wc, 0), max(Cn, 0)), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_reduce(_p(im), C.c_int(H), C.c_int(W), C.c_int(Cn), _p(out), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out[:, :, 0] if flat else out


def expand(d_coarse, shape, mode="guided", im_fine=None, im_coarse=None, want_source=True):
    """stereo_pyramid_expand: the coarse map to the fine size `shape` = (H, W) -> (out H x W float64, source H x W
    int32 or None).  mode 'nearest' / 0 needs no images; 'guided' / 1 takes the view's own image at both scales."""
    mode = _mode(mode)
    d_coarse = _map(d_coarse, "d_coarse")
    H, W = (int(v) for v in shape)
    Hc, Wc = d_coarse.shape
    Cn = 1
    if mode == 1:
        if im_fine is None or im_coarse is None:
            raise StereoHipError("expand: the guided mode needs im_fine and im_coarse")
        im_fine, im_coarse = _image(im_fine, "im_fine"), _image(im_coarse, "im_coarse")
        Cn = im_fine.shape[2]
        if im_fine.shape != (H, W, Cn) or im_coarse.shape != (Hc, Wc, Cn):
            raise StereoHipError("expand: im_fine must be H x W x C and im_coarse of d_coarse's size with the same C "
                                 "(got %s and %s)" % (im_fine.shape, im_coarse.shape))
    else:
        im_fine = im_coarse = None
    out = np.zeros((max(H, 0), max(W, 0)), order="F")
    source = np.zeros((max(H, 0), max(W, 0)), np.int32, order="F") if want_source else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_expand(_p(d_coarse), C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W), C.c_int(mode),
                                          _p(im_fine), _p(im_coarse), C.c_int(Cn), _p(out), _p(source, C.c_int32), err,
                                          C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source


# ---------------------------------------------------------------- device forms

def _device_image(t, what, shape=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
        raise StereoHipError("%s must be a contiguous (C, W, H) float64 tensor on the device (column-major H x W x C)" % what)
    if t.device.index != torch.cuda.current_device():
        raise StereoHipError("%s must be on the current device" % what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise StereoHipError("%s must have the size (C, W, H) = %s (got %s)" % (what, tuple(shape), tuple(t.shape)))
    return t


def image_to_device(im):
    """An H x W x C host image as the (C, W, H) tensor the device forms take."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(_image(im, "im").transpose(2, 1, 0))).cuda()


def image_to_host(t):
    return t.cpu().numpy().transpose(2, 1, 0)


def reduce_device(im, out=None, stream=None):
    """stereo_pyramid_reduce_device on a (C, W, H) tensor, launched on `stream` (a torch stream or a raw handle; default:
    torch's current stream) without waiting for it -> the (C, Wc, Hc) tensor."""
    import torch
    im = _device_image(im, "im")
    Cn, W, H = im.shape
    Hc, Wc = coarse_size(H, W)
    out = torch.empty((Cn, Wc, Hc), dtype=torch.float64, device=im.device) if out is None else _device_image(out, "out", (Cn, Wc, Hc))
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_reduce_device(C.c_void_p(im.data_ptr()), C.c_int(H), C.c_int(W), C.c_int(Cn),
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(_stream(stream)), err,
                                                 C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out


def expand_device(d_coarse, shape, mode="guided", im_fine=None, im_coarse=None, out=None, source=None, stream=None,
                  want_source=True):
    """stereo_pyramid_expand_device: `d_coarse` a (Wc, Hc) map tensor, the images (C, W, H) / (C, Wc, Hc) tensors,
    `shape` = (H, W) -> (out (W, H) float64, source (W, H) int32 or None)."""
    import torch
    mode = _mode(mode)
    d_coarse = _device_map(d_coarse, "d_coarse", np.float64)
    H, W = (int(v) for v in shape)
    Wc, Hc = d_coarse.shape
    Cn = 1
    if mode == 1:
        if im_fine is None or im_coarse is None:
            raise StereoHipError("expand_device: the guided mode needs im_fine and im_coarse")
        im_fine = _device_image(im_fine, "im_fine")
        Cn = im_fine.shape[0]
        _device_image(im_fine, "im_fine", (Cn, W, H))
        im_coarse = _device_image(im_coarse, "im_coarse", (Cn, Wc, Hc))
    else:
        im_fine = im_coarse = None
    out = torch.empty((W, H), dtype=torch.float64, device=d_coarse.device) if out is None else _device_map(out, "out", np.float64, (W, H))
    if source is None and want_source:
        source = torch.empty((W, H), dtype=torch.int32, device=d_coarse.device)
    elif source is not None:
        source = _device_map(source, "source", np.int32, (W, H))
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_expand_device(vp(d_coarse), C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W), C.c_int(mode),
                                                 vp(im_fine), vp(im_coarse), C.c_int(Cn), vp(out), vp(source),
                                                 C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source


# ---------------------------------------------------------------- a plane map to the next finer scale

def _coarse_planes(p_coarse, H, W):
    from .plane_band import _planes
    Hc, Wc = coarse_size(H, W)
    p = np.asarray(p_coarse, dtype=np.float64)
    if p.ndim != 2 or p.shape != (4, Hc * Wc):
        raise StereoHipError("expand_planes: p_coarse must be 4 x (Hc * Wc) planes of the coarse size %d x %d of %d x %d "
                             "(got %s)" % (Hc, Wc, H, W, p.shape))
    return _planes(p), Hc, Wc


def expand_planes(p_coarse, shape, mode="guided", im_fine=None, im_coarse=None, want_source=True):
    """stereo_pyramid_expand_planes: the coarse plane map (4 x Nc, pixels column major) to the fine size `shape` =
    (H, W) as planes -> (out 4 x N float64, source H x W int32 or None).  The modes and the images are expand's."""
    mode = _mode(mode)
    H, W = (int(v) for v in shape)
    p_coarse, Hc, Wc = _coarse_planes(p_coarse, H, W)
    Cn = 1
    if mode == 1:
        if im_fine is None or im_coarse is None:
            raise StereoHipError("expand_planes: the guided mode needs im_fine and im_coarse")
        im_fine, im_coarse = _image(im_fine, "im_fine"), _image(im_coarse, "im_coarse")
        Cn = im_fine.shape[2]
        if im_fine.shape != (H, W, Cn) or im_coarse.shape != (Hc, Wc, Cn):
            raise StereoHipError("expand_planes: im_fine must be H x W x C and im_coarse of the coarse size with the same C "
                                 "(got %s and %s)" % (im_fine.shape, im_coarse.shape))
    else:
        im_fine = im_coarse = None
    out = np.zeros((4, max(H * W, 1)), order="F")
    source = np.zeros((max(H, 0), max(W, 0)), np.int32, order="F") if want_source else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_expand_planes(_p(p_coarse), C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W), C.c_int(mode),
                                                 _p(im_fine), _p(im_coarse), C.c_int(Cn), _p(out), _p(source, C.c_int32), err,
                                                 C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source


def expand_planes_device(p_coarse, shape, mode="guided", im_fine=None, im_coarse=None, out=None, source=None, stream=None,
                         want_source=True):
    """stereo_pyramid_expand_planes_device: `p_coarse` a contiguous float64 tensor of 4 Nc elements (shape (Nc, 4), as
    in plane_band.py), the images (C, W, H) / (C, Wc, Hc) tensors, `shape` = (H, W), launched on `stream` without
    waiting for it -> (out (N, 4) float64, source (W, H) int32 or None)."""
    import torch
    mode = _mode(mode)
    H, W = (int(v) for v in shape)
    Hc, Wc = coarse_size(H, W)
    p_coarse = band._flat(p_coarse, "p_coarse", torch.float64, 4 * Hc * Wc)
    Cn = 1
    if mode == 1:
        if im_fine is None or im_coarse is None:
            raise StereoHipError("expand_planes_device: the guided mode needs im_fine and im_coarse")
        im_fine = _device_image(im_fine, "im_fine")
        Cn = im_fine.shape[0]
        _device_image(im_fine, "im_fine", (Cn, W, H))
        im_coarse = _device_image(im_coarse, "im_coarse", (Cn, Wc, Hc))
    else:
        im_fine = im_coarse = None
    out = band._out(out, "out", 4 * H * W, p_coarse.device, new=(H * W, 4))
    if source is None and want_source:
        source = torch.empty((W, H), dtype=torch.int32, device=p_coarse.device)
    elif source is not None:
        source = _device_map(source, "source", np.int32, (W, H))
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_expand_planes_device(vp(p_coarse), C.c_int(Hc), C.c_int(Wc), C.c_int(H), C.c_int(W),
                                                        C.c_int(mode), vp(im_fine), vp(im_coarse), C.c_int(Cn), vp(out),
                                                        vp(source), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out, source


# ---------------------------------------------------------------- a level's volume from the finer one

def _short(v, what):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1:
        raise StereoHipError("%s must be a vector" % what)
    return np.ascontiguousarray(v)


def _coarse_volume_shape(Hc, Wc, Kc, layout):
    return (Hc, Wc, Kc) if layout == 0 else (Kc, Hc * Wc)


def reduce_volume(vol, shape, disparities, sample_at, layout=0):
    """stereo_pyramid_reduce_volume: the NCC volume `vol` of `shape` = (H, W) pixels with slices at `disparities`
    (layout 0: H x W x D, layout 1: D x N) -> the volume of the coarse size whose slice j is the 2 x 2 block mean of the
    sampler's values at the disparity sample_at[j], in the input's layout (Hc x Wc x Kc or Kc x Nc, Fortran order)."""
    H, W = (int(v) for v in shape)
    vol, D = band._volume(vol, layout, H, W)
    disparities, sample_at = _short(disparities, "disparities"), _short(sample_at, "sample_at")
    if disparities.shape[0] != D:
        raise StereoHipError("reduce_volume: %d disparities for a volume of %d slices" % (disparities.shape[0], D))
    Hc, Wc = coarse_size(H, W)
    Kc = sample_at.shape[0]
    out = np.zeros(_coarse_volume_shape(max(Hc, 0), max(Wc, 0), Kc, 0 if layout == 0 else 1), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_reduce_volume(_p(vol), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)),
                                                 _p(disparities), _p(sample_at), C.c_int(Kc), _p(out), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out


def reduce_volume_device(vol, shape, disparities, sample_at, layout=0, out=None, stream=None, d_disparities=None,
                         d_sample_at=None):
    """stereo_pyramid_reduce_volume_device: `vol` a flat float64 tensor of H * W * D elements in storage order, launched
    on `stream` (a torch stream or a raw handle; default: torch's current stream) without waiting for it.  `disparities`
    and `sample_at` are host vectors; `d_disparities` / `d_sample_at`: their device copies, made here when not given.
    -> the flat tensor of Hc * Wc * Kc elements."""
    import torch
    H, W = (int(v) for v in shape)
    disparities, sample_at = _short(disparities, "disparities"), _short(sample_at, "sample_at")
    D, Kc = disparities.shape[0], sample_at.shape[0]
    Hc, Wc = coarse_size(H, W)
    vol = band._flat(vol, "vol", torch.float64, H * W * D)
    made_here = d_disparities is None or d_sample_at is None
    d_disparities = band.to_device_vector(disparities) if d_disparities is None else band._flat(d_disparities, "d_disparities", torch.float64, D)
    d_sample_at = band.to_device_vector(sample_at) if d_sample_at is None else band._flat(d_sample_at, "d_sample_at", torch.float64, Kc)
    if made_here and stream is not None:
        torch.cuda.current_stream().synchronize()     # the copies ran on torch's current stream, the kernel will not
    out = torch.empty(Hc * Wc * Kc, dtype=torch.float64, device=vol.device) if out is None else band._flat(out, "out", torch.float64, Hc * Wc * Kc)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_pyramid_reduce_volume_device(vp(vol), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)),
                                                        _p(disparities), vp(d_disparities), _p(sample_at), vp(d_sample_at),
                                                        C.c_int(Kc), vp(out), C.c_void_p(_stream(stream)), err,
                                                        C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out


# ---------------------------------------------------------------- the level model

def level_model(kernel, tol, level):
    """(tol_l, edge weight) of level `level` (scale s = 2^level) in coarse disparity units: tol / s^k and s^(k - 1),
    k = 1 or 2 the smoothness kernel's exponent.  The unary weight is the caller's at every level."""
    k = int(kernel)
    if k not in (1, 2):
        raise StereoHipError("the level model is defined for the smoothness kernels 1 and 2 (got %r)" % (kernel,))
    s = float(1 << int(level))
    return float(tol) / s ** k, s ** (k - 1)


def level_disparities(disparities, level):
    """The slices of a level: the caller's at level 0, arange(floor(min / s), ceil(max / s) + 1) above."""
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    if level == 0:
        return disparities
    s = float(1 << int(level))
    return np.arange(math.floor(disparities.min() / s), math.ceil(disparities.max() / s) + 1, dtype=np.float64)


def level_sample_at(finer, coarser):
    """The finer level's disparities its coarser level's slices stand for: twice the slice, and for a slice whose doubled
    value leaves the finer range the nearest end of it (so the sampler's -1e6 never enters a level's volume)."""
    finer = np.asarray(finer, dtype=np.float64).reshape(-1)
    return np.clip(2.0 * np.asarray(coarser, dtype=np.float64).reshape(-1), finer.min(), finer.max())


def level_volumes(volume, shape, disparities, levels, layout=0):
    """The NCC volumes of the levels 0 .. `levels` from the full-size one (`shape` = (H, W), slices `disparities`): each
    level by reduce_volume_device from the one below it, as the images are reduced, with the slices of level_disparities
    and the sample positions of level_sample_at.  A level's device buffer is released once the next one is made.
    -> the list of host volumes in the input's layout, level 0 first (the input itself)."""
    import torch
    H, W = (int(v) for v in shape)
    vol, _ = band._volume(volume, layout, H, W)
    out = [vol]
    d_vol = torch.from_numpy(vol.reshape(-1, order="F")).cuda()
    for l in range(1, levels + 1):
        finer, coarser = level_disparities(disparities, l - 1), level_disparities(disparities, l)
        d_vol = reduce_volume_device(d_vol, (H, W), finer, level_sample_at(finer, coarser), layout)
        H, W = coarse_size(H, W)
        out.append(d_vol.cpu().numpy().reshape(_coarse_volume_shape(H, W, coarser.shape[0], layout), order="F"))
    return out


UNARY = ("images", "blocks")


def check_unary(unary):
    """'images': a level's volume is the NCC of the reduced images; 'blocks': the block mean of the
    finer level's volume, the level model's own unary."""
    if not isinstance(unary, str) or unary not in UNARY:
        raise StereoHipError("pyramid: unary must be 'images' or 'blocks' (got %r)" % (unary,))
    return unary


def _check_offsets(v):
    if not (np.isfinite(v).all() and (np.diff(v) > 0).all() and (v == 0.0).any()):
        raise StereoHipError("bands: a vector of offsets must be finite, strictly ascending and contain 0 (got %s)" % (v.tolist(),))


def check_plan(levels, maxiter, bands, expand):
    """The checked arguments of a pyramid solve -> (levels, maxiter per level 0 .. levels, bands per level 0 .. levels - 1
    as lists of float64 vectors, the expand mode's number)."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MAX_LEVELS:
        raise StereoHipError("pyramid: levels (the number of reductions) must be 1 .. %d (got %r)" % (MAX_LEVELS, levels))
    levels = int(levels)
    if expand not in MODES:
        raise StereoHipError("pyramid: expand must be 'nearest' or 'guided' (got %r)" % (expand,))
    if np.ndim(maxiter) == 0:
        maxiter = [int(maxiter)] * (levels + 1)
    else:
        maxiter = [int(m) for m in maxiter]
        if len(maxiter) != levels + 1:
            raise StereoHipError("pyramid: maxiter must be a scalar or one value per scale, level 0 first (%d values, got %d)"
                                 % (levels + 1, len(maxiter)))
    if bands is None:
        bands = [[DEFAULT_BAND]] * levels
    try:
        n = len(bands)
    except TypeError:
        raise StereoHipError("pyramid: bands must hold one sequence of offset vectors per level 0 .. levels - 1")
    if n != levels or isinstance(bands, dict):
        raise StereoHipError("pyramid: bands must hold one sequence of offset vectors per level 0 .. levels - 1 "
                             "(%d, got %d)" % (levels, n))
    checked = []
    for l, vectors in enumerate(bands):
        try:
            vectors = band.check_levels(vectors)
        except (TypeError, ValueError):
            raise StereoHipError("pyramid: bands[%d] must be a sequence of offset vectors" % l)
        for v in vectors:
            _check_offsets(v)
        checked.append(vectors)
    return levels, maxiter, checked, MODES[expand]


def check_propagate(propagate, levels):
    """`propagate` of a pyramid solve -> per level 0 .. levels - 1 a list of checked candidate levels
    (candidates.check_level), empty where a level has none; None stays None."""
    if propagate is None:
        return None
    from . import candidates
    try:
        n = len(propagate)
    except TypeError:
        n = -1
    if n != levels or isinstance(propagate, (dict, str)):
        raise StereoHipError("pyramid: propagate must hold one sequence of candidate levels per level 0 .. levels - 1 "
                             "(%d, got %d)" % (levels, n))
    checked = []
    for l, passes in enumerate(propagate):
        if passes is None:
            passes = []
        if isinstance(passes, dict):
            passes = [passes]
        try:
            checked.append([candidates.check_level(c) for c in passes])
        except TypeError:
            raise StereoHipError("pyramid: propagate[%d] must be a sequence of candidate levels" % l)
    return checked


CARRY = ("none", "levels", "scales")


def check_carry(carry):
    """'none': every stage starts from zero messages; 'levels': the bands of one scale carry from one to the next;
    'scales': also the last stage of a scale into the first band of the next finer one."""
    if carry not in CARRY:
        raise StereoHipError("pyramid: carry must be 'none', 'levels' or 'scales' (got %r)" % (carry,))
    return carry


def reduce_images(images, levels):
    """Every image reduced `levels` times on the device -> per level 0 .. levels the list of host images (level 0: the
    inputs as float64) and the list of their device tensors."""
    host = [[np.asarray(im, dtype=np.float64) for im in images]]
    dev = [[image_to_device(im) for im in host[0]]]
    for _ in range(levels):
        dev.append([reduce_device(t) for t in dev[-1]])
        host.append([image_to_host(t) for t in dev[-1]])
    return host, dev


def _expand_view(dispmap, shape, mode, d_fine, d_coarse):
    """One view's map to the next finer scale with the view's device images -> (map, source) on the host."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(np.asarray(dispmap, dtype=np.float64).T)).cuda()
    out, source = expand_device(d, shape, mode, d_fine, d_coarse)
    return out.cpu().numpy().T, source.cpu().numpy().T


class PyramidResult:
    """solve_pair_ncc_pyramid's result.  `levels[l]`, l = 0 (the input's size) .. the number of reductions, is that
    scale's PairResult: per view the maps, labels, energies, bounds, iterations and kernel families of its passes (at the
    coarsest scale the solve, below it one pass per offset vector), status, residual, filled and source of its last
    check, and below the coarsest scale `expanded` / `expand_source`, the map the level started from and the
    expansion's candidate numbers; `levels[l].times` has the level's seconds per stage.  `disparities[l]`, `tol[l]`,
    `smooth_weight[l]`: the level's model.  `left` / `right` are the views of level 0; `times` the seconds of the
    stages outside a level (`reduce`; with unary 'blocks' also `volumes`: the full-size volumes and their reductions) and
    per level (`level_<l>`); `unary`: where the levels' volumes came from (check_unary)."""

    def __init__(self):
        self.levels, self.disparities, self.tol, self.smooth_weight = [], [], [], []
        self.times = {}
        self.unary = "images"

    @property
    def left(self):
        return self.levels[0].left

    @property
    def right(self):
        return self.levels[0].right

    @property
    def views(self):
        return self.levels[0].views


def solve_pair_ncc_pyramid(images, disparities, kernel, unary_weight, tol, levels, maxiter, max_relgap, bands=None,
                           expand="guided", check_tol=1.0, carry="none", unary="images", propagate=None):
    """Both views of a rectified pair, coarse to fine.  Both images are reduced `levels` times (1 .. 5)
    on the device; solve_pair_ncc runs at the coarsest scale with that level's model (level_model, level_disparities);
    then for each finer level l each view's map is expanded with the view's own images of the two scales (`expand`:
    'guided' or 'nearest'), and for every vector of offsets in bands[l] (default: one band, [-2 .. 2]; one coarse label
    is two fine pixels) both views run their band problem around the current map as a two-member TrwsBatch
    (consistency.run_band_levels, the loop of solve_pair_ncc(band_levels=)), with the level's volume from pair_volumes
    on the level's images; every pass ends in a cross-check with check_tol / 2^l and a fill.  The caller's sub-pixel
    levels are further vectors in bands[0].  maxiter: a scalar, or one value per scale with level 0 first.
    carry (check_carry): 'levels' carries the messages between the bands of one scale, 'scales' also from the last stage
    of a scale into the first band of the next finer one; every view's `carried` says per pass whether it was.
    unary (check_unary): 'blocks' takes pair_volumes once, at full size, and every level's volumes from level_volumes
    (DESIGN.md 6.6); the images are reduced all the same, for the guided expansion.
    propagate (check_propagate): per level 0 .. levels - 1 a list of candidate levels that run after the
    expansion and before that level's bands, both views as a two-member TrwsBatch, each pass ending in the same check
    and fill; a candidate pass neither takes nor leaves carried messages, so the band after one starts from zero.
    -> PyramidResult."""
    levels, maxiter, bands, mode = check_plan(levels, maxiter, bands, expand)
    propagate = check_propagate(propagate, levels)
    carry = check_carry(carry)
    unary = check_unary(unary)
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    if len(images) != 2:
        raise StereoHipError("solve_pair_ncc_pyramid: images must be the two views of a pair, left first (got %d)" % len(images))
    shapes = [np.shape(im) for im in images]
    if shapes[0] != shapes[1] or len(shapes[0]) != 3 or shapes[0][2] != 3:
        raise StereoHipError("solve_pair_ncc_pyramid: the two images must be H x W x 3 arrays of one size (got %s and %s)" % tuple(shapes))
    if disparities.size < 1:
        raise StereoHipError("solve_pair_ncc_pyramid: no disparities")
    level_model(kernel, tol, 0)
    _lib.require_device()
    clock = time.perf_counter
    out = PyramidResult()
    t0 = clock()
    host, dev = reduce_images(images, levels)
    out.times["reduce"] = clock() - t0
    out.levels = [None] * (levels + 1)
    out.unary = unary
    for l in range(levels + 1):
        tol_l, w_l = level_model(kernel, tol, l)
        out.disparities.append(level_disparities(disparities, l))
        out.tol.append(tol_l); out.smooth_weight.append(w_l)
    block_volumes = None                      # per view the volumes of the levels 0 .. levels
    if unary == "blocks":
        t0 = clock()
        block_volumes = [level_volumes(vol, shapes[0][:2], disparities, levels, layout=1)
                         for vol in consistency.pair_volumes(host[0], disparities)]
        out.times["volumes"] = clock() - t0

    t0 = clock()
    L = levels
    out.levels[L] = consistency.solve_pair_ncc(host[L], out.disparities[L], kernel, unary_weight, out.tol[L], maxiter[L],
                                               max_relgap, check_tol=check_tol / (1 << L), smooth_weight=out.smooth_weight[L],
                                               carry=carry == "scales",
                                               volumes=None if block_volumes is None else [v[L] for v in block_volumes])
    out.times["level_%d" % L] = clock() - t0
    for l in range(levels - 1, -1, -1):
        t0 = clock()
        H, W = host[l][0].shape[:2]
        res = out.levels[l] = consistency.PairResult()
        for i, (view, coarse) in enumerate(zip(res.views, out.levels[l + 1].views)):
            view.expanded, view.expand_source = _expand_view(coarse.dispmap, (H, W), mode, dev[l][i], dev[l + 1][i])
            view.dispmap = view.expanded
        res.times["expand"] = clock() - t0
        t1 = clock()
        volumes = consistency.pair_volumes(host[l], out.disparities[l]) if block_volumes is None else [v[l] for v in block_volumes]
        res.times["volumes"] = clock() - t1
        conn = T.construct_neighborhood(H, W)
        alphas = np.ones(conn.shape[1]) * out.smooth_weight[l]
        band_plans = {}
        try:
            stages = out.levels[l + 1].stages if carry == "scales" else None
            if propagate is not None and propagate[l]:
                from . import candidates
                problems = [candidates.CandidateProblem(vol, out.disparities[l], unary_weight, view.dispmap, conn, alphas, layout=1)
                            for vol, view in zip(volumes, res.views)]
                consistency.run_band_levels(res, problems, propagate[l], band_plans, kernel, conn, out.tol[l], maxiter[l],
                                            max_relgap, check_tol / (1 << l), name="propagate")
                stages = None                 # (a candidate pass hands on no messages)
            problems = [band.BandProblem(vol, out.disparities[l], unary_weight, view.dispmap, conn, alphas, layout=1)
                        for vol, view in zip(volumes, res.views)]
            consistency.run_band_levels(res, problems, bands[l], band_plans, kernel, conn, out.tol[l], maxiter[l], max_relgap,
                                        check_tol / (1 << l), carry=carry != "none", stages=stages, scales=True)
        finally:
            for plan in (p for pair in band_plans.values() for p in pair):
                plan.close()
        out.times["level_%d" % l] = clock() - t0
    return out


# ---------------------------------------------------------------- one view (dispmap_ncc.solve_pyramid)

def _check_volume_argument(volume, unary):
    if volume is not None and unary != "blocks":
        raise StereoHipError("pyramid: a volume is taken with unary='blocks' only ('images' makes every level's own)")


def _view_setup(out, images, disparities, kernel, tol, levels, unary, volume):
    """What the one-view solves share before the coarsest solve: the images reduced `levels` times, the level model in
    `out` (disparities, tol, smooth_weight, unary, times["volumes"]) and the levels' volumes.
    -> (host images per level, device images per level, the volumes' layout, level_volume(l) -> level l's volume)."""
    host, dev = reduce_images(images[:2], levels)
    out.unary = unary
    for l in range(levels + 1):
        tol_l, w_l = level_model(kernel, tol, l)
        out.disparities.append(level_disparities(disparities, l))
        out.tol.append(tol_l); out.smooth_weight.append(w_l)
    out.times["volumes"] = 0.0
    layout, volumes = 1, None

    def level_volume(l):
        """Level l's volume: a block volume, or ('images') made here from the level's images, one level at a time."""
        t0 = time.perf_counter()
        vol = volumes[l] if volumes is not None else T.ncc_volume(host[l][0], host[l][1], out.disparities[l], 2, layout=1)
        out.times["volumes"] += time.perf_counter() - t0
        return vol

    if unary == "blocks":
        t0 = time.perf_counter()
        if volume is None:
            volume = T.ncc_volume(host[0][0], host[0][1], disparities, 2, layout=1)
        layout = 0 if np.ndim(volume) == 3 else 1
        volumes = level_volumes(volume, host[0][0].shape[:2], disparities, levels, layout)
        out.times["volumes"] = time.perf_counter() - t0
    return host, dev, layout, level_volume


def _solve_coarsest(out, host, level_volume, layout, kernel, unary_weight, maxiter, max_relgap, want_stage):
    """The coarsest level of a one-view solve: one TrwsPlan on the level's slices; its labels, energy, bound, iterations,
    path and carried = False go into `out`.  -> (the level's map H x W, its carry.Stage if want_stage else None)."""
    L = len(out.disparities) - 1
    H, W = host[L][0].shape[:2]
    conn = T.construct_neighborhood(H, W)
    vol = level_volume(L)
    if layout == 0:
        vol = vol.reshape((H * W, -1), order="F").T           # D x N for the upload
    plan = TrwsPlan(int(kernel), out.disparities[L].shape[0], H * W, conn)
    try:
        plan.upload(unary_weight * (1.0 - vol), np.ones(conn.shape[1]) * out.smooth_weight[L], out.tol[L],
                    positions=out.disparities[L])
        plan.iterate(maxiter[L], max_relgap)
        labels, en, lb, it = plan.result()
        out.paths[L].append(plan.path())
        out.carried[L].append(False)
        stage = carry_mod.full_range_stage(plan, out.disparities[L], conn, (H, W)) if want_stage else None
    finally:
        plan.close()
    out.labels[L].append(labels); out.energy[L].append(en); out.lower_bound[L].append(lb); out.iterations[L].append(it)
    return out.disparities[L][labels.astype(np.int64) - 1].reshape(W, H).T, stage


class ViewPyramidResult:
    """solve_view_ncc_pyramid's result: `dispmap` (level 0's last map) and per level l, index l: `maps` (the maps of the
    level's passes), `expanded` / `expand_source` (None at the coarsest level), `labels`, `energy`, `lower_bound`,
    `iterations`, `paths`, `carried` (lists per pass), `disparities`, `tol`, `smooth_weight`; `unary`: where the levels'
    volumes came from (check_unary), `times["volumes"]`: the seconds spent making them."""

    def __init__(self, n):
        self.dispmap = None
        self.unary, self.times = "images", {}
        for name in ("maps", "labels", "energy", "lower_bound", "iterations", "paths", "carried"):
            setattr(self, name, [[] for _ in range(n)])
        self.expanded, self.expand_source = [None] * n, [None] * n
        self.disparities, self.tol, self.smooth_weight = [], [], []


def solve_view_ncc_pyramid(images, disparities, kernel, unary_weight, tol, levels, maxiter, max_relgap, bands=None,
                           expand="guided", carry="none", unary="images", volume=None, propagate=None):
    """One view, coarse to fine: `images` = (the reference image, the other one), a pixel at column x with disparity d
    matching column x - d of the other.  The steps of solve_pair_ncc_pyramid for one view with solo plans: the volume
    of a level is terms.ncc_volume on the level's images, the coarsest level one TrwsPlan on the level's slices, every
    finer level band.refine_band around the expanded map.  No cross-check.  carry: as in solve_pair_ncc_pyramid.
    unary (check_unary): with 'blocks' every level's volume comes from level_volumes on the full-size volume, which is
    `volume` where given (H x W x D, or D x N: told apart by the number of dimensions) and terms.ncc_volume on the
    images otherwise.  propagate: as in solve_pair_ncc_pyramid (candidates.refine_candidates before a level's bands).
    -> ViewPyramidResult."""
    levels, maxiter, bands, mode = check_plan(levels, maxiter, bands, expand)
    propagate = check_propagate(propagate, levels)
    carry = check_carry(carry)
    unary = check_unary(unary)
    _check_volume_argument(volume, unary)
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    level_model(kernel, tol, 0)
    _lib.require_device()
    out = ViewPyramidResult(levels + 1)
    host, dev, layout, level_volume = _view_setup(out, images, disparities, kernel, tol, levels, unary, volume)
    current, stage = _solve_coarsest(out, host, level_volume, layout, kernel, unary_weight, maxiter, max_relgap, carry == "scales")
    out.maps[levels].append(current)
    for l in range(levels - 1, -1, -1):
        H, W = host[l][0].shape[:2]
        out.expanded[l], out.expand_source[l] = _expand_view(current, (H, W), mode, dev[l][0], dev[l + 1][0])
        conn = T.construct_neighborhood(H, W)
        vol, alphas = level_volume(l), np.ones(conn.shape[1]) * out.smooth_weight[l]
        start, results = out.expanded[l], []
        if propagate is not None and propagate[l]:
            from . import candidates
            results.append(candidates.refine_candidates(vol, out.disparities[l], unary_weight, start, kernel, out.tol[l], propagate[l],
                                                        maxiter[l], max_relgap, alphas=alphas, layout=layout, conn=conn))
            start, stage = results[0].dispmap, None          # (a candidate pass hands on no messages)
        r = band.refine_band(vol, out.disparities[l], unary_weight, start, kernel, out.tol[l], bands[l], maxiter[l],
                             max_relgap, alphas=alphas, layout=layout, conn=conn,
                             carry=carry != "none", carry_start=(stage, True) if carry == "scales" else None)
        stage = r.stage
        results.append(r)
        for name in ("maps", "labels", "energy", "carried", "lower_bound", "iterations", "paths"):
            getattr(out, name)[l] = [v for x in results for v in getattr(x, name)]
        current = r.dispmap
    out.dispmap = current
    return out


# ---------------------------------------------------------------- one view, planes carried and fitted

class ViewPlanePyramidResult(ViewPyramidResult):
    """solve_view_ncc_plane_pyramid's result: `planes` (4 x N, level 0's last plane map), `dispmap` (their disparities at
    their own pixels, H x W) and per level l, index l: `plane_maps` (4 x N_l per pass; at the coarsest level the one
    fronto-parallel map of its solve), `expanded` (4 x N_l) / `expand_source` (None at the coarsest level), `labels`,
    `energy`, `lower_bound`, `iterations`, `paths`, `carried` (lists per pass, candidate passes before bands),
    `disparities`, `tol`, `smooth_weight`; `unary` and `times["volumes"]` as in ViewPyramidResult."""

    def __init__(self, n):
        super().__init__(n)
        self.planes, self.plane_maps = None, self.maps


def plane_disparities(planes, shape):
    """4 x N planes -> H x W: every plane's disparity at its own pixel, -((a X + b Y) + d) / c at the 1-based point."""
    H, W = (int(v) for v in shape)
    p = np.asarray(planes, dtype=np.float64)
    X, Y = np.repeat(np.arange(1.0, W + 1), H), np.tile(np.arange(1.0, H + 1), W)
    with np.errstate(all="ignore"):
        return (-((p[0] * X + p[1] * Y) + p[3]) / p[2]).reshape(W, H).T


def check_plane_propagate(propagate, levels):
    """`propagate` of a plane pyramid solve -> per level 0 .. levels - 1 a list of plane-candidate levels as the caller
    wrote them, each checked (plane_candidates.check_level) with 'wta' standing for a source that is made when the level
    runs; None stays None."""
    if propagate is None:
        return None
    from . import plane_candidates
    try:
        n = len(propagate)
    except TypeError:
        n = -1
    if n != levels or isinstance(propagate, (dict, str)):
        raise StereoHipError("pyramid: propagate must hold one sequence of plane-candidate levels per level 0 .. levels - 1 "
                             "(%d, got %d)" % (levels, n))
    checked = []
    for l, passes in enumerate(propagate):
        if passes is None:
            passes = []
        if isinstance(passes, dict):
            passes = [passes]
        try:
            passes = list(passes)
        except TypeError:
            raise StereoHipError("pyramid: propagate[%d] must be a sequence of plane-candidate levels" % l)
        for c in passes:
            plane_candidates.check_level(_with_wta(c, "base"))
        checked.append(passes)
    return checked


def _with_wta(level, wta):
    """A plane-candidate level as the caller wrote it, its 'wta' sources replaced by `wta`."""
    if not isinstance(level, dict) or "sources" not in level:
        return level
    from . import plane_candidates
    sources = level["sources"]
    if isinstance(sources, (str, np.ndarray, plane_candidates.OrOwn, plane_candidates.Fit)):
        sources = [sources]
    return dict(level, sources=[wta if isinstance(s, str) and s == "wta" else s for s in sources])


def solve_view_ncc_plane_pyramid(images, disparities, kernel, unary_weight, tol, levels, maxiter, max_relgap, bands=None,
                                 expand="guided", carry="none", unary="images", volume=None, propagate=None):
    """One view, coarse to fine, as PLANES.  The reduction, the level model, the levels' volumes (unary,
    volume) and the coarsest solve are solve_view_ncc_pyramid's; the coarsest map becomes plane_candidates.fronto(map).
    Each finer level l then runs, in order: expand_planes_device with the view's images of the two scales (`expand`);
    the plane-candidate levels of propagate[l] (plane_candidates.refine_plane_candidates on an NccSource of the level's
    volume; a level's sources are 'base', plane_candidates.Fit(...), 'wta' -- the level volume's winner-take-all map as
    OrOwn(fronto(...)) -- and 4 x N_l arrays); the plane bands bands[l] (plane_band.refine_plane_band), with tol_l and
    the edge weight s^(k - 1); offsets are in the level's disparity units.  carry: 'none', or 'levels' for
    refine_plane_band(carry=True) within a scale; 'scales' is refused (messages have no meaning across a plane
    expansion yet).  propagate=None runs no candidate pass.  -> ViewPlanePyramidResult."""
    from . import plane_band, plane_candidates
    levels, maxiter, bands, mode = check_plan(levels, maxiter, bands, expand)
    propagate = check_plane_propagate(propagate, levels)
    if check_carry(carry) == "scales":
        raise StereoHipError("plane pyramid: carry must be 'none' or 'levels'; 'scales' is not defined here (messages have "
                             "no meaning across a plane expansion yet)")
    unary = check_unary(unary)
    _check_volume_argument(volume, unary)
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    level_model(kernel, tol, 0)
    _lib.require_device()
    import torch
    out = ViewPlanePyramidResult(levels + 1)
    host, dev, layout, level_volume = _view_setup(out, images, disparities, kernel, tol, levels, unary, volume)
    current, _ = _solve_coarsest(out, host, level_volume, layout, kernel, unary_weight, maxiter, max_relgap, False)
    planes = plane_candidates.fronto(current)
    out.plane_maps[levels].append(planes)
    for l in range(levels - 1, -1, -1):
        H, W = host[l][0].shape[:2]
        d_coarse = torch.from_numpy(np.array(planes.T, order="C")).cuda()              # (Nc, 4): 4 x Nc column major
        d_fine, d_source = expand_planes_device(d_coarse, (H, W), mode, dev[l][0], dev[l + 1][0])
        planes = np.asfortranarray(d_fine.cpu().numpy().T)
        out.expanded[l], out.expand_source[l] = planes, d_source.cpu().numpy().T
        conn = T.construct_neighborhood(H, W)
        vol, alphas = level_volume(l), np.ones(conn.shape[1]) * out.smooth_weight[l]
        source = plane_band.NccSource(vol, out.disparities[l], unary_weight, layout, (H, W))
        results = []
        if propagate is not None and propagate[l]:
            wta = None
            if any(s is None for c in propagate[l] if isinstance(c, dict) for s in _with_wta(c, None).get("sources", ())):
                wta = plane_candidates.OrOwn(plane_candidates.fronto(T.ncc_best_disp(vol, out.disparities[l], layout, (H, W))))
            results.append(plane_candidates.refine_plane_candidates(source, planes, kernel, out.tol[l],
                                                                    [_with_wta(c, wta) for c in propagate[l]], maxiter[l],
                                                                    max_relgap, alphas=alphas, conn=conn))
            planes = results[0].planes
        results.append(plane_band.refine_plane_band(source, planes, kernel, out.tol[l], bands[l], maxiter[l], max_relgap,
                                                    alphas=alphas, conn=conn, carry=carry == "levels"))
        planes = results[-1].planes
        for name in ("maps", "labels", "energy", "carried", "lower_bound", "iterations", "paths"):
            getattr(out, name)[l] = [v for x in results for v in getattr(x, name)]
    out.planes = planes
    out.dispmap = plane_disparities(planes, host[0][0].shape[:2])
    return out
