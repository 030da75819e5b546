"""Candidate bands: per-pixel label sets propagated from neighbours (the definition:
include/stereo_hip.h).

A candidate table ``cand`` (K x N, label fastest, pixels column major) says what label k means at pixel i: a disparity
of its own.  ``gather`` builds one from a map ``base``, the band's ``offsets`` (strictly ascending, containing 0.0), M
source maps and T taps ``(dy, dx)``: rows ``base + offsets_k``, then for every source and tap the source's value at the
clamped neighbour, copied.  ``candidates_inputs`` makes the TRW-S problem of any table -- ``unary`` (K x N) from the NCC
volume by the reference's sampler, ``q`` / ``qprim`` (K x E) as stereo_trws_positions gives them for the planes
``[0 0 1 -cand]`` -- and ``candidates_apply`` reads the map a labelling selects.  ``refine_candidates`` builds these on
the device, solves them level by level and applies the labels.

Host forms take NumPy arrays in MATLAB shapes, device forms torch tensors of the current device, as in band.py: a map is
a contiguous (W, H) tensor, a table a flat float64 tensor of K*N elements, M sources one contiguous (M, W, H) tensor.
The helpers of the wrappers and the level loop are band.py's; the checks of a candidate level (check_level,
check_levels, labels_of) are here for plane_candidates.py as well.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import band
from . import terms as T
from ._lib import StereoHipError
from .band import (_bad, _conn, _device_labels, _device_vectors, _edges, _flat, _labels, _out, _raise_bad, _vec, _volume, _vp,
                   bind_inputs, run_levels, to_device_vector)
from .consistency import _device_map, _map, _p, _stream

SOURCE_NAMES = ("base", "wta")


def _taps(taps):
    """T x 2 int32, rows (dy, dx)."""
    t = np.asarray(taps if taps is not None else [])
    if t.size == 0:
        return np.zeros((0, 2), np.int32)
    if t.ndim != 2 or t.shape[1] != 2:
        raise StereoHipError("taps must be T pairs (dy, dx)")
    if not np.array_equal(t, np.rint(t)):
        raise StereoHipError("taps must be whole numbers")
    if np.abs(t).max() >= 1 << 31:
        raise StereoHipError("taps: |dy| and |dx| must be below 2^15")
    return np.ascontiguousarray(t, dtype=np.int32)


def _sources(sources, shape):
    """M x (H*W) float64, C order: source m in column-major pixel order."""
    maps = [_map(s, "a source") for s in sources]
    for m in maps:
        if m.shape != tuple(shape):
            raise StereoHipError("a source must have the base's size")
    out = np.zeros((len(maps), shape[0] * shape[1]))
    for m, s in enumerate(maps):
        out[m] = s.reshape(-1, order="F")
    return out


def _table(cand, N):
    cand = np.asarray(cand, dtype=np.float64)
    if cand.ndim != 2 or cand.shape[1] != N:
        raise StereoHipError("cand must be K x (H*W)")
    return np.asfortranarray(cand)


def gather(base, offsets, sources=(), taps=()):
    """stereo_candidates_gather -> cand, K x N (Fortran order), K = len(offsets) + len(sources) * len(taps)."""
    base = _map(base, "base")
    H, W = base.shape
    offsets, taps = _vec(offsets, "offsets"), _taps(taps)
    src = _sources(sources, (H, W))
    Ko, M, Tn = offsets.shape[0], src.shape[0], taps.shape[0]
    K = Ko + M * Tn
    cand = np.zeros((max(K, 1), H * W), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_gather(_p(base), C.c_int(H), C.c_int(W), _p(offsets), C.c_int(Ko),
                                             _p(src) if M * Tn else None, C.c_int(M), _p(taps, C.c_int32) if M * Tn else None,
                                             C.c_int(Tn), _p(cand), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return cand


def candidates_inputs(ncc, disparities, unary_weight, cand, shape, conn, layout=0):
    """stereo_candidates_inputs for the table `cand` (K x N) of an image of `shape` = (H, W)
    -> (unary K x N, q K x E, qprim K x E), Fortran order."""
    H, W = (int(v) for v in shape)
    cand = _table(cand, H * W)
    vol, D = _volume(ncc, layout, H, W)
    disparities, conn = _vec(disparities, "disparities"), _conn(conn)
    if disparities.shape[0] != D:
        raise StereoHipError("candidates_inputs: %d disparities for a volume of %d slices" % (disparities.shape[0], D))
    K, E, N = cand.shape[0], conn.shape[1], H * W
    unary = np.zeros((K, N), order="F")
    q, qprim = np.zeros((K, E), order="F"), np.zeros((K, E), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_inputs(_p(vol), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)), _p(disparities),
                                             C.c_double(float(unary_weight)), _p(cand), C.c_int(K), C.c_int64(E),
                                             _p(conn, C.c_uint32), _p(unary), _p(q), _p(qprim), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return unary, q, qprim


def candidates_apply(cand, labels, shape):
    """stereo_candidates_apply -> H x W: cand[labels - 1, pixel].  `labels`: one based, N values as plan.result() returns
    them or H x W."""
    H, W = (int(v) for v in shape)
    cand = _table(cand, H * W)
    lab = _labels(labels, (H, W))
    out = np.zeros((H, W), order="F")
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_apply(_p(cand), C.c_int(H), C.c_int(W), C.c_int(cand.shape[0]), _p(lab, C.c_int32),
                                            _p(out), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return out


# ---------------------------------------------------------------- device forms

def taps_to_device(taps):
    """The taps as the flat int32 tensor of 2 T entries the device forms read as d_taps."""
    import torch
    return torch.from_numpy(np.array(_taps(taps).reshape(-1), dtype=np.int32)).cuda()


def _device_vectors_of_gather(stream, offsets, d_offsets, taps, d_taps, taken):
    """band._device_vectors for a gather: the offsets always, the taps only where a source is read (`taken`)."""
    if not taken:
        return _device_vectors(stream, (offsets, d_offsets, "d_offsets"))[0], d_taps
    return _device_vectors(stream, (offsets, d_offsets, "d_offsets"), (taps, d_taps, "d_taps"))


def gather_device(base, offsets, sources=None, taps=(), cand=None, bad=None, stream=None, d_offsets=None, d_taps=None,
                  check=True):
    """stereo_candidates_gather_device: `base` a (W, H) float64 map tensor, `sources` None or a contiguous (M, W, H)
    tensor, `offsets` and `taps` host arrays (`d_offsets` / `d_taps`: their device copies, made here when not given).
    check=True reads the count of pixels at which the base or a source is not finite back (this waits for the stream)
    and raises; check=False leaves it in `bad`.  -> (cand: flat tensor of K*N elements, bad)."""
    import torch
    base = _device_map(base, "base", np.float64)
    W, H = base.shape
    offsets, taps = _vec(offsets, "offsets"), _taps(taps)
    Ko, Tn, N = offsets.shape[0], taps.shape[0], H * W
    M = 0
    if sources is not None:
        if not isinstance(sources, torch.Tensor) or sources.dim() != 3 or tuple(sources.shape[1:]) != (W, H):
            raise StereoHipError("sources must be a contiguous (M, W, H) float64 tensor on the device")
        M = sources.shape[0]
        sources = _flat(sources, "sources", torch.float64, M * N)
    K = Ko + M * Tn
    dev = base.device
    d_offsets, d_taps = _device_vectors_of_gather(stream, offsets, d_offsets, taps, d_taps, M * Tn)
    cand, bad = _out(cand, "cand", K * N, dev, new=max(K, 1) * N), _bad(bad, dev)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_gather_device(_vp(base), C.c_int(H), C.c_int(W), _p(offsets), _vp(d_offsets), C.c_int(Ko),
                                                    _vp(sources) if M * Tn else None, C.c_int(M),
                                                    _p(taps, C.c_int32) if M * Tn else None, _vp(d_taps) if M * Tn else None,
                                                    C.c_int(Tn), _vp(cand), _vp(bad), C.c_void_p(_stream(stream)), err,
                                                    C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "gather_device: the base or a source is not finite at %d pixel(s)")
    return cand, bad


def candidates_inputs_device(ncc, disparities, unary_weight, cand, shape, conn, layout=0, unary=None, q=None, qprim=None,
                             bad=None, stream=None, d_disparities=None, check=True):
    """stereo_candidates_inputs_device on torch tensors: `cand` a flat float64 tensor of K*N elements for an image of
    `shape` = (H, W); the rest as band.band_inputs_device.  check=True reads the count of pixels with a candidate that
    is not finite back and raises.  -> (unary, q, qprim, bad): flat tensors K*N, K*E, K*E and the int32 counter."""
    import torch
    H, W = (int(v) for v in shape)
    N = H * W
    disparities = _vec(disparities, "disparities")
    D = disparities.shape[0]
    cand = _flat(cand, "cand", torch.float64)
    if N < 1 or cand.numel() % N:
        raise StereoHipError("cand must hold K * H * W elements")
    K = cand.numel() // N
    ncc = _flat(ncc, "ncc", torch.float64, N * D)
    conn, E = _edges(conn)
    dev = cand.device
    d_disparities, = _device_vectors(stream, (disparities, d_disparities, "d_disparities"))
    unary, q, qprim = _out(unary, "unary", K * N, dev), _out(q, "q", K * E, dev), _out(qprim, "qprim", K * E, dev)
    bad = _bad(bad, dev)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_inputs_device(_vp(ncc), C.c_int(H), C.c_int(W), C.c_int(D), C.c_int(int(layout)),
                                                    _p(disparities), _vp(d_disparities), C.c_double(float(unary_weight)), _vp(cand),
                                                    C.c_int(K), C.c_int64(E), _vp(conn), _vp(unary), _vp(q), _vp(qprim), _vp(bad),
                                                    C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "candidates_inputs_device: a candidate is not finite at %d pixel(s)")
    return unary, q, qprim, bad


def candidates_apply_device(cand, labels, shape, out=None, bad=None, stream=None, check=True):
    """stereo_candidates_apply_device: `cand` a flat float64 tensor of K*N elements, `labels` a (W, H) or flat int32
    tensor, one based.  check=True reads the count of labels outside 1 .. K back and raises.  -> (out (W, H), bad)."""
    import torch
    H, W = (int(v) for v in shape)
    N = H * W
    cand = _flat(cand, "cand", torch.float64)
    if N < 1 or cand.numel() % N:
        raise StereoHipError("cand must hold K * H * W elements")
    K = cand.numel() // N
    labels = _flat(labels, "labels", torch.int32, N)
    out = torch.empty((W, H), dtype=torch.float64, device=cand.device) if out is None else _device_map(out, "out", np.float64, (W, H))
    bad = _bad(bad, cand.device)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_candidates_apply_device(_vp(cand), C.c_int(H), C.c_int(W), C.c_int(K), _vp(labels), _vp(out), _vp(bad),
                                                   C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    _raise_bad(bad, check, "candidates_apply_device: %d label(s) outside 1 .. %d", K)
    return out, bad


# ---------------------------------------------------------------- levels

def _check_source(s):
    if isinstance(s, str):
        if s not in SOURCE_NAMES:
            raise StereoHipError("candidates: a source is 'base', 'wta' or an H x W map (got %r)" % (s,))
    elif np.ndim(s) != 2:
        raise StereoHipError("candidates: a source is 'base', 'wta' or an H x W map")


def check_level(level, check_source=_check_source, prefix="candidates", single=(str, np.ndarray)):
    """A candidate level as dict(offsets: float64 vector, taps: T x 2 int32, sources: list of 'base' / 'wta' / H x W
    maps), checked as far as it can be without the image: the band's rules for the offsets, whole-number taps below
    2^15, K = Ko + M T within 1 .. max_offsets().  plane_candidates.py checks its levels here too: check_source refuses
    what is not a source, prefix ("candidates" / "plane candidates") starts the messages, single: the types of one
    source given without a list."""
    if not isinstance(level, dict) or set(level) - {"offsets", "taps", "sources"}:
        raise StereoHipError("a %s level must be dict(offsets=, taps=, sources=) (got %r)" % (prefix[:-1].replace(" ", "-"), level))
    offsets = _vec(level.get("offsets", [0.0]), "a level's offsets")
    if offsets.shape[0] < 1 or not (np.isfinite(offsets).all() and (np.diff(offsets) > 0).all() and (offsets == 0.0).any()):
        raise StereoHipError("%s: a vector of offsets must be finite, strictly ascending and contain 0 (got %s)"
                             % (prefix, offsets.tolist()))
    taps = _taps(level.get("taps", ()))
    if taps.size and np.abs(taps).max() >= 1 << 15:
        raise StereoHipError("%s: a tap's |dy| and |dx| must be below 2^15" % prefix)
    sources = level.get("sources", ())
    sources = [sources] if isinstance(sources, single) else list(sources)
    for s in sources:
        check_source(s)
    K = offsets.shape[0] + len(sources) * taps.shape[0]
    if K > band.max_offsets():
        raise StereoHipError("%s: K = Ko + M * T must be 1 .. %d (got %d)" % (prefix, band.max_offsets(), K))
    return dict(offsets=offsets, taps=taps, sources=sources)


def check_levels(levels, prefix="candidates", **how):
    """`levels` as a list of checked candidate levels (check_level, which takes `prefix` and `how`); at least one."""
    if isinstance(levels, dict):
        levels = [levels]
    levels = [check_level(l, prefix=prefix, **how) for l in levels]
    if not levels:
        raise StereoHipError("refine_%s: levels must hold at least one %s level" % (prefix.replace(" ", "_"), prefix[:-1].replace(" ", "-")))
    return levels


def labels_of(level):
    """K of a checked candidate level, before it is built."""
    return level["offsets"].shape[0] + len(level["sources"]) * level["taps"].shape[0]


class CandidateProblem(band.BandProblem):
    """One view's candidate problems on the device, with BandProblem's interface: the volume, the connectivity and the
    smoothness weights go up once; build() gathers a level's table around the current base, makes its inputs and binds
    them to `plan`; apply() moves the base on.  A candidate level's labels have no common offset grid, so it neither
    takes nor leaves carried messages: stage(), leave() and carry_from() give None."""

    def __init__(self, ncc, disparities, unary_weight, base, conn, alphas=None, layout=0):
        super().__init__(ncc, disparities, unary_weight, base, conn, alphas, layout)
        self.d_cand = self.d_wta = None

    labels_of = staticmethod(labels_of)

    def wta(self):
        """The volume's winner-take-all map (stereo_ncc_best_disp) as a (W, H) tensor, made once.  (Where it is not
        finite -- a volume with NaN slices -- a level takes the pixel's base in its place.)"""
        import torch
        if self.d_wta is None:
            vol = self.d_ncc.cpu().numpy()
            D = self.disparities.shape[0]
            vol = vol.reshape((self.H, self.W, D) if self.layout == 0 else (D, self.N), order="F")
            best = T.ncc_best_disp(vol, self.disparities, self.layout, (self.H, self.W))
            self.d_wta = torch.from_numpy(np.ascontiguousarray(best.T)).cuda()
        return self.d_wta

    def _source_tensor(self, level):
        import torch
        maps = []
        for s in level["sources"]:
            if isinstance(s, str) and s == "base":
                maps.append(self.d_base)
            elif isinstance(s, str):
                w = self.wta()
                maps.append(torch.where(torch.isfinite(w), w, self.d_base))
            else:
                s = _map(s, "a source")
                if s.shape != (self.H, self.W):
                    raise StereoHipError("candidates: a source must have the base's size")
                maps.append(torch.from_numpy(np.ascontiguousarray(s.T)).cuda())
        return torch.stack(maps).contiguous() if maps and level["taps"].shape[0] else None

    def build(self, level, plan=None, tol=0.0, zero_columns=None, carry=None):
        """The inputs of the candidate level `level` (check_level's dict) around the current base, bound to `plan` (None:
        to nothing).
        zero_columns: as in BandProblem.build.  carry must be None."""
        if carry is not None:
            raise StereoHipError("candidates: a candidate level does not take carried messages")
        self.offsets = level["offsets"]
        self.d_offsets = to_device_vector(self.offsets)
        self.d_built_base = self.d_base
        self.d_cand, _ = gather_device(self.d_base, self.offsets, self._source_tensor(level), level["taps"], d_offsets=self.d_offsets)
        self.d_unary, self.d_q, self.d_qprim, _ = candidates_inputs_device(
            self.d_ncc, self.disparities, self.unary_weight, self.d_cand, (self.H, self.W), self.d_conn, self.layout,
            d_disparities=self.d_disparities)
        if zero_columns is not None:
            self.d_unary.view(self.N, -1)[zero_columns] = 0.0
        bind_inputs(self, plan, tol)

    def stage(self, plan):
        return None

    def carry_from(self, stage, scales=False):
        return None

    def apply(self, labels):
        """The map the labels of the level built last select -> the new base on the host, H x W."""
        self.d_base, _ = candidates_apply_device(self.d_cand, _device_labels(labels), (self.H, self.W))
        return self.d_base.cpu().numpy().T


def refine_candidates(ncc, disparities, unary_weight, base, kernel, tol, levels, maxiter, max_relgap, alphas=None, layout=0,
                      conn=None, solver="trws"):
    """Refines the map `base` level by level: for each candidate level in `levels` -- dict(offsets=, taps=, sources=),
    a source being an H x W map, 'base' (the current map) or 'wta' (the volume's ncc_best_disp map, computed once) --
    the table is gathered around the current map on the device, its problem built (stereo_candidates_inputs_device),
    bound to a TrwsPlan(kernel, K, N, conn) -- one plan per distinct K -- iterated up to `maxiter` times and applied;
    the selected map is the next level's base.  Nothing K x N or K x E touches the host.  conn: 2 x E zero based,
    default the image grid.  Every level starts from zero messages.  solver: "trws", or "scanline" -- every level one scanline
    aggregation on its inputs (band.run_levels).  -> band.BandResult (`carried` all False)."""
    band.check_solver(solver)
    levels = check_levels(levels)
    base = _map(base, "base")
    H, W = base.shape
    conn = T.construct_neighborhood(H, W) if conn is None else conn
    prob = CandidateProblem(ncc, disparities, unary_weight, base, conn, alphas, layout)
    out = band.BandResult()
    run_levels(prob, levels, out, kernel, tol, maxiter, max_relgap, solver=solver)
    out.dispmap = out.maps[-1]
    return out
