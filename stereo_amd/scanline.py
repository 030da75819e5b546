"""Scanline aggregation (no reference counterpart; the definition: include/stereo_hip.h): the exact
min-sum dynamic programme of the model's own pairwise term along the scanlines of up to 8 directions, summed into a
D x N volume, and the labels, map and confidence the sum gives; ``model_energy``, the energy of any labelling under the
model TRW-S minimises; and ``solve_pair_ncc_scanline``, both views of a pair from the aggregation, cross-checked, with
optional candidate and band levels around the scanline maps.  ``aggregate_weighted`` takes a weight per
pixel and direction in the place of one weight per direction; contrast.step_weights makes such weights from an image.

A volume is D x N, label fastest (layout 1), N = H * W, pixel id = col * H + row.  A direction is (dy, dx): the
predecessor of pixel (y, x) is (y - dy, x - dx).  Host forms take NumPy arrays; device forms take torch tensors of the
current device: a volume as a flat contiguous float64 tensor of D * N elements, a map as a contiguous (W, H) tensor, as
consistency.lr_check_device takes it.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from . import band
from . import consistency
from . import terms as T
from ._lib import StereoHipError
from .consistency import _device_map, _p, _stream

DIRECTIONS_4 = ((0, 1), (0, -1), (1, 0), (-1, 0))
DIRECTIONS_8 = DIRECTIONS_4 + ((1, 1), (-1, -1), (1, -1), (-1, 1))


def max_labels():
    """The largest D (stereo_scanline_max_labels)."""
    return int(_lib.lib().stereo_scanline_max_labels())


class ScanlineResult:
    """`labels` (N, int32, one based), `dispmap` and `confidence` (H x W), `volume` (D x N, the summed costs S, or None).
    From aggregate_device the four are tensors: N int32, (W, H), (W, H), flat D * N."""

    def __init__(self, labels, dispmap, confidence, volume):
        self.labels, self.dispmap, self.confidence, self.volume = labels, dispmap, confidence, volume


def _directions(directions, weights):
    """-> (2 R int32 array of (dy, dx) pairs, R float64 weights); the library checks the values."""
    try:
        d = np.array([[int(v) for v in pair] for pair in directions], dtype=np.int32).reshape(-1, 2)
    except (TypeError, ValueError):
        raise StereoHipError("scanline: directions must be a sequence of (dy, dx) pairs")
    R = d.shape[0]
    w = np.ones(R) if weights is None else np.array(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != R:
        raise StereoHipError("scanline: %d weights for %d directions" % (w.shape[0], R))
    return np.ascontiguousarray(d.reshape(-1)), np.ascontiguousarray(w)


def _shape(shape):
    H, W = (int(v) for v in shape)
    return H, W


def aggregate(unary, shape, positions, kernel, tol, directions=DIRECTIONS_8, weights=None, want_volume=False):
    """stereo_scanline_aggregate: `unary` D x N (label fastest) of `shape` = (H, W) pixels, `positions` the D label
    positions, kernel 1 / 2 and `tol` the model's truncated linear / quadratic term, one weight per direction (default 1).
    -> ScanlineResult on the host (`volume` only with want_volume)."""
    H, W = _shape(shape)
    unary = np.asarray(unary, dtype=np.float64)
    positions = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1))
    D = positions.shape[0]
    if unary.ndim != 2 or unary.shape != (D, max(H, 0) * max(W, 0)):
        raise StereoHipError("scanline: unary must be D x N = %d x %d (got %s)" % (D, max(H, 0) * max(W, 0), unary.shape))
    unary = np.asfortranarray(unary)
    d, w = _directions(directions, weights)
    n = max(H * W, 1)
    labels = np.zeros(n, np.int32)
    dispmap, conf = np.zeros((max(H, 0), max(W, 0)), order="F"), np.zeros((max(H, 0), max(W, 0)), order="F")
    volume = np.zeros((D, H * W), order="F") if want_volume and H > 0 and W > 0 else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_aggregate(_p(unary), C.c_int(H), C.c_int(W), C.c_int(D), _p(positions), C.c_int(int(kernel)),
                                              C.c_double(float(tol)), _p(d, C.c_int32), _p(w), C.c_int(w.shape[0]),
                                              _p(volume), _p(labels, C.c_int32), _p(dispmap), _p(conf), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels[:H * W], dispmap, conf, volume)


def aggregate_device(unary, shape, positions, kernel, tol, directions=DIRECTIONS_8, weights=None, volume=None, labels=None,
                     dispmap=None, confidence=None, stream=None, d_positions=None):
    """stereo_scanline_aggregate_device on torch tensors of the current device, launched on `stream` (a torch stream or a
    raw handle; default: torch's current stream) without waiting for it.  `unary`: a flat float64 tensor of D * N
    elements, which must be finite.  `positions` is a host vector; `d_positions` its device copy, made here when not given
    (as band.band_inputs_device takes its short vectors).  `volume` (flat, D * N: the workspace and the summed costs),
    `labels` (N int32), `dispmap` and `confidence` ((W, H) maps): tensors to write into; made here otherwise.
    -> ScanlineResult of tensors."""
    import torch
    H, W = _shape(shape)
    positions = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1))
    D = positions.shape[0]
    N = max(H, 0) * max(W, 0)
    unary = band._flat(unary, "unary", torch.float64, D * N)
    d, w = _directions(directions, weights)
    (d_positions,) = band._device_vectors(stream, (positions, d_positions, "d_positions"))
    volume = band._out(volume, "volume", D * N, unary.device)
    labels = torch.empty(N, dtype=torch.int32, device=unary.device) if labels is None else band._flat(labels, "labels", torch.int32, N)
    dispmap = torch.empty((W, H), dtype=torch.float64, device=unary.device) if dispmap is None else _device_map(dispmap, "dispmap", np.float64, (W, H))
    confidence = torch.empty((W, H), dtype=torch.float64, device=unary.device) if confidence is None else _device_map(confidence, "confidence", np.float64, (W, H))
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_aggregate_device(band._vp(unary), C.c_int(H), C.c_int(W), C.c_int(D), band._vp(d_positions),
                                                     C.c_int(int(kernel)), C.c_double(float(tol)), _p(d, C.c_int32), _p(w),
                                                     C.c_int(w.shape[0]), band._vp(volume), band._vp(labels), band._vp(dispmap),
                                                     band._vp(confidence), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels, dispmap, confidence, volume)


def aggregate_weighted(unary, shape, positions, kernel, tol, step_weights, directions=DIRECTIONS_8, want_volume=False):
    """stereo_scanline_aggregate_weighted: aggregate with `step_weights` (R x N, finite and >= 0: row r
    holds per pixel the weight of the step into it along directions[r]; contrast.step_weights makes them from an
    image) in the place of one weight per direction.  -> ScanlineResult on the host (`volume` only with want_volume)."""
    H, W = _shape(shape)
    unary = np.asarray(unary, dtype=np.float64)
    positions = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1))
    D = positions.shape[0]
    N = max(H, 0) * max(W, 0)
    if unary.ndim != 2 or unary.shape != (D, N):
        raise StereoHipError("scanline: unary must be D x N = %d x %d (got %s)" % (D, N, unary.shape))
    unary = np.asfortranarray(unary)
    d, R = _directions_edges(directions)
    wstep = np.asarray(step_weights, dtype=np.float64)
    if wstep.shape != (R, N):
        raise StereoHipError("scanline: step_weights must be R x N = %d x %d (got %s)" % (R, N, wstep.shape))
    wstep = np.ascontiguousarray(wstep)
    labels = np.zeros(max(N, 1), np.int32)
    dispmap, conf = np.zeros((max(H, 0), max(W, 0)), order="F"), np.zeros((max(H, 0), max(W, 0)), order="F")
    volume = np.zeros((D, N), order="F") if want_volume and N > 0 else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_aggregate_weighted(_p(unary), C.c_int(H), C.c_int(W), C.c_int(D), _p(positions),
                                                       C.c_int(int(kernel)), C.c_double(float(tol)), _p(d, C.c_int32), _p(wstep),
                                                       C.c_int(R), _p(volume), _p(labels, C.c_int32), _p(dispmap), _p(conf), err,
                                                       C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels[:N], dispmap, conf, volume)


def aggregate_weighted_device(unary, shape, positions, kernel, tol, step_weights, directions=DIRECTIONS_8, volume=None,
                              labels=None, dispmap=None, confidence=None, stream=None, d_positions=None):
    """stereo_scanline_aggregate_weighted_device: aggregate_device with `step_weights`, a flat float64 tensor of R * N
    elements (element (r, p) at p + N * r, as contrast.step_weights_device writes it), in the place of `weights`.
    -> ScanlineResult of tensors."""
    import torch
    H, W = _shape(shape)
    positions = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).reshape(-1))
    D = positions.shape[0]
    N = max(H, 0) * max(W, 0)
    unary = band._flat(unary, "unary", torch.float64, D * N)
    d, R = _directions_edges(directions)
    step_weights = band._flat(step_weights, "step_weights", torch.float64, R * N)
    (d_positions,) = band._device_vectors(stream, (positions, d_positions, "d_positions"))
    volume = band._out(volume, "volume", D * N, unary.device)
    labels = torch.empty(N, dtype=torch.int32, device=unary.device) if labels is None else band._flat(labels, "labels", torch.int32, N)
    dispmap = torch.empty((W, H), dtype=torch.float64, device=unary.device) if dispmap is None else _device_map(dispmap, "dispmap", np.float64, (W, H))
    confidence = torch.empty((W, H), dtype=torch.float64, device=unary.device) if confidence is None else _device_map(confidence, "confidence", np.float64, (W, H))
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_aggregate_weighted_device(band._vp(unary), C.c_int(H), C.c_int(W), C.c_int(D),
                                                              band._vp(d_positions), C.c_int(int(kernel)), C.c_double(float(tol)),
                                                              _p(d, C.c_int32), band._vp(step_weights), C.c_int(R),
                                                              band._vp(volume), band._vp(labels), band._vp(dispmap),
                                                              band._vp(confidence), C.c_void_p(_stream(stream)), err,
                                                              C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels, dispmap, confidence, volume)


def model_energy(unary, conn, alphas, positions, kernel, tol, labels):
    """The energy of the labelling `labels` (N, ONE based) under the model the header documents, on shared positions:
    sum_i unary[labels_i, i] + sum_e alphas_e * min(v(|pos[labels_a] - pos[labels_b]|), tol) over the edges e = (a, b) of
    `conn` (2 x E, zero based), v(d) = d (kernel 1) or d * d (kernel 2).  NumPy on the host, N + E terms: the currency of
    a TRW-S result for a map that did not come from TRW-S."""
    if int(kernel) not in (1, 2):
        raise StereoHipError("model_energy: kernel must be 1 or 2 (got %r)" % (kernel,))
    unary = np.asarray(unary, dtype=np.float64)
    conn = np.asarray(conn).astype(np.int64)
    positions = np.asarray(positions, dtype=np.float64).reshape(-1)
    x = np.asarray(labels).reshape(-1).astype(np.int64) - 1
    D, N = unary.shape
    if conn.ndim != 2 or conn.shape[0] != 2 or positions.shape[0] != D or x.shape[0] != N:
        raise StereoHipError("model_energy: unary D x N, conn 2 x E, D positions and N labels")
    if x.size and (x.min() < 0 or x.max() >= D):
        raise StereoHipError("model_energy: labels must be 1 .. %d" % D)
    alphas = np.broadcast_to(np.asarray(alphas, dtype=np.float64).reshape(-1), (conn.shape[1],))
    d = np.abs(positions[x[conn[0]]] - positions[x[conn[1]]])
    pair = alphas * np.minimum(d if int(kernel) == 1 else d * d, float(tol))
    return float(unary[x, np.arange(N)].sum() + pair.sum())


# ---------------------------------------------------------------- per-edge positions

def edges_max_labels():
    """The largest K of the per-edge form (stereo_scanline_edges_max_labels)."""
    return int(_lib.lib().stereo_scanline_edges_max_labels())


def _directions_edges(directions):
    try:
        d = np.array([[int(v) for v in pair] for pair in directions], dtype=np.int32).reshape(-1, 2)
    except (TypeError, ValueError):
        raise StereoHipError("scanline: directions must be a sequence of (dy, dx) pairs")
    return np.ascontiguousarray(d.reshape(-1)), d.shape[0]


def _counter(bad, dev, stream):
    """band._bad; a counter made here is zeroed on torch's current stream, which has to be done before another
    `stream` touches it."""
    import torch
    made = bad is None
    bad = band._bad(bad, dev)
    if made and stream is not None:
        torch.cuda.current_stream().synchronize()
    return bad


def edge_table(conn, shape):
    """stereo_scanline_edges_table on the host (no device needed): `conn` 2 x E zero based on the H x W grid `shape`
    -> the 4 N int32 table the header documents.  An edge the grid does not have is refused, named."""
    H, W = _shape(shape)
    conn = band._conn(conn)
    table = np.zeros(4 * max(H, 0) * max(W, 0), np.int32)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_table(_p(conn, C.c_uint32), C.c_int64(conn.shape[1]), C.c_int(H), C.c_int(W),
                                                _p(table, C.c_int32), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return table


def edge_table_device(d_conn, E, shape, table=None, bad=None, stream=None, check=True):
    """stereo_scanline_edges_table_device: `d_conn` a flat int32 tensor of 2 E entries (as the level builders keep it).
    check=True reads the count of invalid edges back (this waits for the stream) and raises; the host form names them.
    -> (table: 4 N int32 tensor, bad)."""
    import torch
    H, W = _shape(shape)
    N = max(H, 0) * max(W, 0)
    d_conn = band._flat(d_conn, "conn", torch.int32, 2 * int(E))
    table = torch.empty(4 * N, dtype=torch.int32, device=d_conn.device) if table is None else band._flat(table, "table", torch.int32, 4 * N)
    bad = _counter(bad, d_conn.device, stream)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_table_device(band._vp(d_conn), C.c_int64(int(E)), C.c_int(H), C.c_int(W), band._vp(table),
                                                       band._vp(bad), C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    band._raise_bad(bad, check, "edge_table_device: %d edge(s) that the %d x %d grid does not have, or has already "
                    "(scanline.edge_table names the first)", H, W)
    return table, bad


def aggregate_edges(unary, shape, conn, q, qprim, alphas, kernel, tol, directions=DIRECTIONS_4, want_volume=False):
    """stereo_scanline_edges_aggregate: `unary` K x N (label fastest) of `shape` = (H, W) pixels, `conn` 2 x E zero
    based, `q` / `qprim` K x E, `alphas` E weights, kernel 1 / 2 and `tol` the model's truncated term.
    -> ScanlineResult on the host with dispmap None (`volume` only with want_volume)."""
    H, W = _shape(shape)
    unary = np.asarray(unary, dtype=np.float64)
    N = max(H, 0) * max(W, 0)
    if unary.ndim != 2 or unary.shape[1] != N:
        raise StereoHipError("scanline: unary must be K x N = K x %d (got %s)" % (N, unary.shape))
    K = unary.shape[0]
    conn = band._conn(conn)
    E = conn.shape[1]
    q, qprim = np.asarray(q, dtype=np.float64), np.asarray(qprim, dtype=np.float64)
    alphas = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).reshape(-1))
    if q.shape != (K, E) or qprim.shape != (K, E) or alphas.shape[0] != E:
        raise StereoHipError("scanline: q and qprim must be K x E = %d x %d and alphas E values" % (K, E))
    unary, q, qprim = np.asfortranarray(unary), np.asfortranarray(q), np.asfortranarray(qprim)
    d, R = _directions_edges(directions)
    labels = np.zeros(max(N, 1), np.int32)
    conf = np.zeros((max(H, 0), max(W, 0)), order="F")
    volume = np.zeros((K, N), order="F") if want_volume and N > 0 else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_aggregate(C.c_int(int(kernel)), _p(unary), C.c_int(H), C.c_int(W), C.c_int(K), C.c_int64(E),
                                                    _p(conn, C.c_uint32), _p(q), _p(qprim), _p(alphas), C.c_double(float(tol)),
                                                    _p(d, C.c_int32), C.c_int(R), _p(volume), _p(labels, C.c_int32), _p(conf), err,
                                                    C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels[:N], None, conf, volume)


def aggregate_edges_device(unary, shape, table, q, qprim, alphas, kernel, tol, directions=DIRECTIONS_4, volume=None, labels=None,
                           confidence=None, stream=None):
    """stereo_scanline_edges_aggregate_device on torch tensors of the current device, launched on `stream` (a torch
    stream or a raw handle; default: torch's current stream) without waiting for it.  `unary`: flat float64, K * N;
    `table`: edge_table_device's; `q`, `qprim`: flat, K * E; `alphas`: E (E is its length, K = unary's length / N).
    `volume` (flat K * N: the workspace and the summed costs), `labels` (N int32) and `confidence` ((W, H)): tensors to
    write into; made here otherwise.  -> ScanlineResult of tensors, dispmap None."""
    import torch
    H, W = _shape(shape)
    N = max(H, 0) * max(W, 0)
    unary = band._flat(unary, "unary", torch.float64)
    if N < 1 or unary.numel() % N or unary.numel() < N:
        raise StereoHipError("scanline: unary must hold K * N = K * %d elements (got %d)" % (N, unary.numel()))
    K = unary.numel() // N
    alphas = band._flat(alphas, "alphas", torch.float64)
    E = alphas.numel()
    table = band._flat(table, "table", torch.int32, 4 * N)
    q, qprim = band._flat(q, "q", torch.float64, K * E), band._flat(qprim, "qprim", torch.float64, K * E)
    d, R = _directions_edges(directions)
    volume = band._out(volume, "volume", K * N, unary.device)
    labels = torch.empty(N, dtype=torch.int32, device=unary.device) if labels is None else band._flat(labels, "labels", torch.int32, N)
    confidence = torch.empty((W, H), dtype=torch.float64, device=unary.device) if confidence is None else _device_map(confidence, "confidence", np.float64, (W, H))
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_aggregate_device(C.c_int(int(kernel)), band._vp(unary), C.c_int(H), C.c_int(W), C.c_int(K),
                                                           C.c_int64(E), band._vp(table), band._vp(q), band._vp(qprim), band._vp(alphas),
                                                           C.c_double(float(tol)), _p(d, C.c_int32), C.c_int(R), band._vp(volume),
                                                           band._vp(labels), band._vp(confidence), C.c_void_p(_stream(stream)), err,
                                                           C.c_size_t(len(err)))
    _lib.check(rc, err)
    return ScanlineResult(labels, None, confidence, volume)


def model_energy_edges(unary, conn, q, qprim, alphas, kernel, tol, labels, want_terms=False):
    """The energy of the labelling `labels` (N, ONE based) under the general model the header documents:
    sum_i unary[labels_i, i] + sum_e alphas_e * min(v(|qprim[labels_a, e] - q[labels_b, e]|), tol) over the edges
    e = (a, b) of `conn` (2 x E, zero based); `unary` K x N, `q` / `qprim` K x E.  NumPy on the host: the general-model
    sibling of model_energy.  want_terms: -> (energy, the N + E terms, each with the definition's operations)."""
    if int(kernel) not in (1, 2):
        raise StereoHipError("model_energy_edges: kernel must be 1 or 2 (got %r)" % (kernel,))
    unary = np.asarray(unary, dtype=np.float64)
    conn = np.asarray(conn).astype(np.int64)
    q, qprim = np.asarray(q, dtype=np.float64), np.asarray(qprim, dtype=np.float64)
    x = np.asarray(labels).reshape(-1).astype(np.int64) - 1
    if unary.ndim != 2 or conn.ndim != 2 or conn.shape[0] != 2:
        raise StereoHipError("model_energy_edges: unary K x N, conn 2 x E, q and qprim K x E, E alphas and N labels")
    K, N = unary.shape
    E = conn.shape[1]
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1)
    if q.shape != (K, E) or qprim.shape != (K, E) or alphas.shape[0] != E or x.shape[0] != N:
        raise StereoHipError("model_energy_edges: unary K x N, conn 2 x E, q and qprim K x E, E alphas and N labels")
    if x.size and (x.min() < 0 or x.max() >= K):
        raise StereoHipError("model_energy_edges: labels must be 1 .. %d" % K)
    if conn.size and (conn.min() < 0 or conn.max() >= N):
        raise StereoHipError("model_energy_edges: conn must be 0 .. %d" % (N - 1))
    e = np.arange(E)
    d = np.abs(qprim[x[conn[0]], e] - q[x[conn[1]], e])
    with np.errstate(over="ignore"):
        pair = alphas * np.minimum(d if int(kernel) == 1 else d * d, float(tol))
    terms = np.concatenate([unary[x, np.arange(N)], pair])
    energy = float(terms[:N].sum() + pair.sum())
    return (energy, terms) if want_terms else energy


def level_energy_device(unary, conn, q, qprim, alphas, kernel, tol, labels, terms=None, bad=None, stream=None, check=True):
    """stereo_scanline_edges_energy_device: the N + E terms of the labelling `labels` (N int32 tensor, one based) under
    the inputs of a level -- flat tensors `unary` K * N, `conn` 2 E int32, `q` / `qprim` K * E, `alphas` E -- written on
    the device and summed on the host (this waits for the stream).  check=True raises for a label outside 1 .. K.
    -> (energy, terms: N + E float64 tensor)."""
    import torch
    labels = band._flat(labels, "labels", torch.int32)
    N = labels.numel()
    unary = band._flat(unary, "unary", torch.float64)
    if N < 1 or unary.numel() % N or unary.numel() < N:
        raise StereoHipError("level_energy_device: unary must hold K * N = K * %d elements (got %d)" % (N, unary.numel()))
    K = unary.numel() // N
    conn, E = band._edges(conn)
    alphas = band._flat(alphas, "alphas", torch.float64, E)
    q, qprim = band._flat(q, "q", torch.float64, K * E), band._flat(qprim, "qprim", torch.float64, K * E)
    terms = band._out(terms, "terms", N + E, unary.device)
    bad = _counter(bad, unary.device, stream)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_energy_device(C.c_int(int(kernel)), band._vp(unary), C.c_int(K), C.c_int64(N), C.c_int64(E),
                                                        band._vp(conn), band._vp(q), band._vp(qprim), band._vp(alphas),
                                                        C.c_double(float(tol)), band._vp(labels), band._vp(terms), band._vp(bad),
                                                        C.c_void_p(_stream(stream)), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    if stream is not None:
        stream.synchronize() if hasattr(stream, "synchronize") else torch.cuda.ExternalStream(int(stream)).synchronize()
    host = terms.cpu().numpy()
    band._raise_bad(bad, check, "level_energy_device: %d label(s) outside 1 .. %d", K)
    return float(host[:N].sum() + host[N:].sum()), terms


class ScanlineLevel:
    """One level solved by scanline aggregation, with the three things the level loops read from a TrwsPlan:
    result() -> (labels, energy, NaN, 0), path() -> 0.  `problem_table` keeps a problem's edge table."""

    def __init__(self, labels, energy):
        self.labels, self.energy = labels, energy

    def result(self):
        return self.labels, self.energy, float("nan"), 0

    def path(self):
        return 0


def problem_shape(prob):
    """(H, W) of a level problem (band / candidates keep H and W, the plane problems their source)."""
    return (prob.H, prob.W) if hasattr(prob, "H") else (prob.source.H, prob.source.W)


def problem_table(prob):
    """The edge table of a level problem's `d_conn`, built once and kept on the problem.  A `conn` that is not the
    image grid's is refused with the host table's message."""
    if getattr(prob, "d_edge_table", None) is None:
        shape = problem_shape(prob)
        table, bad = edge_table_device(prob.d_conn, prob.E, shape, check=False)
        if int(bad.item()):
            edge_table(prob.conn, shape)        # (raises, naming the edge)
            raise StereoHipError("scanline: the problem's conn is not a grid's")
        prob.d_edge_table = table
    return prob.d_edge_table


def solve_level(prob, level, kernel, tol, zero_columns=None):
    """One level of `prob` (the protocol of band.run_levels) solved by aggregation over DIRECTIONS_4 on torch's current
    stream: build(plan=None), aggregate_edges_device on what it left, the level's model energy from the terms kernel.
    -> ScanlineLevel (labels on the host, N int32 one based)."""
    K = prob.labels_of(level)
    if K > edges_max_labels():
        raise StereoHipError("solver='scanline': a level of %d labels (at most %d)" % (K, edges_max_labels()))
    table = problem_table(prob)
    if zero_columns is None:
        prob.build(level, None, tol)
    else:
        prob.build(level, None, tol, zero_columns=zero_columns)
    r = aggregate_edges_device(prob.d_unary, problem_shape(prob), table, prob.d_q, prob.d_qprim, prob.d_alphas, kernel, tol)
    energy, _ = level_energy_device(prob.d_unary, prob.d_conn, prob.d_q, prob.d_qprim, prob.d_alphas, kernel, tol, r.labels)
    return ScanlineLevel(r.labels.cpu().numpy(), energy)


def solve_pair_ncc_scanline(images, disparities, kernel, unary_weight, tol, check_tol=1.0, directions=DIRECTIONS_8,
                            smooth_weight=None, candidate_levels=None, band_levels=None, maxiter=30, max_relgap=0.0,
                            volumes=None, level_solver="trws", contrast=None, post_filter=None):
    """Both views of a rectified pair without a full-range solve.  In this order: the two NCC volumes
    (consistency.pair_volumes, or `volumes`); each view's unary_weight * (1 - ncc) aggregated on the device along
    `directions`, every direction weighing `smooth_weight` (default 1); the two maps checked against each other with
    check_tol and filled.  That first pass has energy = model_energy of the scanline labels on the image grid with every edge weighing
    smooth_weight, lower_bound NaN, iterations 0 and path 0.  Then the optional candidate levels and the
    optional band levels around the scanline map, both views as a two-member TrwsBatch per level with up
    to `maxiter` iterations (consistency.run_band_levels, as solve_pair_ncc_pyramid runs them around an expanded map).
    level_solver="scanline": both kinds of level are solved by aggregation on their own inputs, not by TRW-S
    (aggregate_edges_device).
    contrast: a contrast.Contrast in the place of smooth_weight -- giving both is refused.  Each view's
    step weights (contrast.step_weights_device) and edge weights (contrast.edge_weights_device on the image grid) come
    from that view's own image, in the columns its unary is in; the aggregation is aggregate_weighted_device, and
    model_energy and the candidate and band levels, with either level_solver, get that view's edge weights as alphas.
    post_filter: a mapfilter.MedianFilter: after every check and fill, candidate and band levels
    included, each view's `filled` map filtered into `filtered` / `filter_source`, as in consistency.solve_pair_ncc.
    -> consistency.PairResult."""
    import torch
    from . import candidates
    from . import contrast as contrast_mod
    disparities = np.asarray(disparities, dtype=np.float64).reshape(-1)
    if len(images) != 2:
        raise StereoHipError("solve_pair_ncc_scanline: images must be the two views of a pair, left first (got %d)" % len(images))
    shapes = [np.shape(im) for im in images]
    if shapes[0] != shapes[1] or len(shapes[0]) != 3 or shapes[0][2] != 3:
        raise StereoHipError("solve_pair_ncc_scanline: the two images must be H x W x 3 arrays of one size (got %s and %s)" % tuple(shapes))
    if disparities.size < 1:
        raise StereoHipError("solve_pair_ncc_scanline: no disparities")
    H, W = shapes[0][:2]
    K, N = disparities.shape[0], H * W
    if candidate_levels is not None:
        candidate_levels = candidates.check_levels(candidate_levels)
    if band_levels is not None:
        band_levels = band.check_levels(band_levels)
    band.check_solver(level_solver)
    directions = [tuple(d) for d in directions]
    if contrast is not None and smooth_weight is not None:
        raise StereoHipError("solve_pair_ncc_scanline: smooth_weight or contrast, not both")
    smooth_weight = 1.0 if smooth_weight is None else float(smooth_weight)
    weights = [smooth_weight] * len(directions)
    _lib.require_device()
    out = consistency.PairResult()
    clock = time.perf_counter
    t0 = clock()
    if volumes is None:
        volumes = consistency.pair_volumes(images, disparities)
    else:
        volumes = [np.asarray(v, dtype=np.float64) for v in volumes]
        if len(volumes) != 2 or any(v.shape != (K, N) for v in volumes):
            raise StereoHipError("solve_pair_ncc_scanline: volumes must be the two D x N volumes of the pair (%d x %d)" % (K, N))
    unaries = consistency.pair_unaries(images, disparities, unary_weight, volumes)
    out.times["volumes"] = clock() - t0
    conn = T.construct_neighborhood(H, W)
    alphas = [np.ones(conn.shape[1]) * smooth_weight] * 2          # per view

    t0 = clock()
    d_positions = band.to_device_vector(disparities)
    if contrast is not None:
        d_conn = torch.from_numpy(np.ascontiguousarray(conn.T.reshape(-1), dtype=np.int32)).cuda()
        alphas = []
    for image, view, unary in zip(images, out.views, unaries):
        d_unary = torch.from_numpy(np.asfortranarray(unary).reshape(-1, order="F")).cuda()
        if contrast is None:
            r = aggregate_device(d_unary, (H, W), disparities, kernel, tol, directions, weights, d_positions=d_positions)
        else:
            d_image = contrast_mod.image_to_device(image)
            alphas.append(contrast_mod.edge_weights_device(d_image, np.shape(image), d_conn, contrast)[0].cpu().numpy())
            wstep = contrast_mod.step_weights_device(d_image, np.shape(image), directions, contrast)
            r = aggregate_weighted_device(d_unary, (H, W), disparities, kernel, tol, wstep, directions, d_positions=d_positions)
        view.labels = r.labels.cpu().numpy()
        view.dispmap = r.dispmap.cpu().numpy().T
        view.maps.append(view.dispmap)
    out.times["scanline"] = clock() - t0
    t0 = clock()
    for view, unary, a in zip(out.views, unaries, alphas):
        view.energy.append(model_energy(unary, conn, a, disparities, kernel, tol, view.labels))
        view.lower_bound.append(float("nan")); view.iterations.append(0); view.paths.append(0); view.carried.append(False)
    out.times["energy"] = clock() - t0
    t0 = clock()
    for view, other, direction in ((out.left, out.right, 1), (out.right, out.left, -1)):
        view.status, view.residual = consistency.lr_check(view.dispmap, other.dispmap, direction, check_tol)
        view.filled, view.source = consistency.lr_fill(view.dispmap, view.status)
    consistency.filter_views(out, post_filter, images)
    out.times["check_fill"] = clock() - t0

    band_plans = {}
    try:
        if candidate_levels:
            problems = [candidates.CandidateProblem(vol, disparities, unary_weight, view.dispmap, conn, a, layout=1)
                        for vol, view, a in zip(volumes, out.views, alphas)]
            consistency.run_band_levels(out, problems, candidate_levels, band_plans, kernel, conn, tol, maxiter, max_relgap,
                                        check_tol, name="propagate", solver=level_solver, post_filter=post_filter, images=images)
        if band_levels:
            problems = [band.BandProblem(vol, disparities, unary_weight, view.dispmap, conn, a, layout=1)
                        for vol, view, a in zip(volumes, out.views, alphas)]
            consistency.run_band_levels(out, problems, band_levels, band_plans, kernel, conn, tol, maxiter, max_relgap, check_tol,
                                        solver=level_solver, post_filter=post_filter, images=images)
    finally:
        for plan in (p for pair in band_plans.values() for p in pair):
            plan.close()
    return out
