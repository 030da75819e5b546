"""Messages carried from one band level or pyramid scale to the next (the definition:
include/stereo_hip.h, stereo_band_carry).

A solver state's message rows are ``(E, K)`` float64, label fastest, and row e is a function on the labels of the
edge's RECEIVING node (``receivers``).  ``carry_messages`` reads every old row as a piecewise linear function on the
old level's offset axis and samples it at the new level's offsets, ``shift[r] + stretch * off_new[j]`` for the
receiving node r; ``Carry`` is the record a band problem takes to start from such messages instead of from zero.
"""
import ctypes as C
import hashlib

import numpy as np

from . import _lib
from ._lib import StereoHipError

_receivers_cache = {}


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _vec(a, dtype=np.float64):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1))


def _conn0(conn0):
    c = np.asarray(conn0)
    if c.ndim != 2 or c.shape[0] != 2:
        raise StereoHipError("connectivity must be 2 x E")
    return np.asfortranarray(c, dtype=np.uint32)


def receivers(N, conn0, phase=1, message_mode=0):
    """stereo_trws_state_receivers_host (host only) -> (E,) int32: the node on whose labels the message row of every
    edge is indexed in a state of `phase` of a plan created with (N, conn0, message_mode): the endpoint later in the
    plan's node order in phases 1 and 2, the earlier one in phase 0."""
    c = _conn0(conn0)
    # the graph analysis behind it costs about what creating a plan does; the two views of a pair and the levels of a
    # scale ask for the same graph again and again, so the last few answers are kept (by content)
    key = (int(N), int(message_mode), int(phase), c.shape[1], hashlib.blake2b(c.tobytes(order="F"), digest_size=16).digest())
    if key in _receivers_cache:
        return _receivers_cache[key].copy()
    out = np.zeros(c.shape[1], np.int32)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_trws_state_receivers_host(C.c_int64(int(N)), C.c_int64(c.shape[1]), _p(c, C.c_uint32),
                                                     C.c_int(int(message_mode)), C.c_int(int(phase)), _p(out, C.c_int32),
                                                     err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    if len(_receivers_cache) >= 8:
        _receivers_cache.pop(next(iter(_receivers_cache)))
    _receivers_cache[key] = out.copy()
    return out


def carry_messages(M_old, off_old, off_new, receiver_new, shift, edge_src=None, stretch=1.0, gain=1.0):
    """stereo_band_carry on host arrays: `M_old` (E_old, K_old), `receiver_new` (E_new,) and `edge_src` (E_new,) int32,
    `shift` (N_new,).  The library checks the arguments (None goes through as NULL) before it looks for the device.
    -> (M_new (E_new, K_new), the number of edges that named a row or a node out of range)."""
    off_old, off_new, shift = _vec(off_old), _vec(off_new), _vec(shift)
    receiver_new, edge_src = _vec(receiver_new, np.int32), _vec(edge_src, np.int32)
    K_old = 0 if off_old is None else off_old.shape[0]
    K_new = 0 if off_new is None else off_new.shape[0]
    E_new = 0 if receiver_new is None else receiver_new.shape[0]
    if M_old is not None:
        M_old = np.ascontiguousarray(M_old, dtype=np.float64)
        if M_old.ndim != 2 or M_old.shape[1] != K_old:
            raise StereoHipError("carry_messages: M_old must be (E_old, K_old) with one column per old offset")
    E_old = 0 if M_old is None else M_old.shape[0]
    if edge_src is not None and edge_src.shape[0] != E_new:
        raise StereoHipError("carry_messages: edge_src must hold one entry per new edge")
    M_new = np.zeros((E_new, K_new))
    bad = C.c_int64(0)
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_carry(_p(M_old), C.c_int64(E_old), C.c_int(K_old), _p(off_old), _p(edge_src, C.c_int32),
                                      _p(receiver_new, C.c_int32), C.c_int64(0 if shift is None else shift.shape[0]),
                                      _p(shift), C.c_double(float(stretch)), C.c_double(float(gain)), _p(off_new),
                                      C.c_int(K_new), C.c_int64(E_new), _p(M_new), C.byref(bad), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return M_new, int(bad.value)


def _flat(t, what, dtype, n=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise StereoHipError("%s must be a contiguous %s tensor on the device" % (what, dtype))
    if t.device.index != torch.cuda.current_device():
        raise StereoHipError("%s must be on the current device" % what)
    if n is not None and t.numel() != n:
        raise StereoHipError("%s must hold %d elements (got %d)" % (what, n, t.numel()))
    return t


def carry_messages_device(M_old, off_old, off_new, receiver_new, shift, edge_src=None, stretch=1.0, gain=1.0, out=None,
                          bad=None, stream=None, d_off_old=None, d_off_new=None, check=True):
    """stereo_band_carry_device on torch tensors of the current device: `M_old` (E_old, K_old) float64, `receiver_new`
    and `edge_src` int32 (E_new,), `shift` float64 (N_new,); `off_old` / `off_new` are host vectors, `d_off_old` /
    `d_off_new` their device copies (made here when not given).  Launched on `stream` (a torch stream or a raw handle;
    default: torch's current stream).  check=True reads the count of offending edges back (this waits) and raises;
    check=False leaves it in `bad` and does not wait.  -> (M_new (E_new, K_new), bad)."""
    import torch
    from .consistency import _stream
    off_old, off_new = _vec(off_old), _vec(off_new)
    K_old, K_new = off_old.shape[0], off_new.shape[0]
    M_old = _flat(M_old, "M_old", torch.float64)
    if K_old < 1 or M_old.numel() % K_old:
        raise StereoHipError("M_old must hold E_old x K_old elements")
    E_old = M_old.numel() // K_old
    receiver_new = _flat(receiver_new, "receiver_new", torch.int32)
    E_new = receiver_new.numel()
    shift = _flat(shift, "shift", torch.float64)
    if edge_src is not None:
        edge_src = _flat(edge_src, "edge_src", torch.int32, E_new)
    dev = M_old.device
    made_here = d_off_old is None or d_off_new is None
    d_off_old = torch.from_numpy(np.array(off_old)).cuda() if d_off_old is None else _flat(d_off_old, "d_off_old", torch.float64, K_old)
    d_off_new = torch.from_numpy(np.array(off_new)).cuda() if d_off_new is None else _flat(d_off_new, "d_off_new", torch.float64, K_new)
    if made_here and stream is not None:
        torch.cuda.current_stream().synchronize()     # the copies ran on torch's current stream, the kernel will not
    out = torch.empty((E_new, K_new), dtype=torch.float64, device=dev) if out is None else _flat(out, "out", torch.float64, E_new * K_new)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if bad is None else _flat(bad, "bad", torch.int32, 1)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    err = _lib.errbuf()
    rc = _lib.lib().stereo_band_carry_device(vp(M_old), C.c_int64(E_old), C.c_int(K_old), _p(off_old), vp(d_off_old),
                                             vp(edge_src), vp(receiver_new), C.c_int64(shift.numel()), vp(shift),
                                             C.c_double(float(stretch)), C.c_double(float(gain)), _p(off_new), vp(d_off_new),
                                             C.c_int(K_new), C.c_int64(E_new), vp(out), vp(bad), C.c_void_p(_stream(stream)),
                                             err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    if check:
        n = int(bad.item())
        if n:
            raise StereoHipError("carry_messages_device: %d edge(s) name a row or a node out of range" % n)
    return out, bad


def scale_edge_map(conn_coarse, recv_coarse, conn_fine, recv_fine, parent):
    """`edge_src` for a step between pyramid scales, pure NumPy: a fine edge (a -> b) takes the coarse edge
    (parent[a] -> parent[b]) if that pair is a coarse edge with the same orientation whose receiver is the parent of the
    fine edge's receiver; otherwise -1 (both ends in one block, no such coarse edge, the receiver on the other end).
    conn_*: 2 x E zero based; recv_*: (E,) as `receivers` gives them; parent: (N_fine,) ints.  -> (E_fine,) int32."""
    cc, cf = np.asarray(conn_coarse).astype(np.int64), np.asarray(conn_fine).astype(np.int64)
    if cc.ndim != 2 or cc.shape[0] != 2 or cf.ndim != 2 or cf.shape[0] != 2:
        raise StereoHipError("connectivity must be 2 x E")
    parent = np.asarray(parent).astype(np.int64).reshape(-1)
    recv_coarse, recv_fine = np.asarray(recv_coarse).astype(np.int64).reshape(-1), np.asarray(recv_fine).astype(np.int64).reshape(-1)
    if recv_coarse.shape[0] != cc.shape[1] or recv_fine.shape[0] != cf.shape[1]:
        raise StereoHipError("scale_edge_map: one receiver per edge")
    out = np.full(cf.shape[1], -1, np.int32)
    if cc.shape[1] == 0 or cf.shape[1] == 0:
        return out
    stride = int(max(cc.max(), parent.max())) + 1
    keys = cc[0] * stride + cc[1]
    order = np.argsort(keys, kind="stable")             # (a pair named twice: its first edge)
    pa, pb = parent[cf[0]], parent[cf[1]]
    want = pa * stride + pb
    at = np.minimum(np.searchsorted(keys[order], want), keys.shape[0] - 1)
    edge = order[at]
    hit = (keys[edge] == want) & (pa != pb) & (recv_coarse[edge] == parent[recv_fine])
    out[hit] = edge[hit]
    return out


class Carry:
    """What a band problem's build() takes to start from the previous stage's messages:
    d_messages  (E_old, K_old) float64 tensor: that stage's saved state (save_state_device), phase 1
    offsets     its offsets on the host (a full-range solve with shared positions: its disparities)
    shift       (N_new,) float64 tensor: where the new level's offset 0 at node r lies on the old offset axis
    edge_src    (E_new,) int32 tensor or None (the same edges)
    receiver    (E_new,) int32 tensor, the NEW problem's receivers in phase 1, or None: the problem works them out
    stretch, gain  as in stereo_band_carry."""

    def __init__(self, d_messages, offsets, shift, edge_src=None, receiver=None, stretch=1.0, gain=1.0):
        self.d_messages, self.offsets, self.shift = d_messages, _vec(offsets), shift
        self.edge_src, self.receiver, self.stretch, self.gain = edge_src, receiver, float(stretch), float(gain)


class Stage:
    """What a solved stage leaves behind for the stage after it: `d_messages` (its state's (E, K) tensor), its
    `offsets`, `d_base` (the flat (N,) tensor its offsets were measured from, None: zero -- a full-range solve, whose
    offsets are its disparities), and the graph they belong to: `conn` (2 x E), `receiver` ((E,), host, phase 1) and
    `shape` (H, W)."""

    def __init__(self, d_messages, offsets, d_base, conn, receiver, shape):
        self.d_messages, self.offsets, self.d_base = d_messages, _vec(offsets), d_base
        self.conn, self.receiver, self.shape = conn, receiver, tuple(shape)


def box_parent(H, W):
    """(N,) int64: the node of the box-reduced (H + 1) // 2 x (W + 1) // 2 grid a node of the H x W grid lies in
    (nodes are col * H + row on both)."""
    i = np.arange(H * W, dtype=np.int64)
    return ((i // H) >> 1) * ((H + 1) // 2) + ((i % H) >> 1)


def full_range_stage(plan, disparities, conn, shape):
    """The Stage of a full-range solve with the shared positions `disparities` (its messages live on that axis), or
    None where they cannot be carried: positions that are not finite and strictly ascending, a state not in phase 1."""
    d = _vec(disparities)
    if d.shape[0] < 1 or not (np.isfinite(d).all() and (np.diff(d) > 0).all()):
        return None
    N = shape[0] * shape[1]
    d_m = save_messages(plan, N)
    return None if d_m is None else Stage(d_m, d, None, _conn0(conn), receivers(N, conn, 1), shape)


def carry_between(stage, d_base, conn, receiver, shape, scales=False):
    """The Carry from `stage` into a band problem around `d_base` (flat (N,) tensor) on the graph (conn, receiver,
    shape), or None without a stage.  On one scale the edges are the same and the shift is the difference of the two
    bases, taken on the device.  scales=True: the stage is one box reduction coarser; a fine edge inherits from the
    coarse edge between its ends' parents (scale_edge_map), one coarse disparity unit is two fine ones (stretch 0.5,
    shift = 0.5 base_fine - base_coarse[parent]) and one finer edge carries twice the coarse message (gain 2,
    DESIGN.md 6.5)."""
    import torch
    if stage is None:
        return None
    if not scales:
        shift = d_base if stage.d_base is None else d_base - stage.d_base
        return Carry(stage.d_messages, stage.offsets, shift.contiguous())
    H, W = shape
    if stage.shape != ((H + 1) // 2, (W + 1) // 2):
        raise StereoHipError("carry: the coarser stage must be the box reduction of this one")
    parent = box_parent(H, W)
    shift = 0.5 * d_base
    if stage.d_base is not None:
        shift = shift - stage.d_base[torch.from_numpy(parent).cuda()]
    edge_src = scale_edge_map(stage.conn, stage.receiver, conn, receiver, parent)
    return Carry(stage.d_messages, stage.offsets, shift.contiguous(), torch.from_numpy(edge_src).cuda(), stretch=0.5, gain=2.0)


def save_messages(plan, N):
    """The messages of `plan` at rest, saved on the device BEFORE the next build (a bind wipes the plan) -> the
    (E, K) tensor, or None where they cannot be carried as a phase-1 state (the plan stopped on max_relgap with a
    backward sweep ahead)."""
    import torch
    d_m = torch.empty((plan.E, plan.K), dtype=torch.float64, device="cuda")
    d_x = torch.empty(int(N), dtype=torch.int32, device="cuda")
    st = plan.save_state_device(d_m.data_ptr(), d_x.data_ptr())
    torch.cuda.synchronize()
    return d_m if st.phase == 1 else None


def load_carried(plan, carry, offsets, d_receiver, N, d_offsets=None):
    """The transfer of `carry` onto the level `offsets` of a plan that has its inputs, loaded as a state of phase 1
    with 0 iterations, energy and bound 0 and every label at offset 0: the first launch is then a backward sweep."""
    import torch
    offsets = _vec(offsets)
    zero = np.flatnonzero(offsets == 0.0)
    if zero.shape[0] != 1:
        raise StereoHipError("carry: the level's offsets must contain 0.0")
    d_m = torch.empty((plan.E, plan.K), dtype=torch.float64, device="cuda")
    d_x = torch.empty(int(N), dtype=torch.int32, device="cuda")
    st = plan.save_state_device(d_m.data_ptr(), d_x.data_ptr())     # (the header of this plan: kernel, sizes, key, mode)
    torch.cuda.synchronize()
    carry_messages_device(carry.d_messages, carry.offsets, offsets, d_receiver if carry.receiver is None else carry.receiver,
                          carry.shift, carry.edge_src, carry.stretch, carry.gain, out=d_m, d_off_new=d_offsets,
                          d_off_old=torch.from_numpy(np.array(carry.offsets)).cuda())
    d_x.fill_(int(zero[0]))
    torch.cuda.synchronize()
    st.phase, st.iterations, st.energy, st.lower_bound, st.lower_bound_next = 1, 0, 0.0, 0.0, 0.0
    plan.load_state_device(st, d_m.data_ptr(), d_x.data_ptr())
