"""Plane-band refinement without a device: every refusal of the C entries and the Python wrappers (the
arguments are checked before the device is looked for), the ABI numbers, and the properties of the restatement of the
definition (tests/plane_band_restate.py): a label moves its plane's disparity by exactly its offset, one slanted plane
costs nothing where the fronto-parallel band pays the slope, and the zero offset is the assignment itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import band_restate
import plane_band_restate as R
from band_restate import same, same_bits
from oracle import terms as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, CH, E = 3, 4, 5, 2, 2
N = H * W


def _lib():
    from stereo_amd import _lib as L
    return L.lib()


def _call(fn, *args):
    err = C.create_string_buffer(1024)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _planes():
    P = np.zeros((4, N), order="F")
    P[2] = 1.0
    return P


def _host():
    """keep-alive arrays and the argument values of a valid call"""
    return dict(ncc=np.zeros(N * D), disparities=np.arange(D, dtype=np.float64), im0=np.zeros(N * CH), im1=np.zeros(N * CH),
                P2=R.P2_example().reshape(-1, order="F").copy(), planes=_planes(), offsets=np.array([-0.5, 0.0, 0.5]),
                conn=np.array([0, 1, 1, 2], np.uint32), unary=np.zeros(3 * N), q=np.zeros(3 * E), qprim=np.zeros(3 * E),
                labels=np.ones(N, np.int32), refined=np.zeros(4 * N),
                H=H, W=W, D=D, C=CH, layout=0, K=None, E=E, N=N, d_min=0.5, d_step=4.0)


def _p(x):
    return None if x is None else C.c_void_p(x.ctypes.data)


def _k(v):
    return C.c_int(v["K"] if v["K"] is not None else (0 if v["offsets"] is None else len(v["offsets"])))


def _tail(v, device_form):
    args = [_p(v["planes"]), _p(v["offsets"])]
    if device_form:
        args.append(_p(v["offsets"]))             # (never read: the call is refused before the device is looked for)
    args += [_k(v), C.c_int64(v["E"]), _p(v["conn"]), _p(v["unary"]), _p(v["q"]), _p(v["qprim"])]
    if device_form:
        args += [None, None]                      # bad, stream
    return args


def _ncc_args(v, device_form):
    args = [_p(v["ncc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["D"]), C.c_int(v["layout"]), _p(v["disparities"])]
    if device_form:
        args.append(_p(v["disparities"]))
    return args + [C.c_double(1.0)] + _tail(v, device_form)


def _gs_args(v, device_form):
    args = [_p(v["im0"]), _p(v["im1"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["C"]), _p(v["P2"]),
            C.c_double(v["d_min"]), C.c_double(v["d_step"]), C.c_double(30.0)]
    return args + _tail(v, device_form)


def _apply_args(v, device_form):
    args = [_p(v["planes"]), C.c_int64(v["N"]), _p(v["labels"]), _p(v["offsets"])]
    if device_form:
        args.append(_p(v["offsets"]))
    args += [_k(v), _p(v["refined"])]
    if device_form:
        args += [None, None]
    return args


ENTRIES = {"ncc": ("stereo_plane_band_inputs_ncc", _ncc_args), "globalstereo": ("stereo_plane_band_inputs_globalstereo", _gs_args),
           "apply": ("stereo_plane_band_apply", _apply_args)}


def _refused(entry, device_form, change):
    name, build = ENTRIES[entry]
    name += "_device" if device_form else ""
    v = _host()
    v.update(change)
    rc, msg = _call(getattr(_lib(), name), *build(v, device_form))
    assert rc != 0, (name, change)
    assert msg.startswith(name + ":"), msg
    return msg


OFFSET_REFUSALS = [
    (dict(offsets=np.array([-0.5, np.nan, 0.0])), "not finite"),
    (dict(offsets=np.array([0.0, np.inf])), "not finite"),
    (dict(offsets=np.array([0.0, 0.5, 0.5])), "strictly ascending"),
    (dict(offsets=np.array([0.5, 0.0])), "strictly ascending"),
    (dict(offsets=np.array([-0.5, 0.25, 0.5])), r"contain 0\.0"),
    (dict(offsets=np.zeros(0), K=0), r"1 \.\. 512"),
    (dict(offsets=np.arange(513, dtype=np.float64), K=513), r"1 \.\. 512"),
    (dict(K=-1), r"1 \.\. 512"),
    (dict(offsets=None, K=3), "offsets must not be NULL"),
    (dict(planes=None), "NULL"),
]
SIZE_REFUSALS = [
    (dict(H=0), "H and W"),
    (dict(W=0), "H and W"),
    (dict(W=-2), "H and W"),
    (dict(H=1 << 16, W=1 << 15), r"2\^31"),
    (dict(E=-1), "E must not"),
    (dict(unary=None), "NULL"),
    (dict(conn=None), "NULL"),
    (dict(q=None), "NULL"),
    (dict(qprim=None), "NULL"),
]
REFUSALS = {
    "ncc": OFFSET_REFUSALS + SIZE_REFUSALS + [
        (dict(layout=2), "layout"), (dict(layout=-1), "layout"), (dict(D=0), "D must be"), (dict(ncc=None), "NULL"),
        (dict(disparities=None), "NULL")],
    "globalstereo": OFFSET_REFUSALS + SIZE_REFUSALS + [
        (dict(C=0), "C must be"), (dict(d_step=0.0), "d_step must not be 0"), (dict(im0=None), "NULL"), (dict(im1=None), "NULL"),
        (dict(P2=None), "NULL")],
    "apply": OFFSET_REFUSALS + [
        (dict(N=0), "N must be at least 1"), (dict(N=1 << 31), r"2\^31"), (dict(labels=None), "NULL"), (dict(refined=None), "NULL")],
}
ALL_REFUSALS = [(entry, change, match) for entry in ("ncc", "globalstereo", "apply") for change, match in REFUSALS[entry]]


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("entry,change,match", ALL_REFUSALS, ids=lambda c: c if isinstance(c, str) and c in ENTRIES else (
    ",".join(sorted(c)) if isinstance(c, dict) else None))
def test_refusals_are_made_without_a_device(device_form, entry, change, match):
    msg = _refused(entry, device_form, change)
    assert re.search(match, msg), msg


def test_device_forms_want_the_device_copies_of_the_short_vectors():
    v = _host()
    args = _ncc_args(v, True)
    args[6] = None
    rc, msg = _call(_lib().stereo_plane_band_inputs_ncc_device, *args)
    assert rc != 0 and "d_disparities" in msg
    args = _ncc_args(v, True)
    args[10] = None
    rc, msg = _call(_lib().stereo_plane_band_inputs_ncc_device, *args)
    assert rc != 0 and "d_offsets" in msg
    args = _gs_args(v, True)
    args[11] = None
    rc, msg = _call(_lib().stereo_plane_band_inputs_globalstereo_device, *args)
    assert rc != 0 and "d_offsets" in msg
    args = _apply_args(v, True)
    args[4] = None
    rc, msg = _call(_lib().stereo_plane_band_apply_device, *args)
    assert rc != 0 and "d_offsets" in msg


def test_host_entries_refuse_a_plane_without_a_disparity_and_name_the_pixel():
    pixel = 1 + H * 2                                          # row 1, column 2
    for entry in ("ncc", "globalstereo", "apply"):
        where = "pixel %d" % pixel if entry == "apply" else "row 1, column 2"
        planes = _planes()
        planes[2, pixel] = 0.0
        msg = _refused(entry, False, dict(planes=planes))
        assert "Infinite disparity" in msg and where in msg, msg
        for component in range(4):
            for bad in (np.nan, np.inf, -np.inf):
                planes = _planes()
                planes[component, pixel] = bad
                msg = _refused(entry, False, dict(planes=planes))
                assert "not finite" in msg and where in msg, msg


def test_host_entries_refuse_labels_and_edges_out_of_range():
    for lab in (0, 4, -1):
        labels = np.ones(N, np.int32)
        labels[5] = lab
        msg = _refused("apply", False, dict(labels=labels))
        assert "outside 1 .. 3" in msg and "pixel 5" in msg, msg
    for entry in ("ncc", "globalstereo"):
        msg = _refused(entry, False, dict(conn=np.array([0, 1, 1, N], np.uint32)))
        assert "conn" in msg and "edge 1" in msg, msg


def test_python_wrappers_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import StereoHipError, plane_band
    from stereo_amd import terms as T
    conn = T.construct_neighborhood(H, W)
    planes = _planes()
    im = np.zeros((H, W, CH))
    sources = (stereo_amd.NccSource(np.zeros((H, W, D)), np.arange(D, dtype=np.float64), 1.0),
               stereo_amd.GlobalstereoSource(im, im, R.P2_example(), 30.0))
    for source, rescale in zip(sources, ((0.0, 0.0), (0.5, 4.0))):
        for offsets, match in (([0.0, 0.0], "strictly ascending"), ([1.0, 2.0], "contain 0"), ([np.nan, 0.0], "not finite"),
                               ([], "1 .. 512"), (np.arange(600.0), "1 .. 512")):
            with pytest.raises(StereoHipError, match=match):
                stereo_amd.plane_band_inputs(source, planes, offsets, conn, *rescale)
            with pytest.raises(StereoHipError, match=match):
                stereo_amd.plane_band_apply(planes, np.ones(N), offsets)
        with pytest.raises(StereoHipError, match="4 x N"):
            stereo_amd.plane_band_inputs(source, planes[:, :-1], [0.0], conn, *rescale)
        with pytest.raises(StereoHipError, match="4 x N"):
            stereo_amd.plane_band_inputs(source, planes[:3], [0.0], conn, *rescale)
        flat = planes.copy()
        flat[2, 1 + H * 2] = 0.0
        with pytest.raises(StereoHipError, match="Infinite disparity.*row 1, column 2"):
            stereo_amd.plane_band_inputs(source, flat, [0.0], conn, *rescale)
    with pytest.raises(StereoHipError, match="d_step must not be 0"):
        stereo_amd.plane_band_inputs(sources[1], planes, [0.0], conn)
    with pytest.raises(StereoHipError, match="no rescaling"):
        stereo_amd.plane_band_inputs(sources[0], planes, [0.0], conn, 0.0, 4.0)
    with pytest.raises(StereoHipError, match="unary source"):
        stereo_amd.plane_band_inputs(object(), planes, [0.0], conn)
    with pytest.raises(StereoHipError, match="disparities for a volume"):
        stereo_amd.NccSource(np.zeros((H, W, D)), np.arange(D - 1.0), 1.0)
    with pytest.raises(StereoHipError, match="shape="):
        stereo_amd.NccSource(np.zeros((D, N)), np.arange(D * 1.0), 1.0, layout=1)
    with pytest.raises(StereoHipError, match="4 x 3"):
        stereo_amd.GlobalstereoSource(im, im, np.zeros((3, 4)), 30.0)
    with pytest.raises(StereoHipError, match="one size"):
        stereo_amd.GlobalstereoSource(im, im[:, :-1], R.P2_example(), 30.0)
    with pytest.raises(StereoHipError, match="outside 1 .. 2"):
        stereo_amd.plane_band_apply(planes, np.full(N, 3.0), [0.0, 1.0])
    with pytest.raises(StereoHipError, match="whole numbers"):
        stereo_amd.plane_band_apply(planes, np.full(N, 1.5), [0.0, 1.0])
    with pytest.raises(StereoHipError, match="one value per plane"):
        stereo_amd.plane_band_apply(planes, np.ones(N - 1), [0.0, 1.0])
    with pytest.raises(StereoHipError, match="at least one"):
        plane_band.check_levels([])
    for name in ("plane_band_inputs", "plane_band_apply", "plane_band_inputs_device", "plane_band_apply_device",
                 "refine_plane_band", "NccSource", "GlobalstereoSource", "PlaneBandProblem"):
        assert name in stereo_amd.__all__ and callable(getattr(stereo_amd, name))
    for cls in (stereo_amd.dispmap_ncc, stereo_amd.dispmap_globalstereo):
        assert cls.refine_plane_band is stereo_amd.dispmap_super.refine_plane_band          # implemented once
        assert cls._plane_band_source is not stereo_amd.dispmap_super._plane_band_source    # over a per-class hook
    bare = object.__new__(stereo_amd.dispmap_super)
    with pytest.raises(StereoHipError, match="at least one"):
        bare.refine_plane_band([])
    with pytest.raises(StereoHipError, match="names no unary source"):
        bare.refine_plane_band([[0.0]])


def test_the_three_abi_numbers_agree_and_count_the_plane_band_section():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 13
    for name in ("stereo_plane_band_inputs_ncc", "stereo_plane_band_inputs_globalstereo", "stereo_plane_band_apply",
                 "stereo_plane_band_inputs_ncc_device", "stereo_plane_band_inputs_globalstereo_device",
                 "stereo_plane_band_apply_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the restatement

OFFSETS = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
SHAPES = [(1, 9), (9, 1), (5, 7)]


def _grid(Hh, Ww):
    ind1, ind2 = OT.construct_neighborhood(Hh, Ww)
    return np.stack([ind1, ind2])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_label_moves_the_planes_disparity_by_exactly_its_offset(shape):
    Hh, Ww = shape
    base = band_restate.base_map(Hh, Ww, 6, 2.0, 3)
    planes = R.planes_through(base, 1)
    assert set(planes[2]) <= {1.0, -1.0, 2.0} and planes[2, 0] == -1.0 and planes[2, 1] == 2.0
    assert np.array_equal(planes[:2] * 4, np.rint(planes[:2] * 4)) and np.array_equal(planes[3] * 4, np.rint(planes[3] * 4))
    points = OT.get_points(Hh, Ww)
    own = OT.disparity_from_assignment(planes, points)
    assert np.array_equal(own, base.T.reshape(-1))
    for delta, P in zip(OFFSETS, R.proposals(planes, OFFSETS)):
        assert np.array_equal(P[:3], planes[:3])
        assert np.array_equal(OT.disparity_from_assignment(P, points), own + delta)
    labels = np.random.default_rng(4).integers(1, len(OFFSETS) + 1, size=Hh * Ww)
    moved = R.apply(planes, labels, OFFSETS)
    assert np.array_equal(moved[:3], planes[:3])
    assert np.array_equal(OT.disparity_from_assignment(moved, points), own + OFFSETS[labels - 1])
    with pytest.raises(ValueError):
        R.apply(planes, np.full(Hh * Ww, len(OFFSETS) + 1), OFFSETS)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_slanted_plane_costs_nothing_where_the_fronto_parallel_band_pays_the_slope(shape):
    Hh, Ww = shape
    a, b, c = 0.25, -0.5, 2.0
    planes = R.slanted_map(Hh, Ww, a, b, c, -9.0)
    conn = _grid(Hh, Ww)
    ncc, disp = band_restate.volume(Hh, Ww, 6, 1), band_restate.disparities_for(6, False)
    _, q, qprim = R.inputs_ncc(ncc, disp, 3.0, planes, OFFSETS, conn)
    assert q.shape == (len(OFFSETS), conn.shape[1]) and same_bits(q, qprim)
    im0, im1 = R.images(Hh, Ww, 2, 3)
    _, q, qprim = R.inputs_globalstereo(im0, im1, R.P2_example(), 0.5, 4.0, 30.0, planes, OFFSETS, conn)
    assert same_bits(q, qprim)
    # the band of DESIGN.md 6.2 on the same map's disparities: every edge pays the slope along its direction
    points = OT.get_points(Hh, Ww)
    base = OT.disparity_from_assignment(planes, points).reshape(Ww, Hh).T
    _, fq, fqprim = band_restate.band_inputs(ncc, disp, 3.0, base, OFFSETS, conn)
    along_x = points[0][conn[0]] != points[0][conn[1]]
    slope = np.where(along_x, abs(a / c), abs(b / c))
    assert np.array_equal(np.abs(fq - fqprim), np.broadcast_to(slope, fq.shape)) and slope.min() > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_zero_offset_is_the_assignment_itself(shape):
    Hh, Ww = shape
    zero = list(OFFSETS).index(0.0)
    conn = _grid(Hh, Ww)
    points = OT.get_points(Hh, Ww)
    p2 = points[:, conn[1]]
    weights = np.random.default_rng(2).integers(1, 9, size=conn.shape[1]).astype(np.float64)
    base = band_restate.base_map(Hh, Ww, 6, 2.0, 3)
    ncc, disp = band_restate.volume(Hh, Ww, 6, 1), band_restate.disparities_for(6, False)
    im0, im1 = R.images(Hh, Ww, 3, 3)
    for dyadic in (True, False):
        planes = R.planes_through(base, 1, dyadic)
        unary, q, qprim = R.inputs_ncc(ncc, disp, 3.0, planes, OFFSETS, conn)
        assert same(unary[zero], OT.ncc_unary_cost(ncc, disp, 3.0, planes, points))
        cases = [(q, qprim, 0.0, 0.0)]
        for d_min, d_step in (R.GS_DYADIC, (0.0, 40.0)):
            unary, q, qprim = R.inputs_globalstereo(im0, im1, R.P2_example(), d_min, d_step, 30.0, planes, OFFSETS, conn)
            assert same(unary[zero], OT.globalstereo_unary_cost(im0, im1, R.P2_example(), d_min, d_step, 30.0, planes, points))
            cases.append((q, qprim, d_min, d_step))
        for q, qprim, d_min, d_step in cases:
            fn = R.disp_fn(d_min, d_step)
            assert same(q[zero], fn(planes[:, conn[1]], p2)) and same(qprim[zero], fn(planes[:, conn[0]], p2))
            for kernel in (1, 2):
                E00 = OT.all_pairwise_costs(kernel, weights, 2.0, planes, planes, conn[0], conn[1], points, disp_fn=fn)[0]
                assert same(OT.pairwise_cost(kernel, weights, q[zero], qprim[zero], 2.0), E00)


@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (5, 7), (67, 3), (3, 67)], ids=lambda s: "%dx%d" % s)
def test_the_crafted_globalstereo_pixels_reach_the_borders(shape):
    Hh, Ww = shape
    d_min, d_step = R.GS_DYADIC
    for P2, size, axis in ((R.P2_example(), Ww, 0), (R.P2_rows(), Hh, 1)):
        base = R.gs_base_map(Hh, Ww, P2, d_min, d_step, 3)
        planes = R.planes_through(base, 2)
        got = R.gs_projected(P2, d_min, d_step, planes, Hh, Ww)[axis]
        want = [0.5, float(size), size + 1.0, 1.0, size - 0.5]
        n = min(len(want), Hh * Ww)
        assert np.array_equal(got[:n], want[:n])
        other = R.gs_projected(P2, d_min, d_step, planes, Hh, Ww)[1 - axis]
        assert np.array_equal(other, OT.get_points(Hh, Ww)[1 - axis])
