"""Plane candidates without a device: every refusal of the C entries and the Python wrappers (the
arguments are checked before the device is looked for), the ABI numbers, the restatement's own properties
(tests/plane_candidates_restate.py) and the slanted chain of the issue, whose optimum the device test then has to reach."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import band_restate
import candidates_restate as CR
import first_principles as fp
import plane_band_restate as PB
import plane_candidates_restate as R
from band_restate import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, E, CH = 3, 4, 5, 2, 2
KO, M, T = 3, 2, 2
K = KO + M * T
NEVER = -1e300
ENTRIES = ("stereo_plane_candidates_gather", "stereo_plane_candidates_inputs_ncc", "stereo_plane_candidates_inputs_globalstereo",
           "stereo_plane_candidates_apply", "stereo_plane_candidates_gather_device", "stereo_plane_candidates_inputs_ncc_device",
           "stereo_plane_candidates_inputs_globalstereo_device", "stereo_plane_candidates_apply_device")


def _lib():
    from stereo_amd import _lib as L
    return L.lib()


def _call(fn, *args):
    err = C.create_string_buffer(1024)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _aligned(n):
    """n zero doubles that start on a 16-byte boundary (the device forms refuse other plane arrays)"""
    raw = np.zeros(n + 1)
    return raw[1:] if raw.ctypes.data % 16 else raw[:n]


def _unit_planes(count):
    p = _aligned(4 * count)
    p[2::4] = 1.0
    return p


def _host():
    """keep-alive arrays and the argument values of a valid call"""
    return dict(ncc=np.zeros(H * W * D), disparities=np.arange(D, dtype=np.float64), im0=np.zeros(H * W * CH), im1=np.zeros(H * W * CH),
                P2=np.zeros(12), planes=_unit_planes(H * W), offsets=np.array([-0.5, 0.0, 0.5]), sources=_unit_planes(M * H * W),
                taps=np.array([0, 1, -1, 0], np.int32), pcand=_unit_planes(K * H * W), conn=np.array([0, 1, 1, 2], np.uint32),
                unary=np.zeros(K * H * W), q=np.zeros(K * E), qprim=np.zeros(K * E), labels=np.ones(H * W, np.int32),
                out=_aligned(4 * H * W))


def _p(x):
    return None if x is None else C.c_void_p(x.ctypes.data)


def _gather_args(v, device_form):
    Ko = v["Ko"] if v["Ko"] is not None else (0 if v["offsets"] is None else len(v["offsets"]))
    args = [_p(v["planes"]), C.c_int(v["H"]), C.c_int(v["W"]), _p(v["offsets"])]
    if device_form:
        args.append(_p(v["offsets"]))          # (never read: the call is refused before the device is looked for)
    args += [C.c_int(Ko), _p(v["sources"]), C.c_int(v["M"]), _p(v["taps"])]
    if device_form:
        args.append(_p(v["taps"]))
    args += [C.c_int(v["T"]), _p(v["pcand"])]
    if device_form:
        args += [None, None]
    return args


def _tail(v, device_form):
    args = [_p(v["pcand"]), C.c_int(v["K"]), C.c_int64(v["E"]), _p(v["conn"]), _p(v["unary"]), _p(v["q"]), _p(v["qprim"])]
    if device_form:
        args += [None, None]
    return args


def _ncc_args(v, device_form):
    args = [_p(v["ncc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["D"]), C.c_int(v["layout"]), _p(v["disparities"])]
    if device_form:
        args.append(_p(v["disparities"]))
    return args + [C.c_double(1.0)] + _tail(v, device_form)


def _gs_args(v, device_form):
    return [_p(v["im0"]), _p(v["im1"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["C"]), _p(v["P2"]), C.c_double(0.5),
            C.c_double(v["d_step"]), C.c_double(30.0)] + _tail(v, device_form)


def _apply_args(v, device_form):
    args = [_p(v["pcand"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["K"]), _p(v["labels"]), _p(v["out"])]
    if device_form:
        args += [None, None]
    return args


SIZE_REFUSALS = [
    (dict(H=0), "H and W"),
    (dict(W=0), "H and W"),
    (dict(W=-2), "H and W"),
    (dict(H=1 << 16, W=1 << 15), r"2\^31"),
]
GATHER_REFUSALS = SIZE_REFUSALS + [
    (dict(offsets=np.array([-0.5, np.nan, 0.0])), "not finite"),
    (dict(offsets=np.array([0.0, np.inf])), "not finite"),
    (dict(offsets=np.array([0.0, 0.5, 0.5])), "strictly ascending"),
    (dict(offsets=np.array([0.5, 0.0])), "strictly ascending"),
    (dict(offsets=np.array([-0.5, 0.25, 0.5])), r"contain 0\.0"),
    (dict(offsets=np.zeros(0), Ko=0), r"1 \.\. 512"),
    (dict(offsets=np.arange(513, dtype=np.float64), Ko=513), r"1 \.\. 512"),
    (dict(Ko=-1), r"1 \.\. 512"),
    (dict(offsets=None, Ko=3), "offsets must not be NULL"),
    (dict(planes=None), "NULL"),
    (dict(pcand=None), "NULL"),
    (dict(M=-1), "M and T must not be negative"),
    (dict(T=-1), "M and T must not be negative"),
    (dict(sources=None), "sources and taps must not be NULL"),
    (dict(taps=None), "sources and taps must not be NULL"),
    (dict(offsets=np.arange(-255.0, 255.0), M=1, T=3, taps=np.zeros(6, np.int32)), r"K = Ko \+ M \* T must be 1 \.\. 512 \(got 513\)"),
    (dict(M=1 << 20, T=1 << 20), r"1 \.\. 512"),
    (dict(taps=np.array([0, 1, 1 << 15, 0], np.int32)), r"tap 1 has \|dy\| or \|dx\| of 2\^15 or more"),
    (dict(taps=np.array([0, -(1 << 15), 0, 0], np.int32)), r"tap 0 has \|dy\| or \|dx\| of 2\^15 or more"),
]
TABLE_REFUSALS = [
    (dict(E=-1), "E must not"),
    (dict(K=0), r"1 \.\. 512"),
    (dict(K=513), r"1 \.\. 512"),
    (dict(K=-3), r"1 \.\. 512"),
    (dict(pcand=None), "NULL"),
    (dict(unary=None), "NULL"),
    (dict(conn=None), "NULL"),
    (dict(q=None), "NULL"),
    (dict(qprim=None), "NULL"),
]
NCC_REFUSALS = SIZE_REFUSALS + TABLE_REFUSALS + [
    (dict(layout=2), "layout"),
    (dict(layout=-1), "layout"),
    (dict(D=0), "D must be"),
    (dict(ncc=None), "NULL"),
    (dict(disparities=None), "NULL"),
]
GS_REFUSALS = SIZE_REFUSALS + TABLE_REFUSALS + [
    (dict(C=0), "C must be"),
    (dict(d_step=0.0), "d_step must not be 0"),
    (dict(im0=None), "NULL"),
    (dict(im1=None), "NULL"),
    (dict(P2=None), "NULL"),
]
APPLY_REFUSALS = SIZE_REFUSALS + [
    (dict(K=0), r"1 \.\. 512"),
    (dict(K=513), r"1 \.\. 512"),
    (dict(pcand=None), "NULL"),
    (dict(labels=None), "NULL"),
    (dict(out=None), "NULL"),
]
_ids = lambda c: None if isinstance(c, str) else ",".join(sorted(c))
_forms = pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])


def _refused(name, device_form, args, match):
    fn = getattr(_lib(), name + ("_device" if device_form else ""))
    rc, msg = _call(fn, *args)
    assert rc != 0 and re.search(match, msg), msg
    assert msg.startswith(name + ("_device" if device_form else ":"))


@_forms
@pytest.mark.parametrize("change,match", GATHER_REFUSALS, ids=_ids)
def test_gather_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, Ko=None, M=M, T=T)
    v.update(change)
    _refused("stereo_plane_candidates_gather", device_form, _gather_args(v, device_form), match)


@_forms
@pytest.mark.parametrize("change,match", NCC_REFUSALS, ids=_ids)
def test_inputs_ncc_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, D=D, layout=0, K=K, E=E)
    v.update(change)
    _refused("stereo_plane_candidates_inputs_ncc", device_form, _ncc_args(v, device_form), match)


@_forms
@pytest.mark.parametrize("change,match", GS_REFUSALS, ids=_ids)
def test_inputs_globalstereo_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, C=CH, d_step=4.0, K=K, E=E)
    v.update(change)
    _refused("stereo_plane_candidates_inputs_globalstereo", device_form, _gs_args(v, device_form), match)


@_forms
@pytest.mark.parametrize("change,match", APPLY_REFUSALS, ids=_ids)
def test_apply_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, K=K)
    v.update(change)
    _refused("stereo_plane_candidates_apply", device_form, _apply_args(v, device_form), match)


def test_without_sources_or_taps_the_two_may_be_null_and_without_edges_their_arrays():
    """M * T == 0 is the plane band's table: NULL sources and taps pass the checks (the call then stops at the device, or
    runs); so do NULL conn, q and qprim with E == 0."""
    for m, t in ((0, 0), (0, 2), (2, 0)):
        v = dict(_host(), H=H, W=W, Ko=None, M=m, T=t, sources=None, taps=None)
        rc, msg = _call(_lib().stereo_plane_candidates_gather, *_gather_args(v, False))
        assert rc == 0 or "no HIP device" in msg, msg
    v = dict(_host(), H=H, W=W, D=D, layout=0, K=K, E=0, C=CH, d_step=4.0, conn=None, q=None, qprim=None)
    for fn, args in ((_lib().stereo_plane_candidates_inputs_ncc, _ncc_args(v, False)),
                     (_lib().stereo_plane_candidates_inputs_globalstereo, _gs_args(v, False))):
        rc, msg = _call(fn, *args)
        assert rc == 0 or "no HIP device" in msg, msg


def test_device_forms_want_the_device_copies_of_the_short_vectors_and_aligned_planes():
    v = dict(_host(), H=H, W=W, Ko=None, M=M, T=T)
    for at, name in ((4, "d_offsets"), (9, "d_taps")):
        args = _gather_args(v, True)
        args[at] = None
        rc, msg = _call(_lib().stereo_plane_candidates_gather_device, *args)
        assert rc != 0 and name in msg
    args = _ncc_args(dict(_host(), H=H, W=W, D=D, layout=0, K=K, E=E), True)
    args[6] = None
    rc, msg = _call(_lib().stereo_plane_candidates_inputs_ncc_device, *args)
    assert rc != 0 and "d_disparities" in msg
    # a plane moves as two 16-byte accesses
    def odd(n):
        raw = np.zeros(n + 2)
        out = raw[1:] if raw.ctypes.data % 16 == 0 else raw[2:]
        assert out.ctypes.data % 16 == 8
        return out
    for name in ("planes", "sources", "pcand"):
        a = _host()
        a[name] = odd(a[name].shape[0])
        rc, msg = _call(_lib().stereo_plane_candidates_gather_device, *_gather_args(dict(a, H=H, W=W, Ko=None, M=M, T=T), True))
        assert rc != 0 and "%s must be 16-byte aligned" % name in msg, msg
    a = _host()
    a["pcand"] = odd(4 * K * H * W)
    for fn, args in ((_lib().stereo_plane_candidates_inputs_ncc_device, _ncc_args(dict(a, H=H, W=W, D=D, layout=0, K=K, E=E), True)),
                     (_lib().stereo_plane_candidates_inputs_globalstereo_device, _gs_args(dict(a, H=H, W=W, C=CH, d_step=4.0, K=K, E=E), True)),
                     (_lib().stereo_plane_candidates_apply_device, _apply_args(dict(a, H=H, W=W, K=K), True))):
        rc, msg = _call(fn, *args)
        assert rc != 0 and "pcand must be 16-byte aligned" in msg, msg
    a = _host()
    a["out"] = odd(4 * H * W)
    rc, msg = _call(_lib().stereo_plane_candidates_apply_device, *_apply_args(dict(a, H=H, W=W, K=K), True))
    assert rc != 0 and "out must be 16-byte aligned" in msg, msg


def test_host_entries_refuse_offending_planes_and_name_the_pixel_and_the_label():
    gather = lambda a: _call(_lib().stereo_plane_candidates_gather, *_gather_args(dict(a, H=H, W=W, Ko=None, M=M, T=T), False))
    for bad, component, match in ((np.nan, 0, "is not finite"), (np.inf, 1, "is not finite"), (-np.inf, 3, "is not finite"),
                                  (0.0, 2, r"Infinite disparity \(c == 0\)"), (-0.0, 2, r"Infinite disparity \(c == 0\)")):
        a = _host()
        a["planes"][4 * (1 + H * 2) + component] = bad              # row 1, column 2
        rc, msg = gather(a)
        assert rc != 0 and re.search(match, msg) and "planes" in msg and "row 1, column 2" in msg, msg
        a = _host()
        a["sources"][4 * (H * W + 2 + H * 3) + component] = bad     # source 1, row 2, column 3
        rc, msg = gather(a)
        assert rc != 0 and re.search(match, msg) and "source 1" in msg and "row 2, column 3" in msg, msg
        a = _host()
        a["pcand"][4 * (K * (1 + H * 2) + 4) + component] = bad     # row 1, column 2, label 5
        for fn, args in ((_lib().stereo_plane_candidates_inputs_ncc, _ncc_args(dict(a, H=H, W=W, D=D, layout=0, K=K, E=E), False)),
                         (_lib().stereo_plane_candidates_inputs_globalstereo, _gs_args(dict(a, H=H, W=W, C=CH, d_step=4.0, K=K, E=E), False)),
                         (_lib().stereo_plane_candidates_apply, _apply_args(dict(a, H=H, W=W, K=K), False))):
            rc, msg = _call(fn, *args)
            assert rc != 0 and re.search(match, msg) and "row 1, column 2" in msg and "label 5" in msg, msg


def test_host_entries_refuse_labels_and_edges_out_of_range():
    for lab in (0, K + 1, -1):
        a = _host()
        a["labels"][5] = lab
        rc, msg = _call(_lib().stereo_plane_candidates_apply, *_apply_args(dict(a, H=H, W=W, K=K), False))
        assert rc != 0 and "outside 1 .. %d" % K in msg and "pixel 5" in msg, msg
    a = _host()
    a["conn"][3] = H * W
    for fn, args in ((_lib().stereo_plane_candidates_inputs_ncc, _ncc_args(dict(a, H=H, W=W, D=D, layout=0, K=K, E=E), False)),
                     (_lib().stereo_plane_candidates_inputs_globalstereo, _gs_args(dict(a, H=H, W=W, C=CH, d_step=4.0, K=K, E=E), False))):
        rc, msg = _call(fn, *args)
        assert rc != 0 and "conn" in msg and "edge 1" in msg, msg


def test_python_wrappers_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import StereoHipError, plane_candidates
    from stereo_amd import terms as Tm
    N = H * W
    planes = np.zeros((4, N))
    planes[2] = 1.0
    src = stereo_amd.NccSource(np.zeros((H, W, D)), np.arange(D, dtype=np.float64), 1.0)
    gs = stereo_amd.GlobalstereoSource(np.zeros((H, W, CH)), np.zeros((H, W, CH)), PB.P2_example(), 30.0)
    conn = Tm.construct_neighborhood(H, W)
    for offsets, match in (([0.0, 0.0], "strictly ascending"), ([1.0, 2.0], "contain 0"), ([np.nan, 0.0], "not finite"),
                           ([], "1 .. 512"), (np.arange(600.0), "1 .. 512")):
        with pytest.raises(StereoHipError, match=match):
            plane_candidates.gather(planes, offsets, (H, W), [planes], [(0, 1)])
    with pytest.raises(StereoHipError, match="pairs"):
        plane_candidates.gather(planes, [0.0], (H, W), [planes], [1, 2, 3])
    with pytest.raises(StereoHipError, match="whole numbers"):
        plane_candidates.gather(planes, [0.0], (H, W), [planes], [(0.5, 0)])
    with pytest.raises(StereoHipError, match=r"2\^15"):
        plane_candidates.gather(planes, [0.0], (H, W), [planes], [(0, 1 << 15)])
    with pytest.raises(StereoHipError, match="4 x N planes of the image's size"):
        plane_candidates.gather(planes, [0.0], (H, W), [np.zeros((4, N + 1))], [(0, 1)])
    with pytest.raises(StereoHipError, match="planes must be 4 x N"):
        plane_candidates.gather(np.zeros((3, N)), [0.0], (H, W))
    zero_c = planes.copy()
    zero_c[2, 2 + H * 3] = 0.0
    with pytest.raises(StereoHipError, match=r"Infinite disparity \(c == 0\) in source 0 at pixel \(row 2, column 3\)"):
        plane_candidates.gather(planes, [0.0], (H, W), [zero_c], [(0, 1)])
    table = np.repeat(planes[:, None, :], 2, axis=1)
    with pytest.raises(StereoHipError, match=r"4 x K x \(H\*W\)"):
        stereo_amd.plane_candidates_inputs(src, np.zeros((4, 2, N + 1)), (H, W), conn)
    with pytest.raises(StereoHipError, match=r"4 x K x \(H\*W\)"):
        stereo_amd.plane_candidates_inputs(src, np.zeros((2, N)), (H, W), conn)
    with pytest.raises(StereoHipError, match="the unary source is 3 x 4"):
        stereo_amd.plane_candidates_inputs(src, np.zeros((4, 2, N)), (W, H), conn)
    with pytest.raises(StereoHipError, match="NccSource or a GlobalstereoSource"):
        stereo_amd.plane_candidates_inputs(object(), table, (H, W), conn)
    with pytest.raises(StereoHipError, match="no rescaling"):
        stereo_amd.plane_candidates_inputs(src, table, (H, W), conn, d_min=0.5, d_step=4.0)
    with pytest.raises(StereoHipError, match="d_step must not be 0"):
        stereo_amd.plane_candidates_inputs(gs, table, (H, W), conn)
    nan_table = table.copy()
    nan_table[3, 1, 2 + H * 3] = np.nan
    for source, extra in ((src, {}), (gs, dict(d_min=0.5, d_step=4.0))):
        with pytest.raises(StereoHipError, match=r"not finite at pixel \(row 2, column 3\), label 2"):
            stereo_amd.plane_candidates_inputs(source, nan_table, (H, W), conn, **extra)
    with pytest.raises(StereoHipError, match="outside 1 .. 2"):
        stereo_amd.plane_candidates_apply(table, np.full(N, 3.0), (H, W))
    with pytest.raises(StereoHipError, match="whole numbers"):
        stereo_amd.plane_candidates_apply(table, np.full(N, 1.5), (H, W))
    # levels
    with pytest.raises(StereoHipError, match="at least one"):
        plane_candidates.check_levels([])
    for level, match in ((dict(offsets=[1.0]), "contain 0"), (dict(taps=[(0, 1 << 15)], sources=["base"]), r"2\^15"),
                         (dict(sources=["wta"], taps=[(0, 1)]), "'base' or 4 x N planes"), (dict(offset=[0.0]), "dict"),
                         (dict(sources=[np.zeros((H, W))], taps=[(0, 1)]), "'base' or 4 x N planes"), ([0.0], "dict"),
                         (dict(offsets=np.arange(-255.0, 256.0), taps=[(0, 1), (1, 0)], sources=["base"]), "1 .. 512")):
        with pytest.raises(StereoHipError, match=match):
            plane_candidates.check_level(level)
    lv = plane_candidates.check_level(dict(taps=[(0, 1), (1, 0)], sources=["base", planes]))
    assert lv["offsets"].tolist() == [0.0] and plane_candidates.PlaneCandidateProblem.labels_of(lv) == 5
    assert len(plane_candidates.check_levels(dict(sources="base", taps=[(0, 0)]))) == 1
    for name in ("plane_candidates_inputs", "plane_candidates_apply", "plane_candidates_inputs_device", "plane_candidates_apply_device",
                 "refine_plane_candidates", "PlaneCandidateProblem"):
        assert name in stereo_amd.__all__ and callable(getattr(stereo_amd, name))
    for name in ("gather", "gather_device", "fronto", "check_level", "check_levels"):
        assert callable(getattr(plane_candidates, name))
    assert issubclass(stereo_amd.PlaneCandidateProblem, stereo_amd.PlaneBandProblem)
    for cls in (stereo_amd.dispmap_ncc, stereo_amd.dispmap_globalstereo):
        assert callable(cls.refine_plane_candidates)
    # fronto: [0 0 1 -v], column major, the sign of zero as the candidate band's proposal has it
    m = np.arange(N, dtype=np.float64).reshape(H, W) / 4.0
    assert same_bits(plane_candidates.fronto(m), R.fronto(m)) and np.signbit(plane_candidates.fronto(m)[3, 0])


def test_the_classes_refuse_bad_levels_before_the_device_and_globalstereo_still_refuses_candidate_bands():
    import stereo_amd
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(stereo_amd.StereoHipError, match="dispmap_globalstereo does not take its unary from the NCC sampler"):
        glob.refine_candidates([dict()])
    with pytest.raises(stereo_amd.StereoHipError, match="'base' or 4 x N planes"):
        glob.refine_plane_candidates([dict(sources=["wta"], taps=[(0, 0)])])
    with pytest.raises(stereo_amd.StereoHipError, match="at least one"):
        glob.refine_plane_candidates([])
    ncc = object.__new__(stereo_amd.dispmap_ncc)
    ncc.sz = (H, W)
    with pytest.raises(stereo_amd.StereoHipError, match="contain 0"):
        ncc.refine_plane_candidates(dict(offsets=[0.5], sources=["base"], taps=[(0, 1)]))
    with pytest.raises(stereo_amd.StereoHipError, match="'base' or 4 x N planes"):
        ncc.refine_plane_candidates(dict(sources=[np.zeros((H + 2, W))], taps=[(0, 1)]))


def test_the_abi_numbers_agree_and_the_eight_entries_are_declared_and_exported():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 18
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the restatement's own properties

def _ncc_case(shuffled):
    Hh, Ww, Dd = 5, 7, 6
    ncc = band_restate.volume(Hh, Ww, Dd, 1)
    disp = band_restate.disparities_for(Dd, shuffled)
    planes = PB.planes_through(band_restate.base_map(Hh, Ww, Dd, 2.0, 3), 4)
    from oracle import terms as OT
    return Hh, Ww, ncc, disp, planes, np.stack(OT.construct_neighborhood(Hh, Ww))


@pytest.mark.parametrize("shuffled", [False, True])
def test_without_sources_the_restatement_is_the_plane_bands(shuffled):
    Hh, Ww, ncc, disp, planes, conn = _ncc_case(shuffled)
    offsets = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
    want = PB.inputs_ncc(ncc, disp, 3.0, planes, offsets, conn)
    im0, im1 = PB.images(Hh, Ww, 3, 2)
    want_gs = PB.inputs_globalstereo(im0, im1, PB.P2_example(), *PB.GS_DYADIC, 30.0, planes, offsets, conn)
    labels = np.random.default_rng(5).integers(1, 6, size=Hh * Ww)
    for sources, taps in (((), ()), ((planes,), ()), ((), ((0, 1),))):
        pcand = R.gather(planes, offsets, (Hh, Ww), sources, taps)
        assert pcand.shape == (4, 5, Hh * Ww)
        for g, w in zip(R.inputs_ncc(ncc, disp, 3.0, pcand, conn), want):
            assert same_bits(g, w)
        for g, w in zip(R.inputs_globalstereo(im0, im1, PB.P2_example(), *PB.GS_DYADIC, 30.0, pcand, conn), want_gs):
            assert same_bits(g, w)
        assert same_bits(R.apply(pcand, labels), PB.apply(planes, labels, offsets))
    with pytest.raises(ValueError):
        R.apply(pcand, np.full(Hh * Ww, 6))


def test_with_a_fronto_parallel_table_the_restatement_is_the_candidate_bands():
    """the table fronto(cand_k) gives candidates_restate.candidates_inputs byte for byte, the sign of zero included"""
    Hh, Ww, ncc, disp, _, conn = _ncc_case(False)
    base = band_restate.base_map(Hh, Ww, 6, 2.0, 3)
    other = np.arange(Hh * Ww, dtype=np.float64).reshape(Hh, Ww) / 4.0
    other[0, 0] = -0.0
    offsets, taps = np.array([-0.5, 0.0, 0.5]), [(0, 0), (1, 0), (0, -1), (9, -9)]
    cand = CR.gather(base, offsets, [base, other], taps)
    assert (cand == 0).any()
    pcand = R.table_of(cand)
    assert pcand.shape == (4, 3 + 2 * 4, Hh * Ww) and same_bits(pcand[:, 4, :], R.fronto(CR.candidates_apply(cand, np.full(Hh * Ww, 5), (Hh, Ww))))
    want = CR.candidates_inputs(ncc, disp, 3.0, cand, (Hh, Ww), conn)
    for g, w in zip(R.inputs_ncc(ncc, disp, 3.0, pcand, conn), want):
        assert same_bits(g, w)
    zero = want[1] == 0
    assert zero.any() and np.signbit(want[1][zero]).all()
    # gathered from fronto-parallel planes it is the same table but for rounding: base + offset against -(-base - offset)
    got = R.gather(R.fronto(base), offsets, (Hh, Ww), [R.fronto(base), R.fronto(other)], taps)
    assert same_bits(got[:, 3:, :], pcand[:, 3:, :]) and same_bits(-got[3, :3, :], cand[:3])


def test_the_zero_tap_of_the_base_duplicates_the_zero_offset_and_taps_beyond_the_image_clamp():
    Hh, Ww = 5, 7
    N = Hh * Ww
    planes = PB.planes_through(band_restate.base_map(Hh, Ww, 6, 2.0, 3), 4)
    other = PB.planes_through(band_restate.base_map(Hh, Ww, 6, 2.0, 8), 9, dyadic=False)
    offsets = np.array([-0.5, 0.0, 0.5])
    taps = [(0, 0), (1, 0), (0, -1), (-9, 0), (0, 9), (9, -9)]
    pcand = R.gather(planes, offsets, (Hh, Ww), [planes, other], taps)
    assert pcand.shape == (4, 3 + 2 * 6, N)
    # tap (0, 0) of the base is the offset 0.0: the copy is the plane's bits, d - c * 0.0 the plane's value (a d of -0
    # with a negative c comes out as +0, the plane band's own arithmetic)
    assert same_bits(pcand[:, 3], planes) and np.array_equal(pcand[:, 1], planes) and (planes[3] == 0).any()
    assert same_bits(pcand[:, 1][:, planes[3] != 0], planes[:, planes[3] != 0])
    assert same_bits(pcand[:3, 0], planes[:3]) and same_bits(pcand[3, 0], planes[3] - planes[2] * -0.5)
    img = lambda rows: rows.reshape(4, Ww, Hh).transpose(0, 2, 1)                          # 4 x H x W
    src = img(planes)
    assert same_bits(img(pcand[:, 4])[:, :-1], src[:, 1:]) and same_bits(img(pcand[:, 4])[:, -1], src[:, -1])      # (1, 0): the row below
    assert same_bits(img(pcand[:, 5])[:, :, 1:], src[:, :, :-1]) and same_bits(img(pcand[:, 5])[:, :, 0], src[:, :, 0])
    assert same_bits(img(pcand[:, 6]), np.tile(src[:, :1], (1, Hh, 1)))                    # beyond the top: row 0
    assert same_bits(img(pcand[:, 7]), np.tile(src[:, :, -1:], (1, 1, Ww)))                # beyond the right: the last column
    assert same_bits(img(pcand[:, 8]), np.tile(src[:, -1:, :1], (1, Hh, Ww)))              # a corner
    assert same_bits(pcand[:, 9], other)                     # the second source follows the first one's T rows, copied
    # a label that selects a tap applies the neighbour's plane, nothing re-anchored
    assert same_bits(R.apply(pcand, np.full(N, 5)), pcand[:, 4])
    # equal neighbours give equal rows: duplicates are not removed
    flat = PB.slanted_map(Hh, Ww)
    dup = R.gather(flat, [0.0], (Hh, Ww), [flat], [(0, 1), (1, 0)])
    assert dup.shape == (4, 3, N) and same_bits(dup, np.repeat(flat[:, None, :], 3, axis=1))
    # a copied plane is the neighbour's surface extended to this pixel: on one slanted plane q == qprim for every tap label
    from oracle import terms as OT
    conn = np.stack(OT.construct_neighborhood(Hh, Ww))
    _, q, qprim = R.inputs_ncc(band_restate.volume(Hh, Ww, 6, 1), band_restate.disparities_for(6, False), 1.0, dup, conn)
    assert same_bits(q, qprim)


# ---------------------------------------------------------------- the chain

def chain_problems(shape):
    c = R.chain(shape)
    pcand = R.gather(c["base"], c["level"]["offsets"], shape, [c["base"]], c["level"]["taps"])
    cand = CR.gather(c["base_disp"], c["fronto_level"]["offsets"], [c["base_disp"]], c["fronto_level"]["taps"])
    mk = lambda u, q, qp: dict(unary=np.ascontiguousarray(u.T), conn=c["conn"].T.copy(), q=np.ascontiguousarray(q.T),
                               qprim=np.ascontiguousarray(qp.T), alphas=np.ones(R.CHAIN_N - 1), lam=R.CHAIN_LAMBDA)
    return (c, pcand, mk(*R.inputs_ncc(c["ncc"], c["disp"], R.CHAIN_WEIGHT, pcand, c["conn"])),
            mk(*PB.inputs_ncc(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base"], R.CHAIN_BAND, c["conn"])),
            mk(*CR.candidates_inputs(c["ncc"], c["disp"], R.CHAIN_WEIGHT, cand, shape, c["conn"])))


@pytest.mark.parametrize("shape", [(1, 17), (17, 1)], ids=lambda s: "%dx%d" % s)
def test_the_slanted_chain_has_the_true_planes_as_its_optimum_and_neither_band_reaches_it(shape, oracle):
    """Every number is dyadic: the volume is a multiple of 2^-7 with slices one apart, plane components, points, taps'
    planes and offsets are multiples of 1/2 below 2^5, so disparities are multiples of 1/2 below 2^6, a sample is a
    multiple of 2^-10 below 2^11 and a unary (weight 4, or 4 (1 + 1e6)) one of 2^-8 below 2^23; squared position
    differences are multiples of 2^-2, truncated at 2.  Sums of 17 + 16 such terms need under 40 bits: fp64 holds every
    energy and message exactly."""
    c, pcand, p, p_band, p_fronto = chain_problems(shape)
    assert pcand.shape == (4, 9, 17)
    # the true plane is a candidate at every pixel
    is_true = (pcand == c["truth"][:, None, :]).all(axis=0)
    assert is_true.any(axis=0).all()
    wrong = (c["base"] != c["truth"]).any(axis=0)
    assert wrong.sum() == 9 and np.abs(c["base_disp"].reshape(-1) - c["true_disp"])[wrong].tolist() == [6.0] * 9
    true_labels = is_true.argmax(axis=0)
    for kernel, band_opt in ((1, 57.67578125), (2, 57.41796875)):
        assert fp.energy_exact(p, kernel, R.CHAIN_LAMBDA, true_labels) == Fraction(2)      # unary 0 everywhere, one truncated step
        opt, _ = fp.chain_dp(p, kernel, R.CHAIN_LAMBDA)
        opt_band, _ = fp.chain_dp(p_band, kernel, R.CHAIN_LAMBDA)
        opt_fronto, _ = fp.chain_dp(p_fronto, kernel, R.CHAIN_LAMBDA)
        print("chain %dx%d kernel %d: plane candidates %r, plane band %r, candidate band %r" % (shape + (kernel, opt, opt_band, opt_fronto)))
        assert opt == 2.0 and opt_band == band_opt and opt_fronto == 57.65625
        labels, en, lb, it = oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], R.CHAIN_LAMBDA, 3, NEVER, mode=1)
        print("   oracle: energy %r, bound %r, %d iteration(s)" % (en, lb, it))
        assert en == lb == 2.0 and it <= 3
        assert same_bits(R.apply(pcand, labels), c["truth"])
