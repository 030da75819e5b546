"""Band refinement without a device: every refusal of the C entries and the Python wrappers (the
arguments are checked before the device is looked for), the restatement of the definition (tests/band_restate.py)
against the oracle's unary of the per-pixel planes, and the ABI numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import band_restate
from oracle import terms as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, E = 3, 4, 5, 2


def _lib():
    from stereo_amd import _lib as L
    return L.lib()


def _call(fn, *args):
    err = C.create_string_buffer(1024)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _host():
    """keep-alive arrays and the argument values of a valid call"""
    a = dict(ncc=np.zeros(H * W * D), disparities=np.arange(D, dtype=np.float64), base=np.zeros(H * W),
             offsets=np.array([-0.5, 0.0, 0.5]), conn=np.array([0, 1, 1, 2], np.uint32), unary=np.zeros(3 * H * W),
             q=np.zeros(3 * E), qprim=np.zeros(3 * E), labels=np.ones(H * W, np.int32), refined=np.zeros(H * W))
    return a


def _inputs_args(a, v, device_form):
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    args = [p(v["ncc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["D"]), C.c_int(v["layout"]), p(v["disparities"])]
    if device_form:
        args.append(p(v["disparities"]))          # (never read: the call is refused before the device is looked for)
    args += [C.c_double(1.0), p(v["base"]), p(v["offsets"])]
    if device_form:
        args.append(p(v["offsets"]))
    args += [C.c_int(v["K"] if v["K"] is not None else (0 if v["offsets"] is None else len(v["offsets"]))), C.c_int64(v["E"]),
             p(v["conn"]), p(v["unary"]), p(v["q"]), p(v["qprim"])]
    if device_form:
        args += [None, None]
    return args


def _apply_args(a, v, device_form):
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    args = [p(v["base"]), C.c_int(v["H"]), C.c_int(v["W"]), p(v["labels"]), p(v["offsets"])]
    if device_form:
        args.append(p(v["offsets"]))
    args += [C.c_int(v["K"] if v["K"] is not None else (0 if v["offsets"] is None else len(v["offsets"]))), p(v["refined"])]
    if device_form:
        args += [None, None]
    return args


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
    (dict(H=0), "H and W"),
    (dict(W=0), "H and W"),
    (dict(W=-2), "H and W"),
    (dict(H=1 << 16, W=1 << 15), r"2\^31"),
    (dict(base=None), "NULL"),
]
INPUT_REFUSALS = OFFSET_REFUSALS + [
    (dict(layout=2), "layout"),
    (dict(layout=-1), "layout"),
    (dict(D=0), "D must be"),
    (dict(E=-1), "E must not"),
    (dict(ncc=None), "NULL"),
    (dict(disparities=None), "NULL"),
    (dict(unary=None), "NULL"),
    (dict(conn=None), "NULL"),
    (dict(q=None), "NULL"),
    (dict(qprim=None), "NULL"),
]
APPLY_REFUSALS = OFFSET_REFUSALS + [(dict(labels=None), "NULL"), (dict(refined=None), "NULL")]


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,match", INPUT_REFUSALS, ids=lambda c: None if isinstance(c, str) else ",".join(sorted(c)))
def test_inputs_refusals(device_form, change, match):
    a = _host()
    v = dict(a, H=H, W=W, D=D, layout=0, K=None, E=E)
    v.update(change)
    fn = _lib().stereo_band_inputs_device if device_form else _lib().stereo_band_inputs
    rc, msg = _call(fn, *_inputs_args(a, v, device_form))
    assert rc != 0 and re.search(match, msg), msg
    assert msg.startswith("stereo_band_inputs_device" if device_form else "stereo_band_inputs:")


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,match", APPLY_REFUSALS, ids=lambda c: None if isinstance(c, str) else ",".join(sorted(c)))
def test_apply_refusals(device_form, change, match):
    a = _host()
    v = dict(a, H=H, W=W, K=None)
    v.update(change)
    fn = _lib().stereo_band_apply_device if device_form else _lib().stereo_band_apply
    rc, msg = _call(fn, *_apply_args(a, v, device_form))
    assert rc != 0 and re.search(match, msg), msg


def test_device_forms_want_the_device_copies_of_the_short_vectors():
    a = _host()
    v = dict(a, H=H, W=W, D=D, layout=0, K=None, E=E)
    args = _inputs_args(a, v, True)
    args[6] = None
    rc, msg = _call(_lib().stereo_band_inputs_device, *args)
    assert rc != 0 and "d_disparities" in msg
    args = _apply_args(a, v, True)
    args[5] = None
    rc, msg = _call(_lib().stereo_band_apply_device, *args)
    assert rc != 0 and "d_offsets" in msg


def test_host_entries_refuse_a_base_that_is_not_finite_and_name_the_pixel():
    for bad in (np.nan, np.inf, -np.inf):
        a = _host()
        a["base"][1 + H * 2] = bad                       # row 1, column 2
        v = dict(a, H=H, W=W, D=D, layout=0, K=None, E=E)
        rc, msg = _call(_lib().stereo_band_inputs, *_inputs_args(a, v, False))
        assert rc != 0 and "row 1, column 2" in msg, msg
        rc, msg = _call(_lib().stereo_band_apply, *_apply_args(a, v, False))
        assert rc != 0 and "row 1, column 2" in msg, msg


def test_host_entries_refuse_labels_and_edges_out_of_range():
    for lab in (0, 4, -1):
        a = _host()
        a["labels"][5] = lab
        rc, msg = _call(_lib().stereo_band_apply, *_apply_args(a, dict(a, H=H, W=W, K=None), False))
        assert rc != 0 and "outside 1 .. 3" in msg and "pixel 5" in msg, msg
    a = _host()
    a["conn"][3] = H * W
    rc, msg = _call(_lib().stereo_band_inputs, *_inputs_args(a, dict(a, H=H, W=W, D=D, layout=0, K=None, E=E), False))
    assert rc != 0 and "conn" in msg and "edge 1" in msg, msg


def test_python_wrappers_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import StereoHipError, band
    from stereo_amd import terms as T
    ncc, disp, base = np.zeros((H, W, D)), np.arange(D, dtype=np.float64), np.zeros((H, W))
    conn = T.construct_neighborhood(H, W)
    for offsets, match in (([0.0, 0.0], "strictly ascending"), ([1.0, 2.0], "contain 0"), ([np.nan, 0.0], "not finite"),
                           ([], "1 .. 512"), (np.arange(600.0), "1 .. 512")):
        with pytest.raises(StereoHipError, match=match):
            stereo_amd.band_inputs(ncc, disp, 1.0, base, offsets, conn)
        with pytest.raises(StereoHipError, match=match):
            stereo_amd.band_apply(base, np.ones(H * W), offsets)
    with pytest.raises(StereoHipError, match="layout"):
        stereo_amd.band_inputs(ncc, disp, 1.0, base, [0.0], conn, layout=3)
    with pytest.raises(StereoHipError, match="H x W x D"):
        stereo_amd.band_inputs(np.zeros((H, W + 1, D)), disp, 1.0, base, [0.0], conn)
    with pytest.raises(StereoHipError, match="D x"):
        stereo_amd.band_inputs(np.zeros((D, H * W + 1)), disp, 1.0, base, [0.0], conn, layout=1)
    with pytest.raises(StereoHipError, match="disparities for a volume"):
        stereo_amd.band_inputs(ncc, disp[:-1], 1.0, base, [0.0], conn)
    nan_base = base.copy()
    nan_base[2, 3] = np.nan
    with pytest.raises(StereoHipError, match="row 2, column 3"):
        stereo_amd.band_inputs(ncc, disp, 1.0, nan_base, [0.0], conn)
    with pytest.raises(StereoHipError, match="outside 1 .. 2"):
        stereo_amd.band_apply(base, np.full(H * W, 3.0), [0.0, 1.0])
    with pytest.raises(StereoHipError, match="whole numbers"):
        stereo_amd.band_apply(base, np.full(H * W, 1.5), [0.0, 1.0])
    with pytest.raises(StereoHipError, match="at least one"):
        band.check_levels([])
    assert band.max_offsets() == 512
    for name in ("band_inputs", "band_apply", "band_inputs_device", "band_apply_device", "refine_band"):
        assert name in stereo_amd.__all__ and callable(getattr(stereo_amd, name))
    assert callable(stereo_amd.dispmap_ncc.refine_band)


def test_globalstereo_refuses_band_refinement():
    import stereo_amd
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(stereo_amd.StereoHipError, match="dispmap_globalstereo does not take its unary from the NCC sampler"):
        glob.refine_band([[0.0]])


def test_solve_pair_ncc_checks_its_levels_first():
    import stereo_amd
    im = np.zeros((4, 6, 3))
    with pytest.raises(stereo_amd.StereoHipError, match="at least one"):
        stereo_amd.solve_pair_ncc([im, im], np.arange(3.0), 1, 40.0, 2.0, 1, 0.0, band_levels=[])


@pytest.mark.parametrize("shuffled", [False, True])
def test_restatement_rows_are_the_oracle_unary_of_the_per_pixel_planes(shuffled):
    Hh, Ww, Dd = 5, 7, 6
    ncc = band_restate.volume(Hh, Ww, Dd, 1)
    disp = band_restate.disparities_for(Dd, shuffled)
    offsets = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
    base = band_restate.base_map(Hh, Ww, Dd, 2.0, 3)
    ind1, ind2 = OT.construct_neighborhood(Hh, Ww)
    conn = np.stack([ind1, ind2])
    unary, q, qprim = band_restate.band_inputs(ncc, disp, 3.0, base, offsets, conn)
    assert unary.shape == (5, Hh * Ww) and q.shape == qprim.shape == (5, conn.shape[1])
    points = OT.get_points(Hh, Ww)
    b = base.T.reshape(-1)
    for k, delta in enumerate(offsets):
        P = np.zeros((4, Hh * Ww))
        P[2], P[3] = 1.0, -(b + delta)
        assert np.array_equal(OT.disparity_from_assignment(P, points), b + delta)      # the plane's disparity, exactly
        assert band_restate.same_bits(unary[k], OT.ncc_unary_cost(ncc, disp, 3.0, P, points))
        assert np.array_equal(q[k], b[ind2] + delta) and np.array_equal(qprim[k], b[ind1] + delta)
    # the crafted pixels do what they are there for: out of range costs unary_weight * (1 + 1e6), a slice costs its value
    out_of_range = 3.0 * (1.0 + 1e6)
    assert unary[2, 2] == out_of_range and unary[2, 3] == out_of_range        # base below / above the range
    assert unary[2, 4] != out_of_range and unary[3, 4] == out_of_range        # on the last slice: + 0.5 leaves the range
    if not shuffled:      # (the first slice: t2 == 1 gives the slice itself)
        assert unary[2, 5] == 3.0 * (1.0 - ncc.transpose(1, 0, 2).reshape(-1, Dd)[5, list(disp).index(2.0)])
    assert q[4][list(ind2).index(6)] == 0.0                                   # base -2 with offset +2
    assert band_restate.same(band_restate.band_apply(base, np.full(Hh * Ww, 4.0), offsets), base + 0.5)
    with pytest.raises(ValueError):
        band_restate.band_apply(base, np.full(Hh * Ww, 6.0), offsets)


def test_the_three_abi_numbers_agree_and_count_the_band_section():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 12
    for name in ("stereo_band_inputs", "stereo_band_apply", "stereo_band_inputs_device", "stereo_band_apply_device",
                 "stereo_band_max_offsets"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the sanitizer program

def test_builder_argument_checks_are_clean_under_sanitizers(tmp_path):
    """tools/sanitize_band_args.cpp: the checks and scans of the four level builders (band_common.h and the four .hip
    files) under ASan + UBSan on the host, a stand-alone program; no device call is made."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    exe = str(tmp_path / "sanitize_band_args")
    csrc = os.path.join(ROOT, "stereo_amd", "csrc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-w",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           *[os.path.join(csrc, name + ".hip") for name in ("band", "plane_band", "candidates", "plane_candidates")],
           os.path.join(ROOT, "tools", "sanitize_band_args.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_BAND_ARGS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
