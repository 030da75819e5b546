"""Left-right consistency without a device: the restatement of the two definitions (tests/lr_restate.py) on the
two-plane scene against the geometric answer written out, the refusal rules of the four C entries (arguments are
checked before the device is looked for), and the ABI numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lr_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# background d = 2, box d = 6 at left columns 20-29 = right columns 14-23, 40 columns
LEFT_STATUS = [3, 3] + [0] * 14 + [1] * 4 + [0] * 20
RIGHT_STATUS = [0] * 24 + [1] * 4 + [0] * 10 + [3, 3]
LEFT_RESIDUAL = [np.nan, np.nan] + [0.0] * 14 + [-4.0] * 4 + [0.0] * 20
RIGHT_RESIDUAL = [0.0] * 24 + [-4.0] * 4 + [0.0] * 10 + [np.nan, np.nan]
LEFT_FILLED = [2.0] * 20 + [6.0] * 10 + [2.0] * 10
LEFT_SOURCE = [2, 2] + list(range(2, 16)) + [15] * 4 + list(range(20, 40))
RIGHT_FILLED = [2.0] * 14 + [6.0] * 10 + [2.0] * 16
RIGHT_SOURCE = list(range(24)) + [28] * 4 + list(range(28, 38)) + [37, 37]

SCENE = dict(left=(1, LEFT_STATUS, LEFT_RESIDUAL, LEFT_FILLED, LEFT_SOURCE),
             right=(-1, RIGHT_STATUS, RIGHT_RESIDUAL, RIGHT_FILLED, RIGHT_SOURCE))


def scene_maps(view, H=3):
    left, right = lr_restate.two_plane_scene(H)
    return (left, right) if view == "left" else (right, left)


@pytest.mark.parametrize("view", ["left", "right"])
@pytest.mark.parametrize("tol", [0.0, 1.0])
def test_restatement_gives_the_geometric_answer_on_the_two_plane_scene(view, tol):
    direction, status, residual, filled, source = SCENE[view]
    ref, other = scene_maps(view)
    st, res = lr_restate.lr_check(ref, other, direction, tol)
    fl, src = lr_restate.lr_fill(ref, st)
    for y in range(ref.shape[0]):
        assert st[y].tolist() == status
        assert lr_restate.same(res[y], np.array(residual))
        assert fl[y].tolist() == filled
        assert src[y].tolist() == source
    assert st.dtype == np.int32 and src.dtype == np.int32


def test_restatement_details():
    # ties of the nearest column go to the higher index: x - d = 1.5 -> column 2
    ref = np.array([[0.0, 0.0, 0.0, 1.5]])
    other = np.array([[9.0, 9.0, 1.5, 9.0]])
    st, res = lr_restate.lr_check(ref, other, 1, 0.0)
    assert st[0, 3] == 0 and res[0, 3] == 0.0
    # a row without a consistent pixel, and equal disparities on both sides: the left one
    st = np.array([[1, 2, 3], [0, 1, 0]], np.int32)
    fl, src = lr_restate.lr_fill(np.array([[1.0, 2.0, 3.0], [5.0, 7.0, 5.0]]), st)
    assert np.isnan(fl[0]).all() and src[0].tolist() == [-1, -1, -1]
    assert fl[1].tolist() == [5.0, 5.0, 5.0] and src[1].tolist() == [0, 0, 2]


def _lib():
    from stereo_amd import _lib
    return _lib.lib()


def _call(fn, *args):
    err = C.create_string_buffer(512)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _arrays():
    """Arrays the entries may be handed: never read here (every call below is refused before the device is looked
    for), but real memory of the right kind all the same -- device memory where a device exists."""
    import stereo_amd
    n = 12
    if stereo_amd.device_count() > 0:
        import torch
        keep = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
        keep += [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        return keep, [C.c_void_p(t.data_ptr()) for t in keep]
    keep = [np.zeros(n) for _ in range(3)] + [np.zeros(n, np.int32) for _ in range(2)]
    return keep, [C.c_void_p(a.ctypes.data) for a in keep]


BAD_CHECK = [
    (dict(direction=0), "direction"), (dict(direction=2), "direction"), (dict(tol=-1.0), "tol"),
    (dict(tol=float("nan")), "tol"), (dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(W=-3), "at least 1"),
    (dict(H=65536, W=32768), "2\\^31"), (dict(d_ref=None), "NULL"), (dict(d_other=None), "NULL"),
    (dict(status=None), "NULL"),
]
BAD_FILL = [
    (dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(H=46341, W=46341), "2\\^31"), (dict(d_ref=None), "NULL"),
    (dict(status=None), "NULL"), (dict(filled=None), "NULL"),
]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_CHECK)
def test_check_refusals(device_form, change, match):
    keep, (a, b, res, st, _) = _arrays()
    host_keep = [np.zeros(12) for _ in range(3)] + [np.zeros(12, np.int32)]
    if not device_form:       # the host form reads host memory
        a, b, res = (C.c_void_p(x.ctypes.data) for x in host_keep[:3])
        st = C.c_void_p(host_keep[3].ctypes.data)
    v = dict(d_ref=a, d_other=b, H=3, W=4, direction=1, tol=1.0, status=st, residual=res)
    v.update(change)
    args = [v["d_ref"], v["d_other"], C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["direction"]), C.c_double(v["tol"]),
            v["status"], v["residual"]]
    if device_form:
        args.append(None)
    rc, msg = _call(_lib().stereo_lr_check_device if device_form else _lib().stereo_lr_check, *args)
    assert rc != 0 and re.search(match, msg), msg
    assert _lib().stereo_hip_last_error().decode() == msg


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_FILL)
def test_fill_refusals(device_form, change, match):
    keep, (a, _, out, st, src) = _arrays()
    host_keep = [np.zeros(12), np.zeros(12), np.zeros(12, np.int32), np.zeros(12, np.int32)]
    if not device_form:
        a, out = C.c_void_p(host_keep[0].ctypes.data), C.c_void_p(host_keep[1].ctypes.data)
        st, src = C.c_void_p(host_keep[2].ctypes.data), C.c_void_p(host_keep[3].ctypes.data)
    v = dict(d_ref=a, status=st, H=3, W=4, filled=out, source=src)
    v.update(change)
    args = [v["d_ref"], v["status"], C.c_int(v["H"]), C.c_int(v["W"]), v["filled"], v["source"]]
    if device_form:
        args.append(None)
    rc, msg = _call(_lib().stereo_lr_fill_device if device_form else _lib().stereo_lr_fill, *args)
    assert rc != 0 and re.search(match, msg), msg


def test_fill_chunks_hook_refuses_a_count_outside_the_workgroup():
    keep, (a, _, out, st, src) = _arrays()
    for chunks in (0, -1, 17):
        rc, msg = _call(_lib().stereo_lr_fill_device_chunks, a, st, C.c_int(3), C.c_int(4), out, src, C.c_int(chunks), None)
        assert rc != 0 and "chunks" in msg
    assert 1 <= _lib().stereo_lr_fill_chunks() <= 16


def test_fill_refuses_in_place_use():
    keep, (a, _, out, st, src) = _arrays()
    for fn, tail in ((_lib().stereo_lr_fill_device, [None]), ):
        rc, msg = _call(fn, a, st, C.c_int(3), C.c_int(4), a, src, *tail)
        assert rc != 0 and "in place" in msg
        rc, msg = _call(fn, a, st, C.c_int(3), C.c_int(4), out, st, *tail)
        assert rc != 0 and "in place" in msg
    d, s = np.zeros(12), np.zeros(12, np.int32)
    pd, ps = C.c_void_p(d.ctypes.data), C.c_void_p(s.ctypes.data)
    rc, msg = _call(_lib().stereo_lr_fill, pd, ps, C.c_int(3), C.c_int(4), pd, None)
    assert rc != 0 and "in place" in msg
    rc, msg = _call(_lib().stereo_lr_fill, pd, ps, C.c_int(3), C.c_int(4), C.c_void_p(np.zeros(12).ctypes.data), ps)
    assert rc != 0 and "in place" in msg


def test_solve_pair_ncc_checks_its_images_first():
    import stereo_amd
    from stereo_amd import StereoHipError
    im = np.zeros((4, 6, 3))
    with pytest.raises(StereoHipError, match="two views"):
        stereo_amd.solve_pair_ncc([im], np.arange(3.0), 1, 40.0, 2.0, 1, 0.0)
    with pytest.raises(StereoHipError, match="one size"):
        stereo_amd.solve_pair_ncc([im, np.zeros((4, 7, 3))], np.arange(3.0), 1, 40.0, 2.0, 1, 0.0)
    with pytest.raises(StereoHipError, match="one size"):
        stereo_amd.solve_pair_ncc([im[:, :, 0], im[:, :, 0]], np.arange(3.0), 1, 40.0, 2.0, 1, 0.0)


def test_python_wrappers_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import StereoHipError
    m = np.zeros((3, 4))
    with pytest.raises(StereoHipError, match="direction"):
        stereo_amd.lr_check(m, m, 0, 1.0)
    with pytest.raises(StereoHipError, match="tol"):
        stereo_amd.lr_check(m, m, 1, -0.5)
    with pytest.raises(StereoHipError, match="same size"):
        stereo_amd.lr_check(m, np.zeros((3, 5)), 1, 1.0)
    with pytest.raises(StereoHipError, match="H x W"):
        stereo_amd.lr_check(np.zeros(4), np.zeros(4), 1, 1.0)
    with pytest.raises(StereoHipError, match="status must have"):
        stereo_amd.lr_fill(m, np.zeros((4, 3), np.int32))
    for name in ("lr_check", "lr_fill", "lr_check_device", "lr_fill_device", "solve_pair_ncc"):
        assert name in stereo_amd.__all__ and callable(getattr(stereo_amd, name))
    assert callable(stereo_amd.dispmap_ncc.mirrored) and callable(stereo_amd.dispmap_super.cross_check)


def test_cross_check_refuses_what_it_is_not_defined_for():
    import stereo_amd
    from stereo_amd import StereoHipError
    ncc = object.__new__(stereo_amd.dispmap_ncc)
    ncc.sz = (4, 5)
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    glob.sz = (4, 5)
    with pytest.raises(StereoHipError, match="dispmap_globalstereo reaches its second view through a projection"):
        glob.cross_check(ncc)
    with pytest.raises(StereoHipError, match="dispmap_globalstereo"):
        ncc.cross_check(glob)
    other = object.__new__(stereo_amd.dispmap_ncc)
    other.sz = (4, 6)
    with pytest.raises(StereoHipError, match="sizes differ"):
        ncc.cross_check(other)


def test_the_three_abi_numbers_agree_and_count_the_new_section():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 11
    for name in ("stereo_lr_check", "stereo_lr_fill", "stereo_lr_check_device", "stereo_lr_fill_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
