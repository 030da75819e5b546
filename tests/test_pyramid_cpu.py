"""The image pyramid without a device: the restatement of the two definitions (tests/pyramid_restate.py)
against what they mean on even sizes, the level-model identity through oracle.terms, the refusal rules of the four C
entries (arguments are checked before the device is looked for), the ABI numbers, and the arguments
solve_pair_ncc_pyramid refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyramid_restate as R
from oracle import terms as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement

@pytest.mark.parametrize("shape", [(2, 2, 1), (6, 8, 3), (12, 4, 2)], ids=str)
def test_restated_reduce_of_an_even_image_is_the_block_mean(shape):
    H, W, Cn = shape
    im = np.random.default_rng(H * W).integers(0, 256, size=shape).astype(np.float64)
    want = im.reshape(H // 2, 2, W // 2, 2, Cn).sum(axis=(1, 3)) / 4.0          # integers below 1024: every sum is exact
    got = R.reduce(im)
    assert got.shape == (H // 2, W // 2, Cn) and np.array_equal(got, want)
    assert np.array_equal(got * 4.0, np.rint(got * 4.0))


def test_restated_reduce_replicates_the_last_row_and_column():
    im = np.arange(15, dtype=np.float64).reshape(3, 5, 1)
    got = R.reduce(im)
    assert got.shape == (2, 3, 1)
    assert got[1, 2, 0] == im[2, 4, 0] and got[0, 2, 0] == (im[0, 4, 0] + im[1, 4, 0]) / 2.0
    assert got[1, 0, 0] == (im[2, 0, 0] + im[2, 1, 0]) / 2.0


@pytest.mark.parametrize("shape", [(2, 2), (6, 8), (12, 4)], ids=str)
def test_restated_nearest_expand_is_twice_the_repeat(shape):
    H, W = shape
    d = np.random.default_rng(H + W).integers(0, 64, size=(H // 2, W // 2)) / 4.0
    out, source = R.expand(d, (H, W), 0)
    assert np.array_equal(out, 2.0 * np.repeat(np.repeat(d, 2, axis=0), 2, axis=1))
    assert source.dtype == np.int32 and (source == 0).all()


def test_restated_candidates():
    assert R.candidates(0, 0, 3, 4) == [(0, 0), (0, 0), (0, 0), (0, 0)]                  # both neighbours clamped onto the parent
    assert R.candidates(3, 2, 3, 4) == [(1, 1), (2, 1), (1, 0), (2, 0)]                  # odd y: below; even x: left
    assert R.candidates(5, 7, 3, 4) == [(2, 3), (2, 3), (2, 3), (2, 3)]                  # the last pixel of an even size
    assert R.candidates(4, 6, 3, 4) == [(2, 3), (1, 3), (2, 2), (1, 2)]                  # H = 5: the replicated row's parent


# ---------------------------------------------------------------- the level model

def pairwise_sum(kernel, weight, tol, dispmap):
    """The smoothness term of a fronto-parallel map on the image grid, through the oracle's restatement of the
    reference (every directed edge of construct_neighborhood, weight `weight`)."""
    H, W = dispmap.shape
    ind1, ind2 = OT.construct_neighborhood(H, W)
    a = np.zeros((4, H * W))
    a[2] = 1.0
    a[3] = -dispmap.T.reshape(-1)
    E00 = OT.all_pairwise_costs(kernel, np.full(ind1.shape[0], weight), tol, a, a, ind1, ind2, OT.get_points(H, W))[0]
    return float(E00.sum())


@pytest.mark.parametrize("tol", [3.0, 8.0, 0.5])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("kernel", [1, 2])
def test_level_model_identity_is_exact(kernel, level, tol):
    """Restricted to maps that are constant on s x s blocks, the fine energy's smoothness term is s^2 times the level
    model's: dyadic maps (multiples of 1/4 below 8) on 6 x 10 coarse pixels keep every term a multiple of 2^-4 below
    2^12 and every sum exact."""
    from stereo_amd import pyramid
    s = 2 ** level
    coarse = np.random.default_rng([kernel, level]).integers(0, 32, size=(6, 10)) / 4.0
    fine = coarse
    for _ in range(level):
        fine = R.expand(fine, (2 * fine.shape[0], 2 * fine.shape[1]), 0)[0]
    assert fine.shape == (6 * s, 10 * s) and np.array_equal(fine, s * np.repeat(np.repeat(coarse, s, axis=0), s, axis=1))
    tol_l, weight = R.level_model(kernel, tol, level)
    assert (tol_l, weight) == (tol / s ** kernel, float(s ** (kernel - 1)))
    assert pyramid.level_model(kernel, tol, level) == (tol_l, weight)
    fine_sum = pairwise_sum(kernel, 1.0, tol, fine)
    coarse_sum = pairwise_sum(kernel, weight, tol_l, coarse)
    assert fine_sum > 0 and fine_sum == s * s * coarse_sum


def test_level_disparities():
    from stereo_amd import pyramid
    d = np.arange(8, dtype=np.float64)
    for fn in (R.level_disparities, pyramid.level_disparities):
        assert np.array_equal(fn(d, 0), d)                               # level 0: the caller's own slices
        assert fn(d, 1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]            # ceil(7 / 2) = 4
        assert fn(d, 2).tolist() == [0.0, 1.0, 2.0]
        assert fn(np.arange(256.0), 2).shape == (65,)                    # 0 .. ceil(255 / 4) = 64: one past the K <= 64 family
        assert fn(np.array([-3.0, 5.5]), 1).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0, 3.0]
        assert fn(d, 1).dtype == np.float64


# ---------------------------------------------------------------- refusals of the C entries

def _lib():
    from stereo_amd import _lib
    return _lib.lib()


def _call(fn, *args):
    err = C.create_string_buffer(512)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _arrays(device_form, n=7):
    """Arrays the entries may be handed: never read here (every call is refused before the device is looked for), but
    real memory of the right kind all the same -- device memory for the device forms where a device exists."""
    import stereo_amd
    if device_form and stereo_amd.device_count() > 0:
        import torch
        keep = [torch.zeros(64, dtype=torch.float64, device="cuda") for _ in range(n)]
        return keep, [C.c_void_p(t.data_ptr()) for t in keep]
    keep = [np.zeros(64) for _ in range(n)]
    return keep, [C.c_void_p(a.ctypes.data) for a in keep]


BAD_REDUCE = [
    (dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(C=0), "at least 1"), (dict(H=-2), "at least 1"),
    (dict(H=65536, W=32768), "2\\^31"), (dict(im=None), "NULL"), (dict(out=None), "NULL"), (dict(out="im"), "alias"),
]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_REDUCE)
def test_reduce_refusals(device_form, change, match):
    keep, (im, out) = _arrays(device_form, 2)
    v = dict(im=im, H=3, W=4, C=2, out=out)
    v.update(change)
    if v["out"] == "im":
        v["out"] = v["im"]
    args = [v["im"], C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["C"]), v["out"]]
    if device_form:
        args.append(None)
    name = "stereo_pyramid_reduce_device" if device_form else "stereo_pyramid_reduce"
    rc, msg = _call(getattr(_lib(), name), *args)
    assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), msg
    assert _lib().stereo_hip_last_error().decode() == msg


BAD_EXPAND = [
    (dict(H=0, Hc=0), "at least 1"), (dict(W=0, Wc=0), "at least 1"), (dict(C=0), "at least 1"),
    (dict(H=65536, W=32768, Hc=32768, Wc=16384), "2\\^31"),
    (dict(d_coarse=None), "NULL"), (dict(out=None), "NULL"), (dict(im_fine=None), "NULL"), (dict(im_coarse=None), "NULL"),
    (dict(Hc=2), "sizes do not match"), (dict(Wc=3), "sizes do not match"), (dict(H=7, W=8), "sizes do not match"),
    (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
    (dict(out="d_coarse"), "alias"), (dict(out="im_fine"), "alias"), (dict(out="im_coarse"), "alias"),
    (dict(source="d_coarse"), "alias"), (dict(source="out"), "alias"), (dict(source="im_fine"), "alias"),
    (dict(mode=0, out="d_coarse"), "alias"), (dict(mode=0, C=0), "at least 1"),
]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_EXPAND, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_expand_refusals(device_form, change, match):
    keep, (d, f, g, out, src) = _arrays(device_form, 5)
    v = dict(d_coarse=d, Hc=3, Wc=4, H=5, W=7, mode=1, im_fine=f, im_coarse=g, C=1, out=out, source=src)
    v.update(change)
    for key in ("out", "source"):
        if isinstance(v[key], str):
            v[key] = v[v[key]]
    args = [v["d_coarse"], C.c_int(v["Hc"]), C.c_int(v["Wc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["mode"]),
            v["im_fine"], v["im_coarse"], C.c_int(v["C"]), v["out"], v["source"]]
    if device_form:
        args.append(None)
    name = "stereo_pyramid_expand_device" if device_form else "stereo_pyramid_expand"
    rc, msg = _call(getattr(_lib(), name), *args)
    assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), msg
    assert _lib().stereo_hip_last_error().decode() == msg


def test_python_wrappers_refuse_before_the_device():
    from stereo_amd import pyramid, StereoHipError
    with pytest.raises(StereoHipError, match="H x W x C"):
        pyramid.reduce(np.zeros(4))
    with pytest.raises(StereoHipError, match="sizes do not match"):
        pyramid.expand(np.zeros((3, 4)), (5, 9), "nearest")
    with pytest.raises(StereoHipError, match="needs im_fine"):
        pyramid.expand(np.zeros((3, 4)), (5, 7), "guided")
    with pytest.raises(StereoHipError, match="same C"):
        pyramid.expand(np.zeros((3, 4)), (5, 7), "guided", np.zeros((5, 7, 3)), np.zeros((3, 4, 1)))
    with pytest.raises(StereoHipError, match="'nearest' or 'guided'"):
        pyramid.expand(np.zeros((3, 4)), (5, 7), "bilinear")
    with pytest.raises(StereoHipError, match="mode"):
        pyramid.expand(np.zeros((3, 4)), (5, 7), 2)


def test_the_three_abi_numbers_agree_and_count_the_new_section():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 14
    for name in ("stereo_pyramid_reduce", "stereo_pyramid_expand", "stereo_pyramid_reduce_device", "stereo_pyramid_expand_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the solve's arguments

def test_solve_pair_ncc_pyramid_refuses_its_arguments_first():
    import stereo_amd
    from stereo_amd import StereoHipError
    im = np.zeros((8, 12, 3))
    args = ([im, im], np.arange(4.0), 1, 40.0, 2.0)
    for levels in (0, 6, -1, 1.5, True, None):
        with pytest.raises(StereoHipError, match="levels"):
            stereo_amd.solve_pair_ncc_pyramid(*args, levels, 3, 0.0)
    with pytest.raises(StereoHipError, match="expand"):
        stereo_amd.solve_pair_ncc_pyramid(*args, 1, 3, 0.0, expand="bilinear")
    with pytest.raises(StereoHipError, match="expand"):
        stereo_amd.solve_pair_ncc_pyramid(*args, 1, 3, 0.0, expand=1)
    band = [-1.0, 0.0, 1.0]
    malformed = [
        [[band]],                             # one level's bands for two reductions
        [[band], [band], [band]],             # three
        [[band], []],                         # a level without a vector
        [[band], band],                       # numbers where vectors belong
        [[band], [[0.0, -1.0, 1.0]]],         # not ascending
        [[band], [[1.0, 2.0]]],               # without 0
        [[band], [[-1.0, 0.0, np.nan]]],      # not finite
        [[band], [[[0.0]]]],                  # a matrix
        {0: [band], 1: [band]},               # not a sequence
        5,
    ]
    for bands in malformed:
        with pytest.raises(StereoHipError, match="bands|offsets|vector"):
            stereo_amd.solve_pair_ncc_pyramid(*args, 2, 3, 0.0, bands=bands)
    with pytest.raises(StereoHipError, match="maxiter"):
        stereo_amd.solve_pair_ncc_pyramid(*args, 2, [3, 3], 0.0)
    with pytest.raises(StereoHipError, match="two views"):
        stereo_amd.solve_pair_ncc_pyramid([im], np.arange(4.0), 1, 40.0, 2.0, 1, 3, 0.0)
    with pytest.raises(StereoHipError, match="one size"):
        stereo_amd.solve_pair_ncc_pyramid([im, np.zeros((8, 13, 3))], np.arange(4.0), 1, 40.0, 2.0, 1, 3, 0.0)
    with pytest.raises(StereoHipError, match="kernels 1 and 2"):
        stereo_amd.solve_pair_ncc_pyramid([im, im], np.arange(4.0), 3, 40.0, 2.0, 1, 3, 0.0)
    assert "solve_pair_ncc_pyramid" in stereo_amd.__all__


def test_solve_pyramid_refuses_what_it_is_not_defined_for():
    import stereo_amd
    from stereo_amd import StereoHipError
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(StereoHipError, match="dispmap_globalstereo reaches its second view through a projection"):
        glob.solve_pyramid(1)
    ncc = object.__new__(stereo_amd.dispmap_ncc)
    ncc._smooth_weights = np.array([1.0, 2.0])
    with pytest.raises(StereoHipError, match="smooth_weights"):
        ncc.solve_pyramid(1)
