"""A pyramid level's volume as the block mean of the finer one, without a device: the level-model
identity's unary half on the restatement (tests/pyramid_volume_restate.py), what two reductions are, the sample
positions of a level, the refusal rules of the two C entries (arguments are checked before the device is looked for)
and of the Python entries, and the ABI numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import band_restate
import pyramid_restate as R
import pyramid_volume_restate as RV
from oracle import terms as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, D = 8, 12, 9
SLICES = np.arange(3.0, 12.0)
WEIGHT = 40.0


def dyadic_levels():
    """The 6-bit dyadic volume and its two restated reductions, with each level's slices."""
    slices = [R.level_disparities(SLICES, l) for l in range(3)]
    vols = [band_restate.volume(H, W, D, 1)]
    for l in (1, 2):
        vols.append(RV.reduce_volume(vols[-1], slices[l - 1], RV.level_sample_at(slices[l - 1], slices[l])))
    return vols, slices


# ---------------------------------------------------------------- the definitions

def test_level_sample_at():
    from stereo_amd import pyramid
    for fn in (RV.level_sample_at, pyramid.level_sample_at):
        l1 = R.level_disparities(SLICES, 1)
        assert l1.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
        assert fn(SLICES, l1).tolist() == [3.0, 4.0, 6.0, 8.0, 10.0, 11.0]       # 2 and 12 leave 3 .. 11: the nearest end
        l2 = R.level_disparities(SLICES, 2)
        assert l2.tolist() == [0.0, 1.0, 2.0, 3.0] and fn(l1, l2).tolist() == [1.0, 2.0, 4.0, 6.0]
        assert fn(np.arange(8.0), R.level_disparities(np.arange(8.0), 1)).tolist() == [0.0, 2.0, 4.0, 6.0, 7.0]
        assert fn(np.array([7.0, 3.0, 5.0]), [1.0, 2.0, 4.0]).tolist() == [3.0, 4.0, 7.0]    # min and max, not the ends
        assert fn(SLICES, l1).dtype == np.float64


def test_the_sampler_at_a_slice_returns_the_slice():
    vols, slices = dyadic_levels()
    for vol, d in zip(vols, slices):
        h, w, _ = vol.shape
        for i, at in enumerate(d):
            assert np.array_equal(OT.sample_ncc_from_disp(vol, d, np.full(h * w, at)), vol[:, :, i]), (vol.shape, at)


def test_two_reductions_at_slices_are_the_4x4_block_mean_of_the_picked_slices():
    vols, slices = dyadic_levels()
    picked = [0, 1, 5, 8]                               # level 2 samples level 1 at 1, 2, 4, 6: the fine slices 3, 4, 8, 11
    assert (SLICES[picked] == RV.level_sample_at(SLICES, RV.level_sample_at(slices[1], slices[2]))).all()
    want = vols[0][:, :, picked].reshape(H // 4, 4, W // 4, 4, 4).sum(axis=(1, 3)) / 16.0     # multiples of 2^-6: exact
    assert vols[2].shape == (H // 4, W // 4, 4) and np.array_equal(vols[2], want)
    assert vols[1].shape == (H // 2, W // 2, 6) and not (vols[1] == -1e6).any() and not (vols[2] == -1e6).any()


def test_the_level_models_unary_identity_is_exact():
    """Restricted to maps that are constant on 4 x 4 blocks, the fine energy's unary term is 16 times the level-2
    model's, block by block: 16 U_2(P, m(P)) is the sum of the block's 16 fine unaries at 4 m(P).  (The pairwise half:
    test_pyramid_cpu.test_level_model_identity_is_exact.)  6-bit dyadic values keep every sum exact."""
    vols, slices = dyadic_levels()
    in_range = slices[2][(4.0 * slices[2] >= SLICES.min()) & (4.0 * slices[2] <= SLICES.max())]
    assert in_range.tolist() == [1.0, 2.0]
    rng = np.random.default_rng(11)
    for trial in range(4):
        m = rng.choice(in_range, size=(H // 4, W // 4))
        fine = 4.0 * np.repeat(np.repeat(m, 4, axis=0), 4, axis=1)
        m_up = m
        for _ in range(2):                                          # the nearest expansion, restated
            m_up = R.expand(m_up, (2 * m_up.shape[0], 2 * m_up.shape[1]), 0)[0]
        assert np.array_equal(m_up, fine)
        planes = np.zeros((4, H * W))
        planes[2], planes[3] = 1.0, -fine.T.reshape(-1)
        U_fine = OT.ncc_unary_cost(vols[0], SLICES, WEIGHT, planes, OT.get_points(H, W)).reshape(W, H).T
        k = (m - slices[2][0]).astype(np.int64)
        U_2 = WEIGHT * (1.0 - np.take_along_axis(vols[2], k[:, :, None], axis=2)[:, :, 0])
        blocks = U_fine.reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3))
        assert np.array_equal(16.0 * U_2, blocks) and (blocks > 0).all()


def test_restated_reduce_volume_replicates_and_keeps_the_order():
    vol = band_restate.volume(3, 5, 4, 2)
    d = band_restate.disparities_for(4, False)                       # 2, 3, 4, 5
    got = RV.reduce_volume(vol, d, [3.0, 1.0, 5.0])
    assert got.shape == (2, 3, 3)
    assert got[1, 2, 0] == vol[2, 4, 1] and got[0, 2, 0] == (vol[0, 4, 1] + vol[1, 4, 1]) / 2.0      # replication
    assert (got[:, :, 1] == -1e6).all()                              # below the range: four times -1e6, a quarter of it
    assert np.array_equal(got[:, :, 2], RV.reduce_volume(vol[:, :, 3:], d[3:], [5.0])[:, :, 0])      # the last slice itself


# ---------------------------------------------------------------- refusals of the C entries

def _lib():
    from stereo_amd import _lib
    return _lib.lib()


def _call(fn, *args):
    err = C.create_string_buffer(512)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _arrays(device_form, n):
    """Arrays the entries may be handed: never read here (every call is refused before the device is looked for), but
    real memory of the right kind all the same -- device memory for the device forms where a device exists."""
    import stereo_amd
    if device_form and stereo_amd.device_count() > 0:
        import torch
        keep = [torch.zeros(64, dtype=torch.float64, device="cuda") for _ in range(n)]
        return keep, [C.c_void_p(t.data_ptr()) for t in keep]
    keep = [np.zeros(64) for _ in range(n)]
    return keep, [C.c_void_p(a.ctypes.data) for a in keep]


BAD = [
    (dict(H=0), "at least 1"), (dict(W=0), "at least 1"), (dict(D=0), "at least 1"), (dict(Kc=0), "at least 1"),
    (dict(H=-2), "at least 1"), (dict(Kc=-1), "at least 1"),
    (dict(H=65536, W=32768), "2\\^31"),
    (dict(H=1, W=2 ** 31 - 1, Kc=2 ** 30), "Hc \\* Wc \\* Kc must be below 2\\^63 / 8"),
    (dict(H=1, W=2 ** 31 - 1, D=2 ** 30), "H \\* W \\* D must be below 2\\^63 / 8"),
    (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
    (dict(ncc=None), "NULL"), (dict(disparities=None), "NULL"), (dict(sample_at=None), "NULL"), (dict(out=None), "NULL"),
    (dict(disparities=[2.0, np.nan, 4.0]), "disparities\\[1\\] is not finite"),
    (dict(disparities=[2.0, 3.0, np.inf]), "disparities\\[2\\] is not finite"),
    (dict(sample_at=[2.0, -np.inf]), "sample_at\\[1\\] is not finite"), (dict(sample_at=[np.nan, 3.0]), "sample_at\\[0\\] is not finite"),
    (dict(out="ncc"), "alias"),
]
BAD_DEVICE_FORM = [(dict(d_disparities=None), "NULL"), (dict(d_sample_at=None), "NULL")]      # its copies of the short vectors
CASES = [(form, change, match) for form in (False, True) for change, match in BAD + (BAD_DEVICE_FORM if form else [])]


@pytest.mark.parametrize("device_form,change,match", CASES,
                         ids=["%s-%s" % ("device" if f else "host", "-".join("%s=%s" % kv for kv in c.items())) for f, c, _ in CASES])
def test_reduce_volume_refusals(device_form, change, match):
    keep, (ncc, out, dd, ds) = _arrays(device_form, 4)
    v = dict(ncc=ncc, H=3, W=4, D=3, layout=1, disparities=[2.0, 3.0, 4.0], d_disparities=dd, sample_at=[2.5, 3.0],
             d_sample_at=ds, Kc=2, out=out)
    v.update(change)
    if v["out"] == "ncc":
        v["out"] = v["ncc"]
    host = {k: None if v[k] is None else np.array(v[k], dtype=np.float64) for k in ("disparities", "sample_at")}
    hp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    args = [v["ncc"], C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["D"]), C.c_int(v["layout"]), hp(host["disparities"])]
    if device_form:
        args.append(v["d_disparities"])
    args.append(hp(host["sample_at"]))
    if device_form:
        args.append(v["d_sample_at"])
    args += [C.c_int(v["Kc"]), v["out"]]
    if device_form:
        args.append(None)
    name = "stereo_pyramid_reduce_volume_device" if device_form else "stereo_pyramid_reduce_volume"
    rc, msg = _call(getattr(_lib(), name), *args)
    assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), msg
    assert _lib().stereo_hip_last_error().decode() == msg


def test_python_entries_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import pyramid, StereoHipError
    vol = np.zeros((3, 4, 3))
    with pytest.raises(StereoHipError, match="H x W x D"):
        pyramid.reduce_volume(vol, (3, 5), [2.0, 3.0, 4.0], [2.0])
    with pytest.raises(StereoHipError, match="D x \\(H\\*W\\)"):
        pyramid.reduce_volume(np.zeros((3, 11)), (3, 4), [2.0, 3.0, 4.0], [2.0], layout=1)
    with pytest.raises(StereoHipError, match="2 disparities for a volume of 3 slices"):
        pyramid.reduce_volume(vol, (3, 4), [2.0, 3.0], [2.0])
    with pytest.raises(StereoHipError, match="sample_at must be a vector"):
        pyramid.reduce_volume(vol, (3, 4), [2.0, 3.0, 4.0], [[2.0]])
    with pytest.raises(StereoHipError, match="layout"):
        pyramid.reduce_volume(vol, (3, 4), [2.0, 3.0, 4.0], [2.0], layout=2)
    with pytest.raises(StereoHipError, match="not finite"):
        pyramid.reduce_volume(vol, (3, 4), [2.0, 3.0, 4.0], [np.nan])
    with pytest.raises(StereoHipError, match="at least 1"):
        pyramid.reduce_volume(vol, (3, 4), [2.0, 3.0, 4.0], [])
    im = np.zeros((8, 12, 3))
    args = ([im, im], np.arange(4.0), 1, 40.0, 2.0, 1, 3, 0.0)
    for unary in ("other", "", None, 1, "Blocks"):
        with pytest.raises(StereoHipError, match="unary must be 'images' or 'blocks'"):
            stereo_amd.solve_pair_ncc_pyramid(*args, unary=unary)
        with pytest.raises(StereoHipError, match="unary must be 'images' or 'blocks'"):
            pyramid.solve_view_ncc_pyramid(*args, unary=unary)
        with pytest.raises(StereoHipError, match="unary must be 'images' or 'blocks'"):
            object.__new__(stereo_amd.dispmap_ncc).solve_pyramid(1, unary=unary)
    with pytest.raises(StereoHipError, match="unary='blocks' only"):
        pyramid.solve_view_ncc_pyramid(*args, volume=np.zeros((4, 96)))
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(StereoHipError, match="dispmap_globalstereo reaches its second view through a projection"):
        glob.solve_pyramid(1, unary="blocks")
    assert pyramid.check_unary("images") == "images" and pyramid.check_unary("blocks") == "blocks"


def test_the_three_abi_numbers_agree_and_count_the_new_entries():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 16
    for name in ("stereo_pyramid_reduce_volume", "stereo_pyramid_reduce_volume_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
