"""The plane pyramid without a device: what the restatements of stereo_pyramid_expand_planes and
stereo_planes_fit_local (tests/plane_pyramid_restate.py, tests/plane_fit_restate.py) promise on dyadic planes, where
every operation is exact, and the refusals of the new entry points, which come before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plane_fit_restate as FR
import plane_pyramid_restate as PR
import pyramid_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DYADIC = [(0.25, -0.5, 2.0, -9.0), (0.125, 0.375, 1.0, -3.5), (0.0, 0.0, 1.0, -4.0), (-0.75, 0.0, -4.0, 6.0)]
INF = float("inf")


def field(plane, n):
    return np.repeat(np.array(plane, np.float64).reshape(4, 1), n, axis=1)


# ---------------------------------------------------------------- expansion

@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (5, 7), (6, 8), (7, 9)], ids=lambda s: "%dx%d" % s)
def test_expanded_plane_has_twice_the_coarse_disparity_at_the_coarse_coordinate(shape):
    H, W = shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    rng = np.random.default_rng([H, W, 1])
    coarse = np.array(DYADIC).T[:, rng.integers(0, len(DYADIC), size=Hc * Wc)]          # another plane per coarse pixel
    image_f, image_c = rng.uniform(0, 255, size=(H, W, 3)), rng.uniform(0, 255, size=(Hc, Wc, 3))
    for mode in (0, 1):
        fine, source = PR.expand_planes(coarse, (H, W), mode, image_f, image_c)
        assert (source >= 0).all() and (mode == 1 or (source == 0).all())
        for x in range(W):
            for y in range(H):
                cy, cx = R.candidates(y, x, Hc, Wc)[source[y, x]]
                parent = coarse[:, cy + Hc * cx]
                got = FR.disparity(fine[:, y + H * x], x + 1.0, y + 1.0)
                want = 2.0 * FR.disparity(parent, (x + 1.5) / 2.0, (y + 1.5) / 2.0)
                assert got == want and np.isfinite(got), (mode, y, x)


def test_one_slanted_plane_stays_one_plane_and_costs_nothing():
    from oracle import terms as O
    H, W = 7, 10
    Hc, Wc = 4, 5
    plane = DYADIC[0]
    coarse = field(plane, Hc * Wc)
    rng = np.random.default_rng(3)
    image_f, image_c = rng.uniform(0, 255, size=(H, W, 3)), rng.uniform(0, 255, size=(Hc, Wc, 3))
    ind1, ind2 = O.construct_neighborhood(H, W)
    points = O.get_points(H, W)
    weights = np.ones(ind1.shape[0])
    for mode in (0, 1):
        fine, _ = PR.expand_planes(coarse, (H, W), mode, image_f, image_c)
        assert np.array_equal(fine, field(PR.to_fine(np.array(plane)), H * W))          # one plane again
        for kernel in (1, 2):
            e00 = O.all_pairwise_costs(kernel, weights, 5.0, fine, fine, ind1, ind2, points)[0]
            assert np.array_equal(e00, np.zeros_like(e00))
        # the scalar expansion of the same surface is a staircase: it pays
        coarse_map = FR.own_disparities(coarse, Hc, Wc)
        stairs = PR.fronto(R.expand(coarse_map, (H, W), mode, image_f, image_c)[0])
        assert O.all_pairwise_costs(1, weights, 5.0, stairs, stairs, ind1, ind2, points)[0].sum() > 0


def test_invalid_candidates_of_the_expansion():
    H, W, Hc, Wc = 6, 8, 3, 4
    coarse = field(DYADIC[1], Hc * Wc)
    flat_f, flat_c = np.full((H, W, 1), 7.0), np.full((Hc, Wc, 1), 5.0)
    for bad in ([np.nan, 0, 1, 0], [0, np.inf, 1, 0], [0, 0, 0.0, 1], [0, 0, 1, -np.inf]):
        c = coarse.copy()
        c[:, 1 + Hc * 2] = bad                                   # the parent of the fine pixels (2..3, 4..5)
        near, src = PR.expand_planes(c, (H, W), 0)
        assert np.isnan(near[:, 3 + H * 5]).all() and src[3, 5] == 0 and not np.isnan(near[:, 1 + H * 5]).any()
        guided, src = PR.expand_planes(c, (H, W), 1, flat_f, flat_c)
        assert src[3, 5] == 1 and np.array_equal(guided[:, 3 + H * 5], PR.to_fine(coarse[:, 0]))    # ties: the first valid
    c = coarse.copy()
    c[2] = 0.0
    guided, src = PR.expand_planes(c, (H, W), 1, flat_f, flat_c)
    assert np.isnan(guided).all() and (src == -1).all()
    # a fronto-parallel plane keeps the scalar expansion's value
    d = np.arange(12.0).reshape(Hc, Wc) / 4.0 - 1.0
    fine, _ = PR.expand_planes(PR.fronto(d), (H, W), 0)
    assert PR.same_but_zero_sign(fine, PR.fronto(R.expand(d, (H, W), 0)[0]))


# ---------------------------------------------------------------- fit

def assert_recovers(fitted, planes, H, W, where=None):
    for x in range(W):
        for y in range(H):
            i = y + H * x
            for X, Y in ((1.0, 1.0), (x + 1.0, y + 1.0), (float(W), float(H))) if where is None else where(x, y):
                assert FR.disparity(fitted[:, i], X, Y) == FR.disparity(planes[:, i], X, Y), (y, x, X, Y)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("shape", [(3, 3), (5, 7), (7, 6), (9, 11)], ids=lambda s: "%dx%d" % s)
def test_fit_returns_a_dyadic_plane_exactly(shape, radius):
    H, W = shape
    for plane in DYADIC:
        planes = field(plane, H * W)
        fitted, bad = FR.fit_local(planes, (H, W), radius, INF)
        assert bad == 0 and (fitted[2] == 1.0).all()
        assert_recovers(fitted, planes, H, W)
        # the fit sees only z: the fronto-parallel planes of the same surface give the same planes
        again, bad = FR.fit_local(PR.fronto(FR.own_disparities(planes, H, W)), (H, W), radius, INF)
        assert bad == 0 and again.tobytes() == fitted.tobytes()


def test_fit_keeps_two_planes_apart_across_a_jump():
    H, W, radius, tau = 8, 10, 2, 3.0
    planes = np.zeros((4, H * W))
    for x in range(W):
        planes[:, H * x:H * (x + 1)] = np.array(DYADIC[0] if x < 5 else (-0.125, 0.25, 1.0, -40.0)).reshape(4, 1)
    z = FR.own_disparities(planes, H, W)
    assert np.abs(z[:, 4] - z[:, 5]).min() > tau                 # the jump is larger than tau everywhere
    for source in (planes, PR.fronto(z)):
        fitted, bad = FR.fit_local(source, (H, W), radius, tau)
        assert bad == 0
        assert_recovers(fitted, planes, H, W)
    mixed, _ = FR.fit_local(planes, (H, W), radius, INF)          # without tau the border columns mix the two
    assert FR.disparity(mixed[:, H * 4], 1.0, 1.0) != FR.disparity(planes[:, H * 4], 1.0, 1.0)


@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_fit_of_a_one_pixel_wide_image_is_the_own_fronto_parallel_plane(shape):
    H, W = shape
    for plane in DYADIC:
        planes = field(plane, H * W)
        fitted, bad = FR.fit_local(planes, (H, W), 2, INF)
        z = FR.own_disparities(planes, H, W)
        assert bad == 0 and np.array_equal(fitted, PR.fronto(z))


def test_fit_copies_an_invalid_plane_through_and_skips_it_as_a_tap():
    H, W = 5, 7
    planes = field(DYADIC[0], H * W)
    planes[:, 2 + H * 3] = [0.5, 0.25, 0.0, 1.0]
    planes[:, 0] = [np.nan, 0.0, 1.0, 2.0]
    fitted, bad = FR.fit_local(planes, (H, W), 2, INF)
    assert bad == 2 and np.array_equal(fitted[:, 2 + H * 3], planes[:, 2 + H * 3]) and np.isnan(fitted[0, 0])
    ok = np.ones(H * W, bool)
    ok[[0, 2 + H * 3]] = False
    clean, _ = FR.fit_local(field(DYADIC[0], H * W), (H, W), 2, INF)
    for i in np.flatnonzero(ok):
        y, x = i % H, i // H
        assert FR.disparity(fitted[:, i], 1.0, 1.0) == FR.disparity(clean[:, i], 1.0, 1.0), (y, x)
    zero, _ = FR.fit_local(planes, (H, W), 2, 0.0)               # tau = 0: only taps at the pixel's own disparity
    assert np.isfinite(zero[:, ok]).all()


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
    real memory of the right kind and of the size the checked sizes ask for."""
    import stereo_amd
    if device_form and stereo_amd.device_count() > 0:
        import torch
        keep = [torch.zeros(4096, dtype=torch.float64, device="cuda") for _ in range(n)]
        return keep, [C.c_void_p(t.data_ptr()) for t in keep]
    keep = [np.zeros(4096) for _ in range(n)]
    return keep, [C.c_void_p(a.ctypes.data) for a in keep]


def _ids(v):
    return "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None


BAD_EXPAND_PLANES = [
    (dict(H=0, Hc=0), "at least 1"), (dict(W=0, Wc=0), "at least 1"), (dict(C=0), "at least 1"),
    (dict(H=65536, W=32768, Hc=32768, Wc=16384), "2\\^31"),
    (dict(p_coarse=None), "p_coarse and out must not be NULL"), (dict(out=None), "NULL"), (dict(im_fine=None), "NULL"),
    (dict(im_coarse=None), "NULL"),
    (dict(Hc=2), "sizes do not match"), (dict(Wc=3), "sizes do not match"), (dict(H=7, W=8), "sizes do not match"),
    (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
    (dict(out="p_coarse"), "alias"), (dict(out="im_fine"), "alias"), (dict(out="im_coarse"), "alias"),
    (dict(source="p_coarse"), "alias"), (dict(source="out"), "alias"), (dict(source="im_fine"), "alias"),
    (dict(mode=0, out="p_coarse"), "alias"),
    (dict(out=("p_coarse", 64)), "alias"), (dict(out=("im_fine", -64)), "alias"), (dict(source=("out", 256)), "alias"),
]


def _resolve(v, keys):
    """'name' -> that argument's pointer; ('name', bytes) -> that pointer moved, an overlap no pointer comparison sees."""
    for key in keys:
        if isinstance(v[key], str):
            v[key] = v[v[key]]
        elif isinstance(v[key], tuple):
            v[key] = C.c_void_p(v[v[key][0]].value + v[key][1])


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_EXPAND_PLANES, ids=_ids)
def test_expand_planes_refusals(device_form, change, match):
    keep, (p, f, g, out, src) = _arrays(device_form, 5)
    v = dict(p_coarse=p, Hc=3, Wc=4, H=5, W=7, mode=1, im_fine=f, im_coarse=g, C=1, out=out, source=src)
    v.update(change)
    _resolve(v, ("out", "source"))
    args = [v["p_coarse"], C.c_int(v["Hc"]), C.c_int(v["Wc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["mode"]),
            v["im_fine"], v["im_coarse"], C.c_int(v["C"]), v["out"], v["source"]]
    if device_form:
        args.append(None)
    name = "stereo_pyramid_expand_planes_device" if device_form else "stereo_pyramid_expand_planes"
    rc, msg = _call(getattr(_lib(), name), *args)
    assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), msg
    assert _lib().stereo_hip_last_error().decode() == msg


BAD_FIT = [
    (dict(H=0), "at least 1"), (dict(W=-1), "at least 1"), (dict(H=65536, W=32768), "2\\^31"),
    (dict(planes=None), "NULL"), (dict(out=None), "NULL"),
    (dict(radius=0), "radius must be 1 .. 8"), (dict(radius=9), "radius must be 1 .. 8"), (dict(radius=-3), "radius"),
    (dict(tau=-1.0), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=-0.5 * INF), "tau"),
    (dict(out="planes"), "alias"), (dict(out=("planes", 32 * 34)), "alias"), (dict(out=("planes", -32)), "alias"),
]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("change,match", BAD_FIT, ids=_ids)
def test_fit_local_refusals(device_form, change, match):
    keep, (planes, out, bad) = _arrays(device_form, 3)
    v = dict(planes=planes, H=5, W=7, radius=2, tau=1.0, out=out)
    v.update(change)
    _resolve(v, ("out",))
    args = [v["planes"], C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["radius"]), C.c_double(v["tau"]), v["out"], bad]
    if device_form:
        args.append(None)
    name = "stereo_planes_fit_local_device" if device_form else "stereo_planes_fit_local"
    rc, msg = _call(getattr(_lib(), name), *args)
    assert rc != 0 and re.search(match, msg) and msg.startswith(name + ":"), msg
    assert _lib().stereo_hip_last_error().decode() == msg


def test_device_forms_refuse_planes_that_are_not_16_byte_aligned():
    keep, (p, f, g, out, src) = _arrays(True, 5)
    shifted = lambda q: C.c_void_p(q.value + 8)
    for a, b in ((shifted(p), out), (p, shifted(out))):
        rc, msg = _call(_lib().stereo_pyramid_expand_planes_device, a, C.c_int(3), C.c_int(4), C.c_int(5), C.c_int(7),
                        C.c_int(0), None, None, C.c_int(1), b, src, None)
        assert rc != 0 and "16-byte aligned" in msg
        rc, msg = _call(_lib().stereo_planes_fit_local_device, a, C.c_int(5), C.c_int(7), C.c_int(2), C.c_double(1.0), b,
                        None, None)
        assert rc != 0 and "16-byte aligned" in msg


def test_python_wrappers_refuse_before_the_device():
    from stereo_amd import pyramid, plane_candidates, StereoHipError
    planes = np.zeros((4, 12))
    with pytest.raises(StereoHipError, match="4 x \\(Hc \\* Wc\\)"):
        pyramid.expand_planes(planes, (5, 9), "nearest")
    with pytest.raises(StereoHipError, match="4 x \\(Hc \\* Wc\\)"):
        pyramid.expand_planes(np.zeros((3, 4)), (5, 7), "nearest")
    with pytest.raises(StereoHipError, match="needs im_fine"):
        pyramid.expand_planes(planes, (5, 7), "guided")
    with pytest.raises(StereoHipError, match="same C"):
        pyramid.expand_planes(planes, (5, 7), "guided", np.zeros((5, 7, 3)), np.zeros((3, 4, 1)))
    with pytest.raises(StereoHipError, match="'nearest' or 'guided'"):
        pyramid.expand_planes(planes, (5, 7), "bilinear")
    with pytest.raises(StereoHipError, match="mode"):
        pyramid.expand_planes(planes, (5, 7), 2)
    with pytest.raises(StereoHipError, match="4 x N"):
        plane_candidates.fit_local(np.zeros((4, 11)), (3, 4))
    with pytest.raises(StereoHipError, match="radius must be 1 .. 8"):
        plane_candidates.fit_local(planes, (3, 4), radius=9)
    with pytest.raises(StereoHipError, match="tau"):
        plane_candidates.fit_local(planes, (3, 4), tau=-1.0)


def test_fit_is_a_source_of_a_plane_candidate_level():
    from stereo_amd import candidates, plane_candidates as pc, StereoHipError
    fit = pc.Fit()
    assert (fit.radius, fit.tau) == (2, 1.0) and (pc.Fit(8, INF).radius, pc.Fit(8, INF).tau) == (8, INF)
    assert pc.Fit(1, 0).tau == 0.0 and "radius=3" in repr(pc.Fit(3))
    for radius in (0, 9, 2.0, True, None):
        with pytest.raises(StereoHipError, match="radius"):
            pc.Fit(radius)
    for tau in (-1.0, float("nan"), "1", None, True):
        with pytest.raises(StereoHipError, match="tau"):
            pc.Fit(2, tau)
    level = pc.check_level(dict(sources=[fit, "base"], taps=[(0, 0), (0, 1)]))
    assert level["sources"][0] is fit and candidates.labels_of(level) == 1 + 2 * 2
    assert pc.check_level(dict(sources=fit, taps=[(0, 0)]))["sources"] == [fit]           # one source without a list
    assert pc.check_levels([dict(sources=[pc.Fit(3, 2.0)], taps=[(0, 0)])])[0]["sources"][0].radius == 3
    with pytest.raises(StereoHipError, match="'base', 'wta' or an H x W map"):
        candidates.check_level(dict(sources=[fit], taps=[(0, 0)]))                        # a scalar candidate level has no planes to fit


def test_the_three_abi_numbers_agree_and_count_the_new_section():
    import stereo_amd
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 19
    for name in ("stereo_pyramid_expand_planes", "stereo_pyramid_expand_planes_device", "stereo_planes_fit_local",
                 "stereo_planes_fit_local_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
    assert "solve_view_ncc_plane_pyramid" in stereo_amd.__all__ and callable(stereo_amd.solve_view_ncc_plane_pyramid)


# ---------------------------------------------------------------- the solve's arguments

def test_solve_view_ncc_plane_pyramid_refuses_its_arguments_first():
    import stereo_amd
    from stereo_amd import StereoHipError, plane_candidates as pc
    im = np.zeros((8, 12, 3))
    args = ([im, im], np.arange(4.0), 1, 40.0, 2.0)
    solve = stereo_amd.solve_view_ncc_plane_pyramid
    for levels in (0, 6, True, None):
        with pytest.raises(StereoHipError, match="levels"):
            solve(*args, levels, 3, 0.0)
    with pytest.raises(StereoHipError, match="expand"):
        solve(*args, 1, 3, 0.0, expand="bilinear")
    with pytest.raises(StereoHipError, match="bands|offsets"):
        solve(*args, 2, 3, 0.0, bands=[[[-1.0, 0.0, 1.0]]])
    with pytest.raises(StereoHipError, match="'scales' is not defined here"):
        solve(*args, 1, 3, 0.0, carry="scales")
    with pytest.raises(StereoHipError, match="carry must be"):
        solve(*args, 1, 3, 0.0, carry="all")
    with pytest.raises(StereoHipError, match="unary"):
        solve(*args, 1, 3, 0.0, unary="means")
    with pytest.raises(StereoHipError, match="volume is taken"):
        solve(*args, 1, 3, 0.0, volume=np.zeros((8, 12, 4)))
    with pytest.raises(StereoHipError, match="kernels 1 and 2"):
        solve([im, im], np.arange(4.0), 3, 40.0, 2.0, 1, 3, 0.0)
    good = dict(sources=[pc.Fit(), "base", "wta"], taps=[(0, 0), (0, 1)])
    for propagate in ([[good], [good]], good, "wta", 5, [5], [[dict(sources=["best"], taps=[(0, 0)])]],
                      [[dict(sources=[np.zeros((8, 12))], taps=[(0, 0)])]], [[dict(source=[])]],
                      [[dict(offsets=[1.0, 2.0])]], [[dict(sources=[pc.Fit()], taps=[(0, 1 << 15)])]]):
        with pytest.raises(StereoHipError, match="propagate|plane candidates|plane-candidate"):
            solve(*args, 1, 3, 0.0, propagate=propagate)
    if stereo_amd.device_count() < 1:             # everything above passed the checks; what is left needs the device
        with pytest.raises(StereoHipError, match="no HIP device"):
            solve(*args, 1, 3, 0.0, propagate=[[good]], carry="levels")


def test_solve_plane_pyramid_refuses_what_it_is_not_defined_for():
    import stereo_amd
    from stereo_amd import StereoHipError
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(StereoHipError, match="solve_plane_pyramid: dispmap_globalstereo reaches its second view through a projection"):
        glob.solve_plane_pyramid(1)
    ncc = object.__new__(stereo_amd.dispmap_ncc)
    ncc._smooth_weights = np.array([1.0, 2.0])
    with pytest.raises(StereoHipError, match="solve_plane_pyramid.*smooth_weights"):
        ncc.solve_plane_pyramid(1)
