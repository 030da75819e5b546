"""The map filter on the device: both C entries against the NumPy restatement
(tests/map_filter_restate.py, which test_map_filter_cpu holds against first principles) bit for bit on `out` (NaN
payloads included), `source` and `kept` -- the result is a selection and every sum is formed by the same rounded additions
in the same order, so there is no tolerance to choose -- and the Python surface (take_planes, post_filter= on the two pair
solves, dispmap_ncc.filter_map) against its pieces.

The shapes are the smallest at which the geometry (windows larger than the image, every border), the tile (64 rows by 4
columns per workgroup: H around 64 and past two tiles, W around 4 and past two tiles, so the lane tail, the halo across
tiles both ways and more than one tile each way occur) and every radius can go wrong."""
import functools
import os

import numpy as np
import pytest

import map_filter_restate as MR
from weighted_helpers import PARAMS, image

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 7), (7, 5)]
TILE_H, TILE_W = [63, 64, 65, 130], [3, 4, 5, 9]           # the kernel's tile is 64 x 4
RADII = [1, 2, 3, 4]
ZERO_LOW = (1.25, 0.0, 0.125, 0.5)                           # a ramp that reaches weight 0
ZERO_STEP = (1.0, 0.0, 0.25, 0.25)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def holes(rng, d, r):
    """NaN (with a payload), +Inf and -Inf holes; the corner block is all NaN, so the corner's window has no finite tap
    and that target is itself NaN."""
    d = d.copy()
    bad = rng.random(d.shape) < 0.2
    d[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    d[:r + 1, :r + 1] = np.nan
    d[0:1, 0:1].view(np.int64)[...] = 0x7FF8000000ABCDEF        # a payload that a copy must keep
    return d


def data_classes(shape, r, seed=0):
    """name -> (d, image, params, pixel_weight, targets)"""
    H, W = shape
    rng = np.random.default_rng([H, W, r, seed])
    ints = rng.integers(0, 4, size=shape).astype(np.float64)
    normal = rng.standard_normal(shape) * 3.0
    mask = (rng.random(shape) < 0.6).astype(np.int32)
    dyadic_pw = rng.integers(0, 5, size=shape).astype(np.float64) / 4.0
    some_pw = rng.random(shape) * (rng.random(shape) < 0.7)
    return {
        # ties everywhere: the first-in-tap-order rule of `source`
        "ints": (ints, None, None, None, None),
        "ints_guided_c1": (ints, image(rng, H, W, 1), ZERO_STEP, dyadic_pw, mask),
        # the summation order shows: weights that are not dyadic
        "normal_guided_c3": (normal, image(rng, H, W, 3, dyadic=False), PARAMS["ramp"], some_pw, mask),
        "normal_weighted": (normal, None, None, some_pw, None),
        "normal_guided_only": (normal, image(rng, H, W, 3, dyadic=False), ZERO_LOW, None, np.ones(shape, np.int32)),
        "holes": (holes(rng, normal, r), None, None, None, None),
        "holes_guided_c3": (holes(rng, ints, r), image(rng, H, W, 3), ZERO_LOW, some_pw, mask | (np.arange(H)[:, None] < 2)),
        "no_targets": (holes(rng, normal, r), image(rng, H, W, 1), PARAMS["step"], some_pw, np.zeros(shape, np.int32)),
        "zero_weights": (holes(rng, normal, r), None, None, np.zeros(shape), mask),
    }


def flat(a, dtype):
    import torch
    return torch.from_numpy(np.asfortranarray(a, dtype=dtype).reshape(-1, order="F").copy()).cuda()


def check_device(name, d, im, par, pw, tg, r):
    import torch
    from stereo_amd import Contrast, contrast, mapfilter
    H, W = d.shape
    want_out, want_src, want_kept = MR.weighted_median(d, r, im, par, pw, tg)
    t_d = flat(d, np.float64)
    t_im = contrast.image_to_device(im) if im is not None else None
    t_pw = flat(pw, np.float64) if pw is not None else None
    t_tg = flat(tg, np.int32) if tg is not None else None
    before = [None if t is None else t.clone() for t in (t_d, t_im, t_pw, t_tg)]
    shape = (H, W) if im is None else (H, W, im.shape[2])
    out, source, kept = mapfilter.weighted_median_device(t_d, shape, r, t_im, Contrast(*par) if par else None, t_pw, t_tg)
    torch.cuda.synchronize()
    what = (name, d.shape, r)
    assert np.array_equal(bits(out.cpu().numpy().reshape(W, H).T), bits(want_out)), what
    assert source.dtype == torch.int32 and np.array_equal(source.cpu().numpy().reshape(W, H).T, want_src), what
    assert int(kept.item()) == want_kept, what
    for t, b in zip((t_d, t_im, t_pw, t_tg), before):                    # the inputs are only read
        assert t is None or np.array_equal(bits(t.double().cpu().numpy()), bits(b.double().cpu().numpy())), what
    # without a source map, into tensors of the caller, on a stream of its own
    mine = torch.full((W, H), 7.0, dtype=torch.float64, device="cuda")
    count = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    out2, none, kept2 = mapfilter.weighted_median_device(t_d, shape, r, t_im, Contrast(*par) if par else None, t_pw, t_tg,
                                                         out=mine, kept=count, stream=stream, want_source=False)
    stream.synchronize()
    assert out2 is mine and none is None and kept2 is count and int(count.item()) == want_kept
    assert np.array_equal(bits(mine.cpu().numpy().T), bits(want_out)), what
    return want_out, want_src, want_kept


def check_host(name, d, im, par, pw, tg, r):
    from stereo_amd import Contrast, mapfilter
    want_out, want_src, want_kept = MR.weighted_median(d, r, im, par, pw, tg)
    before = [None if a is None else np.array(a) for a in (d, im, pw, tg)]
    out, source, kept = mapfilter.weighted_median(d, r, im, Contrast(*par) if par else None, pw, tg)
    what = (name, d.shape, r)
    assert np.array_equal(bits(out), bits(want_out)) and source.dtype == np.int32 and np.array_equal(source, want_src), what
    assert kept == want_kept, what
    for a, b in zip((d, im, pw, tg), before):
        assert a is None or np.array_equal(bits(a), bits(b))
    out, source, kept = mapfilter.weighted_median(d, r, im, Contrast(*par) if par else None, pw, tg, want_source=False)
    assert source is None and np.array_equal(bits(out), bits(want_out)) and kept == want_kept


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_every_data_class_on_the_small_geometries(shape, r, hip):
    for name, args in data_classes(shape, r).items():
        check_device(name, *args, r)
        check_host(name, *args, r)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("W", TILE_W)
@pytest.mark.parametrize("H", TILE_H)
def test_device_equals_the_restatement_around_the_tile(H, W, r, hip):
    classes = data_classes((H, W), r, seed=1)
    for name in ("normal_guided_c3", "holes_guided_c3"):
        check_device(name, *classes[name], r)


@pytest.mark.parametrize("r", RADII)
def test_every_data_class_on_more_than_one_tile_each_way(r, hip):
    """130 x 9: three tiles down, three across.  What the classes are there for is seen to happen."""
    shape = (130, 9)
    classes = data_classes(shape, r, seed=2)
    ids = np.arange(130)[:, None] + 130 * np.arange(9)[None, :]
    for name, args in classes.items():
        out, src, kept = check_device(name, *args, r)
        check_host(name, *args, r)
        d, tg = args[0], args[4]
        if name == "zero_weights":
            assert kept == int(tg.sum()) and np.array_equal(bits(out), bits(d))
        if name == "no_targets":
            assert kept == 0 and np.array_equal(bits(out), bits(d)) and np.array_equal(src, ids)
        if name == "holes":
            assert kept >= 1 and bits(out)[0, 0] == 0x7FF8000000ABCDEF and (out != d)[np.isfinite(d)].any()
        if name == "ints":
            assert kept == 0 and (src != ids).any()


@pytest.mark.parametrize("r", RADII)
def test_unguided_equals_guided_by_a_constant_image_with_unit_weights(r, hip):
    from stereo_amd import Contrast, mapfilter
    rng = np.random.default_rng([21, r])
    shape = (65, 5)
    d = holes(rng, rng.standard_normal(shape), r)
    tg = (rng.random(shape) < 0.7).astype(np.int32)
    plain = mapfilter.weighted_median(d, r, targets=tg)
    guided = mapfilter.weighted_median(d, r, np.full(shape + (3,), 0.375), Contrast(1.0, 0.25, 0.5, 1.0), np.ones(shape), tg)
    assert np.array_equal(bits(plain[0]), bits(guided[0])) and np.array_equal(plain[1], guided[1]) and plain[2] == guided[2]


def test_take_planes_agrees_with_the_source_map(hip):
    from stereo_amd import mapfilter
    rng = np.random.default_rng(8)
    H, W = 9, 11
    d = rng.integers(0, 6, size=(H, W)).astype(np.float64)
    planes = np.vstack([rng.standard_normal((2, H * W)) * 0, np.ones((1, H * W)), -d.T.reshape(1, -1)])    # fronto-parallel
    planes[0] = np.arange(H * W)                         # (a tag per pixel: which plane came from where)
    out, source, kept = mapfilter.weighted_median(d, 2, pixel_weight=(rng.random((H, W)) < 0.5).astype(np.float64))
    got = mapfilter.take_planes(planes, source)
    assert np.array_equal(got[3], -out.T.reshape(-1)) and np.array_equal(got[0], source.T.reshape(-1))
    assert np.array_equal(got, planes[:, source.T.reshape(-1)])


# ---------------------------------------------------------------- where it plugs in

PK = 8
WEIGHT, TOL, CHECK_TOL, ITERS, NEVER = 40.0, 2.0, 1.0, 4, -1e300
BANDS = [[-0.5, -0.25, 0.0, 0.25, 0.5]]
CANDIDATES = [dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base", "wta"])]
VIEW_FIELDS = ("labels", "dispmap", "status", "residual", "filled", "source", "energy", "lower_bound", "iterations", "maps",
               "paths", "carried", "expanded", "expand_source")


@functools.lru_cache(maxsize=None)
def teddy_crop():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_pair.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    return im0[100:124, 200:232].copy(), im1[100:124, 200:232].copy()


def same_field(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, list):
        return len(a) == len(b) and all(same_field(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def filters():
    from stereo_amd import Contrast, MedianFilter
    return [MedianFilter(2, Contrast(2, 0.5, 8, 40)), MedianFilter(1, sources="all", targets="all"), MedianFilter(4)]


def assert_filtered_by_hand(got, plain, f, images):
    from stereo_amd import mapfilter
    for view, ref, im in zip(got.views, plain.views, images):
        for name in VIEW_FIELDS:
            assert same_field(getattr(view, name), getattr(ref, name)), name
        assert ref.filtered is None and ref.filter_source is None
        pw, tg = f.masks(view.status)
        out, source, _ = mapfilter.weighted_median(view.filled, f.radius, im if f.contrast else None, f.contrast, pw, tg)
        assert np.array_equal(bits(view.filtered), bits(out)) and np.array_equal(view.filter_source, source)
        r_out, r_source, _ = MR.weighted_median(view.filled, f.radius, im if f.contrast else None,
                                                (f.contrast.w_high, f.contrast.w_low, f.contrast.g0, f.contrast.g1)
                                                if f.contrast else None, pw, tg)
        assert np.array_equal(bits(view.filtered), bits(r_out)) and np.array_equal(view.filter_source, r_source)
        if tg is not None:
            assert np.array_equal(bits(view.filtered)[tg == 0], bits(view.filled)[tg == 0])


def test_solve_pair_ncc_with_a_post_filter(hip):
    images, disparities = teddy_crop(), np.arange(PK, dtype=np.float64)
    call = lambda **kw: hip.solve_pair_ncc(images, disparities, 1, WEIGHT, TOL, ITERS, NEVER, check_tol=CHECK_TOL,
                                           refine_iters=2, band_levels=BANDS, **kw)
    plain = call()
    for f in filters()[:2]:
        assert_filtered_by_hand(call(post_filter=f), plain, f, images)


def test_solve_pair_ncc_scanline_with_a_post_filter(hip):
    images, disparities = teddy_crop(), np.arange(PK, dtype=np.float64)
    for levels in (dict(), dict(candidate_levels=CANDIDATES, band_levels=BANDS, maxiter=ITERS, max_relgap=NEVER)):
        call = lambda **kw: hip.solve_pair_ncc_scanline(images, disparities, 1, WEIGHT, TOL, check_tol=CHECK_TOL, **levels, **kw)
        plain = call()
        f = filters()[0]
        assert_filtered_by_hand(call(post_filter=f), plain, f, images)
    assert (plain.left.status != 0).any()          # (there is something to filter)


def test_dispmap_ncc_filter_map_plain_and_mirrored(hip):
    from stereo_amd import StereoHipError, mapfilter
    images = list(teddy_crop())
    dm = hip.dispmap_ncc(images, np.arange(PK, dtype=np.float64), 1, WEIGHT, TOL)
    mirror = dm.mirrored()
    for obj in (dm, mirror):
        obj.set_disparity(obj.best_disp_from_ncc())
    with pytest.raises(StereoHipError, match="call cross_check"):
        dm.filter_map(filters()[0])
    dm.cross_check(mirror, CHECK_TOL)
    mirror.cross_check(dm, CHECK_TOL)
    for f in filters():
        for obj, own in ((dm, images[0]), (mirror, images[1])):
            before = bits(obj.filled_dispmap).copy()
            got = obj.filter_map(f)
            pw, tg = f.masks(obj.consistency)
            out, source, _ = mapfilter.weighted_median(obj.filled_dispmap, f.radius, own if f.contrast else None, f.contrast, pw, tg)
            assert got is obj.filtered_dispmap and np.array_equal(bits(got), bits(out))
            assert np.array_equal(obj.filtered_source, source) and np.array_equal(bits(obj.filled_dispmap), before)
    assert (dm.consistency != 0).any() and (mirror.consistency != 0).any()
    with pytest.raises(StereoHipError, match="MedianFilter is needed"):
        dm.filter_map(2)
