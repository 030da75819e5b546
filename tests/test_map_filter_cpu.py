"""The map filter without a device: the NumPy restatement (tests/map_filter_restate.py) against first
principles with zero tolerance -- the plain lower median under unit weights, an independent sort-and-cumulate weighted
median under dyadic weights (multiples of 1/64 below 2^7 over at most 81 taps: every sum is exact, in whatever order it
is formed), what `source` points at, and an image edge that no weight crosses; the MedianFilter masks; every refusal of
the two C entries, which come before the device is looked for."""
import ctypes as C
import re

import numpy as np
import pytest

import map_filter_restate as MR
from weighted_helpers import PARAMS, image

SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 7), (7, 5), (9, 11)]


def holes(rng, d, share=0.15):
    d = d.copy()
    bad = rng.random(d.shape) < share
    d[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    return d


def window(H, W, y, x, r):
    """The taps of (y, x) inside the image in tap order: (y', x')."""
    return [(y + dy, x + dx) for dy, dx in MR.taps(r) if 0 <= y + dy < H and 0 <= x + dx < W]


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_unit_weights_are_the_plain_lower_median(shape, r):
    H, W = shape
    rng = np.random.default_rng([H, W, r])
    for d in (rng.integers(0, 4, size=shape).astype(np.float64), holes(rng, rng.standard_normal(shape))):
        out, source, kept = MR.weighted_median(d, r)
        n_kept = 0
        for y in range(H):
            for x in range(W):
                values = sorted(d[q] for q in window(H, W, y, x, r) if np.isfinite(d[q]))
                if values:
                    assert out[y, x] == values[(len(values) - 1) // 2], (y, x)
                else:
                    n_kept += 1
                    assert np.array_equal(out[y, x:x + 1].view(np.int64), d[y, x:x + 1].view(np.int64))
                    assert source[y, x] == y + H * x
        assert kept == n_kept


def sorted_weighted_median(values, weights):
    """The lower weighted median by sorting: the smallest value whose cumulated weight, doubled, reaches the total."""
    order = np.argsort(values, kind="stable")
    v, w = np.asarray(values)[order], np.asarray(weights)[order]
    total = w.sum()
    if not total > 0:
        return None
    cum = np.cumsum(w)
    # (equal values share one W_le: the cumulated weight at the last of them)
    for i in range(len(v)):
        last = np.searchsorted(v, v[i], side="right") - 1
        if 2.0 * cum[last] >= total:
            return v[i]
    raise AssertionError("no weighted median")


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "%dx%d" % s)
def test_dyadic_weights_equal_sort_and_cumulate(shape, r, guided):
    H, W = shape
    rng = np.random.default_rng([H, W, r, int(guided)])
    d = holes(rng, rng.integers(-3, 4, size=shape).astype(np.float64) * 0.5)
    pw = rng.integers(0, 65, size=shape).astype(np.float64) / 64.0
    pw[rng.random(shape) < 0.3] = 0.0
    targets = rng.random(shape) < 0.8
    # a dyadic image and a step ramp with dyadic levels: the products and all sums stay exact
    im = image(rng, H, W, 2) if guided else None
    par = (1.5, 0.5, 0.25, 0.25) if guided else None
    out, source, kept = MR.weighted_median(d, r, im, par, pw, targets)
    n_kept = 0
    for y in range(H):
        for x in range(W):
            own = d[y, x:x + 1].view(np.int64)
            if not targets[y, x]:
                assert np.array_equal(out[y, x:x + 1].view(np.int64), own) and source[y, x] == y + H * x
                continue
            taps = [q for q in window(H, W, y, x, r) if np.isfinite(d[q])]
            weights = []
            for q in taps:
                w = pw[q]
                if guided:
                    g = np.abs(im[y, x] - im[q]).max()
                    w = (par[0] if g <= par[2] else par[1]) * w
                weights.append(w)
            want = sorted_weighted_median([d[q] for q in taps], weights) if taps else None
            if want is None:
                n_kept += 1
                assert np.array_equal(out[y, x:x + 1].view(np.int64), own) and source[y, x] == y + H * x
                continue
            assert out[y, x] == want, (y, x)
            # the source: the first valid positive-weight tap in tap order with the output's value
            first = next(q for q, w in zip(taps, weights) if w > 0 and d[q] == want)
            assert source[y, x] == first[0] + H * first[1], (y, x)
    assert kept == n_kept


def test_candidate_order_and_summation_order():
    """Non-dyadic weights: the output is a window value whose doubled W_le (summed in tap order) reaches the total while
    the next smaller value's does not -- checked with the same ordered sums written as Python floats."""
    H, W, r = 6, 7, 2
    rng = np.random.default_rng(11)
    d = holes(rng, rng.standard_normal((H, W)))
    pw = rng.random((H, W))
    im = image(rng, H, W, 3, dyadic=False)
    out, source, kept = MR.weighted_median(d, r, im, PARAMS["ramp"], pw)
    import contrast_restate as CR
    for y in range(H):
        for x in range(W):
            taps = [q for q in window(H, W, y, x, r) if np.isfinite(d[q])]
            ws = [float(CR.ramp(np.abs(im[y, x] - im[q]).max(), *PARAMS["ramp"]) * pw[q]) for q in taps]
            total = 0.0
            for w in ws:
                total = total + w

            def w_le(v):
                acc = 0.0
                for q, w in zip(taps, ws):
                    acc = acc + (w if d[q] <= v else 0.0)
                return acc
            if not total > 0:
                continue
            assert 2.0 * w_le(out[y, x]) >= total
            below = [d[q] for q in taps if d[q] < out[y, x]]
            assert all(2.0 * w_le(v) < total for v in below)
            sy, sx = source[y, x] % H, source[y, x] // H
            assert (sy, sx) in taps and d[sy, sx] == out[y, x] and ws[taps.index((sy, sx))] > 0


def test_no_weight_crosses_a_step_edge():
    """Constant on each side of a vertical image edge, salt noise on one side; a step ramp whose low level is 0: the
    other side's taps weigh nothing and the noise, a minority in every window, is voted out -- exactly constant sides."""
    H, W, edge = 12, 14, 6
    rng = np.random.default_rng(3)
    im = np.zeros((H, W, 1))
    im[:, edge:] = 1.0
    d = np.where(np.arange(W)[None, :] < edge, 2.0, 9.0) * np.ones((H, 1))
    salt = np.zeros((H, W), bool)
    salt[2::4, 1:edge:3] = True           # isolated pixels left of the edge
    noisy = np.where(salt, 50.0, d)
    for r in (1, 2, 4):
        out, source, kept = MR.weighted_median(noisy, r, im, (1.0, 0.0, 0.5, 0.5))
        assert np.array_equal(out, d) and kept == 0
        assert ((source // H < edge) == (np.arange(W)[None, :] < edge)).all()      # a source on the pixel's own side


def test_median_filter_masks():
    from stereo_amd import Contrast, StereoHipError
    from stereo_amd.mapfilter import MedianFilter
    status = np.array([[0, 1, 2], [3, 4, 0]], dtype=np.int32)
    pw, tg = MedianFilter(2).masks(status)
    assert pw.dtype == np.float64 and np.array_equal(pw, [[1, 0, 0], [0, 0, 1]])
    assert tg.dtype == np.int32 and np.array_equal(tg, [[0, 1, 1], [1, 1, 0]])
    assert MedianFilter(1, sources="all", targets="all").masks(status) == (None, None)
    pw, tg = MedianFilter(1, sources="all").masks(status)
    assert pw is None and np.array_equal(tg, status != 0)
    f = MedianFilter(3, Contrast(2, 0.5, 8, 40))
    assert f.radius == 3 and f.contrast.g1 == 40.0 and f.sources == "consistent" and f.targets == "filled"
    for bad in (dict(sources="some"), dict(targets="none"), dict(contrast=(1, 2, 3, 4))):
        with pytest.raises(StereoHipError):
            MedianFilter(1, **bad)


def test_take_planes():
    from stereo_amd import StereoHipError
    from stereo_amd.mapfilter import take_planes
    H, W = 3, 4
    planes = np.arange(4 * H * W, dtype=np.float64).reshape(4, H * W)
    source = np.arange(H * W).reshape(W, H).T[:, ::-1].astype(np.int32)           # every pixel takes its row's mirror
    got = take_planes(planes, source)
    assert got.shape == (4, H * W) and np.array_equal(got, planes[:, source.T.reshape(-1)])
    assert np.array_equal(take_planes(planes, np.arange(H * W)), planes)
    with pytest.raises(StereoHipError):
        take_planes(planes, np.full((H, W), H * W))
    with pytest.raises(StereoHipError):
        take_planes(planes[:, :-1], source)


# ---------------------------------------------------------------- refusals, before the device is looked for

def median_call(device, **change):
    """One of the two entries on small host arrays with one argument changed -> (rc, message)."""
    from stereo_amd import _lib
    from stereo_amd.contrast import _Params
    a = dict(H=2, W=3, radius=1, C=2, params=(1.0, 0.5, 0.1, 0.2), im=[0.25] * 12, pixel_weight=[1.0] * 6, targets=[1] * 6,
             d=[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], null=(), alias=None)
    a.update(change)
    keep = []

    def arr(name, values, dtype):
        if name in a["null"]:
            return None
        v = np.array(values, dtype=dtype)
        keep.append(v)
        return v.ctypes.data_as(C.c_void_p)
    d, im = arr("d", a["d"], np.float64), arr("im", a["im"], np.float64)
    pw, tg = arr("pixel_weight", a["pixel_weight"], np.float64), arr("targets", a["targets"], np.int32)
    inputs = dict(d=d, im=im, pixel_weight=pw, targets=tg)
    out, source = arr("out", [0.0] * 6, np.float64), arr("source", [0] * 6, np.int32)
    kept = arr("kept", [0], np.int32)
    if a["alias"] is not None:
        which, what = a["alias"]
        if which == "out":
            out = inputs.get(what, source)
        elif which == "source":
            source = inputs.get(what, kept)
        else:
            kept = inputs[what]
    par = None if "params" in a["null"] else C.byref(_Params(*a["params"]))
    args = [d, C.c_int(a["H"]), C.c_int(a["W"]), C.c_int(a["radius"]), im, C.c_int(a["C"]), par, pw, tg, out, source, kept]
    err = _lib.errbuf()
    L = _lib.lib()
    if device:
        rc = L.stereo_map_weighted_median_device(*args, None, err, C.c_size_t(len(err)))
    else:
        rc = L.stereo_map_weighted_median(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


REFUSALS = [
    (dict(H=0), "H and W must be at least 1"),
    (dict(W=-1), "H and W must be at least 1"),
    (dict(H=1 << 16, W=1 << 15), "below 2\\^31"),
    (dict(radius=0), "radius must be 1 .. 4 \\(got 0\\)"),
    (dict(radius=5), "radius must be 1 .. 4 \\(got 5\\)"),
    (dict(null=("d",)), "must not be NULL"),
    (dict(null=("out",)), "must not be NULL"),
    (dict(null=("kept",)), "must not be NULL"),
    (dict(null=("im",)), "given together"),
    (dict(null=("params",)), "given together"),
    (dict(C=0), "C must be at least 1"),
    (dict(params=(-1.0, 0.5, 0.1, 0.2)), "finite and non-negative"),
    (dict(params=(1.0, float("nan"), 0.1, 0.2)), "finite and non-negative"),
    (dict(params=(1.0, 0.5, 0.3, 0.2)), "g0 must not be above g1"),
    (dict(alias=("out", "d")), "must not be an input"),
    (dict(alias=("out", "im")), "must not be an input"),
    (dict(alias=("out", "pixel_weight")), "must not be an input"),
    (dict(alias=("source", "targets")), "must not be an input"),
    (dict(alias=("kept", "targets")), "must not be an input"),
    (dict(alias=("out", "source")), "must be three arrays"),
    (dict(alias=("source", "kept")), "must be three arrays"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_of_both_entries(change, message, device):
    rc, text = median_call(device, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_map_weighted_median_device:" if device else "stereo_map_weighted_median:")
    assert "no HIP device" not in text


def test_refusals_of_the_host_entry_only():
    for bad in (float("nan"), float("inf")):
        rc, text = median_call(False, im=[0.25] * 7 + [bad] + [0.25] * 4)
        assert rc != 0 and "im must be finite (pixel 1, channel 1)" in text and "no HIP device" not in text, text
    for bad in (-0.5, float("nan"), float("inf")):
        rc, text = median_call(False, pixel_weight=[1.0, 1.0, bad, 1.0, bad, 1.0])
        assert rc != 0 and "a pixel weight must be finite and non-negative (pixel 2)" in text, text
        assert "no HIP device" not in text


def test_optional_arguments_and_no_cpu_fallback():
    """im with params, pixel_weight, targets and source may all be absent; what is left is a call that needs the device
    and says so where there is none."""
    import stereo_amd
    for device in (False, True):
        for null in ((), ("im", "params"), ("pixel_weight", "targets", "source"), ("im", "params", "pixel_weight", "targets")):
            if device and stereo_amd.device_count() > 0:
                continue        # (host arrays are not device arrays: only the host entry may run them)
            rc, text = median_call(device, null=null)
            if stereo_amd.device_count() > 0:
                assert rc == 0, text
            else:
                assert rc != 0 and "no HIP device" in text, text


def test_python_refusals():
    from stereo_amd import Contrast, StereoHipError, mapfilter
    d = np.zeros((2, 3))
    assert mapfilter.max_radius() == 4 == MR.MAX_RADIUS
    with pytest.raises(StereoHipError, match="radius must be 1 .. 4"):
        mapfilter.weighted_median(d, 5)
    with pytest.raises(StereoHipError, match="given together"):
        mapfilter.weighted_median(d, 1, image=np.zeros((2, 3, 3)))
    with pytest.raises(StereoHipError, match="a Contrast is needed"):
        mapfilter.weighted_median(d, 1, image=np.zeros((2, 3, 3)), contrast=(1, 1, 0, 0))
    with pytest.raises(StereoHipError, match="the map's size"):
        mapfilter.weighted_median(d, 1, image=np.zeros((3, 3, 3)), contrast=Contrast(1, 1, 0, 0))
    with pytest.raises(StereoHipError, match="the map's size"):
        mapfilter.weighted_median(d, 1, pixel_weight=np.ones((3, 2)))
    with pytest.raises(StereoHipError, match="a pixel weight must be finite and non-negative \\(pixel 3\\)"):
        mapfilter.weighted_median(d, 1, pixel_weight=np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0]]))
    with pytest.raises(StereoHipError, match="needs the view's image"):
        mapfilter.MedianFilter(1, Contrast(1, 1, 0, 0)).apply(d, np.zeros((2, 3), np.int32))


def test_plug_in_refusals():
    from stereo_amd import StereoHipError, consistency
    out = consistency.PairResult()
    consistency.filter_views(out, None, None)
    assert out.left.filtered is None and out.left.filter_source is None
    with pytest.raises(StereoHipError, match="a mapfilter.MedianFilter is needed"):
        consistency.filter_views(out, 3, None)
    # filter_map refuses what cross_check refuses, before anything else is looked at
    from stereo_amd import MedianFilter, dispmap_globalstereo
    with pytest.raises(StereoHipError, match="filter_map: dispmap_globalstereo reaches its second view through a projection"):
        dispmap_globalstereo.__new__(dispmap_globalstereo).filter_map(MedianFilter(1))
