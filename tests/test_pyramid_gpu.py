"""The image pyramid on the device: stereo_pyramid_reduce / stereo_pyramid_expand and their device forms
against the restatement of the definitions (tests/pyramid_restate.py) byte for byte; solve_pair_ncc's smooth_weight; and
solve_pair_ncc_pyramid / dispmap_ncc.solve_pyramid against the same pipeline written by hand from the restated reduce
and expand, pair_volumes, solo TrwsPlans, band_restate and lr_restate."""
import functools

import numpy as np
import pytest

import band_restate
import lr_restate
import pyramid_restate as R
from pyramid_restate import same, same_bits
from test_consistency_gpu import rendered_pair, PH, PW, PK, UNARY_WEIGHT, TOL

pytestmark = pytest.mark.gpu

NEVER = -1e300
# odd and even sizes, both sides of a 64-lane tile along y and along x
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 7), (6, 8), (67, 3), (3, 67), (130, 5)]


def image(H, W, Cn, kind, seed):
    rng = np.random.default_rng([H, W, Cn, seed])
    if kind == "integers":
        return rng.integers(0, 256, size=(H, W, Cn)).astype(np.float64)
    return rng.uniform(-3.0, 260.0, size=(H, W, Cn)) * rng.choice([1.0, 1e-3, 1e3], size=(H, W, Cn))


def coarse_map(Hc, Wc, seed, salted=True):
    rng = np.random.default_rng([Hc, Wc, seed, 3])
    d = rng.integers(-8, 120, size=(Hc, Wc)) / 4.0
    if salted:
        salt = rng.random((Hc, Wc))
        d[salt < 0.08] = np.nan
        d[(salt >= 0.08) & (salt < 0.12)] = np.inf
        d[(salt >= 0.12) & (salt < 0.16)] = -np.inf
    return d


# ---------------------------------------------------------------- 1: against the restatement

@pytest.mark.parametrize("kind", ["integers", "doubles"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_reduce_and_expand_equal_the_restatement(shape, Cn, kind, hip):
    from stereo_amd import pyramid
    H, W = shape
    im = image(H, W, Cn, kind, 1)
    want = R.reduce(im)
    got = pyramid.reduce(im)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    assert got.shape == (Hc, Wc, Cn) and same_bits(got, want)
    if Cn == 1:
        assert same_bits(pyramid.reduce(im[:, :, 0]), want[:, :, 0])         # an H x W image comes back H x W
    d = coarse_map(Hc, Wc, 2)
    for mode, name in ((0, "nearest"), (1, "guided")):
        want_out, want_src = R.expand(d, (H, W), mode, im, want)
        out, src = pyramid.expand(d, (H, W), name, im, want)
        assert out.shape == (H, W) and src.dtype == np.int32
        assert same_bits(out, want_out) and np.array_equal(src, want_src), (mode, shape)
        out2, none = pyramid.expand(d, (H, W), mode, im, want, want_source=False)
        assert none is None and same_bits(out2, want_out)
    out, src = pyramid.expand(d, (H, W), "nearest")                          # the nearest mode needs no images
    assert same_bits(out, R.expand(d, (H, W), 0)[0]) and (src == 0).all()
    assert np.array_equal(np.isnan(out), np.isnan(np.repeat(np.repeat(d, 2, 0), 2, 1)[:H, :W] * 2.0))


# ---------------------------------------------------------------- 2: crafted cases of the expansion

def test_expand_crafted_cases(hip):
    from stereo_amd import pyramid
    H, W, Hc, Wc = 6, 8, 3, 4
    d = np.arange(12, dtype=np.float64).reshape(Hc, Wc) + 1.0
    flat_f, flat_c = np.full((H, W, 3), 7.0), np.full((Hc, Wc, 3), 5.0)
    out, src = pyramid.expand(d, (H, W), "guided", flat_f, flat_c)
    assert (src == 0).all() and np.array_equal(out, 2.0 * np.repeat(np.repeat(d, 2, 0), 2, 1))      # a constant image: all ties
    # an exact match at candidate 3: fine pixel (3, 5), parent (1, 2), ny = 2, nx = 3
    coarse = np.random.default_rng(4).uniform(0, 255, size=(Hc, Wc, 3))
    fine = np.random.default_rng(5).uniform(300, 400, size=(H, W, 3))
    fine[3, 5] = coarse[2, 3]
    out, src = pyramid.expand(d, (H, W), "guided", fine, coarse)
    assert R.candidates(3, 5, Hc, Wc)[3] == (2, 3) and src[3, 5] == 3 and out[3, 5] == 2.0 * d[2, 3]
    # ... and skipped once its disparity is not finite; nothing else moves
    d2 = d.copy()
    d2[2, 3] = np.inf
    out2, src2 = pyramid.expand(d2, (H, W), "guided", fine, coarse)
    want2 = R.expand(d2, (H, W), 1, fine, coarse)
    assert src2[3, 5] != 3 and src2[3, 5] >= 0 and np.isfinite(out2[3, 5])
    assert same_bits(out2, want2[0]) and np.array_equal(src2, want2[1])
    # the parent itself is not finite: the first finite candidate starts as the best
    d3 = d.copy()
    d3[1, 2] = np.nan
    out3, src3 = pyramid.expand(d3, (H, W), "guided", flat_f, flat_c)
    assert src3[3, 5] == 1 and out3[3, 5] == 2.0 * d[2, 2] and src3[2, 4] == 1 and out3[2, 4] == 2.0 * d[0, 2]
    out3n, src3n = pyramid.expand(d3, (H, W), "nearest")
    assert np.isnan(out3n[2:4, 4:6]).all() and (src3n == 0).all()             # nearest doubles whatever is there
    # all four candidates not finite: NaN and -1
    d4 = d.copy()
    d4[1:3, 2:4] = [[np.nan, np.inf], [-np.inf, np.nan]]
    out4, src4 = pyramid.expand(d4, (H, W), "guided", fine, coarse)
    assert np.isnan(out4[3, 5]) and src4[3, 5] == -1
    assert same_bits(out4, R.expand(d4, (H, W), 1, fine, coarse)[0])
    # border pixels: (0, 0) has both neighbours clamped onto the parent; a parent that is not finite leaves nothing
    assert src[0, 0] == 0 and out[0, 0] == 2.0 * d[0, 0] and src[H - 1, W - 1] == 0
    d5 = d.copy()
    d5[0, 0] = np.nan
    out5, src5 = pyramid.expand(d5, (H, W), "guided", fine, coarse)
    assert np.isnan(out5[0, 0]) and src5[0, 0] == -1 and src5[1, 1] >= 1 and np.isfinite(out5[1, 1])
    # a NaN image pixel: every distance is NaN, the earliest finite candidate stays
    fine6 = fine.copy()
    fine6[3, 5, 1] = np.nan
    out6, src6 = pyramid.expand(d, (H, W), "guided", fine6, coarse)
    assert src6[3, 5] == 0 and out6[3, 5] == 2.0 * d[1, 2]
    out6b, src6b = pyramid.expand(d3, (H, W), "guided", fine6, coarse)
    assert src6b[3, 5] == 1 and out6b[3, 5] == 2.0 * d[2, 2]
    # a NaN in the coarse image at candidate 0 only: its NaN distance stands, no later one is "smaller"
    coarse7 = coarse.copy()
    coarse7[1, 2, 0] = np.nan
    out7, src7 = pyramid.expand(d, (H, W), "guided", fine, coarse7)
    assert src7[3, 5] == 0 and same_bits(out7, R.expand(d, (H, W), 1, fine, coarse7)[0])


# ---------------------------------------------------------------- 3: device forms

def test_device_forms_on_a_side_stream_give_the_host_forms_bits(hip):
    import torch
    from stereo_amd import pyramid
    H, W, Cn = 67, 131, 3
    im = image(H, W, Cn, "doubles", 9)
    Hc, Wc = pyramid.coarse_size(H, W)
    d = coarse_map(Hc, Wc, 9)
    red = pyramid.reduce(im)
    host = {name: pyramid.expand(d, (H, W), name, im, red) for name in ("nearest", "guided")}
    d_im = pyramid.image_to_device(im)
    d_d = torch.from_numpy(np.ascontiguousarray(d.T)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    d_red = pyramid.reduce_device(d_im, stream=side)
    dev = {name: pyramid.expand_device(d_d, (H, W), name, d_im, d_red, stream=side) for name in ("nearest", "guided")}
    no_source = pyramid.expand_device(d_d, (H, W), "guided", d_im, d_red, stream=side, want_source=False)
    side.synchronize()
    assert tuple(d_red.shape) == (Cn, Wc, Hc) and same_bits(pyramid.image_to_host(d_red), red)
    for name in ("nearest", "guided"):
        assert same_bits(dev[name][0].cpu().numpy().T, host[name][0])
        assert np.array_equal(dev[name][1].cpu().numpy().T, host[name][1])
    assert no_source[1] is None and same_bits(no_source[0].cpu().numpy().T, host["guided"][0])
    with pytest.raises(hip.StereoHipError, match="column-major"):
        pyramid.reduce_device(d_im.permute(0, 2, 1))
    with pytest.raises(hip.StereoHipError, match="size"):
        pyramid.expand_device(d_d, (H, W), "guided", d_im, d_red[:, :-1].contiguous())
    one = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    with pytest.raises(hip.StereoHipError, match="alias"):
        pyramid.expand_device(one, (1, 1), "nearest", out=one)


# ---------------------------------------------------------------- 4: repeated reduction

def test_two_reductions_are_the_4x4_block_mean(hip):
    from stereo_amd import pyramid
    H, W, Cn = 72, 12, 3
    im = image(H, W, Cn, "integers", 6)
    twice = pyramid.reduce(pyramid.reduce(im))
    want = im.reshape(H // 4, 4, W // 4, 4, Cn).sum(axis=(1, 3)) / 16.0     # integers below 2^12: exact
    assert twice.shape == (H // 4, W // 4, Cn) and np.array_equal(twice, want)


# ---------------------------------------------------------------- 5: solve_pair_ncc's smooth_weight

ITERS = 4


def assert_same_pair(a, b):
    for va, vb in zip(a.views, b.views):
        assert (va.energy, va.lower_bound, va.iterations, va.paths) == (vb.energy, vb.lower_bound, vb.iterations, vb.paths)
        for field in ("labels", "dispmap", "status", "source"):
            assert np.array_equal(getattr(va, field), getattr(vb, field)), field
        assert same(va.residual, vb.residual) and same(va.filled, vb.filled)
        assert len(va.maps) == len(vb.maps) and all(same_bits(x, y) for x, y in zip(va.maps, vb.maps))


def test_smooth_weight_one_is_the_call_without_it(hip):
    disparities = np.arange(PK, dtype=np.float64)
    for kernel in (1, 2):
        for extra in (dict(), dict(refine_iters=2, band_levels=[[-0.5, 0.0, 0.5]])):
            args = (rendered_pair(), disparities, kernel, UNARY_WEIGHT, TOL, ITERS, NEVER)
            a = hip.solve_pair_ncc(*args, check_tol=1.0, **extra)
            b = hip.solve_pair_ncc(*args, check_tol=1.0, smooth_weight=1.0, **extra)
            assert list(a.times) == list(b.times)
            assert_same_pair(a, b)


def test_smooth_weight_two_equals_solo_plans_with_doubled_weights(hip):
    from stereo_amd import consistency, terms as T
    from stereo_amd.trws import TrwsPlan
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc(rendered_pair(), disparities, 2, UNARY_WEIGHT, TOL, ITERS, NEVER, smooth_weight=2.0)
    plain = hip.solve_pair_ncc(rendered_pair(), disparities, 2, UNARY_WEIGHT, TOL, ITERS, NEVER)
    conn = T.construct_neighborhood(PH, PW)
    E = conn.shape[1]
    for view, unary, other in zip(got.views, consistency.pair_unaries(rendered_pair(), disparities, UNARY_WEIGHT), plain.views):
        plan = TrwsPlan(2, PK, PH * PW, conn)
        plan.upload(unary, 2.0 * np.ones(E), TOL, positions=disparities)
        plan.iterate(ITERS, NEVER)
        labels, en, lb, it = plan.result()
        plan.close()
        assert np.array_equal(view.labels, labels) and (view.energy, view.lower_bound, view.iterations) == ([en], [lb], [it])
        assert view.energy != other.energy                       # the weight reached the solver


# ---------------------------------------------------------------- 6: the pyramid solve against the pipeline by hand

BAND = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
BANDS = {1: None,                                               # the default: one band [-2 .. 2] per level
         2: [[BAND, np.array([-0.5, 0.0, 0.5])], [BAND]]}       # level 0: the band and a sub-pixel level; level 1: the band
CHECK_TOL = 1.0


def bands_of(levels):
    return [[BAND]] * levels if BANDS[levels] is None else BANDS[levels]


@functools.lru_cache(maxsize=None)
def restated_images(flipped=False):
    """Per level 0 .. 2 the two images of the rendered pair (flipped: the mirrored object's own pair, flipped columns in
    swapped order), reduced by the restatement."""
    left, right = rendered_pair()
    out = [[right[:, ::-1].copy(), left[:, ::-1].copy()] if flipped else [left, right]]
    for _ in range(2):
        out.append([R.reduce(im) for im in out[-1]])
    return out


def view_by_hand(volumes, guides, disparities, levels, mode, kernel, relgap):
    """One view's passes.  volumes[l]: the view's D x N volume at level l; guides[l]: the view's own image.
    -> per level a dict(maps, labels, energy, bound, iters, paths, expanded, expand_source)."""
    from stereo_amd import terms as T
    from stereo_amd.trws import TrwsPlan
    out = [dict(maps=[], energy=[], bound=[], iters=[], expanded=None, expand_source=None) for _ in range(levels + 1)]

    def run(rec, plan, to_map):
        plan.iterate(ITERS, relgap)
        rec["labels"], en, lb, it = plan.result()
        plan.close()
        rec["energy"].append(en); rec["bound"].append(lb); rec["iters"].append(it)
        rec["maps"].append(to_map(rec["labels"]))

    L = levels
    H, W = guides[L].shape[:2]
    conn = T.construct_neighborhood(H, W)
    tol_l, weight = R.level_model(kernel, TOL, L)
    disp = R.level_disparities(disparities, L)
    plan = TrwsPlan(kernel, disp.shape[0], H * W, conn)
    plan.upload(UNARY_WEIGHT * (1.0 - volumes[L]), weight * np.ones(conn.shape[1]), tol_l, positions=disp)
    run(out[L], plan, lambda labels: disp[labels.astype(np.int64) - 1].reshape(W, H).T)
    for l in range(levels - 1, -1, -1):
        H, W = guides[l].shape[:2]
        conn = T.construct_neighborhood(H, W)
        tol_l, weight = R.level_model(kernel, TOL, l)
        disp = R.level_disparities(disparities, l)
        rec = out[l]
        rec["expanded"], rec["expand_source"] = R.expand(out[l + 1]["maps"][-1], (H, W), mode, guides[l], guides[l + 1])
        base = rec["expanded"]
        hwd = volumes[l].reshape((disp.shape[0], H, W), order="F").transpose(1, 2, 0)
        for offsets in bands_of(levels)[l]:
            unary, q, qprim = band_restate.band_inputs(hwd, disp, UNARY_WEIGHT, base, offsets, conn)
            plan = TrwsPlan(kernel, len(offsets), H * W, conn)
            plan.upload(unary, weight * np.ones(conn.shape[1]), tol_l, q=q, qprim=qprim)
            run(rec, plan, lambda labels: band_restate.band_apply(base, labels, offsets))
            base = rec["maps"][-1]
    return out


@functools.lru_cache(maxsize=None)
def pair_by_hand(levels, mode, kernel):
    from stereo_amd import consistency
    images = restated_images()
    disparities = np.arange(PK, dtype=np.float64)
    volumes = [consistency.pair_volumes(images[l], R.level_disparities(disparities, l)) for l in range(levels + 1)]
    views = [view_by_hand([v[i] for v in volumes], [im[i] for im in images], disparities, levels, mode, kernel, NEVER)
             for i in range(2)]
    for l in range(levels + 1):
        maps = [views[i][l]["maps"][-1] for i in range(2)]
        for i, direction in ((0, 1), (1, -1)):
            rec = views[i][l]
            rec["status"], rec["residual"] = lr_restate.lr_check(maps[i], maps[1 - i], direction, CHECK_TOL / 2 ** l)
            rec["filled"], rec["source"] = lr_restate.lr_fill(maps[i], rec["status"])
    return views


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("expand", ["nearest", "guided"])
@pytest.mark.parametrize("levels", [1, 2])
def test_solve_pair_ncc_pyramid_equals_the_pipeline_by_hand(levels, expand, kernel, hip):
    from stereo_amd import pyramid
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_pyramid(rendered_pair(), disparities, kernel, UNARY_WEIGHT, TOL, levels, ITERS, NEVER,
                                     bands=BANDS[levels], expand=expand, check_tol=CHECK_TOL)
    want = pair_by_hand(levels, pyramid.MODES[expand], kernel)
    assert len(got.levels) == levels + 1 and got.left is got.levels[0].left
    for l in range(levels + 1):
        assert np.array_equal(got.disparities[l], R.level_disparities(disparities, l))
        assert (got.tol[l], got.smooth_weight[l]) == R.level_model(kernel, TOL, l)
        for view, ref in zip(got.levels[l].views, (want[0][l], want[1][l])):
            assert np.array_equal(view.labels, ref["labels"]), l
            assert (view.energy, view.lower_bound, view.iterations) == (ref["energy"], ref["bound"], ref["iters"]), l
            assert len(view.maps) == len(ref["maps"]) == (1 if l == levels else len(bands_of(levels)[l]))
            assert all(same_bits(a, b) for a, b in zip(view.maps, ref["maps"])) and view.dispmap is view.maps[-1]
            assert len(view.paths) == len(view.maps) and all(p in (1, 2, 3, 4, 5) for p in view.paths)
            if l < levels:
                assert view.paths == [2] * len(view.maps)        # a band is a K <= 64 problem with positions per edge: Pipe
            assert np.array_equal(view.status, ref["status"]) and same(view.residual, ref["residual"])
            assert same(view.filled, ref["filled"]) and np.array_equal(view.source, ref["source"])
            if l < levels:
                assert same_bits(view.expanded, ref["expanded"]) and np.array_equal(view.expand_source, ref["expand_source"])
                assert {"expand", "volumes", "band_1", "band_1_check_fill"} <= set(got.levels[l].times)
            else:
                assert view.expanded is None
    assert {"reduce"} | {"level_%d" % l for l in range(levels + 1)} == set(got.times)


def test_maxiter_per_scale(hip):
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_pyramid(rendered_pair(), disparities, 1, UNARY_WEIGHT, TOL, 2, [2, 3, 5], NEVER)
    assert [got.levels[l].left.iterations for l in range(3)] == [[2.0], [3.0], [5.0]]


# ---------------------------------------------------------------- 7: the objects

def test_dispmap_ncc_solve_pyramid_plain_and_mirrored(hip):
    from stereo_amd import terms as T
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        images = restated_images(flipped=obj._mirrored)
        assert all(np.array_equal(a, b) for a, b in zip(images[0], obj.images))
        volumes = [T.ncc_volume(images[l][0], images[l][1], R.level_disparities(disparities, l), 2, layout=1) for l in range(3)]
        want = view_by_hand(volumes, [im[0] for im in images], disparities, 2, 1, 1, 0.0)
        out = obj.solve_pyramid(2, bands=BANDS[2], maxiter=ITERS, expand="guided")
        final = want[0]["maps"][-1]
        # (the object keeps planes [0 0 1 -d]: a disparity 0 comes back as -0, so values are compared here, bytes below)
        assert same(obj.current_dispmap(), final[:, ::-1] if obj._mirrored else final)
        assert same_bits(out.dispmap, final)
        for l in range(3):
            assert (out.energy[l], out.lower_bound[l], out.iterations[l]) == (want[l]["energy"], want[l]["bound"], want[l]["iters"])
            assert all(same_bits(a, b) for a, b in zip(out.maps[l], want[l]["maps"]))
        assert np.isfinite(obj.energy())
    glob = object.__new__(hip.dispmap_globalstereo)
    with pytest.raises(hip.StereoHipError, match="dispmap_globalstereo"):
        glob.solve_pyramid(2)
