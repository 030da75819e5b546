"""A pyramid level's volume as the block mean of the finer one, on the device:
stereo_pyramid_reduce_volume and its device form against the restatement of the definition
(tests/pyramid_volume_restate.py) byte for byte; solve_pair_ncc's `volumes`; and unary="blocks" in
solve_pair_ncc_pyramid / dispmap_ncc.solve_pyramid against the pipeline written by hand (test_pyramid_gpu.view_by_hand)
on the restated block volumes."""
import functools

import numpy as np
import pytest

import band_restate
import lr_restate
import pyramid_restate as R
import pyramid_volume_restate as RV
from pyramid_restate import same, same_bits
from test_consistency_gpu import rendered_pair, PK, UNARY_WEIGHT, TOL
from test_pyramid_gpu import BANDS, CHECK_TOL, ITERS, NEVER, SHAPES, assert_same_pair, bands_of, view_by_hand

pytestmark = pytest.mark.gpu


def crafted_samples(D):
    """For the slices 2 .. D + 1: on a slice, exactly midway between two (the tie goes to the larger index), the first
    and the last slice, a quarter off a slice, below the range and above it (-1e6 enters the sum in the defined order)."""
    lo, hi = 2.0, D + 1.0
    return np.array([lo + D // 2, lo + 0.5, lo, hi, lo + D // 2 + 0.25, lo - 1.25, hi + 1.75])


def volume(H, W, D, kind, seed):
    if kind == "dyadic":
        return band_restate.volume(H, W, D, seed)
    return np.random.default_rng([H, W, D, seed, 5]).uniform(-1.0, 1.0, size=(H, W, D))


@functools.lru_cache(maxsize=None)
def case(H, W, D, shuffled, kind, Kc=None):
    """(volume H x W x D, slices, sample_at, the restated reduction): worked out once, shared by the layouts."""
    vol = volume(H, W, D, kind, 3)
    slices = band_restate.disparities_for(D, shuffled)
    sample_at = crafted_samples(D)
    if Kc is not None:
        more = 1.0 + (D + 2.0) * np.random.default_rng([D, Kc]).integers(0, 64, size=Kc) / 64.0
        sample_at = np.concatenate([sample_at, more])[:Kc]
    return vol, slices, sample_at, RV.reduce_volume(vol, slices, sample_at)


def check(H, W, D, shuffled, kind, layout, Kc=None):
    from stereo_amd import pyramid
    vol, slices, sample_at, want = case(H, W, D, shuffled, kind, Kc)
    got = pyramid.reduce_volume(RV.to_layout(vol, layout), (H, W), slices, sample_at, layout)
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    assert got.shape == ((Hc, Wc, len(sample_at)) if layout == 0 else (len(sample_at), Hc * Wc))
    assert same_bits(RV.from_layout(got, Hc, Wc, layout), want), (H, W, D, shuffled, kind, layout, Kc)
    return want


# ---------------------------------------------------------------- 1: against the restatement

@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_reduce_volume_equals_the_restatement(shape, layout, hip):
    for D in (1, 3, 9):
        for shuffled in (False, True):
            want = check(*shape, D, shuffled, "dyadic", layout)
            assert (want[:, :, 5] == -1e6).all() and (want[:, :, 6] == -1e6).all() and (np.abs(want[:, :, 2:4]) <= 1.0).all()
    check(*shape, 9, False, "doubles", layout)
    check(*shape, 9, True, "doubles", layout)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("Kc", [1, 7, 70])          # 70 runs past one wave along j in layout 1
def test_reduce_volume_sample_counts(Kc, layout, hip):
    for shuffled in (False, True):
        check(5, 7, 9, shuffled, "dyadic", layout, Kc)


def test_the_tie_goes_to_the_larger_index_and_the_ends_are_the_slices(hip):
    from stereo_amd import pyramid
    vol, slices, sample_at, want = case(6, 8, 9, False, "dyadic")
    block = lambda a: 0.25 * (((a[0::2, 0::2] + a[1::2, 0::2]) + a[0::2, 1::2]) + a[1::2, 1::2])
    assert np.array_equal(want[:, :, 0], block(vol[:, :, 4])) and np.array_equal(want[:, :, 2], block(vol[:, :, 0]))
    assert np.array_equal(want[:, :, 3], block(vol[:, :, 8]))
    # 2.5 is midway between the slices 2 and 3: the parabola is the one around slice 3 (index 1), not around 2 (the end)
    v = RV.OT.sample_ncc_from_disp(vol, slices, np.full(48, 2.5))
    assert not np.array_equal(v, vol[:, :, 0]) and np.array_equal(want[:, :, 1], block(v))
    assert same_bits(pyramid.reduce_volume(vol, (6, 8), slices, sample_at), want)


def test_the_paths_past_the_launch_limits(hip):
    """Layout 1 with more samples than a block stages in LDS (every lane looks its own slice up); layout 0 with more
    samples than gridDim.z and more columns than gridDim.y (a block strides over them)."""
    from stereo_amd import pyramid
    vol = volume(2, 3, 3, "doubles", 8)
    slices = band_restate.disparities_for(3, False)
    for layout, Kc in ((1, 8200), (0, 65600), (1, 65600)):
        sample_at = np.resize(crafted_samples(3), Kc)
        got = pyramid.reduce_volume(RV.to_layout(vol, layout), (2, 3), slices, sample_at, layout)
        assert same_bits(RV.from_layout(got, 1, 2, layout), RV.reduce_volume(vol, slices, sample_at)), (layout, Kc)
    W = 2 * 65535 + 3                                                 # Wc = 65537 columns
    wide = volume(1, W, 2, "doubles", 9)
    slices = band_restate.disparities_for(2, False)
    want = RV.reduce_volume(wide, slices, [2.25, 3.0])
    for layout in (0, 1):
        got = pyramid.reduce_volume(RV.to_layout(wide, layout), (1, W), slices, [2.25, 3.0], layout)
        assert same_bits(RV.from_layout(got, 1, (W + 1) // 2, layout), want), layout


# ---------------------------------------------------------------- 2: the device form, level_volumes

def test_device_form_on_a_side_stream_gives_the_host_forms_bits(hip):
    import torch
    from stereo_amd import pyramid
    H, W, D = 67, 131, 9
    vol, slices, sample_at, want = case(H, W, D, False, "doubles", 70)
    Hc, Wc = pyramid.coarse_size(H, W)
    for layout in (0, 1):
        host = pyramid.reduce_volume(RV.to_layout(vol, layout), (H, W), slices, sample_at, layout)
        assert same_bits(RV.from_layout(host, Hc, Wc, layout), want)
        d_vol = torch.from_numpy(RV.to_layout(vol, layout).reshape(-1, order="F").copy()).cuda()
        d_slices, d_sample_at = torch.from_numpy(slices.copy()).cuda(), torch.from_numpy(sample_at.copy()).cuda()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        dev = pyramid.reduce_volume_device(d_vol, (H, W), slices, sample_at, layout, stream=side, d_disparities=d_slices,
                                           d_sample_at=d_sample_at)
        into = torch.zeros(Hc * Wc * 70, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert pyramid.reduce_volume_device(d_vol, (H, W), slices, sample_at, layout, out=into, stream=side) is into
        side.synchronize()
        assert dev.dtype == torch.float64 and tuple(dev.shape) == (Hc * Wc * 70,)
        assert dev.cpu().numpy().tobytes() == host.reshape(-1, order="F").tobytes() == into.cpu().numpy().tobytes()
    with pytest.raises(hip.StereoHipError, match="contiguous"):
        pyramid.reduce_volume_device(torch.zeros(2 * H * W * D, dtype=torch.float64, device="cuda")[::2], (H, W), slices, sample_at)
    with pytest.raises(hip.StereoHipError, match="must hold %d elements" % (H * W * D)):
        pyramid.reduce_volume_device(d_vol[:-1], (H, W), slices, sample_at)
    with pytest.raises(hip.StereoHipError, match="must hold %d elements" % (Hc * Wc * 70)):
        pyramid.reduce_volume_device(d_vol, (H, W), slices, sample_at, out=into[:-1])
    with pytest.raises(hip.StereoHipError, match="contiguous"):
        pyramid.reduce_volume_device(d_vol.float(), (H, W), slices, sample_at)
    one = torch.zeros(1, dtype=torch.float64, device="cuda")
    with pytest.raises(hip.StereoHipError, match="alias"):
        pyramid.reduce_volume_device(one, (1, 1), [2.0], [2.0], out=one)


@pytest.mark.parametrize("layout", [0, 1])
def test_level_volumes_are_the_restated_reductions_level_by_level(layout, hip):
    from stereo_amd import pyramid
    H, W, D = 13, 22, 9
    vol = volume(H, W, D, "doubles", 4)
    slices = np.arange(3.0, 12.0)
    got = pyramid.level_volumes(RV.to_layout(vol, layout), (H, W), slices, 2, layout)
    want, size = vol, (H, W)
    assert len(got) == 3 and same_bits(RV.from_layout(got[0], H, W, layout), vol)
    for l in (1, 2):
        finer, coarser = R.level_disparities(slices, l - 1), R.level_disparities(slices, l)
        want = RV.reduce_volume(want, finer, RV.level_sample_at(finer, coarser))
        size = ((size[0] + 1) // 2, (size[1] + 1) // 2)
        assert same_bits(RV.from_layout(got[l], size[0], size[1], layout), want) and not (want == -1e6).any(), l


# ---------------------------------------------------------------- 3: the keywords that change nothing

def test_solve_pair_ncc_with_its_own_volumes_is_the_call_without_them(hip):
    from stereo_amd import consistency
    disparities = np.arange(PK, dtype=np.float64)
    for kernel, extra in ((1, dict()), (2, dict(refine_iters=2, band_levels=[[-0.5, 0.0, 0.5]]))):
        args = (rendered_pair(), disparities, kernel, UNARY_WEIGHT, TOL, ITERS, NEVER)
        a = hip.solve_pair_ncc(*args, check_tol=1.0, **extra)
        b = hip.solve_pair_ncc(*args, check_tol=1.0, volumes=consistency.pair_volumes(rendered_pair(), disparities), **extra)
        assert list(a.times) == list(b.times)
        assert_same_pair(a, b)
    with pytest.raises(hip.StereoHipError, match="volumes must be the two D x N volumes"):
        hip.solve_pair_ncc(*args, volumes=[np.zeros((PK, 5))] * 2)


def test_unary_images_is_the_call_without_the_keyword(hip):
    disparities = np.arange(PK, dtype=np.float64)
    args = (rendered_pair(), disparities, 2, UNARY_WEIGHT, TOL, 2, ITERS, NEVER)
    a = hip.solve_pair_ncc_pyramid(*args, bands=BANDS[2])
    b = hip.solve_pair_ncc_pyramid(*args, bands=BANDS[2], unary="images")
    assert a.unary == b.unary == "images" and set(a.times) == set(b.times) and "volumes" not in a.times
    for l in range(3):
        assert_same_pair(a.levels[l], b.levels[l])
        assert list(a.levels[l].times) == list(b.levels[l].times)
        for va, vb in zip(a.levels[l].views, b.levels[l].views):
            assert (va.expanded is None and vb.expanded is None) if l == 2 else \
                (same_bits(va.expanded, vb.expanded) and np.array_equal(va.expand_source, vb.expand_source))


# ---------------------------------------------------------------- 4: unary="blocks" against the pipeline by hand

def restated_level_volumes(hwd, disparities, levels):
    """Per level 0 .. levels the D x N volume: the restated reductions of the H x W x D volume `hwd`."""
    out = [hwd]
    for l in range(1, levels + 1):
        finer, coarser = R.level_disparities(disparities, l - 1), R.level_disparities(disparities, l)
        out.append(RV.reduce_volume(out[-1], finer, RV.level_sample_at(finer, coarser)))
    return [RV.to_layout(v, 1) for v in out]


def cropped_pair(crop):
    return tuple(im[:crop[0], :crop[1]].copy() for im in rendered_pair())


@functools.lru_cache(maxsize=None)
def blocks_by_hand(levels, mode, kernel, crop):
    from stereo_amd import consistency
    images = [list(cropped_pair(crop))]
    for _ in range(levels):
        images.append([R.reduce(im) for im in images[-1]])
    disparities = np.arange(PK, dtype=np.float64)
    H, W = crop
    full = consistency.pair_volumes(images[0], disparities)
    views = []
    for i in range(2):
        hwd = np.asarray(full[i]).reshape((PK, H, W), order="F").transpose(1, 2, 0)
        views.append(view_by_hand(restated_level_volumes(hwd, disparities, levels), [im[i] for im in images], disparities,
                                  levels, mode, kernel, NEVER))
    for l in range(levels + 1):
        maps = [views[i][l]["maps"][-1] for i in range(2)]
        for i, direction in ((0, 1), (1, -1)):
            rec = views[i][l]
            rec["status"], rec["residual"] = lr_restate.lr_check(maps[i], maps[1 - i], direction, CHECK_TOL / 2 ** l)
            rec["filled"], rec["source"] = lr_restate.lr_fill(maps[i], rec["status"])
    return views


@pytest.mark.parametrize("levels,expand,kernel,crop", [
    (1, "nearest", 1, (24, 40)), (2, "guided", 2, (24, 40)), (1, "guided", 2, (24, 40)), (2, "nearest", 1, (24, 40)),
    (2, "guided", 1, (23, 39)),                      # odd sizes: replication runs through the solve
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_unary_blocks_equals_the_pipeline_by_hand(levels, expand, kernel, crop, hip):
    from stereo_amd import pyramid
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_pyramid(cropped_pair(crop), disparities, kernel, UNARY_WEIGHT, TOL, levels, ITERS, NEVER,
                                     bands=BANDS[levels], expand=expand, check_tol=CHECK_TOL, unary="blocks")
    want = blocks_by_hand(levels, pyramid.MODES[expand], kernel, crop)
    assert got.unary == "blocks" and len(got.levels) == levels + 1
    assert {"reduce", "volumes"} | {"level_%d" % l for l in range(levels + 1)} == set(got.times)
    for l in range(levels + 1):
        assert np.array_equal(got.disparities[l], R.level_disparities(disparities, l))
        for view, ref in zip(got.levels[l].views, (want[0][l], want[1][l])):
            assert np.array_equal(view.labels, ref["labels"]), l
            assert (view.energy, view.lower_bound, view.iterations) == (ref["energy"], ref["bound"], ref["iters"]), l
            assert len(view.maps) == len(ref["maps"]) == (1 if l == levels else len(bands_of(levels)[l]))
            assert all(same_bits(a, b) for a, b in zip(view.maps, ref["maps"])) and view.dispmap is view.maps[-1]
            assert np.array_equal(view.status, ref["status"]) and same(view.residual, ref["residual"])
            assert same(view.filled, ref["filled"]) and np.array_equal(view.source, ref["source"])
            if l < levels:
                assert same_bits(view.expanded, ref["expanded"]) and np.array_equal(view.expand_source, ref["expand_source"])
                assert {"expand", "volumes", "band_1", "band_1_check_fill"} <= set(got.levels[l].times)
            else:
                assert view.expanded is None


def test_blocks_and_images_solve_different_level_models(hip):
    disparities = np.arange(PK, dtype=np.float64)
    args = (rendered_pair(), disparities, 1, UNARY_WEIGHT, TOL, 1, ITERS, NEVER)
    a = hip.solve_pair_ncc_pyramid(*args, unary="images")
    b = hip.solve_pair_ncc_pyramid(*args, unary="blocks")
    assert a.levels[1].left.energy != b.levels[1].left.energy          # the keyword reached the coarsest solve


def test_dispmap_ncc_solve_pyramid_blocks_plain_and_mirrored(hip):
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        images = [list(obj.images[:2])]
        for _ in range(2):
            images.append([R.reduce(im) for im in images[-1]])
        own = np.array(obj.ncc)                                          # H x W x D, the object's internal columns
        want = view_by_hand(restated_level_volumes(own, disparities, 2), [im[0] for im in images], disparities, 2, 1, 1, 0.0)
        out = obj.solve_pyramid(2, bands=BANDS[2], maxiter=ITERS, expand="guided", unary="blocks")
        assert same_bits(obj.ncc, own) and out.unary == "blocks" and out.times["volumes"] > 0
        final = want[0]["maps"][-1]
        assert same(obj.current_dispmap(), final[:, ::-1] if obj._mirrored else final)
        assert same_bits(out.dispmap, final)
        for l in range(3):
            assert (out.energy[l], out.lower_bound[l], out.iterations[l]) == (want[l]["energy"], want[l]["bound"], want[l]["iters"])
            assert all(same_bits(a, b) for a, b in zip(out.maps[l], want[l]["maps"]))
            if l < 2:
                assert same_bits(out.expanded[l], want[l]["expanded"])
