"""Weighted scanline aggregation and the contrast builders on the device: the two new aggregation
entries against the NumPy restatement (tests/scanline_weighted_restate.py, which test_scanline_weighted_cpu holds
against first principles) bit for bit on S, labels, map and confidence -- a minimum of finite doubles does not depend on
its order and every other operation is one rounded add or product, so there is no tolerance to choose; against the
existing entries where the two definitions coincide; the builders against tests/contrast_restate.py bit for bit; and the
Python surface (solve_pair_ncc_scanline, solve_pair_ncc, dispmap_ncc) against its pieces.

The shapes are the smallest at which the chain geometry (one pixel, one row, one column, a square of 2, both
orientations of a rectangle whose sides differ), the lane grouping (D around every power of two's group, around 64 and
around the wide kernel's 128, 192, 256), the padded columns (step weights of 0.0 at D below its group's size) and the
chain count (more chains than one wave carries, more waves than one) can each go wrong."""
import functools
import os

import numpy as np
import pytest

import contrast_restate as CR
import first_principles as fp
import scanline_restate as R
import scanline_weighted_restate as WR
from band_restate import same, same_bits
from weighted_helpers import AXIS_DIRECTIONS, PARAMS, image, steps_from_edges

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 7), (7, 5)]
GROUPING = [1, 2, 3, 5, 17, 60, 64, 65, 100, 129, 200, 256]
DIRECTION_LISTS = [[d] for d in R.DIRECTIONS_8] + [list(R.DIRECTIONS_8)]


def flat(a):
    import torch
    return torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()


def case(D, shape, R_, seed, dyadic):
    """(unary D x N, positions D, wstep R x N)"""
    H, W = shape
    rng = np.random.default_rng([D, H, W, R_, seed, int(dyadic)])
    if dyadic:
        unary = rng.integers(0, 4 << 6, size=(D, H * W)).astype(np.float64) / 64.0
        positions = rng.integers(0, 4 * D + 4, size=D).astype(np.float64) * 0.25
        wstep = rng.choice(fp.ALPHAS, size=(R_, H * W))
    else:
        unary = rng.standard_normal((D, H * W)) * 3.0
        positions = rng.standard_normal(D) * (1.0 + D / 8.0)
        wstep = rng.uniform(0.0, 2.0, size=(R_, H * W))
    return np.asfortranarray(unary), positions, wstep


def check_device(unary, shape, positions, kernel, tol, wstep, directions):
    import torch
    from stereo_amd import scanline
    S, labels, dmap, conf = WR.aggregate(unary, shape, positions, kernel, tol, wstep, directions)
    assert np.isfinite(S).all()
    d_unary, d_wstep = flat(unary), torch.from_numpy(np.ascontiguousarray(wstep).reshape(-1)).cuda()
    dev = scanline.aggregate_weighted_device(d_unary, shape, positions, kernel, tol, d_wstep, directions)
    torch.cuda.synchronize()
    what = (shape, len(positions), kernel, tol, directions)
    assert np.array_equal(dev.volume.cpu().numpy().reshape(S.shape, order="F"), S), what
    assert dev.labels.dtype == torch.int32 and np.array_equal(dev.labels.cpu().numpy(), labels), what
    assert np.array_equal(dev.dispmap.cpu().numpy().T, dmap) and np.array_equal(dev.confidence.cpu().numpy().T, conf), what
    assert np.array_equal(d_unary.cpu().numpy(), unary.reshape(-1, order="F"))               # the inputs are only read
    assert np.array_equal(d_wstep.cpu().numpy(), np.ascontiguousarray(wstep).reshape(-1))
    return S


def check_host(unary, shape, positions, kernel, tol, wstep, directions):
    from stereo_amd import scanline
    S, labels, dmap, conf = WR.aggregate(unary, shape, positions, kernel, tol, wstep, directions)
    got = scanline.aggregate_weighted(unary, shape, positions, kernel, tol, wstep, directions, want_volume=True)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels) and np.array_equal(got.volume, S)
    assert np.array_equal(got.dispmap, dmap) and np.array_equal(got.confidence, conf)
    assert scanline.aggregate_weighted(unary, shape, positions, kernel, tol, wstep, directions).volume is None


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("D", GROUPING)
def test_device_equals_the_restatement(D, kernel, hip):
    tol = 2.0 if kernel == 1 else 6.0
    for shape in GEOMETRY:
        for dyadic in (True, False):
            for directions in DIRECTION_LISTS:
                unary, positions, wstep = case(D, shape, len(directions), kernel, dyadic)
                check_device(unary, shape, positions, kernel, tol, wstep, directions)


@pytest.mark.parametrize("D", [1, 3, 64, 65])
def test_host_entry_equals_the_restatement(D, hip):
    for shape in ((1, 1), (5, 7)):
        for kernel, dyadic in ((1, True), (2, False)):
            unary, positions, wstep = case(D, shape, 8, 40 + kernel, dyadic)
            check_host(unary, shape, positions, kernel, 1.5, wstep, R.DIRECTIONS_8)
    unary, positions, wstep = case(D, (5, 7), 3, 50, True)
    check_host(unary, (5, 7), positions, 1, 1.5, wstep, [(1, 1), (0, -1), (1, 1)])           # a duplicate


@pytest.mark.parametrize("D", [3, 60, 65])
def test_zero_step_weights_keep_S_finite(D, hip):
    """0.0 * Inf in a padded column would be a NaN (D = 3 in a group of 4, 60 in one of 64); 65: the wide kernel."""
    for kernel in (1, 2):
        unary, positions, wstep = case(D, (5, 7), 8, 60 + kernel, False)
        wstep[:, np.arange(35) % 3 == kernel] = 0.0
        S = check_device(unary, (5, 7), positions, kernel, 1.25, wstep, R.DIRECTIONS_8)
        assert np.isfinite(S).all()
        check_host(unary, (5, 7), positions, kernel, 1.25, wstep, R.DIRECTIONS_8)
    unary, positions, wstep = case(D, (5, 7), 4, 63, True)
    S = check_device(unary, (5, 7), positions, 1, 2.0, np.zeros_like(wstep), R.DIRECTIONS_4)
    assert np.isfinite(S).all()


@pytest.mark.parametrize("shape,D", [((3, 200), 3), ((40, 33), 60)], ids=["3x200x3", "40x33x60"])
def test_more_chains_than_one_workgroup(shape, D, hip):
    unary, positions, wstep = case(D, shape, 8, 70, False)
    check_device(unary, shape, positions, 1, 2.0, wstep, R.DIRECTIONS_8)


# ---------------------------------------------------------------- agreement with the existing entries

@pytest.mark.parametrize("D", [3, 60, 64, 65, 200])
def test_constant_step_weights_give_the_unweighted_entrys_bits(D, hip):
    import torch
    from stereo_amd import scanline
    shape, weights = (7, 5), [0.3, 0.7, 1.1, 0.0, 0.1, 1.3, 0.6, 1.7]
    for kernel in (1, 2):
        unary, positions, _ = case(D, shape, 8, 80 + kernel, False)
        d_unary = flat(unary)
        want = scanline.aggregate_device(d_unary, shape, positions, kernel, 0.7, R.DIRECTIONS_8, weights)
        wstep = torch.from_numpy(np.repeat(np.array(weights), 35)).cuda()
        got = scanline.aggregate_weighted_device(d_unary, shape, positions, kernel, 0.7, wstep, R.DIRECTIONS_8)
        torch.cuda.synchronize()
        for a, b in ((want.volume, got.volume), (want.labels, got.labels), (want.dispmap, got.dispmap), (want.confidence, got.confidence)):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("K", [9, 64])
def test_axis_directions_equal_the_per_edge_entry(K, hip):
    import torch
    from stereo_amd import scanline
    H, W = 5, 7
    p = fp.dyadic_problem(np.random.default_rng(K), H, W, K, shared=True)
    rng = np.random.default_rng([K, 1])
    conn = np.ascontiguousarray(p["conn"].T)
    alphas, unary = rng.uniform(0.0, 2.0, size=conn.shape[1]), np.asfortranarray(rng.standard_normal((K, H * W)) * 3.0)
    positions = p["positions"] + rng.random(K) * 0.125
    q = np.asfortranarray(np.tile(positions[:, None], (1, conn.shape[1])))
    d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
    table, _ = scanline.edge_table_device(d_conn, conn.shape[1], (H, W))
    for kernel in (1, 2):
        want = scanline.aggregate_edges_device(flat(unary), (H, W), table, flat(q), flat(q), torch.from_numpy(alphas).cuda(), kernel, 1.75)
        wstep = torch.from_numpy(steps_from_edges(conn, alphas, (H, W)).reshape(-1)).cuda()
        got = scanline.aggregate_weighted_device(flat(unary), (H, W), positions, kernel, 1.75, wstep, AXIS_DIRECTIONS)
        torch.cuda.synchronize()
        assert np.array_equal(want.volume.cpu().numpy(), got.volume.cpu().numpy())
        assert np.array_equal(want.labels.cpu().numpy(), got.labels.cpu().numpy())
        assert np.array_equal(want.confidence.cpu().numpy(), got.confidence.cpu().numpy())


@functools.lru_cache(maxsize=None)
def teddy():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_crop.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    assert im0.shape == (64, 96, 3)
    return im0, im1


def test_teddy_crop_with_the_images_own_step_weights(hip):
    from stereo_amd import Contrast, contrast, terms as T
    im0, im1 = teddy()
    disparities = np.arange(24, dtype=np.float64)
    unary = np.asfortranarray(40.0 * (1.0 - T.ncc_volume(im0, im1, disparities, 2, layout=1)))
    par = (2.0, 0.25, 4.0, 40.0)
    wstep = contrast.step_weights(im0, R.DIRECTIONS_8, Contrast(*par))
    assert np.array_equal(wstep, CR.step_weights(im0, R.DIRECTIONS_8, par))
    assert len(np.unique(wstep)) > 20                                       # the ramp is exercised, not only its ends
    check_device(unary, (64, 96), disparities, 1, 2.0, wstep, R.DIRECTIONS_8)


# ---------------------------------------------------------------- the two builders

@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("channels", [1, 3])
def test_builders_equal_the_restatement(channels, name, hip):
    import torch
    from stereo_amd import Contrast, contrast
    par, c = PARAMS[name], Contrast(*PARAMS[name])
    for shape, dyadic in (((1, 1), True), ((1, 7), False), ((7, 1), True), ((5, 7), True), ((5, 7), False), ((33, 40), False)):
        H, W = shape
        rng = np.random.default_rng([H, W, channels])
        im = image(rng, H, W, channels, dyadic)
        conn = np.ascontiguousarray(fp.grid_edges(H, W).T)
        if conn.shape[1]:                                                    # any graph on the pixels: also far pairs
            far = rng.integers(0, H * W, size=(2, 9))
            conn = np.concatenate([conn[:, rng.permutation(conn.shape[1])], far], axis=1)
        want_e, want_s = CR.edge_weights(im, conn, par), CR.step_weights(im, R.DIRECTIONS_8, par)
        assert np.array_equal(contrast.step_weights(im, R.DIRECTIONS_8, c), want_s)
        d_im = contrast.image_to_device(im)
        got_s = contrast.step_weights_device(d_im, im.shape, R.DIRECTIONS_8, c)
        assert np.array_equal(got_s.cpu().numpy().reshape(8, H * W), want_s)
        one = contrast.step_weights_device(d_im, im.shape, [(-1, 1)], c)
        assert np.array_equal(one.cpu().numpy(), want_s[7])
        if conn.shape[1]:
            assert np.array_equal(contrast.edge_weights(im, conn, c), want_e)
            d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.int32).reshape(-1, order="F").copy()).cuda()
            got_e, bad = contrast.edge_weights_device(d_im, im.shape, d_conn, c)
            assert np.array_equal(got_e.cpu().numpy(), want_e) and int(bad.item()) == 0
        assert np.array_equal(d_im.cpu().numpy(), np.asfortranarray(im).reshape(-1, order="F"))


def test_builders_on_a_side_stream_into_given_tensors_and_bad_edges(hip):
    import torch
    from stereo_amd import Contrast, StereoHipError, contrast
    H, W, par = 5, 7, PARAMS["ramp"]
    c = Contrast(*par)
    im = image(np.random.default_rng(9), H, W, 3, False)
    conn = np.ascontiguousarray(fp.grid_edges(H, W).T)
    d_im = contrast.image_to_device(im)
    d_conn = torch.from_numpy(np.asfortranarray(conn, dtype=np.int32).reshape(-1, order="F").copy()).cuda()
    alphas = torch.empty(conn.shape[1], dtype=torch.float64, device="cuda")
    wstep = torch.empty(4 * H * W, dtype=torch.float64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a, b = contrast.edge_weights_device(d_im, im.shape, d_conn, c, alphas=alphas, bad=bad, stream=side, check=False)
    s = contrast.step_weights_device(d_im, im.shape, AXIS_DIRECTIONS, c, wstep=wstep, stream=side)
    side.synchronize()
    assert a is alphas and b is bad and s is wstep and int(bad.item()) == 0
    assert np.array_equal(alphas.cpu().numpy(), CR.edge_weights(im, conn, par))
    assert np.array_equal(wstep.cpu().numpy().reshape(4, H * W), CR.step_weights(im, AXIS_DIRECTIONS, par))
    # `bad` counts the edges with an endpoint outside the image; they weigh 0.0 and the others are untouched
    broken = conn.copy()
    broken[1, 3], broken[0, 10] = H * W, H * W + 5
    d_broken = torch.from_numpy(np.asfortranarray(broken, dtype=np.int32).reshape(-1, order="F").copy()).cuda()
    got, bad = contrast.edge_weights_device(d_im, im.shape, d_broken, c, check=False)
    want = CR.edge_weights(im, conn, par)
    want[[3, 10]] = 0.0
    assert int(bad.item()) == 2 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(StereoHipError, match="2 edge\\(s\\) with an endpoint outside"):
        contrast.edge_weights_device(d_im, im.shape, d_broken, c)
    with pytest.raises(StereoHipError, match="edge 3 .* has an endpoint outside"):
        contrast.edge_weights(im, broken, c)


# ---------------------------------------------------------------- end to end (the synthetic pair of test_scanline_gpu)

PH, PW, PK = 24, 32, 8
WEIGHT, TOL, CHECK_TOL, ITERS, NEVER = 40.0, 2.0, 1.0, 4, -1e300
CANDIDATES = [dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base", "wta"])]          # K = 9
BANDS = [[-0.5, -0.25, 0.0, 0.25, 0.5]]                                                                         # K = 5
CONTRAST = (1.5, 0.25, 20.0, 120.0)         # in the images' 0 .. 255 units; the random texture spreads over the ramp


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    """test_scanline_gpu.synthetic_pair's data: a two-plane scene with a random texture, 24 x 32 x 3: background d = 2, a
    box with d = 5 on rows 4-19 at left columns 14-23 = right columns 9-18."""
    rng = np.random.default_rng(31)
    back = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    left, right = back[:, :PW].copy(), back[:, 2:PW + 2].copy()
    left[4:20, 14:24] = box[4:20, 14:24]
    right[4:20, 9:19] = box[4:20, 14:24]
    return left, right


def check_and_fill(hip, maps):
    out = []
    for i, direction in ((0, 1), (1, -1)):
        status, residual = hip.lr_check(maps[i], maps[1 - i], direction, CHECK_TOL)
        out.append((status, residual) + tuple(hip.lr_fill(maps[i], status)))
    return out


def assert_checked(view, ref):
    status, residual, filled, source = ref
    assert np.array_equal(view.status, status) and same(view.residual, residual)
    assert same(view.filled, filled) and np.array_equal(view.source, source)


def first_pass_by_hand(hip, kernel):
    """builders -> weighted aggregate per view -> (volumes, unaries, conn, alphas per view, ScanlineResult per view)"""
    from stereo_amd import Contrast, consistency, contrast, scanline, terms as T
    c = Contrast(*CONTRAST)
    disparities = np.arange(PK, dtype=np.float64)
    volumes = consistency.pair_volumes(synthetic_pair(), disparities)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT, volumes)
    conn = T.construct_neighborhood(PH, PW)
    alphas = [contrast.edge_weights(im, conn, c) for im in synthetic_pair()]
    assert all(np.array_equal(a, CR.edge_weights(im, conn, CONTRAST)) for a, im in zip(alphas, synthetic_pair()))
    assert len(np.unique(alphas[0])) > 50 and not np.array_equal(alphas[0], alphas[1])
    first = [scanline.aggregate_weighted(u, (PH, PW), disparities, kernel, TOL, contrast.step_weights(im, scanline.DIRECTIONS_8, c))
             for u, im in zip(unaries, synthetic_pair())]
    return disparities, volumes, unaries, conn, alphas, first


@pytest.mark.parametrize("kernel", [1, 2])
def test_solve_pair_scanline_contrast_without_levels(kernel, hip):
    from stereo_amd import Contrast, StereoHipError, scanline
    disparities, volumes, unaries, conn, alphas, want = first_pass_by_hand(hip, kernel)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL,
                                      contrast=Contrast(*CONTRAST))
    for view, ref, checked, u, a in zip(got.views, want, check_and_fill(hip, [w.dispmap for w in want]), unaries, alphas):
        assert np.array_equal(view.labels, ref.labels) and same_bits(view.dispmap, ref.dispmap)
        assert view.energy == [scanline.model_energy(u, conn, a, disparities, kernel, TOL, ref.labels)]
        assert np.isnan(view.lower_bound[0]) and view.iterations == [0] and view.paths == [0] and len(view.maps) == 1
        assert_checked(view, checked)
    with pytest.raises(StereoHipError, match="smooth_weight or contrast, not both"):
        hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, smooth_weight=1.0, contrast=Contrast(*CONTRAST))


@pytest.mark.parametrize("level_solver", ["trws", "scanline"])
def test_solve_pair_scanline_contrast_with_levels_equals_the_pipeline_by_hand(level_solver, hip):
    from stereo_amd import Contrast, band, candidates, scanline
    from stereo_amd.trws import TrwsBatch, TrwsPlan
    kernel = 1
    disparities, volumes, unaries, conn, alphas, first = first_pass_by_hand(hip, kernel)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL,
                                      candidate_levels=CANDIDATES, band_levels=BANDS, maxiter=ITERS, max_relgap=NEVER,
                                      level_solver=level_solver, contrast=Contrast(*CONTRAST))
    maps = [[r.dispmap] for r in first]
    energy = [[scanline.model_energy(u, conn, a, disparities, kernel, TOL, r.labels)] for u, a, r in zip(unaries, alphas, first)]
    bound, iters, labels = [[], []], [[], []], [None, None]

    def level(problems, what, K):
        if level_solver == "scanline":
            solved = [scanline.solve_level(prob, what, kernel, TOL) for prob in problems]
        else:
            solved = [TrwsPlan(kernel, K, PH * PW, conn) for _ in range(2)]
            for prob, plan in zip(problems, solved):
                prob.build(what, plan, TOL)
            with TrwsBatch(solved) as batch:
                batch.iterate(ITERS, NEVER)
        for i, (prob, plan) in enumerate(zip(problems, solved)):
            labels[i], en, lb, it = plan.result()
            energy[i].append(en); bound[i].append(lb); iters[i].append(it)
            maps[i].append(prob.apply(labels[i]))
            if level_solver == "trws":
                plan.close()

    cand = candidates.check_levels(CANDIDATES)[0]
    level([candidates.CandidateProblem(v, disparities, WEIGHT, m[-1], conn, a, layout=1) for v, m, a in zip(volumes, maps, alphas)], cand, 9)
    level([band.BandProblem(v, disparities, WEIGHT, m[-1], conn, a, layout=1) for v, m, a in zip(volumes, maps, alphas)],
          np.asarray(BANDS[0]), 5)
    for i, (view, checked) in enumerate(zip(got.views, check_and_fill(hip, [m[-1] for m in maps]))):
        assert view.energy == energy[i] and same(np.array(view.lower_bound[1:]), np.array(bound[i])) and np.isnan(view.lower_bound[0])
        assert view.iterations == [0] + iters[i]
        assert len(view.maps) == 3 and all(same_bits(a, b) for a, b in zip(view.maps, maps[i])) and view.dispmap is view.maps[-1]
        assert np.array_equal(view.labels, labels[i])
        assert_checked(view, checked)


def test_solve_pair_ncc_contrast_equals_plans_uploaded_by_hand(hip):
    from stereo_amd import Contrast, StereoHipError, consistency, contrast, terms as T
    from stereo_amd.trws import TrwsBatch, TrwsPlan
    kernel, disparities = 1, np.arange(PK, dtype=np.float64)
    c = Contrast(*CONTRAST)
    got = hip.solve_pair_ncc(synthetic_pair(), disparities, kernel, WEIGHT, TOL, ITERS, NEVER, check_tol=CHECK_TOL, contrast=c)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT)
    conn = T.construct_neighborhood(PH, PW)
    plans = [TrwsPlan(kernel, PK, PH * PW, conn) for _ in range(2)]
    try:
        for plan, u, im in zip(plans, unaries, synthetic_pair()):
            plan.upload(u, contrast.edge_weights(im, conn, c), TOL, positions=disparities)
        with TrwsBatch(plans) as batch:
            batch.iterate(ITERS, NEVER)
        for view, plan in zip(got.views, plans):
            labels, en, lb, it = plan.result()
            assert np.array_equal(view.labels, labels) and view.energy == [en] and view.lower_bound == [lb] and view.iterations == [it]
    finally:
        for plan in plans:
            plan.close()
    with pytest.raises(StereoHipError, match="smooth_weight or contrast, not both"):
        hip.solve_pair_ncc(synthetic_pair(), disparities, kernel, WEIGHT, TOL, ITERS, NEVER, smooth_weight=0.5, contrast=c)


def test_dispmap_ncc_set_contrast_plain_and_mirrored(hip):
    from stereo_amd import Contrast, contrast, scanline
    im0, im1 = teddy()
    images = [im0[:24, :32], im1[:24, :32]]
    c = Contrast(2.0, 0.25, 4.0, 40.0)
    dm = hip.dispmap_ncc(images, np.arange(8.0), 1, 40.0, 2.0)
    mirror = dm.mirrored()
    for obj, reference, own in ((dm, images[0], images[0]), (mirror, images[1][:, ::-1], images[1])):
        assert np.array_equal(obj.smooth_weights, np.ones(obj.neighborhood.shape[1]))
        obj.set_contrast(c)
        assert np.array_equal(obj.smooth_weights, contrast.edge_weights(reference, obj.neighborhood, c))
        assert len(np.unique(obj.smooth_weights)) > 10
        vol = obj.unary_volume()
        unary = np.asfortranarray(vol.transpose(2, 1, 0).reshape(8, 32 * 24))
        got = obj.aggregate_scanlines(contrast=c)
        want = scanline.aggregate_weighted(unary, (24, 32), obj.disparities, 1, 2.0, contrast.step_weights(own, scanline.DIRECTIONS_8, c),
                                           want_volume=True)
        assert np.array_equal(got.volume, want.volume) and np.array_equal(got.labels, want.labels)
        assert np.array_equal(got.dispmap, want.dispmap) and np.array_equal(got.confidence, want.confidence)
    assert not np.array_equal(dm.smooth_weights, mirror.smooth_weights)


def test_without_contrast_the_results_are_the_unweighted_ones(hip):
    from stereo_amd import consistency, scanline, terms as T
    from stereo_amd.trws import TrwsBatch, TrwsPlan
    kernel, disparities = 2, np.arange(PK, dtype=np.float64)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT)
    conn = T.construct_neighborhood(PH, PW)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL, contrast=None)
    same_call = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL, smooth_weight=1.0)
    for view, other, u in zip(got.views, same_call.views, unaries):
        ref = scanline.aggregate(u, (PH, PW), disparities, kernel, TOL)
        assert np.array_equal(view.labels, ref.labels) and same_bits(view.dispmap, ref.dispmap)
        assert view.energy == [scanline.model_energy(u, conn, 1.0, disparities, kernel, TOL, ref.labels)] == other.energy
        assert np.array_equal(view.labels, other.labels)
    got = hip.solve_pair_ncc(synthetic_pair(), disparities, kernel, WEIGHT, TOL, ITERS, NEVER, check_tol=CHECK_TOL, contrast=None)
    plans = [TrwsPlan(kernel, PK, PH * PW, conn) for _ in range(2)]
    try:
        for plan, u in zip(plans, unaries):
            plan.upload(u, np.ones(conn.shape[1]), TOL, positions=disparities)
        with TrwsBatch(plans) as batch:
            batch.iterate(ITERS, NEVER)
        for view, plan in zip(got.views, plans):
            labels, en, lb, it = plan.result()
            assert np.array_equal(view.labels, labels) and view.energy == [en] and view.lower_bound == [lb] and view.iterations == [it]
    finally:
        for plan in plans:
            plan.close()
    dm = hip.dispmap_ncc([teddy()[0][:24, :32], teddy()[1][:24, :32]], np.arange(8.0), 1, 40.0, 2.0)
    a, b = dm.aggregate_scanlines(), dm.aggregate_scanlines(contrast=None)
    assert np.array_equal(a.volume, b.volume) and np.array_equal(a.labels, b.labels)
