"""Scanline aggregation on the device: stereo_scanline_aggregate and its device form against the NumPy
restatement (tests/scanline_restate.py, which test_scanline_cpu holds against first principles), bit for bit on S,
labels, map and confidence -- a minimum of finite doubles does not depend on its order and every other operation is one
rounded add or product, so there is no tolerance to choose; and solve_pair_ncc_scanline against its pieces.

The shapes are the smallest at which the chain geometry (one pixel, one row, one column, a square of 2, both
orientations of a rectangle whose sides differ), the lane grouping (D around every power of two's group and around 64 .. 256)
and the chain count (more chains than one wave carries, more waves than one) can each go wrong."""
import functools
import os

import numpy as np
import pytest

import scanline_restate as R
from band_restate import same, same_bits

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 1), (1, 6), (6, 1), (2, 2), (5, 7), (7, 5)]
GROUPING = [1, 2, 63, 64, 65, 128, 129, 256]
MIXED = ([(1, 1), (0, -1), (1, 1), (-1, 0), (1, -1)], [0.5, 2.0, 1.25, 0.0, 3.0])     # a duplicate, unequal weights, a 0
DIRECTION_LISTS = [([d], None) for d in R.DIRECTIONS_8] + [(list(R.DIRECTIONS_4), None), (list(R.DIRECTIONS_8), None), MIXED]


def volume(D, N, seed, dyadic=True):
    rng = np.random.default_rng(seed)
    if dyadic:
        return np.asfortranarray(rng.integers(0, 4 << 6, size=(D, N)).astype(np.float64) / 64.0)
    return np.asfortranarray(rng.standard_normal((D, N)) * 3.0)


def check(hip, unary, shape, positions, kernel, tol, directions, weights=None):
    """Host entry and device entry against the restatement."""
    import torch
    from stereo_amd import scanline
    H, W = shape
    positions = np.asarray(positions, dtype=np.float64)
    S, labels, dmap, conf = R.aggregate(unary, shape, positions, kernel, tol, directions, weights)
    assert np.isfinite(S).all()
    got = scanline.aggregate(unary, shape, positions, kernel, tol, directions, weights, want_volume=True)
    what = (shape, positions.shape[0], kernel, tol, directions, weights)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels), what
    assert np.array_equal(got.volume, S), what
    assert np.array_equal(got.dispmap, dmap) and np.array_equal(got.confidence, conf), what
    assert scanline.aggregate(unary, shape, positions, kernel, tol, directions, weights).volume is None
    d_unary = torch.from_numpy(np.asfortranarray(unary).reshape(-1, order="F").copy()).cuda()
    dev = scanline.aggregate_device(d_unary, shape, positions, kernel, tol, directions, weights)
    torch.cuda.synchronize()
    assert np.array_equal(dev.volume.cpu().numpy().reshape(S.shape, order="F"), S), what
    assert dev.labels.dtype == torch.int32 and np.array_equal(dev.labels.cpu().numpy(), labels), what
    assert np.array_equal(dev.dispmap.cpu().numpy().T, dmap) and np.array_equal(dev.confidence.cpu().numpy().T, conf), what
    assert np.array_equal(d_unary.cpu().numpy(), np.asfortranarray(unary).reshape(-1, order="F"))     # the input is only read
    return got


@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_chain_geometry(shape, hip):
    H, W = shape
    unary = volume(3, H * W, [H, W])
    for directions, weights in DIRECTION_LISTS:
        check(hip, unary, shape, [0.0, 1.0, 2.5], 1, 1.5, directions, weights)


@pytest.mark.parametrize("D", GROUPING)
def test_lane_grouping(D, hip):
    rng = np.random.default_rng(D)
    positions = rng.integers(0, 4 * D + 4, size=D).astype(np.float64) * 0.25
    check(hip, volume(D, 12, [D, 1]), (3, 4), positions, 2, 6.0, R.DIRECTIONS_8)
    check(hip, volume(D, 12, [D, 2]), (3, 4), np.sort(positions), 1, 2.0, R.DIRECTIONS_4, [1.0, 0.5, 2.0, 0.25])


def test_more_chains_than_one_workgroup(hip):
    check(hip, volume(60, 37 * 29, 7), (37, 29), np.arange(60.0), 1, 2.0, R.DIRECTIONS_8)


@pytest.mark.parametrize("kernel", [1, 2])
def test_truncation_weights_and_positions(kernel, hip):
    shape, D = (5, 7), 6
    unary = volume(D, 35, [kernel, 3])
    ascending = np.arange(D, dtype=np.float64)
    for tol in (0.0, 1e9, 2.0):                                         # cuts everything, never cuts, cuts inside the range
        check(hip, unary, shape, ascending, kernel, tol, R.DIRECTIONS_8)
    check(hip, unary, shape, ascending, kernel, 2.0, R.DIRECTIONS_4, [0.0, 0.0, 0.0, 0.0])        # S = 4 U
    check(hip, unary, shape, ascending, kernel, 2.0, R.DIRECTIONS_4, [0.0, 1.0, 0.0, 2.0])
    check(hip, unary, shape, [3.0, 0.5, 3.0, -1.25, 7.0, 0.5], kernel, 3.0, R.DIRECTIONS_8)     # not ascending, repeated values


@functools.lru_cache(maxsize=None)
def teddy_unary():
    from stereo_amd import terms as T
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_crop.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    H, W = im0.shape[:2]
    disparities = np.arange(24, dtype=np.float64)
    ncc = T.ncc_volume(im0, im1, disparities, 2, layout=1)
    assert H >= 40 and W >= 48 and disparities.shape[0] <= 256
    crop = ncc.reshape(24, W, H)[:, :48, :40].reshape(24, 48 * 40)
    unary = np.asfortranarray(40.0 * (1.0 - crop))
    unary.setflags(write=False)
    return unary, disparities


@pytest.mark.parametrize("kernel", [1, 2])
def test_data_that_is_not_dyadic(kernel, hip):
    """The bitwise claim does not rest on exact sums."""
    check(hip, volume(17, 9 * 11, [kernel, 5], dyadic=False), (9, 11), np.linspace(-1.0, 2.3, 17), kernel, 0.7, R.DIRECTIONS_8,
          [0.3, 0.7, 1.1, 0.9, 0.1, 1.3, 0.6, 1.7])
    unary, disparities = teddy_unary()
    assert np.isfinite(unary).all()
    check(hip, unary, (40, 48), disparities, kernel, 2.0 if kernel == 1 else 5.0, R.DIRECTIONS_8)


def test_ties_give_the_first_label_and_confidence_zero(hip):
    got = check(hip, np.full((5, 35), 2.5, order="F"), (5, 7), np.arange(5.0), 1, 2.0, R.DIRECTIONS_8)
    assert (got.labels == 1).all() and (got.confidence == 0.0).all() and (got.dispmap == 0.0).all()
    got = check(hip, np.full((1, 35), 2.5, order="F"), (5, 7), [4.0], 2, 2.0, R.DIRECTIONS_4)
    assert (got.labels == 1).all() and np.isposinf(got.confidence).all() and (got.dispmap == 4.0).all()


def test_device_form_on_a_side_stream_into_given_tensors(hip):
    import torch
    from stereo_amd import StereoHipError, scanline
    H, W, D = 7, 5, 9
    unary, positions = volume(D, H * W, 21), np.arange(D, dtype=np.float64)
    S, labels, dmap, conf = R.aggregate(unary, (H, W), positions, 2, 4.0, R.DIRECTIONS_8)
    d_unary = torch.from_numpy(unary.reshape(-1, order="F").copy()).cuda()
    d_positions = torch.from_numpy(positions).cuda()
    out = dict(volume=torch.empty(D * H * W, dtype=torch.float64, device="cuda"), labels=torch.empty(H * W, dtype=torch.int32, device="cuda"),
               dispmap=torch.empty((W, H), dtype=torch.float64, device="cuda"), confidence=torch.empty((W, H), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    r = scanline.aggregate_device(d_unary, (H, W), positions, 2, 4.0, R.DIRECTIONS_8, stream=side, d_positions=d_positions, **out)
    side.synchronize()
    assert r.volume is out["volume"] and r.labels is out["labels"] and r.dispmap is out["dispmap"]
    assert np.array_equal(r.volume.cpu().numpy().reshape(S.shape, order="F"), S) and np.array_equal(r.labels.cpu().numpy(), labels)
    assert np.array_equal(r.dispmap.cpu().numpy().T, dmap) and np.array_equal(r.confidence.cpu().numpy().T, conf)
    with pytest.raises(StereoHipError, match="unary must hold"):
        scanline.aggregate_device(d_unary[:-1].contiguous(), (H, W), positions, 2, 4.0)
    with pytest.raises(StereoHipError, match="dispmap must"):
        scanline.aggregate_device(d_unary, (H, W), positions, 2, 4.0, dispmap=torch.empty((H, W), dtype=torch.float64, device="cuda"))
    with pytest.raises(StereoHipError, match="a direction must be"):
        scanline.aggregate_device(d_unary, (H, W), positions, 2, 4.0, [(1, 2)])


def test_dispmap_ncc_aggregate_scanlines_plain_and_mirrored(hip):
    from stereo_amd import scanline
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_crop.npz"))
    images = [g["im0"][:24, :32].astype(np.float64), g["im1"][:24, :32].astype(np.float64)]
    dm = hip.dispmap_ncc(images, np.arange(8.0), 1, 40.0, 2.0)
    for obj in (dm, dm.mirrored()):
        before = obj.assignment.copy()
        vol = obj.unary_volume()
        unary = np.asfortranarray(vol.transpose(2, 1, 0).reshape(8, 32 * 24))
        got = obj.aggregate_scanlines(directions=scanline.DIRECTIONS_4, weights=[1.0, 1.0, 0.5, 0.5])
        want = scanline.aggregate(unary, (24, 32), obj.disparities, 1, 2.0, scanline.DIRECTIONS_4, [1.0, 1.0, 0.5, 0.5], want_volume=True)
        assert np.array_equal(got.volume, want.volume) and np.array_equal(got.labels, want.labels)
        assert np.array_equal(got.dispmap, want.dispmap) and np.array_equal(got.confidence, want.confidence)
        assert np.array_equal(obj.aggregate_scanlines().labels, scanline.aggregate(unary, (24, 32), obj.disparities, 1, 2.0).labels)
        assert np.array_equal(obj.assignment, before)                   # nothing is stored in the object


# ---------------------------------------------------------------- solve_pair_ncc_scanline

PH, PW, PK = 24, 32, 8
WEIGHT, TOL, CHECK_TOL, ITERS, NEVER = 40.0, 2.0, 1.0, 4, -1e300
CANDIDATES = [dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base", "wta"])]          # K = 1 + 2 * 4 = 9
BANDS = [[-0.5, -0.25, 0.0, 0.25, 0.5]]                                                                         # K = 5


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    """A two-plane scene with a random texture, 24 x 32 x 3: background d = 2, a box with d = 5 on rows 4-19 at left
    columns 14-23 = right columns 9-18."""
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


@pytest.mark.parametrize("kernel", [1, 2])
def test_solve_pair_without_levels_is_aggregate_check_and_fill(kernel, hip):
    from stereo_amd import consistency, scanline, terms as T
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL, smooth_weight=0.5)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT)
    conn = T.construct_neighborhood(PH, PW)
    want = [scanline.aggregate(u, (PH, PW), disparities, kernel, TOL, scanline.DIRECTIONS_8, [0.5] * 8) for u in unaries]
    for view, ref, checked, u in zip(got.views, want, check_and_fill(hip, [w.dispmap for w in want]), unaries):
        assert np.array_equal(view.labels, ref.labels) and same_bits(view.dispmap, ref.dispmap) and view.maps[0] is view.dispmap
        assert view.energy == [scanline.model_energy(u, conn, 0.5, disparities, kernel, TOL, ref.labels)]
        assert len(view.lower_bound) == 1 and np.isnan(view.lower_bound[0])
        assert view.iterations == [0] and view.paths == [0] and view.carried == [False] and len(view.maps) == 1
        assert_checked(view, checked)
    assert {"volumes", "scanline", "check_fill"} <= set(got.times)


@pytest.mark.parametrize("kernel", [1, 2])
def test_solve_pair_with_levels_equals_the_pipeline_by_hand(kernel, hip):
    from stereo_amd import band, candidates, consistency, scanline, terms as T
    from stereo_amd.trws import TrwsBatch, TrwsPlan
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL,
                                      candidate_levels=CANDIDATES, band_levels=BANDS, maxiter=ITERS, max_relgap=NEVER)
    volumes = consistency.pair_volumes(synthetic_pair(), disparities)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT, volumes)
    conn = T.construct_neighborhood(PH, PW)
    alphas = np.ones(conn.shape[1])
    first = [scanline.aggregate(u, (PH, PW), disparities, kernel, TOL) for u in unaries]
    maps = [[r.dispmap] for r in first]
    energy = [[scanline.model_energy(u, conn, alphas, disparities, kernel, TOL, r.labels)] for u, r in zip(unaries, first)]
    bound, iters, labels = [[], []], [[], []], [None, None]

    def level(problems, what, K):
        plans = [TrwsPlan(kernel, K, PH * PW, conn) for _ in range(2)]
        for prob, plan in zip(problems, plans):
            prob.build(what, plan, TOL)
        with TrwsBatch(plans) as batch:
            batch.iterate(ITERS, NEVER)
        for i, (prob, plan) in enumerate(zip(problems, plans)):
            assert plan.path() == 2
            labels[i], en, lb, it = plan.result()
            energy[i].append(en); bound[i].append(lb); iters[i].append(it)
            maps[i].append(prob.apply(labels[i]))
            plan.close()

    cand = candidates.check_levels(CANDIDATES)[0]
    assert candidates.labels_of(cand) == 9
    level([candidates.CandidateProblem(v, disparities, WEIGHT, m[-1], conn, alphas, layout=1) for v, m in zip(volumes, maps)], cand, 9)
    level([band.BandProblem(v, disparities, WEIGHT, m[-1], conn, alphas, layout=1) for v, m in zip(volumes, maps)],
          np.asarray(BANDS[0]), 5)
    for i, (view, checked) in enumerate(zip(got.views, check_and_fill(hip, [m[-1] for m in maps]))):
        assert view.energy == energy[i] and view.lower_bound[1:] == bound[i] and np.isnan(view.lower_bound[0])
        assert view.iterations == [0] + iters[i] and view.paths == [0, 2, 2] and view.carried == [False] * 3
        assert len(view.maps) == 3 and all(same_bits(a, b) for a, b in zip(view.maps, maps[i])) and view.dispmap is view.maps[-1]
        assert np.array_equal(view.labels, labels[i])
        assert_checked(view, checked)
    assert {"propagate_1", "propagate_1_check_fill", "band_1", "band_1_check_fill"} <= set(got.times)
