"""Levels solved by scanline aggregation: refine_band, refine_plane_band, refine_candidates and
refine_plane_candidates with solver="scanline" against the pipeline put together by hand -- build(plan=None),
aggregate_edges_device, apply, level by level -- bit for bit; the bookkeeping of such a level; the default and
solver="trws" against a run that does not pass the keyword; solve_pair_ncc_scanline(level_solver="scanline") against its
pieces; and the dispmap methods, which pass the keyword through."""
import functools

import numpy as np
import pytest

import plane_band_restate as PR
from band_restate import same, same_bits

pytestmark = pytest.mark.gpu

PH, PW, PK = 24, 32, 8
WEIGHT, TOL, CHECK_TOL, ITERS, NEVER = 40.0, 2.0, 1.0, 4, -1e300
CANDIDATES = [dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base", "wta"])]          # K = 1 + 2 * 4 = 9
BANDS = [[-0.5, -0.25, 0.0, 0.25, 0.5]]                                                                         # K = 5
TWO_BANDS = [np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), np.array([-0.25, 0.0, 0.25])]                               # K = 5, then 3
PLANE_CANDIDATES = [dict(offsets=[-0.25, 0.0, 0.25], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base"]),  # K = 3 + 4 = 7
                    dict(offsets=[0.0], taps=[(-1, -1), (1, 1)], sources=["base"])]                               # K = 3


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    """test_scanline_gpu.py's pair: a two-plane scene with a random texture, 24 x 32 x 3: background d = 2, a box with
    d = 5 on rows 4-19 at left columns 14-23 = right columns 9-18."""
    rng = np.random.default_rng(31)
    back = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    left, right = back[:, :PW].copy(), back[:, 2:PW + 2].copy()
    left[4:20, 14:24] = box[4:20, 14:24]
    right[4:20, 9:19] = box[4:20, 14:24]
    return left, right


@functools.lru_cache(maxsize=None)
def scene():
    """(the left view's D x N volume, disparities, its winner-take-all map, conn, slanted planes through that map); made
    once, only read"""
    from stereo_amd import consistency, terms as T
    disparities = np.arange(PK, dtype=np.float64)
    volume = consistency.pair_volumes(synthetic_pair(), disparities)[0]
    base = T.ncc_best_disp(volume, disparities, 1, (PH, PW))
    base = np.where(np.isfinite(base), base, 0.0)
    planes = PR.planes_through(base, 12)
    return volume, disparities, base, T.construct_neighborhood(PH, PW), planes


def by_hand(prob, levels, kernel):
    """The reference pipeline -> (maps, labels, energies): per level build(plan=None), the table from the problem's own
    conn, aggregate_edges_device over DIRECTIONS_4, the model energy of the labels on the host, apply."""
    import torch
    from stereo_amd import scanline
    shape = (PH, PW)
    maps, labels, energies = [], [], []
    for level in levels:
        prob.build(level, None, TOL)
        table, _ = scanline.edge_table_device(prob.d_conn, prob.E, shape)
        r = scanline.aggregate_edges_device(prob.d_unary, shape, table, prob.d_q, prob.d_qprim, prob.d_alphas, kernel, TOL,
                                            scanline.DIRECTIONS_4)
        torch.cuda.synchronize()
        K = prob.labels_of(level)
        lab = r.labels.cpu().numpy()
        energies.append(scanline.model_energy_edges(prob.d_unary.cpu().numpy().reshape(K, prob.N, order="F"), prob.conn,
                                                    prob.d_q.cpu().numpy().reshape(K, prob.E, order="F"),
                                                    prob.d_qprim.cpu().numpy().reshape(K, prob.E, order="F"),
                                                    prob.d_alphas.cpu().numpy(), kernel, TOL, lab))
        labels.append(lab)
        maps.append(prob.apply(lab))
    return maps, labels, energies


def assert_scanline_levels(out, maps, labels, energies):
    n = len(maps)
    assert len(out.maps) == n and all(same_bits(a, b) for a, b in zip(out.maps, maps))
    assert all(np.array_equal(a, b) for a, b in zip(out.labels, labels))
    assert out.energy == energies
    assert len(out.lower_bound) == n and all(np.isnan(b) for b in out.lower_bound)
    assert out.iterations == [0] * n and out.paths == [0] * n and out.carried == [False] * n
    assert len(set(np.concatenate(labels).tolist())) > 1                 # (the levels move something)


@pytest.mark.parametrize("kernel", [1, 2])
def test_refine_band_by_scanlines_equals_the_pipeline_by_hand(kernel, hip):
    from stereo_amd import band
    volume, disparities, base, conn, _ = scene()
    alphas = np.linspace(0.5, 1.5, conn.shape[1])
    out = hip.refine_band(volume, disparities, WEIGHT, base, kernel, TOL, TWO_BANDS, ITERS, NEVER, alphas=alphas, layout=1, solver="scanline")
    ref = by_hand(band.BandProblem(volume, disparities, WEIGHT, base, conn, alphas, layout=1), TWO_BANDS, kernel)
    assert_scanline_levels(out, *ref)
    assert same_bits(out.dispmap, ref[0][-1]) and out.stage is None


@pytest.mark.parametrize("kernel", [1, 2])
def test_refine_candidates_by_scanlines_equals_the_pipeline_by_hand(kernel, hip):
    from stereo_amd import candidates
    volume, disparities, base, conn, _ = scene()
    levels = candidates.check_levels(CANDIDATES + [dict(offsets=[-0.5, 0.0, 0.5], taps=[(0, -1), (0, 1)], sources=["base"])])
    out = hip.refine_candidates(volume, disparities, WEIGHT, base, kernel, TOL, levels, ITERS, NEVER, layout=1, solver="scanline")
    ref = by_hand(candidates.CandidateProblem(volume, disparities, WEIGHT, base, conn, None, layout=1), levels, kernel)
    assert_scanline_levels(out, *ref)
    assert same_bits(out.dispmap, ref[0][-1])


def plane_source(hip):
    volume, disparities = scene()[:2]
    return hip.NccSource(volume, disparities, WEIGHT, 1, (PH, PW))


@pytest.mark.parametrize("kernel", [1, 2])
def test_refine_plane_band_by_scanlines_equals_the_pipeline_by_hand(kernel, hip):
    from stereo_amd import plane_band
    conn, planes = scene()[3:]
    out = hip.refine_plane_band(plane_source(hip), planes, kernel, TOL, TWO_BANDS, ITERS, NEVER, solver="scanline")
    ref = by_hand(plane_band.PlaneBandProblem(plane_source(hip), planes, conn), TWO_BANDS, kernel)
    assert_scanline_levels(out, *ref)
    assert same_bits(out.planes, ref[0][-1])


@pytest.mark.parametrize("kernel", [1, 2])
def test_refine_plane_candidates_by_scanlines_equals_the_pipeline_by_hand(kernel, hip):
    from stereo_amd import plane_candidates
    conn, planes = scene()[3:]
    levels = plane_candidates.check_levels(PLANE_CANDIDATES)
    out = hip.refine_plane_candidates(plane_source(hip), planes, kernel, TOL, levels, ITERS, NEVER, solver="scanline")
    ref = by_hand(plane_candidates.PlaneCandidateProblem(plane_source(hip), planes, conn), levels, kernel)
    assert_scanline_levels(out, *ref)
    assert same_bits(out.planes, ref[0][-1])


def test_refusals_of_a_scanline_level(hip):
    from stereo_amd import StereoHipError
    volume, disparities, base, conn, _ = scene()
    with pytest.raises(StereoHipError, match="a level of 65 labels \\(at most 64\\)"):
        hip.refine_band(volume, disparities, WEIGHT, base, 1, TOL, [np.arange(65) / 64.0 - 0.5], ITERS, NEVER, layout=1, solver="scanline")
    chords = np.concatenate([conn, np.array([[0], [PH + 1]])], 1)                  # one diagonal edge: not a grid's
    with pytest.raises(StereoHipError, match="stereo_scanline_edges_table: edge %d \\(0, %d\\) does not join" % (conn.shape[1], PH + 1)):
        hip.refine_band(volume, disparities, WEIGHT, base, 1, TOL, BANDS, ITERS, NEVER, layout=1, conn=chords, solver="scanline")
    with pytest.raises(StereoHipError, match="solver must be 'trws' or 'scanline'"):
        hip.refine_band(volume, disparities, WEIGHT, base, 1, TOL, BANDS, ITERS, NEVER, layout=1, solver="sgm")


def same_levels(a, b):
    return (all(same_bits(x, y) for x, y in zip(a.maps, b.maps)) and all(np.array_equal(x, y) for x, y in zip(a.labels, b.labels))
            and a.energy == b.energy and a.lower_bound == b.lower_bound and a.iterations == b.iterations and a.paths == b.paths
            and a.carried == b.carried and len(a.maps) == len(b.maps))


def test_the_default_and_solver_trws_are_what_they_were(hip):
    from stereo_amd import candidates, plane_candidates
    volume, disparities, base, conn, planes = scene()
    plain = hip.refine_band(volume, disparities, WEIGHT, base, 1, TOL, TWO_BANDS, ITERS, NEVER, layout=1, carry=True)
    named = hip.refine_band(volume, disparities, WEIGHT, base, 1, TOL, TWO_BANDS, ITERS, NEVER, layout=1, carry=True, solver="trws")
    assert same_levels(plain, named) and plain.paths == [2, 2] and plain.iterations == [ITERS] * 2
    levels = candidates.check_levels(CANDIDATES)
    plain = hip.refine_candidates(volume, disparities, WEIGHT, base, 1, TOL, levels, ITERS, NEVER, layout=1)
    named = hip.refine_candidates(volume, disparities, WEIGHT, base, 1, TOL, levels, ITERS, NEVER, layout=1, solver="trws")
    assert same_levels(plain, named) and plain.paths == [2] and np.isfinite(plain.lower_bound).all()
    plain = hip.refine_plane_band(plane_source(hip), planes, 2, TOL, TWO_BANDS, ITERS, NEVER)
    named = hip.refine_plane_band(plane_source(hip), planes, 2, TOL, TWO_BANDS, ITERS, NEVER, solver="trws")
    assert same_levels(plain, named) and plain.paths == [2, 2]
    levels = plane_candidates.check_levels(PLANE_CANDIDATES[:1])
    plain = hip.refine_plane_candidates(plane_source(hip), planes, 2, TOL, levels, ITERS, NEVER)
    named = hip.refine_plane_candidates(plane_source(hip), planes, 2, TOL, levels, ITERS, NEVER, solver="trws")
    assert same_levels(plain, named) and plain.paths == [2]


def check_and_fill(hip, maps):
    out = []
    for i, direction in ((0, 1), (1, -1)):
        status, residual = hip.lr_check(maps[i], maps[1 - i], direction, CHECK_TOL)
        out.append((status, residual) + tuple(hip.lr_fill(maps[i], status)))
    return out


@pytest.mark.parametrize("kernel", [1, 2])
def test_the_pair_solve_with_scanline_levels_equals_its_pieces(kernel, hip):
    from stereo_amd import band, candidates, consistency, scanline, terms as T
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL,
                                      candidate_levels=CANDIDATES, band_levels=BANDS, maxiter=ITERS, max_relgap=NEVER,
                                      level_solver="scanline")
    volumes = consistency.pair_volumes(synthetic_pair(), disparities)
    unaries = consistency.pair_unaries(synthetic_pair(), disparities, WEIGHT, volumes)
    conn = T.construct_neighborhood(PH, PW)
    alphas = np.ones(conn.shape[1])
    first = [scanline.aggregate(u, (PH, PW), disparities, kernel, TOL) for u in unaries]
    maps = [[r.dispmap] for r in first]
    energy = [[scanline.model_energy(u, conn, alphas, disparities, kernel, TOL, r.labels)] for u, r in zip(unaries, first)]
    labels = [None, None]
    cand = candidates.check_levels(CANDIDATES)
    for i, v in enumerate(volumes):
        m, l, e = by_hand(candidates.CandidateProblem(v, disparities, WEIGHT, maps[i][-1], conn, alphas, layout=1), cand, kernel)
        maps[i] += m; energy[i] += e
        m, l, e = by_hand(band.BandProblem(v, disparities, WEIGHT, maps[i][-1], conn, alphas, layout=1), [np.asarray(BANDS[0])], kernel)
        maps[i] += m; energy[i] += e; labels[i] = l[-1]
    for i, (view, checked) in enumerate(zip(got.views, check_and_fill(hip, [m[-1] for m in maps]))):
        assert view.energy == energy[i] and len(view.lower_bound) == 3 and np.isnan(view.lower_bound).all()
        assert view.iterations == [0, 0, 0] and view.paths == [0, 0, 0] and view.carried == [False] * 3
        assert len(view.maps) == 3 and all(same_bits(a, b) for a, b in zip(view.maps, maps[i])) and view.dispmap is view.maps[-1]
        assert np.array_equal(view.labels, labels[i])
        status, residual, filled, source = checked
        assert np.array_equal(view.status, status) and same(view.residual, residual)
        assert same(view.filled, filled) and np.array_equal(view.source, source)
    assert {"propagate_1", "propagate_1_check_fill", "band_1", "band_1_check_fill"} <= set(got.times)
    # the default is the TRW-S level it was
    plain = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL, band_levels=BANDS,
                                        maxiter=ITERS, max_relgap=NEVER)
    named = hip.solve_pair_ncc_scanline(synthetic_pair(), disparities, kernel, WEIGHT, TOL, check_tol=CHECK_TOL, band_levels=BANDS,
                                        maxiter=ITERS, max_relgap=NEVER, level_solver="trws")
    for a, b in zip(plain.views, named.views):
        assert a.energy == b.energy and a.lower_bound[1:] == b.lower_bound[1:] and a.paths == b.paths == [0, 2]
        assert same_bits(a.dispmap, b.dispmap)


def test_the_dispmap_ncc_methods_pass_the_solver_through(hip):
    from stereo_amd import band, candidates
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc(list(synthetic_pair()), disparities, 1, WEIGHT, TOL)
    for obj in (dm, dm.mirrored()):
        base = obj._unflip(obj.current_dispmap())
        want = band.refine_band(obj.ncc, disparities, WEIGHT, base, 1, TOL, TWO_BANDS, 3, 0.0, solver="scanline")
        got = obj.refine_band(TWO_BANDS, maxiter=3, solver="scanline")
        assert got.paths == [0, 0] and got.energy == want.energy and same_bits(obj._unflip(obj.current_dispmap()), want.dispmap)
        with pytest.raises(hip.StereoHipError, match="solver='scanline' has no messages to carry"):
            obj.refine_band(TWO_BANDS, maxiter=3, carry=True, solver="scanline")
    for obj in (dm,):
        base = obj._unflip(obj.current_dispmap())
        want = candidates.refine_candidates(obj.ncc, disparities, WEIGHT, base, 1, TOL, CANDIDATES, 3, 0.0, solver="scanline")
        got = obj.refine_candidates(CANDIDATES, maxiter=3, solver="scanline")
        assert got.paths == [0] and got.energy == want.energy and same_bits(obj._unflip(obj.current_dispmap()), want.dispmap)
        obj.assignment = PR.planes_through(np.rint(obj._unflip(obj.current_dispmap())), 12)
        before = obj.assignment.copy()
        want = hip.refine_plane_band(hip.NccSource(obj.ncc, disparities, WEIGHT), before, 1, TOL, TWO_BANDS, 3, 0.0, solver="scanline")
        got = obj.refine_plane_band(TWO_BANDS, maxiter=3, solver="scanline")
        assert got.paths == [0, 0] and got.energy == want.energy and same_bits(obj.assignment, want.planes)
        before = obj.assignment.copy()
        want = hip.refine_plane_candidates(hip.NccSource(obj.ncc, disparities, WEIGHT), before, 1, TOL, PLANE_CANDIDATES, 3, 0.0,
                                           solver="scanline")
        got = obj.refine_plane_candidates(PLANE_CANDIDATES, maxiter=3, solver="scanline")
        assert got.paths == [0, 0] and got.energy == want.energy and same_bits(obj.assignment, want.planes)


def test_the_dispmap_globalstereo_methods_pass_the_solver_through(hip):
    H, W = 19, 27
    im0, im1 = PR.images(H, W, 3, 19)
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))])[:, :, None], (1, 1, 2))
    P[0, 3, 1] = -0.25
    segment = 1 + (np.arange(H)[:, None] // 7) * 4 + (np.arange(W)[None, :] // 9)
    gs = hip.dispmap_globalstereo([im0, im1], P, (0, 9), 4, segment=segment, rng=np.random.default_rng(3))
    gs.max_relgap = 0.0
    base = np.random.default_rng(5).integers(0, 4 * 36 + 1, size=(H, W)).astype(np.float64) / 4.0
    offsets = (np.arange(9, dtype=np.float64) - 4) / 4.0
    levels = [offsets / 16.0, offsets / 64.0]
    gs.assignment = PR.planes_through(base, 14)
    trws = gs.refine_plane_band(levels, maxiter=3)
    gs.assignment = PR.planes_through(base, 14)
    before = gs.assignment.copy()
    out = gs.refine_plane_band(levels, maxiter=3, solver="scanline")
    assert trws.paths == [2, 2] and out.paths == [0, 0] and out.iterations == [0, 0] and np.isnan(out.lower_bound).all()
    assert same_bits(gs.assignment, out.planes) and same_bits(gs.assignment[:3], before[:3]) and not same_bits(gs.assignment[3], before[3])
    gs.update_energy()
    assert abs(gs.energy() - out.energy[-1]) <= 1e-12 * abs(out.energy[-1])          # the object's own energy of these planes
    level = dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base"])
    out = gs.refine_plane_candidates(level, maxiter=3, solver="scanline")
    assert out.paths == [0] and out.iterations == [0] and same_bits(gs.assignment, out.planes)
    gs.update_energy()
    assert abs(gs.energy() - out.energy[-1]) <= 1e-12 * abs(out.energy[-1])
