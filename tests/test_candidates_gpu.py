"""Candidate bands on the device: stereo_candidates_gather / _inputs / _apply and their device forms
against the restatement of the definition (tests/candidates_restate.py) and against K calls of stereo_ncc_unary plus
stereo_trws_positions, bit for bit; the `bad` counters; one level against the CPU oracle on the restated inputs; the chain
whose optimum test_candidates_cpu pins; levels chained by hand; the pyramid with propagate= against the pipeline of solo
plans; the dispmap_ncc method."""
import functools

import numpy as np
import pytest

import band_restate
import candidates_restate as R
import first_principles as fp
import lr_restate
import pyramid_restate
from band_restate import same, same_bits

pytestmark = pytest.mark.gpu

NEVER = -1e300
SHAPES = [(1, 9), (9, 1), (5, 7), (67, 3), (3, 67)]      # 67 crosses a wave along y; K N and K E are no multiples of 256
DEPTHS = [1, 2, 3, 6]                                    # D = 1: t2 is first and last; D = 2: no interior slice
UNARY_WEIGHT = 4.0
NEAR = [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1)]        # (0, 0) and the radius 1
FAR = [(100, 0), (0, -100), (-70, 70), (0, 68), (68, 0), (2, -3)]          # beyond either side of every shape here
GRID = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]            # 25 taps, (0, 0) among them
# (Ko, M, taps): total K = 1, 3, 3, 17, 17, 64, 65, 65 -- 17, 64 and 65 put a block boundary inside a pixel's labels
RECIPES = [(1, 0, []), (3, 0, NEAR[:2]), (1, 1, NEAR[:2]), (9, 2, [NEAR[0], NEAR[2], NEAR[3], FAR[2]]),
           (9, 1, NEAR + FAR[:1]), (9, 1, GRID + NEAR + FAR + GRID[:17]), (3, 2, GRID + FAR), (1, 2, GRID + NEAR)]
assert [ko + m * len(t) for ko, m, t in RECIPES] == [1, 3, 3, 17, 17, 64, 65, 65]


def offsets_for(K):
    return (np.arange(K, dtype=np.float64) - K // 2) / 4.0       # K = 1: [0]; quarter-pixel steps around 0


def label_fastest(ncc):
    """H x W x D -> D x N (layout 1)"""
    H, W, D = ncc.shape
    return np.asfortranarray(ncc.transpose(2, 1, 0).reshape(D, W * H))


@functools.lru_cache(maxsize=None)
def case(H, W, D, recipe, shuffled):
    """One problem and its restated answer, built once, never changed.  Base and sources are band_restate.base_map with
    different seeds: each has, at its first pixels, a value on a slice, midway between two, below and above the range and on
    the two end slices, and the taps carry those to the neighbours."""
    from stereo_amd import terms as T
    Ko, M, taps = RECIPES[recipe]
    ncc = band_restate.volume(H, W, D, 11)
    disp = band_restate.disparities_for(D, shuffled)
    offsets = offsets_for(Ko)
    base = band_restate.base_map(H, W, D, offsets[-1], 5)
    sources = [band_restate.base_map(H, W, D, 0.0, 20 + m)[::-1, ::-1].copy() if m else band_restate.base_map(H, W, D, 0.0, 20)
               for m in range(M)]
    conn = T.construct_neighborhood(H, W)
    cand = R.gather(base, offsets, sources, taps)
    want = R.candidates_inputs(ncc, disp, UNARY_WEIGHT, cand, (H, W), conn)
    labels = np.random.default_rng([H, W, recipe]).integers(1, cand.shape[0] + 1, size=H * W).astype(np.float64)
    applied = R.candidates_apply(cand, labels, (H, W))
    for a in (ncc, disp, offsets, base, conn, cand, labels, applied) + want + tuple(sources):
        a.setflags(write=False)
    return dict(ncc=ncc, disp=disp, offsets=offsets, base=base, sources=sources, taps=taps, conn=conn, cand=cand, want=want,
                labels=labels, applied=applied, K=cand.shape[0])


def to_device(m):
    import torch
    return torch.from_numpy(np.array(np.asarray(m).T, order="C")).cuda()


def sources_to_device(sources):
    import torch
    return torch.stack([to_device(s) for s in sources]).contiguous() if sources else None


def device_problem(c, layout):
    import torch
    vol = c["ncc"] if layout == 0 else label_fastest(c["ncc"])
    d_ncc = torch.from_numpy(np.asfortranarray(vol).reshape(-1, order="F").copy()).cuda()
    d_conn = torch.from_numpy(np.asfortranarray(c["conn"], dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
    return d_ncc, d_conn


# ---------------------------------------------------------------- 1: gather, inputs, apply against the restatement

@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_and_device_forms_equal_the_restatement(shape, D, hip):
    import torch
    from stereo_amd import candidates
    H, W = shape
    N = H * W
    for recipe in range(len(RECIPES)):
        for shuffled in (False, True):
            c = case(H, W, D, recipe, shuffled)
            K, E = c["K"], c["conn"].shape[1]
            what = (H, W, D, RECIPES[recipe][:2], K, shuffled)
            cand = candidates.gather(c["base"], c["offsets"], c["sources"], c["taps"])
            assert cand.shape == (K, N) and same_bits(cand, c["cand"]), what
            assert same_bits(hip.candidates_apply(cand, c["labels"], (H, W)), c["applied"]), what
            d_cand, bad = candidates.gather_device(to_device(c["base"]), c["offsets"], sources_to_device(c["sources"]), c["taps"])
            assert int(bad.item()) == 0 and same_bits(d_cand.cpu().numpy().reshape(N, K).T, c["cand"]), what
            out, bad = hip.candidates_apply_device(d_cand, torch.from_numpy(c["labels"].astype(np.int32)).cuda(), (H, W))
            assert int(bad.item()) == 0 and same_bits(out.cpu().numpy().T, c["applied"]), what
            for layout in (0, 1):
                vol = c["ncc"] if layout == 0 else label_fastest(c["ncc"])
                got = hip.candidates_inputs(vol, c["disp"], UNARY_WEIGHT, cand, (H, W), c["conn"], layout=layout)
                assert got[0].shape == (K, N) and got[1].shape == got[2].shape == (K, E), what
                d_ncc, d_conn = device_problem(c, layout)
                unary, q, qprim, bad = hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_cand, (H, W), d_conn, layout)
                assert int(bad.item()) == 0
                dev = (unary.cpu().numpy().reshape(N, K).T, q.cpu().numpy().reshape(E, K).T, qprim.cpu().numpy().reshape(E, K).T)
                for g, d, restated in zip(got, dev, c["want"]):
                    assert same_bits(g, restated), what + (layout,)
                    assert same_bits(d, restated), what + (layout,)


def test_device_forms_on_a_side_stream_and_their_argument_checks(hip):
    import torch
    from stereo_amd import candidates
    H, W, D = 67, 3, 6
    c = case(H, W, D, 3, True)
    K, N, E = c["K"], H * W, c["conn"].shape[1]
    d_ncc, d_conn = device_problem(c, 1)
    d_base, d_src = to_device(c["base"]), sources_to_device(c["sources"])
    d_lab = torch.from_numpy(c["labels"].astype(np.int32)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    d_cand, bad0 = candidates.gather_device(d_base, c["offsets"], d_src, c["taps"], stream=side, check=False)
    unary, q, qprim, bad1 = hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_cand, (H, W), d_conn, 1, stream=side, check=False)
    out, bad2 = hip.candidates_apply_device(d_cand, d_lab, (H, W), stream=side, check=False)
    side.synchronize()
    assert int(bad0.item()) == int(bad1.item()) == int(bad2.item()) == 0
    assert same_bits(d_cand.cpu().numpy().reshape(N, K).T, c["cand"]) and same_bits(out.cpu().numpy().T, c["applied"])
    assert same_bits(unary.cpu().numpy().reshape(N, K).T, c["want"][0])
    assert same_bits(q.cpu().numpy().reshape(E, K).T, c["want"][1]) and same_bits(qprim.cpu().numpy().reshape(E, K).T, c["want"][2])
    with pytest.raises(hip.StereoHipError, match="column-major"):
        candidates.gather_device(d_base.T, c["offsets"], d_src, c["taps"])
    with pytest.raises(hip.StereoHipError, match=r"\(M, W, H\)"):
        candidates.gather_device(d_base, c["offsets"], d_src[0], c["taps"])
    with pytest.raises(hip.StereoHipError, match="K \\* H \\* W"):
        hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_cand[:-1], (H, W), d_conn, 1)
    with pytest.raises(hip.StereoHipError, match="elements"):
        hip.candidates_inputs_device(d_ncc[:-1], c["disp"], UNARY_WEIGHT, d_cand, (H, W), d_conn, 1)


# ---------------------------------------------------------------- 2: the product against itself: one sampler

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_inputs_equal_K_calls_of_the_existing_entries(shape, hip):
    from stereo_amd import terms as T
    H, W = shape
    points = T.get_points(H, W)
    for D, recipe, shuffled in ((6, 3, False), (3, 4, True), (1, 2, False), (2, 7, True)):
        c = case(H, W, D, recipe, shuffled)
        K = c["K"]
        got = hip.candidates_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, c["cand"], (H, W), c["conn"])
        props = [R.planes(row) for row in c["cand"]]
        unary = np.stack([T.ncc_unary(c["ncc"], c["disp"], UNARY_WEIGHT, P) for P in props])
        q, qprim = T.trws_positions(c["conn"], points, props) if c["conn"].shape[1] else (np.zeros((K, 0)),) * 2
        for g, mine in zip(got, (unary, q, qprim)):
            assert same_bits(g, mine), (H, W, D, recipe)


# ---------------------------------------------------------------- 3: the counters

def test_values_that_are_not_finite_and_labels_out_of_range_are_counted(hip):
    import torch
    from stereo_amd import candidates
    H, W, D = 67, 3, 3
    c = case(H, W, D, 3, False)                  # Ko = 9, two sources, four taps: K = 17
    K, N, E = c["K"], H * W, c["conn"].shape[1]
    base, sources = c["base"].copy(), [s.copy() for s in c["sources"]]
    base[0, 0] = np.nan
    base[64, 1] = np.inf
    sources[0][63, 0] = -np.inf
    sources[1][64, 1] = np.nan                   # the pixel whose base is bad already: counted once
    sources[1][66, 2] = np.nan
    with pytest.raises(hip.StereoHipError, match=r"base is not finite at pixel \(row 0, column 0\)"):
        candidates.gather(base, c["offsets"], sources, c["taps"])
    with pytest.raises(hip.StereoHipError, match=r"source 0 is not finite at pixel \(row 63, column 0\)"):
        candidates.gather(c["base"], c["offsets"], sources, c["taps"])
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")        # (the entry zeroes it)
    d_cand, bad = candidates.gather_device(to_device(base), c["offsets"], sources_to_device(sources), c["taps"], bad=bad, check=False)
    assert int(bad.item()) == 4
    with pytest.raises(hip.StereoHipError, match="not finite at 4 pixel"):
        candidates.gather_device(to_device(base), c["offsets"], sources_to_device(sources), c["taps"])
    # the table is what the restatement gathers from the same maps, the values that are not finite included
    got = d_cand.cpu().numpy().reshape(N, K).T
    want = R.gather(base, c["offsets"], sources, c["taps"])
    assert same(got, want) and np.array_equal(np.isinf(got), np.isinf(want))
    # inputs counts the pixels with a candidate that is not finite; the other pixels' columns are untouched by them
    offenders = ~np.isfinite(want).all(axis=0)
    assert offenders.sum() > 4                                          # the taps spread them
    d_ncc, d_conn = device_problem(c, 0)
    unary, q, qprim, bad = hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_cand, (H, W), d_conn, 0, check=False)
    assert int(bad.item()) == offenders.sum()
    clean = np.where(np.isfinite(want), want, 0.0)
    ref = R.candidates_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, clean, (H, W), c["conn"])
    assert same_bits(unary.cpu().numpy().reshape(N, K)[~offenders].T, ref[0][:, ~offenders])
    with pytest.raises(hip.StereoHipError, match="not finite at %d pixel" % offenders.sum()):
        hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_cand, (H, W), d_conn, 0)
    with pytest.raises(hip.StereoHipError, match=r"cand is not finite at pixel \(row 0, column 0\), label 1"):
        hip.candidates_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, want, (H, W), c["conn"])
    # labels outside 1 .. K
    d_good, _ = candidates.gather_device(to_device(c["base"]), c["offsets"], sources_to_device(c["sources"]), c["taps"])
    for wrong in ([0], [K + 1, -3]):
        broken = c["labels"].copy()
        where = [N // 2, N - 1][:len(wrong)]
        broken[where] = wrong
        with pytest.raises(hip.StereoHipError, match="outside 1 .. %d" % K):
            hip.candidates_apply(c["cand"], broken, (H, W))
        out, bad = hip.candidates_apply_device(d_good, torch.from_numpy(broken.astype(np.int32)).cuda(), (H, W), check=False)
        got = out.cpu().numpy().reshape(-1)
        ok = np.ones(N, bool)
        ok[where] = False
        assert int(bad.item()) == len(wrong) and np.isnan(got[~ok]).all()
        assert same_bits(got[ok], c["applied"].T.reshape(-1)[ok])
        with pytest.raises(hip.StereoHipError, match="%d label" % len(wrong)):
            hip.candidates_apply_device(d_good, torch.from_numpy(broken.astype(np.int32)).cuda(), (H, W))
    # an edge that names a pixel outside the image: NaN positions, everything else as it was
    conn = np.array(c["conn"], dtype=np.uint32)
    conn[1, 5] = N
    conn[0, E - 1] = 0xFFFFFFFF
    d_bad_conn = torch.from_numpy(np.asfortranarray(conn).reshape(-1, order="F").view(np.int32).copy()).cuda()
    unary, q, qprim, bad = hip.candidates_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_good, (H, W), d_bad_conn, 0)
    q, qprim = q.cpu().numpy().reshape(E, K).T, qprim.cpu().numpy().reshape(E, K).T
    assert np.isnan(q[:, 5]).all() and np.isnan(qprim[:, E - 1]).all()
    wq, wqp = c["want"][1].copy(), c["want"][2].copy()
    wq[:, 5] = np.nan
    wqp[:, E - 1] = np.nan
    assert same(q, wq) and same(qprim, wqp) and same_bits(unary.cpu().numpy().reshape(N, K).T, c["want"][0])
    with pytest.raises(hip.StereoHipError, match="edge 5"):
        hip.candidates_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, c["cand"], (H, W), conn)


# ---------------------------------------------------------------- 4: one level against the oracle

LEVEL_TAPS = [(0, 0), (1, 0), (0, -1)]


@functools.lru_cache(maxsize=None)
def level_case(H, W):
    """K = 3 + 2 * 3 = 9 around band_restate's base: the base and another map at (0, 0) and two neighbours."""
    from stereo_amd import terms as T
    ncc = band_restate.volume(H, W, 6, 11)
    disp = band_restate.disparities_for(6, False)
    offsets = offsets_for(3)
    base = band_restate.base_map(H, W, 6, offsets[-1], 5)
    other = band_restate.base_map(H, W, 6, 0.0, 31)[::-1].copy()
    conn = T.construct_neighborhood(H, W)
    level = dict(offsets=offsets, taps=LEVEL_TAPS, sources=["base", other])
    cand = R.gather(base, offsets, [base, other], LEVEL_TAPS)
    want = R.candidates_inputs(ncc, disp, UNARY_WEIGHT, cand, (H, W), conn)
    return dict(ncc=ncc, disp=disp, base=base, other=other, conn=conn, level=level, cand=cand, want=want)


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (67, 3)], ids=lambda s: "%dx%d" % s)
def test_one_level_equals_the_oracle_on_the_restated_inputs(shape, kernel, hip, oracle):
    H, W = shape
    c = level_case(H, W)
    unary, q, qprim = c["want"]
    E = c["conn"].shape[1]
    tol = 2.0
    ref = oracle.trws(kernel, np.ascontiguousarray(unary.T), c["conn"].T, np.ascontiguousarray(q.T), np.ascontiguousarray(qprim.T),
                      np.ones(E), tol, 5, NEVER, mode=1)
    got = hip.refine_candidates(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], kernel, tol, [c["level"]], 5, NEVER)
    assert got.paths == [2]                                # the Pipe family: K <= 64, exact messages, positions per edge
    assert np.array_equal(got.labels[0], ref[0])
    assert (got.energy, got.lower_bound, got.iterations) == ([ref[1]], [ref[2]], [ref[3]])
    assert got.carried == [False]
    assert same_bits(got.dispmap, R.candidates_apply(c["cand"], ref[0], (H, W))) and got.maps[0] is got.dispmap
    # the label-fastest volume gives the same problem
    got1 = hip.refine_candidates(label_fastest(c["ncc"]), c["disp"], UNARY_WEIGHT, c["base"], kernel, tol, [c["level"]], 5, NEVER, layout=1)
    assert np.array_equal(got1.labels[0], ref[0]) and got1.energy == got.energy and got1.lower_bound == got.lower_bound


# ---------------------------------------------------------------- 5: the chain

@pytest.mark.parametrize("shape", [(1, 17), (17, 1)], ids=lambda s: "%dx%d" % s)
def test_candidates_on_the_chain_reach_the_true_map_and_the_band_does_not(shape, hip):
    """The chain of test_candidates_cpu (its docstring has the exactness argument: every energy and message is exact in
    fp64).  The candidate level reaches energy = bound = the dynamic programme's optimum, which is the energy of the true
    map; the band around the same base cannot: its result is held against the DP optimum of the band problem."""
    from fractions import Fraction
    c = R.chain(shape)
    cand = R.gather(c["base"], c["level"]["offsets"], [c["base"]], c["level"]["taps"])
    unary, q, qprim = R.candidates_inputs(c["ncc"], c["disp"], R.CHAIN_WEIGHT, cand, shape, c["conn"])
    mk = lambda u, a, b: dict(unary=np.ascontiguousarray(u.T), conn=c["conn"].T.copy(), q=np.ascontiguousarray(a.T),
                              qprim=np.ascontiguousarray(b.T), alphas=np.ones(R.CHAIN_N - 1), lam=R.CHAIN_LAMBDA)
    p = mk(unary, q, qprim)
    pb = mk(*band_restate.band_inputs(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base"], R.CHAIN_BAND, c["conn"]))
    opt, _ = fp.chain_dp(p, 2, R.CHAIN_LAMBDA)
    opt_band, _ = fp.chain_dp(pb, 2, R.CHAIN_LAMBDA)
    got = hip.refine_candidates(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base"], 2, R.CHAIN_LAMBDA, [c["level"]], 3, NEVER, conn=c["conn"])
    print("chain %dx%d: energy %r bound %r optimum %r (band's optimum %r)" % (shape + (got.energy[0], got.lower_bound[0], opt, opt_band)))
    assert opt == 2.0 and got.energy[0] == opt and got.lower_bound[0] == opt
    assert fp.energy_exact(p, 2, R.CHAIN_LAMBDA, got.labels[0].astype(np.int64) - 1) == Fraction(opt)
    assert same_bits(got.dispmap, c["truth"])
    banded = hip.refine_band(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base"], 2, R.CHAIN_LAMBDA, [R.CHAIN_BAND], 3, NEVER, conn=c["conn"])
    print("             the band: energy %r bound %r" % (banded.energy[0], banded.lower_bound[0]))
    assert opt_band > opt and banded.energy[0] >= opt_band > opt
    assert fp.energy_exact(pb, 2, R.CHAIN_LAMBDA, banded.labels[0].astype(np.int64) - 1) >= Fraction(opt_band)
    assert not same(banded.dispmap, c["truth"])


# ---------------------------------------------------------------- 6: levels, and the pyramid

def test_two_levels_equal_two_calls_chained_by_hand(hip):
    c = level_case(5, 7)
    first = c["level"]
    second = dict(offsets=offsets_for(9) / 4.0, taps=[(0, 0), (0, 1)], sources=["wta", "base"])      # K = 13: a plan of its own
    args = (c["disp"], UNARY_WEIGHT)
    both = hip.refine_candidates(c["ncc"], *args, c["base"], 1, 2.0, [first, second], 4, NEVER)
    one = hip.refine_candidates(c["ncc"], *args, c["base"], 1, 2.0, [first], 4, NEVER)
    two = hip.refine_candidates(c["ncc"], *args, one.dispmap, 1, 2.0, [second], 4, NEVER)
    assert len(both.maps) == 2 and same_bits(both.maps[0], one.dispmap) and same_bits(both.dispmap, two.dispmap)
    assert np.array_equal(both.labels[0], one.labels[0]) and np.array_equal(both.labels[1], two.labels[0])
    assert both.energy == one.energy + two.energy and both.lower_bound == one.lower_bound + two.lower_bound
    assert both.iterations == [4.0, 4.0] and both.paths == [2, 2] and both.carried == [False, False]
    # 'wta' is the volume's best-disparity map, 'base' the map the level starts from
    from stereo_amd import terms as T
    wta = T.ncc_best_disp(c["ncc"], c["disp"])
    by_map = hip.refine_candidates(c["ncc"], *args, one.dispmap, 1, 2.0, [dict(second, sources=[wta, one.dispmap])], 4, NEVER)
    assert np.array_equal(by_map.labels[0], two.labels[0]) and same_bits(by_map.dispmap, two.dispmap) and by_map.energy == two.energy
    # an equal K shares the plan: the second bind starts from zero as the first did
    again = hip.refine_candidates(c["ncc"], *args, c["base"], 1, 2.0, [first, first], 4, NEVER)
    solo = hip.refine_candidates(c["ncc"], *args, one.dispmap, 1, 2.0, [first], 4, NEVER)
    assert np.array_equal(again.labels[1], solo.labels[0]) and again.energy[1:] == solo.energy


ITERS = 4
CHECK_TOL = 1.0
BAND = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
PYRAMID_BANDS = [[BAND, np.array([-0.5, 0.0, 0.5])], [BAND]]
RING = [(-1, 0), (1, 0), (0, -1), (0, 1), (-2, 0), (2, 0), (0, -2), (0, 2)]
PROPAGATE = [[dict(offsets=[-0.5, 0.0, 0.5], taps=RING, sources=["base"]), dict(offsets=[0.0], taps=[(0, 0)] + RING[:4], sources=["wta", "base"])],
             [dict(offsets=[-1.0, 0.0, 1.0], taps=[(0, 0)] + RING, sources=["wta"])]]


@functools.lru_cache(maxsize=None)
def pyramid_by_hand(kernel):
    """solve_pair_ncc_pyramid(levels=2, propagate=PROPAGATE, bands=PYRAMID_BANDS) from solo plans: the restated reduce and
    expand, pair_volumes, CandidateProblem and BandProblem built and applied one view at a time, lr_restate."""
    from stereo_amd import candidates, band, consistency, terms as T
    from stereo_amd.trws import TrwsPlan
    from test_consistency_gpu import PK, UNARY_WEIGHT as WEIGHT, TOL
    from test_pyramid_gpu import restated_images
    images = restated_images()
    disparities = np.arange(PK, dtype=np.float64)
    levels = 2
    volumes = [consistency.pair_volumes(images[l], pyramid_restate.level_disparities(disparities, l)) for l in range(levels + 1)]
    views = []
    for i in range(2):
        out = [dict(maps=[], labels=[], energy=[], bound=[], iters=[], expanded=None) for _ in range(levels + 1)]

        def run(rec, plan, to_map):
            plan.iterate(ITERS, NEVER)
            labels, en, lb, it = plan.result()
            assert plan.path() == 2 or rec is out[levels]
            plan.close()
            rec["labels"].append(labels); rec["energy"].append(en); rec["bound"].append(lb); rec["iters"].append(it)
            rec["maps"].append(to_map(labels))

        H, W = images[levels][i].shape[:2]
        conn = T.construct_neighborhood(H, W)
        tol_l, weight = pyramid_restate.level_model(kernel, TOL, levels)
        disp = pyramid_restate.level_disparities(disparities, levels)
        plan = TrwsPlan(kernel, disp.shape[0], H * W, conn)
        plan.upload(WEIGHT * (1.0 - volumes[levels][i]), weight * np.ones(conn.shape[1]), tol_l, positions=disp)
        run(out[levels], plan, lambda labels: disp[labels.astype(np.int64) - 1].reshape(W, H).T)
        for l in range(levels - 1, -1, -1):
            H, W = images[l][i].shape[:2]
            conn = T.construct_neighborhood(H, W)
            tol_l, weight = pyramid_restate.level_model(kernel, TOL, l)
            disp = pyramid_restate.level_disparities(disparities, l)
            alphas = weight * np.ones(conn.shape[1])
            rec = out[l]
            rec["expanded"], _ = pyramid_restate.expand(out[l + 1]["maps"][-1], (H, W), 1, images[l][i], images[l + 1][i])
            prob = candidates.CandidateProblem(volumes[l][i], disp, WEIGHT, rec["expanded"], conn, alphas, layout=1)
            for level in candidates.check_levels(PROPAGATE[l]):
                plan = TrwsPlan(kernel, prob.labels_of(level), H * W, conn)
                prob.build(level, plan, tol_l)
                run(rec, plan, prob.apply)
            prob = band.BandProblem(volumes[l][i], disp, WEIGHT, rec["maps"][-1], conn, alphas, layout=1)
            for offsets in PYRAMID_BANDS[l]:
                plan = TrwsPlan(kernel, len(offsets), H * W, conn)
                prob.build(np.asarray(offsets), plan, tol_l)
                run(rec, plan, prob.apply)
        views.append(out)
    for l in range(levels + 1):
        maps = [views[i][l]["maps"][-1] for i in range(2)]
        for i, direction in ((0, 1), (1, -1)):
            rec = views[i][l]
            rec["status"], rec["residual"] = lr_restate.lr_check(maps[i], maps[1 - i], direction, CHECK_TOL / 2 ** l)
            rec["filled"], rec["source"] = lr_restate.lr_fill(maps[i], rec["status"])
    return views


@pytest.mark.parametrize("kernel", [1, 2])
def test_the_pyramid_with_propagate_equals_the_pipeline_by_hand(kernel, hip):
    from test_consistency_gpu import rendered_pair, PK, UNARY_WEIGHT as WEIGHT, TOL
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_pyramid(rendered_pair(), disparities, kernel, WEIGHT, TOL, 2, ITERS, NEVER, bands=PYRAMID_BANDS,
                                     expand="guided", check_tol=CHECK_TOL, propagate=PROPAGATE)
    want = pyramid_by_hand(kernel)
    for l in range(3):
        passes = 1 if l == 2 else len(PROPAGATE[l]) + len(PYRAMID_BANDS[l])
        for view, ref in zip(got.levels[l].views, (want[0][l], want[1][l])):
            assert len(view.maps) == len(view.energy) == len(view.paths) == len(view.carried) == passes
            assert (view.energy, view.lower_bound, view.iterations) == (ref["energy"], ref["bound"], ref["iters"]), l
            assert np.array_equal(view.labels, ref["labels"][-1]), l
            assert all(same_bits(a, b) for a, b in zip(view.maps, ref["maps"])) and view.dispmap is view.maps[-1]
            assert view.carried == [False] * passes
            assert np.array_equal(view.status, ref["status"]) and same(view.residual, ref["residual"])
            assert same(view.filled, ref["filled"]) and np.array_equal(view.source, ref["source"])
            if l < 2:
                assert view.paths == [2] * passes and same_bits(view.expanded, ref["expanded"])
                assert {"propagate_1", "propagate_1_check_fill", "band_1", "band_1_check_fill"} <= set(got.levels[l].times)
    # the passes did something: a propagated label was chosen somewhere
    assert any((ref["labels"][0] > 3).any() for ref in (want[0][0], want[1][0]))


def test_the_pyramid_without_propagate_is_what_it_was_and_carry_stops_at_a_candidate_pass(hip):
    from test_consistency_gpu import rendered_pair, PK, UNARY_WEIGHT as WEIGHT, TOL
    disparities = np.arange(PK, dtype=np.float64)
    args = (rendered_pair(), disparities, 1, WEIGHT, TOL, 2, ITERS, NEVER)
    for carry in ("none", "scales"):
        a = hip.solve_pair_ncc_pyramid(*args, bands=PYRAMID_BANDS, carry=carry)
        b = hip.solve_pair_ncc_pyramid(*args, bands=PYRAMID_BANDS, carry=carry, propagate=None)
        e = hip.solve_pair_ncc_pyramid(*args, bands=PYRAMID_BANDS, carry=carry, propagate=[[], None])
        for other in (b, e):
            assert list(a.times) == list(other.times)
            for la, lb in zip(a.levels, other.levels):
                assert list(la.times) == list(lb.times)
                for va, vb in zip(la.views, lb.views):
                    assert (va.energy, va.lower_bound, va.iterations, va.paths, va.carried) == (vb.energy, vb.lower_bound, vb.iterations, vb.paths, vb.carried)
                    assert np.array_equal(va.labels, vb.labels) and np.array_equal(va.status, vb.status)
                    assert len(va.maps) == len(vb.maps) and all(same_bits(x, y) for x, y in zip(va.maps, vb.maps))
                    assert same(va.filled, vb.filled) and same(va.residual, vb.residual)
    # carried messages: the band after a candidate pass starts from zero and says so; the bands after it carry on
    with_carry = hip.solve_pair_ncc_pyramid(*args, bands=PYRAMID_BANDS, carry="scales", propagate=[PROPAGATE[0][:1], []])
    assert a.levels[0].left.carried == [True, True] and a.levels[1].left.carried == [True]
    assert with_carry.levels[0].left.carried == [False, False, True] and with_carry.levels[1].left.carried == [True]
    # one view: the same passes in ViewPyramidResult
    from stereo_amd import pyramid
    solo = pyramid.solve_view_ncc_pyramid(rendered_pair(), disparities, 1, WEIGHT, TOL, 2, ITERS, NEVER, bands=PYRAMID_BANDS,
                                          propagate=PROPAGATE)
    pair = pyramid_by_hand(1)[0]
    for l in range(3):
        assert (solo.energy[l], solo.lower_bound[l], solo.iterations[l]) == (pair[l]["energy"], pair[l]["bound"], pair[l]["iters"])
        assert all(same_bits(x, y) for x, y in zip(solo.maps[l], pair[l]["maps"])) and len(solo.maps[l]) == len(pair[l]["maps"])
    assert same_bits(solo.dispmap, pair[0]["maps"][-1])


# ---------------------------------------------------------------- 7: the objects

def test_dispmap_ncc_refine_candidates_plain_and_mirrored(hip):
    from stereo_amd import candidates
    from test_band_gpu import small_pair, PK, PAIR_WEIGHT, PAIR_TOL
    left, right = small_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    m = dm.mirrored()
    for obj in (dm, m):
        obj.max_relgap = 0.0
        obj.set_disparity(np.rint(obj.current_dispmap()))
        before = obj.current_dispmap().copy()
        extra = np.full(before.shape, 1.0)
        extra[:, :3] = 2.0                                  # in the image's own columns
        levels = [dict(offsets=[-0.25, 0.0, 0.25], taps=[(0, 1), (0, 2), (1, 0)], sources=["base", "wta", extra])]
        internal = before[:, ::-1] if obj._mirrored else before
        flip = (lambda a: a[:, ::-1]) if obj._mirrored else (lambda a: a)
        inner = [dict(levels[0], taps=[(0, -1), (0, -2), (1, 0)] if obj._mirrored else levels[0]["taps"],
                      sources=["base", "wta", flip(extra)])]
        want = candidates.refine_candidates(obj.ncc, disparities, PAIR_WEIGHT, internal, 1, PAIR_TOL, inner, 3, 0.0)
        out = obj.refine_candidates(levels, maxiter=3)
        after = obj.current_dispmap()
        assert same(after, flip(want.dispmap))        # (the object keeps planes: a disparity 0 comes back as -0)
        assert out.energy == want.energy and len(out.energy) == 1 and np.array_equal(out.labels[0], want.labels[0])
        assert np.isfinite(obj.energy())
    glob = object.__new__(hip.dispmap_globalstereo)
    with pytest.raises(hip.StereoHipError, match="dispmap_globalstereo"):
        glob.refine_candidates(levels)
