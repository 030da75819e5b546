"""Band refinement on the device: stereo_band_inputs / stereo_band_apply and their device forms against
K calls of stereo_ncc_unary, stereo_trws_positions and the restatement of the definition (tests/band_restate.py), bit for
bit; the solve against the CPU oracle on the restated inputs and, on a chain, against dynamic programming; refine_band's
levels; solve_pair_ncc with band levels against the same pipeline built from solo plans and the restatements; the
dispmap_ncc method."""
import functools

import numpy as np
import pytest

import band_restate as R
import first_principles as fp
import lr_restate
from band_restate import same, same_bits

pytestmark = pytest.mark.gpu

NEVER = -1e300
SHAPES = [(1, 9), (9, 1), (5, 7), (67, 3), (3, 67)]      # 67 crosses a wave along y; K N and K E are no multiples of 256
DEPTHS = [1, 2, 3, 6]                                    # D = 1: t2 is first and last; D = 2: no interior slice
BAND_K = [1, 3, 9, 17, 65]                               # 65 for the builder alone (no solve)
UNARY_WEIGHT = 4.0


def offsets_for(K):
    return (np.arange(K, dtype=np.float64) - K // 2) / 4.0       # K = 1: [0]; quarter-pixel steps around 0


def label_fastest(ncc):
    """H x W x D -> D x N (layout 1)"""
    H, W, D = ncc.shape
    return np.asfortranarray(ncc.transpose(2, 1, 0).reshape(D, W * H))


@functools.lru_cache(maxsize=None)
def case(H, W, D, K, shuffled):
    """One problem and its restated answer, built once, never changed."""
    from stereo_amd import terms as T
    ncc = R.volume(H, W, D, 11)
    disp = R.disparities_for(D, shuffled)
    offsets = offsets_for(K)
    base = R.base_map(H, W, D, offsets[-1], 5)
    conn = T.construct_neighborhood(H, W)
    want = R.band_inputs(ncc, disp, UNARY_WEIGHT, base, offsets, conn)
    for a in (ncc, disp, offsets, base, conn) + want:
        a.setflags(write=False)
    return dict(ncc=ncc, disp=disp, offsets=offsets, base=base, conn=conn, want=want)


# ---------------------------------------------------------------- 1: the builder

@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_inputs_equal_the_existing_kernels_and_the_restatement(shape, D, hip):
    from stereo_amd import terms as T
    H, W = shape
    points = T.get_points(H, W)
    for K in BAND_K:
        for shuffled in (False, True):
            c = case(H, W, D, K, shuffled)
            got0 = hip.band_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], c["offsets"], c["conn"])
            got1 = hip.band_inputs(label_fastest(c["ncc"]), c["disp"], UNARY_WEIGHT, c["base"], c["offsets"], c["conn"], layout=1)
            what = (H, W, D, K, shuffled)
            props = [R.planes(c["base"], d) for d in c["offsets"]]
            unary = np.stack([T.ncc_unary(c["ncc"], c["disp"], UNARY_WEIGHT, P) for P in props])
            q, qprim = T.trws_positions(c["conn"], points, props) if c["conn"].shape[1] else (np.zeros((K, 0)),) * 2
            for got in (got0, got1):
                assert got[0].shape == (K, H * W) and got[1].shape == got[2].shape == (K, c["conn"].shape[1]), what
                for g, mine, restated in zip(got, (unary, q, qprim), c["want"]):
                    assert same_bits(g, mine), what            # the existing kernels, K calls
                    assert same_bits(g, restated), what        # the definition


def test_the_crafted_pixels_reach_every_rule_of_the_sampler(hip):
    c = case(5, 7, 6, 9, False)
    unary = hip.band_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], c["offsets"], c["conn"])[0]
    out = UNARY_WEIGHT * (1.0 + 1e6)
    zero = 4                                              # offsets[4] == 0
    flat = c["ncc"].transpose(1, 0, 2).reshape(-1, 6)     # [pixel, slice]
    assert unary[zero, 0] != out                          # on an interior slice
    assert unary[zero, 1] == UNARY_WEIGHT * (1.0 - (flat[1, 1] * 0.75 + flat[1, 0] * 0.375 - flat[1, 2] * 0.125))   # midway: the tie goes to slice 1
    assert (unary[:, 2] == out).all() and unary[zero, 3] == out        # below the range with every offset; above it
    assert unary[zero, 4] == UNARY_WEIGHT * (1.0 - flat[4, 5]) and (unary[zero + 1:, 4] == out).all()   # the last slice; beyond it
    assert unary[zero, 5] == UNARY_WEIGHT * (1.0 - flat[5, 0]) and (unary[:zero, 5] == out).all()       # the first slice; before it


def to_device(m):
    import torch
    return torch.from_numpy(np.array(np.asarray(m).T, order="C")).cuda()


def device_problem(c, layout):
    import torch
    vol = c["ncc"] if layout == 0 else label_fastest(c["ncc"])
    d_ncc = torch.from_numpy(np.asfortranarray(vol).reshape(-1, order="F").copy()).cuda()
    d_conn = torch.from_numpy(np.asfortranarray(c["conn"], dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()
    return d_ncc, d_conn


@pytest.mark.parametrize("layout", [0, 1])
def test_device_forms_on_a_side_stream_give_the_host_forms_bits(layout, hip):
    import torch
    for (H, W), D, K in (((1, 9), 1, 1), ((3, 67), 3, 9), ((67, 3), 6, 17)):
        c = case(H, W, D, K, True)
        d_ncc, d_conn = device_problem(c, layout)
        d_base = to_device(c["base"])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        unary, q, qprim, bad = hip.band_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_base, c["offsets"], d_conn, layout, stream=side,
                                                      check=False)
        side.synchronize()
        E = c["conn"].shape[1]
        assert int(bad.item()) == 0
        assert same_bits(unary.cpu().numpy().reshape(H * W, K).T, c["want"][0])
        assert same_bits(q.cpu().numpy().reshape(E, K).T, c["want"][1]) and same_bits(qprim.cpu().numpy().reshape(E, K).T, c["want"][2])
    with pytest.raises(hip.StereoHipError, match="column-major"):
        hip.band_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, d_base.T, c["offsets"], d_conn, layout)
    with pytest.raises(hip.StereoHipError, match="elements"):
        hip.band_inputs_device(d_ncc[:-1], c["disp"], UNARY_WEIGHT, d_base, c["offsets"], d_conn, layout)


# ---------------------------------------------------------------- 2: a base that is not finite

def test_a_base_that_is_not_finite(hip):
    import torch
    H, W, D, K = 67, 3, 3, 9
    c = case(H, W, D, K, False)
    base = c["base"].copy()
    where = [(0, 0), (63, 0), (64, 1), (66, 2), (5, 1)]
    for (y, x), v in zip(where, (np.nan, np.inf, -np.inf, np.nan, np.inf)):
        base[y, x] = v
    with pytest.raises(hip.StereoHipError, match="row 0, column 0"):
        hip.band_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, base, c["offsets"], c["conn"])
    d_ncc, d_conn = device_problem(c, 0)
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")        # (the entry zeroes it)
    unary, q, qprim, bad = hip.band_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, to_device(base), c["offsets"], d_conn, bad=bad, check=False)
    assert int(bad.item()) == len(where)
    # the other pixels' columns are what they are without the offenders
    keep = np.isfinite(base.T.reshape(-1))
    assert same_bits(unary.cpu().numpy().reshape(H * W, K)[keep].T, c["want"][0][:, keep])
    with pytest.raises(hip.StereoHipError, match="not finite at 5 pixel"):
        hip.band_inputs_device(d_ncc, c["disp"], UNARY_WEIGHT, to_device(base), c["offsets"], d_conn)


# ---------------------------------------------------------------- 3: apply

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_apply_equals_the_restatement(shape, hip):
    import torch
    H, W = shape
    for K in (1, 3, 9, 17):
        offsets = offsets_for(K)
        base = R.base_map(H, W, 6, offsets[-1], 9)
        labels = np.random.default_rng([H, W, K]).integers(1, K + 1, size=H * W).astype(np.float64)
        want = R.band_apply(base, labels, offsets)
        assert same_bits(hip.band_apply(base, labels, offsets), want)
        assert same_bits(hip.band_apply(base, labels.reshape(W, H).T, offsets), want)
        d_lab = torch.from_numpy(labels.astype(np.int32)).cuda()
        refined, bad = hip.band_apply_device(to_device(base), d_lab, offsets)
        assert same_bits(refined.cpu().numpy().T, want) and int(bad.item()) == 0
        for wrong in (0, K + 1):
            broken = labels.copy()
            broken[H * W // 2] = wrong
            with pytest.raises(hip.StereoHipError, match="outside 1 .. %d" % K):
                hip.band_apply(base, broken, offsets)
            refined, bad = hip.band_apply_device(to_device(base), torch.from_numpy(broken.astype(np.int32)).cuda(), offsets, check=False)
            got = refined.cpu().numpy().T
            assert int(bad.item()) == 1 and np.isnan(got.T.reshape(-1)[H * W // 2])
            ok = np.arange(H * W) != H * W // 2
            assert same_bits(got.T.reshape(-1)[ok], want.T.reshape(-1)[ok])
            with pytest.raises(hip.StereoHipError, match="1 label"):
                hip.band_apply_device(to_device(base), torch.from_numpy(broken.astype(np.int32)).cuda(), offsets)


# ---------------------------------------------------------------- 4: the solve against the oracle

@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (67, 3)], ids=lambda s: "%dx%d" % s)
def test_one_level_equals_the_oracle_on_the_restated_inputs(shape, kernel, hip, oracle):
    H, W = shape
    c = case(H, W, 6, 9, False)
    unary, q, qprim = c["want"]
    E = c["conn"].shape[1]
    tol = 2.0
    ref = oracle.trws(kernel, np.ascontiguousarray(unary.T), c["conn"].T, np.ascontiguousarray(q.T), np.ascontiguousarray(qprim.T),
                      np.ones(E), tol, 5, NEVER, mode=1)
    got = hip.refine_band(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], kernel, tol, [c["offsets"]], 5, NEVER)
    assert got.paths == [2]                                # the Pipe family: K <= 64, exact messages, positions per edge
    assert np.array_equal(got.labels[0], ref[0])
    assert (got.energy, got.lower_bound, got.iterations) == ([ref[1]], [ref[2]], [ref[3]])
    assert same_bits(got.dispmap, R.band_apply(c["base"], ref[0], c["offsets"])) and got.maps[0] is got.dispmap
    # the label-fastest volume gives the same problem
    got1 = hip.refine_band(label_fastest(c["ncc"]), c["disp"], UNARY_WEIGHT, c["base"], kernel, tol, [c["offsets"]], 5, NEVER, layout=1)
    assert np.array_equal(got1.labels[0], ref[0]) and got1.energy == got.energy and got1.lower_bound == got.lower_bound


# ---------------------------------------------------------------- 5: first principles, no oracle in between

@pytest.mark.parametrize("shape", [(1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_band_on_a_chain_reaches_the_dynamic_programmes_optimum(shape, hip):
    """Every number is dyadic (first_principles' argument): the volume is a multiple of 2^-6 with slices one apart, so
    the parabola's coefficients are multiples of 2^-7; base and offsets are multiples of 1/4, so a sample is a multiple
    of 2^-11 below 2^10 and a unary (weight 4, or 4 (1 + 1e6)) one of 2^-9 below 2^23; squared position differences are
    multiples of 2^-4.  Sums of 9 + 8 such terms need under 40 bits: fp64 holds every energy and message exactly.  The
    quadratic kernel only: with positions on a regular grid the linear kernel's exact-message mode meets the envelope
    ties that first_principles.FINE_BITS describes, and the bound is then not held to the optimum."""
    H, W = shape
    N = 9
    ncc = R.volume(H, W, 6, 21)
    disp = R.disparities_for(6, False)
    offsets = offsets_for(9)
    base = R.base_map(H, W, 6, offsets[-1], 13)
    conn = np.stack([np.arange(N - 1), np.arange(1, N)])           # the path 0 - 1 - ... - 8, one edge per pair
    lam = 2.0
    unary, q, qprim = R.band_inputs(ncc, disp, UNARY_WEIGHT, base, offsets, conn)
    p = dict(unary=np.ascontiguousarray(unary.T), conn=conn.T.copy(), q=np.ascontiguousarray(q.T),
             qprim=np.ascontiguousarray(qprim.T), alphas=np.ones(N - 1), lam=lam)
    opt, _ = fp.chain_dp(p, 2, lam)
    got = hip.refine_band(ncc, disp, UNARY_WEIGHT, base, 2, lam, [offsets], 3, NEVER, conn=conn)
    print("chain %dx%d: energy %r bound %r optimum %r" % (H, W, got.energy[0], got.lower_bound[0], opt))
    assert got.energy[0] == opt and got.lower_bound[0] == opt
    from fractions import Fraction
    assert fp.energy_exact(p, 2, lam, got.labels[0].astype(np.int64) - 1) == Fraction(opt)
    assert same_bits(got.dispmap, R.band_apply(base, got.labels[0], offsets))


# ---------------------------------------------------------------- 6: levels

def test_two_levels_equal_two_calls_chained_by_hand(hip):
    c = case(5, 7, 6, 9, False)
    coarse, fine = c["offsets"], c["offsets"] / 4.0
    args = (c["disp"], UNARY_WEIGHT)
    both = hip.refine_band(c["ncc"], *args, c["base"], 1, 2.0, [coarse, fine], 4, NEVER)
    one = hip.refine_band(c["ncc"], *args, c["base"], 1, 2.0, [coarse], 4, NEVER)
    two = hip.refine_band(c["ncc"], *args, one.dispmap, 1, 2.0, [fine], 4, NEVER)
    assert len(both.maps) == 2 and same_bits(both.maps[0], one.dispmap) and same_bits(both.dispmap, two.dispmap)
    assert np.array_equal(both.labels[0], one.labels[0]) and np.array_equal(both.labels[1], two.labels[0])
    assert both.energy == one.energy + two.energy and both.lower_bound == one.lower_bound + two.lower_bound
    assert both.iterations == [4.0, 4.0] and both.paths == [2, 2]
    # a level with another K gets a plan of its own
    mixed = hip.refine_band(c["ncc"], *args, c["base"], 1, 2.0, [coarse, offsets_for(3)], 4, NEVER)
    assert same_bits(mixed.maps[0], one.dispmap) and len(mixed.maps) == 2


# ---------------------------------------------------------------- 7: both views of a pair

PH, PW, PK = 12, 16, 4
PAIR_WEIGHT, PAIR_TOL, PAIR_ITERS = 40.0, 2.0, 4
PAIR_LEVELS = (offsets_for(9), offsets_for(9) / 4.0)


@functools.lru_cache(maxsize=None)
def small_pair():
    """12 x 16 x 3, a random texture: background d = 1, a box with d = 3 on rows 3-8 at left columns 8-11 = right 5-8."""
    rng = np.random.default_rng(17)
    back = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    left, right = back[:, :PW].copy(), back[:, 1:PW + 1].copy()
    left[3:9, 8:12] = box[3:9, 8:12]
    right[3:9, 5:9] = box[3:9, 8:12]
    return left, right


def pipeline_by_hand(refine_iters):
    """solve_pair_ncc's steps from solo plans, the band restatement and lr_restate"""
    from stereo_amd import consistency, terms as T
    from stereo_amd.trws import TrwsPlan
    disparities = np.arange(PK, dtype=np.float64)
    volumes = consistency.pair_volumes(small_pair(), disparities)          # (library code: test_consistency_gpu checks it)
    conn = T.construct_neighborhood(PH, PW)
    E, N = conn.shape[1], PH * PW
    views = [dict(energy=[], bound=[], iters=[]) for _ in range(2)]

    def solved(view, plan, dispmap_of):
        labels, en, lb, it = plan.result()
        view["labels"] = labels
        view["energy"].append(en); view["bound"].append(lb); view["iters"].append(it)
        view["map"] = dispmap_of(labels)

    def check_fill():
        for view, other, direction in ((views[0], views[1], 1), (views[1], views[0], -1)):
            view["status"], view["residual"] = lr_restate.lr_check(view["map"], other["map"], direction, 0.5)
        for view in views:
            view["filled"], view["source"] = lr_restate.lr_fill(view["map"], view["status"])

    by_index = lambda labels: disparities[labels.astype(np.int64) - 1].reshape(PW, PH).T
    plans = []
    for vol, view in zip(volumes, views):
        plan = TrwsPlan(1, PK, N, conn)
        plan.upload(PAIR_WEIGHT * (1.0 - vol), np.ones(E), PAIR_TOL, positions=disparities)
        plan.iterate(PAIR_ITERS, NEVER)
        solved(view, plan, by_index)
        plans.append(plan)
    check_fill()
    if refine_iters:
        for vol, view, plan in zip(volumes, views, plans):
            state = plan.save_state()
            zeroed = np.array(PAIR_WEIGHT * (1.0 - vol), order="F")
            zeroed[:, view["status"].T.reshape(-1) == 1] = 0.0
            plan.upload(zeroed, np.ones(E), PAIR_TOL, positions=disparities)
            plan.load_state(state)
            plan.iterate(refine_iters, NEVER)
            solved(view, plan, by_index)
        check_fill()
    for plan in plans:
        plan.close()
    for offsets in PAIR_LEVELS:
        for vol, view in zip(volumes, views):
            hwd = vol.reshape((PK, PH, PW), order="F").transpose(1, 2, 0)
            unary, q, qprim = R.band_inputs(hwd, disparities, PAIR_WEIGHT, view["map"], offsets, conn)
            if refine_iters:
                unary[:, view["status"].T.reshape(-1) == 1] = 0.0
            plan = TrwsPlan(1, len(offsets), N, conn)
            plan.upload(unary, np.ones(E), PAIR_TOL, q=q, qprim=qprim)
            plan.iterate(PAIR_ITERS, NEVER)
            base = view["map"]
            solved(view, plan, lambda labels: R.band_apply(base, labels, offsets))
            plan.close()
        check_fill()
    return views


@pytest.mark.parametrize("refine_iters", [0, 2])
def test_solve_pair_ncc_with_band_levels_equals_the_pipeline_by_hand(refine_iters, hip):
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc(small_pair(), disparities, 1, PAIR_WEIGHT, PAIR_TOL, PAIR_ITERS, NEVER, check_tol=0.5,
                             refine_iters=refine_iters, band_levels=PAIR_LEVELS)
    want = pipeline_by_hand(refine_iters)
    passes = (2 if refine_iters else 1) + len(PAIR_LEVELS)
    for view, ref in zip(got.views, want):
        assert (view.energy, view.lower_bound, view.iterations) == (ref["energy"], ref["bound"], ref["iters"])
        assert len(view.energy) == len(view.maps) == passes and view.maps[-1] is view.dispmap
        assert np.array_equal(view.labels, ref["labels"]) and same_bits(view.dispmap, ref["map"])
        assert np.array_equal(view.status, ref["status"]) and same(view.residual, ref["residual"])
        assert same(view.filled, ref["filled"]) and np.array_equal(view.source, ref["source"])


def test_solve_pair_ncc_without_band_levels_is_what_it_was(hip):
    disparities = np.arange(PK, dtype=np.float64)
    args = (small_pair(), disparities, 1, PAIR_WEIGHT, PAIR_TOL, PAIR_ITERS, NEVER)
    for refine_iters in (0, 2):
        a = hip.solve_pair_ncc(*args, check_tol=1.0, refine_iters=refine_iters)
        b = hip.solve_pair_ncc(*args, check_tol=1.0, refine_iters=refine_iters, band_levels=None)
        assert [k for k in a.times] == [k for k in b.times]
        for va, vb in zip(a.views, b.views):
            assert (va.energy, va.lower_bound, va.iterations) == (vb.energy, vb.lower_bound, vb.iterations)
            assert len(va.energy) == (2 if refine_iters else 1)
            for field in ("labels", "dispmap", "status", "source"):
                assert np.array_equal(getattr(va, field), getattr(vb, field)), field
            assert same(va.residual, vb.residual) and same(va.filled, vb.filled)
            assert np.array_equal(va.dispmap, np.rint(va.dispmap))


# ---------------------------------------------------------------- 8: the objects

def test_dispmap_ncc_refine_band_plain_and_mirrored(hip):
    from stereo_amd import band
    left, right = small_pair()
    disparities = np.arange(PK, dtype=np.float64)
    levels = [offsets_for(9), offsets_for(9) / 4.0]
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    m = dm.mirrored()
    for obj in (dm, m):
        obj.max_relgap = 0.0
        obj.set_disparity(np.rint(obj.current_dispmap()))
        before = obj.current_dispmap().copy()
        internal = before[:, ::-1] if obj._mirrored else before
        want = band.refine_band(obj.ncc, disparities, PAIR_WEIGHT, internal, 1, PAIR_TOL, levels, 3, 0.0)
        out = obj.refine_band(levels, maxiter=3)
        after = obj.current_dispmap()
        assert same_bits(after, want.dispmap[:, ::-1] if obj._mirrored else want.dispmap)
        assert out.energy == want.energy and len(out.energy) == 2
        assert np.isfinite(obj.energy())
    glob = object.__new__(hip.dispmap_globalstereo)
    with pytest.raises(hip.StereoHipError, match="dispmap_globalstereo"):
        glob.refine_band(levels)
