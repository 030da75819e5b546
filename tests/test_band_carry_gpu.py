"""-m gpu: messages carried from one band level or pyramid scale to the next.

The transfer kernel against the restated definition (tests/carry_restate.py) byte for byte; a level that starts from
carried messages against the restatement of minimize.cpp from those messages in phase 1 -- labels, energy, bound and
iteration count, nothing with a tolerance -- for the fronto-parallel band, the plane band and the two-member batch of a
pair; the level that repeats itself against the uninterrupted plan; carry=False against the call without the keyword;
bound <= optimum <= energy against enumeration; and the pyramid with carry='scales' against the same pipeline written
from the public pieces.  Every comparison is == / np.array_equal."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import band_restate as BR
import carry_restate as R
import first_principles as fp
import plane_band_restate as PR
import pyramid_restate
from band_restate import same_bits
from helpers import grid_conn
from test_band_gpu import small_pair, PH, PW, PK, PAIR_WEIGHT, PAIR_TOL, PAIR_ITERS

pytestmark = pytest.mark.gpu

NEVER = -1e300
UNARY_WEIGHT = 4.0
LEVEL_1 = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
LEVEL_2 = np.array([-0.25, 0.0, 0.25])
ITERS = 3


# ---------------------------------------------------------------- 1: the kernel

def uneven(K, seed):
    """K strictly ascending offsets with uneven, non-dyadic steps, around 0"""
    steps = np.random.default_rng([K, seed]).uniform(0.1, 0.9, size=K)
    v = np.cumsum(steps)
    return v - v[K // 2]


@functools.lru_cache(maxsize=None)
def transfer_case(H, W, K_old, K_new):
    """One transfer and its restated answer, built once, never changed."""
    from stereo_amd.carry import receivers
    conn0 = grid_conn(H, W).T
    N, E_new = H * W, conn0.shape[1]
    E_old = E_new + 3
    rng = np.random.default_rng([H, W, K_old, K_new])
    off_old, off_new = uneven(K_old, 1), uneven(K_new, 2)
    M_old = rng.normal(scale=5.0, size=(E_old, K_old))
    recv = receivers(N, conn0, 1)
    span = off_old[-1] - off_old[0] + off_new[-1] - off_new[0] + 1.0
    shift = rng.uniform(-0.6, 0.6, size=N) * (off_old[-1] - off_old[0] + 0.5)
    shift[1], shift[2], shift[3], shift[4] = np.nan, span, -span, 0.0          # not finite; past both ends; none
    src = rng.permutation(E_old)[:E_new].astype(np.int32)
    src[[0, 7, E_new - 1]] = -1
    src[5] = E_old                                                            # out of range: counted, zero row
    want, bad = R.carry(M_old, off_old, off_new, recv, shift, src, 0.5, 2.0)
    assert bad == 1 and not want[5].any() and not want[0].any()
    assert (want[np.isin(recv, [2, 3]) & (src >= 0) & (src < E_old)] == 0.0).all()      # flat rows: past an end
    c = dict(M_old=M_old, off_old=off_old, off_new=off_new, recv=recv, shift=shift, src=src, want=want)
    for a in c.values():
        a.setflags(write=False)
    return c


SIZES = [(5, 5), (9, 17), (64, 3), (3, 64), (1, 1), (33, 2), (100, 9), (600, 5)]


@pytest.mark.parametrize("shape", [(5, 6), (7, 9)], ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement(shape, hip):
    import torch
    from stereo_amd.carry import carry_messages, carry_messages_device
    H, W = shape
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    for K_old, K_new in SIZES:
        c = transfer_case(H, W, K_old, K_new)
        what = (H, W, K_old, K_new)
        got, bad = carry_messages(c["M_old"], c["off_old"], c["off_new"], c["recv"], c["shift"], c["src"], 0.5, 2.0)
        assert bad == 1 and got.tobytes() == c["want"].tobytes(), what
        args = (dev(c["M_old"]), c["off_old"], c["off_new"], dev(c["recv"]), dev(c["shift"]), dev(c["src"]), 0.5, 2.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        out, d_bad = carry_messages_device(*args, stream=side, check=False,
                                           bad=torch.full((1,), 77, dtype=torch.int32, device="cuda"))   # (the entry zeroes it)
        side.synchronize()
        assert int(d_bad.item()) == 1 and out.cpu().numpy().tobytes() == c["want"].tobytes(), what
        with pytest.raises(hip.StereoHipError, match="1 edge"):
            carry_messages_device(*args)
    # without edge_src: the same edges; stretch and gain 1
    c = transfer_case(H, W, 9, 17)
    M = c["M_old"][:c["recv"].shape[0]]
    want, _ = R.carry(M, c["off_old"], c["off_new"], c["recv"], c["shift"])
    got, bad = carry_messages(M, c["off_old"], c["off_new"], c["recv"], c["shift"])
    assert bad == 0 and got.tobytes() == want.tobytes()
    # a receiver outside the nodes: counted, zero row, the others untouched
    recv = c["recv"].copy()
    recv[3], recv[4] = -1, H * W
    got2, bad = carry_messages(M, c["off_old"], c["off_new"], recv, c["shift"])
    keep = np.ones(len(recv), bool)
    keep[[3, 4]] = False
    assert bad == 2 and not got2[[3, 4]].any() and got2[keep].tobytes() == want[keep].tobytes()


# ---------------------------------------------------------------- 2: a carried level against minimize.cpp restated

def trws_inputs(unary, q, qprim, conn):
    """K x N / K x E arrays as the restatement's dict"""
    return dict(unary=np.ascontiguousarray(unary.T), conn=np.ascontiguousarray(np.asarray(conn).T), q=np.ascontiguousarray(q.T),
                qprim=np.ascontiguousarray(qprim.T), alphas=np.ones(np.asarray(conn).shape[1]))


@functools.lru_cache(maxsize=None)
def band_case():
    from stereo_amd import terms as T
    H, W, D = 5, 6, 7
    c = dict(ncc=BR.volume(H, W, D, 31), disp=BR.disparities_for(D, False), conn=T.construct_neighborhood(H, W))
    c["base"] = BR.base_map(H, W, D, LEVEL_1[-1], 9)
    for a in c.values():
        a.setflags(write=False)
    return c


def level_one_by_hand(c, kernel, tol):
    """level 1 from the public pieces -> (the saved state, labels, the base level 2 stands around)"""
    from stereo_amd.band import BandProblem
    from stereo_amd.trws import TrwsPlan
    prob = BandProblem(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], c["conn"])
    plan = TrwsPlan(kernel, len(LEVEL_1), prob.N, prob.conn)
    prob.build(LEVEL_1, plan, tol)
    plan.iterate(ITERS, NEVER)
    state = plan.save_state()
    labels = plan.result()[0]
    plan.close()
    assert state.phase == 1
    return state, labels, prob.apply(labels)


@pytest.mark.parametrize("kernel", [1, 2])
def test_refine_band_carried_level_equals_the_restatement(kernel, hip, oracle):
    from stereo_amd.carry import receivers
    c = band_case()
    tol = 2.0
    got = hip.refine_band(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], kernel, tol, [LEVEL_1, LEVEL_2], ITERS, NEVER, carry=True)
    assert got.carried == [False, True]
    state, labels, base1 = level_one_by_hand(c, kernel, tol)
    assert np.array_equal(got.labels[0], labels) and same_bits(got.maps[0], base1)
    N = base1.size
    shift = (base1 - c["base"]).T.reshape(-1)
    assert shift.any()                                          # (level 1 moved something: the transfer has work to do)
    M, bad = R.carry(state.messages, LEVEL_1, LEVEL_2, receivers(N, c["conn"], 1), shift)
    assert bad == 0 and M.any()
    p = trws_inputs(*BR.band_inputs(c["ncc"], c["disp"], UNARY_WEIGHT, base1, LEVEL_2, c["conn"]), c["conn"])
    x, en, lb, _ = R.minimize(oracle, p, M, 1, ITERS, tol, kernel)
    print("carried band level, kernel %d: energy %r bound %r" % (kernel, en, lb))
    assert np.array_equal(got.labels[1], x + 1.0)
    assert (got.energy[1], got.lower_bound[1], got.iterations[1]) == (en, lb, float(ITERS))


def test_refine_plane_band_carried_level_equals_the_restatement(hip, oracle):
    from stereo_amd.carry import receivers
    from stereo_amd.plane_band import PlaneBandProblem
    from stereo_amd.trws import TrwsPlan
    c = band_case()
    H, W = c["base"].shape
    tol, kernel = 2.0, 1
    planes = PR.planes_through(c["base"], 6)
    source = hip.NccSource(c["ncc"], c["disp"], UNARY_WEIGHT, 0, (H, W))
    got = hip.refine_plane_band(source, planes, kernel, tol, [LEVEL_1, LEVEL_2], ITERS, NEVER, carry=True)
    assert got.carried == [False, True]
    prob = PlaneBandProblem(source, planes, c["conn"])
    plan = TrwsPlan(kernel, len(LEVEL_1), prob.N, prob.conn)
    prob.build(LEVEL_1, plan, tol)
    plan.iterate(ITERS, NEVER)
    state, labels = plan.save_state(), plan.result()[0]
    plan.close()
    planes1 = prob.apply(labels)
    assert np.array_equal(got.labels[0], labels) and same_bits(got.plane_maps[0], planes1)
    shift = LEVEL_1[labels.astype(np.int64) - 1]
    assert shift.any()
    M, bad = R.carry(state.messages, LEVEL_1, LEVEL_2, receivers(prob.N, c["conn"], 1), shift)
    p = trws_inputs(*hip.plane_band_inputs(source, planes1, LEVEL_2, c["conn"]), c["conn"])
    x, en, lb, _ = R.minimize(oracle, p, M, 1, ITERS, tol, kernel)
    assert bad == 0 and np.array_equal(got.labels[1], x + 1.0)
    assert (got.energy[1], got.lower_bound[1], got.iterations[1]) == (en, lb, float(ITERS))


def test_batch_members_take_carried_messages_as_single_plans_do(hip):
    """run_band_levels with carry: each view of the two-member batch equals refine_band(carry=True) on that view alone"""
    from stereo_amd import band, consistency
    from stereo_amd.consistency import PairResult, run_band_levels
    c = band_case()
    H, W = c["base"].shape
    other = dict(ncc=BR.volume(H, W, 7, 32), base=BR.base_map(H, W, 7, LEVEL_1[-1], 10))
    views = [(c["ncc"], c["base"]), (other["ncc"], other["base"])]
    problems = [band.BandProblem(ncc, c["disp"], UNARY_WEIGHT, base, c["conn"]) for ncc, base in views]
    out, plans = PairResult(), {}
    for view, (_, base) in zip(out.views, views):
        view.dispmap = base
    try:
        run_band_levels(out, problems, [LEVEL_1, LEVEL_2], plans, 1, c["conn"], 2.0, ITERS, NEVER, 1.0, carry=True)
    finally:
        for plan in (p for pair in plans.values() for p in pair):
            plan.close()
    for view, (ncc, base) in zip(out.views, views):
        solo = hip.refine_band(ncc, c["disp"], UNARY_WEIGHT, base, 1, 2.0, [LEVEL_1, LEVEL_2], ITERS, NEVER, carry=True)
        assert view.carried == [False, True] == solo.carried
        assert (view.energy, view.lower_bound, view.iterations) == (solo.energy, solo.lower_bound, solo.iterations)
        assert np.array_equal(view.labels, solo.labels[-1]) and same_bits(view.dispmap, solo.dispmap)
    assert all(st is not None and st.d_messages.shape == (problems[0].E, len(LEVEL_2)) for st in out.stages)


def chain_by_hand(prob, levels, kernel, tol):
    """band.run_levels restated through the problem's protocol with a fresh plan for every level; the hand-over is taken
    after apply(), where the loop takes it before"""
    from stereo_amd.trws import TrwsPlan
    rows, carry = [], None
    for level in levels:
        plan = TrwsPlan(kernel, prob.labels_of(level), prob.N, prob.conn)
        try:
            prob.build(level, plan, tol, carry=carry)
            plan.iterate(ITERS, NEVER)
            labels, en, lb, it = plan.result()
            moved = prob.apply(labels)
            carry = prob.carry_from(prob.leave(plan, labels))
        finally:
            plan.close()
        rows.append((labels, en, lb, it, moved))
    return rows


@pytest.mark.parametrize("carry", [False, True])
def test_levels_whose_K_repeats_equal_the_levels_chained_by_hand(carry, hip, monkeypatch):
    """K = 3, 5, 3 on a 5 x 7 image: the loop reuses the first plan for the third level (two plans are made, both are
    closed) and gives, bit for bit, what a fresh plan per level gives -- for the band and for the plane band, whose
    hand-over the loop takes before apply() and the chain by hand after it."""
    from stereo_amd import band, terms as T
    from stereo_amd.plane_band import PlaneBandProblem
    H, W, D = 5, 7, 6
    ncc, disp, conn = BR.volume(H, W, D, 41), BR.disparities_for(D, False), T.construct_neighborhood(H, W)
    base = BR.base_map(H, W, D, LEVEL_1[-1], 12)
    levels = [np.array([-0.5, 0.0, 0.5]), LEVEL_1, LEVEL_2]
    made = []

    class Counted(band.TrwsPlan):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
            self.closed = 0

        def close(self):
            self.closed += 1
            super().close()

    monkeypatch.setattr(band, "TrwsPlan", Counted)
    tol, kernel = 2.0, 1
    got = hip.refine_band(ncc, disp, UNARY_WEIGHT, base, kernel, tol, levels, ITERS, NEVER, carry=carry)
    assert [p.closed for p in made] == [1, 1]
    planes = PR.planes_through(base, 6)
    source = hip.NccSource(ncc, disp, UNARY_WEIGHT, 0, (H, W))
    got_planes = hip.refine_plane_band(source, planes, kernel, tol, levels, ITERS, NEVER, carry=carry)
    assert [p.closed for p in made] == [1, 1, 1, 1]
    monkeypatch.undo()
    wrap = (lambda prob: prob) if carry else NoCarry      # (without carry the loop's levels start from zero)
    want = chain_by_hand(wrap(band.BandProblem(ncc, disp, UNARY_WEIGHT, base, conn)), levels, kernel, tol)
    want_planes = chain_by_hand(wrap(PlaneBandProblem(source, planes, conn)), levels, kernel, tol)
    for res, rows, maps in ((got, want, got.maps), (got_planes, want_planes, got_planes.plane_maps)):
        assert res.carried == [False, carry, carry]
        for level, (labels, en, lb, it, moved) in enumerate(rows):
            assert np.array_equal(res.labels[level], labels) and same_bits(maps[level], moved), level
            assert (res.energy[level], res.lower_bound[level], res.iterations[level]) == (en, lb, it), level
    assert same_bits(got.dispmap, want[-1][4]) and same_bits(got_planes.planes, want_planes[-1][4])
    assert (got.stage is not None) == carry


class NoCarry:
    """a problem whose levels leave nothing"""

    def __init__(self, prob):
        self.prob = prob

    def __getattr__(self, name):
        return getattr(self.prob, name)

    def leave(self, plan, labels):
        return None


# ---------------------------------------------------------------- 3: the level that repeats itself

def test_a_repeated_level_goes_on_as_the_uninterrupted_plan(hip):
    """Offsets that repeat around a base that did not move: the problem is the same, the saved rows have minimum 0 and
    come back bit for bit, so the carried plan's next iterations are the uninterrupted plan's."""
    from stereo_amd.band import BandProblem
    from stereo_amd.trws import TrwsPlan
    c = band_case()
    prob = BandProblem(c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], c["conn"])
    a = TrwsPlan(1, len(LEVEL_1), prob.N, prob.conn)
    b = TrwsPlan(1, len(LEVEL_1), prob.N, prob.conn)
    try:
        prob.build(LEVEL_1, a, 2.0)
        a.iterate(ITERS, NEVER)
        stage = prob.stage(a)
        saved = a.save_state()
        assert (saved.messages.min(axis=1) == 0.0).all()
        moved = prob.apply(np.full(prob.N, 3.0))                # every label at offset 0
        assert same_bits(moved, c["base"])
        prob.build(LEVEL_1, b, 2.0, carry=prob.carry_from(stage))
        loaded = b.save_state()
        assert (loaded.phase, loaded.iterations, loaded.energy, loaded.lower_bound) == (1, 0, 0.0, 0.0)
        assert (loaded.labels == 2).all() and loaded.messages.tobytes() == saved.messages.tobytes()
        for _ in range(2):
            a.iterate(1, NEVER)
            b.iterate(1, NEVER)
            ra, rb = a.result(), b.result()
            assert np.array_equal(ra[0], rb[0]) and ra[1:3] == rb[1:3]
        assert (ra[3], rb[3]) == (ITERS + 2.0, 2.0)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 4: off is what it was

def same_result(a, b, maps):
    assert (a.energy, a.lower_bound, a.iterations, a.paths) == (b.energy, b.lower_bound, b.iterations, b.paths)
    assert len(a.labels) == len(b.labels) and all(np.array_equal(x, y) for x, y in zip(a.labels, b.labels))
    assert all(same_bits(x, y) for x, y in zip(getattr(a, maps), getattr(b, maps)))


def test_carry_false_is_the_call_without_the_keyword(hip):
    c = band_case()
    H, W = c["base"].shape
    args = (c["ncc"], c["disp"], UNARY_WEIGHT, c["base"], 1, 2.0, [LEVEL_1, LEVEL_2], ITERS, NEVER)
    a, b = hip.refine_band(*args), hip.refine_band(*args, carry=False)
    same_result(a, b, "maps")
    assert a.carried == b.carried == [False, False] and a.stage is None and b.stage is None
    source = hip.NccSource(c["ncc"], c["disp"], UNARY_WEIGHT, 0, (H, W))
    pargs = (source, PR.planes_through(c["base"], 6), 1, 2.0, [LEVEL_1, LEVEL_2], ITERS, NEVER)
    a, b = hip.refine_plane_band(*pargs), hip.refine_plane_band(*pargs, carry=False)
    same_result(a, b, "plane_maps")
    assert a.carried == b.carried == [False, False]
    disparities = np.arange(PK, dtype=np.float64)
    sargs = (small_pair(), disparities, 1, PAIR_WEIGHT, PAIR_TOL, PAIR_ITERS, NEVER)
    a = hip.solve_pair_ncc(*sargs, band_levels=[LEVEL_1, LEVEL_2])
    b = hip.solve_pair_ncc(*sargs, band_levels=[LEVEL_1, LEVEL_2], carry=False)
    on = hip.solve_pair_ncc(*sargs, band_levels=[LEVEL_1, LEVEL_2], carry=True)
    assert list(a.times) == list(b.times)
    for va, vb, von in zip(a.views, b.views, on.views):
        same_result(va, vb, "maps")
        assert np.array_equal(va.status, vb.status) and BR.same(va.filled, vb.filled)
        assert va.carried == vb.carried == [False] * 3 and von.carried == [False, True, True]
        assert (von.energy[0], von.lower_bound[0]) == (va.energy[0], va.lower_bound[0])       # the full-range pass is untouched
    a = hip.solve_pair_ncc_pyramid(*sargs[:5], 1, PAIR_ITERS, NEVER)
    b = hip.solve_pair_ncc_pyramid(*sargs[:5], 1, PAIR_ITERS, NEVER, carry="none")
    for l in range(2):
        for va, vb in zip(a.levels[l].views, b.levels[l].views):
            same_result(va, vb, "maps")
    with pytest.raises(hip.StereoHipError, match="carry must be"):
        hip.solve_pair_ncc_pyramid(*sargs[:5], 1, PAIR_ITERS, NEVER, carry=True)


# ---------------------------------------------------------------- 5: first principles

@pytest.mark.parametrize("kernel", [1, 2])
def test_a_carried_level_brackets_the_optimum(kernel, hip):
    """3 x 3, K = 3, the inputs dyadic (first_principles): the optimum by enumeration is exact.  The carried messages
    are a reparametrisation like any other, so at every iteration bound <= optimum <= energy, and the energy is the
    exact cost of the labelling reported with it."""
    from stereo_amd.carry import carry_messages, receivers
    from stereo_amd.trws import TrwsPlan
    rng = np.random.default_rng([3, 3, 3, kernel])
    pa = fp.dyadic_problem(rng, 3, 3, 3, False)
    pb = dict(pa, unary=fp._dyadic(rng, (9, 3), 4, 6), q=fp._dyadic(rng, pa["q"].shape, 8, 6), qprim=fp._dyadic(rng, pa["q"].shape, 8, 6))
    lam = 2.0
    conn0 = pa["conn"].T
    a = TrwsPlan(kernel, 3, 9, conn0)
    a.upload(pa["unary"].T, pa["alphas"], lam, q=pa["q"].T, qprim=pa["qprim"].T)
    a.iterate(2, NEVER)
    old = a.save_state()
    a.close()
    shift = np.array([0.0, 0.5, -0.5, 0.25, 0.0, -0.25, 1.0, -1.0, 0.5])
    M, bad = carry_messages(old.messages, [-0.5, 0.0, 0.5], [-0.25, 0.0, 0.25], receivers(9, conn0, 1), shift)
    assert bad == 0 and M.any()
    b = TrwsPlan(kernel, 3, 9, conn0)
    b.upload(pb["unary"].T, pb["alphas"], lam, q=pb["q"].T, qprim=pb["qprim"].T)
    st = b.save_state()
    st.phase, st.messages, st.labels = 1, M, np.ones(9, np.int32)
    b.load_state(st)
    opt, _ = fp.optimum_exhaustive(pb, kernel, lam)
    for t in range(1, 6):
        b.iterate(1, NEVER)
        labels, en, lb, it = b.result()
        print("kernel %d iteration %d: bound %r optimum %r energy %r" % (kernel, t, lb, opt, en))
        assert it == t and lb <= opt <= en
        assert fp.energy_exact(pb, kernel, lam, labels.astype(np.int64) - 1) == Fraction(float(en))
    b.close()


# ---------------------------------------------------------------- 6: the pyramid, carried across the scales

BAND = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])


def test_pyramid_carried_across_scales_equals_the_pipeline_from_the_public_pieces(hip):
    import torch
    from stereo_amd import consistency, terms as T
    from stereo_amd.band import BandProblem
    from stereo_amd.carry import Carry, receivers, scale_edge_map
    from stereo_amd.trws import TrwsPlan
    kernel = 1
    disparities = np.arange(PK, dtype=np.float64)
    got = hip.solve_pair_ncc_pyramid(small_pair(), disparities, kernel, PAIR_WEIGHT, PAIR_TOL, 1, PAIR_ITERS, NEVER,
                                     bands=[[BAND, LEVEL_2]], expand="nearest", carry="scales")
    levels_only = hip.solve_pair_ncc_pyramid(small_pair(), disparities, kernel, PAIR_WEIGHT, PAIR_TOL, 1, PAIR_ITERS, NEVER,
                                             bands=[[BAND, LEVEL_2]], expand="nearest", carry="levels")
    images = [list(small_pair())]
    images.append([pyramid_restate.reduce(im) for im in images[0]])
    Hc, Wc = images[1][0].shape[:2]
    assert (PH, PW, Hc, Wc) == (12, 16, 6, 8)
    disp_c = pyramid_restate.level_disparities(disparities, 1)
    tol_c, w_c = pyramid_restate.level_model(kernel, PAIR_TOL, 1)
    conn_c, conn_f = T.construct_neighborhood(Hc, Wc), T.construct_neighborhood(PH, PW)
    Nc, Nf = Hc * Wc, PH * PW
    i = np.arange(Nf)
    parent = ((i // PH) >> 1) * Hc + ((i % PH) >> 1)
    edge_src = scale_edge_map(conn_c, receivers(Nc, conn_c, 1), conn_f, receivers(Nf, conn_f, 1), parent)
    assert (edge_src >= 0).any() and (edge_src < 0).any()
    vols_c = consistency.pair_volumes(images[1], disp_c)
    vols_f = consistency.pair_volumes(images[0], disparities)
    for v, (view_c, view_f, view_l) in enumerate(zip(got.levels[1].views, got.levels[0].views, levels_only.levels[0].views)):
        plan = TrwsPlan(kernel, disp_c.shape[0], Nc, conn_c)
        plan.upload(PAIR_WEIGHT * (1.0 - vols_c[v]), w_c * np.ones(conn_c.shape[1]), tol_c, positions=disp_c)
        plan.iterate(PAIR_ITERS, NEVER)
        labels, en, lb, it = plan.result()
        coarse = plan.save_state()
        plan.close()
        assert np.array_equal(view_c.labels, labels) and (view_c.energy, view_c.lower_bound) == ([en], [lb])
        assert view_c.carried == [False]
        map_c = disp_c[labels.astype(np.int64) - 1].reshape(Wc, Hc).T
        expanded, _ = pyramid_restate.expand(map_c, (PH, PW), 0)
        assert same_bits(view_f.expanded, expanded)
        # level 0: the band from the coarse solve's messages (its base is zero, its offsets its disparities), then the
        # sub-pixel level from the band's
        prob = BandProblem(vols_f[v], disparities, PAIR_WEIGHT, expanded, conn_f, np.ones(conn_f.shape[1]), layout=1)
        carry = Carry(torch.from_numpy(coarse.messages).cuda(), disp_c, torch.from_numpy(0.5 * expanded.T.reshape(-1)).cuda(),
                      torch.from_numpy(edge_src).cuda(), stretch=0.5, gain=2.0)
        plan = TrwsPlan(kernel, len(BAND), Nf, conn_f)
        prob.build(BAND, plan, PAIR_TOL, carry=carry)
        plan.iterate(PAIR_ITERS, NEVER)
        labels, en, lb, it = plan.result()
        band_state = plan.save_state()
        plan.close()
        map_1 = prob.apply(labels)
        assert (view_f.energy[0], view_f.lower_bound[0], view_f.iterations[0]) == (en, lb, it) and same_bits(view_f.maps[0], map_1)
        carry = Carry(torch.from_numpy(band_state.messages).cuda(), BAND, torch.from_numpy((map_1 - expanded).T.reshape(-1)).cuda())
        plan = TrwsPlan(kernel, len(LEVEL_2), Nf, conn_f)
        prob.build(LEVEL_2, plan, PAIR_TOL, carry=carry)
        plan.iterate(PAIR_ITERS, NEVER)
        labels, en, lb, it = plan.result()
        plan.close()
        assert np.array_equal(view_f.labels, labels) and (view_f.energy[1], view_f.lower_bound[1], view_f.iterations[1]) == (en, lb, it)
        assert same_bits(view_f.dispmap, prob.apply(labels))
        assert view_f.carried == [True, True] and view_l.carried == [False, True]


# ---------------------------------------------------------------- 7: the objects

def test_the_objects_pass_carry_on(hip):
    """dispmap_ncc.refine_band / refine_plane_band / solve_pyramid with carry are the functions behind them with carry"""
    from stereo_amd import band, plane_band
    left, right = small_pair()
    disparities = np.arange(PK, dtype=np.float64)
    levels = [LEVEL_1, LEVEL_2]
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    dm.max_relgap = 0.0
    dm.set_disparity(np.rint(dm.current_dispmap()))
    before = dm.current_dispmap().copy()
    want = band.refine_band(dm.ncc, disparities, PAIR_WEIGHT, before, 1, PAIR_TOL, levels, 3, 0.0, carry=True)
    cold = band.refine_band(dm.ncc, disparities, PAIR_WEIGHT, before, 1, PAIR_TOL, levels, 3, 0.0)
    out = dm.refine_band(levels, maxiter=3, carry=True)
    assert out.carried == [False, True] and (out.energy, out.lower_bound) == (want.energy, want.lower_bound)
    assert same_bits(dm.current_dispmap(), want.dispmap)
    assert (out.energy[0], out.lower_bound[0]) == (cold.energy[0], cold.lower_bound[0]) and out.lower_bound[1] != cold.lower_bound[1]
    planes = dm.assignment.copy()
    source, _ = dm._plane_band_source()
    want = plane_band.refine_plane_band(source, planes, 1, PAIR_TOL, levels, 3, 0.0, alphas=dm.smooth_weights, conn=dm.neighborhood,
                                        d_min=dm.d_min, d_step=dm.d_step, carry=True)
    out = dm.refine_plane_band(levels, maxiter=3, carry=True)
    assert out.carried == [False, True] and (out.energy, out.lower_bound) == (want.energy, want.lower_bound)
    assert same_bits(out.planes, want.planes)
    # one view of the pyramid, carried across the scales: the pair pyramid's left view
    # (max_relgap NEVER: a stage that the gap criterion stops with a backward sweep ahead is not carried from)
    from stereo_amd import pyramid
    kw = dict(bands=[[BAND, LEVEL_2]], expand="nearest", carry="scales")
    pair = hip.solve_pair_ncc_pyramid(small_pair(), disparities, 1, PAIR_WEIGHT, PAIR_TOL, 1, PAIR_ITERS, NEVER, **kw)
    out = pyramid.solve_view_ncc_pyramid([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL, 1, PAIR_ITERS, NEVER, **kw)
    assert out.carried == [[True, True], [False]]
    for l in range(2):
        view = pair.levels[l].left
        assert (out.energy[l], out.lower_bound[l], out.iterations[l]) == (view.energy, view.lower_bound, view.iterations), l
        assert all(same_bits(a, b) for a, b in zip(out.maps[l], view.maps))
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    dm.max_relgap = 0.0
    want = pyramid.solve_view_ncc_pyramid([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL, 1, PAIR_ITERS, 0.0, **kw)
    out = dm.solve_pyramid(1, maxiter=PAIR_ITERS, **kw)
    assert (out.carried, out.energy, out.lower_bound, out.iterations) == (want.carried, want.energy, want.lower_bound, want.iterations)
    assert out.carried[0][1] is True and same_bits(out.dispmap, want.dispmap)
    with pytest.raises(hip.StereoHipError, match="carry must be"):
        dm.solve_pyramid(1, carry="all")
