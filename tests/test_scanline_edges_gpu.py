"""Scanline aggregation on per-edge positions on the device: stereo_scanline_edges_aggregate and its
device form against the NumPy restatement (tests/scanline_edges_restate.py, which test_scanline_edges_cpu holds against
first principles), bit for bit on S, labels and confidence -- a minimum of finite doubles does not depend on its order
and every other operation is one rounded add or product, so there is no tolerance to choose; the device edge table
against the host's; the energy terms against the host's; and whole chains against a TRW-S plan.

The shapes are the smallest at which the chain geometry (one pixel, one row, one column, a square of 2, both
orientations of a rectangle whose sides differ), the lane grouping (K around every power of two's group up to 64) and
the chain count (more chains than one wave carries, more waves than one) can each go wrong."""
import functools
import os

import numpy as np
import pytest

import first_principles as fp
import scanline_edges_restate as R
from test_scanline_edges_cpu import CHAIN_SEEDS, chain_instance, model

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 1), (1, 6), (6, 1), (2, 2), (5, 7), (7, 5)]
GROUPING = [1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 63, 64]
DIRECTION_LISTS = [[d] for d in R.DIRECTIONS_4] + [list(R.DIRECTIONS_4), [(1, 0), (0, -1), (1, 0)]]      # the last: a duplicate
TRWS_ITERATIONS = 5         # the cap of the chain test: a chain needs one iteration; the plan has to be there by this one


def two_per_pair(H, W):
    from stereo_amd import terms as T
    return T.construct_neighborhood(H, W)


def one_per_pair(H, W, rng):
    """dyadic_problem's graph: one edge per pair, permuted, about half flipped"""
    conn = fp.grid_edges(H, W)
    conn = conn[rng.permutation(len(conn))]
    flip = rng.random(len(conn)) < 0.5
    conn[flip] = conn[flip][:, ::-1]
    return np.ascontiguousarray(conn.T)


def problem(shape, K, seed, conn=None, dyadic=True):
    """(unary K x N, conn 2 x E, q, qprim K x E, alphas E): independent values per directed edge; positions repeat and
    are in no order within a row (the dyadic ones are drawn from 32 K values, the others are rounded normals)."""
    H, W = shape
    rng = np.random.default_rng([H, W, K, seed])
    conn = two_per_pair(H, W) if conn is None else conn
    E = conn.shape[1]
    if dyadic:
        unary = rng.integers(0, 4 << 6, size=(K, H * W)).astype(np.float64) / 64.0
        q = rng.integers(0, 8 << 2, size=(K, E)).astype(np.float64) / 4.0
        qprim = rng.integers(0, 8 << 2, size=(K, E)).astype(np.float64) / 4.0
        alphas = rng.choice(fp.ALPHAS, size=E)
    else:
        unary = rng.standard_normal((K, H * W)) * 3.0
        q, qprim = rng.standard_normal((K, E)) * 2.0, rng.standard_normal((K, E)) * 2.0
        alphas = rng.uniform(0.0, 2.0, size=E)
    return np.asfortranarray(unary), conn, np.asfortranarray(q), np.asfortranarray(qprim), alphas


def flat(a):
    import torch
    return torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()


def device_conn(conn):
    import torch
    return torch.from_numpy(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32).copy()).cuda()


def check(hip, shape, unary, conn, q, qprim, alphas, kernel, tol, directions=R.DIRECTIONS_4):
    """Host entry and device entry against the restatement; the inputs come back unmodified."""
    import torch
    from stereo_amd import scanline
    H, W = shape
    K, E = unary.shape[0], conn.shape[1]
    S, labels, conf = R.aggregate(unary, shape, conn, q, qprim, alphas, kernel, tol, directions)
    assert np.isfinite(S).all()
    what = (shape, K, E, kernel, tol, directions)
    before = [a.copy() for a in (unary, conn, q, qprim, alphas)]
    got = scanline.aggregate_edges(unary, shape, conn, q, qprim, alphas, kernel, tol, directions, want_volume=True)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels), what
    assert np.array_equal(got.volume, S), what
    assert got.dispmap is None and np.array_equal(got.confidence, conf), what
    assert scanline.aggregate_edges(unary, shape, conn, q, qprim, alphas, kernel, tol, directions).volume is None
    assert all(np.array_equal(a, b) for a, b in zip(before, (unary, conn, q, qprim, alphas)))
    d_in = [flat(unary), flat(q), flat(qprim), torch.from_numpy(np.array(alphas)).cuda()]
    d_conn = device_conn(conn)
    table, bad = scanline.edge_table_device(d_conn, E, shape)
    assert int(bad.item()) == 0 and np.array_equal(table.cpu().numpy(), scanline.edge_table(conn, shape)), what
    assert np.array_equal(table.cpu().numpy(), R.edge_table(conn, shape))
    dev = scanline.aggregate_edges_device(d_in[0], shape, table, d_in[1], d_in[2], d_in[3], kernel, tol, directions)
    torch.cuda.synchronize()
    assert np.array_equal(dev.volume.cpu().numpy().reshape(S.shape, order="F"), S), what
    assert dev.labels.dtype == torch.int32 and np.array_equal(dev.labels.cpu().numpy(), labels), what
    assert dev.dispmap is None and np.array_equal(dev.confidence.cpu().numpy().T, conf), what
    for t, a in zip(d_in, (unary, q, qprim, alphas)):
        assert np.array_equal(t.cpu().numpy(), np.asfortranarray(a).reshape(-1, order="F"))      # the inputs are only read
    return got


@pytest.mark.parametrize("shape", GEOMETRY, ids=lambda s: "%dx%d" % s)
def test_chain_geometry(shape, hip):
    p = problem(shape, 3, 0)
    for directions in DIRECTION_LISTS:
        check(hip, shape, *p, 1, 1.5, directions)


@pytest.mark.parametrize("K", GROUPING)
def test_lane_grouping(K, hip):
    for kernel, tol in ((1, 2.0), (2, 6.0)):
        check(hip, (3, 4), *problem((3, 4), K, kernel), kernel, tol)


def test_more_chains_than_one_workgroup(hip):
    check(hip, (37, 29), *problem((37, 29), 9, 7), 1, 2.0)


@pytest.mark.parametrize("kernel", [1, 2])
def test_graph_classes(kernel, hip):
    shape = (5, 7)
    rng = np.random.default_rng(kernel)
    two, one = two_per_pair(*shape), one_per_pair(*shape, rng)
    check(hip, shape, *problem(shape, 4, 1, two), kernel, 2.0)
    check(hip, shape, *problem(shape, 4, 2, one), kernel, 2.0)
    check(hip, shape, *problem(shape, 4, 3, two[:, rng.random(two.shape[1]) < 0.6]), kernel, 2.0)          # pairs with one edge or none
    check(hip, shape, *problem(shape, 4, 4, one[:, rng.random(one.shape[1]) < 0.5]), kernel, 2.0)          # pairs with no edge
    unary, conn, q, qprim, alphas = problem(shape, 4, 5, one)
    alphas[::3] = 0.0
    check(hip, shape, unary, conn, q, qprim, alphas, kernel, 2.0)
    unary, conn, q, qprim, alphas = problem(shape, 4, 6, np.zeros((2, 0), np.int64))                      # E = 0
    got = check(hip, shape, unary, conn, q, qprim, alphas, kernel, 2.0, [(0, 1), (1, 0), (0, 1)])
    # T = 0 everywhere and no chain is cut: L_r(p, k) = U(p, k) + the minima of the pixels before p, so S is R U plus one
    # constant per pixel (exact on these dyadic unaries) and the labels are the unary's
    rest = got.volume - ((unary + unary) + unary)
    assert np.array_equal(rest, np.tile(rest[:1], (4, 1))) and rest.max() > 0.0
    assert np.array_equal(got.labels, unary.argmin(axis=0) + 1)


def test_device_table_counts_a_bad_edge(hip):
    import torch
    from stereo_amd import StereoHipError, scanline
    shape = (5, 7)
    good = one_per_pair(*shape, np.random.default_rng(3))
    for edge in ((3, 3), (0, 35), (0, 2), (4, 5), tuple(good[:, 0])):         # loop, range, far, wrap-around, a slot taken twice
        conn = np.concatenate([good, np.array(edge).reshape(2, 1)], 1)
        table, bad = scanline.edge_table_device(device_conn(conn), conn.shape[1], shape, check=False)
        assert int(bad.item()) == 1
        assert np.array_equal(table.cpu().numpy(), scanline.edge_table(good, shape))            # nothing else is written
        with pytest.raises(StereoHipError, match="1 edge\\(s\\) that the 5 x 7 grid does not have"):
            scanline.edge_table_device(device_conn(conn), conn.shape[1], shape)
    table, bad = scanline.edge_table_device(torch.empty(0, dtype=torch.int32, device="cuda"), 0, shape)
    assert (table.cpu().numpy() == -1).all() and int(bad.item()) == 0


@pytest.mark.parametrize("kernel", [1, 2])
def test_truncation(kernel, hip):
    shape = (5, 7)
    p = problem(shape, 6, kernel)
    for tol in (0.0, 1e9, 2.0):                                         # cuts everything, never cuts, cuts inside the range
        check(hip, shape, *p, kernel, tol)


@functools.lru_cache(maxsize=None)
def teddy_level_inputs(kind):
    """The inputs of a K = 9 band level ('band') or candidate level ('candidates') on the 40 x 48 Teddy crop, straight
    from the device builders -> (unary, conn, q, qprim, alphas) on the host."""
    import torch
    from stereo_amd import band, candidates, terms as T
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_crop.npz"))
    im0, im1 = g["im0"][:40, :48].astype(np.float64), g["im1"][:40, :48].astype(np.float64)
    H, W = 40, 48
    disparities = np.arange(24, dtype=np.float64)
    ncc = T.ncc_volume(im0, im1, disparities, 2, layout=1)
    base = T.ncc_best_disp(ncc, disparities, 1, (H, W))
    base = np.where(np.isfinite(base), base, 0.0)
    conn = T.construct_neighborhood(H, W)
    if kind == "band":
        prob = band.BandProblem(ncc, disparities, 40.0, base, conn, layout=1)
        level = np.arange(-4, 5) / 4.0
    else:
        prob = candidates.CandidateProblem(ncc, disparities, 40.0, base, conn, layout=1)
        level = candidates.check_levels([dict(offsets=[0.0], taps=[(0, -1), (0, 1), (-1, 0), (1, 0)], sources=["base", "wta"])])[0]
    assert prob.labels_of(level) == 9
    prob.build(level, None, 2.0)
    torch.cuda.synchronize()
    E = conn.shape[1]
    out = (prob.d_unary.cpu().numpy().reshape(9, H * W, order="F"), conn, prob.d_q.cpu().numpy().reshape(9, E, order="F"),
           prob.d_qprim.cpu().numpy().reshape(9, E, order="F"), prob.d_alphas.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("kernel", [1, 2])
def test_data_that_is_not_dyadic(kernel, hip):
    """The bitwise claim does not rest on exact sums."""
    check(hip, (9, 11), *problem((9, 11), 17, kernel, dyadic=False), kernel, 0.7)
    for kind in ("band", "candidates"):
        p = teddy_level_inputs(kind)
        assert all(np.isfinite(a).all() for a in p)
        check(hip, (40, 48), *p, kernel, 2.0 if kernel == 1 else 5.0)


def test_a_plane_band_level_where_q_is_not_qprim(hip):
    import torch
    import band_restate as BR
    import plane_band_restate as PR
    from stereo_amd import plane_band, terms as T
    H, W, K = 5, 7, 5
    ncc = BR.volume(H, W, 6, 11)
    offsets = (np.arange(K, dtype=np.float64) - K // 2) / 4.0
    planes = PR.planes_through(BR.base_map(H, W, 6, offsets[-1], 5), 6, False)
    conn = T.construct_neighborhood(H, W)
    prob = plane_band.PlaneBandProblem(hip.NccSource(ncc, BR.disparities_for(6, False), 4.0), planes, conn)
    prob.build(offsets, None, 2.0)
    torch.cuda.synchronize()
    E = conn.shape[1]
    q, qprim = prob.d_q.cpu().numpy().reshape(K, E, order="F"), prob.d_qprim.cpu().numpy().reshape(K, E, order="F")
    assert not np.array_equal(q, qprim)
    for kernel in (1, 2):
        check(hip, (H, W), prob.d_unary.cpu().numpy().reshape(K, H * W, order="F"), conn, q, qprim, prob.d_alphas.cpu().numpy(), kernel, 2.0)


def test_ties_give_the_first_label_and_confidence_zero(hip):
    shape = (5, 7)
    _, conn, q, qprim, alphas = problem(shape, 5, 0)
    got = check(hip, shape, np.full((5, 35), 2.5, order="F"), conn, np.zeros_like(q), np.zeros_like(q), alphas, 1, 2.0)
    assert (got.labels == 1).all() and (got.confidence == 0.0).all()
    _, conn, q, qprim, alphas = problem(shape, 1, 0)
    got = check(hip, shape, np.full((1, 35), 2.5, order="F"), conn, q, qprim, alphas, 2, 2.0)
    assert (got.labels == 1).all() and np.isposinf(got.confidence).all()


def test_device_form_on_a_side_stream_into_given_tensors(hip):
    import torch
    from stereo_amd import StereoHipError, scanline
    shape, K = (7, 5), 9
    H, W = shape
    unary, conn, q, qprim, alphas = problem(shape, K, 21)
    S, labels, conf = R.aggregate(unary, shape, conn, q, qprim, alphas, 2, 4.0)
    d_unary, d_q, d_qprim, d_alphas = flat(unary), flat(q), flat(qprim), torch.from_numpy(np.array(alphas)).cuda()
    d_conn = device_conn(conn)
    out = dict(volume=torch.empty(K * H * W, dtype=torch.float64, device="cuda"), labels=torch.empty(H * W, dtype=torch.int32, device="cuda"),
               confidence=torch.empty((W, H), dtype=torch.float64, device="cuda"))
    table = torch.empty(4 * H * W, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    t, bad = scanline.edge_table_device(d_conn, conn.shape[1], shape, table=table, stream=side, check=False)
    r = scanline.aggregate_edges_device(d_unary, shape, table, d_q, d_qprim, d_alphas, 2, 4.0, stream=side, **out)
    side.synchronize()
    assert t is table and int(bad.item()) == 0
    assert r.volume is out["volume"] and r.labels is out["labels"] and r.confidence is out["confidence"]
    assert np.array_equal(r.volume.cpu().numpy().reshape(S.shape, order="F"), S) and np.array_equal(r.labels.cpu().numpy(), labels)
    assert np.array_equal(r.confidence.cpu().numpy().T, conf)
    with pytest.raises(StereoHipError, match="unary must hold"):
        scanline.aggregate_edges_device(d_unary[:-1].contiguous(), shape, table, d_q, d_qprim, d_alphas, 2, 4.0)
    with pytest.raises(StereoHipError, match="q must hold"):
        scanline.aggregate_edges_device(d_unary, shape, table, d_q[:-1].contiguous(), d_qprim, d_alphas, 2, 4.0)
    with pytest.raises(StereoHipError, match="the model has no diagonal edges"):
        scanline.aggregate_edges_device(d_unary, shape, table, d_q, d_qprim, d_alphas, 2, 4.0, [(1, 1)])
    with pytest.raises(StereoHipError, match="S must not be unary"):
        scanline.aggregate_edges_device(d_unary, shape, table, d_q, d_qprim, d_alphas, 2, 4.0, volume=d_unary)


@pytest.mark.parametrize("kernel", [1, 2])
def test_energy_terms(kernel, hip):
    import torch
    from stereo_amd import StereoHipError, scanline
    shape, K = (9, 11), 7
    N = 99
    for dyadic in (True, False):
        unary, conn, q, qprim, alphas = problem(shape, K, kernel, dyadic=dyadic)
        E = conn.shape[1]
        labels = np.random.default_rng([kernel, dyadic]).integers(1, K + 1, size=N).astype(np.int32)
        want, terms = scanline.model_energy_edges(unary, conn, q, qprim, alphas, kernel, 2.0, labels, want_terms=True)
        d = [flat(unary), device_conn(conn), flat(q), flat(qprim), torch.from_numpy(np.array(alphas)).cuda()]
        got, d_terms = scanline.level_energy_device(*d, kernel, 2.0, torch.from_numpy(labels).cuda())
        assert np.array_equal(d_terms.cpu().numpy(), terms)                       # every term has the definition's bits
        bound = (N + E) * 2.0 ** -52 * float(np.abs(terms).sum())                 # any-order summation of N + E terms
        print("energy kernel %d dyadic %s: device %r host %r bound %.3g" % (kernel, dyadic, got, want, bound))
        assert abs(got - want) <= bound
        if dyadic:
            assert got == want
    labels[5], labels[17] = 0, K + 1
    with pytest.raises(StereoHipError, match="2 label\\(s\\) outside 1 .. 7"):
        scanline.level_energy_device(*d, kernel, 2.0, torch.from_numpy(labels).cuda())
    _, d_terms = scanline.level_energy_device(*d, kernel, 2.0, torch.from_numpy(labels).cuda(), check=False)
    assert d_terms.cpu().numpy()[[5, 17]].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", sorted(CHAIN_SEEDS), ids=lambda s: "%dx%d" % s)
def test_whole_chains_against_trws(shape, kernel, hip):
    """On a chain TRW-S is exact dynamic programming (test_first_principles_gpu.py): within TRWS_ITERATIONS the plan's
    energy equals its bound, and the scanline labels of the seeds test_scanline_edges_cpu.py chose cost exactly that.
    Min-plus messages: the exact-message mode of the linear kernel meets first_principles.FINE_BITS' envelope ties on
    this coarse grid."""
    from stereo_amd import scanline
    from stereo_amd.trws import MESSAGES_MINPLUS, TrwsPlan
    H, W = shape
    directions = [(0, 1), (0, -1)] if H == 1 else [(1, 0), (-1, 0)]
    for seed in CHAIN_SEEDS[shape]:
        p = chain_instance(H, W, seed)
        unary, conn, q, qprim, alphas = model(p)
        got = scanline.aggregate_edges(unary, shape, conn, q, qprim, alphas, kernel, p["lam"], directions)
        assert (got.confidence > 0).all()
        mine = scanline.model_energy_edges(unary, conn, q, qprim, alphas, kernel, p["lam"], got.labels)
        plan = TrwsPlan(kernel, unary.shape[0], H * W, conn, MESSAGES_MINPLUS)
        try:
            plan.upload(unary, alphas, p["lam"], q=q, qprim=qprim)
            plan.iterate(TRWS_ITERATIONS, -1e300)
            _, energy, bound, _ = plan.result()
        finally:
            plan.close()
        print("chain %dx%d seed %d kernel %d: scanline %r trws energy %r bound %r" % (H, W, seed, kernel, mine, energy, bound))
        assert energy == bound, "the plan has not reached its bound in %d iterations" % TRWS_ITERATIONS
        assert mine == energy
