"""Scanline aggregation on per-edge positions without a device: the NumPy restatement
(tests/scanline_edges_restate.py) against the first-principles dynamic programme (first_principles.chain_dp, and a DP on
explicit step tables where a pixel pair carries two edges) with zero tolerance; the host edge table against the
restatement's, with its refusals; scanline.model_energy_edges against first_principles.energy_exact as a Fraction; and
every refusal of the C entries, which come before the device is looked for.

Why zero tolerance: the argument of test_scanline_cpu.py's docstring with one more add.  Unaries and per-edge positions
are multiples of 2^-6, alphas of 2^-2, tol is dyadic or never cuts (first_principles.LAMBDAS), so every edge cost is a
multiple of 2^-14 below 2^22, a step table entry is the sum of two of them, and every sum along a chain of at most 9
pixels (9 unaries, 16 edge costs) is exact in fp64 in whatever order it is formed."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import first_principles as fp
import scanline_edges_restate as R

K = 4
SHAPES = [(5, 7), (7, 5)]
OPPOSITE = [((0, 1), (0, -1)), ((1, 0), (-1, 0))]
# whole chains: seeds on which, for both kernels, the restatement's confidence is positive at every node and its labels
# are the optimum (asserted below; a seed that fails is replaced, not excused).  S = mm + U counts the unary twice, so
# its first minimum is the optimum on about one seed in six only (of seeds 0 .. 119: 26 on 1 x 9, 15 on 9 x 1; the
# confidence is positive on nearly all).  Shared with test_scanline_edges_gpu.py.
CHAIN_SEEDS = {(1, 9): (8, 10, 15), (9, 1): (8, 11, 29)}


def model(p):
    """first_principles' problem dict in the library's layout: unary K x N, conn 2 x E, q and qprim K x E, alphas."""
    return (np.asfortranarray(p["unary"].T), np.asfortranarray(p["conn"].T), np.asfortranarray(p["q"].T),
            np.asfortranarray(p["qprim"].T), np.ascontiguousarray(p["alphas"]))


def chain_pixels(shape, direction, y, x):
    """The pixel ids of the chain of `direction` through (y, x), from its first pixel up to and including (y, x)."""
    H, W = shape
    dy, dx = direction
    out = [(y, x)]
    while 0 <= out[-1][0] - dy < H and 0 <= out[-1][1] - dx < W:
        out.append((out[-1][0] - dy, out[-1][1] - dx))
    return [xx * H + yy for yy, xx in out[::-1]]


def edges_by_pair(conn):
    pairs = {}
    for e, (a, b) in enumerate(conn):
        pairs.setdefault((min(int(a), int(b)), max(int(a), int(b))), []).append(e)
    return pairs


def path_problem(p, pairs, ids):
    """The pixels `ids` cut out of the grid problem p (one edge per pair) as a path problem of first_principles: node s
    is ids[s]; the edge rows are taken by id, in the orientation the grid problem has them."""
    rows, conn = [], []
    for s in range(len(ids) - 1):
        (e,) = pairs[(min(ids[s], ids[s + 1]), max(ids[s], ids[s + 1]))]
        rows.append(e)
        conn.append((s, s + 1) if int(p["conn"][e][0]) == ids[s] else (s + 1, s))
    return dict(unary=p["unary"][ids], conn=np.array(conn, dtype=np.int64).reshape(-1, 2), q=p["q"][rows], qprim=p["qprim"][rows],
                alphas=p["alphas"][rows])


def dp_on_tables(unary, tables):
    """Min-sum dynamic programming on a path with explicit step tables: unary (n, K), tables[s][x_s, x_s+1].
    -> the min-marginals (n, K)."""
    n = unary.shape[0]
    F, B = np.zeros_like(unary), np.zeros_like(unary)
    F[0] = unary[0]
    for s in range(1, n):
        F[s] = unary[s] + (F[s - 1][:, None] + tables[s - 1]).min(axis=0)
    for s in range(n - 2, -1, -1):
        B[s] = (tables[s] + (unary[s + 1] + B[s + 1])[None, :]).min(axis=1)
    return F + B


def summed_tables(p, pairs, ids, kernel, lam):
    """tables[s][x_s, x_s+1] of the pixels `ids`: every edge of the pair, turned to that orientation, added up."""
    tables = []
    for s in range(len(ids) - 1):
        t = np.zeros((K, K))
        for e in pairs.get((min(ids[s], ids[s + 1]), max(ids[s], ids[s + 1])), []):
            c = fp.edge_table(p, kernel, lam, e)
            t = t + (c if int(p["conn"][e][0]) == ids[s] else c.T)
        tables.append(t)
    return tables


def half_chains_and_scanlines(p, shape, kernel, lam, min_marginals):
    """Every pixel, every direction: L_r(p, .) is the last node's min-marginals of the prefix that ends at the pixel;
    every opposite pair: L_r + L_-r - U are the whole scanline's.  min_marginals(ids) -> (n, K)."""
    H, W = shape
    unary, conn, q, qprim, alphas = model(p)
    table = R.edge_table(conn, shape)
    L = {d: R.direction_costs(unary, shape, table, q, qprim, alphas, kernel, lam, d) for d in R.DIRECTIONS_4}
    for d in R.DIRECTIONS_4:
        for x in range(W):
            for y in range(H):
                ids = chain_pixels(shape, d, y, x)
                mm = min_marginals(ids)
                assert np.array_equal(L[d][:, x * H + y], mm[len(ids) - 1]), (d, y, x, lam)
    for a, b in OPPOSITE:
        both = (L[a] + L[b]) - unary
        seen = np.zeros(H * W, bool)
        for x in range(W):
            for y in range(H):
                if len(chain_pixels(shape, b, y, x)) > 1:
                    continue                                # (y, x) is not the last pixel of a's chain
                ids = chain_pixels(shape, a, y, x)
                assert np.array_equal(both[:, ids].T, min_marginals(ids)), (a, y, x, lam)
                seen[ids] = True
        assert seen.all()


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_one_edge_per_pair_equals_first_principles(shape, kernel):
    H, W = shape
    for seed, lam in enumerate(fp.LAMBDAS):
        p = fp.dyadic_problem(np.random.default_rng([H, W, kernel, seed]), H, W, K, shared=False)
        pairs = edges_by_pair(p["conn"])
        half_chains_and_scanlines(p, shape, kernel, lam, lambda ids: fp.chain_dp(path_problem(p, pairs, ids), kernel, lam)[1])


def two_per_pair_problem(rng, H, W):
    """construct_neighborhood's graph (two edges per pair, one in each orientation) with independent dyadic q, qprim and
    alphas per directed edge, as a first_principles problem dict."""
    ids = np.arange(H * W).reshape(W, H).T
    s1, f1 = ids[:-1, :].T.ravel(), ids[1:, :].T.ravel()
    s2, f2 = ids[:, :-1].T.ravel(), ids[:, 1:].T.ravel()
    conn = np.stack([np.concatenate([s1, f1, s2, f2]), np.concatenate([f1, s1, f2, s2])], 1).astype(np.int64)
    E = conn.shape[0]
    return dict(unary=fp._dyadic(rng, (H * W, K), 4, 6), conn=conn, q=fp._dyadic(rng, (E, K), 8, 6),
                qprim=fp._dyadic(rng, (E, K), 8, 6), alphas=rng.choice(fp.ALPHAS, size=E), H=H, W=W)


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_two_edges_per_pair_equal_the_dp_on_summed_tables(shape, kernel):
    H, W = shape
    for seed, lam in enumerate(fp.LAMBDAS):
        p = two_per_pair_problem(np.random.default_rng([H, W, kernel, seed, 2]), H, W)
        pairs = edges_by_pair(p["conn"])
        assert all(len(v) == 2 for v in pairs.values())
        half_chains_and_scanlines(p, shape, kernel, lam,
                                  lambda ids: dp_on_tables(p["unary"][ids], summed_tables(p, pairs, ids, kernel, lam)))


def test_the_dp_on_tables_is_chain_dp_where_both_apply():
    p = fp.dyadic_problem(np.random.default_rng(5), 1, 7, K, shared=False)
    pairs = edges_by_pair(p["conn"])
    ids = list(range(7))
    for kernel in (1, 2):
        _, mm = fp.chain_dp(p, kernel, 2.0)
        assert np.array_equal(dp_on_tables(p["unary"][ids], summed_tables(p, pairs, ids, kernel, 2.0)), mm)


def chain_instance(H, W, seed):
    return fp.problem(H, W, K, False, seed)


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", sorted(CHAIN_SEEDS), ids=lambda s: "%dx%d" % s)
def test_whole_chains(shape, kernel):
    """The graph is a chain: S - U of the two directions along it are the problem's min-marginals, so min (S - U) is
    OPT at every node; a unique minimum of S - U at every node is the unique optimum.  S itself counts U twice; that its
    first minimum is the optimum as well is a property of the chosen seeds, asserted with their positive confidence."""
    H, W = shape
    directions = [(0, 1), (0, -1)] if H == 1 else [(1, 0), (-1, 0)]
    for seed in CHAIN_SEEDS[shape]:
        p = chain_instance(H, W, seed)
        lam = p["lam"]
        unary, conn, q, qprim, alphas = model(p)
        opt, mm = fp.chain_dp(p, kernel, lam)
        S, labels, conf = R.aggregate(unary, shape, conn, q, qprim, alphas, kernel, lam, directions)
        assert np.array_equal((S - unary).T, mm)
        assert ((S - unary).min(axis=0) == opt).all()
        assert (conf > 0).all(), (shape, seed, kernel)
        assert fp.energy_exact(p, kernel, lam, labels - 1) == Fraction(opt), (shape, seed, kernel)
        rel = np.sort(mm - opt, axis=1)
        if (rel[:, 1] > 0).all():
            assert fp.energy_exact(p, kernel, lam, mm.argmin(axis=1)) == Fraction(opt)


# ---------------------------------------------------------------- the host table

def host_table(conn, shape):
    from stereo_amd import scanline
    return scanline.edge_table(conn, shape)


def grid_conn(H, W):
    from stereo_amd import terms as T
    return T.construct_neighborhood(H, W)


@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (6, 1), (2, 2), (5, 7)], ids=lambda s: "%dx%d" % s)
def test_host_table_equals_the_restatement(shape):
    H, W = shape
    rng = np.random.default_rng([H, W])
    two = grid_conn(H, W)
    one = fp.dyadic_problem(rng, H, W, 2, shared=False)["conn"].T
    graphs = [two, one, two[:, rng.random(two.shape[1]) < 0.6], one[:, rng.random(one.shape[1]) < 0.6], np.zeros((2, 0), np.int64)]
    for conn in graphs:
        got = host_table(conn, shape)
        assert got.dtype == np.int32 and got.shape == (4 * H * W,)
        assert np.array_equal(got, R.edge_table(conn, shape))
        assert np.count_nonzero(got >= 0) == conn.shape[1]


TABLE_REFUSALS = [
    ([(3, 3)], "edge 0 \\(3, 3\\) is a self-loop"),
    ([(0, 1), (34, 35)], "edge 1 \\(34, 35\\) has an endpoint outside 0 .. 34"),
    ([(0, 1), (4294967295, 0)], "edge 1 .* has an endpoint outside"),
    ([(0, 2)], "edge 0 \\(0, 2\\) does not join two 4-neighbours of the 5 x 7 grid"),
    ([(0, 6)], "edge 0 \\(0, 6\\) does not join two 4-neighbours"),
    ([(0, 1), (4, 5)], "edge 1 \\(4, 5\\) does not join two 4-neighbours"),           # last row of column 0, first of column 1
    ([(5, 4)], "edge 0 \\(5, 4\\) does not join two 4-neighbours"),
    ([(0, 1), (1, 0), (0, 5), (0, 1)], "edge 3 \\(0, 1\\) is the second edge .* \\(edge 0 is the first\\)"),
    ([(5, 0), (1, 0), (5, 0)], "edge 2 \\(5, 0\\) is the second edge .* \\(edge 0 is the first\\)"),
]


@pytest.mark.parametrize("edges,message", TABLE_REFUSALS, ids=[str(i) for i in range(len(TABLE_REFUSALS))])
def test_host_table_refusals_name_the_edge(edges, message):
    from stereo_amd import StereoHipError
    conn = np.array(edges, dtype=np.int64).T
    with pytest.raises(StereoHipError, match="^stereo_scanline_edges_table: " + message):
        host_table(conn, (5, 7))
    with pytest.raises(ValueError, match="edge %d" % (len(edges) - 1)):
        R.edge_table(conn, (5, 7))


def test_a_one_row_grid_has_horizontal_neighbours_only():
    assert np.array_equal(host_table(np.array([[0, 2], [1, 1]]), (1, 3)), R.edge_table(np.array([[0, 2], [1, 1]]), (1, 3)))
    assert host_table(np.array([[0, 2], [1, 1]]), (1, 3)).reshape(3, 2, 2)[:, 0].max() == -1        # no column pair


@pytest.mark.parametrize("kernel", [1, 2])
def test_model_energy_edges_equals_the_exact_energy(kernel):
    from stereo_amd import scanline
    for seed in range(6):
        rng = np.random.default_rng([kernel, seed])
        p = fp.dyadic_problem(rng, 4, 5, 5, shared=False)
        x = rng.integers(0, 5, size=20)
        unary, conn, q, qprim, alphas = model(p)
        got, terms = scanline.model_energy_edges(unary, conn, q, qprim, alphas, kernel, p["lam"], x + 1, want_terms=True)
        assert Fraction(got) == fp.energy_exact(p, kernel, p["lam"], x)
        assert terms.shape == (20 + conn.shape[1],) and sum(Fraction(float(t)) for t in terms) == Fraction(got)
        assert scanline.model_energy_edges(unary, conn, q, qprim, alphas, kernel, p["lam"], x + 1) == got


# ---------------------------------------------------------------- refusals, before the device is looked for

def ptr(keep, values, dtype, null=False):
    if null:
        return None
    v = np.array(values, dtype=dtype)
    keep.append(v)
    return v.ctypes.data_as(C.c_void_p)


BASE = dict(H=2, W=3, K=2, E=2, kernel=1, tol=1.0, R=2, directions=[1, 0, 0, -1], null=())


def call_aggregate(device, **change):
    """stereo_scanline_edges_aggregate (_device) on small host arrays with one argument changed -> (rc, message)."""
    from stereo_amd import _lib
    a = dict(BASE, unary=[0.0] * 12, q=[0.0, 1.0] * 2, qprim=[0.0, 1.0] * 2, alphas=[1.0, 0.5], conn=[0, 1, 2, 0])
    a.update(change)
    keep, null = [], a["null"]
    unary = ptr(keep, a["unary"], np.float64, "unary" in null)
    edges = ptr(keep, [-1] * 24, np.int32, "table" in null) if device else ptr(keep, a["conn"], np.uint32, "conn" in null)
    S = unary if a.get("in_place") else ptr(keep, [0.0] * 12, np.float64, "S" in null)
    args = [C.c_int(a["kernel"]), unary, C.c_int(a["H"]), C.c_int(a["W"]), C.c_int(a["K"]), C.c_int64(a["E"]), edges,
            ptr(keep, a["q"], np.float64, "q" in null), ptr(keep, a["qprim"], np.float64, "qprim" in null),
            ptr(keep, a["alphas"], np.float64, "alphas" in null), C.c_double(a["tol"]),
            ptr(keep, a["directions"], np.int32, "directions" in null), C.c_int(a["R"]), S,
            ptr(keep, [0] * 6, np.int32, "labels" in null), ptr(keep, [0.0] * 6, np.float64, "confidence" in null)]
    err = _lib.errbuf()
    L = _lib.lib()
    if device:
        rc = L.stereo_scanline_edges_aggregate_device(*args, None, err, C.c_size_t(len(err)))
    else:
        rc = L.stereo_scanline_edges_aggregate(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


GRID_REFUSALS = [
    (dict(H=0), "H and W must be at least 1"),
    (dict(W=-1), "H and W must be at least 1"),
    (dict(H=1 << 16, W=1 << 15), "below 2\\^31"),
]
MODEL_REFUSALS = [
    (dict(K=0), "K must be 1 .. 64"),
    (dict(K=65), "K must be 1 .. 64"),
    (dict(kernel=0), "kernel must be 1"),
    (dict(kernel=3), "kernel must be 1"),
    (dict(tol=-1.0), "tol must be non-negative"),
    (dict(tol=float("nan")), "tol must be non-negative"),
]
EDGE_COUNT_REFUSALS = [(dict(E=-1), "E must be 0 .. 2\\^31 - 1"), (dict(E=1 << 31), "E must be 0 .. 2\\^31 - 1")]
AGGREGATE_REFUSALS = GRID_REFUSALS + MODEL_REFUSALS + EDGE_COUNT_REFUSALS + [
    (dict(R=0), "R .* must be 1 .. 8"),
    (dict(R=9), "R .* must be 1 .. 8"),
    (dict(directions=[1, 0, 0, 0]), "a direction must be"),
    (dict(directions=[2, 0, 0, 1]), "a direction must be"),
    (dict(directions=[1, 0, 0, -2]), "a direction must be"),
    (dict(directions=[1, 0, 1, 1]), "the model has no diagonal edges \\(direction 1 is \\(1, 1\\)\\)"),
    (dict(directions=[-1, 1, 1, 0]), "the model has no diagonal edges \\(direction 0 is \\(-1, 1\\)\\)"),
    (dict(null=("unary",)), "must not be NULL"),
    (dict(null=("directions",)), "must not be NULL"),
    (dict(null=("labels",)), "must not be NULL"),
    (dict(null=("q",)), "must not be NULL"),
    (dict(null=("qprim",)), "must not be NULL"),
    (dict(null=("alphas",)), "must not be NULL"),
    (dict(in_place=True), "S must not be unary"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,message", AGGREGATE_REFUSALS, ids=[str(i) for i in range(len(AGGREGATE_REFUSALS))])
def test_refusals_of_both_aggregate_entries(change, message, device):
    import re
    rc, text = call_aggregate(device, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_scanline_edges_aggregate_device:" if device else "stereo_scanline_edges_aggregate:")
    assert "no HIP device" not in text


def test_refusals_of_one_aggregate_entry_only():
    rc, text = call_aggregate(True, null=("S",))
    assert rc != 0 and text.startswith("stereo_scanline_edges_aggregate_device:") and "S and labels must not be NULL" in text
    rc, text = call_aggregate(True, null=("table",))
    assert rc != 0 and "table, q, qprim and alphas must not be NULL" in text
    rc, text = call_aggregate(True, null=("table",), E=0)
    assert rc != 0 and "table, q, qprim and alphas must not be NULL" in text and "no HIP device" not in text
    rc, text = call_aggregate(False, null=("conn",))
    assert rc != 0 and "conn, q, qprim and alphas must not be NULL" in text
    for change, message in ((dict(unary=[0.0] * 11 + [float("nan")]), "unary must be finite"),
                            (dict(unary=[float("inf")] + [0.0] * 11), "unary must be finite"),
                            (dict(q=[0.0, 1.0, float("-inf"), 0.0]), "q and qprim must be finite"),
                            (dict(qprim=[float("nan"), 1.0, 0.0, 0.0]), "q and qprim must be finite"),
                            (dict(alphas=[1.0, -0.5]), "an alpha must be finite and non-negative \\(edge 1\\)"),
                            (dict(alphas=[float("inf"), 1.0]), "an alpha must be finite and non-negative \\(edge 0\\)"),
                            (dict(alphas=[1.0, float("nan")]), "an alpha must be finite and non-negative"),
                            (dict(conn=[0, 1, 2, 2]), "edge 1 \\(2, 2\\) is a self-loop"),
                            (dict(conn=[0, 1, 2, 6]), "edge 1 \\(2, 6\\) has an endpoint outside 0 .. 5"),
                            (dict(conn=[0, 1, 1, 2]), "edge 1 \\(1, 2\\) does not join two 4-neighbours"),
                            (dict(conn=[0, 1, 0, 1]), "edge 1 \\(0, 1\\) is the second edge")):
        import re
        rc, text = call_aggregate(False, **change)
        assert rc != 0 and re.search(message, text) and "no HIP device" not in text, text
        assert text.startswith("stereo_scanline_edges_aggregate:")


def call_table(device, **change):
    from stereo_amd import _lib
    a = dict(H=2, W=3, E=2, conn=[0, 1, 2, 0], null=())
    a.update(change)
    keep = []
    args = [ptr(keep, a["conn"], np.uint32, "conn" in a["null"]), C.c_int64(a["E"]), C.c_int(a["H"]), C.c_int(a["W"]),
            ptr(keep, [0] * 24, np.int32, "table" in a["null"])]
    err = _lib.errbuf()
    if device:
        rc = _lib.lib().stereo_scanline_edges_table_device(*args, ptr(keep, [0], np.int32, "bad" in a["null"]), None, err,
                                                           C.c_size_t(len(err)))
    else:
        rc = _lib.lib().stereo_scanline_edges_table(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


TABLE_ARG_REFUSALS = GRID_REFUSALS + EDGE_COUNT_REFUSALS + [(dict(null=("conn",)), "must not be NULL"),
                                                            (dict(null=("table",)), "must not be NULL")]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,message", TABLE_ARG_REFUSALS, ids=[str(i) for i in range(len(TABLE_ARG_REFUSALS))])
def test_refusals_of_both_table_entries(change, message, device):
    import re
    rc, text = call_table(device, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_scanline_edges_table_device:" if device else "stereo_scanline_edges_table:")
    assert "no HIP device" not in text


def test_refusals_of_the_device_table_only_and_the_empty_graph():
    rc, text = call_table(True, null=("bad",))
    assert rc != 0 and "conn, table and bad must not be NULL" in text and "no HIP device" not in text
    rc, text = call_table(False, E=0, null=("conn",))
    assert rc == 0, text


def call_energy(**change):
    from stereo_amd import _lib
    a = dict(BASE, N=6, null=())
    a.update(change)
    keep, null = [], a["null"]
    err = _lib.errbuf()
    rc = _lib.lib().stereo_scanline_edges_energy_device(
        C.c_int(a["kernel"]), ptr(keep, [0.0] * 12, np.float64, "unary" in null), C.c_int(a["K"]), C.c_int64(a["N"]), C.c_int64(a["E"]),
        ptr(keep, [0, 1, 2, 0], np.uint32, "conn" in null), ptr(keep, [0.0] * 4, np.float64, "q" in null),
        ptr(keep, [0.0] * 4, np.float64, "qprim" in null), ptr(keep, [1.0, 1.0], np.float64, "alphas" in null), C.c_double(a["tol"]),
        ptr(keep, [1] * 6, np.int32, "labels" in null), ptr(keep, [0.0] * 8, np.float64, "terms" in null),
        ptr(keep, [0], np.int32, "bad" in null), None, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


ENERGY_REFUSALS = MODEL_REFUSALS + EDGE_COUNT_REFUSALS + [
    (dict(N=0), "N must be 1 .. 2\\^31 - 1"),
    (dict(N=1 << 31), "N must be 1 .. 2\\^31 - 1"),
] + [(dict(null=(name,)), "must not be NULL") for name in ("unary", "labels", "terms", "bad", "conn", "q", "qprim", "alphas")]


@pytest.mark.parametrize("change,message", ENERGY_REFUSALS, ids=[str(i) for i in range(len(ENERGY_REFUSALS))])
def test_refusals_of_the_energy_entry(change, message):
    import re
    rc, text = call_energy(**change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_scanline_edges_energy_device:") and "no HIP device" not in text


def test_refusals_reach_python_as_StereoHipError():
    from stereo_amd import StereoHipError, scanline
    u, q, a = np.zeros((2, 6)), np.zeros((2, 2)), np.ones(2)
    conn = np.array([[0, 2], [1, 0]])
    assert scanline.edges_max_labels() == 64
    with pytest.raises(StereoHipError, match="the model has no diagonal edges"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, a, 1, 1.0, [(1, 1)])
    with pytest.raises(StereoHipError, match="a direction must be"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, a, 1, 1.0, [(0, 0)])
    with pytest.raises(StereoHipError, match="kernel must be 1"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, a, 5, 1.0)
    with pytest.raises(StereoHipError, match="tol must be non-negative"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, a, 1, -1.0)
    with pytest.raises(StereoHipError, match="R .* must be 1 .. 8"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, a, 1, 1.0, scanline.DIRECTIONS_4 * 2 + ((0, 1),))
    with pytest.raises(StereoHipError, match="K must be 1 .. 64"):
        scanline.aggregate_edges(np.zeros((65, 6)), (2, 3), conn, np.zeros((65, 2)), np.zeros((65, 2)), a, 1, 1.0)
    with pytest.raises(StereoHipError, match="unary must be finite"):
        scanline.aggregate_edges(np.full((2, 6), np.nan), (2, 3), conn, q, q, a, 1, 1.0)
    with pytest.raises(StereoHipError, match="an alpha must be finite and non-negative"):
        scanline.aggregate_edges(u, (2, 3), conn, q, q, -a, 1, 1.0)
    with pytest.raises(StereoHipError, match="edge 1 \\(2, 1\\) does not join"):
        scanline.aggregate_edges(u, (2, 3), np.array([[0, 2], [1, 1]]), q, q, a, 1, 1.0)
    with pytest.raises(StereoHipError, match="unary must be K x N"):
        scanline.aggregate_edges(u, (3, 3), conn, q, q, a, 1, 1.0)
    with pytest.raises(StereoHipError, match="q and qprim must be K x E"):
        scanline.aggregate_edges(u, (2, 3), conn, np.zeros((2, 3)), q, a, 1, 1.0)
    with pytest.raises(StereoHipError, match="is a self-loop"):
        scanline.edge_table(np.array([[1], [1]]), (2, 3))
    with pytest.raises(StereoHipError, match="labels must be 1 .. 2"):
        scanline.model_energy_edges(u, conn, q, q, a, 1, 1.0, [1, 2, 3, 1, 1, 1])
    with pytest.raises(StereoHipError, match="kernel must be 1 or 2"):
        scanline.model_energy_edges(u, conn, q, q, a, 0, 1.0, [1] * 6)


def test_a_scanline_level_has_nothing_to_carry():
    """Refused before any device work: no problem object is made, none is touched."""
    import stereo_amd as hip
    from stereo_amd import StereoHipError, band, consistency
    out = band.LevelsResult()
    with pytest.raises(StereoHipError, match="solver='scanline' has no messages to carry"):
        band.run_levels(None, [np.zeros(1)], out, 1, 1.0, 5, 0.0, carry=True, solver="scanline")
    with pytest.raises(StereoHipError, match="solver='scanline' has no messages to carry"):
        band.run_levels(None, [np.zeros(1)], out, 1, 1.0, 5, 0.0, start=object(), solver="scanline")
    with pytest.raises(StereoHipError, match="solver must be 'trws' or 'scanline'"):
        band.run_levels(None, [np.zeros(1)], out, 1, 1.0, 5, 0.0, solver="sgm")
    with pytest.raises(StereoHipError, match="solver='scanline' has no messages to carry"):
        hip.refine_band(np.zeros((2, 3, 2)), [0.0, 1.0], 1.0, np.zeros((2, 3)), 1, 1.0, [[0.0]], 5, 0.0, carry=True, solver="scanline")
    with pytest.raises(StereoHipError, match="solver='scanline' has no messages to carry"):
        hip.refine_plane_band(None, np.zeros((4, 6)), 1, 1.0, [[0.0]], 5, 0.0, carry=True, solver="scanline")
    with pytest.raises(StereoHipError, match="solver='scanline' has no messages to carry"):
        consistency.run_band_levels(consistency.PairResult(), [None, None], [np.zeros(1)], {}, 1, None, 1.0, 5, 0.0, 1.0, carry=True,
                                    solver="scanline")
    assert out.maps == [] and out.energy == []
