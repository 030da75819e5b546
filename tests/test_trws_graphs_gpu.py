"""-m gpu: TRW-S parity OFF the image grid.  The graph families of graph_families.py -- single-edged, shuffled,
renumbered, masked and thinned grids, rings, chains, trees, random sparse graphs with and without parallel edges --
through every sweep kernel family against the CPU oracle: labels, energy, lower bound and iteration count bit for
bit, with plan.path() asserted, so that a graph which silently left the descriptor-driven kernels (or silently stayed
on them) fails.  The families are spread over the cases; tests/test_schedule_graphs_cpu.py shows for every graph run
here that the host's protocol model terminates on its schedule, and a graph on which it does not (DEADLOCK8) is
asserted to take the generic kernel.

A protocol give-up surfaces as a StereoHipError after STEREO_HIP_TRWS_SPIN_SECONDS, set to a few seconds here."""
import numpy as np
import pytest

import graph_families as gf

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG",
       "STEREO_HIP_TRWS_MESSAGES", "STEREO_HIP_TRWS_CACHE")

SMALL = {f[0]: f[1:] for f in gf.fast_families(1)}
BIG = {f[0]: f[1:] for f in gf.fast_families(2)}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STEREO_HIP_TRWS_SPIN_SECONDS", "3")


def _problem(N, conn, K, seed, integer=False, shared=None, unit_alphas=False):
    """dict(unary (N,K), conn, q, qprim (E,K), alphas (E,), pos): per-edge positions, or one shared ascending vector
    (shared = 'grid' | 'irregular')."""
    rng = np.random.default_rng(seed)
    E = len(conn)
    unary = rng.uniform(0, 40, size=(N, K))
    alphas = rng.uniform(0.5, 2.0, size=E)
    pos = None
    if shared is not None:
        pos = np.arange(K, dtype=np.float64) if shared == "grid" else np.cumsum(rng.uniform(0.05, 2.0, size=K))
        q = np.tile(pos, (E, 1)); qprim = q.copy()
    else:
        slope = rng.uniform(0.5, 1.5, size=(E, 1))
        q = np.arange(K)[None, :] * slope + rng.normal(size=(E, K)) * 1.5
        qprim = np.arange(K)[None, :] * slope + rng.normal(size=(E, K)) * 1.5
    if integer:   # tie-heavy
        unary = np.round(unary / 4)
        alphas = np.maximum(np.round(alphas), 1.0)
        if shared is None:
            q, qprim = np.round(q), np.round(qprim)
    alphas[rng.random(E) < 0.05] = 0.0
    if unit_alphas:
        alphas = np.ones(E)
    return dict(unary=unary, conn=conn, q=q, qprim=qprim, alphas=alphas, pos=pos)


def _run(oracle, kernel, p, tol, iters, path, mode=0, ordering=0, minplus=False):
    """One plan against the oracle; returns the plan's spec_stats()."""
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    ref = oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], tol, iters, -1e300,
                      mode=0 if minplus else 1, ordering=ordering)
    plan = TrwsPlan(kernel, K, N, p["conn"].T, mode)
    if p["pos"] is not None:
        plan.upload(p["unary"].T, p["alphas"], tol, positions=p["pos"])
    else:
        plan.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)
    assert plan.path() == path, "path %d, expected %d" % (plan.path(), path)
    plan.iterate(iters, max_relgap=-1e300)
    lab, en, lb, it = plan.result()
    stats = plan.spec_stats()
    plan.close()
    assert it == ref[3]
    assert np.array_equal(lab, ref[0]), "labels differ at %d of %d nodes" % (int((lab != ref[0]).sum()), N)
    assert en == ref[1] and lb == ref[2]
    return stats


# ---- K <= 64, per-edge positions: trws_pipe_kernel, both smoothness kernels, random and integer costs
PIPE = [
    # family, size, K, kernel, integer, tol, iterations
    ("single-grid", BIG, 12, 1, False, 3.0, 4),
    ("shuffled-grid", BIG, 7, 2, False, 9.0, 3),
    ("permuted-grid", BIG, 16, 1, True, 3.0, 5),
    ("row-major-grid", BIG, 9, 2, True, 8.0, 4),
    ("masked-grid", BIG, 20, 1, False, 4.0, 4),
    ("dropped-edges-grid", BIG, 10, 1, True, 2.0, 5),
    ("two-grids", BIG, 33, 2, False, 16.0, 3),
    ("ring", BIG, 64, 1, False, 6.0, 3),
    ("chain", BIG, 5, 2, True, 4.0, 4),
    ("random-tree", BIG, 8, 1, False, 2.0, 4),
    ("random-sparse", BIG, 14, 1, True, 3.0, 5),
    ("random-sparse-isolated", BIG, 6, 2, False, 9.0, 3),
    ("random-multi", BIG, 11, 1, False, 2.5, 4),
    ("random-multi", SMALL, 3, 2, True, 4.0, 5),
    ("degree-8", SMALL, 13, 1, False, 3.0, 5),
    ("degree-8", SMALL, 4, 2, True, 3.0, 5),
]


@pytest.mark.parametrize("case", PIPE, ids=["%s-K%d-k%d%s" % (c[0], c[2], c[3], "-int" if c[4] else "") for c in PIPE])
def test_pipe_per_edge_positions(case, hip, oracle):
    name, fams, K, kernel, integer, tol, iters = case
    N, conn = fams[name]
    _run(oracle, kernel, _problem(N, conn, K, 100 + K, integer=integer), tol, iters, 2)


# ---- K <= 64, shared positions: granules on (default), off, published late; the speculative schedule where the
# ---- host builds one (test_schedule_graphs_cpu.py: the renumbered and single-edged grids keep the border chain)
SHARED = [
    # family, size, K, tol, positions, unit alphas, speculative schedule active
    ("single-grid", BIG, 16, 4.0, "grid", True, True),
    ("permuted-grid", BIG, 16, 4.0, "grid", True, True),
    ("row-major-grid", BIG, 24, 3.0, "irregular", False, False),
    ("masked-grid", BIG, 16, 4.0, "grid", True, False),
    ("dropped-edges-grid", BIG, 12, 3.0, "grid", False, False),
    ("random-sparse", BIG, 16, 4.0, "grid", True, False),
    ("random-multi", BIG, 20, 5.0, "grid", False, False),     # parallel edges: twins (descriptor word 56)
    ("ring", BIG, 60, 8.0, "grid", True, False),
]


@pytest.mark.parametrize("case", SHARED, ids=[c[0] for c in SHARED])
def test_shared_positions_granules_and_spec(case, hip, oracle, monkeypatch):
    name, fams, K, tol, positions, unit, spec = case
    N, conn = fams[name]
    p = _problem(N, conn, K, 200 + K, shared=positions, unit_alphas=unit)
    stats = _run(oracle, 1, p, tol, 4, 2)
    assert stats["active"] == spec
    monkeypatch.setenv("STEREO_HIP_TRWS_GRANULES", "0")
    _run(oracle, 1, p, tol, 4, 2)
    monkeypatch.delenv("STEREO_HIP_TRWS_GRANULES")
    monkeypatch.setenv("STEREO_HIP_TRWS_DEBUG", "262144")     # a hashed quarter of the nodes publishes late
    _run(oracle, 1, p, tol, 4, 2)
    monkeypatch.delenv("STEREO_HIP_TRWS_DEBUG")
    monkeypatch.setenv("STEREO_HIP_TRWS_SPEC", "0")
    assert not _run(oracle, 1, p, tol, 4, 2)["active"]


def test_single_edged_30x40_grid_runs_the_speculative_schedule(hip, oracle):
    from stereo_amd.trws import spec_schedule
    N, conn = gf.single_grid(30, 40)
    assert [spec_schedule(N, conn.T, d)["nseg"] for d in (0, 1)] == [8, 8]
    stats = _run(oracle, 1, _problem(N, conn, 16, 7, shared="grid", unit_alphas=True), 4.0, 5, 2)
    assert stats["active"]


# ---- 64 < K <= 128, per-edge positions: trws_pipe2_kernel
PIPE2 = [("single-grid", 80, 1, False, 4.0), ("permuted-grid", 128, 1, False, 6.0), ("masked-grid", 65, 2, False, 20.0),
         ("random-sparse", 100, 1, True, 3.0), ("random-multi", 72, 2, True, 9.0), ("random-tree", 96, 1, False, 5.0),
         ("two-grids", 90, 1, True, 4.0)]


@pytest.mark.parametrize("case", PIPE2, ids=["%s-K%d" % c[:2] for c in PIPE2])
def test_pipe2_per_edge_positions(case, hip, oracle):
    name, K, kernel, integer, tol = case
    N, conn = SMALL[name]
    _run(oracle, kernel, _problem(N, conn, K, 300 + K, integer=integer), tol, 3, 4)


# ---- 64 < K <= 256, shared positions: trws_wide_kernel; an even K with the speculative schedule allowed
WIDE = [
    # family, size, K, kernel, positions, integer, tol, unit alphas, speculative schedule active
    ("single-grid", BIG, 128, 1, "grid", False, 4.0, True, True),
    ("row-major-grid", SMALL, 129, 1, "irregular", False, 5.0, False, False),
    ("masked-grid", SMALL, 256, 1, "grid", False, 8.0, False, False),
    ("dropped-edges-grid", SMALL, 100, 2, "grid", False, 16.0, False, False),
    ("random-sparse", SMALL, 200, 1, "irregular", False, 20.0, False, False),
    ("random-multi", SMALL, 96, 1, "grid", True, 4.0, False, False),
    ("shuffled-grid", SMALL, 65, 1, "grid", False, 3.0, False, False),
    ("ring", SMALL, 130, 2, "grid", True, 16.0, False, False),
]


@pytest.mark.parametrize("case", WIDE, ids=["%s-K%d" % (c[0], c[2]) for c in WIDE])
def test_wide_shared_positions(case, hip, oracle):
    name, fams, K, kernel, positions, integer, tol, unit, spec = case
    N, conn = fams[name]
    stats = _run(oracle, kernel, _problem(N, conn, K, 400 + K, integer=integer, shared=positions, unit_alphas=unit), tol, 3, 3)
    assert stats["active"] == spec


# ---- the generic kernel on request, the large-label kernel, the min-plus mode, the index order
def test_generic_kernel_on_request(hip, oracle, monkeypatch):
    monkeypatch.setenv("STEREO_HIP_TRWS_FAST", "0")
    for name, K, kernel in (("masked-grid", 9, 1), ("random-sparse", 20, 2), ("permuted-grid", 70, 1), ("random-multi", 5, 1)):
        N, conn = SMALL[name]
        _run(oracle, kernel, _problem(N, conn, K, 500 + K), 3.0, 4, 1)


def test_large_label_kernel(hip, oracle):
    for name in ("masked-grid", "random-sparse", "random-multi"):
        N, conn = SMALL[name]
        _run(oracle, 1, _problem(N, conn, 600, 600, shared="irregular"), 30.0, 2, 5)
    N, conn = gf.single_grid8(5, 6)     # any graph: also one outside the descriptor kernels' range
    _run(oracle, 1, _problem(N, conn, 600, 601, shared="grid"), 20.0, 2, 5)


def test_minplus_mode(hip, oracle):
    from stereo_amd.trws import MESSAGES_MINPLUS
    for name, K, path, shared in (("dropped-edges-grid", 10, 1, None), ("random-sparse", 12, 1, "grid"), ("masked-grid", 80, 3, "grid"),
                                  ("random-multi", 100, 3, "irregular")):
        N, conn = SMALL[name]
        _run(oracle, 1, _problem(N, conn, K, 700 + K, shared=shared), 3.0, 3, path, mode=MESSAGES_MINPLUS, minplus=True)


def test_index_order(hip, oracle):
    """ORDER_INDEX changes the visiting order and with it the whole schedule.  Every graph here stays on the pipelined
    kernel under the index order too (recorded on an MI355X; the host API has no ordering argument to derive it from):
    a graph that leaves it, or a wrong bit on it, fails."""
    from stereo_amd.trws import ORDER_INDEX
    for name in ("row-major-grid", "single-grid", "chain", "permuted-grid", "random-sparse", "masked-grid"):
        N, conn = SMALL[name]
        _run(oracle, 1, _problem(N, conn, 10, 800), 3.0, 4, 2, mode=ORDER_INDEX, ordering=1)


# ---- more runs than resident workgroups
def test_masked_image_with_more_runs_than_workgroups(hip, oracle):
    """15 % of an image masked out, sized so that the sweeps have more runs than the device keeps workgroups resident
    (at most four per CU): runs wait for a ticket.  tests/test_schedule_graphs_cpu.py passes the same schedules
    through the ticket simulation at these capacities."""
    import torch
    from stereo_amd.trws import schedule
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    resident = 4 * cus
    H, W = 40, 50
    while True:
        N, conn = gf.masked_grid(H, W, 0.15, 3)
        runs = max(len(schedule(N, conn.T, d, resident)["ticket_run"]) for d in (0, 1))
        if runs > resident:
            break
        H, W = 2 * H, 2 * W
        assert H <= 640, "no masked image with more than %d runs" % resident
    print("masked %d x %d: %d nodes, %d runs, at most %d resident workgroups" % (H, W, N, runs, resident))
    _run(oracle, 1, _problem(N, conn, 8, 900), 3.0, 3, 2)
    _run(oracle, 1, _problem(N, conn, 8, 901, shared="grid", unit_alphas=True), 4.0, 3, 2)
    # the wide kernel keeps one workgroup per CU: the 40 x 50 image already has more runs than that
    N, conn = gf.masked_grid(40, 50, 0.15, 3)
    assert max(len(schedule(N, conn.T, d, cus)["ticket_run"]) for d in (0, 1)) > cus or cus > 256
    _run(oracle, 1, _problem(N, conn, 96, 902, shared="grid"), 6.0, 2, 3)


# ---- min-marginals
@pytest.mark.parametrize("name", ["masked-grid", "random-multi"])
def test_min_marginals(name, hip, oracle):
    from mm_restate import default_impl, trws_beliefs
    from stereo_amd.trws import TrwsPlan
    N, conn = SMALL[name]
    p = _problem(N, conn, 9, 1000)
    plan = TrwsPlan(1, 9, N, conn.T)
    plan.upload(p["unary"].T, p["alphas"], 3.0, q=p["q"].T, qprim=p["qprim"].T)
    assert plan.path() == 2
    plan.keep_min_marginals()
    done = 0
    for t in (1, 3):
        plan.iterate(t - done, max_relgap=-1e300)
        done = t
        r = trws_beliefs(oracle, default_impl(oracle), 1, p, 3.0, t)
        mm, conf, am = plan.min_marginals()
        lab, en, lb, it = plan.result()
        assert it == r["iterations"] and np.array_equal(lab, r["labels"]) and en == r["energy"] and lb == r["lb"]
        assert np.array_equal(mm, r["mm"].T), np.abs(mm - r["mm"].T).max()
        assert np.array_equal(conf, r["confidence"]) and np.array_equal(am, r["argmin"] + 1)
    plan.close()


# ---- the gateway
@pytest.mark.parametrize("name", ["masked-grid", "permuted-grid"])
def test_gateway_with_two_gpus_requested(name, hip, oracle, monkeypatch):
    """stereo_trws with STEREO_HIP_GPUS=2: neither graph is the image grid the gateway cuts into row strips (a masked
    image has no H x W node numbering, a renumbered grid no rows of consecutive ids) -- one plan, the single plan's
    result."""
    from stereo_amd import _lib
    N, conn = BIG[name]
    p = _problem(N, conn, 12, 1100)
    args = (1, p["unary"].T, conn.T + 1, p["q"].T, p["qprim"].T, p["alphas"], 3.0, dict(maxiter=4, max_relgap=-1))
    one = hip.trws(*args)
    assert _lib.lib().stereo_trws_gateway_strips() == 1
    monkeypatch.setenv("STEREO_HIP_GPUS", "2")
    two = hip.trws(*args)
    assert _lib.lib().stereo_trws_gateway_strips() == 1
    assert np.array_equal(one[0], two[0]) and one[1:] == two[1:]
    ref = oracle.trws(1, p["unary"], conn, p["q"], p["qprim"], p["alphas"], 3.0, 4, -1.0, mode=1)
    assert np.array_equal(two[0], ref[0]) and two[1:] == ref[1:]


# ---- outside the descriptor kernels' range: the generic kernel, asserted
@pytest.mark.parametrize("which", ["single-grid8", "degree-9", "deadlock8"])
def test_graphs_the_generic_kernel_takes(which, hip, oracle):
    """More than four foreign dependencies (8-neighbourhood), nine incident edges, and the graph inside both limits on
    whose chain schedule the loader protocol cannot terminate (graph_families.DEADLOCK8): path 1, and the oracle's
    result."""
    slow = {f[0]: f[1:] for f in gf.slow_families()}
    N, conn = (gf.DEADLOCK8_N, gf.DEADLOCK8) if which == "deadlock8" else slow[which]
    for K, kernel, shared in ((6, 1, None), (16, 1, "grid"), (70, 2, None), (100, 1, "grid")):
        _run(oracle, kernel, _problem(N, conn, K, 1200 + K, shared=shared), 3.0, 5, 1)


def test_random_sparse_graphs_each_on_the_path_the_host_names(hip, oracle):
    """40 seeded random sparse graphs (the family on which the chain schedule can deadlock): each runs the pipelined
    kernel if the host hands out a schedule for it and the generic kernel if not -- asserted per graph, none skipped."""
    from stereo_amd import StereoHipError
    from stereo_amd.trws import schedule
    generic = 0
    for seed in range(40):
        N, conn = gf.random_sparse(12 + seed, seed, isolated=seed % 3)
        try:
            schedule(N, conn.T, 0, 0)
            path = 2
        except StereoHipError:
            path = 1
            generic += 1
        _run(oracle, 1, _problem(N, conn, 7, 1300 + seed), 3.0, 3, path)
    print("random sparse graphs on the generic kernel: %d of 40" % generic)


# ---- a speculative schedule the host cannot show to terminate is never launched
def test_chains_with_side_runs_and_the_speculative_schedule(hip, oracle):
    """Long chains with short side runs (graph_families.SPEC_DEADLOCK172 / 302 and seeded ones): the pipelined kernel,
    the oracle's bits, and the speculative schedule active exactly where the host hands one out for BOTH directions --
    on the two named graphs it does not (tests/test_schedule_graphs_cpu.py shows why), on some of the seeded ones it does."""
    from stereo_amd.trws import spec_schedule
    graphs = [("172", gf.SPEC_DEADLOCK172_N, gf.SPEC_DEADLOCK172, False), ("302", gf.SPEC_DEADLOCK302_N, gf.SPEC_DEADLOCK302, False)]
    graphs += [("seed %d" % seed, *gf.chain_with_side_runs(150 + 17 * seed, seed, gadgets=1 + seed % 3), None) for seed in range(12)]
    seen = set()
    for name, N, conn, want in graphs:
        sp = [spec_schedule(N, conn.T, d) for d in (0, 1)]
        host = all(x is not None for x in sp) and sp[0]["nseg"] == sp[1]["nseg"]
        if want is not None:
            assert host == want, name
        stats = _run(oracle, 1, _problem(N, conn, 16, 1400 + N, shared="grid", unit_alphas=True), 4.0, 4, 2)
        assert stats["active"] == host, name
        seen.add(host)
    assert seen == {False, True}
