"""-m gpu: the staged prefix of Di (stage row kStP; trws_pipe.hip).

Loader A of the K <= 64 kernel adds the unary row and the node's outgoing rows -- last sweep's messages, which it holds
in registers two visits ahead -- in list order and stages the sum once per node; the compute waves start from it and
add only the tail, list positions nout .. nout + 3 in one batch (a position the node does not have is the zero row)
and, behind one uniform branch, positions nout + 4 .. of a node with more than four incoming rows.  The sum keeps its
association, so labels, energy and lower bound after 3 iterations must be the CPU oracle's bit for bit, and the same
with granules off (STEREO_HIP_TRWS_GRANULES=0) and on the plain schedule (STEREO_HIP_TRWS_SPEC=0).

Shapes, the smallest at which the staging can go wrong: grids 7 x 5 and 12 x 9 (every combination of outgoing and
incoming rows that corners, borders, row ends and interior nodes have), K = 3, 8, 60 and 64 (lanes beyond K, up to
none), both smoothness kernels, shared and per-edge positions; rows in pieces of at most 3 positions; more runs than
workgroups; two logical strips; a batch of two problems; graphs off the grid with a node of eight incoming rows (the
tail branch); weights that differ between the two edges of a pair (twins that are not the same message).  The wide
kernel (24 x 16, K = 66 and 256) has staged its prefix since round 4 and is held to the same bar here.

The speculative schedule needs a border chain of at least 8 segments: the small grids get it with segments of 4 visits
(STEREO_HIP_TRWS_SPEC_SEG=4), 30 x 40 with the default 16.  Every case asserts plan.spec_stats(): active with commits
where it is meant to run (trws_pipe_spec_kernel, trws_wide_spec_kernel), not active elsewhere and under
STEREO_HIP_TRWS_SPEC=0; with development switch 16384 (the runner's rows made wrong) segments are walked a second time.

Two strips add their energies and bounds strip by strip: the interface promises those sums to 1e-12 relative
(include/stereo_hip.h, tests/test_strips_gpu.py), so against the oracle the strips are held to bitwise labels and to
that bound for the two sums -- and to bitwise sums between the three ways of running the same strips."""
import ctypes as C

import numpy as np
import pytest

import graph_families as gf
from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS",
       "STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_MESSAGES", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_CERTIFICATE",
       "STEREO_HIP_TRWS_SPEC_SEG")
WAYS = ({}, {"STEREO_HIP_TRWS_GRANULES": "0"}, {"STEREO_HIP_TRWS_SPEC": "0"})
ITERS = 3
NEVER = -1e300
GRIDS = ((7, 5), (12, 9))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STEREO_HIP_TRWS_SPIN_SECONDS", "3")


_problems, _wanted = {}, {}


def _problem(N, conn, K, where, alphas, seed):
    """dict(unary (N,K), conn (E,2), q, qprim (E,K), alphas (E,), pos); built once per key, never changed"""
    key = (N, conn.shape[0], int(conn.sum()), K, where, alphas, seed)
    if key not in _problems:
        rng = np.random.default_rng(seed)
        E = conn.shape[0]
        unary = rng.uniform(0, 40, size=(N, K))
        a = np.ones(E) if alphas == "unit" else rng.uniform(0.5, 2.0, size=E)
        pos = None
        if where == "shared":
            pos = np.arange(K, dtype=np.float64)
            q = np.tile(pos, (E, 1)); qprim = q.copy()
        else:
            slope = rng.uniform(0.5, 1.5, size=(E, 1))
            q = np.arange(K)[None, :] * slope + rng.normal(size=(E, K)) * 1.5
            qprim = np.arange(K)[None, :] * slope + rng.normal(size=(E, K)) * 1.5
        _problems[key] = dict(key=key, unary=unary, conn=conn, q=q, qprim=qprim, alphas=a, pos=pos)
    return _problems[key]


def _grid(H, W, K, where, alphas="unit"):
    return _problem(H * W, grid_conn(H, W), K, where, alphas, 1000 * H + 10 * W + K)


def _oracle(oracle, kernel, p, tol):
    key = (kernel, tol) + p["key"]
    if key not in _wanted:
        _wanted[key] = oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], tol, ITERS, NEVER, mode=1)
    return _wanted[key]


def _upload(plan, p, tol):
    if p["pos"] is not None:
        plan.upload(p["unary"].T, p["alphas"], tol, positions=p["pos"])
    else:
        plan.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)


def _plan(kernel, p, tol, max_workgroups=0):
    """a whole-problem TrwsPlan with its inputs; max_workgroups > 0: created with a limit on its workgroups (one strip)"""
    from stereo_amd import _lib
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    if not max_workgroups:
        plan = TrwsPlan(kernel, K, N, p["conn"].T)
    else:
        plan = TrwsPlan.__new__(TrwsPlan)
        plan._conn = np.asfortranarray(p["conn"].T, dtype=np.uint32)
        plan.K, plan.N, plan.E = int(K), int(N), int(p["conn"].shape[0])
        plan._h, plan._keep = C.c_void_p(), []
        err = _lib.errbuf()
        rc = _lib.lib().stereo_trws_plan_create_strip(
            C.c_int(kernel), C.c_int(plan.K), C.c_int64(plan.N), C.c_int64(plan.E), plan._conn.ctypes.data_as(C.POINTER(C.c_uint32)),
            C.c_int(0), None, C.c_int(1), C.c_int(0), C.c_int(int(max_workgroups)), None, C.byref(plan._h), err, C.c_size_t(len(err)))
        _lib.check(rc, err)
    _upload(plan, p, tol)
    return plan


def _runs(plan):
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


def _is(got, want):
    lab, en, lb, it = got
    assert it == want[3]
    assert np.array_equal(lab, want[0]), "labels differ at %d of %d nodes" % (int((lab != want[0]).sum()), lab.size)
    assert en == want[1] and lb == want[2], ((en, lb), want[1:3])


def _three_ways(monkeypatch, oracle, kernel, p, tol, path, base={}, max_workgroups=0, spec=False, ways=WAYS):
    """the plan by default, with granules off and on the plain schedule, each against the oracle; returns the runs
    (forward, backward) of the default plan where it was created with a limit.  spec: whether the speculative schedule
    is active in the ways that do not switch it off -- asserted, with its commits, so that a case which is meant to run
    trws_pipe_spec_kernel / trws_wide_spec_kernel cannot quietly run the plain kernel (and the other way round)"""
    want = _oracle(oracle, kernel, p, tol)
    runs = None
    for way in ways:
        with monkeypatch.context() as m:
            for k, v in dict(base, **way).items():
                m.setenv(k, v)
            plan = _plan(kernel, p, tol, max_workgroups)
            assert plan.path() == path, "path %d, expected %d" % (plan.path(), path)
            plan.iterate(ITERS, max_relgap=NEVER)
            got = plan.result()
            stats = plan.spec_stats()
            if max_workgroups and not way:
                runs = _runs(plan)
            plan.close()
        _is(got, want)
        on = spec and way.get("STEREO_HIP_TRWS_SPEC") != "0"
        assert bool(stats["active"]) == on, (way, stats)
        if on:
            assert stats["commits"] > 0 and stats["runner_visits"] > 0, (way, stats)
        if "STEREO_HIP_TRWS_DEBUG" in way:
            assert stats["second_walks"] > 0, (way, stats)
    return runs


# ---- K <= 64: trws_pipe_kernel.  These grids' border chains are too short for the speculative schedule at its default
# ---- segment length (fewer than 8 segments of 16 visits): every way here runs the plain kernel, asserted
@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("kernel,tol", ((1, 4.0), (2, 30.0)))
@pytest.mark.parametrize("K", (3, 8, 60, 64))
@pytest.mark.parametrize("H,W", GRIDS)
def test_grids(H, W, K, kernel, tol, where, hip, oracle, monkeypatch):
    _three_ways(monkeypatch, oracle, kernel, _grid(H, W, K, where), tol, 2)


# ---- K <= 64 with the speculative schedule ON: trws_pipe_spec_kernel.  Segments of 4 visits (STEREO_HIP_TRWS_SPEC_SEG=4)
# ---- give the 12 x 9 and 9 x 12 grids 9 segments per direction, the default 16 gives 30 x 40 its 8.  A segment's first
# ---- visit takes the rows of the node in front from the runner (loader B's tail table points at the stage for them);
# ---- development switch 16384 makes the runner's rows wrong, so that segments are walked a second time from the rows
# ---- loader A kept -- the staged prefix of a second walk must be the sum of THOSE rows
SPEC_WAYS = WAYS + ({"STEREO_HIP_TRWS_DEBUG": "16384"},)
# (the runner walks the truncation window in groups of four entries and wants every index distance beyond the window to
#  cost the truncation value: with three labels that holds for 2 <= tol < 3, trws_inputs.hip: analyse_window)
SPEC_CASES = [(12, 9, 3, "4", "unit", 2.5)] + [(12, 9, K, "4", "unit", 4.0) for K in (8, 60, 64)] + [
    (9, 12, 8, "4", "random", 4.0), (12, 9, 60, "4", "random", 4.0), (30, 40, 8, None, "unit", 4.0), (30, 40, 60, None, "random", 4.0)]


@pytest.mark.parametrize("H,W,K,seg,alphas,tol", SPEC_CASES, ids=["%dx%d-K%d-seg%s-%s" % (c[0], c[1], c[2], c[3] or "16", c[4]) for c in SPEC_CASES])
def test_speculative_schedule(H, W, K, seg, alphas, tol, hip, oracle, monkeypatch):
    from stereo_amd.trws import spec_schedule
    base = {"STEREO_HIP_TRWS_SPEC_SEG": seg} if seg else {}
    p = _grid(H, W, K, "shared", alphas=alphas)
    with monkeypatch.context() as m:
        for k, v in base.items():
            m.setenv(k, v)
        assert all(spec_schedule(H * W, p["conn"].T, d)["nseg"] >= 8 for d in (0, 1))
    _three_ways(monkeypatch, oracle, 1, p, tol, 2, base=base, spec=True, ways=SPEC_WAYS)


@pytest.mark.parametrize("K", (8, 60))
@pytest.mark.parametrize("H,W", GRIDS)
def test_weights_that_differ_within_a_pair(H, W, K, hip, oracle, monkeypatch):
    """the two edges of a pair of pixels carry different weights: twins by the descriptor, not the same message"""
    p = _grid(H, W, K, "shared", alphas="random")
    i1, i2 = p["conn"][:, 0], p["conn"][:, 1]
    fwd = {(a, b): w for a, b, w in zip(i1, i2, p["alphas"])}
    assert any((b, a) in fwd and fwd[(b, a)] != w for (a, b), w in fwd.items())
    _three_ways(monkeypatch, oracle, 1, p, 4.0, 2)


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("H,W,last", ((12, 9, 1), (9, 12, 1), (7, 5, 3)))
def test_rows_in_pieces(H, W, last, where, hip, oracle, monkeypatch):
    """pieces of at most 3 positions on 3 workgroups: a piece's first node takes its in-row message from memory; the
    last piece of a row has `last` positions"""
    assert (W - 2 - last) % 3 == 0
    runs = _three_ways(monkeypatch, oracle, 1, _grid(H, W, 8, where), 4.0, 2, base={"STEREO_HIP_TRWS_ROW_CHUNK": "3"}, max_workgroups=3)
    assert min(runs) >= (H - 2) * ((W - 2 + 2) // 3)   # every interior row in pieces


@pytest.mark.parametrize("where", ("shared", "edges"))
def test_more_runs_than_workgroups(where, hip, oracle, monkeypatch):
    """12 x 9 on four workgroups: runs wait for a ticket"""
    runs = _three_ways(monkeypatch, oracle, 1, _grid(12, 9, 60, where), 4.0, 2, base={"STEREO_HIP_TRWS_BLOCKS": "4"}, max_workgroups=4)
    assert min(runs) > 4


@pytest.mark.parametrize("where", ("shared", "edges"))
def test_two_logical_strips(where, hip, oracle, monkeypatch):
    """(strips keep the plain schedule: the third way runs the same kernel as the first, and says that the switch is
    ignored there)"""
    from stereo_amd.strips import make_strips
    H, W, K, tol = 12, 9, 8, 4.0
    p = _grid(H, W, K, where)
    want = _oracle(oracle, 1, p, tol)
    sums = []
    for way in WAYS:
        with monkeypatch.context() as m:
            for k, v in way.items():
                m.setenv(k, v)
            s = make_strips(1, K, H, W, p["conn"].T, 2)
            _upload(s, p, tol)
            done, _ = s.iterate(ITERS, max_relgap=NEVER)
            lab, en, lb, it = s.result()
            assert done == ITERS and s.path() == 2
            s.close()
        assert it == want[3] and np.array_equal(lab, want[0])
        for x, y in ((en, want[1]), (lb, want[2])):
            assert abs(x - y) <= 1e-12 * max(abs(x), abs(y), 1.0), (x, y)
        sums.append((en, lb))
    assert sums[0] == sums[1] == sums[2]


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("kernel,tol", ((1, 4.0), (2, 30.0)))
def test_a_batch_of_two(kernel, tol, where, hip, oracle, monkeypatch):
    from stereo_amd.trws import TrwsBatch
    problems = [_grid(7, 5, 60, where), _grid(12, 9, 8, where)]
    for way in WAYS:
        with monkeypatch.context() as m:
            for k, v in way.items():
                m.setenv(k, v)
            plans = [_plan(kernel, p, tol) for p in problems]
            assert all(pl.path() == 2 for pl in plans)
            with TrwsBatch(plans) as batch:
                assert batch.iterate(ITERS, NEVER) == [ITERS] * 2
            for pl, p in zip(plans, problems):
                _is(pl.result(), _oracle(oracle, kernel, p, tol))
                pl.close()


OFF_GRID = {f[0]: f[1:] for f in gf.fast_families(1) if f[0] in ("degree-8", "random-multi")}


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("name,K", (("degree-8", 13), ("degree-8", 64), ("random-multi", 20)))
def test_graphs_with_more_than_four_incoming_rows(name, K, where, hip, oracle, monkeypatch):
    """the hub of the star in a chain has one outgoing and seven incoming rows in the backward sweep, seven and one in
    the forward sweep; the sparse graph with parallel edges has nodes of five, six and eight incoming rows, some next
    to two or three outgoing ones -- tails that start in the middle of the row table and take the branch"""
    from stereo_amd.trws import descriptors
    N, conn = OFF_GRID[name]
    f = np.concatenate([descriptors(N, conn.T, d)[:, 2] for d in (0, 1)])   # word 2: n_out | n_in << 4 | ...
    assert ((f >> 4) & 15).max() >= 5 and ((f & 15) + ((f >> 4) & 15)).max() == 8
    _three_ways(monkeypatch, oracle, 1, _problem(N, conn, K, where, "random", 77 + K), 4.0, 2)


# ---- 64 < K <= 256, shared positions: trws_wide_kernel on the plain schedule (24 x 16 has no speculative schedule at
# ---- the default segment length), then trws_wide_spec_kernel with segments of 4 visits (19 per direction), second walks
# ---- included
@pytest.mark.parametrize("K", (66, 256))
def test_wide_kernel(K, hip, oracle, monkeypatch):
    _three_ways(monkeypatch, oracle, 1, _grid(24, 16, K, "shared"), 6.0, 3)


@pytest.mark.parametrize("K", (66, 256))
def test_wide_kernel_speculative_schedule(K, hip, oracle, monkeypatch):
    _three_ways(monkeypatch, oracle, 1, _grid(24, 16, K, "shared"), 6.0, 3, base={"STEREO_HIP_TRWS_SPEC_SEG": "4"}, spec=True, ways=SPEC_WAYS)
