"""-m gpu: sub-row runs on the K <= 64 kernel (STEREO_HIP_TRWS_ROW_CHUNK; trws_graph.h: Sweep::Chunked).

Where a sweep has more runs than resident workgroups, a plan's own launches walk the grid rows in pieces of at most C
positions.  The pieces visit the same nodes in the same order within a row and only move the point where a row's
hand-over goes through memory, so labels, energy, bound, iteration count and serial_messages must be the same bit for
bit with C = 8 and with whole rows (C = 0), after each of 3 iterations, and equal to the CPU oracle; the speculative
schedule's second walks must not change either.

Grids 8 x 24 and 10 x 40 with K = 5 and K = 60, shared positions (the speculative kernel where the schedule is active)
and per-edge positions (the plain kernel), granules on and off, 3 workgroups (fewer than runs: pieces) and no limit
(a workgroup per run: the gate leaves whole rows).  One tall grid has more rows than a device has compute units, so the
pieces meet the speculative schedule without a limit; K = 100 runs the two-labels-per-lane kernel, where the switch is
ignored."""
import ctypes as C

import numpy as np
import pytest

from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS")
ITERS = 3
TOL = 4.0


def _problem(H, W, K, where):
    rng = np.random.default_rng(1000 * H + 10 * W + K)
    conn = grid_conn(H, W)
    unary = rng.uniform(0, 40, size=(H * W, K))
    alphas = rng.uniform(0.5, 2.0, size=conn.shape[0])
    if where == "shared":
        q = np.tile(np.arange(K, dtype=np.float64), (conn.shape[0], 1))
    else:
        q = np.tile(rng.permutation(K).astype(np.float64), (conn.shape[0], 1))
    return unary, conn, alphas, q


def _plan(K, N, conn, max_workgroups):
    """a whole-problem TrwsPlan, created with a limit on its workgroups (stereo_trws_plan_create_strip, one strip)"""
    from stereo_amd import _lib
    from stereo_amd.trws import TrwsPlan
    plan = TrwsPlan.__new__(TrwsPlan)
    plan._conn = np.asfortranarray(conn.T, dtype=np.uint32)
    plan.K, plan.N, plan.E = int(K), int(N), int(conn.shape[0])
    plan._h, plan._keep = C.c_void_p(), []
    err = _lib.errbuf()
    rc = _lib.lib().stereo_trws_plan_create_strip(
        C.c_int(1), C.c_int(plan.K), C.c_int64(plan.N), C.c_int64(plan.E), plan._conn.ctypes.data_as(C.POINTER(C.c_uint32)),
        C.c_int(0), None, C.c_int(1), C.c_int(0), C.c_int(int(max_workgroups)), None, C.byref(plan._h), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return plan


def _runs(plan):
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


def _solve(monkeypatch, env, H, W, K, where, max_workgroups):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    unary, conn, alphas, q = _problem(H, W, K, where)
    plan = _plan(K, H * W, conn, max_workgroups)
    if where == "shared":
        plan.upload(unary.T, alphas, TOL, positions=q[0])
    else:
        plan.upload(unary.T, alphas, TOL, q=q.T, qprim=q.T)
    out = []
    for _ in range(ITERS):
        plan.iterate(1, max_relgap=-1e300)
        lab, en, lb, it = plan.result()
        out.append((lab.copy(), en, lb, it, plan.serial_messages()))
    info = dict(path=plan.path(), runs=_runs(plan), spec=plan.spec_stats())
    plan.close()
    return out, info


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))


_oracle = {}


def _reference(oracle, H, W, K, where):
    """the oracle after each iteration, once per problem"""
    if (H, W, K, where) not in _oracle:
        unary, conn, alphas, q = _problem(H, W, K, where)
        _oracle[H, W, K, where] = [oracle.trws(1, unary, conn, q, q, alphas, TOL, n, -1e300, mode=1) for n in range(1, ITERS + 1)]
    return _oracle[H, W, K, where]


CASES = [(H, W, K, where, gran, wg) for H, W in ((8, 24), (10, 40)) for K in (5, 60) for where in ("shared", "edges")
         for gran in (True, False) for wg in (3, 0)]


@pytest.mark.parametrize("H,W,K,where,gran,wg", CASES)
def test_pieces_change_nothing(H, W, K, where, gran, wg, hip, oracle, monkeypatch):
    base = {} if gran else {"STEREO_HIP_TRWS_GRANULES": "0"}
    rows, rows_info = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_ROW_CHUNK="0"), H, W, K, where, wg)
    pieces, info = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_ROW_CHUNK="8"), H, W, K, where, wg)
    assert info["path"] == rows_info["path"] == 2
    if wg:   # fewer workgroups than rows: the rows are walked in pieces of at most 8
        assert min(info["runs"]) > max(rows_info["runs"]) and min(info["runs"]) >= H * W // 8
    else:    # a workgroup for every row: nothing to gain, whole rows
        assert info["runs"] == rows_info["runs"]
    assert _same(rows, pieces)
    assert info["spec"] == rows_info["spec"]
    ref = _reference(oracle, H, W, K, where)
    for got, want in zip(pieces, ref):
        assert np.array_equal(got[0], want[0]) and got[1:4] == (want[1], want[2], want[3])


@pytest.mark.parametrize("gran", (True, False))
def test_pieces_under_the_speculative_schedule(gran, hip, oracle, monkeypatch):
    """more rows than compute units: pieces without a limit on the workgroups, the border chain speculated"""
    H, W, K, where = 300, 24, 5, "shared"
    base = {} if gran else {"STEREO_HIP_TRWS_GRANULES": "0"}
    rows, rows_info = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_ROW_CHUNK="0"), H, W, K, where, 0)
    pieces, info = _solve(monkeypatch, dict(base, STEREO_HIP_TRWS_ROW_CHUNK="8"), H, W, K, where, 0)
    assert info["spec"]["active"] and rows_info["spec"]["active"]
    from stereo_amd import _lib
    if 0 < _lib.lib().stereo_hip_device_cus() < H - 2:
        assert min(info["runs"]) > max(rows_info["runs"])
    assert _same(rows, pieces)
    assert info["spec"]["second_walks"] == rows_info["spec"]["second_walks"] and info["spec"]["commits"] == rows_info["spec"]["commits"]
    ref = _reference(oracle, H, W, K, where)
    for got, want in zip(pieces, ref):
        assert np.array_equal(got[0], want[0]) and got[1:4] == (want[1], want[2], want[3])


def test_switch_is_ignored_off_the_gate(hip, monkeypatch):
    """K = 100 with per-edge positions: the two-labels-per-lane kernel keeps whole rows whatever the switch says"""
    H, W, K = 8, 24, 100
    rows, rows_info = _solve(monkeypatch, {"STEREO_HIP_TRWS_ROW_CHUNK": "0"}, H, W, K, "edges", 3)
    pieces, info = _solve(monkeypatch, {"STEREO_HIP_TRWS_ROW_CHUNK": "8"}, H, W, K, "edges", 3)
    assert info["path"] == rows_info["path"] == 4
    assert info["runs"] == rows_info["runs"]
    assert _same(rows, pieces)
