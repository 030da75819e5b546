"""-m gpu: who publishes the row granules, and from where (descriptor word 57; trws_pipe.hip).

Round 9 built the publisher on the storer wave (first thing behind the barrier that ends a node's visit, out of the
hand-over ring, lanes beyond K repeating lane K - 1, a run's last node in the run's trailing visit), measured it, and
did not keep it; what ships is the finishing compute wave publishing as before, with the edge ids and the
granule word taken from one per-lane LDS read at the top of the visit instead of three reads behind the message.
These are the shapes at which either publisher can go wrong, and they stay as the check of whichever is in the kernel:
a granule carries the very 64 bits the flag path loads, so labels, energy, bound and iteration count must be the same
after EVERY iteration with granules off (STEREO_HIP_TRWS_GRANULES=0), on (the default) and on with development switch
262144 (a hashed quarter of the nodes publishes a few microseconds late: consumers find old tags and sweep again).

Shapes: K = 64 (no lanes beyond K), 60, 8 and 3 (almost only lanes beyond K) on the speculative kernel; pieces of at
most 3 positions on 3 workgroups, whose last node feeds the next piece's first (interior widths 22, 11 and 10: the
last pieces hold 1, 2 and 1 positions -- one-position runs included); more runs than workgroups on a short row; and
the instantiations that share the roles: smoothness kernel 2, per-edge positions, the plain schedule.  One case is
compared with the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS")
WAYS = ({"STEREO_HIP_TRWS_GRANULES": "0"}, {}, {"STEREO_HIP_TRWS_DEBUG": "262144"})


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


def _plan(kernel, K, N, conn, max_workgroups):
    """a whole-problem TrwsPlan; max_workgroups > 0: created with a limit on its workgroups (one strip), so that a
    small grid has more runs than workgroups and gets pieces"""
    from stereo_amd import _lib
    from stereo_amd.trws import TrwsPlan
    if not max_workgroups:
        return TrwsPlan(kernel, K, N, conn.T)
    plan = TrwsPlan.__new__(TrwsPlan)
    plan._conn = np.asfortranarray(conn.T, dtype=np.uint32)
    plan.K, plan.N, plan.E = int(K), int(N), int(conn.shape[0])
    plan._h, plan._keep = C.c_void_p(), []
    err = _lib.errbuf()
    rc = _lib.lib().stereo_trws_plan_create_strip(
        C.c_int(kernel), C.c_int(plan.K), C.c_int64(plan.N), C.c_int64(plan.E), plan._conn.ctypes.data_as(C.POINTER(C.c_uint32)),
        C.c_int(0), None, C.c_int(1), C.c_int(0), C.c_int(int(max_workgroups)), None, C.byref(plan._h), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    return plan


def _runs(plan):
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


def _solve(monkeypatch, env, kernel, H, W, K, where, tol, iters, max_workgroups=0):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    unary, conn, alphas, q = _problem(H, W, K, where)
    plan = _plan(kernel, K, H * W, conn, max_workgroups)
    if where == "shared":
        plan.upload(unary.T, alphas, tol, positions=q[0])
    else:
        plan.upload(unary.T, alphas, tol, q=q.T, qprim=q.T)
    out = []
    for _ in range(iters):
        plan.iterate(1, max_relgap=-1e300)
        lab, en, lb, it = plan.result()
        out.append((lab.copy(), en, lb, it))
    info = dict(path=plan.path(), runs=_runs(plan) if max_workgroups else None)
    plan.close()
    return out, info


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))


def _three_ways(monkeypatch, base, *args, **kw):
    off, info = _solve(monkeypatch, dict(base, **WAYS[0]), *args, **kw)
    on, info_on = _solve(monkeypatch, dict(base, **WAYS[1]), *args, **kw)
    late, _ = _solve(monkeypatch, dict(base, **WAYS[2]), *args, **kw)
    assert info["path"] == info_on["path"] == 2   # the K <= 64 pipelined kernel
    assert _same(off, on)
    assert _same(off, late)
    return on, info_on


@pytest.mark.parametrize("K", (8, 64, 60, 3))
def test_shared_positions(K, hip, monkeypatch):
    """the speculative kernel's instantiation, 24 x 31: no clamped lanes (K = 64) to almost only clamped lanes (K = 3)"""
    _three_ways(monkeypatch, {}, 1, 24, 31, K, "shared", 4.0, 4)


@pytest.mark.parametrize("H,W,last", ((8, 24, 1), (10, 13, 2), (8, 12, 1)))
def test_last_node_of_a_piece(H, W, last, hip, monkeypatch):
    """pieces of at most 3 positions on 3 workgroups: a piece's last node feeds the next piece's first; the last piece
    of a row is a run of `last` positions"""
    assert (W - 2) % 3 == last % 3
    base = {"STEREO_HIP_TRWS_ROW_CHUNK": "3"}
    pieces, info = _three_ways(monkeypatch, base, 1, H, W, 5, "shared", 4.0, 4, max_workgroups=3)
    rows, rows_info = _solve(monkeypatch, {"STEREO_HIP_TRWS_ROW_CHUNK": "0"}, 1, H, W, 5, "shared", 4.0, 4, max_workgroups=3)
    assert min(info["runs"]) > max(rows_info["runs"]) and min(info["runs"]) >= (H - 2) * ((W - 2 + 2) // 3)   # every interior row in pieces
    assert _same(rows, pieces)


def test_more_runs_than_workgroups(hip, monkeypatch):
    """280 short rows: runs wait for a workgroup, a row's consumer may start long after its producer published"""
    _three_ways(monkeypatch, {}, 1, 280, 9, 4, "shared", 4.0, 4)


@pytest.mark.parametrize("kernel,H,W,K,where,spec,tol", ((2, 20, 26, 12, "shared", True, 30.0), (1, 18, 22, 10, "edges", True, 4.0),
                                                        (1, 24, 31, 8, "shared", False, 4.0)),
                         ids=("kernel2", "per-edge", "nospec"))
def test_plain_instantiations(kernel, H, W, K, where, spec, tol, hip, monkeypatch):
    """the kernels without the speculative schedule share the compute and storer roles"""
    _three_ways(monkeypatch, {} if spec else {"STEREO_HIP_TRWS_SPEC": "0"}, kernel, H, W, K, where, tol, 4)


def test_against_the_oracle(hip, oracle, monkeypatch):
    H, W, K, iters = 16, 21, 8, 3
    got, _ = _three_ways(monkeypatch, {}, 1, H, W, K, "shared", 4.0, iters)
    unary, conn, alphas, q = _problem(H, W, K, "shared")
    want = oracle.trws(1, unary, conn, q, q, alphas, 4.0, iters, -1e300, mode=1)
    lab, en, lb, it = got[-1]
    assert np.array_equal(lab, want[0]) and (en, lb, it) == (want[1], want[2], want[3])
