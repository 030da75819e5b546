"""-m gpu: the loaders of the K <= 64 runner on host-made chain records (trws_spec.h: run_loader,
trws_runner_records.cpp) -- what tests/test_runner_visit_gpu.py does not reach.

The runner decides no result, so a wrong record shows as second walks or a wait that gives up, not as a wrong label:
every case walks 3 iterations, compares labels, energy and bound with the CPU oracle bit for bit after each, on the
speculative schedule (spec_stats() active, commits, second_walks == 0) and on the plain one (STEREO_HIP_TRWS_SPEC=0: not
active).  Unaries are continuous random numbers; STEREO_HIP_TRWS_SPIN_SECONDS=3.

  (a) what a record must NOT hold.  One plan: weights "ones" (the two rows to the next node are twins: one message),
      3 iterations, then an upload of independent weights per directed edge on the SAME plan (two messages) and 3
      more from zero -- the twin verdict follows the data, a stale one would hand wrong rows to the segments.  Then a
      second plan on the same connectivity (the cached graph) with another K, 8 and 60: nothing of K is in a record.
  (b) 30 x 40, K = 8, STEREO_HIP_TRWS_ROW_CHUNK=0,12 and STEREO_HIP_TRWS_BLOCKS=16: the backward sweep walks the sub-row
      descriptor set (more runs than the forward sweep by a factor), the speculative schedule on it, with the records
      made from THAT set.
  (c) 13 x 10 with STEREO_HIP_TRWS_SPEC_SEG=4: 42 chain positions, ten segments, the last of two visits; K = 3 (window
      1, lanes beyond K) and K = 64 (none).
  (d) off the image grid: the permuted 14 x 19 grid of tests/graph_families.py with segments of 4 keeps the speculative
      schedule; its chain nodes wait for foreign nodes and take up to four incoming rows.  Four is the most a chain
      node of that schedule can have: runner_can_walk (trws_graph_desc.cpp) refuses the schedule to a graph with more,
      so "more than four incoming rows" exists only in the CPU test of the records."""
import ctypes as C

import numpy as np
import pytest

import graph_families as gf
from helpers import grid_conn

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS",
       "STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_MESSAGES", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_CERTIFICATE",
       "STEREO_HIP_TRWS_SPEC_SEG")
ITERS = 3
NEVER = -1e300


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STEREO_HIP_TRWS_SPIN_SECONDS", "3")


_problems, _wanted = {}, {}


def _problem(name, N, conn, K, step, seed):
    """dict(unary (N, K), conn, q (E, K), pos, ones, pair); built once per key, never changed"""
    key = (name, K, step)
    if key not in _problems:
        rng = np.random.default_rng(seed)
        pos = np.arange(K, dtype=np.float64) * step
        pair = rng.uniform(0.5, 2.0, size=conn.shape[0])
        w = {(int(i), int(j)): x for (i, j), x in zip(conn, pair)}
        assert any((j, i) in w and w[(j, i)] != x for (i, j), x in w.items())
        _problems[key] = dict(key=key, unary=rng.uniform(0, 40, size=(N, K)), conn=conn, q=np.tile(pos, (conn.shape[0], 1)), pos=pos,
                              ones=np.ones(conn.shape[0]), pair=pair)
    return _problems[key]


def _oracle(oracle, p, form, tol):
    key = (form, tol) + p["key"]
    if key not in _wanted:
        _wanted[key] = [oracle.trws(1, p["unary"], p["conn"], p["q"], p["q"], p[form], tol, n, NEVER, mode=1) for n in range(1, ITERS + 1)]
    return _wanted[key]


def _is(got, want, what):
    lab, en, lb, it = got
    assert it == want[3], what
    assert np.array_equal(lab, want[0]), "%s: labels differ at %d of %d nodes" % (what, int((lab != want[0]).sum()), lab.size)
    assert en == want[1] and lb == want[2], (what, (en, lb), want[1:3])


def _walk(plan, oracle, p, form, tol, what):
    """upload `form`, start from zero, 3 iterations checked against the oracle one by one"""
    plan.upload(p["unary"].T, p[form], tol, positions=p["pos"])
    plan.reset()
    assert plan.path() == 2, "path %d, expected the K <= 64 kernel" % plan.path()
    want = _oracle(oracle, p, form, tol)
    for n in range(ITERS):
        plan.iterate(1, max_relgap=NEVER)
        got = plan.result()
        print(what, form, "iteration", n + 1, "energy", got[1], "bound", got[2], plan.spec_stats())
        _is(got, want[n], "%s, weights %s, iteration %d" % (what, form, n + 1))


def _runs(plan):
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


def _check(monkeypatch, oracle, env, p, tol, forms=("pair",), more=None):
    """both schedules; returns nothing, asserts everything"""
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    for spec in (True, False):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            if not spec:
                m.setenv("STEREO_HIP_TRWS_SPEC", "0")
            plan = TrwsPlan(1, K, N, p["conn"].T)
            before = 0
            for form in forms:
                _walk(plan, oracle, p, form, tol, "speculative" if spec else "plain")
                st = plan.spec_stats()
                if spec:
                    assert st["active"] and st["commits"] > before and st["runner_visits"] > 0, st
                    assert st["second_walks"] == 0, (form, st)
                    before = st["commits"]
                else:
                    assert not st["active"] and st["commits"] == 0, st
            if more and spec:
                more(plan)
            plan.close()


def test_record_holds_no_weight_and_no_label_count(hip, oracle, monkeypatch):
    """(a)"""
    conn = grid_conn(12, 9)
    for K, step in ((8, 1.5), (60, 1.0)):
        _check(monkeypatch, oracle, {"STEREO_HIP_TRWS_SPEC_SEG": "4"}, _problem("12x9", 108, conn, K, step, 12098 + K), 8.0, forms=("ones", "pair"))


def test_backward_sweep_on_sub_row_descriptors(hip, oracle, monkeypatch):
    """(b)"""
    def pieces(plan):
        nf, nb = _runs(plan)
        print("runs forward", nf, "backward", nb)
        assert nb >= 2 * nf, (nf, nb)   # whole rows forward, pieces of at most 12 of the 38-pixel rows backward
    _check(monkeypatch, oracle, {"STEREO_HIP_TRWS_ROW_CHUNK": "0,12", "STEREO_HIP_TRWS_BLOCKS": "16"},
           _problem("30x40", 1200, grid_conn(30, 40), 8, 1.5, 30408), 8.0, more=pieces)


@pytest.mark.parametrize("K,tol,step", ((3, 3.0, 2.0), (64, 8.0, 1.0)))
def test_last_segment_shorter(K, tol, step, hip, oracle, monkeypatch):
    """(c)"""
    from stereo_amd.trws import spec_schedule
    conn = grid_conn(13, 10)
    with monkeypatch.context() as m:
        m.setenv("STEREO_HIP_TRWS_SPEC_SEG", "4")
        for d in (0, 1):
            s = spec_schedule(130, conn.T, d)
            assert s["nseg"] == 10 and (s["c1"] - s["c0"]) % 4 == 2, s
    _check(monkeypatch, oracle, {"STEREO_HIP_TRWS_SPEC_SEG": "4"}, _problem("13x10", 130, conn, K, step, 13100 + K), tol)


def test_off_grid_family(hip, oracle, monkeypatch):
    """(d)"""
    from stereo_amd.trws import descriptors, spec_schedule
    N, conn = gf.permuted_grid(14, 19, 2)
    with monkeypatch.context() as m:
        m.setenv("STEREO_HIP_TRWS_SPEC_SEG", "4")
        for d in (0, 1):
            s = spec_schedule(N, conn.T, d)
            assert s["nseg"] >= 8, s
            D = np.asarray(descriptors(N, conn.T, d)).reshape(-1, 64)[s["c0"]:s["c1"]]
            assert ((D[:, 2] >> 4) & 15).max() == 4 and ((D[:, 2] >> 8) & 15).max() >= 1
    _check(monkeypatch, oracle, {"STEREO_HIP_TRWS_SPEC_SEG": "4"}, _problem("permuted", N, conn, 8, 1.5, 14198), 8.0)
