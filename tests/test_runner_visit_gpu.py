"""-m gpu: the visit of the speculative schedule's runner, K <= 64 (trws_spec.h: run_visit_m,
run_visit_p).

The runner decides no result: the segments recompute every visit with the certified routine, and a row or label of the
runner's that is not the reference's costs a second walk, never a bit.  Parity with the oracle alone therefore cannot
see a runner that has gone wrong -- it would only be slow.  Every case asserts three things:
  (i)   labels, energy and lower bound after EACH of 3 iterations are the CPU oracle's bit for bit, on the speculative
        schedule and on the plain one (STEREO_HIP_TRWS_SPEC=0);
  (ii)  plan.spec_stats() is active with commits and runner visits (and not active on the plain schedule);
  (iii) second_walks == 0: every row and label the runner handed to a segment was the one the segment in front
        produced.
Unaries are continuous random numbers (no exact ties, so the plain min-plus row of the runner is the reference's
envelope).  The seeds are 1000 H + 10 W + K as in test_di_prefix_gpu.py; all of them gave second_walks == 0 with the
library before round 11 as well, none was replaced.

Cases, the smallest that reach each path of the visit:
  grids     12 x 9 and 9 x 12 with STEREO_HIP_TRWS_SPEC_SEG=4 (9 segments per direction), 30 x 40 with the default
            segment of 16 visits (8 segments);
  K         3, 8, 60, 64 (lanes beyond K, up to none);
  window    tol 3: at most 4 entries per side, the G = 1 routine; tol 8: 8 entries, G = 2.  The runner walks the window
            in groups of four entries and keeps the speculative schedule only if every index distance up to the end of
            the last group that lies beyond the window costs more than the truncation (trws_inputs.hip: analyse_window):
            with unit spacing K = 3 has no such tol among 3 and 8, and K = 8 none for tol 8.  Those cases space the
            labels wider -- K = 3, tol 3, step 2 (window 1); K = 8, tol 8, step 1.5 (window 5, G = 2) -- which also
            covers a step that is not 1;
  weights   "ones"; "pair": independent per directed edge, so the two edges of a pair differ and the loader stages two
            messages (nmsg == 2); "zero": 0 on both edges of every third pair of neighbouring border pixels (alpha == 0:
            the constant row); "alt": 1 and 1.5 by the parity of row + column, so consecutive chain edges differ and the
            cached alpha d step / alpha lambda are refreshed on every visit;
  family    "single-grid" of tests/graph_families.py (30 x 40, every pair listed once), whose plan keeps the speculative
            schedule: chain nodes with ONE handed-over row.

The `kinds` keys (trws_spec.h: kRsKinds) the loader stages along the chain, from a host-side walk of the descriptors
(the same for every K and weight form), as key: visits, forward | backward:
  12 x 9          0x0: 1, 0x20098: 36, 0x41908: 1  |  0x0: 1, 0x30098: 13, 0x30908: 21, 0x20098: 3
  9 x 12          0x0: 1, 0x20098: 36, 0x41908: 1  |  0x0: 1, 0x30098: 19, 0x30908: 15, 0x20098: 3
  30 x 40         0x0: 1, 0x20098: 134, 0x41908: 1 |  0x0: 1, 0x30098: 75, 0x30908: 57, 0x20098: 3
  single-grid     0x0: 1, 0x10008: 134, 0x20008: 1 |  0x0: 1, 0x10008: 98, 0x20008: 37   (the generic loop of the dispatch)
so the forward fast path (0x20098), both backward fast paths (0x30098, 0x30908), the chain of tests behind them
(0x20098 backward, 0x41908 forward) and the generic loop are all walked."""
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


def _weights(H, W, conn, form, rng):
    """per directed edge; node id = column * H + row (helpers.grid_conn)"""
    E = conn.shape[0]
    if form == "ones":
        return np.ones(E)
    if form == "pair":
        a = rng.uniform(0.5, 2.0, size=E)
        w = {(int(i), int(j)): x for (i, j), x in zip(conn, a)}
        assert any((j, i) in w and w[(j, i)] != x for (i, j), x in w.items())
        return a
    lo = conn.min(axis=1)
    row, col = conn % H, conn // H
    if form == "zero":
        border = ((row == 0) | (row == H - 1) | (col == 0) | (col == W - 1)).all(axis=1)
        a = np.where(border & (lo % 3 == 0), 0.0, 1.0)
        assert 0 < (a == 0).sum() < border.sum()
        return a
    assert form == "alt"
    return np.where((lo % H + lo // H) % 2 == 0, 1.0, 1.5)


_problems, _wanted = {}, {}


def _problem(name, H, W, K, step, form):
    """dict(unary (N,K), conn (E,2), q, qprim (E,K), alphas (E,), pos); built once per key, never changed"""
    key = (name, H, W, K, step, form)
    if key not in _problems:
        N, conn = (H * W, grid_conn(H, W)) if name == "grid" else gf.single_grid(H, W)
        rng = np.random.default_rng(1000 * H + 10 * W + K)
        unary = rng.uniform(0, 40, size=(N, K))
        pos = np.arange(K, dtype=np.float64) * step
        q = np.tile(pos, (conn.shape[0], 1))
        _problems[key] = dict(key=key, unary=unary, conn=conn, q=q, qprim=q.copy(), alphas=_weights(H, W, conn, form, rng), pos=pos)
    return _problems[key]


def _oracle(oracle, p, tol):
    """the oracle's (labels, energy, bound, iterations) after 1, 2 and 3 iterations"""
    key = (tol,) + p["key"]
    if key not in _wanted:
        _wanted[key] = [oracle.trws(1, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], tol, n, NEVER, mode=1) for n in range(1, ITERS + 1)]
    return _wanted[key]


def _walk(monkeypatch, env, p, tol):
    """one plan, one iteration at a time: its results after each, its spec_stats() at the end"""
    from stereo_amd.trws import TrwsPlan
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        N, K = p["unary"].shape
        plan = TrwsPlan(1, K, N, p["conn"].T)
        plan.upload(p["unary"].T, p["alphas"], tol, positions=p["pos"])
        assert plan.path() == 2, "path %d, expected the K <= 64 kernel" % plan.path()
        got = []
        for _ in range(ITERS):
            plan.iterate(1, max_relgap=NEVER)
            got.append(plan.result())
        stats = plan.spec_stats()
        plan.close()
    return got, stats


def _is(got, want, what):
    lab, en, lb, it = got
    assert it == want[3], what
    assert np.array_equal(lab, want[0]), "%s: labels differ at %d of %d nodes" % (what, int((lab != want[0]).sum()), lab.size)
    assert en == want[1] and lb == want[2], (what, (en, lb), want[1:3])


def _check(monkeypatch, oracle, p, tol, seg):
    from stereo_amd.trws import spec_schedule
    base = {"STEREO_HIP_TRWS_SPEC_SEG": seg} if seg else {}
    with monkeypatch.context() as m:
        for k, v in base.items():
            m.setenv(k, v)
        assert all(spec_schedule(p["unary"].shape[0], p["conn"].T, d)["nseg"] >= 8 for d in (0, 1))
    want = _oracle(oracle, p, tol)
    spec, st = _walk(monkeypatch, base, p, tol)
    plain, st0 = _walk(monkeypatch, dict(base, STEREO_HIP_TRWS_SPEC="0"), p, tol)
    print("speculative", st, "plain", st0)
    for n in range(ITERS):
        _is(spec[n], want[n], "speculative schedule, iteration %d" % (n + 1))
        _is(plain[n], want[n], "plain schedule, iteration %d" % (n + 1))
    assert st["active"] and st["commits"] > 0 and st["runner_visits"] > 0, st
    assert not st0["active"] and st0["commits"] == 0, st0
    assert st["second_walks"] == 0, st


# H, W, segment, K, tol, step, weights
CASES = [
    (12, 9, "4", 3, 3.0, 2.0, "ones"), (12, 9, "4", 8, 3.0, 1.0, "pair"), (12, 9, "4", 8, 8.0, 1.5, "zero"), (12, 9, "4", 60, 8.0, 1.0, "alt"),
    (12, 9, "4", 64, 3.0, 1.0, "zero"), (12, 9, "4", 64, 8.0, 1.0, "ones"),
    (9, 12, "4", 3, 3.0, 2.0, "zero"), (9, 12, "4", 8, 8.0, 1.5, "alt"), (9, 12, "4", 60, 3.0, 1.0, "ones"), (9, 12, "4", 64, 8.0, 1.0, "pair"),
    (30, 40, None, 3, 3.0, 2.0, "alt"), (30, 40, None, 8, 8.0, 1.5, "pair"), (30, 40, None, 60, 8.0, 1.0, "ones"), (30, 40, None, 60, 3.0, 1.0, "pair"),
    (30, 40, None, 64, 8.0, 1.0, "zero"), (30, 40, None, 64, 3.0, 1.0, "alt"),
]


@pytest.mark.parametrize("H,W,seg,K,tol,step,form", CASES, ids=["%dx%d-seg%s-K%d-tol%g-step%g-%s" % (c[0], c[1], c[2] or "16", *c[3:]) for c in CASES])
def test_runner_visit(H, W, seg, K, tol, step, form, hip, oracle, monkeypatch):
    _check(monkeypatch, oracle, _problem("grid", H, W, K, step, form), tol, seg)


@pytest.mark.parametrize("K,tol", ((60, 8.0), (8, 3.0)))
def test_runner_visit_single_edged_grid(K, tol, hip, oracle, monkeypatch):
    """graph_families.single_grid: every pair of pixels listed once -- one handed-over row per chain node, keys 0x10008
    and 0x20008, which take the generic loop of the dispatch"""
    _check(monkeypatch, oracle, _problem("single-grid", 30, 40, K, 1.0, "ones"), tol, None)
