"""The CPU yardstick of the min-marginal tests (tests/mm_restate.py).

First: after t iterations the restatement's labels, energy and bound are oracle.trws's, bit for bit, so the beliefs it
records come from the very message state the reference would have.  Then its own invariants.
"""
import numpy as np
import pytest

from helpers import grid_conn, trws_problem
from mm_restate import default_impl, oracle_trws, trws_beliefs

CASES = [
    # id, kernel, kind, H, W, K, tol, ordering, minplus
    ("lin-general", 1, "general", 5, 6, 7, 3.0, 0, False),
    ("quad-general", 2, "general", 4, 7, 6, 9.0, 0, False),
    ("lin-fronto", 1, "fronto", 6, 5, 9, 2.5, 0, False),
    ("quad-fronto", 2, "fronto", 5, 5, 5, 4.0, 0, False),
    ("lin-index-order", 1, "general", 5, 6, 6, 3.0, 1, False),
    ("lin-minplus", 1, "fronto", 5, 6, 8, 3.0, 0, True),
    ("K1", 1, "general", 4, 5, 1, 3.0, 0, False),
]


def _problem(kind, seed, H, W, K):
    return trws_problem(seed, H, W, K, kind=kind)


def _isolated(seed=5, H=4, W=5, K=6):
    """A grid plus one node with no edge (the last one)."""
    p = trws_problem(seed, H, W, K)
    rng = np.random.default_rng(seed + 100)
    p["unary"] = np.vstack([p["unary"], rng.uniform(0, 40, size=(1, K))])
    return p


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("t", [1, 2, 5])
def test_restatement_is_the_oracle(case, t, oracle):
    name, kernel, kind, H, W, K, tol, ordering, minplus = case
    p = _problem(kind, 11 + K, H, W, K)
    impl = default_impl(oracle, minplus)
    r = trws_beliefs(oracle, impl, kernel, p, tol, t, ordering=ordering)
    lab, en, lb, it = oracle_trws(oracle, impl, kernel, p, tol, t, ordering=ordering)
    assert np.array_equal(r["labels"], lab)
    assert r["energy"] == en and r["lb"] == lb and r["iterations"] == it == t


def test_restatement_with_an_isolated_node(oracle):
    p = _isolated()
    impl = default_impl(oracle)
    for t in (1, 3):
        r = trws_beliefs(oracle, impl, 1, p, 3.0, t)
        lab, en, lb, it = oracle_trws(oracle, impl, 1, p, 3.0, t)
        assert np.array_equal(r["labels"], lab) and r["energy"] == en and r["lb"] == lb
        # nothing reaches the isolated node: its belief is its unary row
        assert np.array_equal(r["D"][-1], p["unary"][-1])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_invariants(case, oracle):
    name, kernel, kind, H, W, K, tol, ordering, minplus = case
    p = _problem(kind, 3 + K, H, W, K)
    r = trws_beliefs(oracle, default_impl(oracle, minplus), kernel, p, tol, 2, ordering=ordering)
    N = H * W
    mm, conf, am = r["mm"], r["confidence"], r["argmin"]
    assert mm.shape == (N, K) and conf.shape == (N,) and am.shape == (N,)
    assert (mm >= 0).all()
    assert (mm[np.arange(N), am] == 0).all()
    # the first zero is the argmin
    assert all(np.flatnonzero(mm[i] == 0)[0] == am[i] for i in range(N))
    if K == 1:
        assert np.isinf(conf).all() and (conf > 0).all()
    else:
        assert np.array_equal(conf, np.sort(mm, axis=1)[:, 1])
        assert (conf >= 0).all()
    # the beliefs are the forward pass's Di: normalising them gives mm exactly
    assert np.array_equal(mm, r["D"] - r["D"].min(axis=1)[:, None])


def test_index_order_structure_matches_the_oracle_orientation(oracle):
    """With ordering 0 the restatement's own walk over oracle.trws_structure equals the oracle's run above; for
    ordering 1 the orientation is restated in Python.  Cross-check it: on a graph whose automatic order IS the index
    order (a path), both structures agree."""
    from mm_restate import _index_order_structure, _structure
    N = 7
    conn = np.array([[i, i + 1] for i in range(N - 1)])
    a = _structure(oracle, N, conn, 0)
    b = _index_order_structure(N, conn)
    if a["order"] == b["order"]:
        assert a["fwd"] == b["fwd"] and a["bwd"] == b["bwd"] and a["dir"] == b["dir"] and a["tail"] == b["tail"]
    g = grid_conn(3, 4)
    s = _index_order_structure(12, g)
    # every edge is oriented from the lower to the higher index and sits in exactly one list of each kind
    assert sorted(e for l in s["fwd"] for e in l) == list(range(len(g)))
    assert sorted(e for l in s["bwd"] for e in l) == list(range(len(g)))
    for i, l in enumerate(s["fwd"]):
        assert all(s["tail"][e] == i for e in l)


def test_six_output_gateway_compiles_and_checks_its_arguments():
    """mex/trws_minmarginals_mex.cpp: trws_mex's inputs and checks, six outputs; trws_mex keeps the reference's four."""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexhost"))
    import host
    assert os.path.exists(host.build("trws_minmarginals_mex"))
    g = host.Gateway("trws_minmarginals_mex")
    K, N, E = 3, 4, 2
    args = [np.int32(1), np.zeros((K, N)), np.zeros((2, E), np.uint32), np.zeros((K, E)), np.zeros((K, E)), np.zeros((E, 1)),
            2.0, {"maxiter": 5.0}]
    with pytest.raises(host.MexError, match="nrhs == 8"):
        g.call(6, np.int32(1))
    with pytest.raises(host.MexError, match="nlhs == 6"):
        g.call(4, *args)
    with pytest.raises(host.MexError, match="int32"):
        g.call(6, *([1.0] + args[1:]))
    with pytest.raises(host.MexError, match="unary.M == q.M"):
        g.call(6, *(args[:3] + [np.zeros((K + 1, E))] + args[4:]))
    with pytest.raises(host.MexError, match="nlhs == 4"):
        host.Gateway("trws_mex").call(6, *args)


def test_bindings_exist():
    from stereo_amd import _lib
    from stereo_amd.trws import TrwsPlan
    L = _lib.lib()
    for n in ("stereo_trws_min_marginals", "stereo_trws_plan_keep_min_marginals", "stereo_trws_plan_min_marginals",
              "stereo_trws_plan_min_marginals_device"):
        assert hasattr(L, n)
    for m in ("keep_min_marginals", "min_marginals", "min_marginals_device"):
        assert callable(getattr(TrwsPlan, m))
