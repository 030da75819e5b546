"""The first-principles checker (tests/first_principles.py) is proved here before it judges a kernel.

* Its exact answers agree with each other: dynamic programming on chains against enumeration, the Fraction energy
  against the float sum.
* check_run passes on the CPU oracle, for every instance test_first_principles_gpu.py runs and both message routines.
* The instances are worth running: on at least a quarter of the enumerated grids the first bound is not tight, so the
  bound checks see a bound that moves, and on every one the oracle's bound reaches the optimum within 30 iterations.
* The rounding slack of the bound checks on loopy graphs is what the oracle itself shows, times 1000.
"""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import first_principles as fp

ITERS_GRID = 30
ITERS_MID = 8


def _oracle_run(oracle, p, kernel, iters, mode):
    """iterations 1 .. iters of the oracle as check_run takes them: the energy and bound of every iteration from the
    trace, the labelling of the last one"""
    lab, en, lb, it, trace = oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], p["lam"], iters, -1e300,
                                         mode=mode, want_trace=True)
    assert it == iters and (trace[-1, 0], trace[-1, 1]) == (en, lb)
    runs = [(None, float(e), float(b)) for e, b, _ in trace]
    runs[-1] = (lab.astype(np.int64) - 1, en, lb)
    return runs


def _oracle_mode(minplus):
    return 0 if minplus else 1      # oracle_trws: 0 brute-force (min-plus) messages, 1 the reference's envelopes


# ---- the helpers agree with each other -----------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,K", [(1, 9, 4), (9, 1, 4), (1, 7, 5), (6, 1, 7), (1, 2, 2), (5, 1, 12), (1, 5, 4), (4, 1, 7)])
@pytest.mark.parametrize("kernel", [1, 2])
def test_chain_dp_equals_enumeration(H, W, K, kernel):
    for shared in (True, False):
        p = fp.problem(H, W, K, shared, seed=3)
        opt, x = fp.optimum_exhaustive(p, kernel, p["lam"])
        dp, mm = fp.chain_dp(p, kernel, p["lam"])
        assert dp == opt
        assert np.array_equal(mm.min(axis=1), np.full(H * W, opt))
        assert Fraction(opt) == fp.energy_exact(p, kernel, p["lam"], x)
        # a min-marginal is the optimum with one node held: enumerate that too, at the ends and in the middle
        N = H * W
        for i in (0, N // 2, N - 1) if K ** N <= 4096 else ():
            for k in range(K):
                held = dict(p, unary=p["unary"].copy())
                held["unary"][i, np.arange(K) != k] += 1024.0
                assert fp.optimum_exhaustive(held, kernel, p["lam"])[0] == mm[i, k]


def test_energy_exact_equals_the_float_sum():
    rng = np.random.default_rng(8)
    for H, W, K, shared in ((3, 4, 5, False), (4, 3, 9, True), (1, 9, 64, False), (24, 20, 16, False)):
        p = fp.problem(H, W, K, shared, seed=1)
        for kernel in (1, 2):
            x = rng.integers(0, K, size=H * W)
            a, b = p["conn"][:, 0], p["conn"][:, 1]
            E = np.arange(len(a))
            d = np.abs(p["qprim"][E, x[a]] - p["q"][E, x[b]])
            pair = p["alphas"] * np.minimum(d if kernel == 1 else d * d, p["lam"])
            total = p["unary"][np.arange(H * W), x].sum() + pair.sum()
            assert Fraction(float(total)) == fp.energy_exact(p, kernel, p["lam"], x) == fp.energy_exact_by_terms(p, kernel, p["lam"], x)
    # numbers off every dyadic grid: the sum over one denominator gives way to the definition
    p = dict(fp.problem(3, 4, 5, False), unary=np.random.default_rng(9).uniform(0, 1, (12, 5)) / 3 * 2.0 ** -40)
    x = rng.integers(0, 5, size=12)
    assert fp._scaled_ints(p["unary"].ravel()) is None
    assert fp.energy_exact(p, 1, 0.3, x) == fp.energy_exact_by_terms(p, 1, 0.3, x)


def test_dyadic_problem_is_what_it_says():
    p = fp.problem(3, 4, 5, False)
    assert p["conn"].shape == (17, 2) and len({frozenset(e) for e in p["conn"].tolist()}) == 17
    low, high = p["conn"].min(axis=1), p["conn"].max(axis=1)
    assert set((high - low).tolist()) == {1, 3} and not ((high - low == 1) & (low % 3 == 2)).any()   # node = col * H + row
    assert 0 < (p["conn"][:, 0] > p["conn"][:, 1]).sum() < 17                                   # some rows are swapped
    for name, top in (("unary", 4), ("q", 8), ("qprim", 8)):
        assert np.array_equal(p[name] * 64, np.round(p[name] * 64)) and p[name].min() >= 0 and p[name].max() < top
    s = fp.problem(3, 4, 5, True)
    assert np.all(np.diff(s["positions"]) > 0) and np.array_equal(s["positions"] * 4, np.round(s["positions"] * 4))
    assert np.array_equal(s["q"], np.tile(s["positions"], (17, 1))) and np.array_equal(s["q"], s["qprim"])
    assert p["lam"] in fp.LAMBDAS and set(p["alphas"].tolist()) <= set(fp.ALPHAS)


def test_the_instances_reach_every_kernel_family():
    """the family each GPU instance must run, by first_principles.expected_path, is the library's own rule's answer
    (stereo_trws_family_rule, host only), and the instances cover families 1 to 5"""
    import ctypes as C
    from stereo_amd import _lib
    fn = _lib.lib().stereo_trws_family_rule
    fn.restype = C.c_int
    seen = set()
    for K in fp.CHAIN_K:
        for kernel in (1, 2):
            for shared in (True, False):
                for minplus in (False, True):
                    err = C.create_string_buffer(512)
                    got = fn(C.c_int(kernel), C.c_int(K), C.c_int(int(minplus)), C.c_int(1), C.c_int(1), C.c_int(0),
                             C.c_int(2 if shared else 0), C.c_double(2.0), err, C.c_size_t(512))
                    assert got == fp.expected_path(K, shared, minplus, kernel), (K, kernel, shared, minplus, err.value)
                    seen.add(got)
    assert seen == {0, 1, 2, 3, 4, 5}
    assert [fp.expected_path(K, shared, False, kernel) for _, _, K, kernel, shared in fp.MIDSIZE] == [2, 4, 3, 5]


# ---- chains: the oracle is exact ----------------------------------------------------------------------------------

def _chain_certificate(p, kernel, runs):
    opt, _ = fp.chain_dp(p, kernel, p["lam"])
    for labels, en, lb in runs:
        assert en == opt and lb == opt, (en, lb, opt)
        if labels is not None:
            assert fp.energy_exact(p, kernel, p["lam"], labels) == Fraction(opt)
    fp.check_run(p, kernel, p["lam"], runs, opt, 0.0)


@pytest.mark.parametrize("K", fp.CHAIN_K)
@pytest.mark.parametrize("kernel", [1, 2])
def test_oracle_on_chains(oracle, K, kernel):
    for H, W, shared, minplus in fp.chain_cases(K, kernel):
        p = fp.instance(H, W, K, shared, kernel, minplus)
        _chain_certificate(p, kernel, _oracle_run(oracle, p, kernel, 3, _oracle_mode(minplus)))


@pytest.mark.parametrize("K", fp.CHAIN_K)
def test_oracle_on_the_coarse_chains_of_the_linear_kernel(oracle, K):
    """what the GPU chain test asks of the coarse instances under the linear kernel's exact messages (FINE_BITS): the
    energy is the labelling's, and no labelling beats the optimum; bound and beliefs are held to nothing there"""
    for H, W, shared, minplus in fp.chain_cases(K, 1):
        if not minplus:
            p = fp.problem(H, W, K, shared)
            opt, _ = fp.chain_dp(p, 1, p["lam"])
            for iters in (1, 2, 3):
                (labels, en, _), = _oracle_run(oracle, p, 1, iters, 1)[-1:]
                assert Fraction(float(en)) == fp.energy_exact(p, 1, p["lam"], labels) and en >= opt


@pytest.mark.parametrize("H,W,K", fp.LONG_CHAINS + fp.FEATURE_CHAINS + fp.BATCH_CHAINS[16] + fp.BATCH_CHAINS[96])
def test_oracle_on_long_chains(oracle, H, W, K):
    for kernel in (1, 2):
        for shared in (True, False):
            for minplus in (False, True):
                p = fp.instance(H, W, K, shared, kernel, minplus)
                _chain_certificate(p, kernel, _oracle_run(oracle, p, kernel, 3, _oracle_mode(minplus)))


def _restated_beliefs(oracle, p, kernel, minplus, iters):
    import mm_restate
    N = p["unary"].shape[0]
    opt, mm = fp.chain_dp(p, kernel, p["lam"])
    r = mm_restate.trws_beliefs(oracle, mm_restate.default_impl(oracle, minplus), kernel, p, p["lam"], iters)
    assert r["energy"] == opt and r["lb"] == opt
    assert np.array_equal(r["mm"], mm - opt)
    assert np.array_equal((mm - opt)[np.arange(N), r["argmin"]], np.zeros(N))
    assert np.array_equal(r["confidence"], np.sort(mm - opt, axis=1)[:, 1])


@pytest.mark.parametrize("H,W,K", fp.LONG_CHAINS + fp.FEATURE_CHAINS + fp.BATCH_CHAINS[16] + fp.BATCH_CHAINS[96])
def test_restated_beliefs_on_long_chains(oracle, H, W, K):
    for kernel, shared, minplus in itertools.product((1, 2), (True, False), (False, True)):
        _restated_beliefs(oracle, fp.instance(H, W, K, shared, kernel, minplus), kernel, minplus, 1)


@pytest.mark.parametrize("K", (5, 17) + fp.CHAIN_K)
def test_restated_beliefs_are_the_true_min_marginals_on_chains(oracle, K):
    """the belief definition (restated in tests/mm_restate.py) on a chain: the true min-marginals minus
    the optimum, their first minimum, their second-smallest entry -- what the device is held to"""
    for H, W in fp.CHAIN_SHAPES:
        for kernel, shared, minplus in itertools.product((1, 2), (True, False), (False, True)):
            if fp.expected_path(K, shared, minplus, kernel):
                for iters in ((1, 3) if K <= 256 else (1,)):
                    _restated_beliefs(oracle, fp.instance(H, W, K, shared, kernel, minplus), kernel, minplus, iters)


def test_why_the_linear_kernel_with_exact_messages_runs_on_the_fine_grid(oracle):
    """first_principles.FINE_BITS: on the coarse grid the envelope messages of the linear kernel meet the reference's tie
    rule -- with the reference's own type classes too, where they are built -- while the min-plus messages, and the
    quadratic kernel's envelopes, keep every property on the same inputs"""
    import mm_restate
    # a chain: the bound ends ABOVE the optimum
    p = fp.problem(9, 1, 2, True, 0, bits=6)
    opt, _ = fp.chain_dp(p, 1, p["lam"])
    _chain_certificate(p, 1, _oracle_run(oracle, p, 1, 3, 0))
    _chain_certificate(p, 2, _oracle_run(oracle, p, 2, 3, 1))
    env = _oracle_run(oracle, p, 1, 3, 1)
    assert (env[-1][1], env[-1][2]) == (9.125, 9.625) and opt == 9.125
    if oracle.have_ref_types():
        ref = oracle.trws(1, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], p["lam"], 3, -1e300, mode=1, use_ref_types=True)
        assert (ref[1], ref[2]) == (env[-1][1], env[-1][2])
    # a chain: energy and bound are the optimum, the beliefs are not the min-marginals
    p = fp.problem(1, 9, 17, True, 0, bits=6)
    opt, mm = fp.chain_dp(p, 1, p["lam"])
    r = mm_restate.trws_beliefs(oracle, "envelope", 1, p, p["lam"], 1)
    assert r["energy"] == opt and r["lb"] == opt and not np.array_equal(r["mm"], mm - opt)
    assert np.array_equal(mm_restate.trws_beliefs(oracle, "brute", 1, p, p["lam"], 1)["mm"], mm - opt)
    # a grid: the bound falls (by 2.3e-3 in iteration 8)
    H, W, K, kernel, shared = fp.MIDSIZE[0]
    assert kernel == 1
    p = fp.problem(H, W, K, shared, 0, bits=6)
    fp.check_run(p, 1, p["lam"], _oracle_run(oracle, p, 1, ITERS_MID, 0), None, fp.SLACK)
    with pytest.raises(AssertionError, match="bound fell"):
        fp.check_run(p, 1, p["lam"], _oracle_run(oracle, p, 1, ITERS_MID, 1), None, fp.SLACK)


# ---- enumerated grids ----------------------------------------------------------------------------------------------

_grid = {}


def _grid_runs(oracle):
    """every enumerated instance on the oracle, both message routines, once: [(case, p, opt, {mode: runs})]"""
    if not _grid:
        out = []
        for case in fp.grid_cases():
            H, W, K, kernel, shared, minplus, seed = case
            p = fp.problem(H, W, K, shared, seed)
            opt, _ = fp.optimum_exhaustive(p, kernel, p["lam"])
            out.append((case, p, opt, {mode: _oracle_run(oracle, p, kernel, ITERS_GRID, mode) for mode in (0, 1)}))
        _grid["runs"] = out
    return _grid["runs"]


def test_oracle_on_enumerated_grids(oracle):
    for case, p, opt, by_mode in _grid_runs(oracle):
        for mode, runs in by_mode.items():
            fp.check_run(p, case[3], p["lam"], runs, opt, fp.SLACK)


def test_the_grids_have_a_bound_that_moves_and_arrives(oracle):
    loose = 0
    for case, p, opt, by_mode in _grid_runs(oracle):
        runs = by_mode[_oracle_mode(case[5])]
        loose += runs[0][2] < opt - 2.0 ** -10
        for mode, r in by_mode.items():
            assert r[-1][2] >= opt * (1 - 1e-9), (case, mode, r[-1][2], opt)
    n = len(_grid_runs(oracle))
    print("first bound not tight on %d of %d enumerated grids" % (loose, n))
    assert n == 48 and 4 * loose >= n, (loose, n)


def test_the_slack_is_the_measured_one(oracle):
    over = dip = 0.0
    for case, p, opt, by_mode in _grid_runs(oracle):
        for runs in by_mode.values():
            o, d = fp.violations(runs, opt)
            over, dip = max(over, o), max(dip, d)
    print("worst relative excess of a bound over the optimum %.3g, worst dip %.3g; recorded %.3g" % (over, dip, fp.MEASURED_VIOLATION))
    assert fp.SLACK == 1000 * fp.MEASURED_VIOLATION
    assert 0 < fp.SLACK < 2.0 ** -14 * 1e-6
    assert max(over, dip) <= fp.SLACK / 1000 * 2


# ---- mid-size grids, nobody knows the optimum --------------------------------------------------------------------

@pytest.mark.parametrize("H,W,K,kernel,shared", fp.MIDSIZE)
def test_oracle_on_midsize_grids(oracle, H, W, K, kernel, shared):
    p = fp.instance(H, W, K, shared, kernel, False)
    for mode in (0, 1):
        fp.check_run(p, kernel, p["lam"], _oracle_run(oracle, p, kernel, ITERS_MID, mode), None, fp.SLACK)


# ---- grids whose rows are walked in pieces -------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,K,chunk,resident", [fp.PIECES_SMALL, fp.PIECES_TALL])
def test_oracle_on_the_grids_walked_in_pieces(oracle, H, W, K, chunk, resident):
    """... and the host-side schedule says that they are: sub-row runs in either direction at this chunk length and
    this many resident workgroups, more of them than workgroups"""
    from stereo_amd.trws import schedule, schedule_chunked
    for kernel, shared in ((1, False), (2, True)) if H * W > 10000 else itertools.product((1, 2), (True, False)):
        p = fp.instance(H, W, K, shared, kernel, False)
        for d in (0, 1):
            rows = len(schedule(H * W, p["conn"].T, d)["ticket_run"])
            pieces = schedule_chunked(H * W, p["conn"].T, d, chunk, resident)
            assert pieces["chunked"] and pieces["chunk"] == chunk and len(pieces["ticket_run"]) > max(rows, resident)
            assert int(np.diff(pieces["run_ptr"]).min()) >= 1
        for mode in (0, 1):
            fp.check_run(p, kernel, p["lam"], _oracle_run(oracle, p, kernel, 4 if H * W > 10000 else ITERS_MID, mode), None, fp.SLACK)
