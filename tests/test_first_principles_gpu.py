"""-m gpu: TRW-S on the device against answers that follow from the energy alone (tests/first_principles.py).

No oracle here.  Chains are trees: after any number of iterations energy == bound == the optimum of a plain dynamic
programme, bit for bit, and the node beliefs are the true min-marginals minus the optimum -- on every kernel family at
the label counts where families change, and through strips, batches, a saved state and the gateway.  Grids small enough
to enumerate: the reported energy is the exact energy of the reported labelling, the bound stays below the optimum,
never falls and arrives.  Mid-size grids: the same without an optimum.  test_first_principles_cpu.py holds the CPU
oracle to every check made here, on the same instances, and measures the rounding slack (first_principles.SLACK).

The last test requires that the module ran kernel families 1 to 5: run the file as a whole.
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import first_principles as fp

pytestmark = pytest.mark.gpu

NEVER = -1e300
ENV = ("STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_MESSAGES",
       "STEREO_HIP_TRWS_BLOCKS", "STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_CERTIFICATE", "STEREO_HIP_TRWS_DEBUG",
       "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_ITERATE_AHEAD", "STEREO_HIP_TRWS_BELIEFS_STRIPS")

_paths = set()     # every kernel family a plan of this module ran on


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _mode(minplus):
    from stereo_amd.trws import MESSAGES_EXACT, MESSAGES_MINPLUS
    return MESSAGES_MINPLUS if minplus else MESSAGES_EXACT


def _upload(solver, p):
    if p["positions"] is not None:
        solver.upload(p["unary"].T, p["alphas"], p["lam"], positions=p["positions"])
    else:
        solver.upload(p["unary"].T, p["alphas"], p["lam"], q=p["q"].T, qprim=p["qprim"].T)


def _plan(p, kernel, minplus=False, beliefs=False, env=None):
    """a plan with the problem's inputs; `env` holds while the plan is created"""
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        plan = TrwsPlan(kernel, K, N, p["conn"].T, message_mode=_mode(minplus))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if beliefs:
        plan.keep_min_marginals(True)
    _upload(plan, p)
    _paths.add(plan.path())
    return plan


def _shown(solver):
    """(labels zero based, energy, bound) as check_run takes them"""
    lab, en, lb, _ = solver.result()
    return lab.astype(np.int64) - 1, en, lb


# ---- chains --------------------------------------------------------------------------------------------------------

_dp = {}


def _chain_answer(p, kernel):
    key = (id(p), kernel)
    if key not in _dp:
        _dp[key] = fp.chain_dp(p, kernel, p["lam"])
    return _dp[key]


def _certificate(p, kernel, shown, beliefs, what):
    """one reading of a solver on a chain against the dynamic programme: everything bitwise"""
    opt, mm_true = _chain_answer(p, kernel)
    labels, en, lb = shown
    print("%s: energy %r bound %r optimum %r" % (what, en, lb, opt))
    assert en == opt and lb == opt, (what, en, lb, opt)
    assert fp.energy_exact(p, kernel, p["lam"], labels) == Fraction(opt), what
    if beliefs is not None:
        mm, conf, arg = beliefs
        want = mm_true - opt
        assert np.array_equal(mm.T, want), (what, float(np.abs(mm.T - want).max()))
        if arg is not None:     # (the gateway returns no argmin)
            assert np.array_equal(want[np.arange(len(arg)), np.asarray(arg, dtype=np.int64) - 1], np.zeros(len(arg))), what
        assert np.array_equal(conf, np.sort(want, axis=1)[:, 1]), what


def _certify_run(p, kernel, solver, what, beliefs=True, first=1):
    """after `first` iteration(s), and again after two further ones"""
    for iters in (first, 2):
        done, stopped = solver.iterate(iters, NEVER)
        assert (done, stopped) == (iters, False)
        _certificate(p, kernel, _shown(solver), solver.min_marginals() if beliefs else None, what)


@pytest.mark.parametrize("K", fp.CHAIN_K)
@pytest.mark.parametrize("kernel", [1, 2])
def test_chains_solve_exactly(hip, K, kernel):
    cases = fp.chain_cases(K, kernel)
    assert len(cases) == (4 if K > 512 else 8)
    for H, W, shared, minplus in cases:
        p = fp.instance(H, W, K, shared, kernel, minplus)
        plan = _plan(p, kernel, minplus, beliefs=True)
        what = "%dx%d K %d kernel %d %s %s path %d" % (H, W, K, kernel, "shared" if shared else "per-edge",
                                                      "minplus" if minplus else "exact", plan.path())
        assert plan.path() == fp.expected_path(K, shared, minplus, kernel), what
        _certify_run(p, kernel, plan, what)
        plan.close()
        if kernel == 1 and not minplus:
            # the coarse grid (first_principles.FINE_BITS): exact ties, the reference's tie rule, bound and beliefs not
            # held to anything -- the energy is still the exact energy of the labelling, and no labelling beats the optimum
            coarse = fp.problem(H, W, K, shared)
            plan = _plan(coarse, kernel)
            for _ in range(3):
                plan.iterate(1, NEVER)
                labels, en, lb = _shown(plan)
                assert Fraction(float(en)) == fp.energy_exact(coarse, kernel, coarse["lam"], labels), what
                assert en >= _chain_answer(coarse, kernel)[0], what
            plan.close()


def test_no_family_takes_positions_per_edge_above_512_labels(hip):
    from stereo_amd.trws import TrwsPlan
    p = fp.problem(1, 9, 513, True)
    q = np.ascontiguousarray(p["q"].T)
    plan = TrwsPlan(1, 513, 9, p["conn"].T)
    with pytest.raises(hip.StereoHipError, match=re.escape("K must be in [1, 512]")):
        plan.upload(p["unary"].T, p["alphas"], p["lam"], q=q, qprim=q[::-1].copy())
    plan.close()


@pytest.mark.parametrize("H,W,K", fp.LONG_CHAINS)
def test_long_chains_solve_exactly(hip, H, W, K):
    """one long serial run (a chain is a single run in either direction, whatever H and W say): hundreds of visits by
    one workgroup, the hand-over from visit to visit; rows in pieces and the ticket dispenser: test_rows_walked_in_pieces"""
    for kernel in (1, 2):
        for shared in (True, False):
            p = fp.instance(H, W, K, shared, kernel, False)
            plan = _plan(p, kernel, beliefs=True)
            assert plan.path() == 2
            _certify_run(p, kernel, plan, "%dx%d K %d kernel %d shared %d" % (H, W, K, kernel, shared))
            plan.close()


# ---- the same certificate through each feature ----------------------------------------------------------------------

FEATURES = [(H, W, K, kernel, shared) for H, W, K in fp.FEATURE_CHAINS for kernel in (1, 2) for shared in (True, False)]


def _strip_rule(kernel, K, minplus, shared, lam):
    """(family, refusal) of the library's own rule (stereo_trws_family_rule, host only) for a row strip with these inputs"""
    from stereo_amd import _lib
    fn = _lib.lib().stereo_trws_family_rule
    fn.restype = C.c_int
    err = C.create_string_buffer(512)
    fam = fn(C.c_int(kernel), C.c_int(K), C.c_int(int(minplus)), C.c_int(1), C.c_int(1), C.c_int(1), C.c_int(2 if shared else 0),
             C.c_double(lam), err, C.c_size_t(512))
    return fam, err.value.decode()


@pytest.mark.parametrize("H,W,K,kernel,shared", FEATURES)
@pytest.mark.parametrize("G", [2, 3])
def test_chain_across_strip_borders(hip, G, H, W, K, kernel, shared):
    from stereo_amd.strips import make_strips
    refused = 0
    for minplus in (False, True):
        p = fp.instance(H, W, K, shared, kernel, minplus)
        family, why = _strip_rule(kernel, K, minplus, shared, p["lam"])
        what = "G %d K %d kernel %d shared %d minplus %d" % (G, K, kernel, shared, minplus)
        if not family:      # refused by rule: the refusal is the rule's, word for word
            assert "row strips" in why, (what, why)
            strips = None
            with pytest.raises(hip.StereoHipError, match=re.escape(why)):
                strips = make_strips(kernel, K, H, W, p["conn"].T, G, message_mode=_mode(minplus))
                _upload(strips, p)
            if strips is not None:
                strips.close()
            refused += 1
            continue
        strips = make_strips(kernel, K, H, W, p["conn"].T, G, message_mode=_mode(minplus))
        strips.keep_min_marginals(True)
        _upload(strips, p)
        assert strips.path() == family and family == fp.expected_path(K, shared, minplus, kernel), what
        _paths.add(strips.path())
        _certify_run(p, kernel, strips, what)
        strips.close()
    # exact messages always run; min-plus ones only on the wide kernel (64 < K <= 256, linear, shared positions)
    assert refused == (0 if (K == 96 and kernel == 1 and shared) else 1)


@pytest.mark.parametrize("K", sorted(fp.BATCH_CHAINS))
@pytest.mark.parametrize("kernel", [1, 2])
def test_chains_in_a_batch(hip, K, kernel):
    from stereo_amd.trws import TrwsBatch
    shapes = [s for s in fp.FEATURE_CHAINS if s[2] == K] + list(fp.BATCH_CHAINS[K])
    problems = [fp.instance(h, w, k, False, kernel, False) for h, w, k in shapes]
    plans = [_plan(p, kernel, beliefs=True) for p in problems]
    assert {pl.path() for pl in plans} == {2 if K == 16 else 4}
    with TrwsBatch(plans) as batch:
        for iters in (1, 2):
            assert batch.iterate(iters, NEVER) == [iters] * 3
            for (h, w, k), p, pl in zip(shapes, problems, plans):
                _certificate(p, kernel, _shown(pl), pl.min_marginals(), "batch member %dx%d K %d kernel %d" % (h, w, k, kernel))
    for pl in plans:
        pl.close()


@pytest.mark.parametrize("H,W,K,kernel,shared", FEATURES)
def test_chain_through_a_saved_state(hip, H, W, K, kernel, shared):
    """save after iteration 1, load into a fresh plan of ANOTHER family (the generic kernel), one more iteration"""
    p = fp.instance(H, W, K, shared, kernel, False)
    a = _plan(p, kernel)
    assert a.path() == fp.expected_path(K, shared, False, kernel) != 1
    a.iterate(1, NEVER)
    _certificate(p, kernel, _shown(a), None, "before the save")
    state = a.save_state()
    a.close()
    b = _plan(p, kernel, beliefs=True, env={"STEREO_HIP_TRWS_FAST": "0"})
    assert b.path() == 1
    b.load_state(state)
    _certificate(p, kernel, _shown(b), None, "after the load")
    assert b.iterate(1, NEVER) == (1, False)
    assert b.result()[3] == 2
    _certificate(p, kernel, _shown(b), b.min_marginals(), "one iteration after the load")
    b.close()


@pytest.mark.parametrize("H,W,K,kernel,shared", FEATURES)
def test_chain_through_the_gateway(hip, monkeypatch, H, W, K, kernel, shared):
    """stereo_trws, plain and with STEREO_HIP_GPUS=2.  A 24 x 1 column shows the gateway no horizontal edge to read the
    image height from, so it stays on one plan either way (the sharded gateway: test_midsize_grids)."""
    from stereo_amd import _lib
    p = fp.instance(H, W, K, shared, kernel, False)
    args = (kernel, p["unary"].T, p["conn"].T + 1, p["q"].T, p["qprim"].T, p["alphas"], p["lam"], dict(maxiter=3, max_relgap=0))
    for gpus in (None, "2"):
        if gpus:
            monkeypatch.setenv("STEREO_HIP_GPUS", gpus)
        lab, en, lb, it = hip.trws(*args)
        assert it == 3 and int(_lib.lib().stereo_trws_gateway_strips()) == 1
        _certificate(p, kernel, (lab.astype(np.int64) - 1, en, lb), None, "gateway GPUS %s" % gpus)
        lab, en, lb, it, mm, conf = hip.trws(*args, min_marginals=True)
        _certificate(p, kernel, (lab.astype(np.int64) - 1, en, lb), (mm, conf, None), "gateway with beliefs GPUS %s" % gpus)


# ---- enumerated grids -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,K", fp.GRID_SHAPES)
def test_enumerated_grids(hip, H, W, K):
    cases = [c for c in fp.grid_cases() if c[:3] == (H, W, K)]
    assert len(cases) == 8
    for _, _, _, kernel, shared, minplus, seed in cases:
        p = fp.problem(H, W, K, shared, seed)
        opt, _ = fp.optimum_exhaustive(p, kernel, p["lam"])
        plan = _plan(p, kernel, minplus)
        assert plan.path() == (1 if minplus else 2)
        runs = []
        for _ in range(30):
            assert plan.iterate(1, NEVER) == (1, False)
            runs.append(_shown(plan))
        plan.close()
        over, dip = fp.violations(runs, opt)
        print("%dx%d K %d kernel %d shared %d minplus %d seed %d: optimum %r, bounds %r .. %r, energies %r .. %r, excess %.3g dip %.3g"
              % (H, W, K, kernel, shared, minplus, seed, opt, runs[0][2], runs[-1][2], runs[0][1], runs[-1][1], over, dip))
        fp.check_run(p, kernel, p["lam"], runs, opt, fp.SLACK)
        # the rounding the device shows is the oracle's: below twice what the oracle was measured at, as the oracle is held
        assert max(over, dip) <= 2 * fp.MEASURED_VIOLATION, (over, dip)


# ---- mid-size grids -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,K,kernel,shared", fp.MIDSIZE)
def test_midsize_grids(hip, monkeypatch, H, W, K, kernel, shared):
    from stereo_amd import _lib
    p = fp.instance(H, W, K, shared, kernel, False)
    plan = _plan(p, kernel)
    assert plan.path() == fp.expected_path(K, shared, False, kernel)
    runs = []
    for _ in range(8):
        assert plan.iterate(1, NEVER) == (1, False)
        runs.append(_shown(plan))
    plan.close()
    print("%dx%d K %d kernel %d: bounds %r, energies %r" % (H, W, K, kernel, [r[2] for r in runs], [r[1] for r in runs]))
    fp.check_run(p, kernel, p["lam"], runs, None, fp.SLACK)
    if K <= 256:
        # the gateway cuts this grid into two row strips by itself: its energy is its labelling's, its bound below every energy seen
        monkeypatch.setenv("STEREO_HIP_GPUS", "2")
        lab, en, lb, it = hip.trws(kernel, p["unary"].T, p["conn"].T + 1, p["q"].T, p["qprim"].T, p["alphas"], p["lam"],
                                   dict(maxiter=8, max_relgap=NEVER))
        assert it == 8 and int(_lib.lib().stereo_trws_gateway_strips()) == 2
        assert Fraction(float(en)) == fp.energy_exact(p, kernel, p["lam"], lab.astype(np.int64) - 1)
        tol = fp.SLACK * max(1.0, abs(min(r[1] for r in runs)))
        assert all(lb <= r[1] + tol for r in runs) and lb <= en + tol and lb >= runs[0][2] - tol


# ---- grids whose rows are walked in pieces ---------------------------------------------------------------------------

def _plan_runs(plan):
    """(forward, backward): the runs the plan's own launches hand out as tickets"""
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


@pytest.mark.parametrize("tall", [False, True])
def test_rows_walked_in_pieces(hip, monkeypatch, tall):
    """Sub-row runs and the ticket dispenser (first_principles.PIECES_SMALL, PIECES_TALL): more runs than resident
    workgroups, rows cut into pieces whose hand-over goes through memory.  The plan says that it walks pieces -- as many
    runs as the host-side schedule has pieces -- and the run keeps every property that needs no optimum."""
    from stereo_amd import _lib
    from stereo_amd.trws import schedule, schedule_chunked
    H, W, K, chunk, resident = fp.PIECES_TALL if tall else fp.PIECES_SMALL
    if tall:    # as a plan comes: backward rows in pieces of 112 where there are more rows than compute units
        assert int(_lib.lib().stereo_hip_device_cus()) == resident
        chunks = (0, chunk)
    else:
        monkeypatch.setenv("STEREO_HIP_TRWS_ROW_CHUNK", str(chunk))
        monkeypatch.setenv("STEREO_HIP_TRWS_BLOCKS", str(resident))
        chunks = (chunk, chunk)
    for kernel, shared in ((1, False), (2, True)) if tall else [(k, s) for k in (1, 2) for s in (True, False)]:
        p = fp.instance(H, W, K, shared, kernel, False)
        want = []
        for d in (0, 1):
            rows = len(schedule(H * W, p["conn"].T, d)["ticket_run"])
            if chunks[d]:
                pieces = schedule_chunked(H * W, p["conn"].T, d, chunks[d], resident)
                assert pieces["chunked"] and len(pieces["ticket_run"]) > max(rows, resident)
                want.append(len(pieces["ticket_run"]))
            else:
                want.append(rows)
        plan = _plan(p, kernel)
        assert plan.path() == 2 and _plan_runs(plan) == tuple(want), (_plan_runs(plan), want)
        runs = []
        for _ in range(4 if tall else 8):
            assert plan.iterate(1, NEVER) == (1, False)
            runs.append(_shown(plan))
        plan.close()
        print("%dx%d K %d kernel %d shared %d runs %r: bounds %r, energies %r" % (H, W, K, kernel, shared, want, [r[2] for r in runs], [r[1] for r in runs]))
        fp.check_run(p, kernel, p["lam"], runs, None, fp.SLACK)


def test_every_kernel_family_was_reached(hip):
    assert _paths >= {1, 2, 3, 4, 5}, sorted(_paths)
