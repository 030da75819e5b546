"""-m gpu: the roles of the K <= 64 sweep kernels as functions of their own (trws_pipe.hip: pipe_compute, pipe_loader_b,
pipe_loader_a, pipe_storer, pipe_primal), in whole solves against the CPU oracle.

Every role's visit loop is a real function that the kernel body calls once per run.  What that can break and the other
suites do not aim at: what a wave keeps from one run to the next (the compute waves' look_streak goes in and out of the
call), the run's values arriving as arguments (p0, p1, run, segment, first-visit and second-walk flags), the parameter
block read from its copy in global memory (a plan's own block; a strip's or a batch member's entry of the launch table)
and a role that leaves through the abort word.  Every case asserts labels, energy and lower bound of
oracle.pyoracle.trws bit for bit after each of 1 .. ITERS iterations.

Runs per workgroup: plans created with a limit of 2 and of 4 workgroups (and STEREO_HIP_TRWS_BLOCKS, which the library
reads once per process) walk all runs on those workgroups, so every role function is entered many times by the same
waves; asserted through the plan's run counts.  Run lengths: STEREO_HIP_TRWS_ROW_CHUNK=3,3 on those plans cuts the
interior rows (W - 2 positions) into pieces of three positions, with a one-position last piece on 12 x 9 and a
two-position one on 30 x 40: the frame p0 - 1 .. p1 at its shortest.

Volumes: noise, sloped (twin pairs: split messages, coop_collect), ties (failed certificates, the serial construction)
and near-ties (second looks that fail and pass in turn: look_streak moves across runs) of
test_message_minimum_paths_gpu.py.  serial_messages() must be 0 on noise, and > 0 on ties at K = 60 and 64, the label
counts that volume was made for: with 3 or 8 labels its block of all-zero rows fails no certificate at all -- measured on
12 x 9, three iterations, 0 serial messages at K = 3 and at K = 8 for every tolerance of 1, 1.5, 2, 2.5, 4 and 8 (K = 60:
6 at tolerance 4, 20 at 8) -- so there that 0 is what is asserted.  The
30 x 40 grid gets the speculative schedule by default: spec_stats() active with commits there, inactive under
STEREO_HIP_TRWS_SPEC=0.

Switches, each on and off: granules off / on / late (development switch 262144), second walks (16384, 30 x 40), no twins
(8192), smoothness kernel 2, per-edge positions, a batch of two, two strips.  Two strips sum energy and bound as two
partial sums each, in another order than the oracle's single sum: labels exact, the two sums within 1e-12 relative (the
bound test_di_prefix_gpu.py's strips use: a few dozen ulps of a sum of ~10^3 terms of one sign pattern), and equal
between the ways."""
import ctypes as C

import numpy as np
import pytest

from helpers import grid_conn
from test_message_minimum_paths_gpu import volume

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK", "STEREO_HIP_TRWS_BLOCKS",
       "STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_MESSAGES", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_CERTIFICATE",
       "STEREO_HIP_TRWS_SPEC_SEG")
ITERS = 3
NEVER = -1e300
TOL = {1: 8.0, 2: 30.0}
VOLUMES = ("noise", "sloped", "ties", "near-ties")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("STEREO_HIP_TRWS_SPIN_SECONDS", "3")


_problems, _wanted = {}, {}


def _problem(name, H, W, K, where="shared"):
    """built once per key, never changed; where = "edges": per-edge positions q != qprim around the shared ones"""
    key = (name, H, W, K, where)
    if key not in _problems:
        conn = grid_conn(H, W)
        unary, alphas = volume(name, H, W, K)
        pos = np.arange(K, dtype=np.float64)
        q = np.tile(pos, (conn.shape[0], 1))
        qprim = q
        if where == "edges":
            rng = np.random.default_rng(7000 + 1000 * H + 10 * W + K)
            q = q + 0.25 * rng.uniform(size=q.shape)
            qprim = np.tile(pos, (conn.shape[0], 1)) + 0.25 * rng.uniform(size=q.shape)
        _problems[key] = dict(key=key, unary=unary, conn=conn, q=q, qprim=qprim, alphas=alphas, pos=pos if where == "shared" else None)
    return _problems[key]


def _oracle(oracle, kernel, p):
    """the oracle's (labels, energy, bound, iterations) after 1 .. ITERS iterations"""
    key = (kernel,) + p["key"]
    if key not in _wanted:
        _wanted[key] = [oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], TOL[kernel], n, NEVER, mode=1)
                        for n in range(1, ITERS + 1)]
    return _wanted[key]


def _plan(kernel, p, max_workgroups=0):
    """a whole-problem TrwsPlan with its inputs; max_workgroups > 0: created with a limit on its workgroups
    (stereo_trws_plan_create_strip, one strip)"""
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
    _upload(plan, kernel, p)
    return plan


def _upload(plan, kernel, p):
    if p["pos"] is not None:
        plan.upload(p["unary"].T, p["alphas"], TOL[kernel], positions=p["pos"])
    else:
        plan.upload(p["unary"].T, p["alphas"], TOL[kernel], q=p["q"].T, qprim=p["qprim"].T)


def _runs(plan):
    from stereo_amd import _lib
    nf, nb = C.c_int64(), C.c_int64()
    _lib.lib().stereo_trws_plan_strip_info(plan._h, None, None, None, C.byref(nf), C.byref(nb), None, None)
    return nf.value, nb.value


def _walk(monkeypatch, env, kernel, p, max_workgroups=0):
    """one plan, one iteration at a time: its results after each; serial_messages(), spec_stats() and the run counts"""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        plan = _plan(kernel, p, max_workgroups)
        assert plan.path() == 2, "path %d, expected the K <= 64 kernel" % plan.path()
        plan.serial_messages(reset=True)
        got = []
        for _ in range(ITERS):
            plan.iterate(1, max_relgap=NEVER)
            got.append(plan.result())
        serial, stats, runs = plan.serial_messages(), plan.spec_stats(), _runs(plan) if max_workgroups else None
        plan.close()
    return got, serial, stats, runs


def _is(got, want, what):
    lab, en, lb, it = got
    assert it == want[3], what
    assert np.array_equal(lab, want[0]), "%s: labels differ at %d of %d nodes" % (what, int((lab != want[0]).sum()), lab.size)
    assert en == want[1] and lb == want[2], (what, (en, lb), want[1:3])


def _check(monkeypatch, oracle, kernel, p, ways):
    """every way (name, environment, workgroup limit) against the oracle, iteration by iteration; returns what each saw"""
    want = _oracle(oracle, kernel, p)
    seen = {}
    for what, env, wg in ways:
        got, serial, st, runs = _walk(monkeypatch, env, kernel, p, wg)
        print(what, "serial messages", serial, "spec", st, "runs", runs)
        for n in range(ITERS):
            _is(got[n], want[n], "%s, iteration %d" % (what, n + 1))
        seen[what] = (serial, st, runs)
    return seen


def _limited(wg, pieces=False):
    # (the limit that does the work is the one the plan is created with, _plan(max_workgroups): the library reads
    #  STEREO_HIP_TRWS_BLOCKS at its first launch in the process and never again -- the entry names the intent, as the
    #  other suites' cases of this kind do, and changes nothing by then)
    env = {"STEREO_HIP_TRWS_BLOCKS": str(wg)}
    if pieces:
        env["STEREO_HIP_TRWS_ROW_CHUNK"] = "3,3"
    return ("%d workgroups%s" % (wg, ", pieces of three" if pieces else ""), env, wg)


CASES = [(12, 9, K, name) for K in (3, 8, 60, 64) for name in VOLUMES] + [(30, 40, K, name) for K in (60, 64) for name in VOLUMES]


@pytest.mark.parametrize("H,W,K,name", CASES, ids=["%dx%d-K%d-%s" % c for c in CASES])
def test_roles_across_runs(H, W, K, name, hip, oracle, monkeypatch):
    p = _problem(name, H, W, K)
    ways = [("default schedule", {}, 0), ("plain schedule", {"STEREO_HIP_TRWS_SPEC": "0"}, 0),
            _limited(2), _limited(4), _limited(2, True), _limited(4, True)]
    if (H, W) == (30, 40):
        ways.append(("second walks", {"STEREO_HIP_TRWS_DEBUG": "16384"}, 0))
    seen = _check(monkeypatch, oracle, 1, p, ways)
    for what, (serial, st, runs) in seen.items():
        if name == "noise":
            assert serial == 0, (what, serial)
        if name == "ties" and K >= 60:
            assert serial > 0, what
        if name == "ties" and K < 60:   # (the module's text: the measured 0, pinned)
            assert serial == 0, (what, serial)
        if runs is not None:
            wg = int(what.split()[0])
            assert min(runs) > wg, (what, runs)   # more runs than workgroups: the same waves enter their role again
            if "pieces" in what:                  # every interior row in pieces of at most three positions
                assert min(runs) >= (H - 2) * ((W - 2 + 2) // 3), (what, runs)
    st = seen["default schedule"][1]
    assert not seen["plain schedule"][1]["active"] and seen["plain schedule"][1]["commits"] == 0, seen["plain schedule"][1]
    if (H, W) == (30, 40):
        assert st["active"] and st["commits"] > 0, st
        assert seen["second walks"][1]["second_walks"] > 0, seen["second walks"][1]
    else:
        assert not st["active"] or st["commits"] > 0, st


GRANULES = {"off": {"STEREO_HIP_TRWS_GRANULES": "0"}, "on": {}, "late": {"STEREO_HIP_TRWS_DEBUG": "262144"}}


@pytest.mark.parametrize("granules", sorted(GRANULES))
@pytest.mark.parametrize("H,W,K", ((12, 9, 60), (30, 40, 64)))
@pytest.mark.parametrize("name", ("sloped", "near-ties"))
def test_granules_off_on_late(name, H, W, K, granules, hip, oracle, monkeypatch):
    """rows handed between runs as granules, behind flags, and as granules that arrive late: loader B's poll loop"""
    p = _problem(name, H, W, K)
    env = GRANULES[granules]
    ways = [("default schedule", env, 0), ("plain schedule", dict(env, STEREO_HIP_TRWS_SPEC="0"), 0)]
    for wg in (2, 4):
        what, e, _ = _limited(wg, True)
        ways.append((what, dict(env, **e), wg))
    _check(monkeypatch, oracle, 1, p, ways)


@pytest.mark.parametrize("twins", ("twins", "no twins"))
@pytest.mark.parametrize("H,W,K", ((12, 9, 60), (30, 40, 64)))
def test_twins_on_and_off(H, W, K, twins, hip, oracle, monkeypatch):
    """the sloped volume makes every pair of pixels a twin pair; development switch 8192 lets every wave finish alone"""
    p = _problem("sloped", H, W, K)
    env = {} if twins == "twins" else {"STEREO_HIP_TRWS_DEBUG": "8192"}
    what, e, _ = _limited(2)
    _check(monkeypatch, oracle, 1, p, [("default schedule", env, 0), ("plain schedule", dict(env, STEREO_HIP_TRWS_SPEC="0"), 0),
                                       (what, dict(env, **e), 2)])


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("kernel", (1, 2))
@pytest.mark.parametrize("H,W,K,name", ((12, 9, 60, "noise"), (12, 9, 8, "ties"), (30, 40, 64, "near-ties")))
def test_smoothness_kernels_and_positions(H, W, K, name, kernel, where, hip, oracle, monkeypatch):
    """the other instantiations of the role functions: the quadratic kernel, per-edge positions (q, qprim and their
    permutations read through the role's parameter block)"""
    p = _problem(name, H, W, K, where)
    seen = _check(monkeypatch, oracle, kernel, p, [("default schedule", {}, 0), _limited(2), _limited(4, True)])
    if where == "edges" or kernel == 2:   # the speculative schedule is the linear kernel's, on shared positions
        assert not seen["default schedule"][1]["active"], seen["default schedule"][1]


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("kernel", (1, 2))
def test_a_batch_of_two(kernel, where, hip, oracle, monkeypatch):
    """the batch kernels: a role reads the member's block in the launch's table; workgroups move between members"""
    from stereo_amd.trws import TrwsBatch
    problems = [_problem("sloped", 12, 9, 60, where), _problem("ties", 12, 9, 8, where)]
    for env in ({}, {"STEREO_HIP_TRWS_GRANULES": "0"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            plans = [_plan(kernel, p) for p in problems]
            assert all(pl.path() == 2 for pl in plans)
            with TrwsBatch(plans) as batch:
                for n in range(ITERS):
                    assert batch.iterate(1, NEVER) == [1] * 2
                    for pl, p in zip(plans, problems):
                        _is(pl.result(), _oracle(oracle, kernel, p)[n], "batch member, iteration %d" % (n + 1))
            for pl in plans:
                pl.close()


@pytest.mark.parametrize("where", ("shared", "edges"))
@pytest.mark.parametrize("name", ("sloped", "ties"))
def test_two_strips(name, where, hip, oracle, monkeypatch):
    """the group kernels: a role reads the strip's block in the launch's table (sums: see the module's text)"""
    from stereo_amd.strips import make_strips
    H, W, K = 12, 9, 60
    p = _problem(name, H, W, K, where)
    want = _oracle(oracle, 1, p)[ITERS - 1]
    sums = []
    for env in ({}, {"STEREO_HIP_TRWS_GRANULES": "0"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            s = make_strips(1, K, H, W, p["conn"].T, 2)
            _upload(s, 1, p)
            done, _ = s.iterate(ITERS, max_relgap=NEVER)
            lab, en, lb, it = s.result()
            assert done == ITERS and s.path() == 2
            s.close()
        assert it == want[3] and np.array_equal(lab, want[0])
        for x, y in ((en, want[1]), (lb, want[2])):
            assert abs(x - y) <= 1e-12 * max(abs(x), abs(y), 1.0), (x, y)
        sums.append((en, lb))
    assert sums[0] == sums[1]
