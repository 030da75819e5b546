"""-m gpu: the TRW-S solver state: save, load, resume, re-shard, warm start.

Every kernel family, row strips and batches promise identical results, so a state that moves between them has an exact
yardstick: the uninterrupted run.  Every comparison below is np.array_equal / == on labels, energy, bound, iteration
count and the saved messages; nothing needs a tolerance.  Where no uninterrupted run exists -- other unaries from some
iteration on, foreign messages -- the yardstick is a restatement of minimize.cpp in this file (in the manner of
mm_restate.py) that takes initial messages, a phase and inputs that change at a given iteration.

Grids are 10 x 40 as in test_iterate_ahead_gpu.py (30 x 40 with unit weights where the speculative schedule must run), the restated cases 5 x 6 with
K = 5, the strips' cases the smallest shapes of test_strips_gpu.py, the K > 512 case the smallest of
test_trws_large_gpu.py."""
import os

import numpy as np
import pytest

from helpers import grid_conn, trws_problem
import mm_restate

pytestmark = pytest.mark.gpu

H, W = 10, 40
NEVER = -1e300
ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK",
       "STEREO_HIP_TRWS_FAST", "STEREO_HIP_TRWS_ITERATE_AHEAD")


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# name: H, W, K, positions, message mode, environment at creation, tol, path, the speculative schedule runs
def _cases():
    from stereo_amd.trws import MESSAGES_MINPLUS, ORDER_INDEX
    return {
        "path2-edges": (H, W, 16, "edges", 0, {}, 4.0, 2, False),
        "path2-shared": (H, W, 16, "shared", 0, {}, 4.0, 2, None),
        # (30, 40, 16) with unit weights, as test_trws_batch_gpu.py has it: alone it runs the speculative border-chain schedule
        "path2-shared-spec": (30, 40, 16, "shared", 0, {}, 4.0, 2, True),
        "path4": (H, W, 70, "edges", 0, {}, 4.0, 4, False),
        "path3-exact": (H, W, 72, "shared", 0, {}, 4.0, 3, None),
        "path3-minplus": (H, W, 72, "shared", MESSAGES_MINPLUS, {}, 4.0, 3, None),
        "path1": (H, W, 16, "edges", 0, {"STEREO_HIP_TRWS_FAST": "0"}, 4.0, 1, False),
        "path1-shared72": (H, W, 72, "shared", 0, {"STEREO_HIP_TRWS_FAST": "0"}, 4.0, 1, False),
        "path5": (7, 9, 513, "shared", 0, {}, 8.0, 5, False),
        "index-order": (H, W, 16, "edges", ORDER_INDEX, {}, 4.0, 2, False),
    }


CASE_NAMES = ["path2-edges", "path2-shared", "path2-shared-spec", "path4", "path3-exact", "path3-minplus", "path1", "path5", "index-order"]


def _inputs(name, seed=11, scale=1.0):
    h, w, K = _cases()[name][:3]
    rng = np.random.default_rng(seed)
    conn = grid_conn(h, w)
    unary = rng.uniform(0, 40, size=(h * w, K)) * scale
    alphas = rng.uniform(0.5, 2.0, size=conn.shape[0])
    return unary, conn, np.ones(conn.shape[0]) if name.endswith("-spec") else alphas


def _make(name, seed=11, scale=1.0, upload=True, keep_mm=False):
    """a fresh plan of the case, with its inputs; the case's environment holds while the plan is created"""
    from stereo_amd.trws import TrwsPlan
    h, w, K, where, mode, env, tol, path, _ = _cases()[name]
    unary, conn, alphas = _inputs(name, seed, scale)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        plan = TrwsPlan(1, K, h * w, conn.T, message_mode=mode)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if keep_mm:
        plan.keep_min_marginals(True)
    if upload:
        if where == "shared":
            plan.upload(unary.T, alphas, tol, positions=np.arange(K, dtype=np.float64))
        else:
            q = np.tile(np.random.default_rng(5).permutation(K).astype(np.float64), (conn.shape[0], 1))
            plan.upload(unary.T, alphas, tol, q=q.T, qprim=q.T)
        assert plan.path() == path
    return plan


def _obs(plan):
    lab, en, lb, it = plan.result()
    return dict(labels=lab.copy(), energy=en, bound=lb, iterations=it)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _same_state(a, b, header=True):
    from stereo_amd.trws import TrwsState
    if header:
        for f in TrwsState.FIELDS:
            assert getattr(a, f) == getattr(b, f), (f, getattr(a, f), getattr(b, f))
    assert np.array_equal(a.labels, b.labels), "labels differ at %d nodes" % int((a.labels != b.labels).sum())
    assert np.array_equal(a.messages, b.messages), "messages differ in %d rows" % int((a.messages != b.messages).any(axis=1).sum())


_straight_cache = {}


def _straight(name, iters, seed=11, scale=1.0):
    """the uninterrupted run: what the plan shows and saves after iterate(iters); computed once per case"""
    key = (name, iters, seed, scale)
    if key not in _straight_cache:
        plan = _make(name, seed, scale)
        plan.iterate(iters, NEVER)
        _straight_cache[key] = (_obs(plan), plan.save_state())
        plan.close()
    return _straight_cache[key]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_resume_equals_straight_and_save_does_not_disturb(name, hip, tmp_path):
    from stereo_amd.trws import TrwsState
    spec = _cases()[name][8]
    whole, whole_state = _straight(name, 6)
    a = _make(name)
    if spec is not None:
        assert a.spec_stats()["active"] == spec
    a.iterate(3, NEVER)
    before = (_obs(a), a.serial_messages(), a.spec_stats())
    st = a.save_state()
    assert (st.phase, st.iterations, st.K, st.N) == (1, 3, a.K, a.N)
    assert st.messages.shape == (a.E, a.K) and st.messages.flags["C_CONTIGUOUS"] and st.labels.dtype == np.int32
    assert np.array_equal(st.labels + 1.0, before[0]["labels"]) and (st.energy, st.lower_bound) == (before[0]["energy"], before[0]["bound"])
    assert _same(before[0], _obs(a)) and before[1:] == (a.serial_messages(), a.spec_stats())
    # the saved plan goes on
    a.iterate(3, NEVER)
    assert _same(_obs(a), whole)
    _same_state(a.save_state(), whole_state)
    a.close()
    # a fresh plan takes the state, here through a file
    st.to_file(str(tmp_path / "s.npz"))
    b = _make(name)
    b.load_state(TrwsState.from_file(str(tmp_path / "s.npz")))
    assert _same(_obs(b), before[0])
    _same_state(b.save_state(), st)
    b.iterate(3, NEVER)
    assert _same(_obs(b), whole)
    _same_state(b.save_state(), whole_state)
    # ... and a plan that has iterated elsewhere (load implies reset)
    b.iterate(1, NEVER)
    b.load_state(st)
    b.iterate(3, NEVER)
    assert _same(_obs(b), whole)
    b.close()


def test_fresh_plan_saves_phase_zero(hip):
    a = _make("path2-edges")
    st = a.save_state()
    assert (st.phase, st.iterations, st.energy, st.lower_bound) == (0, 0, 0.0, 0.0)
    assert not st.messages.any() and not st.labels.any()
    a.iterate(2, NEVER)
    a.load_state(st)
    a.iterate(6, NEVER)
    assert _same(_obs(a), _straight("path2-edges", 6)[0])
    a.close()


def _stop_gap(name):
    """half way between the gaps (E - LB) / E after iterations 1 and 2 of an iterate(1) loop: iterate(6, gap) stops after 2"""
    plan = _make(name)
    gaps = []
    for _ in range(2):
        plan.iterate(1, NEVER)
        o = _obs(plan)
        gaps.append((o["energy"] - o["bound"]) / o["energy"])
    plan.close()
    assert 0 < gaps[1] < gaps[0], gaps
    return 0.5 * (gaps[0] + gaps[1])


@pytest.mark.parametrize("name", ["path2-shared", "path2-shared-spec", "path2-edges"])
def test_phase_two(name, hip, monkeypatch):
    gap = _stop_gap(name)
    whole = _straight(name, 5)[0]
    a = _make(name)
    assert a.iterate(6, gap) == (2, True)
    at_save = _obs(a)
    st = a.save_state()
    assert (st.phase, st.iterations) == (2, 2)
    assert _same(_obs(a), at_save)
    b = _make(name)
    b.load_state(st)
    assert _same(_obs(b), at_save)
    _same_state(b.save_state(), st)
    seen = {}
    for who, plan in (("original", a), ("loaded", b)):
        assert plan.iterate(2, NEVER) == (2, False)
        mid = _obs(plan)
        assert plan.iterate(1, NEVER) == (1, False)
        seen[who] = (mid, _obs(plan), plan.save_state())
        plan.close()
    monkeypatch.setenv("STEREO_HIP_TRWS_ITERATE_AHEAD", "0")
    c = _make(name)
    assert c.iterate(6, gap) == (2, True)
    assert c.save_state().phase == 1
    c.iterate(2, NEVER)
    mid = _obs(c)
    c.iterate(1, NEVER)
    seen["behind"] = (mid, _obs(c), c.save_state())
    c.close()
    for who in ("loaded", "behind"):
        assert _same(seen[who][0], seen["original"][0]) and _same(seen[who][1], seen["original"][1]), who
        _same_state(seen[who][2], seen["original"][2])
    assert _same(seen["original"][1], whole)


@pytest.mark.parametrize("src,dst", [("path2-edges", "path1"), ("path1", "path2-edges"), ("path3-exact", "path1-shared72")])
def test_across_kernel_families(src, dst, hip):
    a = _make(src)
    a.iterate(3, NEVER)
    st = a.save_state()
    a.close()
    b = _make(dst)
    assert b.path() != _cases()[src][7]
    b.load_state(st)
    b.iterate(3, NEVER)
    whole, whole_state = _straight(src, 6)
    assert _same(_obs(b), whole)
    _same_state(b.save_state(), whole_state)
    b.close()


# seed, H, W, K, kind, tol, path: the smallest shapes of test_strips_gpu.py on the K <= 64 and on the wide kernel
RESHARD = {"path2": (105, 9, 40, 8, "general", 2.0, 2), "path3": (107, 12, 14, 256, "fronto", 8.0, 3)}


def _reshard_solver(case, G):
    """one plan (G == 1) or G logical strips of the case's problem, with inputs"""
    from stereo_amd.strips import make_strips
    from stereo_amd.trws import TrwsPlan
    seed, h, w, K, kind, tol, path = RESHARD[case]
    p = trws_problem(seed, h, w, K, kind=kind)
    s = TrwsPlan(1, K, h * w, p["conn"].T) if G == 1 else make_strips(1, K, h, w, p["conn"].T, G)
    if kind == "fronto":
        s.upload(p["unary"].T, p["alphas"], tol, positions=np.arange(K, dtype=np.float64))
    else:
        s.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)
    assert s.path() == path
    return s


@pytest.mark.parametrize("case", sorted(RESHARD))
def test_reshard(case, hip):
    one = _reshard_solver(case, 1)
    straight = []
    for _ in range(4):   # the single plan's states at iterations 3, 6, 9, 12
        one.iterate(3, NEVER)
        straight.append((_obs(one), one.save_state()))
    one.close()
    st = straight[0][1]
    for leg, G in enumerate((2, 3, 1), start=1):
        s = _reshard_solver(case, G)
        s.load_state(st)
        lab, en, lb, it = s.result()
        assert np.array_equal(lab, st.labels + 1.0) and (en, lb, it) == (st.energy, st.lower_bound, st.iterations)
        assert s.iterate(3, NEVER) == (3, False)
        lab, en, lb, it = s.result()
        want = straight[leg][0]
        assert np.array_equal(lab, want["labels"]) and it == want["iterations"]
        if G == 1:
            assert (en, lb) == (want["energy"], want["bound"])
        st = s.save_state()
        print("reshard %s G %d: energy %r (single %r) bound %r (single %r)" % (case, G, st.energy, want["energy"], st.lower_bound, want["bound"]))
        # the state from the strips is the single plan's at the same iteration: header, messages, labels
        _same_state(st, straight[leg][1])
        s.close()


def test_strips_state_on_the_device_and_refusals(hip):
    import torch
    from stereo_amd import StereoHipError
    s = _reshard_solver("path2", 2)
    s.iterate(2, NEVER)
    host = s.save_state()
    d_m = torch.zeros((s.E, s.K), dtype=torch.float64, device="cuda")
    d_x = torch.zeros(s.N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    dev = s.save_state_device(d_m.data_ptr(), d_x.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_m.cpu().numpy(), host.messages) and np.array_equal(d_x.cpu().numpy(), host.labels)
    assert bytes(dev.header()) == bytes(host.header())
    # the scatter: into three strips from the device arrays, then on; equals the host load
    t = _reshard_solver("path2", 3)
    t.load_state_device(dev, d_m.data_ptr(), d_x.data_ptr(), side.cuda_stream)
    t.iterate(2, NEVER)
    u = _reshard_solver("path2", 3)
    u.load_state(host)
    u.iterate(2, NEVER)
    _same_state(t.save_state(), u.save_state())
    u.close()
    t.close()
    # strips that are not in one state
    s.plans[0].reset()
    with pytest.raises(StereoHipError, match="not in one state"):
        s.save_state()
    s.close()
    # a phase-2 state enters a single plan only
    gap = _stop_gap("path2-edges")
    a = _make("path2-edges")
    assert a.iterate(6, gap) == (2, True)
    st = a.save_state()
    a.close()
    assert st.phase == 2
    from stereo_amd.strips import make_strips
    unary, conn, alphas = _inputs("path2-edges")
    g = make_strips(1, 16, H, W, conn.T, 2)
    q = np.tile(np.random.default_rng(5).permutation(16).astype(np.float64), (conn.shape[0], 1))
    g.upload(unary.T, alphas, 4.0, q=q.T, qprim=q.T)
    with pytest.raises(StereoHipError, match="phase"):
        g.load_state(st)
    g.close()


def test_batch_member_loaded_in_mid_run(hip):
    from stereo_amd.trws import TrwsBatch
    name = "path2-edges"
    a = _make(name)
    a.iterate(3, NEVER)
    st = a.save_state()
    a.close()
    plans = [_make(name), _make(name, seed=12), _make(name, seed=13, scale=0.5)]
    plans[0].load_state(st)
    with TrwsBatch(plans) as batch:
        assert batch.iterate(2, NEVER) == [2, 2, 2]
    got = [(_obs(p), p.save_state()) for p in plans]
    for p in plans:
        p.close()
    want = [_straight(name, 5), _straight(name, 2, seed=12), _straight(name, 2, seed=13, scale=0.5)]
    for (o, s), (wo, ws) in zip(got, want):
        assert _same(o, wo)
        _same_state(s, ws)


# ---- the restatement: minimize.cpp from given messages, with inputs that change ------------------------------------

def _restate(oracle, p, M0, phase, iters, tol, change_at=None, unary_b=None, tol_b=None):
    """`iters` iterations of Minimize_TRW_S (minimize.cpp:31-113) from the messages M0 (E, K), which stand as after a
    backward sweep (phase 0) or with the first iteration's forward sweep already run (phase 1).  change_at = t: the
    inputs change the way a plan's do when it is uploaded to after iteration t -- iterations 1 .. t and the FORWARD
    sweep of iteration t + 1 (the plan runs it fused with iteration t's primal pass) see (p["unary"], tol), everything
    after that (unary_b, tol_b).  Returns labels (0-based), energy, bound, messages."""
    impl = mm_restate.default_impl(oracle)
    col_impl = "ref" if impl == "ref" else "brute"
    q = np.ascontiguousarray(p["q"], dtype=np.float64)
    qp = np.ascontiguousarray(p["qprim"], dtype=np.float64)
    alphas = np.asarray(p["alphas"], dtype=np.float64)
    N, K = p["unary"].shape
    g = mm_restate._structure(oracle, N, p["conn"], 0)
    order, fwd, bwd, tail, dirn = g["order"], g["fwd"], g["bwd"], g["tail"], g["dir"]
    gamma = [1.0 / max(len(fwd[i]), len(bwd[i])) if (fwd[i] or bwd[i]) else np.inf for i in range(N)]
    M = np.array(M0, dtype=np.float64)
    x = np.zeros(N, np.int64)

    def inputs(after_change):
        return (np.ascontiguousarray(unary_b, dtype=np.float64), tol_b) if after_change else (np.ascontiguousarray(p["unary"], dtype=np.float64), tol)

    def upd(e, Di, i, d, lam):
        m, v = oracle.update_message(1, Di, gamma[i], M[e], q[e], qp[e], alphas[e], lam, d, dirn[e], impl=impl)
        M[e] = m
        return v

    LB = En = 0.0
    for t in range(1, iters + 1):
        if not (t == 1 and phase == 1):
            unary, lam = inputs(change_at is not None and t > change_at + 1)
            for i in order:
                Di = unary[i].copy()
                for e in fwd[i]:
                    Di += M[e]
                for e in bwd[i]:
                    Di += M[e]
                for e in fwd[i]:
                    upd(e, Di, i, 0, lam)
        unary, lam = inputs(change_at is not None and t > change_at)
        LB = 0.0
        for i in reversed(order):
            Di = unary[i].copy()
            for e in bwd[i]:
                Di += M[e]
            for e in fwd[i]:
                Di += M[e]
            vmin = Di[0]
            for k in range(1, K):
                if vmin > Di[k]:
                    vmin = Di[k]
            Di = Di - vmin
            LB += vmin
            for e in bwd[i]:
                LB += upd(e, Di, i, 1, lam)
        En = 0.0
        for i in order:
            Db = unary[i].copy()
            for e in bwd[i]:
                Db = oracle.add_column(1, q[e], qp[e], alphas[e], lam, x[tail[e]], Db, 0, dirn[e], impl=col_impl)
            Di = Db.copy()
            for e in fwd[i]:
                Di += M[e]
            k = int(np.argmin(Di))
            x[i] = k
            En += Db[k]
    return x, En, LB, M


RH, RW, RK = 5, 6, 5


def _restated_plan(p, tol):
    from stereo_amd.trws import TrwsPlan
    plan = TrwsPlan(1, RK, RH * RW, p["conn"].T)
    plan.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)
    return plan


def test_restatement_is_the_oracle(hip, oracle):
    """the yardstick itself: from zero messages and fixed inputs it is oracle.trws and the plan"""
    p = trws_problem(21, RH, RW, RK, kind="general")
    x, en, lb, M = _restate(oracle, p, np.zeros((p["conn"].shape[0], RK)), 0, 3, 3.0)
    ref = mm_restate.oracle_trws(oracle, mm_restate.default_impl(oracle), 1, p, 3.0, 3)
    assert np.array_equal(ref[0], x + 1.0) and (ref[1], ref[2]) == (en, lb)
    plan = _restated_plan(p, 3.0)
    plan.iterate(3, NEVER)
    assert _same(_obs(plan), dict(labels=x + 1.0, energy=en, bound=lb, iterations=3.0))
    plan.close()


def test_warm_start_with_other_unaries_on_the_device(hip, oracle):
    """iterate(2) on unary A, save on the device, upload unary B with another tol, load, iterate(2)"""
    import torch
    p = trws_problem(21, RH, RW, RK, kind="general")
    unary_b = np.random.default_rng(22).uniform(0, 40, size=p["unary"].shape)
    E = p["conn"].shape[0]
    plan = _restated_plan(p, 3.0)
    plan.iterate(2, NEVER)
    d_m = torch.zeros((E, RK), dtype=torch.float64, device="cuda")
    d_x = torch.zeros(RH * RW, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    st = plan.save_state_device(d_m.data_ptr(), d_x.data_ptr(), side.cuda_stream)
    assert (st.phase, st.iterations) == (1, 2)
    side.synchronize()
    plan.upload(unary_b.T, p["alphas"], 5.0, q=p["q"].T, qprim=p["qprim"].T)
    assert plan.result()[3] == 0
    plan.load_state_device(st, d_m.data_ptr(), d_x.data_ptr(), side.cuda_stream)
    assert plan.result()[3] == 2
    plan.iterate(2, NEVER)
    x, en, lb, M = _restate(oracle, p, np.zeros((E, RK)), 0, 4, 3.0, change_at=2, unary_b=unary_b, tol_b=5.0)
    assert _same(_obs(plan), dict(labels=x + 1.0, energy=en, bound=lb, iterations=4.0))
    # the messages at rest have the forward sweep of iteration 5 in them: one more restated iteration from phase 1
    after = plan.save_state()
    pb = dict(p, unary=unary_b)
    x5, en5, lb5, _ = _restate(oracle, pb, after.messages, 1, 1, 5.0)
    plan.iterate(1, NEVER)
    assert _same(_obs(plan), dict(labels=x5 + 1.0, energy=en5, bound=lb5, iterations=5.0))
    plan.close()


def test_foreign_messages_enter_through_phase_zero(hip, oracle):
    p = trws_problem(23, RH, RW, RK, kind="general")
    E = p["conn"].shape[0]
    plan = _restated_plan(p, 3.0)
    st = plan.save_state()
    assert st.phase == 0
    st.messages = np.random.default_rng(24).normal(scale=5.0, size=(E, RK))
    plan.load_state(st)
    plan.iterate(2, NEVER)
    x, en, lb, _ = _restate(oracle, p, st.messages, 0, 2, 3.0)
    assert _same(_obs(plan), dict(labels=x + 1.0, energy=en, bound=lb, iterations=2.0))
    plan.close()


def test_device_save_equals_host_save(hip):
    import torch
    plan = _make("path2-shared-spec")
    plan.iterate(3, NEVER)
    host = plan.save_state()
    d_m = torch.zeros((plan.E, plan.K), dtype=torch.float64, device="cuda")
    d_x = torch.zeros(plan.N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    dev = plan.save_state_device(d_m.data_ptr(), d_x.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert bytes(dev.header()) == bytes(host.header())
    assert np.array_equal(d_m.cpu().numpy(), host.messages) and np.array_equal(d_x.cpu().numpy(), host.labels)
    plan.close()


def test_min_marginals_after_a_load(hip):
    from stereo_amd import StereoHipError
    name = "path2-edges"
    a = _make(name, keep_mm=True)
    a.iterate(3, NEVER)
    a.min_marginals()
    st = a.save_state()
    b = _make(name, keep_mm=True)
    b.load_state(st)
    with pytest.raises(StereoHipError, match="no min-marginals to read"):
        b.min_marginals()
    a.iterate(1, NEVER)
    b.iterate(1, NEVER)
    for got, want in zip(b.min_marginals(), a.min_marginals()):
        assert np.array_equal(got, want)
    assert _same(_obs(a), _obs(b))
    a.close()
    b.close()


def test_refusals_name_the_field(hip):
    from stereo_amd import StereoHipError
    from stereo_amd.trws import ORDER_INDEX
    name = "path2-edges"
    a = _make(name)
    a.iterate(1, NEVER)
    st = a.save_state()
    want = _obs(a)

    def changed(**kw):
        from stereo_amd.trws import TrwsState
        c = TrwsState(st.header(), st.messages, st.labels)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for field, value in (("magic", 1), ("version", 7), ("kernel", 2), ("K", 17), ("N", st.N + 1), ("E", st.E - 1),
                         ("connectivity_key", st.connectivity_key + 1), ("message_mode", ORDER_INDEX), ("phase", 3)):
        with pytest.raises(StereoHipError, match=r"\b%s\b" % field):
            a.load_state(changed(**{field: value}))
        assert _same(_obs(a), want), field   # a refused load leaves the plan as it was
    with pytest.raises(StereoHipError, match="must be"):
        a.load_state(changed(messages=st.messages[:-1]))
    # another connectivity of the same size; another node order
    unary, conn, alphas = _inputs(name)
    from stereo_amd.trws import TrwsPlan
    other = TrwsPlan(1, 16, H * W, conn[::-1].T)
    q = np.tile(np.arange(16.0), (conn.shape[0], 1))
    other.upload(unary.T, alphas, 4.0, q=q.T, qprim=q.T)
    with pytest.raises(StereoHipError, match="connectivity_key"):
        other.load_state(st)
    other.close()
    b = _make("index-order")
    with pytest.raises(StereoHipError, match="message_mode"):
        b.load_state(st)
    b.close()
    # a plan without inputs
    c = _make(name, upload=False)
    with pytest.raises(StereoHipError, match="upload or bind first, then load"):
        c.load_state(st)
    c.close()
    a.close()


def test_positions_are_analysed_afresh_at_every_upload(hip):
    """ascending shared positions, iterations, then a shared vector that is not ascending: path and results are a fresh
    plan's (pos_first / pos_last / pos_gap of the vector before must not survive the upload)"""
    from stereo_amd.trws import TrwsPlan
    K = 16
    unary, conn, alphas = _inputs("path2-shared")
    other = np.random.default_rng(7).permutation(K).astype(np.float64)
    used = TrwsPlan(1, K, H * W, conn.T)
    used.upload(unary.T, alphas, 4.0, positions=np.arange(K, dtype=np.float64))
    used.iterate(2, NEVER)
    used.upload(unary.T, alphas, 4.0, positions=other)
    fresh = TrwsPlan(1, K, H * W, conn.T)
    fresh.upload(unary.T, alphas, 4.0, positions=other)
    assert used.path() == fresh.path()
    assert used.spec_stats()["active"] == fresh.spec_stats()["active"]
    used.iterate(3, NEVER)
    fresh.iterate(3, NEVER)
    assert _same(_obs(used), _obs(fresh))
    _same_state(used.save_state(), fresh.save_state())
    used.close()
    fresh.close()
