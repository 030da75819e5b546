"""-m gpu: stereo_trws_plan_iterate launches the next backward sweep before the host has summed the iteration before it
(trws_plan.hip: issue_backward_ahead).

When the stop test fires, that sweep is already running; the plan keeps it pending and the next iterate takes it.
Nothing of it may show at the API: after every call, labels, energy, bound, iteration count, the sweep launches counted,
serial_messages, spec_stats and the lower-bound terms of stereo_trws_plan_debug_terms must be what a loop of
iterate(1) calls returns -- that loop never asks for a further iteration, so it never launches ahead and is the
schedule the plan had before.  The same list of calls is run both ways on 10 x 40 x 16 and compared call by call.

The stop threshold comes from the gaps (E - LB) / E that the iterate(1) loop records: half way between the gap after
iteration 1 and the gap after iteration 2, so a call for 6 iterations stops after 2, with the third backward sweep
launched.

A stopped call returns with that sweep still running on its stream: the call that takes it may come on another stream,
or from a batch (always the null stream), and must wait for it -- the same lists of calls with the stopping call on a
non-blocking side stream.  Min-marginals: a plan that keeps them never launches ahead, so the case is a stop with a
pending sweep, then keep_min_marginals, one more iteration and the read."""
import ctypes as C

import numpy as np
import pytest

from helpers import grid_conn

pytestmark = pytest.mark.gpu

H, W, K = 10, 40, 16
NEVER = -1e300
ENV = ("STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_DEBUG", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_ROW_CHUNK")


def _problem():
    rng = np.random.default_rng(11)
    conn = grid_conn(H, W)
    unary = rng.uniform(0, 40, size=(H * W, K))
    return unary, conn, rng.uniform(0.5, 2.0, size=conn.shape[0])


def _upload(plan, where, unary, conn, alphas):
    if where == "shared":
        plan.upload(unary.T, alphas, 4.0, positions=np.arange(K, dtype=np.float64))
    else:
        q = np.tile(np.random.default_rng(5).permutation(K).astype(np.float64), (conn.shape[0], 1))
        plan.upload(unary.T, alphas, 4.0, q=q.T, qprim=q.T)


def _terms(plan):
    from stereo_amd import _lib
    n = C.c_int64()
    _lib.lib().stereo_trws_plan_debug_terms(plan._h, None, C.c_int64(0), C.byref(n))
    out = np.zeros(n.value)
    _lib.lib().stereo_trws_plan_debug_terms(plan._h, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(n.value), C.byref(n))
    return out


def _observe(plan):
    lab, en, lb, it = plan.result()
    return dict(labels=lab.copy(), energy=en, bound=lb, iterations=it, launches=plan.stats()[1],
                serial=plan.serial_messages(), spec=plan.spec_stats(), terms=_terms(plan))


_streams = {}


def _stream(name):
    """a non-blocking side stream per name (not ordered against the null stream), as a raw handle"""
    import torch
    if name not in _streams:
        _streams[name] = torch.cuda.Stream()
    return _streams[name].cuda_stream


def _iterate(plan, n, gap, single, stream=None):
    """single: a loop of iterate(1, gap) on the null stream that ends where the stop test fires"""
    if not single:
        return plan.iterate(n, max_relgap=gap, stream=_stream(stream) if stream else None)
    done, stopped = 0, False
    while done < n and not stopped:
        d, stopped = plan.iterate(1, max_relgap=gap)
        done += d
    return done, stopped


def _run(where, calls, single):
    """The calls on a fresh plan; what the plan shows after each.  single: every ("iterate", n, gap[, stream]) as a loop
    of iterate(1, gap) on the null stream."""
    from stereo_amd.trws import TrwsPlan
    unary, conn, alphas = _problem()
    plan = TrwsPlan(1, K, H * W, conn.T)
    _upload(plan, where, unary, conn, alphas)
    seen = []
    for call in calls:
        if call[0] == "iterate":
            done, stopped = _iterate(plan, call[1], call[2], single, call[3] if len(call) > 3 else None)
            seen.append(("iterate", done, stopped, _observe(plan)))
        elif call[0] == "keep-min-marginals":
            plan.keep_min_marginals(True)
            seen.append(("keep-min-marginals", _observe(plan)))
        elif call[0] == "min-marginals":
            mm, conf, arg = plan.min_marginals()
            seen.append(("min-marginals", dict(mm=mm, conf=conf, arg=arg)))
        elif call[0] == "reset":
            plan.reset()
            seen.append(("reset", _observe(plan)))
        elif call[0] == "upload":
            _upload(plan, where, unary * call[1], conn, alphas)
            seen.append(("upload", _observe(plan)))
        elif call[0] == "zero-counters":
            seen.append(("zero-counters", plan.serial_messages(reset=True), plan.stats(reset=True)[1]))
    plan.close()
    return seen


def _equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if not _equal(g, w):
            what = [k for k in g[-1] if not _equal(g[-1][k], w[-1][k])] if isinstance(g[-1], dict) else []
            raise AssertionError("call %d (%s): differs in %s; head %r against %r" % (i, g[0], what or "its return", g[:-1], w[:-1]))


@pytest.fixture(scope="module", params=["shared", "edges"])
def setting(request, hip):
    """(positions, gap that stops after iteration 2 of 6), from the gaps of the iterate(1) loop"""
    import os
    saved = {k: os.environ.pop(k) for k in ENV if k in os.environ}
    try:
        trace = _run(request.param, [("iterate", 1, NEVER)] * 6, True)
        gaps = [(o["energy"] - o["bound"]) / o["energy"] for _, _, _, o in trace]
        assert gaps[1] < gaps[0] and all(g > 0 for g in gaps), gaps
        yield request.param, 0.5 * (gaps[0] + gaps[1])
    finally:
        os.environ.update(saved)


def test_trace_is_the_oracle(setting, oracle):
    """the yardstick itself: the iterate(1) loop against the CPU oracle"""
    where, _ = setting
    unary, conn, alphas = _problem()
    q = np.tile(np.arange(K, dtype=np.float64), (conn.shape[0], 1)) if where == "shared" else \
        np.tile(np.random.default_rng(5).permutation(K).astype(np.float64), (conn.shape[0], 1))
    ref = oracle.trws(1, unary, conn, q, q, alphas, 4.0, 5, 0.0, mode=1)
    got = _run(where, [("iterate", 5, NEVER)], True)[0][3]
    assert np.array_equal(ref[0], got["labels"]) and (ref[1], ref[2], ref[3]) == (got["energy"], got["bound"], got["iterations"])


def test_five_at_once_equal_five_single(setting):
    where, _ = setting
    calls = [("iterate", 5, NEVER)]
    _assert_same(_run(where, calls, False), _run(where, calls, True))


def test_stop_in_mid_call_and_going_on(setting):
    where, gap = setting
    calls = [("iterate", 6, gap), ("iterate", 2, NEVER), ("iterate", 1, NEVER)]
    got, want = _run(where, calls, False), _run(where, calls, True)
    assert want[0][1:3] == (2, True)   # (the threshold does what it was chosen for)
    _assert_same(got, want)
    # ... and the uninterrupted run
    whole = _run(where, [("iterate", 5, NEVER)], True)
    assert _equal(got[2][3], whole[0][3])


def test_counters_zeroed_after_a_stop(setting):
    where, gap = setting
    calls = [("iterate", 6, gap), ("zero-counters",), ("iterate", 2, NEVER)]
    _assert_same(_run(where, calls, False), _run(where, calls, True))


def test_reset_and_upload_after_a_stop(setting):
    where, gap = setting
    calls = [("iterate", 6, gap), ("reset",), ("iterate", 3, NEVER), ("iterate", 6, gap), ("upload", 0.5), ("iterate", 3, NEVER)]
    _assert_same(_run(where, calls, False), _run(where, calls, True))


def test_stop_on_one_stream_go_on_on_another(setting):
    where, gap = setting
    calls = [("iterate", 6, gap, "a"), ("iterate", 2, NEVER), ("iterate", 6, gap, "b"), ("iterate", 2, NEVER, "a"),
             ("iterate", 6, gap), ("iterate", 1, NEVER, "b")]
    got, want = _run(where, calls, False), _run(where, calls, True)
    assert want[0][1:3] == (2, True)
    _assert_same(got, want)


def test_min_marginals_after_a_stop(setting):
    where, gap = setting
    calls = [("iterate", 6, gap, "a"), ("keep-min-marginals",), ("iterate", 1, NEVER), ("min-marginals",), ("iterate", 3, NEVER),
             ("min-marginals",)]
    _assert_same(_run(where, calls, False), _run(where, calls, True))


def test_batch_takes_a_pending_sweep(setting):
    """a member stopped on a side stream with its next backward sweep launched, a fresh member: the batch's shared
    launches (null stream) take the one and launch for the other"""
    from stereo_amd.trws import TrwsPlan, TrwsBatch
    where, gap = setting
    unary, conn, alphas = _problem()

    def both(single):
        plans = [TrwsPlan(1, K, H * W, conn.T) for _ in range(2)]
        _upload(plans[0], where, unary, conn, alphas)
        _upload(plans[1], where, unary * 0.5, conn, alphas)
        head = _iterate(plans[0], 6, gap, single, "a")
        with TrwsBatch(plans) as batch:
            done = batch.iterate(2, NEVER)
            stats = batch.stats()
        seen = [head, done, stats["launches"]] + [_observe(p) for p in plans]
        for p in plans:
            p.close()
        return seen

    got, want = both(False), both(True)
    assert want[0] == (2, True) and want[1] == [2, 2]
    assert _equal(got, want)
