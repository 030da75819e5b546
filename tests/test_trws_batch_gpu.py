"""-m gpu: batches of independent TRW-S plans (stereo_trws_batch_*, TrwsBatch).

The bar for every member of every batch: labels, energy, lower bound and iteration count are BITWISE what the same
plan gives when it is solved alone (np.array_equal / ==, no tolerance) -- which is what the other test files hold to
the oracle.  Shapes are the smallest at which each path can go wrong; a fixed iteration count is max_relgap=-1e300.
"""
import numpy as np
import pytest

from helpers import grid_conn, trws_problem

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_MESSAGES",
       "STEREO_HIP_TRWS_BLOCKS", "STEREO_HIP_TRWS_GRANULES", "STEREO_HIP_TRWS_CERTIFICATE")
NEVER = -1e300


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _fronto(seed, H, W, K, alphas="random"):
    """One shared ascending positions vector 0 .. K - 1 (test_min_marginals_gpu.py's problems)."""
    rng = np.random.default_rng(seed)
    conn = grid_conn(H, W)
    E = conn.shape[0]
    pos = np.arange(K, dtype=np.float64)
    a = np.ones(E) if alphas == "unit" else rng.uniform(0.5, 2.0, size=E)
    return dict(unary=rng.uniform(0, 40, size=(H * W, K)), conn=conn, alphas=a, positions=pos)


def _plan(hip, kernel, p, tol):
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    plan = TrwsPlan(kernel, K, N, p["conn"].T)
    if "positions" in p:
        plan.upload(p["unary"].T, p["alphas"], tol, positions=p["positions"])
    else:
        plan.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)
    return plan


def _solo(hip, kernel, p, tol, iters, max_relgap=NEVER):
    plan = _plan(hip, kernel, p, tol)
    done, _ = plan.iterate(iters, max_relgap)
    res = plan.result()
    plan.close()
    return res, done


def _same(plan, solo):
    lab, en, lb, it = plan.result()
    assert np.array_equal(lab, solo[0]), int((lab != solo[0]).sum())
    assert en == solo[1] and lb == solo[2] and it == solo[3], ((en, lb, it), solo[1:])


def _batch_equals_solo(hip, kernel, problems, tol, iters, path, before_batch=lambda: None):
    """Every member of one batch over `problems` against its solo solve; returns the batch's stats."""
    from stereo_amd.trws import TrwsBatch
    solos = [_solo(hip, kernel, p, tol, iters)[0] for p in problems]
    plans = [_plan(hip, kernel, p, tol) for p in problems]
    assert all(pl.path() == path for pl in plans)
    before_batch()
    with TrwsBatch(plans) as batch:
        assert batch.iterate(iters, NEVER) == [iters] * len(plans)
        stats = batch.stats()
    for pl, s in zip(plans, solos):
        _same(pl, s)
        pl.close()
    return stats


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("B", [2, 3])
def test_equal_members(hip, kernel, B):
    problems = [trws_problem(100 + 10 * kernel + i, 9, 40, 8, kind="general") for i in range(B)]
    _batch_equals_solo(hip, kernel, problems, 3.0, 4, 2)


@pytest.mark.parametrize("small_first", [True, False])
def test_floating_workgroups(hip, small_first, monkeypatch):
    """A 6 x 7 member next to a 60 x 70 one: the small member's workgroups run out of tickets at once and must move
    over -- the device-side counter in the batch's control words says that some workgroup held runs of both.
    Both problems together have fewer runs than the device keeps workgroups resident, so left alone every run gets a
    workgroup of its own and nobody has a reason to move; the batch is therefore held to eight workgroups (the
    development switch that caps a launch), which is the situation floating exists for: more runs than workgroups."""
    small, large = trws_problem(201, 6, 7, 8, kind="general"), trws_problem(202, 60, 70, 16, kind="general")
    stats = _batch_equals_solo(hip, 1, [small, large] if small_first else [large, small], 3.0, 3, 2,
                               before_batch=lambda: monkeypatch.setenv("STEREO_HIP_TRWS_BLOCKS", "8"))
    assert stats["capacity"] == 8, stats
    assert stats["floated"] >= 1, stats
    assert stats["launches"] == 1 + 2 * 3, stats          # forward once, then backward + fused per iteration: never split


def test_exact_ties(hip):
    """Integer costs and positions: exact ties everywhere, certificates fail, the serial envelope runs inside a batch."""
    from stereo_amd.trws import TrwsBatch
    tie, real = trws_problem(301, 18, 22, 9, kind="general", integer=True), trws_problem(302, 18, 22, 9, kind="general")
    solos = [_solo(hip, 1, p, 3.0, 4)[0] for p in (tie, real)]
    plans = [_plan(hip, 1, p, 3.0) for p in (tie, real)]
    before = plans[0].serial_messages(reset=True)
    with TrwsBatch(plans) as batch:
        batch.iterate(4, NEVER)
    assert plans[0].serial_messages() > 0, before
    for pl, s in zip(plans, solos):
        _same(pl, s)
        pl.close()


def test_shared_positions_and_mixed_instantiation(hip):
    """(30, 40, 16), shared ascending positions, unit weights: alone it runs the speculative border-chain schedule.  With
    a per-edge-positions member the batch is a mixed instantiation; with a second shared-positions member it is
    accepted, runs WITHOUT the speculative schedule (stereo_hip.h) and still gives the solo bits."""
    from stereo_amd import StereoHipError
    from stereo_amd.trws import TrwsBatch
    a, b = _fronto(401, 30, 40, 16, alphas="unit"), _fronto(402, 30, 40, 16, alphas="unit")
    edge = trws_problem(403, 9, 10, 16, kind="general")
    solos = [_solo(hip, 1, p, 4.0, 3)[0] for p in (a, b)]
    pa, pb, pe = _plan(hip, 1, a, 4.0), _plan(hip, 1, b, 4.0), _plan(hip, 1, edge, 4.0)
    assert pa.spec_stats()["active"] and pb.spec_stats()["active"]          # what they would run alone
    with pytest.raises(StereoHipError, match=r"member 1 .*kind of positions.*mixed instantiations"):
        TrwsBatch([pa, pe])
    with TrwsBatch([pa, pb]) as batch:
        batch.iterate(3, NEVER)
        assert batch.stats()["spec"] is False
    for pl in (pa, pb):                                                     # off: no runner visit, no commit happened
        st = pl.spec_stats()
        assert st["runner_visits"] == 0 and st["commits"] == 0 and st["second_walks"] == 0, st
    _same(pa, solos[0]); _same(pb, solos[1])
    for pl in (pa, pb, pe):
        pl.close()


def test_static_partition_pipe2_and_wide(hip):
    stats = _batch_equals_solo(hip, 1, [trws_problem(501 + i, 10, 12, 100, kind="general") for i in range(2)], 4.0, 2, 4)
    assert stats["floated"] == 0
    stats = _batch_equals_solo(hip, 1, [_fronto(511 + i, 12, 14, 256) for i in range(2)], 6.0, 2, 3)
    assert stats["floated"] == 0


def test_static_batch_split_into_consecutive_launches(hip, monkeypatch):
    """Pipe2 members whose static shares do not fit together go into consecutive launches: held to ONE resident
    workgroup (the development switch that caps a launch), every sweep of two members is two launches."""
    problems = [trws_problem(521 + i, 10, 12, 100, kind="general") for i in range(2)]
    stats = _batch_equals_solo(hip, 1, problems, 4.0, 2, 4, before_batch=lambda: monkeypatch.setenv("STEREO_HIP_TRWS_BLOCKS", "1"))
    assert stats["capacity"] == 1 and stats["floated"] == 0, stats
    assert stats["launches"] == 2 * (1 + 2 * 2), stats


def test_individual_stop(hip):
    from stereo_amd.trws import TrwsBatch
    problems = [trws_problem(61, 8, 9, 8, kind="general"), trws_problem(62, 12, 10, 12, kind="general")]
    gap, cap = 0.004, 12
    solos = [_solo(hip, 1, p, 3.0, cap, gap) for p in problems]
    counts = [d for _, d in solos]
    assert counts[0] != counts[1] and max(counts) < cap, counts             # both stop, at different iterations
    plans = [_plan(hip, 1, p, 3.0) for p in problems]
    with TrwsBatch(plans) as batch:
        assert batch.iterate(cap, gap) == counts
        for pl, (s, _) in zip(plans, solos):
            _same(pl, s)
        # stopped members do not move
        assert batch.iterate(2, gap) == [0, 0]
        for pl, (s, _) in zip(plans, solos):
            _same(pl, s)
    for pl in plans:
        pl.close()


def test_one_member_reset_and_solo_then_batch(hip):
    from stereo_amd.trws import TrwsBatch
    pa, pb = trws_problem(701, 9, 11, 10, kind="general"), trws_problem(702, 7, 13, 12, kind="general")
    sa, sb = _solo(hip, 1, pa, 3.0, 4)[0], _solo(hip, 1, pb, 3.0, 4)[0]
    # B = 1 is the plain plan
    assert _batch_equals_solo(hip, 1, [pa], 3.0, 4, 2)["floated"] == 0
    # a batch after reset() equals a fresh batch
    plans = [_plan(hip, 1, pa, 3.0), _plan(hip, 1, pb, 3.0)]
    with TrwsBatch(plans) as batch:
        batch.iterate(2, NEVER)
        batch.reset()
        assert plans[0].result()[3] == 0
        assert batch.iterate(4, NEVER) == [4, 4]
    _same(plans[0], sa); _same(plans[1], sb)
    # a member iterated alone for one iteration, then batched: solo bits for the same total
    # (its forward sweep is pending and its epoch is ahead of the other member's)
    for pl in plans:
        pl.reset()
    plans[0].iterate(1, NEVER)
    with TrwsBatch(plans) as batch:
        assert batch.iterate(3, NEVER) == [3, 3]
        _same(plans[0], sa)
        assert batch.iterate(1, NEVER) == [1, 1]
    _same(plans[1], sb)
    for pl in plans:
        pl.close()


def test_refusals(hip):
    from stereo_amd import StereoHipError
    from stereo_amd.trws import TrwsBatch, TrwsPlan, MESSAGES_MINPLUS
    good = trws_problem(801, 6, 7, 8, kind="general")
    ok = _plan(hip, 1, good, 3.0)
    members = [ok]

    def refused(plans, pattern):
        with pytest.raises(StereoHipError, match=pattern):
            TrwsBatch(plans)

    generic = _plan(hip, 1, trws_problem(802, 3, 4, 300, kind="general"), 3.0)          # K = 300, per-edge positions
    members.append(generic)
    assert generic.path() == 1
    refused([ok, generic], r"member 1 runs the generic kernel family")
    large = _plan(hip, 1, _fronto(803, 3, 4, 600), 7.0)
    members.append(large)
    assert large.path() == 5
    refused([ok, large], r"member 1 runs the large kernel family")
    quad = _plan(hip, 2, good, 3.0)
    members.append(quad)
    refused([ok, quad], r"member 1 .*smoothness kernel.*mixed instantiations")
    shared = _plan(hip, 1, _fronto(804, 6, 7, 8), 3.0)
    members.append(shared)
    refused([ok, ok, shared], r"member 1 is in the batch already")
    refused([ok, shared], r"member 1 .*kind of positions.*mixed instantiations")
    pipe2 = _plan(hip, 1, trws_problem(805, 4, 5, 80, kind="general"), 3.0)
    members.append(pipe2)
    refused([ok, pipe2], r"member 1 .*kernel family.*mixed instantiations")
    N, K = good["unary"].shape
    bare = TrwsPlan(1, K, N, good["conn"].T)
    members.append(bare)
    refused([ok, bare], r"member 1 has no inputs")
    refused([], r"needs 1 \.\. 16 plans")
    refused([ok] * 17, r"member 16 does not fit")
    # a strip (two logical strips of the 6 x 7 grid on this device)
    import ctypes as C
    from stereo_amd import _lib
    conn = np.asfortranarray(good["conn"].T, dtype=np.uint32)
    from stereo_amd.strips import row_strip_owner
    owner = np.ascontiguousarray(row_strip_owner(6, 7, 2), dtype=np.int32)
    strip = C.c_void_p()
    err = _lib.errbuf()
    rc = _lib.lib().stereo_trws_plan_create_strip(C.c_int(1), C.c_int(K), C.c_int64(N), C.c_int64(conn.shape[1]),
                                                  conn.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(0),
                                                  owner.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(2), C.c_int(0), C.c_int(0), None,
                                                  C.byref(strip), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    arr = (C.c_void_p * 2)(ok._h, strip)
    out = C.c_void_p()
    rc = _lib.lib().stereo_trws_batch_create(arr, C.c_int(2), C.byref(out), err, C.c_size_t(len(err)))
    assert rc != 0 and not out.value and b"member 1 is a row strip" in err.value, err.value
    _lib.lib().stereo_trws_plan_destroy(strip)
    # every member is as usable as before
    solo = _solo(hip, 1, good, 3.0, 2)[0]
    ok.iterate(2, NEVER)
    _same(ok, solo)
    quad.iterate(1, NEVER)
    for pl in members:
        pl.close()


def test_beliefs_inside_a_batch(hip):
    """A member that keeps min-marginals gets its phase-1 launch in every batch iteration: the same beliefs as alone,
    and the member without them is not touched."""
    from stereo_amd.trws import TrwsBatch
    pa, pb = trws_problem(901, 7, 8, 12, kind="general"), trws_problem(902, 9, 6, 10, kind="general")
    alone = _plan(hip, 1, pa, 3.0)
    alone.keep_min_marginals()
    alone.iterate(3, NEVER)
    want = alone.min_marginals()
    alone.close()
    sb = _solo(hip, 1, pb, 3.0, 3)[0]
    plans = [_plan(hip, 1, pa, 3.0), _plan(hip, 1, pb, 3.0)]
    plans[0].keep_min_marginals()
    with TrwsBatch(plans) as batch:
        batch.iterate(3, NEVER)
    got = plans[0].min_marginals()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    _same(plans[1], sb)
    with pytest.raises(Exception, match="no min-marginals"):
        plans[1].min_marginals()
    for pl in plans:
        pl.close()
