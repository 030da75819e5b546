"""-m gpu: node beliefs on row strips and the grouped belief launches.

Every strip keeps the beliefs of its own nodes; put together at their node ids they are the single plan's
min-marginals, confidence and argmin bit for bit (np.array_equal everywhere, no tolerance) -- the single plan's are held
to tests/mm_restate.py by test_min_marginals_gpu.py, and one case here is compared with mm_restate directly.  Strips that
share the device, and the members of a batch, take phase 1 in ONE launch per iteration; the grouped device read fills
arrays of the whole problem in one launch.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grid_conn, trws_problem
from mm_restate import default_impl, trws_beliefs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_MESSAGES",
       "STEREO_HIP_TRWS_BELIEFS_STRIPS")
TS = (1, 2, 5)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _fronto(seed, H, W, K):
    rng = np.random.default_rng(seed)
    conn = grid_conn(H, W)
    E = conn.shape[0]
    pos = np.arange(K, dtype=np.float64)
    return dict(unary=rng.uniform(0, 40, size=(H * W, K)), conn=conn, q=np.tile(pos, (E, 1)), qprim=np.tile(pos, (E, 1)),
                alphas=rng.uniform(0.5, 2.0, size=E)), pos


def _upload(s, p, tol, positions=None):
    if positions is not None:
        s.upload(p["unary"].T, p["alphas"], tol, positions=positions)
    else:
        s.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)


def _single(kernel, p, tol, mode=0, positions=None, ts=TS):
    """The single plan's (path, [(labels, energy, bound, iterations, mm, conf, argmin) at every t])."""
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    plan = TrwsPlan(kernel, K, N, p["conn"].T, mode)
    _upload(plan, p, tol, positions)
    plan.keep_min_marginals()
    out, done = [], 0
    for t in ts:
        plan.iterate(t - done, max_relgap=-1e300)
        done = t
        out.append(plan.result() + plan.min_marginals())
    path = plan.path()
    plan.close()
    return path, out


def _strips(kernel, p, H, W, G, tol, mode=0, positions=None, wg=None):
    from stereo_amd.strips import make_strips
    K = p["unary"].shape[1]
    s = make_strips(kernel, K, H, W, p["conn"].T, G, message_mode=mode, workgroups_per_strip=wg)
    _upload(s, p, tol, positions)
    return s


def _same(got, want):
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def _check(kernel, p, H, W, G, tol, mode=0, positions=None, wg=None, path=None, restate=None):
    ref_path, ref = _single(kernel, p, tol, mode, positions)
    if path is not None:
        assert ref_path == path
    s = _strips(kernel, p, H, W, G, tol, mode, positions, wg)
    s.keep_min_marginals()
    assert s.path() == ref_path
    done = 0
    for t, r in zip(TS, ref):
        s.iterate(t - done, max_relgap=-1e300)      # one run, no reset in between
        done = t
        lab, en, lb, it = s.result()
        assert np.array_equal(lab, r[0]) and it == r[3]
        mm, conf, am = s.min_marginals()
        assert mm.shape == r[4].shape
        _same((mm, conf, am), r[4:])
        if restate is not None:
            oracle, minplus, ordering = restate
            m = trws_beliefs(oracle, default_impl(oracle, minplus), kernel, p, tol, t, ordering=ordering)
            _same((mm, conf, am), (m["mm"].T, m["confidence"], m["argmin"] + 1))
    infos = [pl.info() for pl in s.plans]
    s.close()
    return infos


@pytest.mark.parametrize("G", [2, 4])
def test_kernel1_per_edge_positions(G, hip, oracle):
    # 8 x 6 x 15: four nodes per wave, 120-byte rows; G = 4: strips of two rows
    _check(1, trws_problem(301, 8, 6, 15, kind="general"), 8, 6, G, 3.0, path=2, restate=(oracle, False, 0) if G == 2 else None)


def test_kernel2_strips_of_two_and_three_rows(hip):
    _check(2, trws_problem(302, 9, 7, 9, kind="general"), 9, 7, 4, 9.0, path=2)


@pytest.mark.parametrize("G", [2, 3])
def test_path4_strided_label_loop(G, hip):
    _check(1, trws_problem(303, 6, 5, 80, kind="general"), 6, 5, G, 4.0, path=4)


def test_path3_shared_ascending_positions(hip):
    p, pos = _fronto(304, 6, 6, 100)
    _check(1, p, 6, 6, 2, 6.0, positions=pos, path=3)


def test_integer_costs_exact_ties(hip):
    p = trws_problem(305, 8, 6, 9, kind="general", integer=True)
    _, ref = _single(1, p, 2.0, ts=(2,))
    assert (ref[0][5] == 0).any()       # confidence 0: two labels tie for the minimum somewhere
    _check(1, p, 8, 6, 2, 2.0)


def test_two_labels(hip):
    _check(1, trws_problem(306, 8, 6, 2, kind="general"), 8, 6, 2, 3.0)


def test_beliefs_change_nothing_else(hip):
    p = trws_problem(307, 8, 6, 15, kind="general")
    out = []
    for on in (False, True):
        s = _strips(1, p, 8, 6, 2, 3.0)
        if on:
            s.keep_min_marginals()
        res = []
        for _ in range(4):
            s.iterate(1, max_relgap=-1e300)
            lab, en, lb, it = s.result()
            res.append((lab.copy(), en, lb, it))
        out.append(res)
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_fewer_workgroups_than_runs(hip):
    infos = _check(1, trws_problem(308, 8, 6, 15, kind="general"), 8, 6, 2, 3.0, wg=2)
    assert all(i["runs_forward"] > 2 and i["runs_backward"] > 2 for i in infos)


def test_index_order(hip, oracle):
    from stereo_amd.trws import ORDER_INDEX
    _check(1, trws_problem(309, 8, 6, 10, kind="general"), 8, 6, 2, 3.0, mode=ORDER_INDEX)


def test_minplus_mode(hip):
    from stereo_amd.trws import MESSAGES_MINPLUS
    # (strips take the min-plus mode on the wide kernel's plain min-plus branch only: 64 < K <= 256, shared positions)
    p, pos = _fronto(310, 8, 6, 70)
    _check(1, p, 8, 6, 2, 6.0, mode=MESSAGES_MINPLUS, positions=pos, path=3)


def test_lifecycle(hip):
    from stereo_amd import StereoHipError
    p = trws_problem(311, 8, 6, 12, kind="general")
    _, ref = _single(1, p, 3.0, ts=(2, 3, 5))
    s = _strips(1, p, 8, 6, 2, 3.0)
    with pytest.raises(StereoHipError, match="no min-marginals"):      # flag off
        s.min_marginals()
    s.keep_min_marginals()
    with pytest.raises(StereoHipError, match="no min-marginals"):      # before any iteration
        s.min_marginals()
    s.keep_min_marginals(False)
    s.iterate(1, max_relgap=-1e300)
    s.keep_min_marginals()                                             # turned on in mid-run
    with pytest.raises(StereoHipError, match="no min-marginals"):      # no iteration since
        s.min_marginals()
    s.iterate(1, max_relgap=-1e300)
    a = s.min_marginals()
    _same(a, ref[0][4:])
    _same(s.min_marginals(), a)                                        # twice: the same bits
    # the plan-level entries still refuse a strip, and say so
    from stereo_amd import _lib
    import ctypes as C
    err = _lib.errbuf()
    assert _lib.lib().stereo_trws_plan_keep_min_marginals(s.plans[0]._h, C.c_int(1), err, C.c_size_t(len(err))) != 0
    assert b"strip" in err.value
    assert _lib.lib().stereo_trws_plan_min_marginals(s.plans[0]._h, None, None, None, err, C.c_size_t(len(err))) != 0
    assert b"strip" in err.value
    s.keep_min_marginals(False)
    with pytest.raises(StereoHipError, match="no min-marginals"):
        s.min_marginals()
    s.keep_min_marginals()
    s.iterate(1, max_relgap=-1e300)
    _same(s.min_marginals(), ref[1][4:])
    _upload(s, p, 3.0)                                                 # new inputs: a new minimisation
    with pytest.raises(StereoHipError, match="no min-marginals"):
        s.min_marginals()
    s.iterate(5, max_relgap=-1e300)
    _same(s.min_marginals(), ref[2][4:])
    s.close()


def test_one_strip_through_the_strip_entries(hip):
    """nstrips = 1: the strip entries on a plan of the whole problem are the plan's own."""
    p = trws_problem(312, 8, 6, 12, kind="general")
    _, ref = _single(1, p, 3.0, ts=(3,))
    s = _strips(1, p, 8, 6, 1, 3.0)
    s.keep_min_marginals()
    s.iterate(3, max_relgap=-1e300)
    _same(s.min_marginals(), ref[0][4:])
    s.close()


@pytest.mark.parametrize("case", [(8, 6, 15, 4), (6, 5, 80, 3)], ids=["k15", "k80"])
def test_grouped_device_read(case, hip):
    import torch
    H, W, K, G = case
    p = trws_problem(313, H, W, K, kind="general")
    s = _strips(1, p, H, W, G, 3.0)
    s.keep_min_marginals()
    s.iterate(3, max_relgap=-1e300)
    mm, conf, am = s.min_marginals()
    N = H * W
    d_mm = torch.full((N, K), float("nan"), dtype=torch.float64, device="cuda")
    d_conf = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    d_am = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.min_marginals_device(d_mm.data_ptr(), d_conf.data_ptr(), d_am.data_ptr())
    torch.cuda.synchronize()
    h_mm, h_conf, h_am = d_mm.cpu().numpy().T, d_conf.cpu().numpy(), d_am.cpu().numpy()
    assert not np.isnan(h_mm).any() and not np.isnan(h_conf).any() and (h_am >= 0).all()
    _same((h_mm, h_conf, h_am + 1), (mm, conf, am))
    d_c2 = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.min_marginals_device(None, d_c2.data_ptr(), None)                # any output may be left out
    torch.cuda.synchronize()
    assert np.array_equal(d_c2.cpu().numpy(), conf)
    s.close()


def test_batch_members_share_the_phase1_launch(hip):
    from stereo_amd.trws import TrwsBatch, TrwsPlan
    shapes = [(7, 8, 9), (10, 6, 15), (12, 12, 40)]
    probs = [trws_problem(320 + i, H, W, K, kind="general") for i, (H, W, K) in enumerate(shapes)]
    solo = [_single(1, p, 3.0, ts=(1, 3))[1] for p in probs]
    plans = []
    for p, (H, W, K) in zip(probs, shapes):
        plan = TrwsPlan(1, K, H * W, p["conn"].T)
        _upload(plan, p, 3.0)
        plan.keep_min_marginals()
        plans.append(plan)
    with TrwsBatch(plans) as batch:
        done = 0
        for k, t in enumerate((1, 3)):
            assert batch.iterate(t - done, max_relgap=-1e300) == [t - done] * 3
            done = t
            for plan, ref in zip(plans, solo):
                lab, en, lb, it = plan.result()
                assert np.array_equal(lab, ref[k][0]) and (en, lb, it) == ref[k][1:4]
                _same(plan.min_marginals(), ref[k][4:])
    for plan in plans:
        plan.close()


def test_gateway_shards_the_belief_call(hip, monkeypatch):
    from stereo_amd import _lib
    strips_used = lambda: int(_lib.lib().stereo_trws_gateway_strips())
    p = trws_problem(330, 12, 10, 9, kind="fronto")
    args = (1, p["unary"].T, p["conn"].T + 1, p["q"].T, p["qprim"].T, p["alphas"], 3.0, dict(maxiter=5, max_relgap=0.0))
    monkeypatch.setenv("STEREO_HIP_GPUS", "2")
    want = hip.trws(*args, min_marginals=True)
    assert strips_used() == 1
    monkeypatch.setenv("STEREO_HIP_TRWS_BELIEFS_STRIPS", "1")
    for _ in range(2):                                                 # the second call: the cached strips
        got = hip.trws(*args, min_marginals=True)
        assert strips_used() == 2
        assert len(got) == len(want) == 6
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    monkeypatch.delenv("STEREO_HIP_TRWS_BELIEFS_STRIPS")
    hip.trws(*args, min_marginals=True)
    assert strips_used() == 1
    _lib.lib().stereo_trws_cache_clear()


def test_two_processes_through_ipc(hip):
    """One strip per PROCESS (tools/strips_beliefs_ipc_check.py; both ranks share the GPU here): every rank's own rows
    equal a single plan's."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29547", os.path.join(ROOT, "tools", "strips_beliefs_ipc_check.py"), "40", "46", "16"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "IPC_BELIEFS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_one_process_driving_two_devices(hip):
    """TrwsStrips(devices=[0, 1]): a strip per GPU, each with its own phase-1 launch.  Skipped with one GPU."""
    from stereo_amd.strips import TrwsStrips, row_strip_owner
    if hip.device_count() < 2:
        pytest.skip("one GPU visible")
    H, W, K = 24, 20, 12
    p = trws_problem(340, H, W, K, kind="general")
    _, ref = _single(1, p, 2.5, ts=(4,))
    s = TrwsStrips(1, K, H * W, p["conn"].T, row_strip_owner(H, W, 2), 2, devices=[0, 1])
    _upload(s, p, 2.5)
    s.keep_min_marginals()
    s.iterate(4, max_relgap=-1e300)
    _same(s.min_marginals(), ref[0][4:])
    s.close()
