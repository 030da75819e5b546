"""-m gpu: node beliefs after a run (stereo_trws_plan_keep_min_marginals / _min_marginals).

The plan's min-marginals, confidence and argmin equal tests/mm_restate.py's (t iterations of minimize.cpp plus the
forward pass of iteration t + 1 up to each node's Di) bit for bit, on every sweep kernel family, the speculative
border chain, the index order and the min-plus message mode; turning them on changes nothing else.
"""
import os
import sys

import numpy as np
import pytest

from helpers import grid_conn, trws_problem
from mm_restate import default_impl, trws_beliefs

pytestmark = pytest.mark.gpu

ENV = ("STEREO_HIP_TRWS_FAST", "STEREO_HIP_GPUS", "STEREO_HIP_TRWS_SPEC", "STEREO_HIP_TRWS_CACHE", "STEREO_HIP_TRWS_MESSAGES")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _fronto(seed, H, W, K, step=1.0, alphas="random"):
    rng = np.random.default_rng(seed)
    conn = grid_conn(H, W)
    E = conn.shape[0]
    pos = np.arange(K, dtype=np.float64) * step
    a = np.ones(E) if alphas == "unit" else rng.uniform(0.5, 2.0, size=E)
    return dict(unary=rng.uniform(0, 40, size=(H * W, K)), conn=conn, q=np.tile(pos, (E, 1)), qprim=np.tile(pos, (E, 1)),
                alphas=a), pos


def _plan(kernel, p, tol, mode=0, positions=None):
    from stereo_amd.trws import TrwsPlan
    N, K = p["unary"].shape
    plan = TrwsPlan(kernel, K, N, p["conn"].T, mode)
    if positions is not None:
        plan.upload(p["unary"].T, p["alphas"], tol, positions=positions)
    else:
        plan.upload(p["unary"].T, p["alphas"], tol, q=p["q"].T, qprim=p["qprim"].T)
    return plan


def _same_as_restatement(plan, r):
    mm, conf, am = plan.min_marginals()
    lab, en, lb, it = plan.result()
    assert it == r["iterations"]
    assert np.array_equal(lab, r["labels"]) and en == r["energy"] and lb == r["lb"]
    assert mm.shape == r["mm"].T.shape
    assert np.array_equal(mm, r["mm"].T), np.abs(mm - r["mm"].T).max()
    assert np.array_equal(conf, r["confidence"])
    assert np.array_equal(am, r["argmin"] + 1)


def _check(oracle, kernel, p, tol, path, mode=0, positions=None, ts=(1, 2, 5), minplus=False, ordering=0, spec=None):
    plan = _plan(kernel, p, tol, mode, positions)
    assert plan.path() == path
    plan.keep_min_marginals()
    done = 0
    for t in ts:
        plan.iterate(t - done, max_relgap=-1e300)
        done = t
        _same_as_restatement(plan, trws_beliefs(oracle, default_impl(oracle, minplus), kernel, p, tol, t, ordering=ordering))
    if spec is not None:
        assert plan.spec_stats()["active"] == spec
    plan.close()


def test_path2_pipelined(hip, oracle):
    _check(oracle, 1, trws_problem(21, 7, 8, 12, kind="general"), 3.0, 2)
    _check(oracle, 2, trws_problem(22, 6, 7, 15, kind="general"), 9.0, 2, ts=(2,))


def test_path4_two_labels_per_lane(hip, oracle):
    _check(oracle, 1, trws_problem(23, 4, 5, 80, kind="general"), 4.0, 4)


def test_path3_wide(hip, oracle):
    p, pos = _fronto(24, 5, 6, 100)
    _check(oracle, 1, p, 6.0, 3, positions=pos)


def test_path1_generic(hip, oracle, monkeypatch):
    _check(oracle, 1, trws_problem(25, 3, 4, 300, kind="general"), 5.0, 1, ts=(1, 2))
    monkeypatch.setenv("STEREO_HIP_TRWS_FAST", "0")
    _check(oracle, 1, trws_problem(26, 5, 6, 20, kind="general"), 3.0, 1)


def test_path5_large(hip, oracle):
    p, pos = _fronto(27, 3, 4, 600, step=0.25)
    _check(oracle, 1, p, 7.0, 5, positions=pos, ts=(1, 2))


def test_speculative_border_chain(hip, oracle):
    p, pos = _fronto(28, 30, 40, 16, alphas="unit")
    _check(oracle, 1, p, 4.0, 2, positions=pos, spec=True)


def test_index_order(hip, oracle):
    from stereo_amd.trws import ORDER_INDEX
    _check(oracle, 1, trws_problem(29, 6, 7, 10, kind="general"), 3.0, 2, mode=ORDER_INDEX, ordering=1)


def test_minplus_mode(hip, oracle):
    from stereo_amd.trws import MESSAGES_MINPLUS
    _check(oracle, 1, trws_problem(30, 6, 7, 10, kind="general"), 3.0, 1, mode=MESSAGES_MINPLUS, minplus=True)


def test_K1(hip, oracle):
    _check(oracle, 1, trws_problem(31, 4, 5, 1, kind="general"), 3.0, 2, ts=(1, 2))


def test_beliefs_change_nothing_else(hip):
    p, pos = _fronto(32, 20, 24, 16)
    out = []
    for on in (False, True):
        plan = _plan(1, p, 4.0, positions=pos)
        if on:
            plan.keep_min_marginals()
        res = []
        for _ in range(4):
            plan.iterate(1, max_relgap=-1e300)
            lab, en, lb, it = plan.result()
            res.append((lab.copy(), en, lb, it))
        out.append(res)
        plan.close()
    for a, b in zip(*out):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_device_variant_and_repeat(hip):
    import torch
    p = trws_problem(33, 6, 7, 12, kind="general")
    plan = _plan(1, p, 3.0)
    plan.keep_min_marginals()
    plan.iterate(3, max_relgap=-1e300)
    mm, conf, am = plan.min_marginals()
    mm2, conf2, am2 = plan.min_marginals()   # no iteration in between: the same bits
    assert np.array_equal(mm, mm2) and np.array_equal(conf, conf2) and np.array_equal(am, am2)
    N, K = p["unary"].shape
    d_mm = torch.zeros((N, K), dtype=torch.float64, device="cuda")
    d_conf = torch.zeros(N, dtype=torch.float64, device="cuda")
    d_am = torch.zeros(N, dtype=torch.int32, device="cuda")
    plan.min_marginals_device(d_mm.data_ptr(), d_conf.data_ptr(), d_am.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_mm.cpu().numpy().T, mm)
    assert np.array_equal(d_conf.cpu().numpy(), conf)
    assert np.array_equal(d_am.cpu().numpy() + 1, am)
    d_c2 = torch.zeros(N, dtype=torch.float64, device="cuda")
    plan.min_marginals_device(None, d_c2.data_ptr(), None)   # any output may be left out
    torch.cuda.synchronize()
    assert np.array_equal(d_c2.cpu().numpy(), conf)
    plan.close()


def test_error_cases(hip):
    from stereo_amd._lib import StereoHipError
    from stereo_amd.trws import TrwsPlan
    p = trws_problem(34, 5, 6, 8, kind="general")
    plan = _plan(1, p, 3.0)
    with pytest.raises(StereoHipError, match="no min-marginals"):
        plan.min_marginals()                       # flag never set
    plan.iterate(1, max_relgap=-1e300)
    plan.keep_min_marginals()
    with pytest.raises(StereoHipError, match="no min-marginals"):
        plan.min_marginals()                       # no phase 1 since the flag was set
    plan.iterate(1, max_relgap=-1e300)
    plan.min_marginals()
    plan.upload(p["unary"].T, p["alphas"], 3.0, q=p["q"].T, qprim=p["qprim"].T)
    with pytest.raises(StereoHipError, match="no min-marginals"):
        plan.min_marginals()                       # an upload starts a new minimisation
    plan.iterate(1, max_relgap=-1e300)
    plan.min_marginals()
    plan.reset()
    with pytest.raises(StereoHipError, match="no min-marginals"):
        plan.min_marginals()
    plan.iterate(1, max_relgap=-1e300)
    plan.keep_min_marginals(False)
    with pytest.raises(StereoHipError, match="no min-marginals"):
        plan.min_marginals()
    plan.close()
    # a row strip refuses both
    import ctypes as C
    from stereo_amd import _lib
    H, W, K = 8, 6, 8
    conn = np.asfortranarray(grid_conn(H, W).T, dtype=np.uint32)
    owner = np.array([min(i % H * 2 // H, 1) for i in range(H * W)], np.int32)
    h = C.c_void_p()
    err = _lib.errbuf()
    rc = _lib.lib().stereo_trws_plan_create_strip(C.c_int(1), C.c_int(K), C.c_int64(H * W), C.c_int64(conn.shape[1]),
                                                  conn.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(0),
                                                  owner.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(2), C.c_int(0),
                                                  C.c_int(0), None, C.byref(h), err, C.c_size_t(len(err)))
    _lib.check(rc, err)
    try:
        err = _lib.errbuf()
        assert _lib.lib().stereo_trws_plan_keep_min_marginals(h, C.c_int(1), err, C.c_size_t(len(err))) != 0
        assert b"strip" in err.value
        err = _lib.errbuf()
        assert _lib.lib().stereo_trws_plan_min_marginals(h, None, None, None, err, C.c_size_t(len(err))) != 0
        assert b"strip" in err.value
    finally:
        _lib.lib().stereo_trws_plan_destroy(h)


@pytest.mark.parametrize("gpus", [None, "2"])
def test_gateway_equals_the_plan(hip, monkeypatch, gpus):
    from stereo_amd import _lib
    from stereo_amd.trws import trws
    if gpus:
        monkeypatch.setenv("STEREO_HIP_GPUS", gpus)
    H, W, K = 12, 10, 9
    p, pos = _fronto(35, H, W, K)
    args = (1, p["unary"].T, p["conn"].T + 1, p["q"].T, p["qprim"].T, p["alphas"], 3.0, dict(maxiter=4, max_relgap=-1))
    plain = trws(*args)                               # (with STEREO_HIP_GPUS = 2: cached strips of the same problem)
    lab, en, lb, it, mm, conf = trws(*args, min_marginals=True)
    assert _lib.lib().stereo_trws_gateway_strips() == 1
    assert np.array_equal(lab, plain[0]) and (en, lb, it) == plain[1:]
    plan = _plan(1, p, 3.0, positions=pos)
    plan.keep_min_marginals()
    plan.iterate(4, max_relgap=-1e300)
    mm2, conf2, _ = plan.min_marginals()
    plan.close()
    assert mm.shape == (K, H * W) and np.array_equal(mm, mm2) and np.array_equal(conf, conf2)
    again = trws(*args)                               # a plain call afterwards: the same bits as before
    assert np.array_equal(again[0], plain[0]) and again[1:] == plain[1:]


def test_mex_gateway_equals_the_binding(hip):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "mexhost"))
    import host
    from stereo_amd.trws import trws
    H, W, K = 7, 9, 6
    p = trws_problem(211, H, W, K, kind="general")
    g = host.Gateway("trws_minmarginals_mex")
    out = g.call(6, np.int32(1), p["unary"].T, p["conn"].T.astype(np.uint32), p["q"].T, p["qprim"].T,
                 p["alphas"].reshape(-1, 1), 2.0, {"maxiter": 4.0, "max_relgap": -1.0})
    ref = trws(1, p["unary"].T, p["conn"].T + 1, p["q"].T, p["qprim"].T, p["alphas"], 2.0, dict(maxiter=4, max_relgap=-1),
               min_marginals=True)
    assert np.array_equal(out[0].ravel(), ref[0]) and out[1][0, 0] == ref[1] and out[2][0, 0] == ref[2] and out[3][0, 0] == ref[3]
    assert out[4].shape == (K, H * W) and np.array_equal(out[4], ref[4])
    assert out[5].shape == (H * W, 1) and np.array_equal(out[5].ravel(), ref[5])
    with pytest.raises(host.MexError, match="nlhs == 4"):
        host.Gateway("trws_mex").call(6, np.int32(1), p["unary"].T, p["conn"].T.astype(np.uint32), p["q"].T, p["qprim"].T,
                                      p["alphas"].reshape(-1, 1), 2.0, {"maxiter": 4.0})


def _crop():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teddy_crop.npz"))
    return g["im0"].astype(np.float64), g["im1"].astype(np.float64)


@pytest.mark.parametrize("kernel", [1, 2])
def test_dispmap_confidence(kernel, hip):
    """dispmap_super.simultaneous_fusion(..., confidence=True): the device-resident path (fusion context) and the
    stateless path (trws gateway) give the same min-marginals and confidence, equal to stereo_trws_min_marginals on the
    move assembled by hand; confidence is H x W like current_dispmap."""
    from oracle import terms as ot
    from stereo_amd import terms as T
    im0, im1 = _crop()
    H, W = im0.shape[:2]
    N = H * W
    tol = 8.0 if kernel == 1 else 30.0
    props = [ot.fronto_parallel(d, N) for d in (2.0, 7.0, 12.0, 18.0)] + [
        np.stack([np.full(N, 0.05), np.full(N, -0.02), np.ones(N), np.full(N, -8.0)])]
    out = []
    for stateless in (False, True):
        dm = hip.dispmap_ncc([im0, im1], np.arange(0, 24.0), kernel, 40.0, tol)
        dm.maxiter, dm.max_relgap = 6, 0.0
        if stateless:
            dm._context = lambda: None
        a0 = dm.assignment.copy(order="F")
        res = dm.simultaneous_fusion(props, confidence=True)
        assert dm.confidence.shape == (H, W) == dm.current_dispmap().shape
        assert dm.min_marginals.shape == (len(props) + 1, N)
        out.append((res, dm.min_marginals.copy(), dm.confidence.copy(), np.array(dm.assignment)))
    (r0, mm0, c0, a_dev), (r1, mm1, c1, a_sl) = out
    assert r0 == r1 and np.array_equal(a_dev, a_sl)
    assert np.array_equal(mm0, mm1) and np.array_equal(c0, c1)
    allp = props + [a0]
    unary = np.stack([dm.unary_cost(p) for p in allp], axis=0)
    q, qp = T.trws_positions(dm.neighborhood, dm.points, allp)
    L, e, lb, it, mm, conf = hip.trws(np.int32(kernel), unary, dm.neighborhood + 1, q, qp, dm.smooth_weights, tol,
                                      {"maxiter": 6, "max_relgap": 0.0}, min_marginals=True)
    assert (e, lb, it) == r0
    assert np.array_equal(mm, mm0) and np.array_equal(conf.reshape(W, H).T, c0)
    # where the solver is sure, the label it took is the argmin of the beliefs
    assert (c0 >= 0).all()
