"""-m gpu tests of the large-label sweep kernel (512 < K <= 4096, one shared strictly ascending
positions vector; stereo_trws_plan_path 5) against the CPU oracle.  Bar as everywhere for TRW-S:
labels, energy, lower bound and iteration count bit exact."""
import os
import sys

import numpy as np
import pytest

from helpers import grid_conn, trws_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _positions(kind, K, rng):
    if kind == "grid":
        return np.arange(K, dtype=np.float64)
    if kind == "half":
        return np.arange(K, dtype=np.float64) * 0.5 - 7.0
    return np.cumsum(rng.uniform(0.05, 2.0, size=K))  # irregular, strictly ascending


def _oracle(oracle, kernel, unary, conn, pos, alphas, tol, maxiter, mode=1, ordering=0):
    """The oracle with the reference's own message classes where they were built (any K)."""
    E = conn.shape[0]
    q = np.tile(pos, (E, 1))
    ref = oracle.ref_types() is not None and mode == 1
    return oracle.trws(kernel, unary, conn, q, q, alphas, tol, maxiter, -1e300, mode=mode, use_ref_types=ref,
                       ordering=ordering)


def _plan(kernel, K, N, conn, unary, alphas, tol, pos, message_mode=0):
    from stereo_amd.trws import TrwsPlan
    plan = TrwsPlan(kernel, K, N, conn.T, message_mode=message_mode)
    plan.upload(unary.T, alphas, tol, positions=pos)
    return plan


def _same(got, ref):
    lab, en, lb, it = got
    lab_o, en_o, lb_o, it_o = ref
    assert it == it_o
    assert np.array_equal(lab, lab_o), "labels differ at %d nodes" % int((lab != lab_o).sum())
    assert en == en_o and lb == lb_o


LARGE = [
    # seed, H, W, K, kernel, positions, integer, tol, maxiter
    (101, 7, 9, 513, 1, "grid", False, 8.0, 3),
    (102, 6, 7, 600, 1, "irregular", False, 20.0, 3),
    (103, 5, 6, 1000, 1, "half", False, 30.0, 3),
    (104, 9, 11, 1024, 1, "grid", False, 16.0, 3),
    (105, 6, 6, 2048, 1, "grid", False, 40.0, 2),
    (106, 5, 6, 4096, 1, "irregular", False, 60.0, 2),
    (107, 6, 7, 600, 1, "grid", True, 8.0, 4),        # integer costs: exact ties -> serial construction
    (108, 5, 6, 1024, 1, "grid", False, 1e9, 2),      # no truncation: the window is every label
    (109, 6, 7, 700, 1, "grid", False, 0.0, 3),       # lambda = 0
    (110, 1, 12, 800, 1, "grid", False, 8.0, 3),      # a chain
    (111, 6, 7, 600, 2, "grid", False, 64.0, 3),      # quadratic kernel
    (112, 5, 6, 1024, 2, "irregular", False, 100.0, 3),
    (113, 6, 6, 4096, 2, "half", False, 400.0, 2),
    (114, 6, 7, 700, 2, "grid", True, 16.0, 3),       # integer costs: equal costs -> serial hull construction
    (115, 5, 6, 2048, 2, "grid", False, 1e9, 2),      # no truncation
    (116, 1, 10, 1000, 2, "grid", False, 50.0, 3),    # a chain
    (117, 5, 7, 513, 2, "grid", False, 0.0, 3),       # lambda = 0
]


@pytest.mark.parametrize("case", LARGE, ids=[str(c[0]) for c in LARGE])
def test_large_kernel_matches_oracle(case, hip, oracle):
    seed, H, W, K, kernel, pk, integer, tol, maxiter = case
    p = trws_problem(seed, H, W, K, kind="fronto", integer=integer)
    pos = _positions(pk, K, np.random.default_rng(seed + 1000))
    ref = _oracle(oracle, kernel, p["unary"], p["conn"], pos, p["alphas"], tol, maxiter)
    plan = _plan(kernel, K, H * W, p["conn"], p["unary"], p["alphas"], tol, pos)
    assert plan.path() == 5
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)
    if not integer and 0 < tol < 1e6 and (kernel == 1 or (pk == "grid" and H > 1)):
        # the certificate holds for (almost) every message of a generic instance (kernel 2: its margin
        # 1e-9 * 2 alpha max pos^2 is wide at these label counts, and on a chain the messages pile up)
        E = p["conn"].shape[0]
        assert plan.serial_messages() < 0.2 * (2 * E * maxiter + E)


@pytest.mark.parametrize("kernel,K,tol", [(1, 1000, 8.0), (2, 700, 64.0)])
def test_large_kernel_flat_costs(kernel, K, tol, hip, oracle):
    """Unaries with a spread far below alpha * lambda: most sources of a message are useful, the
    windowed min-plus runs -- same bits as the oracle."""
    H, W, maxiter = 6, 7, 3
    p = trws_problem(121, H, W, K, kind="fronto")
    unary = np.ascontiguousarray(p["unary"] * 0.02)
    pos = np.arange(K, dtype=np.float64)
    ref = _oracle(oracle, kernel, unary, p["conn"], pos, p["alphas"], tol, maxiter)
    plan = _plan(kernel, K, H * W, p["conn"], unary, p["alphas"], tol, pos)
    assert plan.path() == 5
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)


def _eight_neighbourhood(H, W):
    """4-neighbourhood plus both diagonals: up to 8 edges per node, not a grid the pipelined kernels take."""
    conn = [tuple(e) for e in grid_conn(H, W)]
    for c in range(W - 1):
        for r in range(H):
            if r + 1 < H:
                conn.append((c * H + r, (c + 1) * H + r + 1))
            if r > 0:
                conn.append((c * H + r, (c + 1) * H + r - 1))
    return np.array(conn, dtype=np.int64)


@pytest.mark.parametrize("kernel", [1, 2])
def test_large_kernel_non_grid_graph(kernel, hip, oracle):
    H, W, K, tol, maxiter = 6, 7, 640, (8.0 if kernel == 1 else 64.0), 3
    rng = np.random.default_rng(131)
    conn = _eight_neighbourhood(H, W)
    E = conn.shape[0]
    unary = rng.uniform(0, 40, size=(H * W, K))
    alphas = rng.uniform(0.5, 2.0, size=E)
    pos = np.arange(K, dtype=np.float64)
    ref = _oracle(oracle, kernel, unary, conn, pos, alphas, tol, maxiter)
    plan = _plan(kernel, K, H * W, conn, unary, alphas, tol, pos)
    assert plan.path() == 5
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)


@pytest.mark.parametrize("kernel", [1, 2])
def test_large_kernel_without_certificate(kernel, hip, oracle, monkeypatch):
    """STEREO_HIP_TRWS_CERTIFICATE=0: every message by the serial construction, the same bits."""
    monkeypatch.setenv("STEREO_HIP_TRWS_CERTIFICATE", "0")
    H, W, K, tol, maxiter = 5, 6, 900, (12.0 if kernel == 1 else 80.0), 3
    p = trws_problem(141, H, W, K, kind="fronto")
    pos = np.arange(K, dtype=np.float64) * 0.25
    ref = _oracle(oracle, kernel, p["unary"], p["conn"], pos, p["alphas"], tol, maxiter)
    plan = _plan(kernel, K, H * W, p["conn"], p["unary"], p["alphas"], tol, pos)
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)
    E = p["conn"].shape[0]
    assert plan.serial_messages() > 2 * E * maxiter - E   # (messages of edges with alpha = 0 need none)


def test_large_kernel_index_order(hip, oracle):
    from stereo_amd.trws import ORDER_INDEX
    H, W, K, tol, maxiter = 6, 8, 777, 10.0, 3
    p = trws_problem(151, H, W, K, kind="fronto")
    pos = np.arange(K, dtype=np.float64)
    ref = _oracle(oracle, 1, p["unary"], p["conn"], pos, p["alphas"], tol, maxiter, ordering=1)
    plan = _plan(1, K, H * W, p["conn"], p["unary"], p["alphas"], tol, pos, message_mode=ORDER_INDEX)
    assert plan.path() == 5
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)


@pytest.mark.parametrize("kernel,K,tol,scale", [(1, 600, 6.0, 1.0), (2, 1024, 50.0, 1.0), (1, 800, 8.0, 0.02)])
def test_large_kernel_minplus_matches_bruteforce_oracle(kernel, K, tol, scale, hip, oracle):
    from stereo_amd.trws import MESSAGES_MINPLUS
    H, W, maxiter = 5, 7, 3
    p = trws_problem(161, H, W, K, kind="fronto")
    unary = np.ascontiguousarray(p["unary"] * scale)
    pos = np.arange(K, dtype=np.float64) * 0.5
    ref = _oracle(oracle, kernel, unary, p["conn"], pos, p["alphas"], tol, maxiter, mode=0)
    plan = _plan(kernel, K, H * W, p["conn"], unary, p["alphas"], tol, pos, message_mode=MESSAGES_MINPLUS)
    assert plan.path() == 5
    plan.iterate(maxiter, max_relgap=-1e300)
    _same(plan.result(), ref)


def test_large_gateway(hip, oracle):
    """stereo_amd.trws() with K x E columns that are one ascending vector: the plan API's and the
    oracle's bits, twice (the second call on the cached plan); per-edge positions and K = 4097 fail."""
    import stereo_amd
    H, W, K, tol, maxiter = 6, 7, 1000, 12.0, 3
    p = trws_problem(171, H, W, K, kind="fronto")
    pos = np.arange(K, dtype=np.float64) * 0.5
    E = p["conn"].shape[0]
    Q = np.ascontiguousarray(np.tile(pos, (E, 1)).T)
    ref = _oracle(oracle, 1, p["unary"], p["conn"], pos, p["alphas"], tol, maxiter)
    plan = _plan(1, K, H * W, p["conn"], p["unary"], p["alphas"], tol, pos)
    plan.iterate(maxiter, max_relgap=-1e300)
    via_plan = plan.result()
    _same(via_plan, ref)
    for _ in range(2):
        got = stereo_amd.trws(1, p["unary"].T, p["conn"].T + 1, Q, Q, p["alphas"], tol, dict(maxiter=maxiter, max_relgap=-1e300))
        assert np.array_equal(np.asarray(got[0]).ravel(), np.asarray(ref[0]).ravel())
        assert got[1] == ref[1] and got[2] == ref[2] and got[3] == ref[3]
    Qe = Q + np.random.default_rng(5).uniform(0, 0.1, size=Q.shape)
    with pytest.raises(hip.StereoHipError, match="K must be in"):
        stereo_amd.trws(1, p["unary"].T, p["conn"].T + 1, Qe, Qe, p["alphas"], tol, dict(maxiter=2))
    K2 = 4097
    U2 = np.zeros((K2, H * W))
    Q2 = np.tile(np.arange(K2, dtype=np.float64)[:, None], (1, E))
    with pytest.raises(hip.StereoHipError, match="K must be in"):
        stereo_amd.trws(1, U2, p["conn"].T + 1, Q2, Q2, p["alphas"], tol, dict(maxiter=2))


def test_large_plan_rejects_other_positions(hip):
    """Above 512 labels a plan takes one finite, strictly ascending positions vector, nothing else."""
    from stereo_amd.trws import TrwsPlan
    H, W, K = 4, 5, 600
    p = trws_problem(181, H, W, K, kind="fronto")
    plan = TrwsPlan(1, K, H * W, p["conn"].T)
    bad = [np.arange(K, dtype=np.float64)[::-1].copy(), np.floor(np.arange(K) / 2.0),
           np.where(np.arange(K) == 7, np.nan, np.arange(K, dtype=np.float64))]
    for pos in bad:
        with pytest.raises(hip.StereoHipError, match="K must be in"):
            plan.upload(p["unary"].T, p["alphas"], 4.0, positions=pos)
    with pytest.raises(hip.StereoHipError, match="K must be in"):
        plan.upload(p["unary"].T, p["alphas"], 4.0, q=p["q"].T, qprim=p["qprim"].T)
    plan.upload(p["unary"].T, p["alphas"], 4.0, positions=np.arange(K, dtype=np.float64))
    assert plan.path() == 5


def test_large_mex_gateway(hip):
    sys.path.insert(0, os.path.join(ROOT, "tests", "mexhost"))
    import host
    H, W, K, tol = 5, 6, 1000, 10.0
    p = trws_problem(191, H, W, K, kind="fronto")
    pos = np.arange(K, dtype=np.float64)
    g = host.Gateway("trws_mex")
    lab, en, lb, it = g.call(4, np.int32(1), p["unary"].T, p["conn"].T.astype(np.uint32), p["q"].T, p["qprim"].T,
                             p["alphas"].reshape(-1, 1), tol, {"maxiter": 3.0, "max_relgap": -1.0})
    plan = _plan(1, K, H * W, p["conn"], p["unary"], p["alphas"], tol, pos)
    plan.iterate(3, max_relgap=-1.0)
    lab2, en2, lb2, it2 = plan.result()
    assert np.array_equal(lab.ravel(), np.asarray(lab2).ravel()) and en[0, 0] == en2 and lb[0, 0] == lb2 and it[0, 0] == it2


def test_large_teddy_crop_sixteenth_pixel(hip, oracle):
    """The NCC volume of the Teddy crop (64 x 96) at disparities 0 : 1/16 : 63.9375 (K = 1024); the solve
    runs on an 8 x 12 window of it (the oracle's reference message classes re-sort every column: a
    minute per 100 edges at this K)."""
    from stereo_amd import terms as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "teddy_crop.npz"))
    im0, im1 = g["im0"].astype(np.float64), g["im1"].astype(np.float64)
    K = 1024
    disp = np.arange(K, dtype=np.float64) / 16.0
    ncc = T.ncc_volume(im0, im1, disp, 2, layout=1)      # (K, 64 * 96), node = col * 64 + row
    Hc, Wc = im0.shape[:2]
    H, W, r0, c0 = 8, 12, 28, 40
    nodes = ((np.arange(W)[:, None] + c0) * Hc + (np.arange(H)[None, :] + r0)).ravel()
    unary = np.ascontiguousarray(40.0 * (1.0 - ncc[:, nodes].T))
    conn = grid_conn(H, W)
    alphas = np.ones(conn.shape[0])
    ref = _oracle(oracle, 1, unary, conn, disp, alphas, 8.0, 3)
    plan = _plan(1, K, H * W, conn, unary, alphas, 8.0, disp)
    assert plan.path() == 5
    plan.iterate(3, max_relgap=-1e300)
    _same(plan.result(), ref)


def test_large_full_size_volume(hip):
    """375 x 450 x 1024 (messages: 2.8 GB): a few iterations run, labels in range, bound <= energy,
    and a reset reproduces the bits."""
    import torch
    sys.path.insert(0, ROOT)
    from bench import synthetic_volume_device
    from stereo_amd.trws import TrwsPlan
    H, W, K = 375, 450, 1024
    dev = torch.device("cuda", 0)
    conn = grid_conn(H, W)
    E = conn.shape[0]
    d_unary = synthetic_volume_device(H, W, K, 3, dev)
    d_alpha = torch.ones(E, dtype=torch.float64, device=dev)
    d_pos = torch.arange(K, dtype=torch.float64, device=dev) * 0.25
    plan = TrwsPlan(1, K, H * W, conn.T)
    plan.bind_device(d_unary.data_ptr(), d_alpha.data_ptr(), 8.0, d_positions=d_pos.data_ptr(), keepalive=(d_unary, d_alpha, d_pos))
    assert plan.path() == 5
    plan.iterate(2, max_relgap=-1e300)
    lab, en, lb, it = plan.result()
    assert it == 2 and lab.min() >= 1 and lab.max() <= K and lb <= en
    plan.reset()
    plan.iterate(2, max_relgap=-1e300)
    lab2, en2, lb2, it2 = plan.result()
    assert np.array_equal(lab, lab2) and en == en2 and lb == lb2 and it == it2
    plan.close()
