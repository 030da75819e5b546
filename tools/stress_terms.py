"""Development tool: randomised parity stress of the term builders and the cost volume (rows a2-a13: plane -> disparity,
pairwise terms, TRW-S positions, NCC volume / sampler / winner-takes-all, globalstereo unary) against the NumPy
restatement oracle/terms.py on random image sizes, disparity lists and plane fields.  Tolerances as in
tests/test_terms_gpu.py: bit exact where only + - * / are used, 1e-12 absolute for the NCC volume (values in [-1, 1]; its label-fastest layout bit for bit against the MATLAB layout),
1e-12 relative for the globalstereo unary (exp / log).    python tools/stress_terms.py [seconds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import stereo_amd
from stereo_amd import terms as st
from oracle import terms as ot

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)


def images(H, W):
    base = rng.uniform(0, 255, size=(H, W + 12, 3))
    for _ in range(int(rng.integers(0, 3))):
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1)) / 3
    flat = rng.integers(0, 4) == 0
    if flat:
        base[:, : (W + 12) // 2] = base[0, 0]      # a flat half: zero variance under the window (sqrt of <= 0, 0 / 0)
    s = int(rng.integers(0, 6))
    return np.round(base[:, 6:6 + W]), np.round(base[:, 6 + s:6 + s + W]), flat


def planes(N):
    P = np.zeros((4, N))
    P[0] = rng.normal() * 0.05 + rng.normal(size=N) * 0.01
    P[1] = rng.normal() * 0.05
    P[2] = rng.choice([1.0, 2.0, -1.0], size=N)
    P[3] = -rng.uniform(0, 8.0, N)
    return P


t0, n, bad, first = time.time(), [0, 0, 0], [0, 0, 0], None
def fail(which, what):
    global first
    bad[which] += 1
    if first is None:
        first = what
while time.time() - t0 < budget:
    which = int(rng.integers(0, 3))
    if which == 0:      # pairwise terms + positions
        H, W = int(rng.integers(2, 40)), int(rng.integers(2, 40)); N = H * W
        kernel = int(rng.integers(1, 3))
        conn = st.construct_neighborhood(H, W); i1, i2 = ot.construct_neighborhood(H, W); pts = st.get_points(H, W)
        ok = np.array_equal(conn[0], i1) and np.array_equal(conn[1], i2) and np.array_equal(pts, ot.get_points(H, W))
        cur, prop = planes(N), planes(N)
        w = rng.uniform(0.5, 3, conn.shape[1]); tol = float(rng.uniform(0.01, 9))
        d_min, d_step = [(0.0, 0.0), (0.0, 236.0), (4.0, 100.0)][int(rng.integers(0, 3))]
        fn = ot.disparity_from_assignment if d_step == 0 else (lambda a, p: ot.globalstereo_rescale(ot.disparity_from_assignment(a, p), d_min, d_step))
        want = ot.all_pairwise_costs(kernel, w, tol, cur, prop, i1, i2, pts, disp_fn=fn)
        got = st.pairwise_terms(kernel, conn, pts, cur, prop, w, tol, d_min, d_step)
        ok = ok and all(np.array_equal(a, b) for a, b in zip(want, got))
        props = [planes(N) for _ in range(int(rng.integers(1, 7)))]
        q, qp = st.trws_positions(conn, pts, props, d_min, d_step)
        wq, wqp = ot.trws_positions(props, i1, i2, pts, disp_fn=fn)
        ok = ok and np.array_equal(q.T, wq) and np.array_equal(qp.T, wqp)
        if not ok: fail(0, ("pairwise", H, W, kernel, d_min, d_step))
    elif which == 1:    # NCC volume, sampler, winner-takes-all
        H, W = int(rng.integers(1, 60)), int(rng.integers(2, 80))
        D = int(rng.integers(1, 101))
        if rng.integers(0, 2):      # integers from 0 (the staged kernels; more than one 64-label chunk from D = 65): every d < W
            W = max(W, D + 1)
            disps = np.arange(0, D, dtype=np.float64)
        else:                       # distinct quarter steps in [0, min(W, 30)] (the per-tap kernel unless all fall on integers)
            grid = np.arange(0, 4 * min(W, 30) + 1)
            disps = np.sort(rng.choice(grid, size=min(D, len(grid)), replace=False)) / 4
        if len(np.unique(disps)) != len(disps):
            continue
        im0, im1, flat = images(H, W)
        want = ot.compute_ncc(im0, im1, disps)
        got = st.ncc_volume(im0, im1, disps)
        lf = st.ncc_volume(im0, im1, disps, layout=1)      # label fastest: other kernels on integer lists, the same bits
        # (windows that straddle a flat region's edge have a variance of a few units against sums of 5e6: the quotient
        #  magnifies the last-bit differences of the box sums -- whose order of addition differs, and MATLAB's conv2's is
        #  not known either -- by 1e5: 9e-12 seen; 1e-9 allowed there, 1e-12 on textured images as in the tests)
        ok = got.shape == want.shape and np.max(np.abs(got - want)) < (1e-9 if flat else 1e-12)
        ok = ok and np.array_equal(lf, got.reshape(H * W, len(disps), order="F").T)
        pts = ot.get_points(H, W)
        P = np.zeros((4, H * W)); P[2] = 1.0; P[0] = rng.normal() * 0.05
        P[3] = -rng.uniform(-1, disps.max() + 1, H * W)
        if rng.integers(0, 3) == 0:
            P[0] = 0; P[3] = -np.round(rng.uniform(0, disps.max(), H * W))
        ok = ok and np.array_equal(ot.ncc_unary_cost(want, disps, 40.0, P, pts), st.ncc_unary(np.asfortranarray(want), disps, 40.0, P))
        wb = ot.best_disp_from_ncc(want, disps); gb = st.ncc_best_disp(np.asfortranarray(want), disps)
        ok = ok and np.array_equal(np.nan_to_num(wb, nan=-7.0), np.nan_to_num(gb, nan=-7.0))
        if not ok:
            if first is None and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
                np.savez(os.path.join(ROOT, "gpurun_out", "stress_terms_first.npz"), im0=im0, im1=im1, disps=disps, P=P, got=got, want=want, gb=gb, wb=wb,
                         gu=st.ncc_unary(np.asfortranarray(want), disps, 40.0, P), wu=ot.ncc_unary_cost(want, disps, 40.0, P, pts))
            fail(1, ("ncc", H, W, disps.tolist()))
    else:               # globalstereo unary
        H, W = int(rng.integers(2, 50)), int(rng.integers(2, 70))
        im0, im1, _ = images(H, W)
        P2 = np.zeros((4, 3)); P2[0, 0] = P2[1, 1] = P2[2, 2] = 1.0; P2[3, 0] = -float(rng.choice([0.25, 0.5, 1.0]))
        pts = ot.get_points(H, W)
        d_min, d_step = 0.0, float(rng.choice([40.0, 236.0]))
        A = np.zeros((4, H * W)); A[2] = 1.0; A[3] = -rng.uniform(0, d_step, H * W); A[0] = rng.normal() * 0.1
        if rng.integers(0, 3) == 0:
            A[3] = -(pts[0] - 1) * 4.0; A[0] = 0     # exactly on / beyond the image border
        C = 3 if rng.integers(0, 2) else 1
        want = ot.globalstereo_unary_cost(im0[:, :, :C], im1[:, :, :C], P2, d_min, d_step, 30.0, A, pts)
        got = st.globalstereo_unary(im0 if C == 3 else im0[:, :, 0], im1 if C == 3 else im1[:, :, 0], P2, d_min, d_step, 30.0, A)
        if not np.max(np.abs(got - want) / np.maximum(1e-300, np.abs(want) + 1e-3)) < 1e-12: fail(2, ("unary", H, W, C, d_step))
    n[which] += 1
print("stress terms: %d pairwise/positions, %d NCC volume/sampler/WTA, %d globalstereo unary cases, %d + %d + %d mismatches, %.0f s%s"
      % (n[0], n[1], n[2], bad[0], bad[1], bad[2], time.time() - t0, "" if first is None else ", first: %s" % (first,)))
sys.exit(1 if sum(bad) else 0)
