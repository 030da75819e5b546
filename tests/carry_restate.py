"""Restatements for the carried messages, in plain loops.

``carry`` is the definition of stereo_band_carry (include/stereo_hip.h) written out: Python floats are IEEE doubles and
every operation below is one rounded operation in the order the definition fixes, so the kernel must give these bits.

``minimize`` is the restatement of minimize.cpp from given messages that tests/test_trws_state_gpu.py keeps as
``_restate`` (existing test files stay as they are, so the copy lives here, without the inputs that change): the
yardstick of a level that starts from carried messages in phase 1.
"""
import math

import numpy as np

import mm_restate


def carry(M_old, off_old, off_new, receiver_new, shift, edge_src=None, stretch=1.0, gain=1.0):
    """-> (M_new (E_new, K_new), bad): `bad` counts the edges whose edge_src is >= E_old or whose receiver is outside
    0 .. N_new - 1; their rows are zero."""
    M_old = np.asarray(M_old, dtype=np.float64)
    off_old = [float(v) for v in off_old]
    off_new = [float(v) for v in off_new]
    E_old, K_old, K_new, E_new, N_new = M_old.shape[0], len(off_old), len(off_new), len(receiver_new), len(shift)
    stretch, gain = float(stretch), float(gain)
    out = np.zeros((E_new, K_new))
    bad = 0
    for e in range(E_new):
        s = e if edge_src is None else int(edge_src[e])
        r = int(receiver_new[e])
        if s >= E_old or r < 0 or r >= N_new:
            bad += 1
            continue
        t = float(shift[r])
        if s < 0 or not math.isfinite(t):
            continue
        row = [float(v) for v in M_old[s]]
        v = [0.0] * K_new
        for j in range(K_new):
            p = stretch * off_new[j]
            u = t + p
            if u <= off_old[0]:
                v[j] = row[0]
            elif u >= off_old[K_old - 1]:
                v[j] = row[K_old - 1]
            else:
                i = 0
                while i + 1 < K_old and off_old[i + 1] <= u:
                    i += 1
                num = u - off_old[i]
                den = off_old[i + 1] - off_old[i]
                w = num / den
                d = row[i + 1] - row[i]
                wd = w * d
                v[j] = row[i] + wd
        m = math.inf
        for j in range(K_new):
            if v[j] < m:              # strict: the first minimum; a NaN never wins
                m = v[j]
        for j in range(K_new):
            diff = v[j] - m
            out[e, j] = gain * diff
    return out, bad


def minimize(oracle, p, M0, phase, iters, tol, kernel=1):
    """`iters` iterations of Minimize_TRW_S (minimize.cpp:31-113) from the messages M0 (E, K), which stand as after a
    backward sweep (phase 0) or with the first iteration's forward sweep already run (phase 1).  p: unary (N, K), conn
    (E, 2), q / qprim (E, K), alphas (E,).  Returns labels (0-based), energy, bound, messages."""
    impl = mm_restate.default_impl(oracle)
    col_impl = "ref" if impl == "ref" else "brute"
    q = np.ascontiguousarray(p["q"], dtype=np.float64)
    qp = np.ascontiguousarray(p["qprim"], dtype=np.float64)
    alphas = np.asarray(p["alphas"], dtype=np.float64)
    unary = np.ascontiguousarray(p["unary"], dtype=np.float64)
    N, K = unary.shape
    g = mm_restate._structure(oracle, N, p["conn"], 0)
    order, fwd, bwd, tail, dirn = g["order"], g["fwd"], g["bwd"], g["tail"], g["dir"]
    gamma = [1.0 / max(len(fwd[i]), len(bwd[i])) if (fwd[i] or bwd[i]) else np.inf for i in range(N)]
    M = np.array(M0, dtype=np.float64)
    x = np.zeros(N, np.int64)
    lam = tol

    def upd(e, Di, i, d):
        m, v = oracle.update_message(kernel, Di, gamma[i], M[e], q[e], qp[e], alphas[e], lam, d, dirn[e], impl=impl)
        M[e] = m
        return v

    LB = En = 0.0
    for t in range(1, iters + 1):
        if not (t == 1 and phase == 1):
            for i in order:
                Di = unary[i].copy()
                for e in fwd[i]:
                    Di += M[e]
                for e in bwd[i]:
                    Di += M[e]
                for e in fwd[i]:
                    upd(e, Di, i, 0)
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
                LB += upd(e, Di, i, 1)
        En = 0.0
        for i in order:
            Db = unary[i].copy()
            for e in bwd[i]:
                Db = oracle.add_column(kernel, q[e], qp[e], alphas[e], lam, x[tail[e]], Db, 0, dirn[e], impl=col_impl)
            Di = Db.copy()
            for e in fwd[i]:
                Di += M[e]
            k = int(np.argmin(Di))
            x[i] = k
            En += Db[k]
    return x, En, LB, M
