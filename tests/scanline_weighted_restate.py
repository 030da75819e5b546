"""Weighted scanline aggregation restated once in NumPy (the definition: include/stereo_hip.h).
Imports nothing from ``stereo_amd/`` or ``oracle/``; the unweighted table comes from scanline_restate.

It is scanline_restate's recurrence with one change: the step INTO pixel p along direction r weighs wstep[r, p],
    L_r(p, k) = U(p, k) + min_l (L_r(p - r, l) + wstep[r, p] * min(v(|pos_k - pos_l|), tol))
the product last, the minimum not subtracted.  wstep is R x N; an entry at a pixel without a predecessor is not read.
"""
import numpy as np

from scanline_restate import DIRECTIONS_8, table


def direction_costs(unary, shape, positions, kernel, tol, direction, wstep_r):
    """L_r, D x N, with the N step weights `wstep_r` of this direction."""
    H, W = shape
    dy, dx = direction
    if not (dy in (-1, 0, 1) and dx in (-1, 0, 1) and (dy, dx) != (0, 0)):
        raise ValueError("a direction is (dy, dx) with dy, dx in {-1, 0, 1}, not both 0")
    U = np.asarray(unary, dtype=np.float64)
    D = U.shape[0]
    assert U.shape == (D, H * W)
    w = np.asarray(wstep_r, dtype=np.float64).reshape(-1)
    assert w.shape == (H * W,)
    B = table(positions, kernel, tol, 1.0)                  # min(v(|pos_k - pos_l|), tol): 1.0 * x is x
    L = np.zeros((D, H * W))
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)      # predecessors first
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for x in xs:
        for y in ys:
            p = x * H + y
            yp, xp = y - dy, x - dx
            if 0 <= yp < H and 0 <= xp < W:
                prev = L[:, xp * H + yp]
                L[:, p] = U[:, p] + (prev[None, :] + w[p] * B).min(axis=1)
            else:
                L[:, p] = U[:, p]
    return L


def aggregate(unary, shape, positions, kernel, tol, step_weights, directions=DIRECTIONS_8):
    """-> (S D x N, labels N int32 one based, map H x W, confidence H x W)"""
    H, W = shape
    directions = list(directions)
    if not 1 <= len(directions) <= 8:
        raise ValueError("1 .. 8 directions")
    wstep = np.asarray(step_weights, dtype=np.float64).reshape(len(directions), H * W)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1)
    S = None
    for direction, w in zip(directions, wstep):
        L = direction_costs(unary, shape, pos, kernel, tol, direction, w)
        S = L if S is None else S + L
    D = S.shape[0]
    labels = (np.argmin(S, axis=0) + 1).astype(np.int32)               # argmin: the first minimum
    rel = S - S.min(axis=0)[None, :]
    conf = np.sort(rel, axis=0)[1] if D > 1 else np.full(H * W, np.inf)
    return S, labels, pos[labels - 1].reshape(W, H).T, conf.reshape(W, H).T
