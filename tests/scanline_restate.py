"""Scanline aggregation restated once in NumPy (the definition: include/stereo_hip.h).  Imports nothing
from ``stereo_amd/`` or ``oracle/``.

unary: D x N float64, label fastest, N = H * W, pixel id = col * H + row.  positions: D doubles.  kernel 1: v(d) = d,
2: v(d) = d * d.  V_r[k, l] = w_r * min(v(|pos_k - pos_l|), tol), the product last.  For direction r = (dy, dx) the
predecessor of (y, x) is (y - dy, x - dx); L_r(p, k) = U(p, k) where it is outside the image and
U(p, k) + min_l (L_r(p - r, l) + V_r[k, l]) otherwise -- the minimum is not subtracted.  Every line below rounds once per
operation, in the order the definition writes them.
"""
import numpy as np

DIRECTIONS_4 = ((0, 1), (0, -1), (1, 0), (-1, 0))
DIRECTIONS_8 = DIRECTIONS_4 + ((1, 1), (-1, -1), (1, -1), (-1, 1))


def table(positions, kernel, tol, w):
    """V[k, l] = w * min(v(|pos_k - pos_l|), tol)"""
    if kernel not in (1, 2):
        raise ValueError("kernel must be 1 or 2")
    pos = np.asarray(positions, dtype=np.float64).reshape(-1)
    d = np.abs(pos[:, None] - pos[None, :])
    with np.errstate(over="ignore"):
        v = d if kernel == 1 else d * d
    return np.float64(w) * np.minimum(v, np.float64(tol))


def chain_pixels(shape, direction, y, x):
    """The pixels (row, col) of the chain of `direction` through (y, x), from its first pixel up to and including (y, x)."""
    H, W = shape
    dy, dx = direction
    out = [(y, x)]
    while 0 <= out[-1][0] - dy < H and 0 <= out[-1][1] - dx < W:
        out.append((out[-1][0] - dy, out[-1][1] - dx))
    return out[::-1]


def direction_costs(unary, shape, positions, kernel, tol, direction, w):
    """L_r, D x N."""
    H, W = shape
    dy, dx = direction
    if not (dy in (-1, 0, 1) and dx in (-1, 0, 1) and (dy, dx) != (0, 0)):
        raise ValueError("a direction is (dy, dx) with dy, dx in {-1, 0, 1}, not both 0")
    U = np.asarray(unary, dtype=np.float64)
    D = U.shape[0]
    assert U.shape == (D, H * W)
    V = table(positions, kernel, tol, w)
    L = np.zeros((D, H * W))
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)      # predecessors first
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for x in xs:
        for y in ys:
            p = x * H + y
            yp, xp = y - dy, x - dx
            if 0 <= yp < H and 0 <= xp < W:
                prev = L[:, xp * H + yp]
                L[:, p] = U[:, p] + (prev[None, :] + V).min(axis=1)
            else:
                L[:, p] = U[:, p]
    return L


def aggregate(unary, shape, positions, kernel, tol, directions=DIRECTIONS_8, weights=None):
    """-> (S D x N, labels N int32 one based, map H x W, confidence H x W)"""
    H, W = shape
    directions = list(directions)
    if not 1 <= len(directions) <= 8:
        raise ValueError("1 .. 8 directions")
    weights = [1.0] * len(directions) if weights is None else list(weights)
    assert len(weights) == len(directions)
    pos = np.asarray(positions, dtype=np.float64).reshape(-1)
    S = None
    for direction, w in zip(directions, weights):
        L = direction_costs(unary, shape, pos, kernel, tol, direction, w)
        S = L if S is None else S + L
    D = S.shape[0]
    labels = (np.argmin(S, axis=0) + 1).astype(np.int32)               # argmin: the first minimum
    rel = S - S.min(axis=0)[None, :]
    conf = np.sort(rel, axis=0)[1] if D > 1 else np.full(H * W, np.inf)
    return S, labels, pos[labels - 1].reshape(W, H).T, conf.reshape(W, H).T
