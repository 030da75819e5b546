"""The contrast rule restated once in NumPy (the definition: include/stereo_hip.h).  Imports nothing
from ``stereo_amd/`` or ``oracle/``.

image: H x W x C float64 (any memory order; pixel id = col * H + row).  g(a, b) = max_c |im(a, c) - im(b, c)|.
The ramp, tested in this order: g <= g0 -> w_high; g >= g1 -> w_low; otherwise
w_high + (w_low - w_high) * ((g - g0) / (g1 - g0)).  Every line below rounds once per operation; this expression order
is the definition.
"""
import numpy as np


def ramp(g, w_high, w_low, g0, g1):
    """rho(g), elementwise on an array of contrasts."""
    g = np.asarray(g, dtype=np.float64)
    w_high, w_low, g0, g1 = (np.float64(v) for v in (w_high, w_low, g0, g1))
    if not (np.isfinite([w_high, w_low, g0, g1]).all() and w_high >= 0 and w_low >= 0 and 0 <= g0 <= g1):
        raise ValueError("w_high >= 0, w_low >= 0 and 0 <= g0 <= g1, all finite")
    out = np.empty(g.shape)
    high = g <= g0
    low = ~high & (g >= g1)
    mid = ~high & ~low
    out[high] = w_high
    out[low] = w_low
    with np.errstate(all="ignore"):
        t = (g[mid] - g0) / (g1 - g0)
        out[mid] = w_high + (w_low - w_high) * t
    return out


def _pixels(image):
    """H x W x C -> (N x C, H, W), pixel id = col * H + row."""
    im = np.asarray(image, dtype=np.float64)
    if im.ndim == 2:
        im = im[:, :, None]
    H, W, C = im.shape
    return im.transpose(1, 0, 2).reshape(H * W, C), H, W


def contrast(image, a, b):
    """g(a, b) for arrays of pixel ids."""
    px, _, _ = _pixels(image)
    return np.abs(px[np.asarray(a)] - px[np.asarray(b)]).max(axis=1)


def edge_weights(image, conn, params):
    """alphas[e] = rho(g(conn[0, e], conn[1, e])); conn 2 x E, zero based; params = (w_high, w_low, g0, g1)."""
    conn = np.asarray(conn).astype(np.int64).reshape(2, -1)
    px, H, W = _pixels(image)
    if conn.size and (conn.min() < 0 or conn.max() >= H * W):
        raise ValueError("an endpoint outside 0 .. N - 1")
    return ramp(contrast(image, conn[0], conn[1]), *params)


def step_weights(image, directions, params):
    """wstep (R x N): rho(g(p, p - r)) where the predecessor (y - dy, x - dx) is inside the image, 0.0 where not."""
    px, H, W = _pixels(image)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    p = (xs * H + ys).reshape(-1)
    out = np.zeros((len(directions), H * W))
    for r, (dy, dx) in enumerate(directions):
        yp, xp = (ys - dy).reshape(-1), (xs - dx).reshape(-1)
        inside = (yp >= 0) & (yp < H) & (xp >= 0) & (xp < W)
        out[r, p[inside]] = ramp(contrast(image, p[inside], xp[inside] * H + yp[inside]), *params)
    return out
