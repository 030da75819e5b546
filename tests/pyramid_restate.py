"""NumPy restatement of the image pyramid's definitions (include/stereo_hip.h), with plain loops: what
stereo_pyramid_reduce and stereo_pyramid_expand must give, bit for bit, and the level model.  Test infrastructure."""
import math

import numpy as np


def reduce(im):
    """H x W x C -> (H + 1) // 2 x (W + 1) // 2 x C: the 2 x 2 box, the last row / column replicated at an odd size."""
    im = np.asarray(im, np.float64)
    H, W, C = im.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((Hc, Wc, C))
    for c in range(C):
        for xc in range(Wc):
            for yc in range(Hc):
                y0, y1 = 2 * yc, min(2 * yc + 1, H - 1)
                x0, x1 = 2 * xc, min(2 * xc + 1, W - 1)
                a00, a10, a01, a11 = im[y0, x0, c], im[y1, x0, c], im[y0, x1, c], im[y1, x1, c]
                out[yc, xc, c] = np.float64(0.25) * (((a00 + a10) + a01) + a11)
    return out


def candidates(y, x, Hc, Wc):
    yc, xc = y >> 1, x >> 1
    ny = min(max(yc + 1 if y & 1 else yc - 1, 0), Hc - 1)
    nx = min(max(xc + 1 if x & 1 else xc - 1, 0), Wc - 1)
    return [(yc, xc), (ny, xc), (yc, nx), (ny, nx)]


def expand(d_coarse, shape, mode, im_fine=None, im_coarse=None):
    """-> (out H x W float64, source H x W int32).  mode 0: nearest; 1: guided by the view's own image."""
    d_coarse = np.asarray(d_coarse, np.float64)
    H, W = shape
    Hc, Wc = d_coarse.shape
    assert (Hc, Wc) == ((H + 1) // 2, (W + 1) // 2)
    out = np.full((H, W), np.nan)
    source = np.full((H, W), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(H):
            for x in range(W):
                cand = candidates(y, x, Hc, Wc)
                if mode == 0:
                    out[y, x], source[y, x] = np.float64(2.0) * d_coarse[cand[0]], 0
                    continue
                best, best_dist = -1, None
                for k, (cy, cx) in enumerate(cand):
                    if not np.isfinite(d_coarse[cy, cx]):
                        continue
                    dist = np.float64(0.0)
                    for c in range(im_fine.shape[2]):
                        e = np.float64(im_fine[y, x, c]) - np.float64(im_coarse[cy, cx, c])
                        dist = dist + e * e
                    if best < 0 or dist < best_dist:
                        best, best_dist = k, dist
                if best >= 0:
                    out[y, x], source[y, x] = np.float64(2.0) * d_coarse[cand[best]], best
    return out, source


def level_model(kernel, tol, level):
    """(tol_l, edge weight) at the scale s = 2^level: tol / s^k, s^(k - 1)."""
    s = float(2 ** level)
    return tol / s ** kernel, s ** (kernel - 1)


def level_disparities(disparities, level):
    disparities = np.asarray(disparities, np.float64)
    if level == 0:
        return disparities
    s = float(2 ** level)
    return np.arange(math.floor(disparities.min() / s), math.ceil(disparities.max() / s) + 1, dtype=np.float64)


def same(a, b):
    """equal values, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def same_bits(a, b):
    """the same bytes where neither is NaN (signs of zeros included), NaN in the same places"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()
