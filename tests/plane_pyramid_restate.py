"""NumPy restatement of the plane expansion's definition (include/stereo_hip.h), with plain loops: what
stereo_pyramid_expand_planes must give, bit for bit.  The candidates are pyramid_restate's.  Test infrastructure."""
import numpy as np

import pyramid_restate as R
from plane_fit_restate import valid

F = np.float64


def fronto(m):
    """An H x W map as 4 x N planes [0, 0, 1, -v], pixels column major."""
    m = np.asarray(m, F)
    out = np.zeros((4, m.size))
    out[2] = 1.0
    out[3] = -m.reshape(-1, order="F")
    return out


def to_fine(p):
    """The coarse plane [a b c d] in the fine scale's coordinates and disparity units."""
    with np.errstate(all="ignore"):
        return np.array([p[0], p[1], p[2], (F(2.0) * F(p[3]) + F(0.5) * F(p[0])) + F(0.5) * F(p[1])])


def expand_planes(p_coarse, shape, mode, im_fine=None, im_coarse=None):
    """-> (out 4 x N float64, source H x W int32).  mode 0: nearest; 1: guided by the view's own image."""
    p_coarse = np.asarray(p_coarse, F)
    H, W = shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    assert p_coarse.shape == (4, Hc * Wc)
    out = np.full((4, H * W), np.nan)
    source = np.full((H, W), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(H):
            for x in range(W):
                cand = [p_coarse[:, cy + Hc * cx] for cy, cx in R.candidates(y, x, Hc, Wc)]
                where = R.candidates(y, x, Hc, Wc)
                if mode == 0:
                    source[y, x] = 0
                    if valid(cand[0]):
                        out[:, y + H * x] = to_fine(cand[0])
                    continue
                best, best_dist = -1, None
                for k, (cy, cx) in enumerate(where):
                    if not valid(cand[k]):
                        continue
                    dist = F(0.0)
                    for c in range(im_fine.shape[2]):
                        e = F(im_fine[y, x, c]) - F(im_coarse[cy, cx, c])
                        dist = dist + e * e
                    if best < 0 or dist < best_dist:
                        best, best_dist = k, dist
                if best >= 0:
                    out[:, y + H * x], source[y, x] = to_fine(cand[best]), best
    return out, source


def same_but_zero_sign(a, b):
    """pyramid_restate.same_bits, except that +0.0 and -0.0 count as the same: the plane expansion's two additions
    leave d = +0.0 where negating an expanded disparity 0 gives -0.0 (include/stereo_hip.h)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a) & ~((a == 0.0) & (b == 0.0))
    return a[ok].tobytes() == b[ok].tobytes()
