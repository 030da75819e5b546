"""NumPy restatement of the two left-right consistency definitions (include/stereo_hip.h), with
plain loops: what stereo_lr_check and stereo_lr_fill must give, bit for bit.  Test infrastructure."""
import numpy as np


def lr_check(d_ref, d_other, direction, tol):
    d_ref, d_other = np.asarray(d_ref, np.float64), np.asarray(d_other, np.float64)
    H, W = d_ref.shape
    status = np.zeros((H, W), np.int32)
    residual = np.full((H, W), np.nan)
    for y in range(H):
        for x in range(W):
            d = d_ref[y, x]
            if not np.isfinite(d):
                status[y, x] = 4
                continue
            xr = np.float64(x) - np.float64(direction) * d
            xi = np.floor(xr + 0.5)
            if xi < 0 or xi > W - 1:
                status[y, x] = 3
                continue
            dr = d_other[y, int(xi)]
            if not np.isfinite(dr):
                status[y, x] = 4
                continue
            r = d - dr
            residual[y, x] = r
            status[y, x] = 0 if abs(r) <= tol else 1 if r < 0 else 2
    return status, residual


def lr_fill(d_ref, status):
    d_ref, status = np.asarray(d_ref, np.float64), np.asarray(status)
    H, W = d_ref.shape
    filled = np.full((H, W), np.nan)
    source = np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in range(W):
            if status[y, x] == 0:
                filled[y, x], source[y, x] = d_ref[y, x], x
                continue
            l = r = -1
            for c in range(x - 1, -1, -1):
                if status[y, c] == 0:
                    l = c
                    break
            for c in range(x + 1, W):
                if status[y, c] == 0:
                    r = c
                    break
            # the smaller disparity; l on equality or when only l exists (r only if STRICTLY smaller: a NaN at a
            # pixel whose status says 0 compares false, so a NaN on the left is copied, one on the right is not)
            if r >= 0 and (l < 0 or d_ref[y, r] < d_ref[y, l]):
                pick = r
            else:
                pick = l
            if pick >= 0:
                filled[y, x], source[y, x] = d_ref[y, pick], pick
    return filled, source


def same(a, b):
    """np.array_equal with NaN positions compared by mask."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def two_plane_scene(H=3):
    """Background d = 2, a box with d = 6 at left columns 20-29 = right columns 14-23, 40 columns.
    -> (left map, right map)."""
    left = np.full((H, 40), 2.0)
    left[:, 20:30] = 6.0
    right = np.full((H, 40), 2.0)
    right[:, 14:24] = 6.0
    return left, right
