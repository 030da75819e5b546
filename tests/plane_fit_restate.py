"""NumPy restatement of the local plane fit's definition (include/stereo_hip.h), with plain loops: what
stereo_planes_fit_local must give, bit for bit.  Test infrastructure."""
import numpy as np

F = np.float64


def valid(p):
    """A plane has a disparity: four finite components and c != 0."""
    return bool(np.isfinite(p).all() and p[2] != 0.0)


def disparity(p, X, Y):
    """A plane's disparity at the 1-based point (X, Y), in the library's order."""
    with np.errstate(all="ignore"):
        return -((F(p[0]) * F(X) + F(p[1]) * F(Y)) + F(p[3])) / F(p[2])


def own_disparities(planes, H, W):
    """z (H x W): every plane's disparity at its own pixel, NaN for a plane that is not valid."""
    z = np.full((H, W), np.nan)
    for x in range(W):
        for y in range(H):
            p = planes[:, y + H * x]
            if valid(p):
                z[y, x] = disparity(p, x + 1.0, y + 1.0)
    return z


def fit_local(planes, shape, radius, tau):
    """-> (out 4 x N, bad): bad counts the pixels whose own plane is not valid; they keep it."""
    planes = np.asarray(planes, F)
    H, W = shape
    assert planes.shape == (4, H * W) and 1 <= radius <= 8 and tau >= 0
    tau = F(tau)
    z = own_disparities(planes, H, W)
    out = np.zeros((4, H * W))
    bad = 0
    with np.errstate(all="ignore"):
        for x in range(W):
            for y in range(H):
                i = y + H * x
                if not valid(planes[:, i]):
                    out[:, i] = planes[:, i]
                    bad += 1
                    continue
                z0 = z[y, x]
                n = Sx = Sy = Sxx = Sxy = Syy = Sz = Sxz = Syz = F(0.0)
                for dx in range(-radius, radius + 1):
                    for dy in range(-radius, radius + 1):
                        xx, yy = x + dx, y + dy
                        if not (0 <= xx < W and 0 <= yy < H):
                            continue
                        e = z[yy, xx] - z0
                        if not abs(e) <= tau:
                            continue
                        fx, fy = F(dx), F(dy)
                        n = n + F(1.0)
                        Sx = Sx + fx
                        Sy = Sy + fy
                        Sxx = Sxx + fx * fx
                        Sxy = Sxy + fx * fy
                        Syy = Syy + fy * fy
                        Sz = Sz + e
                        Sxz = Sxz + fx * e
                        Syz = Syz + fy * e
                c00, c01, c02 = Syy * n - Sy * Sy, Sxy * n - Sy * Sx, Sxy * Sy - Syy * Sx
                det = (Sxx * c00 - Sxy * c01) + Sx * c02
                al = be = ga = F(0.0)
                if n >= 3 and det > 0:
                    c11, c12, c22 = Sxx * n - Sx * Sx, Sxx * Sy - Sxy * Sx, Sxx * Syy - Sxy * Sxy
                    al = ((c00 * Sxz - c01 * Syz) + c02 * Sz) / det
                    be = ((c11 * Syz - c01 * Sxz) - c12 * Sz) / det
                    ga = ((c02 * Sxz - c12 * Syz) + c22 * Sz) / det
                g = ((z0 + ga) - al * F(x + 1.0)) - be * F(y + 1.0)
                out[:, i] = [-al, -be, F(1.0), -g]
    return out, bad
