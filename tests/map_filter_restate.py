"""The map filter restated once in NumPy (the definition: include/stereo_hip.h): plain loops over the
taps in tap order, vectorised over the pixels.  Imports nothing from ``stereo_amd/`` or ``oracle/``; the ramp and the
contrast are tests/contrast_restate.py's, as the definition says.

Tap order: dx = -r .. r outer, dy = -r .. r inner.  A tap is valid inside the image where d is finite.  Every sum starts
at 0.0 and adds one term per tap in tap order (the term is 0.0 where the tap does not count: an exact addition).
"""
import numpy as np

import contrast_restate as CR

MAX_RADIUS = 4


def taps(radius):
    return [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]


def _shift(a, dy, dx, outside):
    """b(y, x) = a(y + dy, x + dx), `outside` where that is not in the array."""
    H, W = a.shape[:2]
    b = np.full(a.shape, outside, dtype=a.dtype)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
    return b


def tap_weights(shape, radius, image=None, params=None, pixel_weight=None):
    """Per tap in tap order the H x W array of w_q = rho(g(p, q)) * pixel_weight(q) (anything at a tap outside the image:
    it is not valid)."""
    H, W = shape
    im = None
    if image is not None:
        im = np.asarray(image, dtype=np.float64)
        im = im[:, :, None] if im.ndim == 2 else im
    out = []
    for dy, dx in taps(radius):
        w = None
        if im is not None:
            g = np.abs(im - _shift(im, dy, dx, 0.0)).max(axis=2)
            w = CR.ramp(g, *params)
        if pixel_weight is not None:
            pw = _shift(np.asarray(pixel_weight, dtype=np.float64), dy, dx, 0.0)
            w = pw if w is None else w * pw                      # one product, rounded once
        out.append(np.ones((H, W)) if w is None else w)
    return out


def weighted_median(d, radius, image=None, params=None, pixel_weight=None, targets=None):
    """-> (out H x W float64, source H x W int32 pixel ids col * H + row, kept).  params = (w_high, w_low, g0, g1)."""
    d = np.array(d, dtype=np.float64)
    H, W = d.shape
    assert 1 <= radius <= MAX_RADIUS and (image is None) == (params is None)
    tp = taps(radius)
    ws = tap_weights((H, W), radius, image, params, pixel_weight)
    clean = np.where(np.isfinite(d), d, np.nan)
    ds = [_shift(clean, dy, dx, np.nan) for dy, dx in tp]          # NaN: not valid; no comparison selects it
    raw = [_shift(d, dy, dx, np.nan) for dy, dx in tp]             # the taps' own bits
    ids = np.arange(H)[:, None] + H * np.arange(W)[None, :]
    target = np.ones((H, W), bool) if targets is None else np.asarray(targets) != 0

    total = np.zeros((H, W))
    for di, wi in zip(ds, ws):
        total = total + np.where(~np.isnan(di), wi, 0.0)
    best = np.full((H, W), np.inf)
    with np.errstate(invalid="ignore"):
        for dj in ds:
            w_le = np.zeros((H, W))
            for di, wi in zip(ds, ws):
                w_le = w_le + np.where(di <= dj, wi, 0.0)
            qualifies = ~np.isnan(dj) & (2.0 * w_le >= total)
            best = np.where(qualifies & (dj < best), dj, best)
        filtered = target & (total > 0)
        out, source = d.copy(), ids.copy()
        found = np.zeros((H, W), bool)
        for (dy, dx), di, ri, wi in zip(tp, ds, raw, ws):
            hit = filtered & ~found & (wi > 0) & (di == best)
            out[hit] = ri[hit]
            source[hit] = (ids + dy + H * dx)[hit]
            found |= hit
    assert (found == filtered).all()
    return out, source.astype(np.int32), int((target & ~(total > 0)).sum())
