"""TEST INFRASTRUCTURE ONLY -- the NCC cost volume in exact integer arithmetic, the instances of the geometry
matrix (tests/test_ncc_volume_gpu.py on the device, tests/test_ncc_exact_cpu.py on the restatement), the host
rule that picks the staged kernel and its column count, restated with its own constants (host_rule), and a caller of
the library's own rule (library_rule: stereo_ncc_volume_rule, host only) for the tests that compare the two.

The exact definition.  Images are H x W x 3 with integer values in [0, 255], d is an integer disparity, 0 <= d < W.
a is the left image, b(:, c) = im1(:, c - d) for c >= d and 0 otherwise (dispmap_ncc.m:145-154 with an integer d: a
pure shift).  Over the 5 x 5 window and the three channels, zero padded (conv2 'same'), let

    Sa = sum a,  Saa = sum a^2,  Sb = sum b,  Sbb = sum b^2,  Sab = sum a b      (integers, all below 2^53).

oracle/terms.compute_ncc (dispmap_ncc.m:116-198) has, with n = 75 = 25 taps x 3 channels,
    mean0 = Sa / n, meanT = Sb / n                                  (box * (1 / 25 / 3), summed over the channels)
    norm0^2 = Saa - 2 mean0 Sa + n mean0^2 = Saa - Sa^2 / n         = V0 / n,   V0 = n Saa - Sa^2
    normT^2 = Sbb - 2 meanT Sb + n meanT^2 = Sbb - Sb^2 / n         = VT / n,   VT = n Sbb - Sb^2
    num     = Sab - mean0 Sb - meanT Sa + n meanT mean0 = Sab - Sa Sb / n = N / n,   N = n Sab - Sa Sb
so that
    NCC = num / norm0 / normT = (N / n) / sqrt(V0 VT / n^2) = N / sqrt(V0 VT).
V0 and VT are n times a sum of squares about the mean: never negative, and zero exactly where the window is constant.
A pixel is LIVE where c >= d (columns left of round(d + 1) are masked, dispmap_ncc.m:190-191: exactly 0), and DEFINED
where it is live and V0 > 0 and VT > 0.  V0, VT <= 75 * 75 * 255^2 < 3.7e8, so V0 VT < 1.4e17 fits int64 and the 64-bit
mantissa of np.longdouble; the value is one correctly rounded square root and one division away from the integers.
A live pixel that is not defined has a zero norm: the quotient is not finite and becomes 0 (dispmap_ncc.m:190).

How far a correct double-precision evaluation may be from it: every term of the three differences above carries a
rounding error relative to ITS size, so the error of the value relative to 2^-52 is governed by
    cond = n Saa / V0 + n Sbb / VT + (n |Sab| + |Sa Sb|) / sqrt(V0 VT)
(>= 2 + |NCC|: the first two summands are >= 1 each, the third is >= |N| / sqrt(V0 VT); it is NOT always >= 3 -- the
matrix below has defined pixels at 2.68) and the bound is |value - exact| <= c * 2^-52 * cond.  R_ORACLE below is the
restatement's largest |value - exact| / (2^-52 cond) over every instance of this module; the device is held to
c = 4 R_ORACLE (a factor 2 as everywhere for device against oracle, DESIGN section 2, and another 2 for the reciprocal
norms of ncc_stats_kernel: about 1.5 more roundings of the value itself, 0.75 * 2^-52 |NCC|, against cond >= 2 + |NCC|).
"""
import ctypes as C

import numpy as np

N_WIN = 75
EPS = 2.0 ** -52

# Largest |oracle/terms.compute_ncc - exact| / (2^-52 cond) over instances(256): measured 0.6647, on "cols31", the
# instance with the most pixels; the others give 0.25 to 0.64 (tests/test_ncc_exact_cpu.py prints the figures and
# asserts on every run that the restatement stays below the constant).
R_ORACLE = 0.665
C_DEVICE = 4 * R_ORACLE

assert np.finfo(np.longdouble).nmant >= 63, "ncc_exact needs an extended-precision np.longdouble"


def _box(x):
    """5 x 5 box sum with zero padding of an (H, W) int64 array."""
    H, W = x.shape
    pad = np.zeros((H + 4, W + 4), np.int64)
    pad[2:2 + H, 2:2 + W] = x
    out = np.zeros((H, W), np.int64)
    for dx in range(5):
        for dy in range(5):
            out += pad[dy:dy + H, dx:dx + W]
    return out


def _as_int(im):
    a = np.asarray(im)
    i = a.astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == 3 and np.array_equal(i, a) and i.min() >= 0 and i.max() <= 255
    return i


def exact_ncc(im0, im1, disparities):
    """-> dict of (H, W, D) arrays: `value` (np.longdouble, 0 where masked or not defined), `cond` (float64, 0 where not
    defined), `live` (c >= d), `defined` (live, V0 > 0, VT > 0)."""
    a, r = _as_int(im0), _as_int(im1)
    H, W, _ = a.shape
    disparities = np.asarray(disparities)
    D = len(disparities)
    Sa = sum(_box(a[:, :, ch]) for ch in range(3))
    Saa = sum(_box(a[:, :, ch] ** 2) for ch in range(3))
    V0 = N_WIN * Saa - Sa * Sa
    value = np.zeros((H, W, D), np.longdouble)
    cond = np.zeros((H, W, D))
    live = np.zeros((H, W, D), bool)
    defined = np.zeros((H, W, D), bool)
    col = np.arange(W)[None, :]
    for i in range(D):
        d = int(disparities[i])
        assert d == disparities[i] and 0 <= d < W
        b = np.zeros_like(r)
        b[:, d:] = r[:, :W - d]
        Sb = sum(_box(b[:, :, ch]) for ch in range(3))
        Sbb = sum(_box(b[:, :, ch] ** 2) for ch in range(3))
        Sab = sum(_box(a[:, :, ch] * b[:, :, ch]) for ch in range(3))
        VT = N_WIN * Sbb - Sb * Sb
        Nn = N_WIN * Sab - Sa * Sb
        assert V0.min() >= 0 and VT.min() >= 0
        lv = np.broadcast_to(col >= d, (H, W))
        df = lv & (V0 > 0) & (VT > 0)
        prod = np.where(df, V0 * VT, 1)
        root = np.sqrt(prod.astype(np.longdouble))      # V0 VT < 2^57: exact in the 64-bit mantissa
        value[:, :, i] = np.where(df, Nn.astype(np.longdouble) / root, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            cn = (N_WIN * Saa / np.where(df, V0, 1) + N_WIN * Sbb / np.where(df, VT, 1)
                  + (N_WIN * np.abs(Sab) + np.abs(Sa * Sb)) / root.astype(np.float64))
        cond[:, :, i] = np.where(df, cn, 0)
        live[:, :, i] = lv
        defined[:, :, i] = df
    return dict(value=value, cond=cond, live=live, defined=defined)


def ratio(got, ex):
    """|got - exact| / (2^-52 cond) on the defined pixels (0 elsewhere); got is (H, W, D)."""
    err = np.abs(np.asarray(got, np.float64).astype(np.longdouble) - ex["value"]).astype(np.float64)
    return np.where(ex["defined"], err / (EPS * np.where(ex["defined"], ex["cond"], 1.0)), 0.0)


def check_against_exact(got, ex, c, what):
    """The two rules that together cover every pixel: within c 2^-52 cond of the exact value where it is defined,
    exactly 0.0 everywhere else (masked columns, zero variance).  Returns (worst ratio, largest cond)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ex["value"].shape, what
    und = ~ex["defined"]
    nz = np.argwhere(und & (got != 0.0))
    assert nz.size == 0, "%s: %d pixels that are masked or have a zero variance are not exactly 0.0; first (row, col, i) = %s: %r (live: %s)" % (
        what, len(nz), tuple(nz[0]), got[tuple(nz[0])], bool(ex["live"][tuple(nz[0])]))
    rt = ratio(got, ex)
    k = np.unravel_index(np.argmax(rt), rt.shape)
    assert rt[k] <= c, "%s: |value - exact| = %.3g 2^-52 cond > %.3g 2^-52 cond at (row, col, i) = %s: device %r, exact %r, cond %.4g" % (
        what, rt[k], c, tuple(int(v) for v in k), got[k], float(ex["value"][k]), ex["cond"][k])
    # Cauchy-Schwarz, |NCC| <= 1: follows from the bound, asserted on its own so that a failure says so
    over = np.where(ex["defined"], np.abs(got) - (1 + c * EPS * ex["cond"]), -1.0)
    k2 = np.unravel_index(np.argmax(over), over.shape)
    assert over[k2] <= 0, "%s: Cauchy-Schwarz: |value| = %r > 1 + c 2^-52 cond at %s (cond %.4g)" % (
        what, abs(got[k2]), tuple(int(v) for v in k2), ex["cond"][k2])
    return float(rt[k]), float(ex["cond"].max())


def true_shift_interior(ex, disparities, shift, W):
    """Mask of the defined pixels of the true disparity's slice whose window lies inside the filled columns on both
    sides (d + 2 <= c <= W - 3): a and b agree on the whole window there, the exact value is 1."""
    m = np.zeros(ex["defined"].shape, bool)
    col = np.arange(W)
    for i, d in enumerate(disparities):
        if d == shift:
            m[:, :, i] = ex["defined"][:, :, i] & ((col >= d + 2) & (col <= W - 3))[None, :]
    return m


# ------------------------------------------------------------------------------------------- images

def _smoothed(rng, H, Wb):
    base = rng.uniform(0, 255, size=(H, Wb, 3))
    for _ in range(2):   # smooth a little so that NCC has structure (as _images of test_terms_gpu.py)
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1)) / 3
    return base


def _cut(base, W, shift):
    """Left and right image as cuts of one base: im1(:, x) = im0(:, x + shift), so b == a at d = shift."""
    return np.round(base[:, 6 + shift:6 + shift + W]), np.round(base[:, 6 + 2 * shift:6 + 2 * shift + W])


def textured(seed, H, W, shift, raw=False):
    base = _smoothed(np.random.default_rng(seed), H, W + 2 * shift + 12)
    if raw:      # not rounded: the scaling checks want a non-integer image too
        return base[:, 6 + shift:6 + shift + W].copy(), base[:, 6 + 2 * shift:6 + 2 * shift + W].copy()
    return _cut(base, W, shift)


LOW_VARIANCE = ("wall", "block255", "block0", "ramp")


def low_variance(kind, seed, H, W, shift):
    """Flat regions are equal in the three channels and take their constant from {0, 200, 255}."""
    rng = np.random.default_rng(seed)
    Wb = W + 2 * shift + 12
    if kind == "wall":       # 200 with a 4 % sprinkle of +-1 and +-2 bumps, per channel sample
        base = np.full((H, Wb, 3), 200.0)
        bump = rng.choice([-2.0, -1.0, 1.0, 2.0], size=base.shape)
        base += np.where(rng.uniform(size=base.shape) < 0.04, bump, 0.0)
    elif kind in ("block255", "block0"):
        base = _smoothed(rng, H, Wb)
        r0, c0 = H // 4, 6 + shift + W // 4
        base[r0:r0 + max(6, H // 2), c0:c0 + max(7, W // 4)] = 255.0 if kind == "block255" else 0.0
    elif kind == "ramp":
        base = np.broadcast_to(((7 * np.arange(Wb)) % 256).astype(np.float64)[None, :, None], (H, Wb, 3)).copy()
    else:
        raise ValueError(kind)
    return _cut(base, W, shift)


# ------------------------------------------------------------------------------------------- host rule

SEG0, SEG1 = 36, 96          # columns of the left / right row segment ncc_lane_kernel stages (kNlSeg0, kNlSeg1)
LANE_ROWS = 12               # output rows of its workgroup (kNlRows)


def chunk_span(disparities):
    d = np.asarray(disparities, np.float64)
    return int(max(d[c:c + 64].max() - d[c:c + 64].min() for c in range(0, len(d), 64)))


def host_rule(H, W, disparities, cus, layout, rowlanes=False, naive=False):
    """launch_ncc_volume restated: -> (path, cols) with path in 'per-tap', 'cross', 'lanes' (cols only for 'lanes')."""
    d = np.asarray(disparities, np.float64)
    if naive or not np.all((d >= 0) & (d < W) & (d == np.floor(d))):
        return "per-tap", None
    span = chunk_span(d)
    if layout != 1 or rowlanes or span + 5 + 8 > SEG1:
        return "cross", None
    rt, dc = -(-H // LANE_ROWS), -(-len(d) // 64)
    chunks = max(1, -(-2 * cus // (rt * dc)))
    cols = max(8, -(-W // chunks))
    return "lanes", min(cols, SEG0 - 5, SEG1 - 5 - span)


PATHS = ("per-tap", "cross", "lanes")       # the path codes of stereo_ncc_volume_rule


def library_rule():
    """-> rule(H, W, disparities, cus, layout, rowlanes=False, naive=False) with nx.host_rule's answer, and the full
    answer (path, cols, chunks, span) as rule.full(...).  No device is touched."""
    from stereo_amd import _lib
    fn = _lib.lib().stereo_ncc_volume_rule
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int] + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 4 + [
        C.c_char_p, C.c_size_t]

    def full(H, W, disparities, cus, layout, rowlanes=False, naive=False):
        d = np.ascontiguousarray(disparities, np.float64)
        out = [C.c_int(-1) for _ in range(4)]
        err = C.create_string_buffer(256)
        rc = fn(H, W, d.ctypes.data_as(C.POINTER(C.c_double)), len(d), 2, layout, cus, int(naive), int(rowlanes),
                *[C.byref(o) for o in out], err, len(err))
        assert rc == 0, err.value.decode()
        path, cols, chunks, span = (o.value for o in out)
        return PATHS[path], cols, chunks, span

    def rule(*args, **kw):
        path, cols, chunks, span = full(*args, **kw)
        if path != "lanes":
            assert (cols, chunks, span) == (0, 0, 0)
            return path, None
        return path, cols
    rule.full = full
    return rule


# ------------------------------------------------------------------------------------------- the geometry matrix

PERM64 = np.random.default_rng(64).permutation(64)
TWO_CHUNKS = np.concatenate([PERM64, [5, 74, 30, 12, 60, 74]]).astype(np.float64)
LOW_DISPS = np.array([0.0, 2.0, 5.0, 27.0, 29.0])
INSTANCE_NAMES = ("two-chunks", "span82", "span83", "span83-base3", "span84", "cols31", "cols10", "cross-ragged",
                  "cross-exact", "cross-stride2", "tiny-6x7", "tiny-6x3", "tiny-1x6", "tiny-6x1") + tuple(
                      "low-" + kind + tail for kind in LOW_VARIANCE for tail in ("", "-two-chunks"))


def instances(cus, meant=True):
    """name -> dict(im0, im1, disps, shift, lanes=(path, cols) the host rule must give for layout 1): every case of
    the matrix.  `cus` is the device's compute-unit count (the widths of the clamp and span cases follow it).
    meant=False: the same construction for a count so small that the widths no longer reach the geometries the cases
    are named for (a comparison of rules wants those too); `lanes` is then whatever the host rule gives."""
    out = {}

    def add(name, im, disps, shift, want):
        disps = np.asarray(disps, np.float64)
        H, W, _ = im[0].shape
        got = host_rule(H, W, disps, cus, 1)
        assert not meant or want is None or got == want, "%s: the host rule gives %s, the case is meant to run %s" % (name, got, want)
        out[name] = dict(im0=im[0], im1=im[1], disps=disps, shift=shift, lanes=got)

    # two label chunks, the second ragged; unsorted, duplicates, not from 0; two row tiles, the second of one row
    add("two-chunks", textured(21, 13, 80, 30), TWO_CHUNKS, 30, ("lanes", 8))
    # span boundary of the staged segment
    Ws = 9 * cus - 5
    add("span82", textured(22, 13, Ws, 82), [0, 82], 82, ("lanes", 9))
    add("span83", textured(23, 13, Ws, 83), [0, 83], 83, ("lanes", 8))
    add("span83-base3", textured(24, 13, Ws, 86), [3, 86], 86, ("lanes", 8))
    add("span84", textured(25, 13, Ws, 84), [0, 84], 84, ("cross", None))
    # column clamp
    add("cols31", textured(26, 12, 31 * 2 * cus + 7, 1), [0, 1, 2], 1, ("lanes", 31))
    add("cols10", textured(27, 12, 10 * 2 * cus - 3, 2), [0, 1, 2], 2, ("lanes", 10))
    # cross kernel's tiles: ragged and exact (lanes for layout 1 unless forced)
    add("cross-ragged", textured(28, 61, 33, 3), np.arange(17), 3, ("lanes", 8))
    add("cross-exact", textured(29, 60, 32, 3), np.arange(16), 3, ("lanes", 8))
    add("cross-stride2", textured(30, 5, 130, 4), np.arange(0, 128, 2), 4, ("cross", None))
    # disparity at the right edge, tiny images
    add("tiny-6x7", textured(31, 6, 7, 1), np.arange(7), 1, ("lanes", 8))
    add("tiny-6x3", textured(32, 6, 3, 1), np.arange(3), 1, ("lanes", 8))
    add("tiny-1x6", textured(33, 1, 6, 1), np.arange(3), 1, ("lanes", 8))
    add("tiny-6x1", textured(34, 6, 1, 0), [0], 0, ("lanes", 8))
    # low variance
    for k, kind in enumerate(LOW_VARIANCE):
        add("low-" + kind, low_variance(kind, 40 + k, 14, 30, 2), LOW_DISPS, 2, ("lanes", 8))
        add("low-" + kind + "-two-chunks", low_variance(kind, 50 + k, 13, 80, 30), TWO_CHUNKS, 30, ("lanes", 8))
    assert tuple(out) == INSTANCE_NAMES
    return out
