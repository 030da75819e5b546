"""NumPy restatement of the plane-candidate problem's definition (include/stereo_hip.h): what
stereo_plane_candidates_gather, stereo_plane_candidates_inputs_ncc / _globalstereo and stereo_plane_candidates_apply must
give, bit for bit.  Label k at pixel i is the plane pcand[:, k, i]; its unary and positions are the oracle's restatement
of the reference (oracle.terms) on the K proposals pcand[:, k, :], and nothing is added.  A table is a (4, K, N) array
(component, label, pixel; pixels column major).  Test infrastructure."""
import numpy as np

from oracle import terms as OT

import candidates_restate
import plane_band_restate


def gather(planes, offsets, shape, sources=(), taps=()):
    """planes 4 x N, sources a list of 4 x N plane maps of an image of `shape` = (H, W), taps a list of (dy, dx)
    -> pcand (4, K, N): the own plane moved by offsets_k (one multiplication, one subtraction), then per source and tap
    the source's plane at the clamped neighbour, copied."""
    P = np.asarray(planes, np.float64)
    H, W = shape
    assert P.shape == (4, H * W)
    rows = plane_band_restate.proposals(P, offsets)
    y, x = np.mgrid[0:H, 0:W]
    for src in sources:
        src = np.asarray(src, np.float64)
        assert src.shape == (4, H * W)
        for dy, dx in taps:
            at = np.clip(y + int(dy), 0, H - 1) + H * np.clip(x + int(dx), 0, W - 1)      # H x W: the neighbour's index
            rows.append(src[:, at.T.reshape(-1)])
    return np.stack(rows, axis=1)


def fronto(m):
    """H x W map -> 4 x N planes [0 0 1 -v]"""
    return candidates_restate.planes(np.asarray(m, np.float64).T.reshape(-1))


def table_of(cand):
    """the fronto-parallel table of a candidate table cand (K x N) -> (4, K, N)"""
    return np.stack([candidates_restate.planes(row) for row in np.asarray(cand, np.float64)], axis=1)


def _proposals(pcand):
    pcand = np.asarray(pcand, np.float64)
    assert pcand.ndim == 3 and pcand.shape[0] == 4
    return [np.array(pcand[:, k, :]) for k in range(pcand.shape[1])]


def inputs_ncc(ncc, disparities, unary_weight, pcand, conn):
    """ncc H x W x D; pcand (4, K, N); conn 2 x E zero based -> (unary K x N, q K x E, qprim K x E)."""
    H, W = ncc.shape[:2]
    points = OT.get_points(H, W)
    props = _proposals(pcand)
    unary = np.stack([OT.ncc_unary_cost(ncc, disparities, unary_weight, P, points) for P in props])
    return (unary,) + plane_band_restate.positions(props, conn, points)


def inputs_globalstereo(im0, im1, P2, d_min, d_step, col_thresh, pcand, conn):
    """im0, im1 H x W x C; P2 4 x 3 -> (unary K x N, q K x E, qprim K x E), positions rescaled."""
    H, W = im0.shape[:2]
    points = OT.get_points(H, W)
    props = _proposals(pcand)
    unary = np.stack([OT.globalstereo_unary_cost(im0, im1, P2, d_min, d_step, col_thresh, P, points) for P in props])
    return (unary,) + plane_band_restate.positions(props, conn, points, d_min, d_step)


def apply(pcand, labels):
    """labels: N values, one based -> 4 x N: pcand[:, label - 1, pixel], copied."""
    pcand = np.asarray(pcand, np.float64)
    k = np.asarray(labels).astype(np.int64).reshape(-1) - 1
    if k.min() < 0 or k.max() >= pcand.shape[1]:
        raise ValueError("label outside 1 .. K")
    return pcand[:, k, np.arange(pcand.shape[2])]


# ---- the chain of the issue: candidates_restate's 17-pixel chain made slanted (shared by the CPU test, which pins the
# optima, and the device test, which solves it) ------------------------------------------------------------------------

CHAIN_N = candidates_restate.CHAIN_N
CHAIN_WEIGHT, CHAIN_LAMBDA = candidates_restate.CHAIN_WEIGHT, candidates_restate.CHAIN_LAMBDA
CHAIN_BAND = candidates_restate.CHAIN_BAND                       # -2 .. 2 by 1/2, K = 9
CHAIN_SLICES = 26
CHAIN_OFFSETS = np.array([-0.5, 0.0, 0.5])
CHAIN_STEPS = (-1, 1, -2, 2, -4, 4)                              # taps along the chain; K = 3 + 6 = 9


def chain(shape):
    """The 17-pixel chain as a 1 x 17 or 17 x 1 image -> dict(ncc H x W x 26, disp, truth 4 x 17, base 4 x 17, conn, level,
    fronto_level).  Slope -1 along the chain: the planes are [-1 0 1 d] (1 x 17) or [0 -1 1 d] (17 x 1); plane A has
    d = -1, disparity t + 1 at the chain coordinate t = 1 .. 17, plane B has d = -7, disparity t + 7.  The truth is A on
    pixels 0 .. 7 and B on pixels 8 .. 16; the base equals the truth but for B on pixels 1, 2, 3 and 6 and A on pixels
    11 .. 15: nine wrong pixels, each 6 away, beyond the plane band's half-width 2.  26 slices at 1 .. 26; the volume is
    on a 2^-7 grid in [-1, 0] but for 1.0 at the true slice."""
    H, W = shape
    assert H * W == CHAIN_N and min(H, W) == 1
    along_x = H == 1
    slope = np.array([-1.0, 0.0, 1.0]) if along_x else np.array([0.0, -1.0, 1.0])
    plane = lambda d: np.concatenate([slope, [d]])
    A, B = plane(-1.0), plane(-7.0)
    is_a = np.arange(CHAIN_N) < 8
    truth = np.where(is_a, A[:, None], B[:, None])
    base_is_a = is_a.copy()
    base_is_a[[1, 2, 3, 6]] = False
    base_is_a[11:16] = True
    base = np.where(base_is_a, A[:, None], B[:, None])
    t = 1.0 + np.arange(CHAIN_N)
    true_disp = np.where(is_a, t + 1.0, t + 7.0)
    disp = 1.0 + np.arange(CHAIN_SLICES, dtype=np.float64)
    rng = np.random.default_rng(2025)
    vol = rng.integers(-128, 1, size=(CHAIN_N, CHAIN_SLICES)).astype(np.float64) / 128.0
    vol[np.arange(CHAIN_N), (true_disp - 1).astype(int)] = 1.0
    taps = [(0, s) if along_x else (s, 0) for s in CHAIN_STEPS]
    conn = np.stack([np.arange(CHAIN_N - 1), np.arange(1, CHAIN_N)])
    return dict(ncc=vol.reshape(H, W, CHAIN_SLICES), disp=disp, truth=np.asfortranarray(truth), base=np.asfortranarray(base),
                true_disp=true_disp, base_disp=np.where(base_is_a, t + 1.0, t + 7.0).reshape(H, W), conn=conn,
                level=dict(offsets=CHAIN_OFFSETS, taps=taps, sources=["base"]),
                fronto_level=dict(offsets=CHAIN_OFFSETS, taps=taps, sources=["base"]))
