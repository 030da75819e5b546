"""NumPy restatement of the plane-band problem's definition (include/stereo_hip.h): what
stereo_plane_band_inputs_ncc / _globalstereo and stereo_plane_band_apply must give.  Label k at pixel i is pixel i's own
plane moved along the disparity axis, P[3] - P[2] * offsets_k; its unary and positions are the oracle's restatement of the
reference (oracle.terms) on those K proposals.  It adds nothing of its own.  Test infrastructure."""
import numpy as np

from oracle import terms as OT


def proposals(planes, offsets):
    """The K proposals, each 4 x N: one multiplication and one subtraction per pixel and label."""
    P = np.asarray(planes, np.float64)
    out = []
    for delta in np.asarray(offsets, np.float64):
        Q = P.copy()
        Q[3] = P[3] - P[2] * delta
        out.append(Q)
    return out


def disp_fn(d_min, d_step):
    """plane -> position: the rescaling of stereo_trws_positions when d_step != 0"""
    if d_step == 0:
        return OT.disparity_from_assignment
    return lambda a, p: OT.globalstereo_rescale(OT.disparity_from_assignment(a, p), d_min, d_step)


def positions(props, conn, points, d_min=0.0, d_step=0.0):
    conn = np.asarray(conn, np.int64)
    q, qprim = OT.trws_positions(props, conn[0], conn[1], points, disp_fn=disp_fn(d_min, d_step))
    return q.T, qprim.T


def inputs_ncc(ncc, disparities, unary_weight, planes, offsets, conn):
    """ncc H x W x D; planes 4 x N; conn 2 x E zero based -> (unary K x N, q K x E, qprim K x E)."""
    H, W = ncc.shape[:2]
    points = OT.get_points(H, W)
    props = proposals(planes, offsets)
    unary = np.stack([OT.ncc_unary_cost(ncc, disparities, unary_weight, P, points) for P in props])
    return (unary,) + positions(props, conn, points)


def inputs_globalstereo(im0, im1, P2, d_min, d_step, col_thresh, planes, offsets, conn):
    """im0, im1 H x W x C; P2 4 x 3 -> (unary K x N, q K x E, qprim K x E), positions rescaled."""
    H, W = im0.shape[:2]
    points = OT.get_points(H, W)
    props = proposals(planes, offsets)
    unary = np.stack([OT.globalstereo_unary_cost(im0, im1, P2, d_min, d_step, col_thresh, P, points) for P in props])
    return (unary,) + positions(props, conn, points, d_min, d_step)


def apply(planes, labels, offsets):
    """labels: N values, one based -> 4 x N."""
    P = np.asarray(planes, np.float64)
    k = np.asarray(labels).astype(np.int64).reshape(-1) - 1
    if k.min() < 0 or k.max() >= len(offsets):
        raise ValueError("label outside 1 .. K")
    out = P.copy()
    out[3] = P[3] - P[2] * np.asarray(offsets, np.float64)[k]
    return out


# ---- the inputs of the tests (shared by the CPU and the device tests, built once) -----------------------------------

def planes_through(base, seed, dyadic=True):
    """4 x N planes whose disparity at the pixel's own point is base (H x W).  dyadic: a and b multiples of 1/4 in
    [-1, 1], c in {1, -1, 2} -- the first pixel has c = -1, the second c = 2 -- and d = -(c base + a x + b y), all exact
    when base is a multiple of 1/4.  Otherwise a, b arbitrary, c = 3, and d is rounded."""
    base = np.asarray(base, np.float64)
    H, W = base.shape
    N = H * W
    rng = np.random.default_rng([H, W, seed, 31])
    pts = OT.get_points(H, W)
    b0 = base.T.reshape(-1)
    if dyadic:
        a = rng.integers(-4, 5, size=N).astype(np.float64) / 4.0
        b = rng.integers(-4, 5, size=N).astype(np.float64) / 4.0
        c = rng.choice(np.array([1.0, -1.0, 2.0]), size=N)
        c[0] = -1.0
        if N > 1:
            c[1] = 2.0
    else:
        a, b, c = rng.normal(0, 0.1, N), rng.normal(0, 0.1, N), np.full(N, 3.0)
    d = -(c * b0 + (a * pts[0] + b * pts[1]))
    return np.asfortranarray(np.stack([a, b, c, d]))


def slanted_map(H, W, a=0.25, b=-0.5, c=2.0, d=-9.0):
    """every pixel carries the same slanted plane"""
    return np.asfortranarray(np.repeat(np.array([[a], [b], [c], [d]]), H * W, axis=1))


# globalstereo: the projection of example_global.m (P2[3, 0] = -0.25: X = x - disp / 4, Y = y) and one that moves along
# the rows instead (Y = y + disp / 2), so that the crafted pixels reach the row branches of the interpolation too
def P2_example():
    P2 = np.zeros((4, 3))
    P2[0, 0] = P2[1, 1] = P2[2, 2] = 1.0
    P2[3, 0] = -0.25
    return P2


def P2_rows():
    P2 = np.zeros((4, 3))
    P2[0, 0] = P2[1, 1] = P2[2, 2] = 1.0
    P2[3, 1] = 0.5
    return P2


GS_DYADIC = (0.5, 4.0)        # d_min, d_step: (v - 0.5) / 4 and 4 (dhat + 0.5) are exact on multiples of 1/4


def images(H, W, C, seed):
    """Two H x W x C images of whole numbers in 100 .. 115: a squared colour difference stays below 225, so
    exp(-ssd / (col_thresh C)) is far from 0 and the unary tells the samples apart (on full-range noise it is log 2
    almost everywhere)."""
    rng = np.random.default_rng([H, W, C, seed, 5])
    return rng.integers(100, 116, size=(H, W, C)).astype(np.float64), rng.integers(100, 116, size=(H, W, C)).astype(np.float64)


def gs_projected(P2, d_min, d_step, planes, H, W):
    """(X, Y) of every pixel, as globalstereo_unary_cost forms them"""
    pts = OT.get_points(H, W)
    dhat = OT.globalstereo_rescale(OT.disparity_from_assignment(planes, pts), d_min, d_step)
    disp = d_step * (dhat + d_min)
    T = [(pts[0] * P2[0, k] + pts[1] * P2[1, k]) + (1.0 * P2[2, k] + disp * P2[3, k]) for k in range(3)]
    return T[0] * (1.0 / T[2]), T[1] * (1.0 / T[2])


GS_TARGETS = ("below 1", "exactly the last", "beyond the last", "exactly 1", "inside")


def gs_base_map(H, W, P2, d_min, d_step, seed):
    """Plane disparities (H x W, multiples of 1/4) for the globalstereo tests.  The first pixels (column major), as far
    as the map has room, project to a coordinate -- X when P2[3, 0] != 0, else Y -- that is, in GS_TARGETS' order: 0.5,
    exactly W (or H), W + 1 (H + 1), exactly 1, and W - 0.5 (H - 0.5).  Exact for the dyadic (d_min, d_step)."""
    rng = np.random.default_rng([H, W, seed, 77])
    N = H * W
    pd = rng.integers(-16, 17, size=N).astype(np.float64) / 4.0
    pts = OT.get_points(H, W)
    along_x = P2[3, 0] != 0
    size, coord, gain = (W, pts[0], P2[3, 0]) if along_x else (H, pts[1], P2[3, 1])
    targets = [0.5, float(size), size + 1.0, 1.0, size - 0.5]
    for i, t in enumerate(targets[:N]):
        disp = (t - coord[i]) / gain                     # coordinate = own + gain * disp
        pd[i] = disp - d_step * d_min + d_min            # disp = d_step ((pd - d_min) / d_step + d_min)
    return pd.reshape(W, H).T.copy()
