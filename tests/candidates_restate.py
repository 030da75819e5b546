"""NumPy restatement of the candidate problem's definition (include/stereo_hip.h): what
stereo_candidates_gather, stereo_candidates_inputs and stereo_candidates_apply must give, bit for bit.  Label k at pixel i
is the fronto-parallel plane [0 0 1 -cand[k, i]]; its unary and positions are the oracle's restatement of the reference
(oracle.terms) on that plane, and nothing is added.  Test infrastructure."""
import numpy as np

from oracle import terms as OT


def gather(base, offsets, sources=(), taps=()):
    """base H x W, sources a list of H x W maps, taps a list of (dy, dx) -> cand K x N, pixels column major:
    rows base + offsets_k, then per source and tap the source at the clamped neighbour, copied."""
    base = np.asarray(base, np.float64)
    H, W = base.shape
    rows = [(base + np.float64(d)).T.reshape(-1) for d in offsets]
    y, x = np.mgrid[0:H, 0:W]
    for src in sources:
        src = np.asarray(src, np.float64)
        assert src.shape == (H, W)
        for dy, dx in taps:
            rows.append(src[np.clip(y + int(dy), 0, H - 1), np.clip(x + int(dx), 0, W - 1)].T.reshape(-1))
    return np.stack(rows)


def planes(cand_row):
    """4 x N: the proposal of one label."""
    c = np.asarray(cand_row, np.float64)
    P = np.zeros((4, c.shape[0]))
    P[2] = 1.0
    P[3] = -c
    return P


def candidates_inputs(ncc, disparities, unary_weight, cand, shape, conn):
    """ncc H x W x D; cand K x N; conn 2 x E zero based -> (unary K x N, q K x E, qprim K x E)."""
    H, W = shape
    points = OT.get_points(H, W)
    props = [planes(row) for row in np.asarray(cand, np.float64)]
    unary = np.stack([OT.ncc_unary_cost(ncc, disparities, unary_weight, P, points) for P in props])
    conn = np.asarray(conn, np.int64)
    q, qprim = OT.trws_positions(props, conn[0], conn[1], points)
    return unary, q.T, qprim.T


def candidates_apply(cand, labels, shape):
    """labels: N values, one based, column-major pixel order -> H x W: cand[label - 1, pixel], copied."""
    H, W = shape
    cand = np.asarray(cand, np.float64)
    k = np.asarray(labels).astype(np.int64).reshape(-1) - 1
    if k.min() < 0 or k.max() >= cand.shape[0]:
        raise ValueError("label outside 1 .. K")
    return cand[k, np.arange(H * W)].reshape(W, H).T


# ---- the chain of the issue: a step 4 -> 10 whose base has three short runs on the wrong side (shared by the CPU test,
# which pins its optimum, and the device test, which solves it) --------------------------------------------------------

CHAIN_N = 17
CHAIN_WEIGHT, CHAIN_LAMBDA = 4.0, 2.0
CHAIN_BAND = np.arange(-2.0, 2.25, 0.5)                         # K = 9
CHAIN_LEVEL = dict(offsets=np.array([-0.5, 0.0, 0.5]), taps=[(0, -1), (0, 1), (0, -2), (0, 2), (0, -4), (0, 4)],
                   sources=["base"])                           # K = 3 + 6 = 9


def chain(shape):
    """The 17-pixel chain as a 1 x 17 or 17 x 1 image -> dict(ncc H x W x 12, disp, truth, base, conn, level).
    12 slices one apart (1 .. 12); the volume is on a 2^-7 grid in [-1, 0] but for 1.0 at the true slice (so a parabola
    through three of its values stays below 1 away from a true slice: the true map alone has unary 0); the truth is 4 on
    pixels 0 .. 7 and 10 on pixels 8 .. 16; the base equals the truth but for the runs 1-3 and 6 (set to 10) and 11-15
    (set to 4): 6 away, beyond the band's half-width 2, with a right pixel 1, 2 or (pixel 13) 4 steps away."""
    H, W = shape
    assert H * W == CHAIN_N and min(H, W) == 1
    disp = 1.0 + np.arange(12, dtype=np.float64)
    truth = np.where(np.arange(CHAIN_N) < 8, 4.0, 10.0)
    base = truth.copy()
    base[[1, 2, 3, 6]] = 10.0
    base[11:16] = 4.0
    rng = np.random.default_rng(2024)
    vol = rng.integers(-128, 1, size=(CHAIN_N, 12)).astype(np.float64) / 128.0
    vol[np.arange(CHAIN_N), (truth - 1).astype(int)] = 1.0
    level = dict(CHAIN_LEVEL)
    if W == 1:                                                  # the chain runs along y
        level["taps"] = [(dx, dy) for dy, dx in CHAIN_LEVEL["taps"]]
    conn = np.stack([np.arange(CHAIN_N - 1), np.arange(1, CHAIN_N)])
    return dict(ncc=vol.reshape(H, W, 12), disp=disp, truth=truth.reshape(H, W), base=base.reshape(H, W), conn=conn, level=level)
