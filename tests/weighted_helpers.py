"""Shared by the weighted-scanline and contrast tests: step weights taken from a grid graph's edge
weights, and small images.  NumPy only."""
import numpy as np

AXIS_DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0))
PARAMS = {"ramp": (2.0, 0.25, 0.125, 0.5), "step": (1.5, 0.5, 0.25, 0.25), "rising": (0.25, 3.0, 0.0625, 0.75)}


def steps_from_edges(conn, alphas, shape, directions=AXIS_DIRECTIONS):
    """wstep (R x N) for axis directions on a grid graph with ONE edge per neighbour pair (any order and orientation):
    wstep[r, p] = the alpha of the edge between p and its predecessor p - r, 0.0 where there is none."""
    H, W = shape
    conn = np.asarray(conn).astype(np.int64).reshape(2, -1)
    weight = {}
    for e in range(conn.shape[1]):
        key = (min(conn[0, e], conn[1, e]), max(conn[0, e], conn[1, e]))
        assert key not in weight
        weight[key] = alphas[e]
    out = np.zeros((len(directions), H * W))
    for r, (dy, dx) in enumerate(directions):
        assert dy == 0 or dx == 0
        for x in range(W):
            for y in range(H):
                yp, xp = y - dy, x - dx
                if 0 <= yp < H and 0 <= xp < W:
                    p, pp = x * H + y, xp * H + yp
                    out[r, p] = weight[(min(p, pp), max(p, pp))]
    return out


def image(rng, H, W, C, dyadic=True):
    """H x W x C with flat patches and edges: values on a 2^-4 grid in [0, 1] (differences are then exact), or any."""
    if dyadic:
        return rng.integers(0, 17, size=(H, W, C)).astype(np.float64) / 16.0
    return rng.random((H, W, C))
