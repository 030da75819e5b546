"""NumPy restatement of the band problem's definition (include/stereo_hip.h): what stereo_band_inputs
and stereo_band_apply must give, bit for bit.  Label k at pixel i is the fronto-parallel plane [0 0 1 -(base_i + offsets_k)];
its unary and positions are the oracle's restatement of the reference (oracle.terms) on that plane.  Test infrastructure."""
import numpy as np

from oracle import terms as OT


def planes(base, delta):
    """4 x N: the proposal of one band label, pixels in column-major order."""
    b = np.asarray(base, np.float64).T.reshape(-1)
    P = np.zeros((4, b.shape[0]))
    P[2] = 1.0
    P[3] = -(b + np.float64(delta))
    return P


def band_inputs(ncc, disparities, unary_weight, base, offsets, conn):
    """ncc H x W x D; conn 2 x E zero based -> (unary K x N, q K x E, qprim K x E)."""
    base = np.asarray(base, np.float64)
    H, W = base.shape
    points = OT.get_points(H, W)
    props = [planes(base, d) for d in offsets]
    unary = np.stack([OT.ncc_unary_cost(ncc, disparities, unary_weight, P, points) for P in props])
    conn = np.asarray(conn, np.int64)
    q, qprim = OT.trws_positions(props, conn[0], conn[1], points)
    return unary, q.T, qprim.T


def band_apply(base, labels, offsets):
    """labels: N values, one based, column-major pixel order -> H x W."""
    base = np.asarray(base, np.float64)
    H, W = base.shape
    k = np.asarray(labels).astype(np.int64).reshape(W, H).T - 1
    if k.min() < 0 or k.max() >= len(offsets):
        raise ValueError("label outside 1 .. K")
    return base + np.asarray(offsets, np.float64)[k]


def same(a, b):
    """equal as IEEE values, NaN in the same places (the sign of a zero is not compared)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(np.isnan(a), np.isnan(b))) and bool(np.array_equal(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0)))


def same_bits(a, b):
    """the same bytes: signs of zeros included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the shapes and inputs of the device tests (shared with the CPU test, built once) ------------------------------

def volume(H, W, D, seed, bits=6):
    """H x W x D correlation values in [-1, 1] on a dyadic grid"""
    rng = np.random.default_rng([H, W, D, seed])
    return rng.integers(-(1 << bits), (1 << bits) + 1, size=(H, W, D)).astype(np.float64) / float(1 << bits)


def disparities_for(D, shuffled, seed=0):
    d = 2.0 + np.arange(D, dtype=np.float64)          # slices at 2, 3, ..., D + 1
    return np.random.default_rng([D, seed]).permutation(d) if shuffled and D > 1 else d


def base_map(H, W, D, max_offset, seed):
    """Quarter-pixel bases over [2 - 2, D + 1 + 2] with, in this order at the first pixels (column major) as far as
    the map has room: exactly on a slice, exactly midway between two (the tie rule), below the range, above it, on the
    last slice (so that base + a positive offset leaves the range), on the first slice, and a zero disparity sum
    (base = -max_offset: base + max_offset is 0)."""
    rng = np.random.default_rng([H, W, D, seed, 7])
    lo, hi = 2.0, D + 1.0
    b = rng.integers(int(4 * (lo - 2)), int(4 * (hi + 2)) + 1, size=H * W).astype(np.float64) / 4.0
    crafted = [lo + (D // 2), lo + 0.5 if D > 1 else lo, lo - 1.25, hi + 1.75, hi, lo, -float(max_offset)]
    b[:min(len(crafted), H * W)] = crafted[:H * W]
    return b.reshape(W, H).T.copy()
