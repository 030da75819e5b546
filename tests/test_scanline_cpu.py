"""Scanline aggregation without a device: the NumPy restatement (tests/scanline_restate.py) against the
first-principles dynamic programme (first_principles.chain_dp) with zero tolerance, scanline.model_energy against
first_principles.energy_exact as a Fraction, and every refusal of the two C entries, which come before the device is
looked for.

Why zero tolerance: unaries are multiples of 2^-6, positions and weights of 2^-2, tol is dyadic or never cuts
(first_principles.LAMBDAS), so every term is a multiple of 2^-14 below 2^22 and every sum along a chain of at most 7
pixels is exact in fp64 in whatever order it is formed (the argument of first_principles' docstring)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import first_principles as fp
import scanline_restate as R

D = 4
SHAPES = [(5, 7), (7, 5)]
OPPOSITE = [((0, 1), (0, -1)), ((1, 0), (-1, 0)), ((1, 1), (-1, -1)), ((1, -1), (-1, 1))]


def dyadic_case(H, W, seed):
    rng = np.random.default_rng(seed)
    unary = rng.integers(0, 4 << 6, size=(D, H * W)).astype(np.float64) / 64.0
    positions = rng.integers(0, 12, size=D).astype(np.float64) * 0.25        # any order; repeats may occur
    weights = {d: float(rng.integers(0, 9)) * 0.25 for pair in OPPOSITE for d in pair[:1]}
    for a, b in OPPOSITE:
        weights[b] = weights[a]                                             # a scanline's two halves are one model
    return unary, positions, weights


def chain_problem(unary, H, pixels, positions, w):
    """The pixels of one chain as a path problem of first_principles: node s is pixels[s], every edge weighs w."""
    n = len(pixels)
    ids = [x * H + y for y, x in pixels]
    conn = np.array([(s, s + 1) for s in range(n - 1)], dtype=np.int64).reshape(-1, 2)
    q = np.tile(positions, (n - 1, 1))
    return dict(unary=np.ascontiguousarray(unary[:, ids].T), conn=conn, q=q, qprim=q.copy(), alphas=np.full(n - 1, w))


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_half_chains_and_scanline_min_marginals_equal_first_principles(shape, kernel):
    H, W = shape
    for seed, lam in enumerate(fp.LAMBDAS):
        unary, positions, weights = dyadic_case(H, W, [H, W, kernel, seed])
        L = {d: R.direction_costs(unary, shape, positions, kernel, lam, d, weights[d]) for d in R.DIRECTIONS_8}
        # every pixel, every direction: the last node's min-marginals of the prefix that ends at the pixel (its B is 0)
        for d in R.DIRECTIONS_8:
            for x in range(W):
                for y in range(H):
                    pixels = R.chain_pixels(shape, d, y, x)
                    opt, mm = fp.chain_dp(chain_problem(unary, H, pixels, positions, weights[d]), kernel, lam)
                    assert np.array_equal(L[d][:, x * H + y], mm[len(pixels) - 1]), (d, y, x, lam)
                    assert opt == L[d][:, x * H + y].min()
        # every opposite pair: the whole scanline's min-marginals
        for a, b in OPPOSITE:
            both = (L[a] + L[b]) - unary
            seen = np.zeros(H * W, bool)
            for x in range(W):
                for y in range(H):
                    if len(R.chain_pixels(shape, b, y, x)) > 1:
                        continue                            # (y, x) is not the last pixel of a's chain
                    pixels = R.chain_pixels(shape, a, y, x)
                    _, mm = fp.chain_dp(chain_problem(unary, H, pixels, positions, weights[a]), kernel, lam)
                    ids = [xx * H + yy for yy, xx in pixels]
                    assert np.array_equal(both[:, ids].T, mm), (a, y, x, lam)
                    seen[ids] = True
            assert seen.all()


def test_restated_outputs_on_a_crafted_volume():
    """labels: the first minimum, one based; confidence: 0 where the minimum occurs twice, +Inf at D = 1."""
    unary = np.array([[3.0, 1.0, 2.0], [1.0, 1.0, 5.0], [1.0, 4.0, 2.0]])          # D = 3, three pixels in a column
    S, labels, dmap, conf = R.aggregate(unary, (3, 1), [10.0, 30.0, 20.0], 1, 0.0, [(0, 1)])
    assert np.array_equal(S, unary) and labels.tolist() == [2, 1, 1] and labels.dtype == np.int32
    assert dmap.ravel().tolist() == [30.0, 10.0, 10.0] and conf.ravel().tolist() == [0.0, 0.0, 0.0]
    S, labels, dmap, conf = R.aggregate(unary[:1], (3, 1), [7.0], 2, 1.0, [(1, 0), (-1, 0)])
    assert labels.tolist() == [1, 1, 1] and np.isposinf(conf).all() and dmap.ravel().tolist() == [7.0] * 3
    assert S.ravel().tolist() == [3.0 + 6.0, 4.0 + 3.0, 6.0 + 2.0]


@pytest.mark.parametrize("kernel", [1, 2])
def test_model_energy_equals_the_exact_energy(kernel):
    from stereo_amd import scanline
    for seed in range(6):
        rng = np.random.default_rng([kernel, seed])
        p = fp.dyadic_problem(rng, 4, 5, 5, shared=True)
        x = rng.integers(0, 5, size=20)
        got = scanline.model_energy(p["unary"].T, p["conn"].T, p["alphas"], p["positions"], kernel, p["lam"], x + 1)
        assert Fraction(got) == fp.energy_exact(p, kernel, p["lam"], x)


# ---------------------------------------------------------------- refusals, before the device is looked for

def raw_call(device, **change):
    """One of the two C entries on small host arrays with one argument changed -> (rc, message)."""
    from stereo_amd import _lib
    a = dict(H=2, W=3, D=2, kernel=1, tol=1.0, R=2, directions=[1, 0, 0, -1], weights=[1.0, 0.5], positions=[0.0, 1.0],
             unary=[0.0] * 12, null=())
    a.update(change)
    keep = []

    def arr(name, values, dtype):
        if name in a["null"]:
            return None
        v = np.array(values, dtype=dtype)
        keep.append(v)
        return v.ctypes.data_as(C.c_void_p)

    err = _lib.errbuf()
    args = [arr("unary", a["unary"], np.float64), C.c_int(a["H"]), C.c_int(a["W"]), C.c_int(a["D"]),
            arr("positions", a["positions"], np.float64), C.c_int(a["kernel"]), C.c_double(a["tol"]),
            arr("directions", a["directions"], np.int32), arr("weights", a["weights"], np.float64), C.c_int(a["R"]),
            arr("S", [0.0] * 12, np.float64), arr("labels", [0] * 6, np.int32), arr("map", [0.0] * 6, np.float64),
            arr("confidence", [0.0] * 6, np.float64)]
    L = _lib.lib()
    if device:
        rc = L.stereo_scanline_aggregate_device(*args, None, err, C.c_size_t(len(err)))
    else:
        rc = L.stereo_scanline_aggregate(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


REFUSALS = [
    (dict(H=0), "H and W must be at least 1"),
    (dict(W=-1), "H and W must be at least 1"),
    (dict(H=1 << 16, W=1 << 15), "below 2\\^31"),
    (dict(D=0), "D must be 1 .. 256"),
    (dict(D=257), "D must be 1 .. 256"),
    (dict(kernel=0), "kernel must be 1"),
    (dict(kernel=3), "kernel must be 1"),
    (dict(tol=-1.0), "tol must be non-negative"),
    (dict(tol=float("nan")), "tol must be non-negative"),
    (dict(R=0), "R .* must be 1 .. 8"),
    (dict(R=9), "R .* must be 1 .. 8"),
    (dict(directions=[1, 0, 0, 0]), "a direction must be"),
    (dict(directions=[2, 0, 0, 1]), "a direction must be"),
    (dict(directions=[1, 0, 1, -2]), "a direction must be"),
    (dict(weights=[1.0, -0.5]), "a weight must be finite and non-negative"),
    (dict(weights=[float("inf"), 1.0]), "a weight must be finite and non-negative"),
    (dict(weights=[1.0, float("nan")]), "a weight must be finite and non-negative"),
    (dict(null=("unary",)), "must not be NULL"),
    (dict(null=("positions",)), "must not be NULL"),
    (dict(null=("directions",)), "must not be NULL"),
    (dict(null=("weights",)), "must not be NULL"),
    (dict(null=("labels",)), "must not be NULL"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_of_both_entries(change, message, device):
    import re
    rc, text = raw_call(device, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_scanline_aggregate_device:" if device else "stereo_scanline_aggregate:")
    assert "no HIP device" not in text


def test_refusals_of_one_entry_only():
    rc, text = raw_call(True, null=("S",))
    assert rc != 0 and "S and labels must not be NULL" in text
    for change, message in ((dict(unary=[0.0] * 11 + [float("nan")]), "unary must be finite"),
                            (dict(unary=[float("inf")] + [0.0] * 11), "unary must be finite"),
                            (dict(positions=[0.0, float("-inf")]), "positions must be finite")):
        rc, text = raw_call(False, **change)
        assert rc != 0 and message in text and "no HIP device" not in text, text


def test_refusals_reach_python_as_StereoHipError():
    from stereo_amd import StereoHipError, scanline
    u = np.zeros((2, 6))
    assert scanline.max_labels() == 256
    assert scanline.DIRECTIONS_8[:4] == scanline.DIRECTIONS_4 and len(set(scanline.DIRECTIONS_8)) == 8
    with pytest.raises(StereoHipError, match="a direction must be"):
        scanline.aggregate(u, (2, 3), [0.0, 1.0], 1, 1.0, [(0, 0)])
    with pytest.raises(StereoHipError, match="a weight must be"):
        scanline.aggregate(u, (2, 3), [0.0, 1.0], 1, 1.0, [(0, 1)], [-1.0])
    with pytest.raises(StereoHipError, match="kernel must be 1"):
        scanline.aggregate(u, (2, 3), [0.0, 1.0], 5, 1.0)
    with pytest.raises(StereoHipError, match="R .* must be 1 .. 8"):
        scanline.aggregate(u, (2, 3), [0.0, 1.0], 1, 1.0, scanline.DIRECTIONS_8 + ((0, 1),))
    with pytest.raises(StereoHipError, match="unary must be finite"):
        scanline.aggregate(np.full((2, 6), np.nan), (2, 3), [0.0, 1.0], 1, 1.0)
    with pytest.raises(StereoHipError, match="unary must be D x N"):
        scanline.aggregate(u, (3, 3), [0.0, 1.0], 1, 1.0)
    with pytest.raises(StereoHipError, match="2 weights for 1 directions"):
        scanline.aggregate(u, (2, 3), [0.0, 1.0], 1, 1.0, [(0, 1)], [1.0, 1.0])
