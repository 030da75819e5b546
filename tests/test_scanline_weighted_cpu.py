"""Weighted scanline aggregation and the contrast rule without a device: the NumPy restatement
(tests/scanline_weighted_restate.py) against the first-principles dynamic programme (first_principles.chain_dp) with
zero tolerance and against the two existing restatements bit for bit; the properties of the contrast restatement
(tests/contrast_restate.py); every refusal of the six new C entries, which come before the device is looked for; the ABI
version.

Why zero tolerance: first_principles.dyadic_problem keeps unaries on multiples of 2^-6, positions of 2^-2, weights in
{0, 1/4, 1/2, 1, 2, 4} and tol dyadic or never cutting, so every term is a multiple of 2^-14 below 2^22 and every sum
along a chain of at most 9 pixels is exact in fp64 in whatever order it is formed."""
import ctypes as C
import re

import numpy as np
import pytest

import contrast_restate as CR
import first_principles as fp
import scanline_edges_restate as ER
import scanline_restate as R
import scanline_weighted_restate as WR
from weighted_helpers import AXIS_DIRECTIONS, PARAMS, image, steps_from_edges

K = 4


def chain_subproblem(p, ids):
    """The pixels `ids` (consecutive grid neighbours) of the grid problem `p` as a path problem of first_principles."""
    pos = {int(v): s for s, v in enumerate(ids)}
    rows = [e for e in range(p["conn"].shape[0])
            if int(p["conn"][e, 0]) in pos and int(p["conn"][e, 1]) in pos
            and abs(pos[int(p["conn"][e, 0])] - pos[int(p["conn"][e, 1])]) == 1]
    assert len(rows) == len(ids) - 1
    conn = np.array([[pos[int(a)], pos[int(b)]] for a, b in p["conn"][rows]], dtype=np.int64).reshape(-1, 2)
    return dict(unary=p["unary"][ids], conn=conn, q=p["q"][rows], qprim=p["qprim"][rows], alphas=p["alphas"][rows])


def half_chains(p, kernel, directions):
    shape = (p["H"], p["W"])
    wstep = steps_from_edges(p["conn"].T, p["alphas"], shape, directions)
    return [WR.direction_costs(p["unary"].T, shape, p["positions"], kernel, p["lam"], d, w) for d, w in zip(directions, wstep)]


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_one_chain_min_marginals_equal_first_principles(shape, kernel):
    H, W = shape
    pair = ((0, 1), (0, -1)) if H == 1 else ((1, 0), (-1, 0))
    for seed in range(8):
        p = fp.dyadic_problem(np.random.default_rng([H, W, kernel, seed]), H, W, K, shared=True)
        fwd, bwd = half_chains(p, kernel, pair)
        _, mm = fp.chain_dp(p, kernel, p["lam"])
        assert np.array_equal(((fwd + bwd) - p["unary"].T).T, mm), seed


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (7, 5)], ids=lambda s: "%dx%d" % s)
def test_every_row_and_column_chain_equals_first_principles(shape, kernel):
    H, W = shape
    for seed in range(4):
        p = fp.dyadic_problem(np.random.default_rng([H, W, kernel, seed]), H, W, K, shared=True)
        right, left, down, up = half_chains(p, kernel, AXIS_DIRECTIONS)
        rows = ((right + left) - p["unary"].T).T
        cols = ((down + up) - p["unary"].T).T
        for y in range(H):
            ids = [x * H + y for x in range(W)]
            _, mm = fp.chain_dp(chain_subproblem(p, ids), kernel, p["lam"])
            assert np.array_equal(rows[ids], mm), (seed, "row", y)
        for x in range(W):
            ids = [x * H + y for y in range(H)]
            _, mm = fp.chain_dp(chain_subproblem(p, ids), kernel, p["lam"])
            assert np.array_equal(cols[ids], mm), (seed, "column", x)


@pytest.mark.parametrize("kernel", [1, 2])
def test_constant_step_weights_are_the_unweighted_restatement(kernel):
    rng = np.random.default_rng([12, kernel])
    H, W, D = 5, 7, 6
    unary, positions = rng.random((D, H * W)) * 3.0, rng.random(D) * 7.0
    weights = rng.random(8) * 2.0
    weights[3] = 0.0
    want = R.aggregate(unary, (H, W), positions, kernel, 2.5, R.DIRECTIONS_8, weights)
    got = WR.aggregate(unary, (H, W), positions, kernel, 2.5, np.tile(weights[:, None], (1, H * W)), R.DIRECTIONS_8)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("labels", range(1, 10))
def test_axis_directions_equal_the_per_edge_restatement(labels, kernel):
    H, W = 4, 5
    p = fp.dyadic_problem(np.random.default_rng([labels, kernel]), H, W, labels, shared=True)
    rng = np.random.default_rng([labels, kernel, 1])
    unary, alphas = rng.random((labels, H * W)), rng.random(p["alphas"].shape[0]) * 2.0      # (not dyadic: bits, not sums)
    positions = p["positions"] + rng.random(labels) * 0.125
    q = np.tile(positions[:, None], (1, alphas.shape[0]))
    want = ER.aggregate(unary, (H, W), p["conn"].T, q, q.copy(), alphas, kernel, 1.75, AXIS_DIRECTIONS)
    wstep = steps_from_edges(p["conn"].T, alphas, (H, W))
    got = WR.aggregate(unary, (H, W), positions, kernel, 1.75, wstep, AXIS_DIRECTIONS)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[3])


# ---------------------------------------------------------------- the contrast restatement

@pytest.mark.parametrize("name", sorted(PARAMS))
def test_contrast_restatement_properties(name):
    par = PARAMS[name]
    w_high, w_low, g0, g1 = par
    rng = np.random.default_rng(5)
    H, W = 5, 6
    for Cn in (1, 3):
        im = image(rng, H, W, Cn, dyadic=False)
        conn = fp.grid_edges(H, W).T
        a = CR.edge_weights(im, conn, par)
        assert np.array_equal(a, CR.edge_weights(im, conn[::-1], par))                       # symmetric in a and b
        assert np.array_equal(CR.edge_weights(np.full((H, W, Cn), 0.375), conn, par), np.full(conn.shape[1], w_high))
        assert np.isfinite(a).all() and (a >= 0).all() and a.min() >= min(w_high, w_low) and a.max() <= max(w_high, w_low)
        # boundary steps are 0.0; an axis step is the matching grid edge's weight
        wstep = CR.step_weights(im, R.DIRECTIONS_8, par)
        for r, (dy, dx) in enumerate(R.DIRECTIONS_8):
            for x in range(W):
                for y in range(H):
                    if not (0 <= y - dy < H and 0 <= x - dx < W):
                        assert wstep[r, x * H + y] == 0.0 and not np.signbit(wstep[r, x * H + y])
        assert np.array_equal(wstep[:4], steps_from_edges(conn, a, (H, W)))
    # exactly w_high at g = g0 and exactly w_low at g = g1, w_high below g0, w_low above g1
    assert CR.ramp(np.array([g0]), *par)[0] == w_high
    assert CR.ramp(np.array([g1]), *par)[0] == (w_high if g0 == g1 else w_low)
    assert CR.ramp(np.array([0.0]), *par)[0] == w_high and CR.ramp(np.array([g1 * 2 + 1]), *par)[0] == w_low
    assert CR.ramp(np.array([np.nextafter(g1, np.inf)]), *par)[0] == w_low


def test_contrast_step_and_midpoint():
    w_high, w_low, g0, _ = PARAMS["step"]
    g = np.array([0.0, g0, np.nextafter(g0, 1.0), 1.0])
    assert CR.ramp(g, *PARAMS["step"]).tolist() == [w_high, w_high, w_low, w_low]
    assert CR.ramp(np.array([0.3125]), *PARAMS["ramp"])[0] == 2.0 + (0.25 - 2.0) * 0.5        # half way, exact
    with pytest.raises(ValueError):
        CR.ramp(g, 1.0, 1.0, 0.5, 0.25)


# ---------------------------------------------------------------- refusals, before the device is looked for

def _arr(keep, null, name, values, dtype):
    if name in null:
        return None
    v = np.array(values, dtype=dtype)
    keep.append(v)
    return v.ctypes.data_as(C.c_void_p)


def _params(values, null):
    from stereo_amd.contrast import _Params
    return None if "params" in null else C.byref(_Params(*values))


def contrast_call(entry, **change):
    """One of the four contrast entries on small host arrays with one argument changed -> (rc, message)."""
    from stereo_amd import _lib
    a = dict(H=2, W=3, C=2, E=2, R=2, conn=[0, 1, 4, 5], directions=[1, 0, 0, -1], params=(1.0, 0.5, 0.1, 0.2),
             im=[0.25] * 12, null=(), alias=None)
    a.update(change)
    keep = []
    err = _lib.errbuf()
    im = _arr(keep, a["null"], "im", a["im"], np.float64)
    head = [im, C.c_int(a["H"]), C.c_int(a["W"]), C.c_int(a["C"])]
    L = _lib.lib()
    if entry.startswith("edge"):
        conn = _arr(keep, a["null"], "conn", a["conn"], np.uint32)
        out = im if a["alias"] == "im" else conn if a["alias"] == "conn" else _arr(keep, a["null"], "alphas", [0.0] * 12, np.float64)
        args = head + [conn, C.c_int64(a["E"]), _params(a["params"], a["null"]), out]
        if entry == "edge_device":
            rc = L.stereo_contrast_edge_weights_device(*args, _arr(keep, a["null"], "bad", [0], np.int32), None, err, C.c_size_t(len(err)))
        else:
            rc = L.stereo_contrast_edge_weights(*args, err, C.c_size_t(len(err)))
    else:
        out = im if a["alias"] == "im" else _arr(keep, a["null"], "wstep", [0.0] * 48, np.float64)
        args = head + [_arr(keep, a["null"], "directions", a["directions"], np.int32), C.c_int(a["R"]),
                       _params(a["params"], a["null"]), out]
        if entry == "step_device":
            rc = L.stereo_contrast_step_weights_device(*args, None, err, C.c_size_t(len(err)))
        else:
            rc = L.stereo_contrast_step_weights(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


CONTRAST_REFUSALS = [
    (dict(H=0), "H, W and C must be at least 1"),
    (dict(W=-1), "H, W and C must be at least 1"),
    (dict(C=0), "H, W and C must be at least 1"),
    (dict(H=1 << 16, W=1 << 15), "below 2\\^31"),
    (dict(null=("im",)), "must not be NULL"),
    (dict(null=("params",)), "must not be NULL"),
    (dict(params=(-1.0, 0.5, 0.1, 0.2)), "finite and non-negative"),
    (dict(params=(1.0, float("nan"), 0.1, 0.2)), "finite and non-negative"),
    (dict(params=(1.0, 0.5, float("inf"), float("inf"))), "finite and non-negative"),
    (dict(params=(1.0, 0.5, 0.1, -0.2)), "finite and non-negative"),
    (dict(params=(1.0, 0.5, 0.3, 0.2)), "g0 must not be above g1"),
    (dict(alias="im"), "must not be"),
]
NAMES = {"edge": "stereo_contrast_edge_weights:", "edge_device": "stereo_contrast_edge_weights_device:",
         "step": "stereo_contrast_step_weights:", "step_device": "stereo_contrast_step_weights_device:"}


@pytest.mark.parametrize("entry", sorted(NAMES))
@pytest.mark.parametrize("change,message", CONTRAST_REFUSALS, ids=[str(i) for i in range(len(CONTRAST_REFUSALS))])
def test_refusals_of_the_four_contrast_entries(change, message, entry):
    rc, text = contrast_call(entry, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith(NAMES[entry]) and "no HIP device" not in text


def test_refusals_of_single_contrast_entries():
    for entry in ("edge", "edge_device"):
        for change, message in ((dict(E=-1), "E must not be negative"), (dict(null=("conn",)), "must not be NULL"),
                                (dict(null=("alphas",)), "must not be NULL"), (dict(alias="conn"), "alphas must not be an input")):
            rc, text = contrast_call(entry, **change)
            assert rc != 0 and message in text and "no HIP device" not in text, text
    rc, text = contrast_call("edge_device", null=("bad",))
    assert rc != 0 and "bad must not be NULL" in text
    for entry in ("step", "step_device"):
        for change, message in ((dict(R=0), "must be 1 .. 8"), (dict(R=9), "must be 1 .. 8"),
                                (dict(directions=[0, 0, 1, 0]), "a direction must be"),
                                (dict(directions=[1, 0, 2, 1]), "a direction must be"),
                                (dict(null=("directions",)), "must not be NULL"), (dict(null=("wstep",)), "must not be NULL")):
            rc, text = contrast_call(entry, **change)
            assert rc != 0 and message in text and "no HIP device" not in text, text
    # on host arrays only: the edge is named; the image must be finite
    rc, text = contrast_call("edge", conn=[0, 1, 4, 6])
    assert rc != 0 and "edge 1 (4, 6) has an endpoint outside 0 .. 5" in text and "no HIP device" not in text
    for entry in ("edge", "step"):
        rc, text = contrast_call(entry, im=[0.25] * 11 + [float("nan")])
        assert rc != 0 and "im must be finite" in text and "no HIP device" not in text


def weighted_call(device, **change):
    """One of the two weighted entries on small host arrays with one argument changed -> (rc, message)."""
    from stereo_amd import _lib
    a = dict(H=2, W=3, D=2, kernel=1, tol=1.0, R=2, directions=[1, 0, 0, -1], step_weights=[0.5] * 12, positions=[0.0, 1.0],
             unary=[0.0] * 12, null=(), alias=None)
    a.update(change)
    keep = []
    err = _lib.errbuf()
    arr = lambda name, values, dtype: _arr(keep, a["null"], name, values, dtype)
    wst = arr("step_weights", a["step_weights"], np.float64)
    unary = arr("unary", a["unary"], np.float64)
    S = wst if a["alias"] == "step_weights" else unary if a["alias"] == "unary" else arr("S", [0.0] * 12, np.float64)
    args = [unary, C.c_int(a["H"]), C.c_int(a["W"]), C.c_int(a["D"]), arr("positions", a["positions"], np.float64),
            C.c_int(a["kernel"]), C.c_double(a["tol"]), arr("directions", a["directions"], np.int32), wst, C.c_int(a["R"]), S,
            arr("labels", [0] * 6, np.int32), arr("map", [0.0] * 6, np.float64), arr("confidence", [0.0] * 6, np.float64)]
    L = _lib.lib()
    if device:
        rc = L.stereo_scanline_aggregate_weighted_device(*args, None, err, C.c_size_t(len(err)))
    else:
        rc = L.stereo_scanline_aggregate_weighted(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


WEIGHTED_REFUSALS = [
    (dict(H=0), "H and W must be at least 1"),
    (dict(W=-1), "H and W must be at least 1"),
    (dict(H=1 << 16, W=1 << 15), "below 2\\^31"),
    (dict(D=0), "D must be 1 .. 256"),
    (dict(D=257), "D must be 1 .. 256"),
    (dict(kernel=3), "kernel must be 1"),
    (dict(tol=-1.0), "tol must be non-negative"),
    (dict(tol=float("nan")), "tol must be non-negative"),
    (dict(R=0), "R .* must be 1 .. 8"),
    (dict(R=9), "R .* must be 1 .. 8"),
    (dict(directions=[1, 0, 0, 0]), "a direction must be"),
    (dict(null=("unary",)), "must not be NULL"),
    (dict(null=("positions",)), "must not be NULL"),
    (dict(null=("directions",)), "must not be NULL"),
    (dict(null=("step_weights",)), "step_weights.* must not be NULL"),
    (dict(null=("labels",)), "must not be NULL"),
    (dict(alias="unary"), "S must not be unary"),
    (dict(alias="step_weights"), "S must not be step_weights"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,message", WEIGHTED_REFUSALS, ids=[str(i) for i in range(len(WEIGHTED_REFUSALS))])
def test_refusals_of_both_weighted_entries(change, message, device):
    rc, text = weighted_call(device, **change)
    assert rc != 0 and re.search(message, text), text
    assert text.startswith("stereo_scanline_aggregate_weighted_device:" if device else "stereo_scanline_aggregate_weighted:")
    assert "no HIP device" not in text


def test_refusals_of_one_weighted_entry_only():
    rc, text = weighted_call(True, null=("S",))
    assert rc != 0 and "S and labels must not be NULL" in text
    # directions (1, 0), (0, -1) on 2 x 3: pixel 1 has a predecessor along (1, 0), pixel 0 has none
    for bad in (-0.5, float("nan"), float("inf")):
        rc, text = weighted_call(False, step_weights=[0.5, bad] + [0.5] * 10)
        assert rc != 0 and "a step weight must be finite and non-negative (direction 0, pixel 1)" in text, text
        assert "no HIP device" not in text
        rc, text = weighted_call(False, step_weights=[bad] + [0.5] * 11)          # not read: not refused for its value
        assert "a step weight" not in text
    for change, message in ((dict(unary=[0.0] * 11 + [float("nan")]), "unary must be finite"),
                            (dict(positions=[0.0, float("-inf")]), "positions must be finite")):
        rc, text = weighted_call(False, **change)
        assert rc != 0 and message in text and "no HIP device" not in text, text


def test_refusals_reach_python_as_StereoHipError():
    from stereo_amd import Contrast, StereoHipError, contrast, scanline
    u, im = np.zeros((2, 6)), np.zeros((2, 3, 3))
    with pytest.raises(StereoHipError, match="a step weight must be"):
        scanline.aggregate_weighted(u, (2, 3), [0.0, 1.0], 1, 1.0, -np.ones((8, 6)))
    with pytest.raises(StereoHipError, match="step_weights must be R x N"):
        scanline.aggregate_weighted(u, (2, 3), [0.0, 1.0], 1, 1.0, np.ones((4, 6)))
    with pytest.raises(StereoHipError, match="a direction must be"):
        scanline.aggregate_weighted(u, (2, 3), [0.0, 1.0], 1, 1.0, np.ones((1, 6)), [(0, 0)])
    with pytest.raises(StereoHipError, match="g0 must not be above g1"):
        contrast.edge_weights(im, [[0], [1]], Contrast(1.0, 0.5, 0.5, 0.25))
    with pytest.raises(StereoHipError, match="edge 0 \\(0, 6\\) has an endpoint outside"):
        contrast.edge_weights(im, [[0], [6]], Contrast(1.0, 0.5, 0.25, 0.5))
    with pytest.raises(StereoHipError, match="finite and non-negative"):
        contrast.step_weights(im, [(0, 1)], Contrast(-1.0, 0.5, 0.25, 0.5))
    with pytest.raises(StereoHipError, match="im must be finite"):
        contrast.step_weights(np.full((2, 3), np.inf), [(0, 1)], Contrast(1.0, 0.5, 0.25, 0.5))
    with pytest.raises(StereoHipError, match="a Contrast is needed"):
        contrast.step_weights(im, [(0, 1)], (1.0, 0.5, 0.25, 0.5))


def test_abi_version():
    from stereo_amd import _lib
    assert _lib.lib().stereo_hip_abi_version() == 22 and _lib.ABI_VERSION == 22
