"""The NumPy restatement of the NCC volume (oracle/terms.compute_ncc) against the exact integer definition
(tests/ncc_exact.py) on every instance of the geometry matrix, with 256 compute units substituted for the widths; the
conditions the instances themselves must meet; the host rule's restatement on the geometries the matrix is built for."""
import numpy as np
import pytest

import ncc_exact as nx
from oracle import terms as ot

CUS = 256


@pytest.fixture(scope="module")
def matrix():
    return nx.instances(CUS)


@pytest.fixture(scope="module")
def measured():
    return {}


@pytest.mark.parametrize("name", nx.INSTANCE_NAMES)
def test_restatement_against_exact(name, matrix, measured):
    inst = matrix[name]
    H, W, _ = inst["im0"].shape
    ex = nx.exact_ncc(inst["im0"], inst["im1"], inst["disps"])
    want = ot.compute_ncc(inst["im0"], inst["im1"], inst["disps"])
    live, defined = ex["live"], ex["defined"]
    und = live & ~defined
    # live pixels with a zero variance term: the restatement is exactly 0.0 there, and they stay a minority
    assert np.all(want[und] == 0.0), "%s: restatement not exactly 0 at %d live pixels with a zero variance term" % (name, np.sum(want[und] != 0))
    assert und.sum() <= 0.2 * live.sum(), "%s: %d of %d live pixels have a zero variance term" % (name, und.sum(), live.sum())
    assert np.all(want[~live] == 0.0)
    worst, cond = nx.check_against_exact(want, ex, nx.R_ORACLE, name + " (restatement)")
    measured[name] = (worst, cond, int(und.sum()), int(live.sum()))
    print("%s: %s, restatement %.4f 2^-52 cond, largest cond %.4g, %d of %d live pixels undefined" % (
        name, inst["lanes"], worst, cond, und.sum(), live.sum()))
    # the true disparity's slice is 1 on the interior: said by the exact reference, not assumed
    m = nx.true_shift_interior(ex, inst["disps"], inst["shift"], W)
    assert np.all(ex["value"][m] == 1)
    if not name.startswith("tiny") or name == "tiny-6x7":
        assert m.any(), "%s: no interior pixel at the true disparity" % name
    assert defined.any()
    assert np.all(np.abs(ex["value"]) <= 1)
    assert np.all(ex["cond"][defined] * (1 + 1e-12) >= 2 + np.abs(ex["value"][defined]).astype(np.float64))


def test_r_oracle_is_the_measured_maximum(matrix, measured):
    """R_ORACLE is a measurement, not a tolerance with slack of its own: the constant is the largest ratio over the
    matrix, rounded up in the third digit."""
    for name in nx.INSTANCE_NAMES:
        if name not in measured:
            inst = matrix[name]
            ex = nx.exact_ncc(inst["im0"], inst["im1"], inst["disps"])
            rt = nx.ratio(ot.compute_ncc(inst["im0"], inst["im1"], inst["disps"]), ex)
            measured[name] = (float(rt.max()), float(ex["cond"].max()), 0, 0)
    worst = max(v[0] for v in measured.values())
    print("R_ORACLE %.4f, measured %.4f, largest cond %.4g" % (nx.R_ORACLE, worst, max(v[1] for v in measured.values())))
    assert worst <= nx.R_ORACLE
    assert worst >= 0.9 * nx.R_ORACLE, "R_ORACLE %.4f is no longer the measured figure %.4f" % (nx.R_ORACLE, worst)
    assert nx.C_DEVICE == 4 * nx.R_ORACLE


def test_matrix_reaches_the_geometries_it_is_built_for(matrix):
    geo = {name: inst["lanes"] for name, inst in matrix.items()}
    assert geo["span82"] == ("lanes", 9) and geo["span83"] == ("lanes", 8) and geo["span83-base3"] == ("lanes", 8)
    assert geo["span84"] == ("cross", None) and geo["cross-stride2"] == ("cross", None)
    assert geo["cols31"] == ("lanes", 31) and geo["cols10"] == ("lanes", 10)
    # cols + span = 91: the last product of the last column pair reads element 95 of the 96-element segment
    assert 9 + nx.chunk_span([0, 82]) == nx.SEG1 - 5
    d = matrix["two-chunks"]["disps"]
    assert len(d) == 70 and sorted(d[:64]) == list(range(64)) and list(d[:64]) != sorted(d[:64]) and d[0] != 0
    assert nx.host_rule(13, 80, d, CUS, 0) == ("cross", None)
    assert nx.host_rule(13, 80, d, CUS, 1, rowlanes=True) == ("cross", None)
    assert nx.host_rule(13, 80, d, CUS, 1, naive=True) == ("per-tap", None)
    assert nx.host_rule(9, 12, [0.5, 1.5], CUS, 1) == ("per-tap", None)
    assert nx.host_rule(9, 12, [12.0], CUS, 1) == ("per-tap", None)


def test_exact_reference_on_a_hand_computed_window():
    """One pixel by hand (Python integers and fractions): a 5 x 5 image is one full window at its centre."""
    from fractions import Fraction
    import math
    rng = np.random.default_rng(1)
    im0 = rng.integers(0, 256, size=(5, 5, 3)).astype(np.float64)
    im1 = rng.integers(0, 256, size=(5, 5, 3)).astype(np.float64)
    ex = nx.exact_ncc(im0, im1, [0, 1])
    for i, d in enumerate((0, 1)):
        a = [int(v) for v in im0.reshape(-1)]
        b3 = np.zeros((5, 5, 3)); b3[:, d:] = im1[:, :5 - d]
        b = [int(v) for v in b3.reshape(-1)]
        Sa, Sb = sum(a), sum(b)
        V0 = 75 * sum(v * v for v in a) - Sa * Sa
        VT = 75 * sum(v * v for v in b) - Sb * Sb
        N = 75 * sum(x * y for x, y in zip(a, b)) - Sa * Sb
        got = ex["value"][2, 2, i]
        # N / sqrt(V0 VT) squared is the fraction N^2 / (V0 VT)
        assert abs(Fraction(float(got)) ** 2 - Fraction(N * N, V0 * VT)) < Fraction(1, 10 ** 15)
        assert (float(got) > 0) == (N > 0)
        assert math.isqrt(V0 * VT) <= 3.7e8
        assert ex["defined"][2, 2, i] and ex["cond"][2, 2, i] >= 2 + abs(float(got))
    assert not ex["live"][:, 0, 1].any() and np.all(ex["value"][:, 0, 1] == 0)
