"""The NumPy restatement of the NCC volume (oracle/terms.compute_ncc) against the exact integer definition
(tests/ncc_exact.py) on every instance of the geometry matrix, with 256 compute units substituted for the widths; the
conditions the instances themselves must meet; the host rule's restatement on the geometries the matrix is built for;
the library's own rule (stereo_ncc_volume_rule, host only) against that restatement, on the matrix and on a sweep of
the rule's boundaries, and under sanitizers as a stand-alone program."""
import itertools

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


# ---------------------------------------------------------------- the library's rule against the restatement

PATHS = nx.PATHS


@pytest.fixture(scope="module")
def library_rule():
    return nx.library_rule()


FOUR_RUNS = {"layout 0": (0, {}), "layout 1": (1, {}), "layout 1 rowlanes": (1, dict(rowlanes=True)),
             "naive": (0, dict(naive=True))}


@pytest.mark.parametrize("cus", [1, 64, 256, 304])
def test_library_rule_on_the_geometry_matrix(cus, library_rule):
    # (one compute unit: the widths that follow the count fall below the disparities, the cases turn per-tap)
    for name, inst in nx.instances(cus, meant=cus >= 64).items():
        H, W, _ = inst["im0"].shape
        for run, (layout, kw) in FOUR_RUNS.items():
            want = nx.host_rule(H, W, inst["disps"], cus, layout, **kw)
            got = library_rule(H, W, inst["disps"], cus, layout, **kw)
            assert got == want, "%s (%d compute units), %s: the library's rule gives %s, the restatement %s" % (
                name, cus, run, got, want)
        path, cols, chunks, span = library_rule.full(H, W, inst["disps"], cus, 1)
        if path == "lanes":
            assert span == nx.chunk_span(inst["disps"]) and chunks == -(-W // cols), (name, cus)


def _spanning(D, span):
    """D integer disparities whose 64-label chunks span `span` at most and the last chunk of more than one label
    exactly (where the last chunk is one label, the chunk before it)."""
    d = np.array([(i % 64) % (span + 1) for i in range(D)], np.float64)
    last = (D - 1) // 64 * 64
    if D - last > 1:
        d[D - 1] = span
    elif last > 0:
        d[last - 1] = span
    return d


def test_library_rule_on_a_boundary_sweep(library_rule):
    """W 1 .. 200 (below the largest disparity too: those are per-tap), H and the compute units around the row tile
    and the 2-workgroups-per-unit target, D around the 64-label chunk, spans around 83 = 96 - 5 - 8; then one vector
    each with a fraction, a negative value, a value equal to W and a NaN; the two switches alone and together."""
    n = 0
    seen = set()
    vectors = [(D, span, _spanning(D, span)) for D in (63, 64, 65, 128, 129) for span in (81, 82, 83, 84, 85)]
    vectors.append((1, 0, _spanning(1, 0)))
    shapes = list(itertools.product((1, 11, 12, 13, 24, 25), (1, 8, 256, 1024)))      # (H, compute units)

    def compare(H, W, d, cus, layout, **kw):
        want = nx.host_rule(H, W, d, cus, layout, **kw)
        got = library_rule(H, W, d, cus, layout, **kw)
        assert got == want, "H %d W %d D %d span %d, %d compute units, layout %d %s: library %s, restatement %s" % (
            H, W, len(d), nx.chunk_span(d), cus, layout, kw, got, want)
        seen.add(got)

    for v, (D, span, d) in enumerate(vectors):
        assert nx.chunk_span(d) == span
        for W in range(1, 201):
            # every width for every vector in the label-fastest layout, the 24 shapes taken in turn (each vector starts
            # elsewhere); every shape at the widths around what the vector needs and at the two ends
            near = W in (1, span, span + 1, span + 2, 200)
            for H, cus in (shapes if near else [shapes[(W + 5 * v) % len(shapes)]]):
                compare(H, W, d, cus, 1)
                n += 1
                if near and H == 13:     # the other three runs, and the two switches together
                    compare(H, W, d, cus, 0)
                    compare(H, W, d, cus, 1, rowlanes=True)
                    compare(H, W, d, cus, 0, naive=True)
                    compare(H, W, d, cus, 1, rowlanes=True, naive=True)
                    n += 4
    for H, W, cus in itertools.product((1, 13), (40, 41), (1, 256)):
        for bad in (0.5, -1.0, 40.0, float("nan")):
            for D, at in ((1, 0), (65, 0), (65, 64)):
                d = _spanning(D, 0)
                d[at] = bad
                for naive, rowlanes, layout in itertools.product((False, True), (False, True), (0, 1)):
                    want = nx.host_rule(H, W, d, cus, layout, rowlanes=rowlanes, naive=naive)
                    assert library_rule(H, W, d, cus, layout, rowlanes=rowlanes, naive=naive) == want, (H, W, cus, bad, D, at, naive, rowlanes, layout)
                    assert want[0] == "per-tap" or (bad == 40.0 and W == 41 and not naive)
                    n += 1
    print("%d calls; answers seen: %s" % (n, sorted(seen, key=str)))
    assert {s[0] for s in seen} == set(PATHS)
    assert {8, 9, 10, 31} <= {s[1] for s in seen if s[0] == "lanes"}


def test_ncc_rule_is_clean_under_sanitizers(tmp_path):
    """tools/sanitize_ncc_rule.cpp: the rule on the same boundaries under ASan + UBSan, a stand-alone program."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = str(tmp_path / "sanitize_ncc_rule")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(root, "include"), "-w", os.path.join(root, "tools", "sanitize_ncc_rule.cpp"),
           os.path.join(root, "stereo_amd", "csrc", "ncc_rule.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_NCC_RULE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
