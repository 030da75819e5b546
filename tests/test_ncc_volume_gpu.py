"""-m gpu tests of the NCC cost volume on every staged kernel geometry, against the EXACT integer definition
(tests/ncc_exact.py: |value - exact| <= 4 R_ORACLE 2^-52 cond where the value is defined, exactly 0.0 everywhere
else), and checks that need no reference: the three staged paths give the same bits, powers of two scale out bit for
bit.  Then the sampler and winner-takes-all on a label-fastest volume with more than 64 labels, and the per-tap kernel
on fractional disparities at the image's right edge (against the NumPy restatement, 1e-12: linspace steps are not
dyadic, so the exact reference does not apply).

Each instance runs four times: layout 0 (ncc_cross_kernel), layout 1 (ncc_lane_kernel where a 64-label chunk spans at
most 83, else ncc_cross_kernel's LDS transpose), layout 1 with STEREO_HIP_NCC_ROWLANES (always the transpose) and
STEREO_HIP_NCC_NAIVE (ncc_volume_kernel, per tap).  The path and the column count each run is MEANT to take come from
the host rule restated in ncc_exact.host_rule and stand in every assertion message.

Measured on an MI355X (256 compute units), worst |value - exact| / (2^-52 cond) over the instances: lanes, cross
layout 0 and cross layout 1 0.692 (the same bits), per-tap 0.684; the bound is 4 R_ORACLE = 2.66."""
import numpy as np
import pytest

import ncc_exact as nx
from oracle import terms as ot

pytestmark = pytest.mark.gpu

WORST = {}   # path -> (ratio, cond, instance)


@pytest.fixture(scope="module")
def cus(hip):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def matrix(cus):
    return nx.instances(cus)


def _hwd(lf, H, W):
    """label-fastest (D, N) volume, pixel index col * H + row -> (H, W, D)"""
    lf = np.asarray(lf)
    return lf.T.reshape(W, H, lf.shape[0]).transpose(1, 0, 2)


def _four_runs(st, monkeypatch, im0, im1, disps):
    """-> {run: (H, W, D) volume}"""
    H, W, _ = im0.shape
    out = {"layout 0": np.asarray(st.ncc_volume(im0, im1, disps)),
           "layout 1": _hwd(st.ncc_volume(im0, im1, disps, layout=1), H, W)}
    with monkeypatch.context() as m:
        m.setenv("STEREO_HIP_NCC_ROWLANES", "1")
        out["layout 1 rowlanes"] = _hwd(st.ncc_volume(im0, im1, disps, layout=1), H, W)
    with monkeypatch.context() as m:
        m.setenv("STEREO_HIP_NCC_NAIVE", "1")
        out["naive"] = np.asarray(st.ncc_volume(im0, im1, disps))
    return out


def _rules(H, W, disps, cus):
    rules = {"layout 0": nx.host_rule(H, W, disps, cus, 0), "layout 1": nx.host_rule(H, W, disps, cus, 1),
             "layout 1 rowlanes": nx.host_rule(H, W, disps, cus, 1, rowlanes=True),
             "naive": nx.host_rule(H, W, disps, cus, 0, naive=True)}
    # the library's own rule with the device's compute-unit count says the same: "meant for" is what runs
    ask = nx.library_rule()
    own = {"layout 0": ask(H, W, disps, cus, 0), "layout 1": ask(H, W, disps, cus, 1),
           "layout 1 rowlanes": ask(H, W, disps, cus, 1, rowlanes=True), "naive": ask(H, W, disps, cus, 0, naive=True)}
    assert own == rules, "%dx%d D=%d, %d compute units: the library's rule gives %s, the restatement %s" % (
        H, W, len(disps), cus, own, rules)
    return rules


def _path_name(run, rule):
    if rule[0] == "cross":
        return "cross layout %s" % run.split()[1]
    return rule[0]


@pytest.mark.parametrize("name", nx.INSTANCE_NAMES)
def test_volume_against_exact_on_every_geometry(name, matrix, cus, hip, monkeypatch):
    from stereo_amd import terms as st
    inst = matrix[name]
    im0, im1, disps = inst["im0"], inst["im1"], inst["disps"]
    H, W, _ = im0.shape
    ex = nx.exact_ncc(im0, im1, disps)
    rules = _rules(H, W, disps, cus)
    assert rules["layout 1"] == inst["lanes"]
    runs = _four_runs(st, monkeypatch, im0, im1, disps)
    for run, got in runs.items():
        what = "%s %dx%d D=%d, %s, meant for %s cols %s" % (name, H, W, len(disps), run, rules[run][0], rules[run][1])
        worst, cond = nx.check_against_exact(got, ex, nx.C_DEVICE, what)
        print("%s: %.4f 2^-52 cond (largest cond %.4g)" % (what, worst, cond))
        path = _path_name(run, rules[run])
        if worst >= WORST.get(path, (-1.0,))[0]:
            WORST[path] = (worst, cond, name)
    # the three staged runs keep one association (ncc_volume.hip, comment above ncc_lane_kernel): the same bits
    for run in ("layout 1", "layout 1 rowlanes"):
        diff = np.argwhere(runs[run] != runs["layout 0"])
        assert diff.size == 0, "%s: %s (%s cols %s) differs from layout 0 (cross) in %d values, first at (row, col, i) = %s: %r against %r" % (
            name, run, rules[run][0], rules[run][1], len(diff), tuple(diff[0]), runs[run][tuple(diff[0])], runs["layout 0"][tuple(diff[0])])
    # the true disparity's slice is 1 in the interior: the exact reference says so, the device within its bound
    m = nx.true_shift_interior(ex, disps, inst["shift"], W)
    assert np.all(ex["value"][m] == 1)
    if m.any():
        assert np.max(np.abs(runs["layout 1"][m] - 1)) <= nx.C_DEVICE * nx.EPS * ex["cond"][m].max()


def test_worst_ratios_per_path():
    """Reports what the matrix measured (run the file as a whole): the figures DESIGN section 6 records."""
    for path in sorted(WORST):
        print("worst ratio, %s: %.4f 2^-52 cond on %s (largest cond of that instance %.4g); bound %.3f" % (
            (path,) + (WORST[path][0], WORST[path][2], WORST[path][1]) + (nx.C_DEVICE,)))
    for path, (worst, _, name) in WORST.items():
        assert worst <= nx.C_DEVICE, (path, name)


# ---- no reference at all: powers of two scale out, bit for bit
def _scaling_cases(matrix):
    raw0, raw1 = nx.textured(61, 13, 80, 30, raw=True)
    frac0, frac1 = nx.textured(62, 11, 23, 3, raw=True)
    t = matrix["two-chunks"]; c = matrix["cross-ragged"]; s = matrix["cross-stride2"]
    return [("lanes", t["im0"], t["im1"], t["disps"], 1), ("lanes, non-integer image", raw0, raw1, nx.TWO_CHUNKS, 1),
            ("cross layout 0", c["im0"], c["im1"], c["disps"], 0), ("cross layout 1", s["im0"], s["im1"], s["disps"], 1),
            ("per-tap, non-integer image, fractional disparities", frac0, frac1, np.array([0.0, 1.5, 2.25, 3.0, 21.5, 22.75]), 0),
            ("per-tap, layout 1", frac0, frac1, np.array([0.3, 3.0, 20.5]), 1)]


@pytest.mark.parametrize("case", range(6))
def test_power_of_two_scaling_is_bit_exact(case, matrix, cus, hip):
    """Nothing in the definition is absolute, and a power of two commutes with every rounding (no value here comes near
    the ends of the exponent range): ncc_volume(s im0, t im1) == ncc_volume(im0, im1)."""
    from stereo_amd import terms as st
    what, im0, im1, disps, layout = _scaling_cases(matrix)[case]
    H, W, _ = im0.shape
    rule = nx.host_rule(H, W, disps, cus, layout)
    assert rule[0] == what.split(",")[0].split(" layout")[0], (what, rule)
    base = np.asarray(st.ncc_volume(im0, im1, disps, layout=layout))
    assert np.max(np.abs(base)) > 0.5
    for s, t in ((2.0, 2.0), (0.5, 4.0), (4.0, 0.25)):
        got = np.asarray(st.ncc_volume(s * im0, t * im1, disps, layout=layout))
        diff = np.argwhere(got != base)
        assert diff.size == 0, "%s (%s cols %s), images scaled by %g and %g: %d values differ, first at %s: %r against %r" % (
            what, rule[0], rule[1], s, t, len(diff), tuple(diff[0]), got[tuple(diff[0])], base[tuple(diff[0])])


# ---- sampler and winner-takes-all on a label-fastest volume with more than one 64-label chunk
def test_sampler_and_wta_on_label_fastest_volume_of_70_labels(hip):
    from stereo_amd import terms as st
    H, W, D = 13, 21, 70
    rng = np.random.default_rng(17)
    disps = np.arange(D, dtype=np.float64)
    ncc = rng.uniform(-1, 1, size=(H, W, D))
    lf = np.asfortranarray(ncc.reshape(H * W, D, order="F").T)       # (D, N), pixel index col * H + row
    assert np.array_equal(_hwd(lf, H, W), ncc)
    pts = ot.get_points(H, W)
    for trial in range(3):
        P = np.zeros((4, H * W)); P[2] = 1.0
        P[0] = rng.normal() * 0.05
        P[3] = -rng.uniform(-1, disps.max() + 1, H * W)
        if trial == 0:
            P[0] = 0; P[3] = -np.round(rng.uniform(0, disps.max(), H * W))   # exactly on samples / ties
        want_u = ot.ncc_unary_cost(ncc, disps, 40.0, P, pts)
        assert np.array_equal(want_u, st.ncc_unary(lf, disps, 40.0, P, layout=1, shape=(H, W))), "trial %d" % trial
        assert np.array_equal(want_u, st.ncc_unary(np.asfortranarray(ncc), disps, 40.0, P)), "trial %d, layout 0" % trial
    wb = ot.best_disp_from_ncc(ncc, disps)
    gb = st.ncc_best_disp(lf, disps, layout=1, shape=(H, W))
    assert gb.shape == (H, W)
    assert np.array_equal(np.nan_to_num(wb, nan=-7.0), np.nan_to_num(gb, nan=-7.0))
    assert len(np.unique(np.argmax(ncc, axis=2) // 64)) == 2         # winners in both 64-label chunks


# ---- fractional disparities at the edges: per-tap kernel against the restatement
@pytest.mark.parametrize("disps", [[10.25, 10.5, 11.0, 11.75], [0.5, 1.5, 2.5], [12.0, 13.5], [9.25, 9.5, 10.0]],
                         ids=["one-column", "half-steps", "beyond-W", "two-columns"])
def test_fractional_disparities_at_the_edges(disps, cus, hip):
    """(9, 12) image.  [10.25 .. 11.75]: the shifted image fills one column (linspace of one sample) or none;
    [9.25 ..]: two; [0.5, 1.5, 2.5]: MATLAB's round goes half away from zero in the mask, ceil in the fill;
    [12, 13.5]: d >= W, both sides all zero."""
    from stereo_amd import terms as st
    H, W = 9, 12
    im0, im1 = nx.textured(71, H, W, 1)
    disps = np.asarray(disps, np.float64)
    assert nx.host_rule(H, W, disps, cus, 0)[0] == "per-tap"
    want = ot.compute_ncc(im0, im1, disps)
    got = np.asarray(st.ncc_volume(im0, im1, disps))
    lf = _hwd(st.ncc_volume(im0, im1, disps, layout=1), H, W)
    assert got.shape == want.shape
    err = np.abs(got - want)
    k = np.unravel_index(np.argmax(err), err.shape)
    assert err[k] < 1e-12, "disparity %g at (row, col) = (%d, %d): device %r, restatement %r" % (disps[k[2]], k[0], k[1], got[k], want[k])
    assert np.array_equal(lf, got)
    for i, d in enumerate(disps):
        first = int(np.floor(d + 1 + 0.5)) - 1        # 0-based first live column: round(d + 1), half away from zero
        assert np.all(got[:, :first, i] == 0.0), "disparity %g: masked columns" % d
        if np.ceil(d + 1) > W:                        # no column is filled
            assert np.all(want[:, :, i] == 0.0) and np.all(got[:, :, i] == 0.0), "disparity %g: nothing is filled" % d
    if np.ceil(disps.min() + 1) <= W:
        assert np.any(want != 0.0)                    # the case is not trivially zero
