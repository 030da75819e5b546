"""Candidate bands without a device: every refusal of the C entries and the Python wrappers (the
arguments are checked before the device is looked for), the ABI numbers, the restatement's own properties
(tests/candidates_restate.py) and the chain of the issue, whose optimum the device test then has to reach."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import band_restate
import candidates_restate as R
import first_principles as fp
from band_restate import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, E = 3, 4, 5, 2
KO, M, T = 3, 2, 2
K = KO + M * T
NEVER = -1e300


def _lib():
    from stereo_amd import _lib as L
    return L.lib()


def _call(fn, *args):
    err = C.create_string_buffer(1024)
    rc = fn(*args, err, C.c_size_t(len(err)))
    return rc, err.value.decode()


def _host():
    """keep-alive arrays and the argument values of a valid call"""
    return dict(ncc=np.zeros(H * W * D), disparities=np.arange(D, dtype=np.float64), base=np.zeros(H * W),
                offsets=np.array([-0.5, 0.0, 0.5]), sources=np.zeros(M * H * W), taps=np.array([0, 1, -1, 0], np.int32),
                cand=np.zeros(K * H * W), conn=np.array([0, 1, 1, 2], np.uint32), unary=np.zeros(K * H * W), q=np.zeros(K * E),
                qprim=np.zeros(K * E), labels=np.ones(H * W, np.int32), out=np.zeros(H * W))


def _p(x):
    return None if x is None else C.c_void_p(x.ctypes.data)


def _gather_args(v, device_form):
    Ko = v["Ko"] if v["Ko"] is not None else (0 if v["offsets"] is None else len(v["offsets"]))
    args = [_p(v["base"]), C.c_int(v["H"]), C.c_int(v["W"]), _p(v["offsets"])]
    if device_form:
        args.append(_p(v["offsets"]))          # (never read: the call is refused before the device is looked for)
    args += [C.c_int(Ko), _p(v["sources"]), C.c_int(v["M"]), _p(v["taps"])]
    if device_form:
        args.append(_p(v["taps"]))
    args += [C.c_int(v["T"]), _p(v["cand"])]
    if device_form:
        args += [None, None]
    return args


def _inputs_args(v, device_form):
    args = [_p(v["ncc"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["D"]), C.c_int(v["layout"]), _p(v["disparities"])]
    if device_form:
        args.append(_p(v["disparities"]))
    args += [C.c_double(1.0), _p(v["cand"]), C.c_int(v["K"]), C.c_int64(v["E"]), _p(v["conn"]), _p(v["unary"]), _p(v["q"]),
             _p(v["qprim"])]
    if device_form:
        args += [None, None]
    return args


def _apply_args(v, device_form):
    args = [_p(v["cand"]), C.c_int(v["H"]), C.c_int(v["W"]), C.c_int(v["K"]), _p(v["labels"]), _p(v["out"])]
    if device_form:
        args += [None, None]
    return args


SIZE_REFUSALS = [
    (dict(H=0), "H and W"),
    (dict(W=0), "H and W"),
    (dict(W=-2), "H and W"),
    (dict(H=1 << 16, W=1 << 15), r"2\^31"),
]
GATHER_REFUSALS = SIZE_REFUSALS + [
    (dict(offsets=np.array([-0.5, np.nan, 0.0])), "not finite"),
    (dict(offsets=np.array([0.0, np.inf])), "not finite"),
    (dict(offsets=np.array([0.0, 0.5, 0.5])), "strictly ascending"),
    (dict(offsets=np.array([0.5, 0.0])), "strictly ascending"),
    (dict(offsets=np.array([-0.5, 0.25, 0.5])), r"contain 0\.0"),
    (dict(offsets=np.zeros(0), Ko=0), r"1 \.\. 512"),
    (dict(offsets=np.arange(513, dtype=np.float64), Ko=513), r"1 \.\. 512"),
    (dict(Ko=-1), r"1 \.\. 512"),
    (dict(offsets=None, Ko=3), "offsets must not be NULL"),
    (dict(base=None), "NULL"),
    (dict(cand=None), "NULL"),
    (dict(M=-1), "M and T must not be negative"),
    (dict(T=-1), "M and T must not be negative"),
    (dict(sources=None), "sources and taps must not be NULL"),
    (dict(taps=None), "sources and taps must not be NULL"),
    (dict(offsets=np.arange(-255.0, 255.0), M=1, T=3, taps=np.zeros(6, np.int32)), r"K = Ko \+ M \* T must be 1 \.\. 512 \(got 513\)"),
    (dict(M=1 << 20, T=1 << 20), r"1 \.\. 512"),
    (dict(taps=np.array([0, 1, 1 << 15, 0], np.int32)), r"tap 1 has \|dy\| or \|dx\| of 2\^15 or more"),
    (dict(taps=np.array([0, -(1 << 15), 0, 0], np.int32)), r"tap 0 has \|dy\| or \|dx\| of 2\^15 or more"),
]
INPUT_REFUSALS = SIZE_REFUSALS + [
    (dict(layout=2), "layout"),
    (dict(layout=-1), "layout"),
    (dict(D=0), "D must be"),
    (dict(E=-1), "E must not"),
    (dict(K=0), r"1 \.\. 512"),
    (dict(K=513), r"1 \.\. 512"),
    (dict(K=-3), r"1 \.\. 512"),
    (dict(ncc=None), "NULL"),
    (dict(disparities=None), "NULL"),
    (dict(cand=None), "NULL"),
    (dict(unary=None), "NULL"),
    (dict(conn=None), "NULL"),
    (dict(q=None), "NULL"),
    (dict(qprim=None), "NULL"),
]
APPLY_REFUSALS = SIZE_REFUSALS + [
    (dict(K=0), r"1 \.\. 512"),
    (dict(K=513), r"1 \.\. 512"),
    (dict(cand=None), "NULL"),
    (dict(labels=None), "NULL"),
    (dict(out=None), "NULL"),
]
_ids = lambda c: None if isinstance(c, str) else ",".join(sorted(c))


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,match", GATHER_REFUSALS, ids=_ids)
def test_gather_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, Ko=None, M=M, T=T)
    v.update(change)
    fn = _lib().stereo_candidates_gather_device if device_form else _lib().stereo_candidates_gather
    rc, msg = _call(fn, *_gather_args(v, device_form))
    assert rc != 0 and re.search(match, msg), msg
    assert msg.startswith("stereo_candidates_gather_device" if device_form else "stereo_candidates_gather:")


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,match", INPUT_REFUSALS, ids=_ids)
def test_inputs_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, D=D, layout=0, K=K, E=E)
    v.update(change)
    fn = _lib().stereo_candidates_inputs_device if device_form else _lib().stereo_candidates_inputs
    rc, msg = _call(fn, *_inputs_args(v, device_form))
    assert rc != 0 and re.search(match, msg), msg
    assert msg.startswith("stereo_candidates_inputs_device" if device_form else "stereo_candidates_inputs:")


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("change,match", APPLY_REFUSALS, ids=_ids)
def test_apply_refusals(device_form, change, match):
    v = dict(_host(), H=H, W=W, K=K)
    v.update(change)
    fn = _lib().stereo_candidates_apply_device if device_form else _lib().stereo_candidates_apply
    rc, msg = _call(fn, *_apply_args(v, device_form))
    assert rc != 0 and re.search(match, msg), msg
    assert msg.startswith("stereo_candidates_apply_device" if device_form else "stereo_candidates_apply:")


def test_without_sources_or_taps_the_two_may_be_null():
    """M * T == 0 is the band's table: NULL sources and taps pass the checks (the call then stops at the device, or runs)"""
    for m, t in ((0, 0), (0, 2), (2, 0)):
        v = dict(_host(), H=H, W=W, Ko=None, M=m, T=t, sources=None, taps=None)
        rc, msg = _call(_lib().stereo_candidates_gather, *_gather_args(v, False))
        assert rc == 0 or "no HIP device" in msg, msg


def test_device_forms_want_the_device_copies_of_the_short_vectors():
    v = dict(_host(), H=H, W=W, Ko=None, M=M, T=T)
    args = _gather_args(v, True)
    args[4] = None
    rc, msg = _call(_lib().stereo_candidates_gather_device, *args)
    assert rc != 0 and "d_offsets" in msg
    args = _gather_args(v, True)
    args[9] = None
    rc, msg = _call(_lib().stereo_candidates_gather_device, *args)
    assert rc != 0 and "d_taps" in msg
    args = _inputs_args(dict(_host(), H=H, W=W, D=D, layout=0, K=K, E=E), True)
    args[6] = None
    rc, msg = _call(_lib().stereo_candidates_inputs_device, *args)
    assert rc != 0 and "d_disparities" in msg


def test_host_entries_refuse_values_that_are_not_finite_and_name_the_pixel_and_the_label():
    for bad in (np.nan, np.inf, -np.inf):
        a = _host()
        a["base"][1 + H * 2] = bad                       # row 1, column 2
        rc, msg = _call(_lib().stereo_candidates_gather, *_gather_args(dict(a, H=H, W=W, Ko=None, M=M, T=T), False))
        assert rc != 0 and "base is not finite" in msg and "row 1, column 2" in msg, msg
        a = _host()
        a["sources"][H * W + 2 + H * 3] = bad            # source 1, row 2, column 3
        rc, msg = _call(_lib().stereo_candidates_gather, *_gather_args(dict(a, H=H, W=W, Ko=None, M=M, T=T), False))
        assert rc != 0 and "source 1 is not finite" in msg and "row 2, column 3" in msg, msg
        a = _host()
        a["cand"][K * (1 + H * 2) + 4] = bad             # row 1, column 2, label 5
        rc, msg = _call(_lib().stereo_candidates_inputs, *_inputs_args(dict(a, H=H, W=W, D=D, layout=0, K=K, E=E), False))
        assert rc != 0 and "row 1, column 2" in msg and "label 5" in msg, msg
        rc, msg = _call(_lib().stereo_candidates_apply, *_apply_args(dict(a, H=H, W=W, K=K), False))
        assert rc != 0 and "row 1, column 2" in msg and "label 5" in msg, msg


def test_host_entries_refuse_labels_and_edges_out_of_range():
    for lab in (0, K + 1, -1):
        a = _host()
        a["labels"][5] = lab
        rc, msg = _call(_lib().stereo_candidates_apply, *_apply_args(dict(a, H=H, W=W, K=K), False))
        assert rc != 0 and "outside 1 .. %d" % K in msg and "pixel 5" in msg, msg
    a = _host()
    a["conn"][3] = H * W
    rc, msg = _call(_lib().stereo_candidates_inputs, *_inputs_args(dict(a, H=H, W=W, D=D, layout=0, K=K, E=E), False))
    assert rc != 0 and "conn" in msg and "edge 1" in msg, msg


def test_python_wrappers_refuse_before_the_device():
    import stereo_amd
    from stereo_amd import StereoHipError, candidates, pyramid
    from stereo_amd import terms as Tm
    ncc, disp, base = np.zeros((H, W, D)), np.arange(D, dtype=np.float64), np.zeros((H, W))
    conn = Tm.construct_neighborhood(H, W)
    for offsets, match in (([0.0, 0.0], "strictly ascending"), ([1.0, 2.0], "contain 0"), ([np.nan, 0.0], "not finite"),
                           ([], "1 .. 512"), (np.arange(600.0), "1 .. 512")):
        with pytest.raises(StereoHipError, match=match):
            candidates.gather(base, offsets, [base], [(0, 1)])
    with pytest.raises(StereoHipError, match="pairs"):
        candidates.gather(base, [0.0], [base], [1, 2, 3])
    with pytest.raises(StereoHipError, match="whole numbers"):
        candidates.gather(base, [0.0], [base], [(0.5, 0)])
    with pytest.raises(StereoHipError, match=r"2\^15"):
        candidates.gather(base, [0.0], [base], [(0, 1 << 15)])
    with pytest.raises(StereoHipError, match="base's size"):
        candidates.gather(base, [0.0], [np.zeros((H + 1, W))], [(0, 1)])
    with pytest.raises(StereoHipError, match=r"K x \(H\*W\)"):
        stereo_amd.candidates_inputs(ncc, disp, 1.0, np.zeros((2, H * W + 1)), (H, W), conn)
    with pytest.raises(StereoHipError, match="layout"):
        stereo_amd.candidates_inputs(ncc, disp, 1.0, np.zeros((2, H * W)), (H, W), conn, layout=3)
    with pytest.raises(StereoHipError, match="disparities for a volume"):
        stereo_amd.candidates_inputs(ncc, disp[:-1], 1.0, np.zeros((2, H * W)), (H, W), conn)
    nan_cand = np.zeros((2, H * W))
    nan_cand[1, 2 + H * 3] = np.nan
    with pytest.raises(StereoHipError, match=r"row 2, column 3\), label 2"):
        stereo_amd.candidates_inputs(ncc, disp, 1.0, nan_cand, (H, W), conn)
    with pytest.raises(StereoHipError, match="outside 1 .. 2"):
        stereo_amd.candidates_apply(np.zeros((2, H * W)), np.full(H * W, 3.0), (H, W))
    with pytest.raises(StereoHipError, match="whole numbers"):
        stereo_amd.candidates_apply(np.zeros((2, H * W)), np.full(H * W, 1.5), (H, W))
    # levels
    with pytest.raises(StereoHipError, match="at least one"):
        candidates.check_levels([])
    for level, match in ((dict(offsets=[1.0]), "contain 0"), (dict(taps=[(0, 1 << 15)], sources=["base"]), r"2\^15"),
                         (dict(sources=["best"], taps=[(0, 1)]), "'base', 'wta'"), (dict(offset=[0.0]), "dict"),
                         ([0.0], "dict"), (dict(offsets=np.arange(-255.0, 256.0), taps=[(0, 1), (1, 0)], sources=["base"]), "1 .. 512")):
        with pytest.raises(StereoHipError, match=match):
            candidates.check_level(level)
    lv = candidates.check_level(dict(taps=[(0, 1), (1, 0)], sources=["base", "wta"]))
    assert lv["offsets"].tolist() == [0.0] and candidates.CandidateProblem.labels_of(lv) == 5
    for bad, match in (([], "one sequence"), ("ab", "one sequence"), ([[dict(offsets=[0.5])], []], "contain 0")):
        with pytest.raises(StereoHipError, match=match):
            pyramid.check_propagate(bad, 2)
    assert pyramid.check_propagate(None, 2) is None
    assert [len(p) for p in pyramid.check_propagate([None, dict(sources=["wta"], taps=[(0, 0)])], 2)] == [0, 1]
    im = np.zeros((8, 8, 3))
    with pytest.raises(StereoHipError, match="one sequence"):
        stereo_amd.solve_pair_ncc_pyramid([im, im], np.arange(3.0), 1, 40.0, 2.0, 2, 1, 0.0, propagate=[[]])
    for name in ("candidates_inputs", "candidates_apply", "candidates_inputs_device", "candidates_apply_device", "refine_candidates",
                 "CandidateProblem"):
        assert name in stereo_amd.__all__ and callable(getattr(stereo_amd, name))
    for name in ("gather", "gather_device"):
        assert callable(getattr(candidates, name))
    assert callable(stereo_amd.dispmap_ncc.refine_candidates)


def test_globalstereo_refuses_candidate_bands():
    import stereo_amd
    glob = object.__new__(stereo_amd.dispmap_globalstereo)
    with pytest.raises(stereo_amd.StereoHipError, match="dispmap_globalstereo does not take its unary from the NCC sampler"):
        glob.refine_candidates([dict()])


def test_the_three_abi_numbers_agree_and_count_the_candidate_section():
    from stereo_amd import _lib
    text = open(os.path.join(ROOT, "include", "stereo_hip.h")).read()
    declared = int(re.search(r"#define STEREO_HIP_ABI_VERSION (\d+)", text).group(1))
    assert _lib.lib().stereo_hip_abi_version() == declared == _lib.ABI_VERSION >= 17
    for name in ("stereo_candidates_gather", "stereo_candidates_inputs", "stereo_candidates_apply",
                 "stereo_candidates_gather_device", "stereo_candidates_inputs_device", "stereo_candidates_apply_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(_lib.lib(), name)


# ---------------------------------------------------------------- the restatement's own properties

@pytest.mark.parametrize("shuffled", [False, True])
def test_without_sources_the_restatement_is_the_bands(shuffled):
    Hh, Ww, Dd = 5, 7, 6
    ncc = band_restate.volume(Hh, Ww, Dd, 1)
    disp = band_restate.disparities_for(Dd, shuffled)
    offsets = np.array([-1.0, -0.25, 0.0, 0.5, 2.0])
    base = band_restate.base_map(Hh, Ww, Dd, 2.0, 3)
    from oracle import terms as OT
    conn = np.stack(OT.construct_neighborhood(Hh, Ww))
    want = band_restate.band_inputs(ncc, disp, 3.0, base, offsets, conn)
    for sources, taps in (((), ()), ((base,), ()), ((), ((0, 1),))):
        cand = R.gather(base, offsets, sources, taps)
        assert cand.shape == (5, Hh * Ww)
        got = R.candidates_inputs(ncc, disp, 3.0, cand, (Hh, Ww), conn)
        for g, w in zip(got, want):
            assert same_bits(g, w)
        labels = np.random.default_rng(5).integers(1, 6, size=Hh * Ww)
        assert same_bits(R.candidates_apply(cand, labels, (Hh, Ww)), band_restate.band_apply(base, labels, offsets))
    with pytest.raises(ValueError):
        R.candidates_apply(cand, np.full(Hh * Ww, 6), (Hh, Ww))


def test_the_zero_tap_of_the_base_duplicates_the_zero_offset_and_taps_beyond_the_image_clamp():
    Hh, Ww = 5, 7
    base = band_restate.base_map(Hh, Ww, 6, 2.0, 3)
    other = np.arange(Hh * Ww, dtype=np.float64).reshape(Hh, Ww) / 4.0 - 0.0
    other[0, 0] = -0.0
    offsets = np.array([-0.5, 0.0, 0.5])
    taps = [(0, 0), (1, 0), (0, -1), (-9, 0), (0, 9), (9, -9)]
    cand = R.gather(base, offsets, [base, other], taps)
    assert cand.shape == (3 + 2 * 6, Hh * Ww)
    assert same_bits(cand[3], cand[1]) and same_bits(cand[1], base.T.reshape(-1))       # tap (0, 0) of the base: the offset 0.0
    img = lambda row: row.reshape(Ww, Hh).T
    assert same_bits(img(cand[4])[:-1], base[1:]) and same_bits(img(cand[4])[-1], base[-1])          # (1, 0): the row below
    assert same_bits(img(cand[5])[:, 1:], base[:, :-1]) and same_bits(img(cand[5])[:, 0], base[:, 0])
    assert same_bits(img(cand[6]), np.tile(base[0], (Hh, 1)))                                       # beyond the top: row 0
    assert same_bits(img(cand[7]), np.tile(base[:, -1:], (1, Ww)))                                  # beyond the right: last column
    assert same_bits(img(cand[8]), np.full((Hh, Ww), base[-1, 0]))                                  # a corner
    assert same_bits(img(cand[9]), other)                     # the second source follows the first one's T rows; -0 is kept
    # a label that selects a tap applies the neighbour's value, copied
    labels = np.full(Hh * Ww, 5)
    assert same_bits(R.candidates_apply(cand, labels, (Hh, Ww)), img(cand[4]))
    # equal neighbours give equal rows: duplicates are not removed
    flat = np.full((Hh, Ww), 3.25)
    dup = R.gather(flat, [0.0], [flat], [(0, 1), (1, 0)])
    assert dup.shape == (3, Hh * Ww) and (dup == 3.25).all()
    # a candidate of 0 has the plane's -0 as its position, whichever zero the table holds
    from oracle import terms as OT
    conn = np.stack(OT.construct_neighborhood(Hh, Ww))
    z = np.zeros((1, Hh * Ww))
    z[0, ::2] = -0.0
    _, q, qprim = R.candidates_inputs(band_restate.volume(Hh, Ww, 6, 1), band_restate.disparities_for(6, False), 1.0, z, (Hh, Ww), conn)
    assert np.signbit(q).all() and np.signbit(qprim).all() and (q == 0).all()


# ---------------------------------------------------------------- the chain

def chain_problems(shape):
    c = R.chain(shape)
    cand = R.gather(c["base"], c["level"]["offsets"], [c["base"]], c["level"]["taps"])
    cu, cq, cqp = R.candidates_inputs(c["ncc"], c["disp"], R.CHAIN_WEIGHT, cand, shape, c["conn"])
    bu, bq, bqp = band_restate.band_inputs(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base"], R.CHAIN_BAND, c["conn"])
    mk = lambda u, q, qp: dict(unary=np.ascontiguousarray(u.T), conn=c["conn"].T.copy(), q=np.ascontiguousarray(q.T),
                               qprim=np.ascontiguousarray(qp.T), alphas=np.ones(R.CHAIN_N - 1), lam=R.CHAIN_LAMBDA)
    return c, cand, mk(cu, cq, cqp), mk(bu, bq, bqp)


@pytest.mark.parametrize("shape", [(1, 17), (17, 1)], ids=lambda s: "%dx%d" % s)
def test_the_chain_has_the_true_map_as_its_optimum_and_the_band_cannot_reach_it(shape, oracle):
    """Every number is dyadic (first_principles' argument, as in test_band_gpu's chain): the volume is a multiple of 2^-7
    with slices one apart, so the parabola's coefficients are multiples of 2^-8 below 2^9; base, taps' values and offsets
    are multiples of 1/2 below 2^4, so a sample is a multiple of 2^-10 below 2^11 and a unary (weight 4, or 4 (1 + 1e6))
    one of 2^-8 below 2^23; squared position differences are multiples of 2^-2, truncated at 2.  Sums of 17 + 16 such
    terms need under 40 bits: fp64 holds every energy and message exactly.  The quadratic kernel, for the reason given
    there."""
    c, cand, p, pb = chain_problems(shape)
    assert cand.shape == (9, 17) and pb["unary"].shape == (17, 9)
    truth = c["truth"].T.reshape(-1)
    # the true value is a candidate at every pixel, and not a band label where the base is wrong
    assert (cand == truth).any(axis=0).all()
    wrong = c["base"].T.reshape(-1) != truth
    assert wrong.sum() == 9 and (np.abs(c["base"] - c["truth"]).max() == 6.0)
    true_labels = np.array([int(np.flatnonzero(cand[:, i] == truth[i])[0]) for i in range(17)])
    e_true = fp.energy_exact(p, 2, R.CHAIN_LAMBDA, true_labels)
    assert e_true == Fraction(2)                     # unary 0 everywhere, one truncated step
    opt, _ = fp.chain_dp(p, 2, R.CHAIN_LAMBDA)
    opt_band, _ = fp.chain_dp(pb, 2, R.CHAIN_LAMBDA)
    print("chain %dx%d: candidates' optimum %r, band's optimum %r" % (shape + (opt, opt_band)))
    assert Fraction(opt) == e_true
    assert opt < opt_band
    for kernel in (1, 2):
        if kernel == 1:      # the linear kernel's own optimum (its truncated step costs the same 2)
            assert fp.energy_exact(p, 1, R.CHAIN_LAMBDA, true_labels) == Fraction(2)
        labels, en, lb, it = oracle.trws(kernel, p["unary"], p["conn"], p["q"], p["qprim"], p["alphas"], R.CHAIN_LAMBDA, 3, NEVER, mode=1)
        assert en == lb == 2.0 and it <= 3
        assert same_bits(R.candidates_apply(cand, labels, shape), c["truth"])
