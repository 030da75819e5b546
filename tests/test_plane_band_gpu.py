"""Plane-band refinement on the device: stereo_plane_band_inputs_ncc / _globalstereo /
stereo_plane_band_apply and their device forms against K calls of the existing unary entries plus stereo_trws_positions on
the shifted proposals and against the restatement of the definition (tests/plane_band_restate.py); the solve against the
CPU oracle on the inputs the builder produced and, on a chain, against dynamic programming; refine_plane_band's levels;
the method of the two problem classes.

The plane maps carry crafted first pixels: for the NCC source a disparity on a slice, midway between two slices, below
and above the volume's range, on the last and the first slice and a zero disparity sum (band_restate.base_map), with
c = -1 at the first pixel and c = 2 at the second; for the globalstereo source a projected X (or Y) of 0.5, exactly W
(H), W + 1 (H + 1), exactly 1 and W - 0.5 (plane_band_restate.gs_base_map; tests/test_plane_band_cpu.py checks that
they land there)."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import band_restate as BR
import first_principles as fp
import plane_band_restate as R
from band_restate import same_bits

pytestmark = pytest.mark.gpu

NEVER = -1e300
SHAPES = [(1, 9), (9, 1), (5, 7), (67, 3), (3, 67)]      # 67 crosses a wave along y; K N and K E are no multiples of 256
BAND_K = [1, 3, 9, 17, 65]                               # 65 for the builder alone (no solve)
UNARY_WEIGHT = 4.0
COL_THRESH = 30.0
GS_REL = 1e-12                                           # what tests/test_terms_gpu.py grants this kernel's log / exp


def offsets_for(K):
    return (np.arange(K, dtype=np.float64) - K // 2) / 4.0       # K = 1: [0]; quarter-pixel steps around 0


def label_fastest(ncc):
    """H x W x D -> D x N (layout 1)"""
    H, W, D = ncc.shape
    return np.asfortranarray(ncc.transpose(2, 1, 0).reshape(D, W * H))


def frozen(d):
    for a in d.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def ncc_case(H, W, D, K, shuffled, dyadic=True):
    """One NCC problem and its restated answer, built once, never changed."""
    from stereo_amd import terms as T
    ncc = BR.volume(H, W, D, 11)
    disp = BR.disparities_for(D, shuffled)
    offsets = offsets_for(K)
    planes = R.planes_through(BR.base_map(H, W, D, offsets[-1], 5), 6, dyadic)
    conn = T.construct_neighborhood(H, W)
    want = R.inputs_ncc(ncc, disp, UNARY_WEIGHT, planes, offsets, conn)
    return frozen(dict(ncc=ncc, disp=disp, offsets=offsets, planes=planes, conn=conn, want=want))


P2S = {"example": R.P2_example, "rows": R.P2_rows}


@functools.lru_cache(maxsize=None)
def gs_case(H, W, C, K, which, rescale=R.GS_DYADIC, dyadic=True):
    """One globalstereo problem and its restated answer, built once, never changed."""
    from stereo_amd import terms as T
    im0, im1 = R.images(H, W, C, 13)
    P2 = P2S[which]()
    d_min, d_step = rescale
    offsets = offsets_for(K)
    planes = R.planes_through(R.gs_base_map(H, W, P2, d_min, d_step, 8), 9, dyadic)
    conn = T.construct_neighborhood(H, W)
    want = R.inputs_globalstereo(im0, im1, P2, d_min, d_step, COL_THRESH, planes, offsets, conn)
    return frozen(dict(im0=im0, im1=im1, P2=P2, d_min=d_min, d_step=d_step, offsets=offsets, planes=planes, conn=conn, want=want))


def ncc_source(hip, c, layout=0):
    H, W = c["ncc"].shape[:2]
    return hip.NccSource(c["ncc"] if layout == 0 else label_fastest(c["ncc"]), c["disp"], UNARY_WEIGHT, layout, (H, W))


def gs_source(hip, c):
    return hip.GlobalstereoSource(c["im0"], c["im1"], c["P2"], COL_THRESH)


def within(got, want, rel):
    return got.shape == want.shape and float(np.max(np.abs(got - want) / np.maximum(1e-300, np.abs(want) + 1e-3), initial=0.0)) < rel


# ---------------------------------------------------------------- 1: the builder

@pytest.mark.parametrize("D", [1, 2, 3, 6])                        # D = 1: t2 is first and last; D = 2: no interior slice
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ncc_inputs_equal_k_calls_of_the_existing_kernels_and_the_restatement(shape, D, hip):
    from stereo_amd import terms as T
    H, W = shape
    points = T.get_points(H, W)
    cases = [(K, shuffled, True) for K in BAND_K for shuffled in (False, True)] + [(9, False, False)]   # the last: c = 3, not dyadic
    for K, shuffled, dyadic in cases:
        c = ncc_case(H, W, D, K, shuffled, dyadic)
        what = (H, W, D, K, shuffled, dyadic)
        props = R.proposals(c["planes"], c["offsets"])
        unary = np.stack([T.ncc_unary(c["ncc"], c["disp"], UNARY_WEIGHT, P) for P in props])
        q, qprim = T.trws_positions(c["conn"], points, props) if c["conn"].shape[1] else (np.zeros((K, 0)),) * 2
        for layout in (0, 1):
            got = hip.plane_band_inputs(ncc_source(hip, c, layout), c["planes"], c["offsets"], c["conn"])
            assert got[0].shape == (K, H * W) and got[1].shape == got[2].shape == (K, c["conn"].shape[1]), what
            for g, mine, restated in zip(got, (unary, q, qprim), c["want"]):
                assert same_bits(g, mine), what            # the existing kernels, K calls
                assert same_bits(g, restated), what        # the definition


def test_the_crafted_pixels_reach_every_rule_of_the_sampler(hip):
    c = ncc_case(5, 7, 6, 9, False)
    unary = hip.plane_band_inputs(ncc_source(hip, c), c["planes"], c["offsets"], c["conn"])[0]
    out = UNARY_WEIGHT * (1.0 + 1e6)
    zero = 4                                              # offsets[4] == 0
    flat = c["ncc"].transpose(1, 0, 2).reshape(-1, 6)     # [pixel, slice]
    assert c["planes"][2, 0] == -1.0 and c["planes"][2, 1] == 2.0
    assert unary[zero, 0] != out                          # on an interior slice, c negative
    assert unary[zero, 1] == UNARY_WEIGHT * (1.0 - (flat[1, 1] * 0.75 + flat[1, 0] * 0.375 - flat[1, 2] * 0.125))   # midway: the tie goes to slice 1
    assert (unary[:, 2] == out).all() and unary[zero, 3] == out        # below the range with every offset; above it
    assert unary[zero, 4] == UNARY_WEIGHT * (1.0 - flat[4, 5]) and (unary[zero + 1:, 4] == out).all()   # the last slice; beyond it
    assert unary[zero, 5] == UNARY_WEIGHT * (1.0 - flat[5, 0]) and (unary[:zero, 5] == out).all()       # the first slice; before it
    q = hip.plane_band_inputs(ncc_source(hip, c), c["planes"], c["offsets"], c["conn"])[1]
    assert q[8][list(c["conn"][1]).index(6)] == 0.0                    # a zero disparity sum: base -1 with offset +1


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_globalstereo_inputs_equal_k_calls_of_the_existing_kernels_and_the_restatement(shape, C, hip):
    from stereo_amd import terms as T
    H, W = shape
    points = T.get_points(H, W)
    cases = [(K, which, R.GS_DYADIC, True) for K in BAND_K for which in ("example", "rows")]
    cases += [(9, "example", (0.0, 40.0), True), (9, "example", (4.0, 100.0), False)]      # d_step no power of two; c = 3, not dyadic
    for K, which, rescale, dyadic in cases:
        c = gs_case(H, W, C, K, which, rescale, dyadic)
        what = (H, W, C, K, which, rescale, dyadic)
        props = R.proposals(c["planes"], c["offsets"])
        unary = np.stack([T.globalstereo_unary(c["im0"], c["im1"], c["P2"], c["d_min"], c["d_step"], COL_THRESH, P) for P in props])
        q, qprim = T.trws_positions(c["conn"], points, props, c["d_min"], c["d_step"]) if c["conn"].shape[1] else (np.zeros((K, 0)),) * 2
        got = hip.plane_band_inputs(gs_source(hip, c), c["planes"], c["offsets"], c["conn"], c["d_min"], c["d_step"])
        assert got[0].shape == (K, H * W) and got[1].shape == got[2].shape == (K, c["conn"].shape[1]), what
        for g, mine in zip(got, (unary, q, qprim)):
            assert same_bits(g, mine), what                # the existing kernels, K calls
        worst = float(np.max(np.abs(got[0] - c["want"][0]) / np.maximum(1e-300, np.abs(c["want"][0]) + 1e-3)))
        print("globalstereo unary against NumPy %s: worst relative difference %.3g" % (what, worst))
        assert within(got[0], c["want"][0], GS_REL), what
        assert same_bits(got[1], c["want"][1]) and same_bits(got[2], c["want"][2]), what
    # the crafted pixels: out of bounds samples -1000, exp() is 0 and the cost is log 2 -- for X = 0.5 and X = W + 1;
    # X exactly W is inside and costs less
    c = gs_case(H, W, C, 9, "example")
    got = hip.plane_band_inputs(gs_source(hip, c), c["planes"], c["offsets"], c["conn"], c["d_min"], c["d_step"])[0]
    assert abs(got[4, 0] - np.log(2.0)) < 1e-15 and got[4, 2] == got[4, 0] and got[4, 1] < got[4, 0] - 1e-6


# ---------------------------------------------------------------- 2: the device forms

def on_device(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the cases are read-only)


def d_planes(planes):
    return on_device(np.asarray(planes).T)                 # (N, 4): the storage of 4 x N column major


def d_conn(conn):
    return on_device(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32))


def fetch(t, K):
    return t.cpu().numpy().reshape(-1, K).T


DEVICE_CASES = (((1, 9), 1), ((3, 67), 9), ((67, 3), 17))


@pytest.mark.parametrize("layout", [0, 1])
def test_ncc_device_form_on_a_side_stream_gives_the_host_forms_bits(layout, hip):
    import torch
    for (H, W), K in DEVICE_CASES:
        c = ncc_case(H, W, 3, K, True)
        host = hip.plane_band_inputs(ncc_source(hip, c, layout), c["planes"], c["offsets"], c["conn"])
        source, dp, dc = ncc_source(hip, c, layout).device(), d_planes(c["planes"]), d_conn(c["conn"])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        unary, q, qprim, bad = hip.plane_band_inputs_device(source, dp, c["offsets"], dc, stream=side, check=False)
        side.synchronize()
        assert int(bad.item()) == 0
        assert same_bits(fetch(unary, K), host[0]) and same_bits(fetch(q, K), host[1]) and same_bits(fetch(qprim, K), host[2])
    with pytest.raises(hip.StereoHipError, match="elements"):
        hip.plane_band_inputs_device(source, dp[:-1], c["offsets"], dc)
    with pytest.raises(hip.StereoHipError, match="contiguous"):
        hip.plane_band_inputs_device(source, c["planes"], c["offsets"], dc)


@pytest.mark.parametrize("which", ["example", "rows"])
def test_globalstereo_device_form_on_a_side_stream_gives_the_host_forms_bits(which, hip):
    import torch
    for (H, W), K in DEVICE_CASES:
        c = gs_case(H, W, 3, K, which)
        host = hip.plane_band_inputs(gs_source(hip, c), c["planes"], c["offsets"], c["conn"], c["d_min"], c["d_step"])
        source, dp, dc = gs_source(hip, c).device(), d_planes(c["planes"]), d_conn(c["conn"])
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        unary, q, qprim, bad = hip.plane_band_inputs_device(source, dp, c["offsets"], dc, c["d_min"], c["d_step"], stream=side, check=False)
        side.synchronize()
        assert int(bad.item()) == 0
        assert same_bits(fetch(unary, K), host[0]) and same_bits(fetch(q, K), host[1]) and same_bits(fetch(qprim, K), host[2])


@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_bad_counts_a_plane_without_a_disparity_once(source_kind, hip):
    import torch
    H, W, K = 67, 3, 9
    if source_kind == "ncc":
        c = ncc_case(H, W, 3, K, False)
        source, rescale = ncc_source(hip, c), ()
    else:
        c = gs_case(H, W, 3, K, "example")
        source, rescale = gs_source(hip, c), (c["d_min"], c["d_step"])
    planes = c["planes"].copy()
    offenders = [(2, 0, 0.0), (3, 63, np.nan), (0, 64, np.inf), (2, 200, np.nan), (1, 130, -np.inf)]   # (component, pixel, value)
    for component, pixel, value in offenders:
        planes[component, pixel] = value
    with pytest.raises(hip.StereoHipError, match="Infinite disparity.*row 0, column 0"):
        hip.plane_band_inputs(source, planes, c["offsets"], c["conn"], *rescale)
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")        # (the entry zeroes it)
    unary, q, qprim, bad = hip.plane_band_inputs_device(source, d_planes(planes), c["offsets"], d_conn(c["conn"]), *rescale, bad=bad,
                                                        check=False)
    assert int(bad.item()) == len(offenders)
    keep = np.ones(H * W, bool)
    keep[[p for _, p, _ in offenders]] = False
    host = hip.plane_band_inputs(source, c["planes"], c["offsets"], c["conn"], *rescale)
    assert same_bits(fetch(unary, K)[:, keep], host[0][:, keep])        # the other pixels' columns are what they are without the offenders
    clean = keep[c["conn"][0]] & keep[c["conn"][1]]
    assert same_bits(fetch(q, K)[:, clean], host[1][:, clean]) and same_bits(fetch(qprim, K)[:, clean], host[2][:, clean])
    with pytest.raises(hip.StereoHipError, match="5 plane"):
        hip.plane_band_inputs_device(source, d_planes(planes), c["offsets"], d_conn(c["conn"]), *rescale)


def test_an_edge_that_names_no_pixel_reads_nothing_and_gets_nan(hip):
    H, W, K = 5, 7, 9
    c = ncc_case(H, W, 3, K, False)
    conn = c["conn"].copy()
    strays = [0, conn.shape[1] // 2, conn.shape[1] - 1]
    conn[0, strays[0]], conn[1, strays[1]], conn[0, strays[2]] = H * W, H * W + 5, 2 ** 31 + 7
    with pytest.raises(hip.StereoHipError, match="conn names a pixel.*edge 0"):
        hip.plane_band_inputs(ncc_source(hip, c), c["planes"], c["offsets"], conn)
    unary, q, qprim, bad = hip.plane_band_inputs_device(ncc_source(hip, c), d_planes(c["planes"]), c["offsets"], d_conn(conn))
    q, qprim = fetch(q, K), fetch(qprim, K)
    ok = np.ones(conn.shape[1], bool)
    ok[strays] = False
    assert np.isnan(q[:, ~ok]).all() and np.isnan(qprim[:, ~ok]).all()
    assert same_bits(q[:, ok], c["want"][1][:, ok]) and same_bits(qprim[:, ok], c["want"][2][:, ok])
    assert same_bits(fetch(unary, K), c["want"][0])


# ---------------------------------------------------------------- 3: apply

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_apply_equals_the_restatement(shape, hip):
    H, W = shape
    N = H * W
    for K in BAND_K:
        offsets = offsets_for(K)
        for dyadic in (True, False):
            planes = R.planes_through(BR.base_map(H, W, 6, offsets[-1], 9), 3, dyadic)
            labels = np.random.default_rng([H, W, K]).integers(1, K + 1, size=N).astype(np.float64)
            want = R.apply(planes, labels, offsets)
            assert same_bits(hip.plane_band_apply(planes, labels, offsets), want)
            refined, bad = hip.plane_band_apply_device(d_planes(planes), on_device(labels, np.int32), offsets)
            assert same_bits(refined.cpu().numpy().T, want) and int(bad.item()) == 0
        for wrong in (0, K + 1):
            broken = labels.copy()
            broken[N // 2] = wrong
            with pytest.raises(hip.StereoHipError, match="outside 1 .. %d" % K):
                hip.plane_band_apply(planes, broken, offsets)
            refined, bad = hip.plane_band_apply_device(d_planes(planes), on_device(broken, np.int32), offsets, check=False)
            got = refined.cpu().numpy().T
            assert int(bad.item()) == 1 and np.isnan(got[:, N // 2]).all()
            ok = np.arange(N) != N // 2
            assert same_bits(got[:, ok], want[:, ok])
            with pytest.raises(hip.StereoHipError, match="1 pixel"):
                hip.plane_band_apply_device(d_planes(planes), on_device(broken, np.int32), offsets)
        flat = planes.copy()
        flat[2, N // 2] = 0.0
        refined, bad = hip.plane_band_apply_device(d_planes(flat), on_device(labels, np.int32), offsets, check=False)
        assert int(bad.item()) == 1 and np.isnan(refined.cpu().numpy()[N // 2]).all()


# ---------------------------------------------------------------- 4: the solve against the oracle

def solve_args(hip, source_kind, H, W):
    """(source, planes, offsets, conn, rescale, tol) of the level the oracle test and the levels test solve"""
    if source_kind == "ncc":
        c = ncc_case(H, W, 6, 9, False)
        return ncc_source(hip, c), c["planes"], c["offsets"], c["conn"], (0.0, 0.0), 2.0
    c = gs_case(H, W, 3, 9, "example")
    return gs_source(hip, c), c["planes"], c["offsets"], c["conn"], (c["d_min"], c["d_step"]), 0.5


@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (67, 3)], ids=lambda s: "%dx%d" % s)
def test_one_level_equals_the_oracle_on_the_inputs_the_builder_produced(shape, kernel, source_kind, hip, oracle):
    H, W = shape
    source, planes, offsets, conn, rescale, tol = solve_args(hip, source_kind, H, W)
    unary, q, qprim = hip.plane_band_inputs(source, planes, offsets, conn, *rescale)
    E = conn.shape[1]
    ref = oracle.trws(kernel, np.ascontiguousarray(unary.T), conn.T, np.ascontiguousarray(q.T), np.ascontiguousarray(qprim.T),
                      np.ones(E), tol, 5, NEVER, mode=1)
    got = hip.refine_plane_band(source, planes, kernel, tol, [offsets], 5, NEVER, d_min=rescale[0], d_step=rescale[1])
    assert got.paths == [2]                                # the Pipe family: K <= 64, exact messages, positions per edge
    assert np.array_equal(got.labels[0], ref[0])
    assert (got.energy, got.lower_bound, got.iterations) == ([ref[1]], [ref[2]], [ref[3]])
    assert same_bits(got.planes, R.apply(planes, ref[0], offsets)) and got.plane_maps[0] is got.planes
    assert len(set(ref[0])) > 1                            # (the level moves something)


# ---------------------------------------------------------------- 5: first principles, no oracle in between

@pytest.mark.parametrize("shape", [(1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_plane_band_on_a_chain_reaches_the_dynamic_programmes_optimum(shape, hip):
    """Every number is dyadic (first_principles' argument), restated for these inputs.  The planes have a and b multiples
    of 1/4 in [-1, 1], c in {1, -1, 2} and d = -(c base + a x + b y) with base a multiple of 1/4 and x, y <= 9, so d and
    d - c offset (offsets multiples of 1/4) are multiples of 1/4 below 2^6, formed without rounding.  A plane's disparity
    at any of the nine points is such a multiple of 1/4 divided by c: a multiple of 2^-3 below 2^6, exact.  The volume is a
    multiple of 2^-6 with slices one apart, so the parabola's coefficients are multiples of 2^-7 (its divisors are 1 and
    2); a sample r d^2 + p d + q at a multiple of 2^-3 is a multiple of 2^-13 below 2^14, and a unary (weight 4, or
    4 (1 + 1e6) outside the range) one of 2^-11 below 2^23.  Squared position differences are multiples of 2^-6 below
    2^14.  Sums of 9 + 8 such terms are multiples of 2^-11 below 2^28: under 40 bits, so fp64 holds every energy and every
    message of an exact dynamic programme without rounding.  The quadratic kernel only: with positions on a regular grid
    the linear kernel's exact-message mode meets the envelope ties that first_principles.FINE_BITS describes, and the
    bound is then not held to the optimum."""
    H, W = shape
    N = 9
    ncc = BR.volume(H, W, 6, 21)
    disp = BR.disparities_for(6, False)
    offsets = offsets_for(9)
    planes = R.planes_through(BR.base_map(H, W, 6, offsets[-1], 13), 4)
    conn = np.stack([np.arange(N - 1), np.arange(1, N)])           # the path 0 - 1 - ... - 8, one edge per pair
    lam = 2.0
    unary, q, qprim = R.inputs_ncc(ncc, disp, UNARY_WEIGHT, planes, offsets, conn)
    assert np.array_equal(q * 8, np.rint(q * 8)) and np.array_equal(unary * 2048, np.rint(unary * 2048))
    assert not np.array_equal(q, qprim)                            # (neighbours lie on different planes: the edges cost)
    p = dict(unary=np.ascontiguousarray(unary.T), conn=conn.T.copy(), q=np.ascontiguousarray(q.T),
             qprim=np.ascontiguousarray(qprim.T), alphas=np.ones(N - 1), lam=lam)
    opt, _ = fp.chain_dp(p, 2, lam)
    got = hip.refine_plane_band(hip.NccSource(ncc, disp, UNARY_WEIGHT), planes, 2, lam, [offsets], 3, NEVER, conn=conn)
    print("chain %dx%d: energy %r bound %r optimum %r" % (H, W, got.energy[0], got.lower_bound[0], opt))
    assert got.energy[0] == opt and got.lower_bound[0] == opt
    assert fp.energy_exact(p, 2, lam, got.labels[0].astype(np.int64) - 1) == Fraction(opt)
    assert same_bits(got.planes, R.apply(planes, got.labels[0], offsets))


# ---------------------------------------------------------------- 6: levels

@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_two_levels_equal_two_calls_chained_by_hand(source_kind, hip):
    source, planes, coarse, conn, rescale, tol = solve_args(hip, source_kind, 5, 7)
    fine = coarse / 4.0
    kw = dict(d_min=rescale[0], d_step=rescale[1])
    both = hip.refine_plane_band(source, planes, 1, tol, [coarse, fine], 4, NEVER, **kw)
    one = hip.refine_plane_band(source, planes, 1, tol, [coarse], 4, NEVER, **kw)
    two = hip.refine_plane_band(source, one.planes, 1, tol, [fine], 4, NEVER, **kw)
    assert len(both.plane_maps) == 2 and same_bits(both.plane_maps[0], one.planes) and same_bits(both.planes, two.planes)
    assert np.array_equal(both.labels[0], one.labels[0]) and np.array_equal(both.labels[1], two.labels[0])
    assert both.energy == one.energy + two.energy and both.lower_bound == one.lower_bound + two.lower_bound
    assert both.iterations == [4.0, 4.0] and both.paths == [2, 2]
    # a level with another K gets a plan of its own
    mixed = hip.refine_plane_band(source, planes, 1, tol, [coarse, offsets_for(3)], 4, NEVER, **kw)
    assert same_bits(mixed.plane_maps[0], one.planes) and len(mixed.plane_maps) == 2


# ---------------------------------------------------------------- 7: the objects

def restated_levels(before, out, levels):
    planes = before
    for labels, offsets in zip(out.labels, levels):
        planes = R.apply(planes, labels, offsets)
    return planes


def check_object(obj, before, out, levels):
    """after refine_plane_band: the assignment is the restated apply, its energy the last level's, a b c untouched"""
    assert len(out.energy) == len(levels)
    assert same_bits(obj.assignment, restated_levels(before, out, levels)) and same_bits(obj.assignment, out.planes)
    assert same_bits(obj.assignment[:3], before[:3]) and not same_bits(obj.assignment[3], before[3])
    obj.update_energy()
    assert abs(obj.energy() - out.energy[-1]) <= 1e-12 * abs(out.energy[-1])


PH, PW, PK = 12, 16, 4
PAIR_WEIGHT, PAIR_TOL = 40.0, 2.0


def small_pair():
    """12 x 16 x 3, a random texture: background d = 1, a box with d = 3 on rows 3-8 at left columns 8-11 = right 5-8."""
    rng = np.random.default_rng(17)
    back = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    left, right = back[:, :PW].copy(), back[:, 1:PW + 1].copy()
    left[3:9, 8:12] = box[3:9, 8:12]
    right[3:9, 5:9] = box[3:9, 8:12]
    return left, right


def test_dispmap_ncc_refine_plane_band_plain_and_mirrored(hip):
    from stereo_amd import band
    left, right = small_pair()
    disparities = np.arange(PK, dtype=np.float64)
    levels = [offsets_for(9), offsets_for(9) / 4.0]
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        internal = np.rint(obj._unflip(obj.current_dispmap()))
        obj.assignment = R.planes_through(internal, 12)              # slanted planes through the rounded map, internal columns
        before = obj.assignment.copy()
        out = obj.refine_plane_band(levels, maxiter=3)
        check_object(obj, before, out, levels)
        want = hip.refine_plane_band(hip.NccSource(obj.ncc, disparities, PAIR_WEIGHT), before, 1, PAIR_TOL, levels, 3, 0.0)
        assert same_bits(out.planes, want.planes) and out.energy == want.energy
        # refine_band on the same object is what it was: the fronto-parallel band around the current map
        base = obj._unflip(obj.current_dispmap())
        flat = band.refine_band(obj.ncc, disparities, PAIR_WEIGHT, base, 1, PAIR_TOL, levels, 3, 0.0)
        got = obj.refine_band(levels, maxiter=3)
        assert same_bits(obj._unflip(obj.current_dispmap()), flat.dispmap) and got.energy == flat.energy
        assert not obj.assignment[:2].any() and (obj.assignment[2] == 1.0).all()


def test_dispmap_globalstereo_refine_plane_band(hip):
    H, W = 19, 27
    im0, im1 = R.images(H, W, 3, 19)
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))])[:, :, None], (1, 1, 2))       # example_global.m:17-18
    P[0, 3, 1] = -0.25
    segment = 1 + (np.arange(H)[:, None] // 7) * 4 + (np.arange(W)[None, :] // 9)
    gs = hip.dispmap_globalstereo([im0, im1], P, (0, 9), 4, segment=segment, rng=np.random.default_rng(3))
    gs.max_relgap = 0.0
    assert gs.d_min == 0.0 and gs.d_step == 36.0
    base = np.random.default_rng(5).integers(0, 4 * 36 + 1, size=(H, W)).astype(np.float64) / 4.0
    gs.assignment = R.planes_through(base, 14)
    before = gs.assignment.copy()
    levels = [offsets_for(9) / 16.0, offsets_for(9) / 64.0]          # the smoothness term's units, where disp_thresh = 0.02 lives
    out = gs.refine_plane_band(levels, maxiter=3)
    check_object(gs, before, out, [l * gs.d_step for l in levels])   # at the C ABI the offsets are in the planes' units
    assert out.paths == [2, 2]
    with pytest.raises(hip.StereoHipError, match="dispmap_globalstereo does not take its unary from the NCC sampler"):
        gs.refine_band(levels)
