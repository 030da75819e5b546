"""Plane candidates on the device: stereo_plane_candidates_gather / _inputs_ncc / _inputs_globalstereo /
_apply and their device forms against the restatement of the definition (tests/plane_candidates_restate.py) and against K
calls of the existing unary entries plus stereo_trws_positions; the counters; the solve against the CPU oracle on the
restated inputs and, on the slanted chain, against dynamic programming; refine_plane_candidates's levels; the method of
the two problem classes.

The own planes and the sources carry band_restate's / plane_band_restate's crafted first pixels (a disparity on a slice,
midway between two, outside the range, on the end slices; a projected X or Y outside, on and inside the image's border),
and the taps carry those planes to the neighbours."""
import functools

import numpy as np
import pytest

import band_restate as BR
import first_principles as fp
import plane_band_restate as PB
import plane_candidates_restate as R
from band_restate import same, same_bits

pytestmark = pytest.mark.gpu

NEVER = -1e300
SHAPES = [(1, 9), (9, 1), (5, 7), (67, 3), (3, 67)]      # 67 crosses a wave along y; K N and K E are no multiples of 256
UNARY_WEIGHT = 4.0
COL_THRESH = 30.0
GS_REL = 1e-12                                           # what tests/test_plane_band_gpu.py grants this sampler's log / exp
NEAR = [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1)]        # (0, 0) and the radius 1
FAR = [(100, 0), (0, -100), (-70, 70), (0, 68), (68, 0), (2, -3)]          # beyond either side of every shape here
GRID = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3)]            # 25 taps, (0, 0) among them
# (Ko, M, taps): K = 1, 3, 17, 64, 65 -- 17, 64 and 65 put a block boundary inside a pixel's labels
RECIPES = [(1, 0, []), (1, 1, NEAR[:2]), (9, 2, [NEAR[0], NEAR[2], NEAR[3], FAR[2]]), (9, 1, GRID + NEAR + FAR + GRID[:17]),
           (3, 2, GRID + FAR)]
assert [ko + m * len(t) for ko, m, t in RECIPES] == [1, 3, 17, 64, 65]
P2S = {"example": PB.P2_example, "rows": PB.P2_rows}


def offsets_for(K):
    return (np.arange(K, dtype=np.float64) - K // 2) / 4.0       # K = 1: [0]; quarter-pixel steps around 0


def label_fastest(ncc):
    """H x W x D -> D x N (layout 1)"""
    H, W, D = ncc.shape
    return np.asfortranarray(ncc.transpose(2, 1, 0).reshape(D, W * H))


def frozen(d):
    for a in d.values():
        for b in (a if isinstance(a, (tuple, list)) else (a,)):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return d


def finish(c, H, W, taps):
    from stereo_amd import terms as T
    c["conn"] = T.construct_neighborhood(H, W)
    c["taps"] = taps
    c["pcand"] = R.gather(c["planes"], c["offsets"], (H, W), c["sources"], taps)
    c["K"] = c["pcand"].shape[1]
    c["labels"] = np.random.default_rng([H, W, c["K"]]).integers(1, c["K"] + 1, size=H * W).astype(np.float64)
    c["applied"] = R.apply(c["pcand"], c["labels"])
    return c


@functools.lru_cache(maxsize=None)
def ncc_case(H, W, D, recipe, shuffled, dyadic=True):
    """One NCC problem and its restated answer, built once, never changed."""
    Ko, M, taps = RECIPES[recipe]
    ncc = BR.volume(H, W, D, 11)
    disp = BR.disparities_for(D, shuffled)
    offsets = offsets_for(Ko)
    planes = PB.planes_through(BR.base_map(H, W, D, offsets[-1], 5), 6, dyadic)
    sources = [PB.planes_through(BR.base_map(H, W, D, 0.0, 20 + m)[::(-1 if m else 1)].copy(), 30 + m, dyadic) for m in range(M)]
    c = finish(dict(ncc=ncc, disp=disp, offsets=offsets, planes=planes, sources=sources), H, W, taps)
    c["want"] = R.inputs_ncc(ncc, disp, UNARY_WEIGHT, c["pcand"], c["conn"])
    return frozen(c)


@functools.lru_cache(maxsize=None)
def gs_case(H, W, C, recipe, which, rescale=PB.GS_DYADIC, dyadic=True):
    """One globalstereo problem and its restated answer, built once, never changed."""
    Ko, M, taps = RECIPES[recipe]
    im0, im1 = PB.images(H, W, C, 13)
    P2 = P2S[which]()
    d_min, d_step = rescale
    offsets = offsets_for(Ko)
    planes = PB.planes_through(PB.gs_base_map(H, W, P2, d_min, d_step, 8), 9, dyadic)
    sources = [PB.planes_through(PB.gs_base_map(H, W, P2, d_min, d_step, 40 + m)[::(-1 if m else 1)].copy(), 50 + m, dyadic)
               for m in range(M)]
    c = finish(dict(im0=im0, im1=im1, P2=P2, d_min=d_min, d_step=d_step, offsets=offsets, planes=planes, sources=sources), H, W, taps)
    c["want"] = R.inputs_globalstereo(im0, im1, P2, d_min, d_step, COL_THRESH, c["pcand"], c["conn"])
    return frozen(c)


def ncc_source(hip, c, layout=0):
    H, W = c["ncc"].shape[:2]
    return hip.NccSource(c["ncc"] if layout == 0 else label_fastest(c["ncc"]), c["disp"], UNARY_WEIGHT, layout, (H, W))


def gs_source(hip, c):
    return hip.GlobalstereoSource(c["im0"], c["im1"], c["P2"], COL_THRESH)


def on_device(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()          # (a copy: the cases are read-only)


def d_planes(planes):
    return on_device(np.asarray(planes).T)                 # (N, 4): the storage of 4 x N column major


def d_sources(sources):
    import torch
    return torch.stack([d_planes(s) for s in sources]).contiguous() if len(sources) else None


def d_conn(conn):
    return on_device(np.asfortranarray(conn, dtype=np.uint32).reshape(-1, order="F").view(np.int32))


def fetch(t, K):
    return t.cpu().numpy().reshape(-1, K).T


def fetch_table(t, K):
    return t.cpu().numpy().reshape(-1, K, 4).transpose(2, 1, 0)         # (4, K, N)


def relative(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1e-300, np.abs(want) + 1e-3), initial=0.0))


def check_tables(hip, c, shape, what):
    """gather and apply, host and device forms, against the restatement -> the device table"""
    from stereo_amd import plane_candidates
    H, W = shape
    N, K = H * W, c["K"]
    pcand = plane_candidates.gather(c["planes"], c["offsets"], shape, c["sources"], c["taps"])
    assert pcand.shape == (4, K, N) and same_bits(pcand, c["pcand"]), what
    assert same_bits(hip.plane_candidates_apply(pcand, c["labels"], shape), c["applied"]), what
    d_pcand, bad = plane_candidates.gather_device(d_planes(c["planes"]), c["offsets"], shape, d_sources(c["sources"]), c["taps"])
    assert int(bad.item()) == 0 and same_bits(fetch_table(d_pcand, K), c["pcand"]), what
    out, bad = hip.plane_candidates_apply_device(d_pcand, on_device(c["labels"], np.int32), shape)
    assert int(bad.item()) == 0 and same_bits(out.cpu().numpy().T, c["applied"]), what
    return d_pcand


# ---------------------------------------------------------------- 1: gather, inputs, apply against the restatement

@pytest.mark.parametrize("D", [1, 2, 3, 6])                        # D = 1: t2 is first and last; D = 2: no interior slice
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ncc_host_and_device_forms_equal_the_restatement(shape, D, hip):
    H, W = shape
    N = H * W
    cases = [(r, shuffled, True) for r in range(len(RECIPES)) for shuffled in (False, True)] + [(2, False, False)]   # the last: not dyadic
    for recipe, shuffled, dyadic in cases:
        c = ncc_case(H, W, D, recipe, shuffled, dyadic)
        K, E = c["K"], c["conn"].shape[1]
        what = (H, W, D, K, shuffled, dyadic)
        d_pcand = check_tables(hip, c, shape, what)
        for layout in (0, 1):
            got = hip.plane_candidates_inputs(ncc_source(hip, c, layout), c["pcand"], shape, c["conn"])
            assert got[0].shape == (K, N) and got[1].shape == got[2].shape == (K, E), what
            unary, q, qprim, bad = hip.plane_candidates_inputs_device(ncc_source(hip, c, layout), d_pcand, shape, d_conn(c["conn"]))
            assert int(bad.item()) == 0
            for g, d, restated in zip(got, (fetch(unary, K), fetch(q, K), fetch(qprim, K)), c["want"]):
                assert same_bits(g, restated), what + (layout,)
                assert same_bits(d, restated), what + (layout,)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_globalstereo_host_and_device_forms_equal_the_restatement(shape, C, hip):
    H, W = shape
    N = H * W
    cases = [(r, which, PB.GS_DYADIC, True) for r in range(len(RECIPES)) for which in ("example", "rows")]
    cases += [(2, "example", (0.0, 40.0), True), (2, "example", (4.0, 100.0), False)]      # d_step no power of two; not dyadic
    worst = 0.0
    for recipe, which, rescale, dyadic in cases:
        c = gs_case(H, W, C, recipe, which, rescale, dyadic)
        K, E = c["K"], c["conn"].shape[1]
        what = (H, W, C, K, which, rescale, dyadic)
        d_pcand = check_tables(hip, c, shape, what)
        got = hip.plane_candidates_inputs(gs_source(hip, c), c["pcand"], shape, c["conn"], c["d_min"], c["d_step"])
        assert got[0].shape == (K, N) and got[1].shape == got[2].shape == (K, E), what
        unary, q, qprim, bad = hip.plane_candidates_inputs_device(gs_source(hip, c), d_pcand, shape, d_conn(c["conn"]), c["d_min"], c["d_step"])
        assert int(bad.item()) == 0
        dev = (fetch(unary, K), fetch(q, K), fetch(qprim, K))
        for g, d in zip(got, dev):
            assert same_bits(g, d), what                   # host and device forms: one kernel
        rel = relative(got[0], c["want"][0])
        worst = max(worst, rel)
        assert got[0].shape == c["want"][0].shape and rel < GS_REL, what
        assert same_bits(got[1], c["want"][1]) and same_bits(got[2], c["want"][2]), what
    print("globalstereo unary against NumPy %dx%dx%d: worst relative difference %.3g (bound %.3g)" % (H, W, C, worst, GS_REL))


# ---------------------------------------------------------------- 2: the product against itself: one copy of each sampler

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_inputs_equal_K_calls_of_the_existing_entries(shape, hip):
    from stereo_amd import terms as T
    H, W = shape
    points = T.get_points(H, W)
    empty = lambda K: (np.zeros((K, 0)),) * 2
    for D, recipe, shuffled in ((6, 2, False), (3, 4, True), (1, 1, False)):
        c = ncc_case(H, W, D, recipe, shuffled)
        K = c["K"]
        props = [np.asfortranarray(c["pcand"][:, k, :]) for k in range(K)]
        unary = np.stack([T.ncc_unary(c["ncc"], c["disp"], UNARY_WEIGHT, P) for P in props])
        q, qprim = T.trws_positions(c["conn"], points, props) if c["conn"].shape[1] else empty(K)
        got = hip.plane_candidates_inputs(ncc_source(hip, c), c["pcand"], shape, c["conn"])
        for g, mine in zip(got, (unary, q, qprim)):
            assert same_bits(g, mine), (H, W, D, recipe)
    for C, recipe, which, rescale in ((3, 2, "example", PB.GS_DYADIC), (1, 4, "rows", PB.GS_DYADIC), (3, 2, "example", (0.0, 40.0))):
        c = gs_case(H, W, C, recipe, which, rescale)
        K = c["K"]
        props = [np.asfortranarray(c["pcand"][:, k, :]) for k in range(K)]
        unary = np.stack([T.globalstereo_unary(c["im0"], c["im1"], c["P2"], c["d_min"], c["d_step"], COL_THRESH, P) for P in props])
        q, qprim = T.trws_positions(c["conn"], points, props, c["d_min"], c["d_step"]) if c["conn"].shape[1] else empty(K)
        got = hip.plane_candidates_inputs(gs_source(hip, c), c["pcand"], shape, c["conn"], c["d_min"], c["d_step"])
        for g, mine in zip(got, (unary, q, qprim)):
            assert same_bits(g, mine), (H, W, C, recipe, which)


# ---------------------------------------------------------------- 3: side streams, argument checks, counters

@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_device_forms_on_a_side_stream_give_the_host_forms_bits(source_kind, hip):
    import torch
    from stereo_amd import plane_candidates
    for shape, recipe in (((1, 9), 0), ((3, 67), 2), ((67, 3), 4)):
        H, W = shape
        if source_kind == "ncc":
            c = ncc_case(H, W, 3, recipe, True)
            source, rescale = ncc_source(hip, c, 1), ()
        else:
            c = gs_case(H, W, 3, recipe, "rows")
            source, rescale = gs_source(hip, c), (c["d_min"], c["d_step"])
        K = c["K"]
        host_table = plane_candidates.gather(c["planes"], c["offsets"], shape, c["sources"], c["taps"])
        host = hip.plane_candidates_inputs(source, host_table, shape, c["conn"], *rescale)
        host_applied = hip.plane_candidates_apply(host_table, c["labels"], shape)
        source.device()
        dp, ds, dc, dl = d_planes(c["planes"]), d_sources(c["sources"]), d_conn(c["conn"]), on_device(c["labels"], np.int32)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        d_pcand, bad0 = plane_candidates.gather_device(dp, c["offsets"], shape, ds, c["taps"], stream=side, check=False)
        unary, q, qprim, bad1 = hip.plane_candidates_inputs_device(source, d_pcand, shape, dc, *rescale, stream=side, check=False)
        out, bad2 = hip.plane_candidates_apply_device(d_pcand, dl, shape, stream=side, check=False)
        side.synchronize()
        assert int(bad0.item()) == int(bad1.item()) == int(bad2.item()) == 0
        assert same_bits(fetch_table(d_pcand, K), host_table) and same_bits(out.cpu().numpy().T, host_applied)
        assert same_bits(fetch(unary, K), host[0]) and same_bits(fetch(q, K), host[1]) and same_bits(fetch(qprim, K), host[2])
    with pytest.raises(hip.StereoHipError, match="elements"):
        plane_candidates.gather_device(dp[:-1], c["offsets"], shape, ds, c["taps"])
    with pytest.raises(hip.StereoHipError, match=r"\(M, N, 4\)"):
        plane_candidates.gather_device(dp, c["offsets"], shape, ds[0], c["taps"])
    with pytest.raises(hip.StereoHipError, match=r"4 \* K \* H \* W"):
        hip.plane_candidates_inputs_device(source, d_pcand[:-1], shape, dc, *rescale)
    with pytest.raises(hip.StereoHipError, match="contiguous"):
        hip.plane_candidates_inputs_device(source, c["pcand"], shape, dc, *rescale)
    with pytest.raises(hip.StereoHipError, match="16-byte aligned"):
        hip.plane_candidates_inputs_device(source, torch.zeros(4 * K * H * W + 1, dtype=torch.float64, device="cuda")[1:], shape, dc, *rescale)


@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_offending_planes_and_labels_out_of_range_are_counted_once_per_pixel(source_kind, hip):
    import torch
    from stereo_amd import plane_candidates
    shape = H, W = 67, 3
    N = H * W
    if source_kind == "ncc":
        c = ncc_case(H, W, 3, 2, False)              # Ko = 9, two sources, four taps: K = 17
        source, rescale = ncc_source(hip, c), ()
        restate = lambda t: R.inputs_ncc(c["ncc"], c["disp"], UNARY_WEIGHT, t, c["conn"])
    else:
        c = gs_case(H, W, 3, 2, "example")
        source, rescale = gs_source(hip, c), (c["d_min"], c["d_step"])
        restate = lambda t: R.inputs_globalstereo(c["im0"], c["im1"], c["P2"], c["d_min"], c["d_step"], COL_THRESH, t, c["conn"])
    K, E = c["K"], c["conn"].shape[1]
    planes, sources = c["planes"].copy(), [s.copy() for s in c["sources"]]
    planes[2, 0] = 0.0                               # c == 0
    planes[3, 64 + H] = np.inf
    sources[0][0, 63] = -np.inf
    sources[1][1, 64 + H] = np.nan                   # the pixel whose own plane is bad already: counted once
    sources[1][2, 66 + 2 * H] = 0.0
    with pytest.raises(hip.StereoHipError, match=r"Infinite disparity \(c == 0\) in planes at pixel \(row 0, column 0\)"):
        plane_candidates.gather(planes, c["offsets"], shape, sources, c["taps"])
    with pytest.raises(hip.StereoHipError, match=r"source 0 is not finite at pixel \(row 63, column 0\)"):
        plane_candidates.gather(c["planes"], c["offsets"], shape, sources, c["taps"])
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")        # (the entry zeroes it)
    d_pcand, bad = plane_candidates.gather_device(d_planes(planes), c["offsets"], shape, d_sources(sources), c["taps"], bad=bad, check=False)
    assert int(bad.item()) == 4
    with pytest.raises(hip.StereoHipError, match="at 4 pixel"):
        plane_candidates.gather_device(d_planes(planes), c["offsets"], shape, d_sources(sources), c["taps"])
    # the table is what the restatement gathers from the same planes, the offending values included
    got = fetch_table(d_pcand, K)
    with np.errstate(invalid="ignore"):
        want = R.gather(planes, c["offsets"], shape, sources, c["taps"])
    assert same(got, want) and np.array_equal(np.isinf(got), np.isinf(want))
    # inputs counts the pixels with an offending candidate; the other pixels' columns are untouched by them
    offending = ~np.isfinite(want).all(axis=0) | (want[2] == 0)           # K x N
    offenders = offending.any(axis=0)
    assert offenders.sum() > 4                                          # the taps spread them
    dc = d_conn(c["conn"])
    unary, q, qprim, bad = hip.plane_candidates_inputs_device(source, d_pcand, shape, dc, *rescale, bad=torch.full_like(bad, 77), check=False)
    assert int(bad.item()) == offenders.sum()
    clean = np.where(offending[None], c["planes"][:, None, :], want)
    ref = restate(clean)
    assert same_bits(fetch(unary, K)[:, ~offenders], ref[0][:, ~offenders]) if source_kind == "ncc" else \
        relative(fetch(unary, K)[:, ~offenders], ref[0][:, ~offenders]) < GS_REL
    untouched = ~offenders[c["conn"][0]] & ~offenders[c["conn"][1]]
    assert same_bits(fetch(q, K)[:, untouched], ref[1][:, untouched]) and same_bits(fetch(qprim, K)[:, untouched], ref[2][:, untouched])
    with pytest.raises(hip.StereoHipError, match="at %d pixel" % offenders.sum()):
        hip.plane_candidates_inputs_device(source, d_pcand, shape, dc, *rescale)
    with pytest.raises(hip.StereoHipError, match=r"Infinite disparity \(c == 0\) in pcand at pixel \(row 0, column 0\), label 1"):
        hip.plane_candidates_inputs(source, want, shape, c["conn"], *rescale)
    # labels outside 1 .. K: four NaN, counted
    d_good, _ = plane_candidates.gather_device(d_planes(c["planes"]), c["offsets"], shape, d_sources(c["sources"]), c["taps"])
    for wrong in ([0], [K + 1, -3]):
        broken = c["labels"].copy()
        where = [N // 2, N - 1][:len(wrong)]
        broken[where] = wrong
        with pytest.raises(hip.StereoHipError, match="outside 1 .. %d" % K):
            hip.plane_candidates_apply(c["pcand"], broken, shape)
        out, bad = hip.plane_candidates_apply_device(d_good, on_device(broken, np.int32), shape, bad=torch.full_like(bad, 77), check=False)
        got = out.cpu().numpy().T
        ok = np.ones(N, bool)
        ok[where] = False
        assert int(bad.item()) == len(wrong) and np.isnan(got[:, ~ok]).all()
        assert same_bits(got[:, ok], c["applied"][:, ok])
        with pytest.raises(hip.StereoHipError, match="%d label" % len(wrong)):
            hip.plane_candidates_apply_device(d_good, on_device(broken, np.int32), shape)
    # an edge that names a pixel outside the image reads nothing and gets NaN; everything else is as it was
    conn = np.array(c["conn"], dtype=np.uint32)
    strays = [0, 5, E - 1]
    conn[0, 0], conn[1, 5], conn[0, E - 1] = N, N + 5, 0xFFFFFFFF
    unary, q, qprim, bad = hip.plane_candidates_inputs_device(source, d_good, shape, d_conn(conn), *rescale)
    q, qprim = fetch(q, K), fetch(qprim, K)
    ok = np.ones(E, bool)
    ok[strays] = False
    assert np.isnan(q[:, ~ok]).all() and np.isnan(qprim[:, ~ok]).all()
    assert same_bits(q[:, ok], c["want"][1][:, ok]) and same_bits(qprim[:, ok], c["want"][2][:, ok])
    host_unary = hip.plane_candidates_inputs(source, c["pcand"], shape, c["conn"], *rescale)[0]
    assert same_bits(fetch(unary, K), host_unary)
    with pytest.raises(hip.StereoHipError, match="conn names a pixel.*edge 0"):
        hip.plane_candidates_inputs(source, c["pcand"], shape, conn, *rescale)


# ---------------------------------------------------------------- 4: one level against the oracle

LEVEL_TAPS = [(0, 0), (1, 0), (0, -1)]


@functools.lru_cache(maxsize=None)
def level_case(source_kind, H, W):
    """K = 3 + 2 * 3 = 9: the own planes and another plane map at (0, 0) and two neighbours"""
    from stereo_amd import terms as T
    conn = T.construct_neighborhood(H, W)
    offsets = offsets_for(3)
    if source_kind == "ncc":
        ncc, disp = BR.volume(H, W, 6, 11), BR.disparities_for(6, False)
        planes = PB.planes_through(BR.base_map(H, W, 6, offsets[-1], 5), 6)
        other = PB.planes_through(BR.base_map(H, W, 6, 0.0, 31)[::-1].copy(), 32)
        pcand = R.gather(planes, offsets, (H, W), [planes, other], LEVEL_TAPS)
        extra = dict(ncc=ncc, disp=disp, rescale=(0.0, 0.0), tol=2.0, want=R.inputs_ncc(ncc, disp, UNARY_WEIGHT, pcand, conn))
    else:
        im0, im1 = PB.images(H, W, 3, 13)
        P2, (d_min, d_step) = PB.P2_example(), PB.GS_DYADIC
        planes = PB.planes_through(PB.gs_base_map(H, W, P2, d_min, d_step, 8), 9)
        other = PB.planes_through(PB.gs_base_map(H, W, P2, d_min, d_step, 41)[::-1].copy(), 42)
        pcand = R.gather(planes, offsets, (H, W), [planes, other], LEVEL_TAPS)
        extra = dict(im0=im0, im1=im1, P2=P2, rescale=(d_min, d_step), tol=0.5)
    return frozen(dict(extra, planes=planes, other=other, conn=conn, pcand=pcand,
                       level=dict(offsets=offsets, taps=LEVEL_TAPS, sources=["base", other])))


def level_source(hip, source_kind, c):
    if source_kind == "ncc":
        return hip.NccSource(c["ncc"], c["disp"], UNARY_WEIGHT)
    return hip.GlobalstereoSource(c["im0"], c["im1"], c["P2"], COL_THRESH)


@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(5, 7), (67, 3)], ids=lambda s: "%dx%d" % s)
def test_one_level_equals_the_oracle_on_the_restated_inputs(shape, kernel, source_kind, hip, oracle):
    H, W = shape
    c = level_case(source_kind, H, W)
    source = level_source(hip, source_kind, c)
    # the NCC inputs are the restatement's, bit for bit; the globalstereo unary agrees with NumPy within GS_REL only, so
    # its oracle run takes the inputs the builder produced, as tests/test_plane_band_gpu.py does
    unary, q, qprim = c["want"] if source_kind == "ncc" else hip.plane_candidates_inputs(source, c["pcand"], shape, c["conn"], *c["rescale"])
    E = c["conn"].shape[1]
    ref = oracle.trws(kernel, np.ascontiguousarray(unary.T), c["conn"].T, np.ascontiguousarray(q.T), np.ascontiguousarray(qprim.T),
                      np.ones(E), c["tol"], 5, NEVER, mode=1)
    got = hip.refine_plane_candidates(source, c["planes"], kernel, c["tol"], [c["level"]], 5, NEVER, d_min=c["rescale"][0],
                                      d_step=c["rescale"][1])
    assert got.paths == [2]                                # the Pipe family: K <= 64, exact messages, positions per edge
    assert np.array_equal(got.labels[0], ref[0])
    assert (got.energy, got.lower_bound, got.iterations) == ([ref[1]], [ref[2]], [ref[3]])
    assert got.carried == [False]
    assert same_bits(got.planes, R.apply(c["pcand"], ref[0])) and got.plane_maps[0] is got.planes
    assert len(set(ref[0])) > 1                            # (the level moves something)


# ---------------------------------------------------------------- 5: the slanted chain

@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shape", [(1, 17), (17, 1)], ids=lambda s: "%dx%d" % s)
def test_plane_candidates_on_the_slanted_chain_reach_the_true_planes_and_the_bands_do_not(shape, kernel, hip):
    """The chain of test_plane_candidates_cpu (its docstring has the exactness argument: every energy and message is exact
    in fp64; its test pins the three optima by dynamic programming).  The plane-candidate level reaches energy = bound =
    2.0, the energy of the true planes; the plane band around the same base and the fronto-parallel candidate level on the
    base's disparity map stay at or above their own optima."""
    from fractions import Fraction
    c = R.chain(shape)
    band_opt = {1: 57.67578125, 2: 57.41796875}[kernel]
    source = hip.NccSource(c["ncc"], c["disp"], R.CHAIN_WEIGHT)
    got = hip.refine_plane_candidates(source, c["base"], kernel, R.CHAIN_LAMBDA, [c["level"]], 3, NEVER, conn=c["conn"])
    print("chain %dx%d kernel %d: energy %r bound %r in %r iteration(s)" % (shape + (kernel, got.energy[0], got.lower_bound[0], got.iterations[0])))
    assert got.energy[0] == 2.0 and got.lower_bound[0] == 2.0
    assert same_bits(got.planes, c["truth"])
    pcand = R.gather(c["base"], c["level"]["offsets"], shape, [c["base"]], c["level"]["taps"])
    u, q, qp = R.inputs_ncc(c["ncc"], c["disp"], R.CHAIN_WEIGHT, pcand, c["conn"])
    p = dict(unary=np.ascontiguousarray(u.T), conn=c["conn"].T.copy(), q=np.ascontiguousarray(q.T), qprim=np.ascontiguousarray(qp.T),
             alphas=np.ones(R.CHAIN_N - 1), lam=R.CHAIN_LAMBDA)
    assert fp.energy_exact(p, kernel, R.CHAIN_LAMBDA, got.labels[0].astype(np.int64) - 1) == Fraction(2)
    banded = hip.refine_plane_band(source, c["base"], kernel, R.CHAIN_LAMBDA, [R.CHAIN_BAND], 3, NEVER, conn=c["conn"])
    fronto = hip.refine_candidates(c["ncc"], c["disp"], R.CHAIN_WEIGHT, c["base_disp"], kernel, R.CHAIN_LAMBDA, [c["fronto_level"]], 3,
                                   NEVER, conn=c["conn"])
    print("     the plane band: energy %r bound %r (optimum %r); the candidate band: energy %r bound %r (optimum 57.65625)"
          % (banded.energy[0], banded.lower_bound[0], band_opt, fronto.energy[0], fronto.lower_bound[0]))
    assert banded.energy[0] >= band_opt and banded.lower_bound[0] <= band_opt
    assert fronto.energy[0] >= 57.65625 and fronto.lower_bound[0] <= 57.65625
    assert not same(banded.planes, c["truth"]) and not same(fronto.dispmap, c["true_disp"].reshape(shape))


# ---------------------------------------------------------------- 6: levels

@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_two_levels_equal_two_calls_chained_by_hand(source_kind, hip):
    c = level_case(source_kind, 5, 7)
    source = level_source(hip, source_kind, c)
    first = c["level"]
    second = dict(offsets=offsets_for(9) / 4.0, taps=[(0, 0), (0, 1)], sources=[c["other"], "base"])      # K = 13: a plan of its own
    kw = dict(d_min=c["rescale"][0], d_step=c["rescale"][1])
    both = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [first, second], 4, NEVER, **kw)
    one = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [first], 4, NEVER, **kw)
    two = hip.refine_plane_candidates(source, one.planes, 1, c["tol"], [second], 4, NEVER, **kw)
    assert len(both.plane_maps) == 2 and same_bits(both.plane_maps[0], one.planes) and same_bits(both.planes, two.planes)
    assert np.array_equal(both.labels[0], one.labels[0]) and np.array_equal(both.labels[1], two.labels[0])
    assert both.energy == one.energy + two.energy and both.lower_bound == one.lower_bound + two.lower_bound
    assert both.iterations == [4.0, 4.0] and both.paths == [2, 2] and both.carried == [False, False]
    # 'base' is the planes the level starts from
    by_array = hip.refine_plane_candidates(source, one.planes, 1, c["tol"], [dict(second, sources=[c["other"], one.planes])], 4, NEVER, **kw)
    assert np.array_equal(by_array.labels[0], two.labels[0]) and same_bits(by_array.planes, two.planes) and by_array.energy == two.energy
    # an equal K shares the plan: the second bind starts from zero as the first did
    again = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [first, first], 4, NEVER, **kw)
    solo = hip.refine_plane_candidates(source, one.planes, 1, c["tol"], [first], 4, NEVER, **kw)
    assert np.array_equal(again.labels[1], solo.labels[0]) and again.energy[1:] == solo.energy


# ---------------------------------------------------------------- 7: the objects

PH, PW, PK = 12, 16, 4
PAIR_WEIGHT, PAIR_TOL = 40.0, 2.0
RING = [(-1, 0), (1, 0), (0, -1), (0, 1)]


def small_pair():
    """The pair of tests/test_plane_band_gpu.py: 12 x 16 x 3, a random texture: background d = 1, a box with d = 3 on rows
    3-8 at left columns 8-11 = right 5-8."""
    rng = np.random.default_rng(17)
    back = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 4, 3))
    left, right = back[:, :PW].copy(), back[:, 1:PW + 1].copy()
    left[3:9, 8:12] = box[3:9, 8:12]
    right[3:9, 5:9] = box[3:9, 8:12]
    return left, right


def loop_by_hand(hip, source, planes, kernel, tol, levels, maxiter, relgap, conn, alphas, d_min=0.0, d_step=0.0):
    """refine_plane_candidates's loop restated with PlaneCandidateProblem: one plan per level"""
    prob = hip.PlaneCandidateProblem(source, planes, conn, alphas, d_min, d_step)
    energies = []
    for level in levels:
        plan = hip.TrwsPlan(int(kernel), prob.labels_of(level), prob.N, prob.conn)
        try:
            prob.build(level, plan, tol)
            plan.iterate(maxiter, relgap)
            labels, en, lb, it = plan.result()
            energies.append(en)
            assert prob.carry_from(plan, labels) is None
            planes = prob.apply(labels)
        finally:
            plan.close()
    return planes, energies


def check_object(obj, out, want_planes, want_energy):
    assert same_bits(obj.assignment, out.planes) and same_bits(out.planes, want_planes) and out.energy == want_energy
    obj.update_energy()
    assert abs(obj.energy() - out.energy[-1]) <= 1e-12 * abs(out.energy[-1])


def test_dispmap_ncc_refine_plane_candidates_plain_and_mirrored(hip):
    from stereo_amd import plane_candidates
    left, right = small_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, PAIR_WEIGHT, PAIR_TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        internal = np.rint(obj._unflip(obj.current_dispmap()))
        obj.assignment = PB.planes_through(internal, 12)                 # slanted planes through the rounded map, internal columns
        before = obj.assignment.copy()
        shifted = np.roll(obj.current_dispmap(), 1, axis=1) + 0.25       # a map in the coordinates current_dispmap() speaks
        other = PB.planes_through(internal[::-1].copy(), 13)             # 4 x N: internal columns, as `assignment` is
        levels = [dict(offsets=[-0.5, 0.0, 0.5], taps=RING + [(0, 2)], sources=["base", "wta"]),
                  dict(offsets=[0.0], taps=[(0, 0), (0, 1)], sources=[shifted, other])]
        out = obj.refine_plane_candidates(levels, maxiter=3)
        assert [len(set(l)) > 1 for l in out.labels] == [True, True]
        flip = np.array([1, -1]) if obj._mirrored else np.array([1, 1])
        by_hand = [dict(offsets=np.array([-0.5, 0.0, 0.5]), taps=np.array(RING + [(0, 2)], np.int32) * flip,
                        sources=["base", plane_candidates.OrOwn(plane_candidates.fronto(obj._best_disp()))]),
                   dict(offsets=np.array([0.0]), taps=np.array([(0, 0), (0, 1)], np.int32) * flip,
                        sources=[plane_candidates.fronto(obj._unflip(shifted)), other])]
        want, energies = loop_by_hand(hip, hip.NccSource(obj.ncc, disparities, PAIR_WEIGHT), before, 1, PAIR_TOL,
                                      plane_candidates.check_levels(by_hand), 3, 0.0, obj.neighborhood, obj.smooth_weights)
        check_object(obj, out, want, energies)
        assert not same_bits(obj.assignment[:3], before[:3])            # a copied plane brings its own slant
    assert dm.mirrored()._mirrored and not dm._mirrored


def test_dispmap_globalstereo_refine_plane_candidates(hip):
    from stereo_amd import plane_candidates
    H, W = 19, 27
    im0, im1 = PB.images(H, W, 3, 19)
    P = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))])[:, :, None], (1, 1, 2))       # example_global.m:17-18
    P[0, 3, 1] = -0.25
    segment = 1 + (np.arange(H)[:, None] // 7) * 4 + (np.arange(W)[None, :] // 9)
    gs = hip.dispmap_globalstereo([im0, im1], P, (0, 9), 4, segment=segment, rng=np.random.default_rng(3))
    gs.max_relgap = 0.0
    assert gs.d_min == 0.0 and gs.d_step == 36.0
    base = np.random.default_rng(5).integers(0, 4 * 36 + 1, size=(H, W)).astype(np.float64) / 4.0
    gs.assignment = PB.planes_through(base, 14)
    before = gs.assignment.copy()
    proposal = PB.planes_through(base[::-1].copy(), 15)
    levels = [dict(offsets=offsets_for(3) / 16.0, taps=RING, sources=["base"]),       # the smoothness term's units
              dict(offsets=[0.0], taps=[(0, 0)], sources=["base", proposal, PB.slanted_map(H, W, 0.25, -0.5, 2.0, -30.0)])]
    out = gs.refine_plane_candidates(levels, maxiter=3)
    assert out.paths == [2, 2] and len(set(out.labels[0])) > 1            # (the first level moves something)
    by_hand = plane_candidates.check_levels([dict(l, offsets=np.asarray(l["offsets"]) * gs.d_step) for l in levels])   # the planes' units
    source = hip.GlobalstereoSource(gs.images[0], gs.images[1], gs.P2, gs.options["col_thresh"])
    want, energies = loop_by_hand(hip, source, before, gs._kernel, gs.tol, by_hand, 3, 0.0, gs.neighborhood, gs.smooth_weights,
                                  gs.d_min, gs.d_step)
    check_object(gs, out, want, energies)
    with pytest.raises(hip.StereoHipError, match="dispmap_globalstereo does not take its unary from the NCC sampler"):
        gs.refine_candidates([dict()])
