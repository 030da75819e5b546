"""The plane pyramid on the device: stereo_pyramid_expand_planes and stereo_planes_fit_local, host and
device forms, against the restatements of their definitions (tests/plane_pyramid_restate.py, tests/plane_fit_restate.py)
byte for byte; plane_candidates.Fit as a source; and solve_view_ncc_plane_pyramid / dispmap_ncc.solve_plane_pyramid
against the pipeline written by hand and, without a candidate pass, against solve_pyramid."""
import functools

import numpy as np
import pytest

import plane_fit_restate as FR
import plane_pyramid_restate as PR
import pyramid_restate as R
from plane_pyramid_restate import same_but_zero_sign
from pyramid_restate import same, same_bits
from test_consistency_gpu import rendered_pair, PK, UNARY_WEIGHT, TOL
from test_pyramid_gpu import BANDS, ITERS, NEVER, SHAPES, bands_of, coarse_map, image, restated_images

pytestmark = pytest.mark.gpu

INF = float("inf")


def to_device(planes):
    """4 x N host planes as the (N, 4) tensor the device forms take."""
    import torch
    return torch.from_numpy(np.array(np.asarray(planes).T, order="C")).cuda()


def to_host(t):
    return np.asfortranarray(t.cpu().numpy().T)


def random_planes(n, seed, salted=True):
    """Slanted planes with disparities of a few units; salted: about one in six is not valid, in every way there is."""
    rng = np.random.default_rng([n, seed, 7])
    p = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.choice([1.0, 2.0, -4.0, 0.5], n),
                  rng.uniform(-30.0, 5.0, n)])
    if salted:
        salt = rng.random(n)
        comp = rng.integers(0, 4, n)
        for lo, value in ((0.00, np.nan), (0.04, np.inf), (0.08, -np.inf)):
            hit = (salt >= lo) & (salt < lo + 0.04)
            p[comp[hit], np.flatnonzero(hit)] = value
        p[2, (salt >= 0.12) & (salt < 0.17)] = 0.0
    return p


def valid_mask(p):
    return np.isfinite(p).all(axis=0) & (p[2] != 0.0)


# ---------------------------------------------------------------- 1: the expansion against the restatement

@functools.lru_cache(maxsize=None)
def expand_case(shape, Cn):
    H, W = shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    im = image(H, W, Cn, "doubles", 1)
    red = R.reduce(im)
    coarse = random_planes(Hc * Wc, H * 1000 + W)
    want = {mode: PR.expand_planes(coarse, (H, W), mode, im, red) for mode in (0, 1)}
    return im, red, coarse, want


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_expand_planes_host_and_device_forms_equal_the_restatement(shape, Cn, hip):
    import torch
    from stereo_amd import pyramid
    H, W = shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    im, red, coarse, want = expand_case(shape, Cn)
    d_im, d_red, d_coarse = pyramid.image_to_device(im), pyramid.image_to_device(red), to_device(coarse)
    # a scalar map that is finite exactly where the plane is valid: the scalar expansion makes the same choices
    scalar = np.where(valid_mask(coarse), np.arange(Hc * Wc, dtype=np.float64), np.nan).reshape(Wc, Hc).T
    for mode, name in ((0, "nearest"), (1, "guided")):
        want_out, want_src = want[mode]
        out, src = pyramid.expand_planes(coarse, (H, W), name, im, red)
        assert out.shape == (4, H * W) and src.shape == (H, W) and src.dtype == np.int32
        assert same_bits(out, want_out) and np.array_equal(src, want_src), (mode, shape)
        d_out, d_src = pyramid.expand_planes_device(d_coarse, (H, W), mode, d_im, d_red)
        torch.cuda.synchronize()
        assert tuple(d_out.shape) == (H * W, 4) and same_bits(to_host(d_out), want_out)
        assert np.array_equal(d_src.cpu().numpy().T, want_src)
        scalar_src = pyramid.expand(scalar, (H, W), name, im, red)[1]
        assert np.array_equal(src, scalar_src if mode == 1 else np.zeros_like(src))
        assert np.array_equal(np.isnan(out).all(axis=0), np.isnan(out).any(axis=0))        # four NaN or none
        if mode == 1:
            assert np.array_equal(np.isnan(out[0]).reshape(W, H).T, src == -1)
    none = pyramid.expand_planes(coarse, (H, W), "nearest", want_source=False)               # the nearest mode needs no images
    assert none[1] is None and same_bits(none[0], want[0][0])


@pytest.mark.parametrize("shape", [(5, 7), (130, 5), (3, 67)], ids=lambda s: "%dx%d" % s)
def test_fronto_parallel_planes_expand_as_the_scalar_map_does(shape, hip):
    from stereo_amd import pyramid, plane_candidates
    H, W = shape
    Hc, Wc = pyramid.coarse_size(H, W)
    im = image(H, W, 3, "doubles", 4)
    red = pyramid.reduce(im)
    d = coarse_map(Hc, Wc, 5)                                     # quarter steps, salted with NaN and +-inf
    d[0, 0], d[-1, -1] = 0.0, np.nan                              # a disparity 0 and a hole, whatever the salt did
    for name in ("nearest", "guided"):
        planes, src = pyramid.expand_planes(plane_candidates.fronto(d), (H, W), name, im, red)
        scalar, scalar_src = pyramid.expand(d, (H, W), name, im, red)
        want = plane_candidates.fronto(scalar)
        hole = ~np.isfinite(want[3])
        want[:, hole] = np.nan                                    # a plane without a disparity comes back as four NaN
        # (bit for bit but for the sign of a zero d: include/stereo_hip.h says why)
        assert same_but_zero_sign(planes, want) and same_bits(planes[:3], want[:3])
        nonzero = ~hole & (want[3] != 0.0)
        assert planes[3, nonzero].tobytes() == want[3, nonzero].tobytes() and nonzero.any()
        if name == "guided":
            assert np.array_equal(src, scalar_src)


def test_expand_planes_on_a_side_stream_and_into_given_outputs(hip):
    import torch
    from stereo_amd import pyramid
    H, W = 67, 131
    im, red, coarse, want = expand_case((H, W), 3)
    d_im, d_red, d_coarse = pyramid.image_to_device(im), pyramid.image_to_device(red), to_device(coarse)
    out = torch.full((H * W, 4), 5.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got, src = pyramid.expand_planes_device(d_coarse, (H, W), "guided", d_im, d_red, out=out, stream=side)
    no_source = pyramid.expand_planes_device(d_coarse, (H, W), "guided", d_im, d_red, stream=side, want_source=False)
    side.synchronize()
    assert got is out and same_bits(to_host(out), want[1][0]) and np.array_equal(src.cpu().numpy().T, want[1][1])
    assert no_source[1] is None and same_bits(to_host(no_source[0]), want[1][0])
    with pytest.raises(hip.StereoHipError, match="hold %d elements" % (4 * 34 * 66)):
        pyramid.expand_planes_device(d_coarse[:-1].contiguous(), (H, W), "nearest")
    one = out[:1]
    with pytest.raises(hip.StereoHipError, match="alias"):
        pyramid.expand_planes_device(one, (1, 1), "nearest", out=one)


# ---------------------------------------------------------------- 2: the fit against the restatement

# (5, 37): three column tiles of 16; (130, 5): three row tiles of 64; (67, 3) and (3, 67): both sides of a wave
FIT_SHAPES = [(1, 1), (1, 5), (3, 3), (5, 7), (67, 3), (3, 67), (130, 5), (5, 37)]
TAUS = [0.0, 1.5, INF]


@functools.lru_cache(maxsize=None)
def fit_case(shape, radius):
    H, W = shape
    planes = random_planes(H * W, H * 100 + W + radius)
    if H * W > 1:
        planes[:, 0] = [0.25, -0.5, 0.0, 1.0]                     # at least one plane that is not valid
    return planes, {tau: FR.fit_local(planes, (H, W), radius, tau) for tau in TAUS}


@pytest.mark.parametrize("radius", [1, 2, 8])
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fit_local_host_and_device_forms_equal_the_restatement(shape, radius, hip):
    import torch
    from stereo_amd import plane_candidates as pc
    H, W = shape
    planes, want = fit_case(shape, radius)
    d_planes = to_device(planes)
    for tau in TAUS:
        want_out, want_bad = want[tau]
        assert want_bad == int((~valid_mask(planes)).sum())
        out, bad = pc.fit_local(planes, (H, W), radius, tau)
        assert out.shape == (4, H * W) and bad == want_bad
        assert same_bits(out, want_out), (shape, radius, tau)
        d_out, d_bad = pc.fit_local_device(d_planes, (H, W), radius, tau)
        torch.cuda.synchronize()
        assert tuple(d_out.shape) == (H * W, 4) and same_bits(to_host(d_out), want_out) and int(d_bad.item()) == want_bad
    if min(H, W) > 1:
        assert not same(want[0.0][0], want[INF][0])               # tau reaches the kernel
    if H * W > 1:
        assert want[INF][1] > 0
        with pytest.raises(hip.StereoHipError, match="fit_local_device: %d plane" % want[INF][1]):
            pc.fit_local_device(d_planes, (H, W), radius, INF, check=True)


def test_fit_local_of_dyadic_planes_on_the_device(hip):
    from stereo_amd import plane_candidates as pc
    H, W = 9, 11
    for plane in ((0.25, -0.5, 2.0, -9.0), (-0.75, 0.0, -4.0, 6.0)):
        planes = np.repeat(np.array(plane).reshape(4, 1), H * W, axis=1)
        out, bad = pc.fit_local(planes, (H, W), 3, INF)
        assert bad == 0
        for i in range(H * W):
            for X, Y in ((1.0, 1.0), (float(W), float(H))):
                assert FR.disparity(out[:, i], X, Y) == FR.disparity(planes[:, i], X, Y)


def test_fit_local_on_a_side_stream_gives_the_host_forms_bits(hip):
    import torch
    from stereo_amd import plane_candidates as pc
    H, W = 67, 37
    planes = random_planes(H * W, 11)
    host, host_bad = pc.fit_local(planes, (H, W), 4, 1.5)
    d_planes = to_device(planes)
    out = torch.full((H * W, 4), 5.0, dtype=torch.float64, device="cuda")
    bad = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got, got_bad = pc.fit_local_device(d_planes, (H, W), 4, 1.5, out=out, bad=bad, stream=side)
    side.synchronize()
    assert got is out and got_bad is bad and same_bits(to_host(out), host) and int(bad.item()) == host_bad > 0
    with pytest.raises(hip.StereoHipError, match="alias"):
        pc.fit_local_device(d_planes, (H, W), 2, 1.0, out=d_planes)
    with pytest.raises(hip.StereoHipError, match="hold %d elements" % (4 * H * W)):
        pc.fit_local_device(d_planes[:-1].contiguous(), (H, W), 2, 1.0)


# ---------------------------------------------------------------- 3: Fit as a source

@pytest.mark.parametrize("source_kind", ["ncc", "globalstereo"])
def test_a_level_with_a_fit_source_equals_the_level_given_the_fits_output(source_kind, hip):
    from stereo_amd import plane_candidates as pc
    from test_plane_candidates_gpu import LEVEL_TAPS, level_case, level_source
    H, W = 5, 7
    c = level_case(source_kind, H, W)
    source = level_source(hip, source_kind, c)
    kw = dict(d_min=c["rescale"][0], d_step=c["rescale"][1])
    fit = pc.Fit(radius=2, tau=1.5)
    fitted, bad = pc.fit_local(c["planes"], (H, W), fit.radius, fit.tau)
    assert bad == 0 and not same(fitted, c["planes"])
    level = dict(offsets=c["level"]["offsets"], taps=LEVEL_TAPS, sources=[fit, "base"])
    got = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [level], 4, NEVER, **kw)
    want = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [dict(level, sources=[fitted, "base"])], 4, NEVER, **kw)
    assert np.array_equal(got.labels[0], want.labels[0]) and same_bits(got.planes, want.planes)
    assert (got.energy, got.lower_bound, got.iterations) == (want.energy, want.lower_bound, want.iterations)
    # a second level fits the FIRST level's result, not the planes the call started from
    two = hip.refine_plane_candidates(source, c["planes"], 1, c["tol"], [level, level], 4, NEVER, **kw)
    refit, _ = pc.fit_local(want.planes, (H, W), fit.radius, fit.tau)
    second = hip.refine_plane_candidates(source, want.planes, 1, c["tol"], [dict(level, sources=[refit, "base"])], 4, NEVER, **kw)
    assert same_bits(two.plane_maps[0], want.planes) and same_bits(two.planes, second.planes)
    assert np.array_equal(two.labels[1], second.labels[0]) and two.energy == want.energy + second.energy


# ---------------------------------------------------------------- 4: the pyramid solve against the pipeline by hand

PROPAGATE_TAPS = [(0, 0), (0, 1), (1, 0)]


def propagate_level():
    from stereo_amd import plane_candidates as pc
    return dict(offsets=[-1.0, 0.0, 1.0], taps=PROPAGATE_TAPS, sources=[pc.Fit(1, 1.0), "base", "wta"])       # K = 3 + 3 * 3


def plane_view_by_hand(hip, images, disparities, levels, mode, kernel, relgap, taps=PROPAGATE_TAPS):
    """One view's passes: the restated reduce (images[l] = the view's two images at level l), a solo TrwsPlan at the
    coarsest scale, the restated expand_planes, refine_plane_candidates and refine_plane_band called directly.
    -> per level a dict(plane_maps, labels, energy, bound, iters, expanded, expand_source)."""
    from stereo_amd import plane_candidates as pc, terms as T
    from stereo_amd.trws import TrwsPlan
    out = [dict(plane_maps=[], labels=[], energy=[], bound=[], iters=[], expanded=None, expand_source=None) for _ in range(levels + 1)]
    L = levels
    H, W = images[L][0].shape[:2]
    conn = T.construct_neighborhood(H, W)
    tol_l, weight = R.level_model(kernel, TOL, L)
    disp = R.level_disparities(disparities, L)
    volume = T.ncc_volume(images[L][0], images[L][1], disp, 2, layout=1)
    plan = TrwsPlan(kernel, disp.shape[0], H * W, conn)
    plan.upload(UNARY_WEIGHT * (1.0 - volume), weight * np.ones(conn.shape[1]), tol_l, positions=disp)
    plan.iterate(ITERS, relgap)
    labels, en, lb, it = plan.result()
    plan.close()
    out[L]["labels"].append(labels); out[L]["energy"].append(en); out[L]["bound"].append(lb); out[L]["iters"].append(it)
    planes = PR.fronto(disp[labels.astype(np.int64) - 1].reshape(W, H).T)
    out[L]["plane_maps"].append(planes)
    for l in range(levels - 1, -1, -1):
        H, W = images[l][0].shape[:2]
        conn = T.construct_neighborhood(H, W)
        tol_l, weight = R.level_model(kernel, TOL, l)
        disp = R.level_disparities(disparities, l)
        rec = out[l]
        rec["expanded"], rec["expand_source"] = PR.expand_planes(planes, (H, W), mode, images[l][0], images[l + 1][0])
        volume = T.ncc_volume(images[l][0], images[l][1], disp, 2, layout=1)
        source = hip.NccSource(volume, disp, UNARY_WEIGHT, 1, (H, W))
        alphas = weight * np.ones(conn.shape[1])
        wta = pc.OrOwn(PR.fronto(T.ncc_best_disp(volume, disp, 1, (H, W))))
        level = dict(propagate_level(), taps=taps)
        level["sources"][2] = wta
        a = hip.refine_plane_candidates(source, rec["expanded"], kernel, tol_l, [level], ITERS, relgap, alphas=alphas, conn=conn)
        b = hip.refine_plane_band(source, a.planes, kernel, tol_l, bands_of(levels)[l], ITERS, relgap, alphas=alphas, conn=conn)
        for r in (a, b):
            rec["plane_maps"] += r.plane_maps; rec["labels"] += r.labels; rec["energy"] += r.energy
            rec["bound"] += r.lower_bound; rec["iters"] += r.iterations
        planes = b.planes
    return out


def assert_equals_by_hand(got, want, levels):
    for l in range(levels + 1):
        assert (got.energy[l], got.lower_bound[l], got.iterations[l]) == (want[l]["energy"], want[l]["bound"], want[l]["iters"]), l
        assert len(got.labels[l]) == len(want[l]["labels"]) and all(np.array_equal(a, b) for a, b in zip(got.labels[l], want[l]["labels"]))
        assert len(got.plane_maps[l]) == len(want[l]["plane_maps"]) == (1 if l == levels else 1 + len(bands_of(levels)[l]))
        assert all(same_bits(a, b) for a, b in zip(got.plane_maps[l], want[l]["plane_maps"])), l
        assert len(got.paths[l]) == len(got.plane_maps[l]) and got.carried[l] == [False] * len(got.plane_maps[l])
        if l < levels:
            assert same_bits(got.expanded[l], want[l]["expanded"]) and np.array_equal(got.expand_source[l], want[l]["expand_source"])
        else:
            assert got.expanded[l] is None and got.expand_source[l] is None
    assert same_bits(got.planes, want[0]["plane_maps"][-1]) and got.planes is got.plane_maps[0][-1]


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("expand", ["nearest", "guided"])
@pytest.mark.parametrize("levels", [1, 2])
def test_solve_view_ncc_plane_pyramid_equals_the_pipeline_by_hand(levels, expand, kernel, hip):
    from stereo_amd import pyramid
    disparities = np.arange(PK, dtype=np.float64)
    images = restated_images()
    got = hip.solve_view_ncc_plane_pyramid(rendered_pair(), disparities, kernel, UNARY_WEIGHT, TOL, levels, ITERS, NEVER,
                                           bands=BANDS[levels], expand=expand, propagate=[[propagate_level()]] * levels)
    want = plane_view_by_hand(hip, images, disparities, levels, pyramid.MODES[expand], kernel, NEVER)
    assert_equals_by_hand(got, want, levels)
    for l in range(levels + 1):
        assert np.array_equal(got.disparities[l], R.level_disparities(disparities, l))
        assert (got.tol[l], got.smooth_weight[l]) == R.level_model(kernel, TOL, l)
    H, W = images[0][0].shape[:2]
    assert got.dispmap.shape == (H, W) and same_bits(got.dispmap, FR.own_disparities(got.planes, H, W))
    if levels == 2 and expand == "guided":
        slanted = (got.planes[0] != 0.0) | (got.planes[1] != 0.0)
        print("kernel %d: %d of %d pixels end on a slanted plane" % (kernel, int(slanted.sum()), slanted.size))


def test_carry_levels_and_block_volumes_run_the_same_steps(hip):
    disparities = np.arange(PK, dtype=np.float64)
    args = (rendered_pair(), disparities, 1, UNARY_WEIGHT, TOL, 2, ITERS, NEVER)
    plain = hip.solve_view_ncc_plane_pyramid(*args, bands=BANDS[2])
    carried = hip.solve_view_ncc_plane_pyramid(*args, bands=BANDS[2], carry="levels")
    assert carried.carried[0] == [False, True] and carried.carried[1] == [False] and plain.carried[0] == [False, False]
    assert carried.energy[1] == plain.energy[1] and carried.energy[0][0] == plain.energy[0][0]
    blocks = hip.solve_view_ncc_plane_pyramid(*args, bands=BANDS[2], unary="blocks")
    assert blocks.unary == "blocks" and blocks.planes.shape == plain.planes.shape and np.isfinite(blocks.planes).all()
    with pytest.raises(hip.StereoHipError, match="'scales' is not defined here"):
        hip.solve_view_ncc_plane_pyramid(*args, carry="scales")


# ---------------------------------------------------------------- 5: the objects

def test_without_a_candidate_pass_solve_plane_pyramid_is_solve_pyramid(hip):
    """Fronto-parallel planes go through the plane band as -(-v - delta) = v + delta and through the expansion as 2 v, and
    both builders equal the shared unary / positions entries byte for byte: the new path is the tested one.  (Compared
    bit for bit but for the sign of a zero: the object's planes [0 0 1 -d] give a disparity 0 back as -0, as
    test_pyramid_gpu's object test says of them.)"""
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        want = obj.solve_pyramid(2, bands=BANDS[2], maxiter=ITERS, expand="guided")
        want_map = obj.current_dispmap()
        obj.init_solution()
        got = obj.solve_plane_pyramid(2, bands=BANDS[2], maxiter=ITERS, expand="guided", propagate=None, carry="none")
        assert same_but_zero_sign(got.dispmap, want.dispmap) and same(got.dispmap, want.dispmap)
        assert same(obj.current_dispmap(), want_map) and same(obj.assignment, got.planes)
        for l in range(3):
            assert (got.energy[l], got.lower_bound[l], got.iterations[l]) == (want.energy[l], want.lower_bound[l], want.iterations[l]), l
            assert all(np.array_equal(a, b) for a, b in zip(got.labels[l], want.labels[l])) and len(got.labels[l]) == len(want.labels[l])
            H, W = want.maps[l][0].shape
            assert all(same_but_zero_sign(FR.own_disparities(p, H, W), m) for p, m in zip(got.plane_maps[l], want.maps[l]))
            if l < 2:
                assert np.array_equal(got.expand_source[l], want.expand_source[l])
                assert same_but_zero_sign(FR.own_disparities(got.expanded[l], H, W), want.expanded[l])
        assert np.isfinite(obj.energy())


def test_dispmap_ncc_solve_plane_pyramid_plain_and_mirrored(hip):
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    for obj in (dm, dm.mirrored()):
        obj.max_relgap = 0.0
        images = restated_images(flipped=obj._mirrored)
        # the caller's taps are in the image's own columns; a mirrored object works in flipped ones
        taps = [(dy, -dx) for dy, dx in PROPAGATE_TAPS] if obj._mirrored else PROPAGATE_TAPS
        want = plane_view_by_hand(hip, images, disparities, 2, 1, 1, 0.0, taps=taps)
        got = obj.solve_plane_pyramid(2, bands=BANDS[2], maxiter=ITERS, expand="guided", propagate=[[propagate_level()]] * 2)
        assert_equals_by_hand(got, want, 2)
        assert same(obj.assignment, got.planes) and np.isfinite(obj.energy())
        assert same(obj._unflip(got.dispmap), obj.current_dispmap())
    glob = object.__new__(hip.dispmap_globalstereo)
    with pytest.raises(hip.StereoHipError, match="solve_plane_pyramid: dispmap_globalstereo"):
        glob.solve_plane_pyramid(2)
    with pytest.raises(hip.StereoHipError, match="'scales' is not defined here"):
        dm.solve_plane_pyramid(1, carry="scales")
