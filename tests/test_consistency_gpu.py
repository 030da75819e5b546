"""Left-right consistency on the device: stereo_lr_check / stereo_lr_fill and their device forms
against the restatement of the definitions (tests/lr_restate.py) bit for bit, NaN positions by mask; the mirrored
dispmap_ncc; and solve_pair_ncc against the same pipeline built from the project's CPU pieces."""
import functools

import numpy as np
import pytest

import lr_restate
from lr_restate import same
from test_consistency_cpu import SCENE, scene_maps

pytestmark = pytest.mark.gpu

NEVER = -1e300
SHAPES = [(1, 1), (1, 7), (63, 5), (64, 64), (65, 130), (130, 3)]


# ---------------------------------------------------------------- check

def check_maps(H, W, direction, seed):
    """Two maps on a quarter-pixel grid (x - d + 0.5 is often an integer: the tie rule), with consistent pixels by
    construction and salted with NaN, +-Inf, negative disparities and disparities beyond W.  With at least 7 columns
    row 0 holds all five statuses whatever the tolerance (up to 1)."""
    rng = np.random.default_rng(seed)
    hi = 4 * min(W, 12) + 1
    ref = rng.integers(0, hi, size=(H, W)) / 4.0
    other = rng.integers(0, hi, size=(H, W)) / 4.0
    for y in range(H):                       # about a third of the pixels: the other view agrees exactly
        for x in range(W):
            xi = int(np.floor(x - direction * ref[y, x] + 0.5))
            if 0 <= xi < W and rng.random() < 0.35:
                other[y, xi] = ref[y, x]
    for m in (ref, other):
        salt = rng.random((H, W))
        m[salt < 0.03] = np.nan
        m[(salt >= 0.03) & (salt < 0.05)] = np.inf
        m[(salt >= 0.05) & (salt < 0.07)] = -np.inf
        m[(salt >= 0.07) & (salt < 0.10)] *= -1.0
        m[(salt >= 0.10) & (salt < 0.13)] += W + 0.25
    if W >= 7:
        s = float(direction)
        ref[0, :7] = [np.nan, 5.0 * s, 0.0, 2.0, 0.0, W + 3.0, np.inf * s]
        other[0, :7] = [7.0, 0.0, 0.0, 7.0, 3.0, 0.0, 0.0]
        other[0, 3 - 2 * direction] = 0.0     # column 3 looks there: residual 2, a mismatch
    return ref, other


@pytest.mark.parametrize("tol", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("direction", [1, -1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_check_equals_the_restatement(shape, direction, tol, hip):
    H, W = shape
    ref, other = check_maps(H, W, direction, 100 * H + W)
    want_st, want_res = lr_restate.lr_check(ref, other, direction, tol)
    st, res = hip.lr_check(ref, other, direction, tol)
    assert st.dtype == np.int32 and st.shape == (H, W)
    assert np.array_equal(st, want_st) and same(res, want_res)
    if W >= 7:
        assert set(np.unique(st).tolist()) == {0, 1, 2, 3, 4}
    st2, none = hip.consistency.lr_check(ref, other, direction, tol, want_residual=False)
    assert none is None and np.array_equal(st2, want_st)


def test_a_residual_of_exactly_tol_is_consistent(hip):
    # column 1 looks at itself (residual -2), column 2 at column 1 (residual -0.5), column 3 too (+0.5)
    ref = np.array([[0.0, 0.0, 1.5, 2.5]])
    other = np.array([[0.0, 2.0, 9.0, 9.0]])
    st, res = hip.lr_check(ref, other, 1, 0.5)
    assert st[0].tolist() == [0, 1, 0, 0] and res[0, 2:].tolist() == [-0.5, 0.5]
    st, _ = hip.lr_check(ref, other, 1, np.nextafter(0.5, 0.0))
    assert st[0].tolist() == [0, 1, 1, 2]
    assert np.array_equal(st, lr_restate.lr_check(ref, other, 1, np.nextafter(0.5, 0.0))[0])


# ---------------------------------------------------------------- fill

def fill_case(H, W, density, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 40, size=(H, W)) / 4.0
    status = np.where(rng.random((H, W)) < density, 0, rng.integers(1, 5, size=(H, W))).astype(np.int32)
    return d, status


def fill_shapes(C):
    return SHAPES + [(3, C - 1), (3, C), (66, C + 1), (3, 2 * C + 1)]


@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
def test_fill_equals_the_restatement(density, hip):
    C = hip.consistency.fill_chunks()
    assert 1 <= C <= 16
    for H, W in fill_shapes(C):
        d, status = fill_case(H, W, density, 1000 * H + W)
        want_f, want_s = lr_restate.lr_fill(d, status)
        f, s = hip.lr_fill(d, status)
        assert s.dtype == np.int32 and same(f, want_f) and np.array_equal(s, want_s), (H, W)
        f2, none = hip.consistency.lr_fill(d, status, want_source=False)
        assert none is None and same(f2, want_f), (H, W)


def chunk_bounds(W, C):
    """Columns [first, last] of the chunks the kernel gives its waves: chunk c starts at c * ceil(W / C)."""
    per = -(-W // C)
    return [(c * per, min((c + 1) * per, W) - 1) for c in range(C) if c * per < W]


@pytest.mark.parametrize("W", ["2C+1", 130])
def test_fill_crafted_rows(W, hip):
    C = hip.consistency.fill_chunks()
    W = 2 * C + 1 if W == "2C+1" else W
    bounds = chunk_bounds(W, C)
    assert len(bounds) > 1
    rng = np.random.default_rng(5)
    patterns = []
    def row(consistent, disp=None):
        st = rng.integers(1, 5, size=W).astype(np.int32)
        st[list(consistent)] = 0
        patterns.append((st, rng.integers(0, 40, size=W) / 4.0 if disp is None else disp))
    row([])                                            # no consistent pixel
    row([0])                                           # only column 0
    row([W - 1])                                       # only column W - 1
    row([a for a, _ in bounds])                        # exactly every chunk's first column
    row([b for _, b in bounds])                        # exactly every chunk's last column
    row([1, W - 2], np.full(W, 3.25))                  # equal disparities on both sides: the left one
    nan_left = rng.integers(0, 40, size=W) / 4.0
    nan_left[bounds[0][1]] = np.nan                    # a NaN disparity at a pixel whose status says 0: copied
    row([bounds[0][1], bounds[1][1]], nan_left)
    nan_right = rng.integers(0, 40, size=W) / 4.0
    nan_right[bounds[1][1]] = np.nan
    row([bounds[0][1], bounds[1][1]], nan_right)
    H = 70                                             # the patterns also sit on both sides of a workgroup's 64 rows
    status = np.stack([patterns[y % len(patterns)][0] for y in range(H)])
    d = np.stack([patterns[y % len(patterns)][1] for y in range(H)])
    want_f, want_s = lr_restate.lr_fill(d, status)
    f, s = hip.lr_fill(d, status)
    assert same(f, want_f) and np.array_equal(s, want_s)
    assert np.isnan(f[0]).all() and (s[0] == -1).all()
    assert (s[5, 2:W - 2] == 1).all() and (f[5] == 3.25).all()
    assert np.isnan(f[6, bounds[0][1] + 1]) and s[6, bounds[0][1] + 1] == bounds[0][1]


# ---------------------------------------------------------------- device forms

def to_device(m):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(m).T)).cuda()


def to_host(t):
    return t.cpu().numpy().T


def test_device_forms_on_a_side_stream_give_the_host_forms_bits(hip):
    import torch
    H, W = 65, 130
    ref, other = check_maps(H, W, 1, 77)
    st, res = hip.lr_check(ref, other, 1, 0.5)
    f, s = hip.lr_fill(ref, st)
    d_ref, d_other = to_device(ref), to_device(other)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    d_st, d_res = hip.lr_check_device(d_ref, d_other, 1, 0.5, stream=side)
    d_f, d_s = hip.lr_fill_device(d_ref, d_st, stream=side)
    d_f2, none = hip.lr_fill_device(d_ref, d_st, stream=side, want_source=False)
    by_chunks = [hip.lr_fill_device(d_ref, d_st, stream=side, chunks=c) for c in (1, 2, 3, 4, 8, 16)]
    side.synchronize()
    assert np.array_equal(to_host(d_st), st) and same(to_host(d_res), res)
    assert same(to_host(d_f), f) and np.array_equal(to_host(d_s), s)
    assert none is None and same(to_host(d_f2), f)
    for cf, cs in by_chunks:
        assert same(to_host(cf), f) and np.array_equal(to_host(cs), s)
    with pytest.raises(hip.StereoHipError, match="column-major"):
        hip.lr_check_device(d_ref.T, d_other.T, 1, 0.5)
    with pytest.raises(hip.StereoHipError, match="size"):
        hip.lr_fill_device(d_ref, d_st[:-1])


# ---------------------------------------------------------------- the scene

@pytest.mark.parametrize("view", ["left", "right"])
def test_two_plane_scene_through_the_library(view, hip):
    direction, status, residual, filled, source = SCENE[view]
    ref, other = scene_maps(view, H=5)
    st, res = hip.lr_check(ref, other, direction, 1.0)
    fl, src = hip.lr_fill(ref, st)
    for y in range(5):
        assert st[y].tolist() == status and same(res[y], np.array(residual))
        assert fl[y].tolist() == filled and src[y].tolist() == source


# ---------------------------------------------------------------- both views of a pair

PH, PW, PK = 24, 40, 8
UNARY_WEIGHT, TOL = 40.0, 2.0


@functools.lru_cache(maxsize=None)
def rendered_pair():
    """The two-plane scene with a random texture, 24 x 40 x 3: background d = 2, a box with d = 6 on rows 4-19 at left
    columns 20-29 = right columns 14-23."""
    rng = np.random.default_rng(11)
    back = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    box = rng.uniform(0, 255, size=(PH, PW + 8, 3))
    left, right = back[:, :PW].copy(), back[:, 2:PW + 2].copy()     # right(x') = back(x' + 2) = left(x' + 2)
    left[4:20, 20:30] = box[4:20, 20:30]
    right[4:20, 14:24] = box[4:20, 20:30]                           # right(x') = box(x' + 6)
    return left, right


@functools.lru_cache(maxsize=None)
def pair_reference():
    """The comparison pipeline, once: the same unary volumes, oracle.trws per view, the NumPy check and fill; for the
    refine pass a solo TrwsPlan per view (the oracle has no warm start): 5 iterations, save, zero the occluded
    columns, upload, load, 3 more."""
    from oracle import pyoracle
    from stereo_amd import consistency, terms as T
    from stereo_amd.trws import TrwsPlan
    disparities = np.arange(PK, dtype=np.float64)
    # (pair_unaries is library code: test_mirrored_object checks it against T.ncc_volume on the flipped pair)
    unaries = consistency.pair_unaries(rendered_pair(), disparities, UNARY_WEIGHT)
    conn = T.construct_neighborhood(PH, PW)
    E = conn.shape[1]
    q = np.tile(disparities, (E, 1))

    def maps(labels):
        return [disparities[l.astype(np.int64) - 1].reshape(PW, PH).T for l in labels]

    def check_fill(dl, dr):
        out = []
        for ref, other, direction in ((dl, dr, 1), (dr, dl, -1)):
            st, res = lr_restate.lr_check(ref, other, direction, 1.0)
            out.append((st, res) + lr_restate.lr_fill(ref, st))
        return out

    first = [pyoracle.trws(1, np.ascontiguousarray(u.T), conn.T, q, q, np.ones(E), TOL, 5, NEVER, mode=1) for u in unaries]
    cf1 = check_fill(*maps([r[0] for r in first]))
    second = []
    for u, (st, _, _, _) in zip(unaries, cf1):
        plan = TrwsPlan(1, PK, PH * PW, conn)
        plan.upload(u, np.ones(E), TOL, positions=disparities)
        plan.iterate(5, NEVER)
        state = plan.save_state()
        zeroed = np.array(u, order="F")
        zeroed[:, st.T.reshape(-1) == 1] = 0.0
        plan.upload(zeroed, np.ones(E), TOL, positions=disparities)
        plan.load_state(state)
        plan.iterate(3, NEVER)
        second.append(plan.result())
        plan.close()
    cf2 = check_fill(*maps([r[0] for r in second]))
    return dict(unaries=unaries, first=first, cf1=cf1, second=second, cf2=cf2)


def assert_views(result, solved, checked, passes):
    for view, ref, (st, res, fl, src) in zip(result.views, solved, checked):
        assert np.array_equal(view.labels, ref[0])
        assert (view.energy[passes - 1], view.lower_bound[passes - 1], view.iterations[passes - 1]) == (ref[1], ref[2], ref[3])
        assert len(view.energy) == len(view.lower_bound) == len(view.iterations) == passes
        assert np.array_equal(view.status, st) and same(view.residual, res)
        assert same(view.filled, fl) and np.array_equal(view.source, src)


@pytest.mark.parametrize("refine_iters", [0, 3])
def test_solve_pair_ncc_equals_the_pipeline_of_cpu_pieces(refine_iters, hip, oracle):
    ref = pair_reference()
    got = hip.solve_pair_ncc(rendered_pair(), np.arange(PK, dtype=np.float64), 1, UNARY_WEIGHT, TOL, 5, NEVER,
                             check_tol=1.0, refine_iters=refine_iters)
    if refine_iters == 0:
        assert_views(got, ref["first"], ref["cf1"], 1)
    else:
        assert_views(got, ref["second"], ref["cf2"], 2)
        for view, first in zip(got.views, ref["first"]):
            assert (view.energy[0], view.lower_bound[0], view.iterations[0]) == first[1:4]
    # the scene is seen: occluded pixels left of the box in the left view, right of it in the right view
    assert (ref["cf1"][0][0] == 1).any() and (ref["cf1"][1][0] == 1).any()


def test_mirrored_object(hip):
    from stereo_amd import consistency, terms as T
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    m = dm.mirrored()
    assert m._mirrored and not dm._mirrored and m.sz == dm.sz
    assert (m.unary_weight, m.tol, m.smoothness_kernel) == (dm.unary_weight, dm.tol, dm.smoothness_kernel)
    assert np.array_equal(m.disparities, dm.disparities)
    # the mirrored unary volume IS the flip of the existing volume function on the flipped pair, swapped
    vol = T.ncc_volume(right[:, ::-1], left[:, ::-1], disparities, 2)
    assert np.array_equal(m.unary_volume(), UNARY_WEIGHT * (1.0 - vol[:, ::-1]))
    assert np.array_equal(dm.unary_volume(), UNARY_WEIGHT * (1.0 - T.ncc_volume(left, right, disparities, 2)))
    # ... and what solve_pair_ncc solves for the right view
    ul, ur = consistency.pair_unaries([left, right], disparities, UNARY_WEIGHT)
    as_hwd = lambda u: u.reshape((PK, PH, PW), order="F").transpose(1, 2, 0)
    assert np.array_equal(as_hwd(ur), m.unary_volume()) and np.array_equal(as_hwd(ul), dm.unary_volume())
    # maps go in and out in the right image's own columns
    assert np.array_equal(m.best_disp_from_ncc(), T.ncc_best_disp(vol, disparities)[:, ::-1])
    assert np.array_equal(m.current_dispmap(), m.best_disp_from_ncc())
    x = np.random.default_rng(3).integers(0, PK, size=(PH, PW)).astype(np.float64)
    m.set_disparity(x)
    assert np.array_equal(m.current_dispmap(), x)
    # right columns 0-13 show the background (d = 2), 14-23 the box (d = 6): the winner's parabola vertex lies within
    # half a step of it.  The mirror of the mirror is the first view
    m.restart()
    assert abs(np.median(m.current_dispmap()[:, 3:12]) - 2.0) < 0.5 and abs(np.median(m.current_dispmap()[6:18, 16:22]) - 6.0) < 0.5
    back = m.mirrored()
    assert not back._mirrored and np.array_equal(back.ncc, dm.ncc)


def test_cross_check_equals_the_raw_calls(hip):
    left, right = rendered_pair()
    disparities = np.arange(PK, dtype=np.float64)
    dm = hip.dispmap_ncc([left, right], disparities, 1, UNARY_WEIGHT, TOL)
    m = dm.mirrored()
    for a, b, direction in ((dm, m, 1), (m, dm, -1)):
        st, filled = a.cross_check(b, tol=1.0)
        want_st, want_res = hip.lr_check(a.current_dispmap(), b.current_dispmap(), direction, 1.0)
        want_f, want_s = hip.lr_fill(a.current_dispmap(), want_st)
        assert np.array_equal(st, want_st) and st is a.consistency and same(filled, want_f) and filled is a.filled_dispmap
        assert same(a.consistency_residual, want_res) and np.array_equal(a.filled_source, want_s)
        assert np.array_equal(st, lr_restate.lr_check(a.current_dispmap(), b.current_dispmap(), direction, 1.0)[0])
    st, filled = dm.cross_check(m, tol=0.25, fill=False)
    assert filled is None and dm.filled_dispmap is None
    small = hip.dispmap_ncc([left[:, :30], right[:, :30]], disparities, 1, UNARY_WEIGHT, TOL)
    with pytest.raises(hip.StereoHipError, match="sizes differ"):
        dm.cross_check(small)
