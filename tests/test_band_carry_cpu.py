"""The host side of the carried messages, no device: the receiving end of every edge's message row
against stereo_trws_analyze, the refusals of stereo_band_carry (each names its argument, before the device is looked
for), properties of the restated definition (tests/carry_restate.py), scale_edge_map on odd sizes, and
tools/sanitize_carry.cpp under ASan + UBSan as a stand-alone program."""
import numpy as np
import pytest

import carry_restate as R
import graph_families
from helpers import grid_conn


# ---------------------------------------------------------------- receivers

FAMILIES = {
    "grid6x8": lambda: (6 * 8, grid_conn(6, 8)),
    "shuffled6x8": lambda: graph_families.shuffled_grid(6, 8, 3),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_receivers_are_the_analysis_head_and_tail(family):
    from stereo_amd.carry import receivers
    from stereo_amd.trws import analyze, ORDER_INDEX
    N, conn = FAMILIES[family]()
    conn0 = conn.T
    an = analyze(N, conn0)
    assert (an["rank"][an["tail"]] < an["rank"][an["head"]]).all()
    for phase, end in ((0, "tail"), (1, "head"), (2, "head")):
        got = receivers(N, conn0, phase)
        assert got.dtype == np.int32 and np.array_equal(got, an[end]), phase
        # node index order: a node's rank is its id
        want = conn0.min(axis=0) if phase == 0 else conn0.max(axis=0)
        assert np.array_equal(receivers(N, conn0, phase, ORDER_INDEX), want), phase
        assert np.array_equal(receivers(N, conn0, phase, ORDER_INDEX | 1), want), phase
    # the two orders do differ on this graph
    assert not np.array_equal(receivers(N, conn0, 1), receivers(N, conn0, 1, ORDER_INDEX))


def test_receivers_refusals():
    from stereo_amd import StereoHipError
    from stereo_amd.carry import receivers
    conn0 = grid_conn(3, 4).T
    for phase in (-1, 3):
        with pytest.raises(StereoHipError, match="phase"):
            receivers(12, conn0, phase)
    with pytest.raises(StereoHipError, match="conn"):
        receivers(11, conn0, 1)
    with pytest.raises(StereoHipError, match="2 x E"):
        receivers(12, conn0.T, 1)
    assert receivers(1, np.zeros((2, 0), int), 1).shape == (0,)


# ---------------------------------------------------------------- refusals of the transfer

def test_every_refusal_names_its_argument_without_a_device():
    from stereo_amd import StereoHipError
    from stereo_amd.carry import carry_messages
    ok = dict(M_old=np.ones((5, 3)), off_old=[-1.0, -0.25, 0.5], off_new=[-0.5, 0.0, 0.125, 2.0], receiver_new=[0, 5, 2, 3],
              shift=np.zeros(6), edge_src=[0, 1, -1, 4], stretch=0.5, gain=2.0)

    def refused(name, **change):
        with pytest.raises(StereoHipError, match=r"stereo_band_carry: .*\b%s\b" % name):
            carry_messages(**dict(ok, **change))

    refused("K_old", M_old=np.ones((5, 0)), off_old=[])
    refused("K_old", M_old=np.ones((5, 4097)), off_old=np.arange(4097.0))
    refused("K_new", off_new=[])
    refused("K_new", off_new=np.arange(513.0))
    refused("off_old", off_old=[-1.0, np.nan, 0.5])
    refused("off_old", off_old=[-1.0, np.inf, 0.5])
    refused("off_old", off_old=[-1.0, -1.0, 0.5])
    refused("off_old", off_old=[-1.0, 0.75, 0.5])
    refused("off_new", off_new=[-0.5, 0.0, 0.0, 2.0])
    refused("off_new", off_new=[-0.5, 0.0, 0.125, -np.inf])
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("stretch", stretch=bad)
        refused("gain", gain=bad)
    refused("edge_src", edge_src=None)                        # E_old = 5, E_new = 4


def test_refusals_of_null_arrays_and_aliased_outputs_through_the_c_entry():
    """the C entries directly: a NULL for every required array, and an output that is an input"""
    import ctypes as C
    from stereo_amd import _lib
    L = _lib.lib()
    M_old, M_new = np.ones((5, 3)), np.zeros((4, 4))
    off_old, off_new = np.array([-1.0, -0.25, 0.5]), np.array([-0.5, 0.0, 0.125, 2.0])
    recv, src, shift = np.array([0, 5, 2, 3], np.int32), np.array([0, 1, -1, 4], np.int32), np.zeros(6)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None

    def call(device, **change):
        a = dict(M_old=M_old, off_old=off_old, d_off_old=off_old, src=src, recv=recv, shift=shift, off_new=off_new,
                 d_off_new=off_new, M_new=M_new, bad=None)
        a.update(change)
        err = _lib.errbuf()
        head = (dp(a["M_old"]), C.c_int64(5), C.c_int(3), dp(a["off_old"]))
        mid = (ip(a["src"]), ip(a["recv"]), C.c_int64(6), dp(a["shift"]), C.c_double(0.5), C.c_double(2.0), dp(a["off_new"]))
        if device:
            rc = L.stereo_band_carry_device(*head, dp(a["d_off_old"]), *mid, dp(a["d_off_new"]), C.c_int(4), C.c_int64(4),
                                            dp(a["M_new"]), ip(a["bad"]), None, err, C.c_size_t(len(err)))
        else:
            rc = L.stereo_band_carry(*head, *mid, C.c_int(4), C.c_int64(4), dp(a["M_new"]),
                                     a["bad"].ctypes.data_as(C.POINTER(C.c_int64)) if a["bad"] is not None else None, err,
                                     C.c_size_t(len(err)))
        return rc, err.value.decode()

    for device in (False, True):
        entry = "stereo_band_carry_device" if device else "stereo_band_carry"
        for name, arg in (("M_old", "M_old"), ("off_old", "off_old"), ("receiver_new", "recv"), ("shift", "shift"),
                          ("off_new", "off_new"), ("M_new", "M_new")):
            rc, why = call(device, **{arg: None})
            assert rc != 0 and why.startswith(entry + ": ") and name in why, (device, name, why)
        for alias in (M_old, shift, off_new):
            rc, why = call(device, M_new=alias)
            assert rc != 0 and "M_new must not be one of the inputs" in why, why
    for name in ("d_off_old", "d_off_new"):
        rc, why = call(True, **{name: None})
        assert rc != 0 and name in why, why
    rc, why = call(True, bad=recv)
    assert rc != 0 and "bad must not be one of the inputs" in why, why
    # what is in order gets as far as the device
    rc, why = call(False)
    import stereo_amd
    if stereo_amd.device_count() < 1:
        assert rc != 0 and "no HIP device" in why, why


# ---------------------------------------------------------------- properties of the restatement

def _rows(E, K, seed):
    """rows whose minimum is already 0, dyadic values"""
    M = np.random.default_rng(seed).integers(0, 64, size=(E, K)) / 8.0
    return M - M.min(axis=1, keepdims=True)


def test_equal_offsets_and_zero_shift_return_the_rows():
    off = np.array([-1.0, -0.3, 0.0, 0.7, 1.9])             # uneven, not dyadic
    M = _rows(7, 5, 1)
    got, bad = R.carry(M, off, off, np.arange(7) % 4, np.zeros(4))
    assert bad == 0 and got.tobytes() == M.tobytes()


def test_a_shift_by_one_step_shifts_the_row_and_replicates_the_end():
    off = np.arange(-4, 5) / 4.0
    M = _rows(6, 9, 2) + 1.0                                 # (the minimum is not zero: the transfer subtracts it)
    recv = np.array([0, 1, 2, 0, 1, 2])
    got, _ = R.carry(M, off, off, recv, np.array([0.25, -0.25, 0.0]))
    for e in range(6):
        want = {0: np.r_[M[e, 1:], M[e, -1]], 1: np.r_[M[e, 0], M[e, :-1]], 2: M[e]}[recv[e]]
        assert np.array_equal(got[e], want - want.min()), e


def test_both_clamps_and_the_zero_rows():
    off_old = np.array([-1.0, -0.3, 0.7])
    off_new = np.array([-0.5, 0.0, 0.5])
    M = np.array([[3.0, 1.0, 2.0]] * 6)
    shift = np.array([-5.0, 5.0, np.nan, np.inf, 0.0])
    got, bad = R.carry(M, off_old, off_new, [0, 1, 2, 3, 4, 4], shift, edge_src=[0, 1, 2, 3, -1, 4])
    assert bad == 0
    assert np.array_equal(got[0], [0.0, 0.0, 0.0]) and np.array_equal(got[1], [0.0, 0.0, 0.0])   # flat: M[0] and M[K - 1]
    assert not got[2:5].any()                                                                    # NaN, inf, edge_src -1
    assert got[5, 1] == (1.0 + (0.0 - -0.3) / (0.7 - -0.3) * (2.0 - 1.0)) - got_min(M[4], off_old, off_new)
    # below the range on the left only, above it on the right only
    got, _ = R.carry(M, off_old, np.array([-2.0, -1.0, -0.3, 0.7, 3.0]), [0], [0.0], edge_src=[0])
    assert np.array_equal(got[0], np.array([3.0, 3.0, 1.0, 2.0, 2.0]) - 1.0)
    # out of range: counted, zero
    got, bad = R.carry(M, off_old, off_new, [0, 5, -1, 4], shift, edge_src=[6, 0, 0, 0])
    assert bad == 3 and not got[:3].any() and got[3].any()


def got_min(row, off_old, off_new):
    """the smallest sample of one row at zero shift (for the check above)"""
    vals = []
    for u in off_new:
        i = int(np.searchsorted(off_old, u, side="right")) - 1
        vals.append(row[i] + (u - off_old[i]) / (off_old[i + 1] - off_old[i]) * (row[i + 1] - row[i]))
    return min(vals)


def test_gain_and_stretch_as_powers_of_two_commute_exactly():
    rng = np.random.default_rng(3)
    off_old = np.sort(rng.choice(np.arange(-40, 41), size=9, replace=False)) / 8.0
    off_new = np.sort(rng.choice(np.arange(-40, 41), size=7, replace=False)) / 8.0
    M = rng.normal(scale=5.0, size=(8, 9))
    recv, shift = np.arange(8) % 3, np.array([0.125, -0.75, 2.0])
    base, _ = R.carry(M, off_old, off_new, recv, shift)
    for gain in (0.5, 2.0, 8.0):
        assert np.array_equal(R.carry(M, off_old, off_new, recv, shift, gain=gain)[0], gain * base)
        assert np.array_equal(R.carry(gain * M, off_old, off_new, recv, shift)[0], gain * base)
    for stretch in (0.5, 2.0):
        # the new offsets scaled by a power of two on the caller's side or by `stretch`: the same samples
        assert np.array_equal(R.carry(M, off_old, off_new, recv, shift, stretch=stretch)[0],
                              R.carry(M, off_old, stretch * off_new, recv, shift)[0])
        # ... and the whole old axis scaled with it: the same rows
        assert np.array_equal(R.carry(M, off_old / stretch, off_new, recv, shift / stretch, stretch=1.0)[0],
                              R.carry(M, off_old, off_new, recv, shift, stretch=stretch)[0])


# ---------------------------------------------------------------- scale_edge_map

def _parent(H, W):
    Hc = (H + 1) // 2
    i = np.arange(H * W)
    return ((i // H) >> 1) * Hc + ((i % H) >> 1)


@pytest.mark.parametrize("fine,coarse", [((5, 6), (3, 3)), ((7, 9), (4, 5))])
def test_scale_edge_map(fine, coarse):
    from stereo_amd.carry import receivers, scale_edge_map
    (H, W), (Hc, Wc) = fine, coarse
    cf, cc = grid_conn(H, W).T, grid_conn(Hc, Wc).T
    parent = _parent(H, W)
    assert parent.max() == Hc * Wc - 1
    rf, rc = receivers(H * W, cf, 1), receivers(Hc * Wc, cc, 1)
    src = scale_edge_map(cc, rc, cf, rf, parent)
    assert src.dtype == np.int32 and src.shape == (cf.shape[1],)
    coarse_of = {(int(a), int(b)): e for e, (a, b) in enumerate(cc.T)}
    crossing = 0
    for e, (a, b) in enumerate(cf.T):
        pa, pb = int(parent[a]), int(parent[b])
        if pa == pb:
            assert src[e] == -1, e                               # inside a block
            continue
        crossing += 1
        c = coarse_of[(pa, pb)]                                  # (a grid edge across a block side: the parents are neighbours)
        if rc[c] == parent[rf[e]]:
            assert src[e] == c, e                                # the coarse edge between the parents, same orientation
        else:
            assert src[e] == -1, e
    assert crossing and (src >= 0).any()
    # no coarse edge is named by an edge whose receiver's parent is not the coarse receiver
    named = src >= 0
    assert np.array_equal(rc[src[named]], parent[rf[named]])
    assert np.array_equal(cc[:, src[named]], parent[cf[:, named]])            # the same orientation
    # coarse receivers on the other end: what was named is not named any more
    other = cc.sum(axis=0) - rc
    assert not ((scale_edge_map(cc, other, cf, rf, parent) >= 0) & named).any()


# ---------------------------------------------------------------- the sanitizer program

def test_carry_host_code_is_clean_under_sanitizers(tmp_path):
    """tools/sanitize_carry.cpp: the receivers entry and the argument checks under ASan + UBSan, a stand-alone program."""
    import glob
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    exe = str(tmp_path / "sanitize_carry")
    csrc = os.path.join(root, "stereo_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"), "-w",
           os.path.join(root, "tools", "sanitize_carry.cpp"), os.path.join(csrc, "carry_host.cpp"),
           *sorted(glob.glob(os.path.join(csrc, "trws_graph*.cpp"))), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_CARRY_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
