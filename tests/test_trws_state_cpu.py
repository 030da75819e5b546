"""The host-side rules of the TRW-S solver state, no device.

stereo_trws_state_check is what a load refuses: every single-field mismatch must be refused with the field's name in
the reason, and the exact / min-plus bit alone must not.  stereo_trws_strip_state_rows_host says which global edge rows
a strip is authoritative for; it must equal a NumPy restatement from stereo_trws_analyze's ranks and the owner table
(phase 1: the owner of the endpoint later in the node order, phase 0: of the earlier one), and over the strips every
edge must be taken exactly once.  tools/sanitize_state_rows.cpp walks both entries under ASan + UBSan as a stand-alone
program.
"""
import numpy as np
import pytest

from helpers import grid_conn
import graph_families


def _header(kernel, K, N, conn0, mode=0, phase=1, iterations=3):
    """a header as a save would fill it, the key through the library's own rule"""
    from stereo_amd.trws import StateHeader
    c = np.asfortranarray(conn0, dtype=np.uint32)
    h = StateHeader()
    h.magic, h.version = 0x53575254, 1
    h.kernel, h.K, h.N, h.E = kernel, K, N, c.shape[1]
    h.message_mode, h.phase, h.iterations = mode, phase, iterations
    # FNV-1a, 64 bit, one step per uint32 word (trws_state.h)
    key = 0xcbf29ce484222325
    for w in c.reshape(-1, order="F"):
        key = ((key ^ int(w)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    h.connectivity_key = key
    h.energy, h.lower_bound, h.lower_bound_next = 12.5, 7.25, 0.0
    return h


def test_state_check_accepts_its_own_plan_and_names_every_mismatch():
    from stereo_amd import StereoHipError
    from stereo_amd.trws import state_check, MESSAGES_MINPLUS, ORDER_INDEX
    H, W, K = 4, 5, 6
    N = H * W
    conn0 = grid_conn(H, W).T
    good = _header(1, K, N, conn0)
    state_check(good, 1, K, N, conn0)
    for phase in (0, 1, 2):
        state_check(_header(1, K, N, conn0, phase=phase), 1, K, N, conn0)
    # exact <-> min-plus may differ between save and load
    state_check(good, 1, K, N, conn0, MESSAGES_MINPLUS)
    state_check(_header(1, K, N, conn0, mode=MESSAGES_MINPLUS | ORDER_INDEX), 1, K, N, conn0, ORDER_INDEX)

    def named(field):
        """the refusal's text for a field: "the state's K (7) is not ..." for the sizes, "<field>: ..." for the rest"""
        return (r"state's %s \(" % field) if field in ("version", "kernel", "K", "N", "E") else (r": %s: " % field)

    def refused(field, header=None, **plan):
        args = dict(kernel=1, K=K, N=N, conn0=conn0, mode=0)
        args.update(plan)
        with pytest.raises(StereoHipError, match=field):
            state_check(header if header is not None else good, args["kernel"], args["K"], args["N"], args["conn0"], args["mode"])

    for field, value in (("magic", 0x12345678), ("version", 2), ("kernel", 2), ("K", K + 1), ("N", N + 1), ("E", conn0.shape[1] - 1),
                         ("connectivity_key", good.connectivity_key ^ 1), ("message_mode", ORDER_INDEX), ("phase", 3),
                         ("phase", -1), ("iterations", -1)):
        bad = type(good).from_buffer_copy(bytes(good))
        setattr(bad, field, value)
        refused(named(field), header=bad)
    # the same from the plan's side
    refused(named("kernel"), kernel=2)
    refused(named("K"), K=K + 1)
    refused(named("N"), N=N + 1)
    refused(named("E"), conn0=conn0[:, :-1])
    swapped = conn0.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]   # the same edges in another order: another state layout
    refused("connectivity_key", conn0=swapped)
    refused("message_mode", mode=ORDER_INDEX)


def _restate_rows(an, owner, g, phase):
    tail, head, rank = an["tail"], an["head"], an["rank"]
    assert (rank[tail] < rank[head]).all()
    return owner[head if phase == 1 else tail] == g


FAMILIES = {
    "grid6x8": lambda: (6 * 8, grid_conn(6, 8)),
    "shuffled6x8": lambda: graph_families.shuffled_grid(6, 8, 3),
}


@pytest.mark.parametrize("G", [2, 3, 4])
@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_strip_state_rows(family, phase, G):
    from stereo_amd.strips import row_strip_owner, strip_state_rows_host, strip_layout_host
    from stereo_amd.trws import analyze
    N, conn = FAMILIES[family]()
    conn0 = conn.T
    an = analyze(N, conn0)
    owner = row_strip_owner(6, 8, G)
    count = np.zeros(conn0.shape[1], int)
    for g in range(G):
        take = strip_state_rows_host(N, conn0, owner, G, g, phase)
        assert np.array_equal(take, _restate_rows(an, owner, g, phase)), (g, phase)
        # an authoritative row is a row the strip stores
        stored = np.zeros(conn0.shape[1], bool)
        stored[strip_layout_host(N, conn0, owner, G, g, 0)["edges"]] = True
        assert (stored | ~take).all()
        count += take
    assert (count == 1).all()
    # the two phases differ exactly on the edges that cross a strip boundary
    crossing = owner[an["tail"]] != owner[an["head"]]
    assert crossing.any()
    for g in range(G):
        differs = strip_state_rows_host(N, conn0, owner, G, g, 0) != strip_state_rows_host(N, conn0, owner, G, g, 1)
        assert not (differs & ~crossing).any()


def test_strip_state_rows_bad_arguments():
    from stereo_amd import StereoHipError
    from stereo_amd.strips import row_strip_owner, strip_state_rows_host
    conn0 = grid_conn(6, 8).T
    owner = row_strip_owner(6, 8, 2)
    for G, g, phase in ((2, 2, 1), (2, -1, 1), (2, 0, 2), (1, 0, 1)):
        with pytest.raises(StereoHipError, match="bad argument"):
            strip_state_rows_host(48, conn0, owner, G, g, phase)


def test_state_file_round_trip(tmp_path):
    """TrwsState.to_file / from_file: data only (np.load without pickle), every field and both arrays back bit for bit"""
    from stereo_amd.trws import TrwsState
    H, W, K = 4, 5, 6
    conn0 = grid_conn(H, W).T
    rng = np.random.default_rng(2)
    h = _header(1, K, H * W, conn0, mode=0x100, phase=2)
    h.lower_bound_next = -3.0e-7
    st = TrwsState(h, rng.normal(size=(conn0.shape[1], K)), rng.integers(0, K, H * W).astype(np.int32))
    path = str(tmp_path / "state.npz")
    st.to_file(path)
    back = TrwsState.from_file(path)
    for name in TrwsState.FIELDS:
        assert getattr(back, name) == getattr(st, name), name
    assert back.messages.flags["C_CONTIGUOUS"] and back.labels.dtype == np.int32
    assert np.array_equal(back.messages, st.messages) and np.array_equal(back.labels, st.labels)
    assert bytes(back.header()) == bytes(h)


def test_state_rules_are_clean_under_sanitizers(tmp_path):
    """tools/sanitize_state_rows.cpp: both host entries under ASan + UBSan, a stand-alone program."""
    import glob
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    exe = str(tmp_path / "sanitize_state_rows")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"), "-w",
           os.path.join(root, "tools", "sanitize_state_rows.cpp"), *sorted(glob.glob(os.path.join(root, "stereo_amd", "csrc", "trws_graph*.cpp"))),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_STATE_ROWS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
