"""CPU: the runner's host-made chain records (stereo_amd/csrc/trws_runner_records.cpp) against
an independent NumPy transcription of the derivation the loaders of the K <= 64 runner made on the device until then
(trws_spec.h: run_loader at the parent of round 12, "rows the node in front hands over" through "cut behind this
node?", gamma, the staged words, the fetch mask and the lane selections for the weights).

tools/runner_records_dump.cpp -- a stand-alone program, nothing is loaded into Python -- builds the graph and prints,
for every direction and every descriptor set the runner can be launched on, the bound descriptors and the records.
The two derivations must agree word for word, all 64 words of every chain position, in both directions, on
  grids 12 x 9 and 9 x 12 with segments of 4, 30 x 40 with 16;
  13 x 10 with segments of 4: 42 chain positions, the last segment is shorter and the `< nseg` cap is hit;
  the single-edged grid of graph_families.py (one handed-over row);
  a grid whose border pairs are listed three times: chain nodes with five and more incoming rows.  Such a graph never
    keeps the speculative schedule (trws_graph_desc.cpp: runner_can_walk refuses more than four), so the tool makes
    the records of its longest chain run all the same: the builder is a function of the descriptors alone;
  the sub-row descriptor sets (row chunk 12, few resident workgroups), the backward sweep's among them.
The census of the `kinds` word in test_runner_visit_gpu.py's docstring is a second, committed reference for word 1."""
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import graph_families as gf
from helpers import grid_conn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DW = RW = 64


def _i32(x):
    return int(np.int32(np.uint32(x & 0xFFFFFFFF)))


def tripled_border_grid(H, W):
    """grid_conn plus one more directed edge (low id first) for every pair of neighbouring BORDER pixels: a border pixel
    off the corners has 2 * 3 + 2 = 8 incident edges, the descriptor kernels' limit"""
    c = grid_conn(H, W)
    row, col = c % H, c // H
    border = ((row == 0) | (row == H - 1) | (col == 0) | (col == W - 1)).all(axis=1)
    return H * W, np.concatenate([c, c[border & (c[:, 0] < c[:, 1])]])


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    tmp = tmp_path_factory.mktemp("runner_records")
    exe = str(tmp / "runner_records_dump")
    cmd = ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-w",
           os.path.join(ROOT, "tools", "runner_records_dump.cpp"), *sorted(glob.glob(os.path.join(ROOT, "stereo_amd", "csrc", "trws_graph*.cpp"))),
           os.path.join(ROOT, "stereo_amd", "csrc", "trws_runner_records.cpp"), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]

    def run(N, conn, seg, chunk_f=0, chunk_b=-1, resident=0, longest=False):
        """[(direction, sub, c0, c1, seg_len, nseg, descriptors (n, 64), records (n, 64))]"""
        path = str(tmp / "graph.txt")
        with open(path, "w") as f:
            f.write("%d %d\n" % (N, len(conn)))
            np.savetxt(f, conn, fmt="%d")
        r = subprocess.run([exe, path, str(seg), str(chunk_f), str(chunk_b), str(resident)] + ["longest"] * longest, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines, sets, i = r.stdout.splitlines(), [], 0
        while i < len(lines):
            assert lines[i].startswith("set "), lines[i]
            d, sub, c0, c1, L, nseg = map(int, lines[i].split()[1:])
            n = c1 - c0
            desc = np.array([ln.split() for ln in lines[i + 1:i + 1 + n]], dtype=np.int64)
            rec = np.array([ln.split() for ln in lines[i + 1 + n:i + 1 + 2 * n]], dtype=np.int64)
            assert desc.shape == (n, DW) and rec.shape == (n, RW)
            sets.append((d, sub, c0, c1, L, nseg, desc, rec))
            i += 1 + 2 * n
        return sets
    return run


def _record(w, wn, first, last, j, L, nseg):
    """the 64 words of position c0 + j from its descriptor w and the next one's wn (zeros behind the run): what the
    device derived at the parent of round 12, in the order of that routine"""
    f, fn = int(w[2]), int(wn[2])
    nout, nin, ndep, md = f & 15, (f >> 4) & 15, (f >> 8) & 15, (f >> 16) & 255
    ntot = nout + nin
    noutn = fn & 15
    ntotn = noutn + ((fn >> 4) & 15)
    # rows the node in front hands over: a ballot over lanes 0-7
    fr = 0 if first else sum(1 << k for k in range(8) if nout <= k < ntot and w[12 + k] >= 0)
    frn = 0 if last else sum(1 << k for k in range(8) if noutn <= k < ntotn and wn[12 + k] >= 0)
    kfirst = (fr & -fr).bit_length() - 1 if fr else ntot
    s0 = s1 = -1
    for k in range(8):
        if (frn >> k) & 1:
            s = int(wn[12 + k])
            if s0 < 0 or s0 == s:
                s0 = s
            else:
                s1 = s
    p0s = int(w[12 + kfirst]) if fr else -1
    kinds = nt = nstaged = 0
    stage_of = [-1, -1, -1, -1]
    for k in range(kfirst, ntot):
        if (fr >> k) & 1:
            kd = 8 if w[12 + k] == p0s else 9
        else:
            kd = nstaged
            if nstaged < 4:
                stage_of[nstaged] = k
            nstaged += 1
        kinds |= kd << (4 * nt)
        nt += 1
    cut = pubkinds = 0
    if not last and (j + 1) % L == 0 and (j + 1) // L < nseg:
        cut = (j + 1) // L
        for k in range(noutn, ntotn):
            if (frn >> k) & 1:
                pubkinds |= (8 if wn[12 + k] == s0 else 9) << (4 * k)
    R = [0] * RW
    # the staged words: lane == kRsNt ? nt : lane == kRsKinds ? ... ; the labels' lanes start at -1, the twin verdict at
    # "one message if any"
    R[0], R[1], R[2], R[5], R[6], R[7], R[8], R[13], R[14] = nt, kinds | (nt << 16), 0 if s0 < 0 else 1, cut, pubkinds, nout, nin, md >> nout, int(w[0])
    R[9:13] = [-1] * 4
    # doubles 8-15 of the staged node: av[lane] = alpha[w[4 + (lane & 7)]]; a0 = av[s0 < 0 ? 0 : s0], a1 = av[s1 < 0 ? that : s1],
    # gamma, ain = av[nout + lane - 3]
    a0 = 0 if s0 < 0 else s0
    a1 = a0 if s1 < 0 else s1
    R[16], R[17], R[18] = int(w[4 + (a0 & 7)]), int(w[4 + (a1 & 7)]), 0
    for lane in range(3, 8):
        R[16 + lane] = int(w[4 + ((nout + lane - 3) & 7)])
    R[24], R[25], R[26], R[27] = kfirst, nout, ndep, int(w[1])
    fm = int(w[55]) & 255
    fetch = sum(1 << k for k in range(8) if nout <= k < ntot and (fm >> k) & 1 and not (fr >> k) & 1)
    R[28] = fetch
    R[29] = sum(1 << k for k in range(8) if (fetch >> k) & 1 and k - nout < 4)   # (lane == k - nout: src; lanes 0-3 reach the words)
    g = 1.0 / float(nout if nout > nin else nin if nin > 0 else 1)
    R[30], R[31] = struct.unpack("<ii", struct.pack("<d", g))
    R[32:40] = [int(x) for x in w[4:12]]
    R[40:48] = [int(x) for x in w[32:40]]
    R[48:51] = stage_of[:3]
    # the old rows of the messages: `if (s0 == k)` for k < 4 only; the rows of twins are compared for a != b in 0 .. 3
    m0 = s0 if 0 <= s0 < 4 else -1
    m1 = s1 if 0 <= s1 < 4 else -1
    R[51], R[52] = m0, m1
    R[53] = 0 if s1 < 0 else 2 if (m0 >= 0 and m1 >= 0) else 1
    R[54], R[55] = s0, s1
    R[56:60] = [int(x) for x in w[20:24]]
    R[60] = nin
    return [_i32(x) for x in R]


def _compare(sets, want_sets):
    assert [(s[0], s[1]) for s in sets] == want_sets, [(s[0], s[1]) for s in sets]
    census = {}
    for d, sub, c0, c1, L, nseg, desc, rec in sets:
        n = c1 - c0
        zeros = np.zeros(DW, np.int64)
        for j in range(n):
            want = _record(desc[j], desc[j + 1] if j + 1 < n else zeros, j == 0, j + 1 == n, j, L, nseg)
            got = [int(x) for x in rec[j]]
            assert got == want, "direction %d sub %d position %d: words %s differ (record %s, transcription %s)" % (
                d, sub, c0 + j, [k for k in range(RW) if got[k] != want[k]], [got[k] for k in range(RW) if got[k] != want[k]],
                [want[k] for k in range(RW) if got[k] != want[k]])
        keys, counts = np.unique(rec[:, 1], return_counts=True)
        census[(d, sub)] = {int(k): int(c) for k, c in zip(keys, counts)}
    return census


GRIDS = {
    (12, 9, 4): ({0x0: 1, 0x20098: 36, 0x41908: 1}, {0x0: 1, 0x30098: 13, 0x30908: 21, 0x20098: 3}),
    (9, 12, 4): ({0x0: 1, 0x20098: 36, 0x41908: 1}, {0x0: 1, 0x30098: 19, 0x30908: 15, 0x20098: 3}),
    (30, 40, 16): ({0x0: 1, 0x20098: 134, 0x41908: 1}, {0x0: 1, 0x30098: 75, 0x30908: 57, 0x20098: 3}),
}


@pytest.mark.parametrize("H,W,seg", sorted(GRIDS))
def test_records_on_grids(H, W, seg, dump):
    census = _compare(dump(H * W, grid_conn(H, W), seg), [(0, 0), (1, 0)])
    assert (census[(0, 0)], census[(1, 0)]) == GRIDS[(H, W, seg)]   # (test_runner_visit_gpu.py's docstring)


def test_records_last_segment_shorter(dump):
    """13 x 10: 42 chain positions in segments of 4 -- ten segments, the last of two visits; no cut at position 40"""
    sets = dump(130, grid_conn(13, 10), 4)
    _compare(sets, [(0, 0), (1, 0)])
    for d, sub, c0, c1, L, nseg, desc, rec in sets:
        assert (c1 - c0, L, nseg) == (42, 4, 10)
        assert [int(x) for x in rec[:, 5]] == [(j + 1) // 4 if (j + 1) % 4 == 0 and (j + 1) // 4 < 10 else 0 for j in range(42)]
        assert rec[39, 5] == 0 and rec[35, 5] == 9


def test_records_single_edged_grid(dump):
    N, conn = gf.single_grid(30, 40)
    census = _compare(dump(N, conn, 16), [(0, 0), (1, 0)])
    assert census[(0, 0)] == {0x0: 1, 0x10008: 134, 0x20008: 1} and census[(1, 0)] == {0x0: 1, 0x10008: 98, 0x20008: 37}


def test_records_many_incoming_rows(dump):
    """border pairs listed three times: chain nodes with five to eight incoming rows, more than one staged row"""
    N, conn = tripled_border_grid(14, 19)
    sets = dump(N, conn, 4, longest=True)
    _compare(sets, [(0, 0), (1, 0)])
    nin = np.concatenate([(s[6][:, 2] >> 4) & 15 for s in sets])
    assert nin.max() >= 5 and (nin >= 5).sum() >= 20, np.bincount(nin)
    assert max(int(s[7][:, 49].max()) for s in sets) >= 0   # a second staged row somewhere


def test_records_sub_row_descriptor_sets(dump):
    """row chunk 12 in both directions with two resident workgroups: the sub-row schedule's descriptors are another
    array with other foreign dependencies, and the runner's records are made from them"""
    sets = dump(1200, grid_conn(30, 40), 16, 12, 12, 2)
    _compare(sets, [(0, 0), (0, 1), (1, 0), (1, 1)])
    sets = dump(1200, grid_conn(30, 40), 16, 0, 12, 4)   # (STEREO_HIP_TRWS_ROW_CHUNK=0,12: the backward sweep's only)
    _compare(sets, [(0, 0), (1, 0), (1, 1)])


def test_builder_under_sanitizers(tmp_path):
    """tools/sanitize_runner_records.cpp, a stand-alone program: the builder on these graphs, on every chain run and on
    degenerate ranges, under ASan + UBSan where they work here, plain -O2 otherwise"""
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    from test_sanitizers import _asan_works
    flags = ["-O2"]
    if shutil.which("gcc") and _asan_works(tmp_path):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "sanitize_runner_records")
    cmd = ["g++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-w",
           os.path.join(ROOT, "tools", "sanitize_runner_records.cpp"), *sorted(glob.glob(os.path.join(ROOT, "stereo_amd", "csrc", "trws_graph*.cpp"))),
           os.path.join(ROOT, "stereo_amd", "csrc", "trws_runner_records.cpp"), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_RUNNER_RECORDS_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
