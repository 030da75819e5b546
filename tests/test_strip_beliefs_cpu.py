"""The lists the belief kernels walk on a row strip (stereo_trws_strip_belief_lists_host), no device.

A NumPy restatement built from stereo_trws_analyze (the firstForward / firstBackward lists by node id, in list order)
and stereo_trws_strip_layout_host (the strip's local node and edge ids) must equal the host entry exactly; every own
node appears once and in rank order, every listed edge has an own endpoint, and the strips' lists put back under global
ids and merged by rank are the single plan's lists.
"""
import numpy as np
import pytest

from helpers import grid_conn

GRIDS = [(9, 40), (8, 6), (5, 7)]


def _restate(N, conn0, owner, G, g, an):
    """own / fptr / fidx / bptr / bidx of strip g from the analysis and the strip's layout."""
    from stereo_amd.strips import strip_layout_host
    if G == 1:
        node_l, edge_l = np.arange(N), np.arange(conn0.shape[1])
        mine = np.ones(N, bool)
    else:
        L = strip_layout_host(N, conn0, owner, G, g, 0)
        node_l = np.full(N, -1); node_l[L["nodes"]] = np.arange(len(L["nodes"]))
        edge_l = np.full(conn0.shape[1], -1); edge_l[L["edges"]] = np.arange(len(L["edges"]))
        mine = owner == g
        assert L["n_own"] == int(mine.sum())
    by_rank = np.argsort(an["rank"], kind="stable")
    own, fptr, fidx, bptr, bidx = [], [0], [], [0], []
    for i in by_rank:
        if not mine[i]:
            continue
        own.append(node_l[i])
        fidx += [edge_l[e] for e in an["fwd_idx"][an["fwd_ptr"][i]:an["fwd_ptr"][i + 1]]]
        bidx += [edge_l[e] for e in an["bwd_idx"][an["bwd_ptr"][i]:an["bwd_ptr"][i + 1]]]
        fptr.append(len(fidx)); bptr.append(len(bidx))
    return dict(own=own, fptr=fptr, fidx=fidx, bptr=bptr, bidx=bidx)


@pytest.mark.parametrize("G", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_strip_belief_lists(grid, G):
    from stereo_amd.strips import row_strip_owner, strip_belief_lists_host, strip_layout_host
    from stereo_amd.trws import analyze
    H, W = grid
    N = H * W
    conn0 = grid_conn(H, W).T
    an = analyze(N, conn0)
    owner = row_strip_owner(H, W, G)
    tail, head = an["tail"], an["head"]
    seen = np.zeros(N, int)
    per_rank = {}
    for g in range(G):
        got = strip_belief_lists_host(N, conn0, owner if G > 1 else None, G, g)
        want = _restate(N, conn0, owner, G, g, an)
        for k in ("own", "fptr", "fidx", "bptr", "bidx"):
            assert np.array_equal(got[k], np.asarray(want[k], np.int32)), (g, k)
        if G > 1:
            L = strip_layout_host(N, conn0, owner, G, g, 0)
            nodes, edges, n_own = L["nodes"], L["edges"], L["n_own"]
        else:
            nodes, edges, n_own = np.arange(N), np.arange(conn0.shape[1]), N
        # own nodes only (local ids below n_own), each once, in rank order
        assert len(got["own"]) == n_own and (got["own"] < n_own).all() and (got["own"] >= 0).all()
        ids = nodes[got["own"]]
        assert (owner[ids] == g).all()
        seen[ids] += 1
        assert (np.diff(an["rank"][ids]) > 0).all()
        # every listed edge is stored by the strip and has an own endpoint
        for ptr, idx in ((got["fptr"], got["fidx"]), (got["bptr"], got["bidx"])):
            assert ptr[0] == 0 and ptr[-1] == len(idx) and (np.diff(ptr) >= 0).all()
            assert (idx >= 0).all() and (idx < len(edges)).all()
            e = edges[idx]
            assert ((owner[tail[e]] == g) | (owner[head[e]] == g)).all()
        for j, i in enumerate(ids):
            per_rank[int(an["rank"][i])] = (list(edges[got["fidx"][got["fptr"][j]:got["fptr"][j + 1]]]),
                                            list(edges[got["bidx"][got["bptr"][j]:got["bptr"][j + 1]]]))
    assert (seen == 1).all()
    # the strips together, back under global ids and in rank order: the single plan's lists
    one = strip_belief_lists_host(N, conn0, None, 1, 0)
    assert np.array_equal(one["own"], np.argsort(an["rank"], kind="stable"))
    fidx = [e for r in range(N) for e in per_rank[r][0]]
    bidx = [e for r in range(N) for e in per_rank[r][1]]
    assert np.array_equal(one["fidx"], fidx) and np.array_equal(one["bidx"], bidx)
    assert np.array_equal(one["fptr"], np.cumsum([0] + [len(per_rank[r][0]) for r in range(N)]))
    assert np.array_equal(one["bptr"], np.cumsum([0] + [len(per_rank[r][1]) for r in range(N)]))


def test_bad_arguments_are_refused():
    from stereo_amd import StereoHipError
    from stereo_amd.strips import row_strip_owner, strip_belief_lists_host
    conn0 = grid_conn(8, 6).T
    with pytest.raises(StereoHipError, match="bad argument"):
        strip_belief_lists_host(48, conn0, row_strip_owner(8, 6, 2), 2, 2)
    with pytest.raises(StereoHipError, match="bad argument"):
        strip_belief_lists_host(48, conn0, None, 2, 0)


def test_list_builder_is_clean_under_sanitizers(tmp_path):
    """tools/sanitize_strip_lists.cpp: the builder over the grids above under ASan + UBSan, a stand-alone program."""
    import glob
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    exe = str(tmp_path / "sanitize_strip_lists")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"), "-w",
           os.path.join(root, "tools", "sanitize_strip_lists.cpp"), *sorted(glob.glob(os.path.join(root, "stereo_amd", "csrc", "trws_graph*.cpp"))),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "SANITIZE_STRIP_LISTS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
