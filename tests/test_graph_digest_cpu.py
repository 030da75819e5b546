"""CPU: every bit of what the host-side graph analysis produces is pinned.  tools/graph_digest.cpp -- a stand-alone
program over stereo_amd/csrc/trws_graph*.cpp, nothing is loaded into Python -- builds a TrwsGraph for some 1100 graphs
and option sets, twice (default and 4-visit speculative segments), and prints a digest of every field per case;
tests/golden/trws_graph_digests.txt is its output on the analysis as it was before it was split into stages.  Under
ASan + UBSan where they work here, plain -O2 otherwise."""
import glob
import os
import shutil
import subprocess

import pytest

from test_sanitizers import _asan_works

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trws_graph_digests.txt")
COUNTED = ("fast_ok", "spec", "chunked", "chunked_spec", "run_order", "chain_run_order")


def test_graph_analysis_matches_recorded_digests(tmp_path):
    if not shutil.which("g++") or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("no g++ / HIP headers here")
    flags = ["-O2"]
    if shutil.which("gcc") and _asan_works(tmp_path):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "graph_digest")
    cmd = ["g++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-w",
           os.path.join(ROOT, "tools", "graph_digest.cpp"), *sorted(glob.glob(os.path.join(ROOT, "stereo_amd", "csrc", "trws_graph*.cpp"))),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for g, w in zip(got, want):
        assert g == w, "first differing case: %s (recorded: %r, now: %r)" % (w.split()[0], w, g)
    assert len(got) == len(want), "%d lines, %d recorded" % (len(got), len(want))
    # the digest keeps reaching every branch of the analysis (a condition on the case set, not a measurement)
    counts = [line.split() for line in got if line.startswith("counts ")]
    assert len(counts) == 2 and got[-1].startswith("counts ")
    for words in counts:
        seen = dict(zip(words[2::2], map(int, words[3::2])))
        for name in COUNTED:
            assert seen[name] >= 50, (words[1], name, seen[name])
