"""CPU: the QPBO host code that makes no HIP call (stereo_amd/csrc/qpbo_graph.cpp, qpbo_rand.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, through tools/sanitize_qpbo_host.cpp: the weak persistency pass on the
whole residual network and on the gathered free subgraph give the same labels, and those are what the strongly connected
components of the free residual graph say (transitive closure); pair grouping and the host-built doubled graph on
parallel, antiparallel and duplicated edges reproduce the caller's energy; the Improve permutation is the plain rand()
loop and leaves the generator where that loop leaves it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asan_works(tmp_path):
    src = tmp_path / "t.c"
    src.write_text("int main(void){return 0;}\n")
    r = subprocess.run(["gcc", "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "t")], capture_output=True)
    return r.returncode == 0 and subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_qpbo_host_code_is_right_and_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++") or not _asan_works(tmp_path):
        pytest.skip("no working -fsanitize=address here")
    csrc = os.path.join(ROOT, "stereo_amd", "csrc")
    exe = str(tmp_path / "sanitize_qpbo_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), "-Wall", os.path.join(ROOT, "tools", "sanitize_qpbo_host.cpp"),
           os.path.join(csrc, "qpbo_graph.cpp"), os.path.join(csrc, "qpbo_rand.cpp"), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SANITIZE_QPBO_HOST_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
