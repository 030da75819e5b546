"""CPU: the host-only part of the TRW-S batches (stereo_amd/csrc/trws_batch.cpp) -- the admission rule
and the launch partition -- under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tools/sanitize_batch.cpp: every refusal with its member index, the member limit, a sweep of partitions)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_batch_rule_is_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    exe = str(tmp_path / "sanitize_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize_batch.cpp"),
           os.path.join(ROOT, "stereo_amd", "csrc", "trws_batch.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "sanitize" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("no sanitizer runtime here")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SANITIZE_BATCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
