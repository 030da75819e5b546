"""Records tests/golden/ref_calls_*.npz: the answers of the reference's own libraries (oracle/_ref) to the calls of the
tests that compare against them live, so that those tests run where oracle/_ref cannot be built (tests/ref_calls.py).
Needs oracle/_ref (make -C oracle ref).  Run from the repository root:  python tests/golden/make_golden_ref_calls.py"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = ["tests/test_oracle_trws.py::test_against_live_reference_types",
         "tests/test_oracle_trws.py::test_restated_envelope_equals_reference_classes_on_adversarial_messages",
         "tests/test_oracle_qpbo.py::test_against_live_reference",
         "tests/test_oracle_qpbo.py::test_tie_labels_of_the_reference_depend_on_its_own_edge_order",
         "tests/test_segment_cpu.py::test_host_stages_against_the_reference_segmenters_live"]

if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from oracle import pyoracle
    if not (pyoracle.have_ref_qpbo() and pyoracle.have_ref_types() and pyoracle.have_ref_segment()
            and pyoracle.ref_segment_gb_lib() is not None):
        sys.exit("oracle/_ref not built: make -C oracle ref")
    env = dict(os.environ, STEREO_RECORD_REF_CALLS="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env))
