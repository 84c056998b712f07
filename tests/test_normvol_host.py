"""<NormDistByVol> on the host (no GPU): evosoro_amd/csrc/normvol_check.cpp is built with the plain C++ compiler and checks the reader
(the four normvol fixtures, the refused combinations and their messages), the sums of the result file against the reference's own files
(tests/golden/expected/normvol_*.xml, written by tests/golden/make_normvol_golden.py) and the trace ranges assemble_batch lays out."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def normvol_output(tmp_path_factory):
    """the check program, built and run once for the module"""
    out = tmp_path_factory.mktemp("normvol_check")
    subprocess.check_call(["make", "-C", CSRC, "normvol_check", "CHECK_OUT=%s" % out], stdout=subprocess.DEVNULL)
    run = subprocess.run([str(out / "normvol_check"), GOLDEN], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_the_reader_accepts_the_fixtures_and_refuses_the_undefined_combinations(normvol_output):
    assert "reader: four fixtures read, six refusals: ok" in normvol_output


def test_the_result_function_reproduces_the_reference_files(normvol_output):
    """from the printed <CMTrace> / <VolumeTrace> points: the life sum against NormFinalDist + NormFrozenDist within what six printed digits
    of the input allow, NormRegimeDist of the robots without an after-life, 0 for an empty trace, the trace blocks as text"""
    assert "sums: four reference files reproduced: ok" in normvol_output
    assert normvol_output.count("life sum") == 4


def test_a_batch_has_three_trace_ranges_per_robot_with_the_option_and_none_without(normvol_output):
    assert "ranges: 5 robots" in normvol_output and "entries: ok" in normvol_output
