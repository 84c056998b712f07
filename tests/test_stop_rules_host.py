"""StopConditionType 4-7 on the host (no GPU): evosoro_amd/csrc/stoprule_check.cpp is built with the plain C++ compiler and checks what the
reader accepts (4-7 in _voxcad) and refuses with which message (8 and above, equilibrium mode, the land_water simulator)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """the check program, built and run once for the module"""
    out = tmp_path_factory.mktemp("stoprule_check")
    subprocess.check_call(["make", "-C", CSRC, "stoprule_check", "CHECK_OUT=%s" % out], stdout=subprocess.DEVNULL)
    run = subprocess.run([str(out / "stoprule_check"), GOLDEN], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_the_reader_accepts_rules_4_to_7_and_refuses_the_rest_by_name(check_output):
    assert "reader: rules 4-7 read, four refusals: ok" in check_output

