"""The corner table of k_shape_curvature on the host (no GPU): evosoro_amd/csrc/curvature_check.cpp is built with the plain C++ compiler and,
for lw_swim6, lw_land6, lw_stiff5 and a full 14^3 cube, lays the table out, checks that no vertex's group straddles a chunk and that every
facet corner is there exactly once, and requires the angle excess evaluated through the table -- the kernel's order of operations -- to be
mesh_angle_excess's bit for bit, in the rest state and in a deformed one."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    """the check program, built and run once for the module"""
    out = tmp_path_factory.mktemp("curvature_check")
    subprocess.check_call(["make", "-C", CSRC, "curvature_check", "CHECK_OUT=%s" % out], stdout=subprocess.DEVNULL)
    run = subprocess.run([str(out / "curvature_check"), GOLDEN], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


@pytest.mark.parametrize("robot, vertices", [("lw_swim6", 323), ("lw_land6", 314), ("lw_stiff5", 189), ("cube14", 1178)])
def test_the_table_gives_the_hosts_angle_excess_bit_for_bit(check_output, robot, vertices):
    line = [l for l in check_output.splitlines() if l.startswith("curvature_check %s:" % robot)]
    assert len(line) == 1 and "%d vertices" % vertices in line[0] and line[0].endswith("rest and deformed state bit-equal: ok"), check_output


def test_robots_without_a_table_are_refused(check_output):
    assert "curvature_check: four robots, two refusals: ok" in check_output
