"""Batch assembly and launch planning (evosoro_amd/csrc/batch.cpp) checked on the host: csrc/batch_check.cpp is built with the plain
C++ compiler (no HIP, no GPU), assembles the golden robots of a variant as one batch under several option sets and compares every
table it unpacks -- bond schedules, wide lists, exclusion rows, tiles, launch groups, masks -- with the robots' models.  Two further modes
check the import pipeline's in-memory route (evosoro_amd/csrc/import.cpp) against the file route and the dominant-kernel choice."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "vxa")

BATCHES = [
    (0, ["rand6_col", "rand6_nocol", "cfg1_00", "bench10_0", "devo4", "stiff5", "cfg4_full20"]),   # cfg4_full20: above 1024 voxels, tiled by default
    (1, ["lw_land6", "lw_swim6", "lw_swim10", "lw_stiff5"]),
]
# --arrays: development layers, evolved stiffness, the mesh
ARRAYS = [
    (0, ["devo4", "stiff5", "rand6_col", "bench10_0"]),
    (1, ["lw_swim6", "lw_stiff5"]),
]


def _vxa(names):
    return [os.path.join(GOLDEN, n + ".vxa") for n in names]


@pytest.fixture(scope="module")
def batch_check(tmp_path_factory):
    """the check program, built once for the module"""
    out = tmp_path_factory.mktemp("batch_check")
    subprocess.check_call(["make", "-C", CSRC, "batch_check", "CHECK_OUT=%s" % out], stdout=subprocess.DEVNULL)
    return str(out / "batch_check")


def test_batch_tables_and_launch_plan_are_consistent(batch_check):
    for variant, names in BATCHES:
        run = subprocess.run([batch_check, str(variant), "256"] + _vxa(names), capture_output=True, text=True)
        assert run.returncode == 0, "variant %d: %s%s" % (variant, run.stdout, run.stderr)
        assert run.stdout.count(": ok") == 6, run.stdout      # one line per option set


def test_robots_handed_over_as_arrays_give_the_batch_their_files_give(batch_check):
    """every file's own lattice and layers through models_from_arrays (what vxh_add_robots takes): the same HostBatch, value for value,
    as the file route; the refusals of that route; of 40 robots with two bad ones the first in index order is reported"""
    for variant, names in ARRAYS:
        run = subprocess.run([batch_check, "--arrays", str(variant)] + _vxa(names), capture_output=True, text=True)
        assert run.returncode == 0, "variant %d: %s%s" % (variant, run.stdout, run.stderr)
        assert run.stdout.count(": ok") == len(names), run.stdout


def test_the_dominant_kernel_of_a_call_follows_its_rule(batch_check):
    """dominant_kernel (batch.cpp) on hand-made calls, one per branch: the tiles win / tie (>=), the best group, the streamed rest wins / ties
    (>), fused = 0, and the other groups together outweighing the tiles"""
    run = subprocess.run([batch_check, "--dominant"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(": ok") >= 7, run.stdout
