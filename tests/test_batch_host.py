"""Batch assembly and launch planning (evosoro_amd/csrc/batch.cpp) checked on the host: csrc/batch_check.cpp is built with the plain
C++ compiler (no HIP, no GPU), assembles the golden robots of a variant as one batch under several option sets and compares every
table it unpacks -- bond schedules, wide lists, exclusion rows, tiles, launch groups, masks -- with the robots' models."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "vxa")

BATCHES = [
    (0, ["rand6_col", "rand6_nocol", "cfg1_00", "bench10_0", "devo4", "stiff5", "cfg4_full20"]),   # cfg4_full20: above 1024 voxels, tiled by default
    (1, ["lw_land6", "lw_swim6", "lw_swim10", "lw_stiff5"]),
]


def test_batch_tables_and_launch_plan_are_consistent(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "batch_check", "CHECK_OUT=%s" % tmp_path], stdout=subprocess.DEVNULL)
    for variant, names in BATCHES:
        run = subprocess.run([str(tmp_path / "batch_check"), str(variant), "256"] + [os.path.join(GOLDEN, n + ".vxa") for n in names],
                             capture_output=True, text=True)
        assert run.returncode == 0, "variant %d: %s%s" % (variant, run.stdout, run.stderr)
        assert run.stdout.count(": ok") == 6, run.stdout      # one line per option set
