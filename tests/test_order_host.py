"""The dispatch-order rule of the resident kernel's launch groups (evosoro_amd/csrc/dispatch_order.hpp: the key of a robot for a launch and
the tie-break by list index) checked on the host: csrc/order_check.cpp is built with the plain C++ compiler (no HIP, no GPU) and builds
the order the way k_dispatch_order does, for list lengths 1, 63, 64, 65, 70, 512, 800 and 4096, over seeded random tables, tables full of
ties, all-zero keys, stopped robots and arbitrary bit patterns: always a permutation, non-increasing in key."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "evosoro_amd", "csrc")


@pytest.fixture(scope="module")
def order_check(tmp_path_factory):
    """the check program, built once for the module"""
    out = tmp_path_factory.mktemp("order_check")
    subprocess.check_call(["make", "-C", CSRC, "order_check", "CHECK_OUT=%s" % out], stdout=subprocess.DEVNULL)
    return str(out / "order_check")


def test_dispatch_order_is_a_permutation_sorted_by_key(order_check):
    run = subprocess.run([order_check], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout and "violations" not in run.stdout, run.stdout
