#!/usr/bin/env python3
"""Writes the stop-rule fixtures (StopConditionType 4-7): tests/golden/vxa/stoprule_*.vxa with this package's writer, and
tests/golden/expected/stoprule_*.xml + stoprule_steps.json with the reference (oracle/_ref/vxprobe: the reference sources behind the
headless main's own loop; it writes the result file and the number of TimeStep calls, which the file does not carry).  CPU only.

Passive blocks (TempEnabled 0) of fat / bone voxels that settle on the floor under gravity; one robot per rule:
    stoprule_ke2      2x2x2, rule 5 (kinetic energy per voxel)
    stoprule_move2    2x2x2, rule 6 (largest voxel move per step)
    stoprule_floor2   2x2x2, rule 7, ends by motion (MOTION_FLOOR_THR) long before its time bound
    stoprule_time2    the same block, rule 7, ends by time: the bound falls ~1400 steps before the motion test would pass
    stoprule_tote3    3x3x3, rule 4 (total energy).  Its `abs(TotEHistory[i] - IniTotVal)` is the floating-point overload in the reference
                      build: the integer one would truncate every difference of these energies (far below 1 J) to 0 and stop at step
                      9001, the first step without a -1 at a sampled index; the reference stops thousands of steps later
    stoprule_move9    9x9x9, rule 6

A fixture is kept only if (a) the reference stops at the SAME step when <GravAcc> is moved by one ulp, (b) it stops between 9001 and
30000 steps -- at 9001 or later every sampled history entry is a recorded one, none the initial -1 --, and (c) stoprule_tote3 stops
later than 9001 and stoprule_time2 earlier than stoprule_floor2.  main() asserts all three and refuses to write otherwise.
"""
import json
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from evosoro_amd.base import Sim, Env  # noqa: E402
from evosoro_amd.tools import read_write_voxelyze as rw  # noqa: E402
from evosoro_amd import workloads  # noqa: E402

PROBE = os.path.join(REPO, "oracle", "_ref", "vxprobe")
RUN_DIR, RUN_NAME = "golden_run", "golden"     # relative on purpose: it is embedded in <FitnessFileName>
GRAV = "<GravAcc>-9.81</GravAcc>"
GRAV_ULP = "<GravAcc>%r</GravAcc>" % float(np.nextafter(-9.81, 0.0))

# value: <StopConditionValue>; rule 7: the time bound in seconds
CASES = OrderedDict([
    ("stoprule_ke2", dict(ident=70, n=2, rule=5, value=2e-8, seed=1)),
    ("stoprule_move2", dict(ident=71, n=2, rule=6, value=1e-6, seed=2)),
    ("stoprule_floor2", dict(ident=72, n=2, rule=7, value=10.0, seed=3)),
    ("stoprule_time2", dict(ident=73, n=2, rule=7, value=0.61, seed=3)),
    ("stoprule_tote3", dict(ident=74, n=3, rule=4, value=1e-6, seed=5)),
    ("stoprule_move9", dict(ident=75, n=9, rule=6, value=1e-6, seed=6)),
])


def vxa_text(case):
    n = case["n"]
    sim = Sim(self_collisions_enabled=case.get("self_col", False), dt_frac=case.get("dt_frac", 0.9), simulation_time=case["value"],
              stop_condition=case["rule"], fitness_eval_init_time=case.get("init", 0.01))
    env = Env(temp_enabled=0)
    mat = np.random.RandomState(case["seed"]).randint(1, 3, size=(n, n, n + 1)).astype(np.int64)     # fat and bone
    mat[:, :, 0] = 0                                   # an empty bottom layer: the block starts one voxel above the floor
    ind = workloads.make_individual(case["ident"], mat)
    random.seed(12345)
    _, text = rw.write_voxelyze_file(sim, env, ind, RUN_DIR, RUN_NAME, write=False, want_text=True)
    assert text.count(GRAV) == 1
    return text


def reference_run(text, ident, max_steps=60000):
    """(TimeStep calls until StopConditionMet, result file) of the reference for this .vxa; steps == max_steps: it did not stop"""
    work = tempfile.mkdtemp(prefix="stoprule_")
    try:
        for d in ("voxelyzeFiles", "fitnessFiles", "tempFiles"):
            os.makedirs(os.path.join(work, RUN_DIR, d))
        vxa = os.path.join(RUN_DIR, "voxelyzeFiles", "robot.vxa")
        with open(os.path.join(work, vxa), "w") as f:
            f.write(text)
        subprocess.run([PROBE, "-f", vxa, "-o", "trace.bin", "-every", "100000000", "-max", str(max_steps)], cwd=work, check=True,
                       stdout=subprocess.DEVNULL)
        with open(os.path.join(work, "trace.bin"), "rb") as f:
            steps = struct.unpack("<i", f.read()[-4:])[0]
        with open(os.path.join(work, RUN_DIR, "fitnessFiles", "softbotsOutput--id_%05i.xml" % ident)) as f:
            return steps, f.read()
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/vxprobe is missing: make -C oracle ref")
    names = [a for a in sys.argv[1:] if a in CASES] or list(CASES)
    dry = "--dry" in sys.argv

    def one(name):
        case = CASES[name]
        text = vxa_text(case)
        steps, xml = reference_run(text, case["ident"])
        steps_ulp, _ = reference_run(text.replace(GRAV, GRAV_ULP), case["ident"])
        return name, text, steps, steps_ulp, xml

    with ThreadPoolExecutor(max_workers=6) as pool:
        done = list(pool.map(one, names))
    table = OrderedDict()
    for name, text, steps, steps_ulp, xml in done:
        print("%s: %d steps, %d with GravAcc + 1 ulp" % (name, steps, steps_ulp))
        if dry:
            continue
        assert steps == steps_ulp, "%s hangs on the last bits: choose another value" % name
        assert 9001 <= steps <= 30000, "%s: outside 9001..30000 steps" % name
        table[name] = steps
        assert name != "stoprule_tote3" or steps > 9001, "the integer reading of abs() would stop here too"
        assert name != "stoprule_time2" or steps < table["stoprule_floor2"], "the motion test passed first"
        with open(os.path.join(HERE, "vxa", name + ".vxa"), "w") as f:
            f.write(text)
        with open(os.path.join(HERE, "expected", name + ".xml"), "w") as f:
            f.write(xml)
    if not dry and names == list(CASES):
        with open(os.path.join(HERE, "expected", "stoprule_steps.json"), "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
