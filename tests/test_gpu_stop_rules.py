"""StopConditionType 4-7 (total energy constant, kinetic energy low, largest move small, largest move below the floor threshold or time up)
against the reference: tests/golden/vxa/stoprule_*.vxa, the reference's result files and step counts beside them
(tests/golden/make_stoprule_golden.py: every fixture stops at the same step when GravAcc moves by one ulp, so the count is held exactly).
The 2x2x2 and 3x3x3 blocks take the wide kernel's STATS instance (the resident kernel's 256-thread one on the suite's "narrow" path), the
9x9x9 block the resident kernel's 768-thread one; with the option fused = 0 the streaming kernels step them (k_stream_stats)."""
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["stoprule_ke2", "stoprule_move2", "stoprule_floor2", "stoprule_time2", "stoprule_tote3", "stoprule_move9"]


def _run(golden_dir, names, pieces=(), tmp_path=None, reset_first=False, options=()):
    """per robot (result, final state, result file) of one batch; pieces: step counts of vxh_step calls in front of vxh_run"""
    from evosoro_amd import engine
    with engine.Engine(engine.VOXCAD, 0) as eng:
        for key, val in options:
            eng.set_option(key, val)
        for n in names:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        if reset_first:
            eng.step(7000)
            eng.reset()
        for k in pieces:
            eng.step(k)
        eng.run()
        out = []
        for i, n in enumerate(names):
            xml = None
            if tmp_path is not None:
                eng.write_result_xml(i, str(tmp_path / (n + ".xml")))
                xml = (tmp_path / (n + ".xml")).read_text()
            out.append((eng.result(i).as_dict(), eng.state(i), xml))
        return out


# (one run per kernel path, shared by every test below.  Not a module-scoped fixture: conftest's kernel_path, which sets the engine options
# through the environment, is function-scoped, and a wider fixture cannot depend on it.)
_BATCH = {}


@pytest.fixture
def batch(golden_dir, tmp_path_factory, kernel_path):
    """the six fixtures as one batch, run once per kernel path of the suite (shared, never changed).  Under these rules "tiles3" is "auto":
    such robots are never tiled."""
    if kernel_path not in _BATCH:
        _BATCH[kernel_path] = dict(zip(NAMES, _run(golden_dir, NAMES, tmp_path=tmp_path_factory.mktemp("stoprules"))))
    return _BATCH[kernel_path]


@pytest.fixture(scope="module")
def expected_steps(golden_dir):
    return json.load(open(os.path.join(golden_dir, "expected", "stoprule_steps.json")))


@pytest.mark.parametrize("name", NAMES)
def test_the_robot_stops_at_the_reference_step_with_the_reference_tags(batch, golden_dir, expected_steps, name):
    res, _, xml = batch[name]
    print("%s: %d steps (reference %d), status %d" % (name, res["steps"], expected_steps[name], res["status"]))
    assert res["status"] == 1 and res["steps"] == expected_steps[name]
    ref = open(os.path.join(golden_dir, "expected", name + ".xml")).read()
    tags = re.findall(r"<(\w+)>([-+.\deE]+)</\1>", ref)
    assert len(tags) >= 16
    for tag, value in tags:         # every numeric tag as printed: six significant digits
        got = re.search(r"<%s>(.*?)</%s>" % (tag, tag), xml).group(1)
        assert float(got) == float(value), (tag, got, value)


@pytest.mark.parametrize("reset_first", [False, True], ids=["fresh", "after_reset"])
@pytest.mark.parametrize("name", ["stoprule_move2", "stoprule_tote3", "stoprule_move9"])
def test_steps_in_pieces_across_launch_boundaries_equal_one_run(batch, golden_dir, name, reset_first):
    """5000 steps (inside a launch of 1024), 4500 more (the sampled history reaches back over both calls), then the rest"""
    res, state, _ = _run(golden_dir, [name], pieces=(5000, 4500), reset_first=reset_first)[0]
    assert res["steps"] == batch[name][0]["steps"]
    assert np.array_equal(state, batch[name][1])


@pytest.mark.parametrize("name", ["stoprule_ke2", "stoprule_time2", "stoprule_move9"])
def test_a_robot_alone_gives_the_bits_it_gives_in_the_batch(batch, golden_dir, name):
    res, state, _ = _run(golden_dir, [name])[0]
    assert res["steps"] == batch[name][0]["steps"] and np.array_equal(state, batch[name][1])


@pytest.mark.parametrize("name", ["stoprule_move9", "stoprule_tote3"])
def test_the_streaming_kernels_stop_at_the_same_step(golden_dir, expected_steps, name):
    """option fused = 0: k_step_begin_stats / k_bonds_stats / k_voxels / k_stream_stats (the 9x9x9 block; the 3x3x3 one for the strain energy)"""
    res = _run(golden_dir, [name], options=(("fused", 0),))[0][0]
    print("%s streamed: %d steps (reference %d), status %d" % (name, res["steps"], expected_steps[name], res["status"]))
    assert res["status"] == 1 and res["steps"] == expected_steps[name]
