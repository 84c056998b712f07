"""Dispatch of the resident kernel's robots by measured cost (evosoro_amd/csrc/dispatch_order.hpp, kernels_order.hpp): every launch of a
k_robot_steps group leaves what each robot cost and whether it is due for a broad-phase run; the next launch hands the robots to its
workgroups longest first (more than 128 steps) or due robots first (up to 128).  The robots do not interact, so the order must be
invisible: every robot steps exactly once per launch, whatever the launch lengths, the list length, the robots that stop on the way --
states bit for bit those of one long call and of the list order (engine option dispatch_order = 0)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_mod():
    from evosoro_amd import engine
    return engine


def _write_robot(tmp_path, ident, material, sim, env, name):
    from evosoro_amd import workloads
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles", exist_ok=True)
    write_voxelyze_file(sim, env, workloads.make_individual(ident, material), str(tmp_path), name)
    return str(tmp_path / "voxelyzeFiles" / ("%s--id_%05i.vxa" % (name, ident)))


def _colliding_robots(tmp_path, sim_of=None):
    """70 colliding random 10^3 robots of more than 512 voxels each (a list that does not fill its last 64-entry word)"""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    env = Env()
    paths = []
    for k in range(70):
        sim = sim_of(k) if sim_of else Sim(dt_frac=0.9, simulation_time=0.2, fitness_eval_init_time=0.004)
        paths.append(_write_robot(tmp_path, k, workloads.random_material((10, 10, 10), 9100 + k, p_empty=0.25 + 0.002 * k), sim, env, "dc"))
    return paths


def _run(eng_mod, paths, options, pieces, block):
    """states, broad-phase runs and step counts of every robot after stepping `pieces` (None: to the end)"""
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for key, val in options.items():
            eng.set_option(key, val)
        for p in paths:
            eng.add_vxa_file(p)
        for n in pieces:
            if n is None:
                eng.run()
            else:
                eng.step(n)
            if n != 0:
                assert eng.counters().dominant_block == block
        res = [eng.result(i) for i in range(len(paths))]
        return [eng.state(i) for i in range(len(paths))], [r.col_rebuilds for r in res], [r.steps for r in res]


def _same(a, b):
    assert a[1] == b[1] and a[2] == b[2]
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)


def test_launch_lengths_change_nothing(eng_mod, tmp_path, kernel_path):
    """launches of 1 to 300 steps, on both sides of the former 128-step boundary, ordered by the measurements of the launch before them"""
    if kernel_path != "auto":
        pytest.skip("resident kernels: the default path")
    paths = _colliding_robots(tmp_path)
    pieces = [1, 3, 25, 25, 130, 116, 300]
    whole = _run(eng_mod, paths, {"tiled": 0}, [600], 768)
    ordered = _run(eng_mod, paths, {"tiled": 0}, pieces, 768)
    listed = _run(eng_mod, paths, {"tiled": 0, "dispatch_order": 0}, pieces, 768)
    assert whole[2] == [600] * len(paths) and max(whole[1]) >= 2          # (the broad-phase term of the key was exercised)
    _same(ordered, whole)
    _same(listed, whole)


@pytest.mark.parametrize("count", [800, 65])
def test_many_small_robots(eng_mod, tmp_path, kernel_path, count):
    """a list longer than any workgroup (800: four workgroups of the ordering kernel, the last one partly filled) and one that ends one
    entry into its second 64-entry word, on k_robot_steps<256>"""
    if kernel_path != "auto":
        pytest.skip("resident kernels: the default path")
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    sim, env = Sim(dt_frac=0.9, simulation_time=0.2, fitness_eval_init_time=0.004), Env()
    paths = [_write_robot(tmp_path, k, workloads.random_material((4, 4, 4), 700 + k, p_empty=0.1 + 0.0002 * k), sim, env, "ds") for k in range(count)]
    opts = {"tiled": 0, "wide": 0}
    whole = _run(eng_mod, paths, opts, [100], 256)
    ordered = _run(eng_mod, paths, opts, [7, 64, 29], 256)
    assert whole[2] == [100] * count
    _same(ordered, whole)
    # ... and launches long enough to be ordered by measured cost (more than 128 steps: k_dispatch_order over the whole list)
    _same(_run(eng_mod, paths, opts, [7, 150, 143], 256), _run(eng_mod, paths, opts, [300], 256))


@pytest.mark.parametrize("per_launch", [64, 150])
def test_robots_that_stop_on_the_way(eng_mod, tmp_path, kernel_path, per_launch):
    """a third of the robots reach their stop condition inside the second of three launches: a robot stepped twice in a launch, or not at
    all, ends with another step count.  Launches of 64 steps (flagged robots first) and of 150 (ordered by measured cost: the third
    launch is ordered with the stopped robots' cost words, key 0)"""
    if kernel_path != "auto":
        pytest.skip("resident kernels: the default path")
    from evosoro_amd.base import Sim
    long_sim = Sim(dt_frac=0.9, simulation_time=0.2, fitness_eval_init_time=0.004)
    probe = _colliding_robots(tmp_path / "probe")
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for p in probe:
            eng.add_vxa_file(p)
        dt = [eng.dims(i)["dt"] for i in range(len(probe))]
    # every third robot stops 6 .. 52 steps into the second launch (StopConditionType 2: simulated time), the others after the three launches
    stop_after = lambda k: per_launch + 6 + 2 * (k % 24)
    paths = _colliding_robots(tmp_path / "mixed", lambda k: long_sim if k % 3 else Sim(dt_frac=0.9, simulation_time=dt[k] * stop_after(k), fitness_eval_init_time=0.004))
    opts = {"tiled": 0, "steps_per_launch": per_launch}
    ordered = _run(eng_mod, paths, opts, [3 * per_launch], 768)
    listed = _run(eng_mod, paths, dict(opts, dispatch_order=0), [3 * per_launch], 768)
    inside_second = sum(1 for s in listed[2] if per_launch < s <= 2 * per_launch)
    assert 20 <= inside_second <= 26 and sum(1 for s in listed[2] if s == 3 * per_launch) == len(paths) - inside_second, listed[2]
    _same(ordered, listed)


def test_one_robot_and_a_call_without_steps(eng_mod, tmp_path, kernel_path):
    """the degenerate lengths: a group of one robot, and a call of 0 remaining steps between two ordered launches, short ones (flags) and
    long ones (a permutation of one entry)"""
    if kernel_path != "auto":
        pytest.skip("resident kernels: the default path")
    paths = _colliding_robots(tmp_path)[:1]
    whole = _run(eng_mod, paths, {"tiled": 0}, [60], 768)
    ordered = _run(eng_mod, paths, {"tiled": 0}, [20, 0, 20, 0, 20], 768)
    assert whole[2] == [60]
    _same(ordered, whole)
    _same(_run(eng_mod, paths, {"tiled": 0}, [20, 0, 140, 0, 150], 768), _run(eng_mod, paths, {"tiled": 0}, [310], 768))
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:          # ... and 0 steps left because every robot has finished
        eng.set_option("tiled", 0)
        eng.add_vxa_file(paths[0])
        eng.set_option("steps_per_launch", 500)
        eng.run()
        done = eng.result(0).steps
        eng.step(10)
        assert eng.result(0).steps == done and eng.result(0).status == eng_mod.ROBOT_FINISHED
