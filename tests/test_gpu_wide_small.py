"""Option wide_small: k_robot_wide<256, MESH, TABG> for robots of up to 128 voxels, LDS sized by the robot, several workgroups per CU.
The instances run the 512-thread instances' device functions on the same operands in the same order, so a robot's state bytes are those it
leaves with the option off; which robots take them is a rule of the robot and the options alone (batch.cpp wide_small).  The kernel-path
matrix of conftest.py is overridden: every run here sets the kernel-choice options itself."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
from test_gpu_parity import FLOOR_VOX, _pos_err, _spread

pytestmark = pytest.mark.gpu

STEPS = 2500      # launches of 1024 steps: two launch boundaries; the IniCM latch at 0.05 s (step 110 to 780, by the robot's dt) lies in the first


def _lattice(shape, keep=None):
    """bone (2) and muscle (3) in a checkerboard: several bond classes, actuation, the small dt of the stiff material; keep: voxels kept, in x-fastest order"""
    mat = 2 + np.indices(shape).sum(axis=0) % 2
    if keep is not None:
        flat = mat.reshape(-1, order="F")
        flat[keep:] = 0
        mat = flat.reshape(shape, order="F")
    return mat


def _robot(kind):
    from evosoro_amd import workloads
    if kind == "swimmer":         # land_water, in a fluid: MESH instance
        return workloads.swimmer(0, (5, 5, 5), 11)
    if kind == "stiffness":       # per-voxel evolved <Stiffness> on a full 5x5x5: 125 voxel classes, 13 KB of tables; with contact rows of 24 partners (28 KB)
                                  # pose tile, records, rows and tables pass the 80 KB share of the LDS and the tables stay in memory: TABG instance
        rng = np.random.RandomState(5)
        return workloads.make_individual(0, _lattice((5, 5, 5)), OrderedDict([("<Stiffness>", np.round(10 ** rng.uniform(6.0, 7.7, size=(5, 5, 5)), 0))]))
    shape, keep = {"1": ((1, 1, 1), None), "2x1x1": ((2, 1, 1), None), "4x4x4": ((4, 4, 4), None), "5x5x5": ((5, 5, 5), None), "8x4x4": ((8, 4, 4), None),
                   "129": ((9, 4, 4), 129)}[kind]
    return workloads.make_individual(0, _lattice(shape, keep))


def _run(tmp_path, kinds, wide_small, steps=STEPS, col_cap=0):
    """the robots as one batch for `steps` steps: (states, step counts, voxel counts, dominant_block, their .vxa paths)"""
    from evosoro_amd import engine
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    water = kinds[0] == "swimmer"
    env = Env()
    if water:
        env.add_param("fluid_environment", 1, "<FluidEnvironment>")
        env.add_param("aggregate_drag_coefficient", 750.0, "<AggregateDragCoefficient>")
    sim = Sim(dt_frac=0.9, simulation_time=2.0, fitness_eval_init_time=0.05)      # (the 2 x 1 x 1 robot's dt is the largest: 2500 steps are 1.1 s)
    paths = {}
    os.makedirs(tmp_path / "voxelyzeFiles", exist_ok=True)
    for kind in set(kinds):
        write_voxelyze_file(sim, env, _robot(kind), str(tmp_path), kind)
        paths[kind] = str(tmp_path / "voxelyzeFiles" / ("%s--id_00000.vxa" % kind))
    with engine.Engine(engine.VOXCAD_LAND_WATER if water else engine.VOXCAD, 0) as eng:
        for key, val in (("tiled", 1), ("tiles_per_robot", 0), ("wide", 1), ("wide_two_tiles", 1), ("col_cap", col_cap), ("wide_small", wide_small)):
            eng.set_option(key, val)
        eng.add_vxa_files([paths[k] for k in kinds])
        eng.step(steps)
        n = len(kinds)
        return ([eng.state(i) for i in range(n)], [eng.result(i).steps for i in range(n)], [eng.dims(i)["nvox"] for i in range(n)],
                eng.counters().dominant_block, [paths[k] for k in kinds])


def _prof_lines(capfd):
    """the launches of the wide kernel as VXH_PROF_WIDE reports them: (block, mesh, tabg, workgroups per CU)"""
    return [tuple(int(x) for x in m) for m in re.findall(r"wide launch block=(\d+) mesh=(\d+) tabg=(\d+) .* (\d+) workgroups per CU", capfd.readouterr().err)]


@pytest.mark.parametrize("kind, nvox, block, mesh, tabg", [("1", 1, 257, 0, 0), ("2x1x1", 2, 257, 0, 0), ("4x4x4", 64, 257, 0, 0), ("5x5x5", 125, 257, 0, 0),
                                                           ("8x4x4", 128, 257, 0, 0), ("129", 129, 513, 0, 0), ("swimmer", None, 257, 1, 0),
                                                           ("stiffness", 125, 257, 0, 1)])
def test_state_bytes_are_those_of_the_512_thread_instances(tmp_path, monkeypatch, capfd, kind, nvox, block, mesh, tabg):
    monkeypatch.setenv("VXH_PROF_WIDE", "1")
    col_cap = 24 if kind == "stiffness" else 0
    want, steps0, _, block0, _ = _run(tmp_path, [kind], 0, col_cap=col_cap)
    capfd.readouterr()
    got, steps1, nv, block1, _ = _run(tmp_path, [kind], 1, col_cap=col_cap)
    launches = _prof_lines(capfd)
    print(kind, "voxels", nv, "steps", steps1, "dominant_block", block0, block1, "launches", launches)
    assert (nvox is None and 0 < nv[0] <= 128) or nv[0] == nvox
    assert steps0 == steps1 == [STEPS]
    assert block0 == 513 and block1 == block
    assert launches and all(l[:3] == (block - 1, mesh, tabg if block == 257 else 0) for l in launches)
    assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("kind", ["5x5x5", "swimmer"])
def test_early_steps_match_the_oracle(tmp_path, kind):
    """the comparison and the bar of test_early_steps_match_oracle (tests/test_gpu_parity.py)"""
    from oracle import vxoracle as vo
    variant = 1 if kind == "swimmer" else 0
    sim = model = None
    for upto in (1, 2, 10, 50, 200):
        states, _, _, block, paths = _run(tmp_path, [kind], 1, steps=upto)
        assert block == 257
        if sim is None:
            model = vo.parse_vxa(paths[0], variant)
            sim, spread = vo.OracleSim(model), _spread(model, (50, 100, 200, 300, 400))
        sim.step(upto - sim.info().steps)
        want, got, lat = sim.state(), states[0], model["lattice_dim"]
        tol = FLOOR_VOX if upto <= 10 else max(FLOOR_VOX, 20 * spread[0])
        qtol = 1e-9 if upto <= 10 else max(1e-9, 20 * spread[1])
        print(kind, upto, "position error", _pos_err(got, want, lat), "bar", tol)
        assert _pos_err(got, want, lat) <= tol
        assert np.abs(got[:, 3:7] - want[:, 3:7]).max() <= qtol
        assert np.abs(got[:, 7] - want[:, 7]).max() / lat < 1e-12


def test_several_robots_per_cu_each_with_the_bytes_it_has_alone(tmp_path, monkeypatch, capfd):
    kinds = ["4x4x4", "5x5x5", "8x4x4"]
    alone = [_run(tmp_path, [k], 1, steps=300)[0][0] for k in kinds]
    n_cu = 256        # (MI355X)
    monkeypatch.setenv("VXH_PROF_WIDE", "1")
    capfd.readouterr()
    states, _, _, block, _ = _run(tmp_path, kinds * n_cu, 1, steps=300)
    launches = _prof_lines(capfd)
    print("CUs", n_cu, "robots", len(states), "launches", launches)
    assert block == 257 and launches and all(l[0] == 256 and l[3] >= 2 for l in launches)
    assert all(np.array_equal(s, alone[i % 3]) for i, s in enumerate(states))


def test_a_robot_whose_contact_rows_pass_the_budget_keeps_the_512_thread_instance(tmp_path):
    """dense 8x4x4 (104 surface voxels) with col_cap = 64: rows of 104 x 64 x 12 B = 78 KB on top of 49 KB of tile and records"""
    want, _, _, block0, _ = _run(tmp_path, ["8x4x4"], 0, col_cap=64)
    got, steps, _, block1, _ = _run(tmp_path, ["8x4x4"], 1, col_cap=64)
    assert steps == [STEPS] and block0 == 513 and block1 == 513
    assert np.array_equal(got[0], want[0])
