"""GPU tests (-m gpu) of the MEDIUM size class of the multi-workgroup kernel (engine option tile_medium; evosoro_amd/csrc/kernels_tiled.hpp):
robots whose tiles own 65-128 voxels take instances with compile-time LDS strides, the voxels on two wavefronts and the bond entries in
registers.  Same device functions on the same operands in the same order as the generic instances: the class must not show in the bits."""
import os
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STEPS = 350


def _case(name):
    """material, per-voxel layers, variant, fluid, tiles per robot, the class its launch must take with the option on"""
    from evosoro_amd import workloads
    rng = np.random.RandomState(31)
    soft = lambda mat: np.where(mat == 2, 1, mat)      # (without bone a block sags onto the floor: the contact lists are rebuilt on the way)
    block = soft(workloads.full_material(10, 1)[:, :, :5])
    if name == "block":            # (a) 10x10x5 in four tiles of 5x5x5 = 125 voxels
        return block, None, 0, False, 4, "MEDIUM"
    if name == "stiffness":        # (b) ... with per-voxel evolved <Stiffness>: class tables beyond 32 KB stay in memory (TABG)
        return block, OrderedDict([("<Stiffness>", np.round(10 ** rng.uniform(6.0, 7.7, size=(10, 10, 5)), 0))]), 0, False, 4, "MEDIUM"
    if name in ("land", "fluid"):  # (c), (d) a land_water lattice in four slabs of 72 voxels, on land (MESH) and in a fluid (FLUID)
        return workloads.full_material(8, 3)[:6, :6], OrderedDict([("<PhaseOffset>", np.round(rng.uniform(-1, 1, size=(6, 6, 8)), 3))]), 1, name == "fluid", 4, "MEDIUM"
    mat = np.zeros((8, 8, 5), dtype=np.int64)
    mat[:, :, :4] = soft(workloads.full_material(8, 2)[:, :, :4])
    if name == "own128":           # (e) two tiles of exactly VXH_TILE_M_OWN = 128 voxels
        return mat, None, 0, False, 2, "MEDIUM"
    mat[3, 3, 4] = 3               # the class boundary: one voxel more, tiles of 128 and 129, the generic instances
    return mat, None, 0, False, 2, "GENERIC"


@pytest.mark.parametrize("name", ["block", "stiffness", "land", "fluid", "own128", "own129"])
def test_the_size_class_does_not_show_in_the_bits(name, tmp_path, monkeypatch, capfd, kernel_path):
    if kernel_path != "auto":
        pytest.skip("the test sets the kernel options itself")
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    mat, layers, variant, fluid, tiles, want_class = _case(name)
    env = Env()
    if fluid:
        env.add_param("fluid_environment", 1, "<FluidEnvironment>")
    os.makedirs(tmp_path / "voxelyzeFiles")
    write_voxelyze_file(Sim(dt_frac=0.9, simulation_time=0.5, fitness_eval_init_time=0.002), env, workloads.make_individual(0, mat, layers), str(tmp_path), "m")
    path = str(tmp_path / "voxelyzeFiles" / "m--id_00000.vxa")
    monkeypatch.setenv("VXH_PROF_TILES", "1")                     # (the planner names the class of every tile launch on stderr)
    runs = []
    for medium in (0, 1):
        with eng_mod.Engine(variant, 0) as eng:
            for key, val in (("tiled", 2), ("tiles_per_robot", tiles), ("tile_medium", medium)):
                eng.set_option(key, val)
            eng.add_vxa_file(path)
            eng.step(STEPS)
            assert eng.counters().dominant_block == 1              # (k_tile_steps stepped it)
            assert "class=%s" % (want_class if medium else "GENERIC") in capfd.readouterr().err
            runs.append((eng.state(0), eng.result(0).as_dict(), eng.result(0).col_rebuilds))
    (off_state, off_result, _), (state, result, rebuilds) = runs
    assert np.array_equal(state, off_state) and result == off_result
    if name == "block":
        osim = vo.OracleSim.from_vxa(path)
        osim.step(STEPS)
        assert rebuilds >= 2 and osim.info().col_rebuilds == rebuilds      # (a broad-phase run inside the run, beyond the one of the first step)
        assert np.abs(state[:, :3] - osim.state()[:, :3]).max() / osim.model["lattice_dim"] < 1e-9


def test_tile_medium_is_a_kernel_choice_flag(golden_dir, kernel_path):
    """refused values; once a step has been taken only the value it has; after a reset both again"""
    if kernel_path != "auto":
        pytest.skip("the test sets the kernel options itself")
    from evosoro_amd import engine as eng_mod

    def status(eng, val):
        try:
            eng.set_option("tile_medium", val)
        except eng_mod.VxhError as e:
            return e.status
        return 0

    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "rand6_col.vxa"))
        assert [status(eng, v) for v in (2, -1, 0.5, float("nan"), 1, 0)] == [-1, -1, -1, -1, 0, 0]
        eng.step(1)
        assert status(eng, 1) == -6 and status(eng, 0) == 0
        eng.reset()
        assert [status(eng, v) for v in (1, 0)] == [0, 0]
