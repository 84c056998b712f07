"""GPU tests (-m gpu) of the multi-workgroup kernel (evosoro_amd/csrc/kernels_tiled.hpp): a robot's trajectory must not
depend on whether, or into how many tiles, it was cut -- the tiled kernel evaluates every bond and voxel with the resident
kernel's arithmetic and sums in its order -- and must match the CPU oracle like every other path.  (The parity tests of
tests/test_gpu_parity.py also run on this kernel: see `kernel_path` in conftest.py.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAND = ["probe6", "rand6_nocol", "rand6_col", "soft5_init0", "stiff5", "grow5", "devo4"]


def _states(eng_mod, paths, options, checkpoints, variant=0):
    out = []
    with eng_mod.Engine(variant, 0) as eng:
        for key, val in options.items():
            eng.set_option(key, val)
        for p in paths:
            eng.add_vxa_file(p)
        done = 0
        for upto in checkpoints:
            eng.step(upto - done)
            done = upto
            out.append([eng.state(i) for i in range(len(paths))])
    return out


def test_tiling_does_not_change_the_trajectory(golden_dir):
    from evosoro_amd import engine as eng_mod
    paths = [os.path.join(golden_dir, "vxa", n + ".vxa") for n in LAND]
    checkpoints = (1, 7, 300, 900)            # 900 steps: past InitCmTime for most robots, launches of 256 steps chained
    ref = _states(eng_mod, paths, {"tiled": 0, "wide": 0}, checkpoints)      # (the resident kernel: the tiled one sums in ITS order)
    bitwise = {}
    for k in (1, 2, 5):
        got = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": k}, checkpoints)
        for c in range(len(checkpoints)):
            for i, name in enumerate(LAND):
                err = np.abs(got[c][i][:, :8] - ref[c][i][:, :8]).max()
                assert err < 1e-12, (k, checkpoints[c], name, err)
                assert np.abs(got[c][i][:, 8:] - ref[c][i][:, 8:]).max() < 1e-9, (k, checkpoints[c], name)
        bitwise[k] = all(np.array_equal(got[-1][i], ref[-1][i]) for i in range(len(LAND)))
    print("tiled == resident bit for bit after 900 steps, by tile count:", bitwise)
    # different tile counts among themselves: the same bits (same code, same order, only the partition differs)
    a = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 2}, (900,))
    b = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 6}, (900,))
    for i, name in enumerate(LAND):
        assert np.array_equal(a[0][i], b[0][i]), name


def test_tiled_whole_runs_match_the_reference_xml(golden_dir):
    from evosoro_amd import engine as eng_mod
    from oracle import vxoracle as vo
    names = ["probe6", "rand6_col", "soft5_init0"]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 2)
        eng.set_option("tiles_per_robot", 4)
        for n in names:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        eng.run()
        for i, n in enumerate(names):
            trace = vo.read_trace(os.path.join(golden_dir, "expected", n + ".final.bin"))
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", n + ".xml"))
            res = eng.result(i)
            lat = vo.parse_vxa(os.path.join(golden_dir, "vxa", n + ".vxa"))["lattice_dim"]
            assert res.status == eng_mod.ROBOT_FINISHED and res.steps == trace["total_steps"], n
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / lat < 1e-9, n
            assert np.abs(np.array(res.ini_cm) - trace["ini_cm"]).max() / lat < 1e-9, n
            assert abs(res.norm_final_dist - want["NormFinalDist"]) <= 1e-5 * abs(want["NormFinalDist"]) + 2e-9, n


def test_stepping_in_pieces_equals_one_run(golden_dir):
    """launch boundaries (history, mode bits, pending MaxVoxVel, exchange buffers) must be invisible: 1 + 2 + 253 + 300 steps
    in separate calls = 556 steps in one"""
    from evosoro_amd import engine as eng_mod
    paths = [os.path.join(golden_dir, "vxa", n + ".vxa") for n in ("rand6_col", "probe6")]
    opts = {"tiled": 2, "tiles_per_robot": 3, "steps_per_launch": 64}
    pieces = _states(eng_mod, paths, opts, (1, 3, 256, 556))[-1]
    whole = _states(eng_mod, paths, opts, (556,))[-1]
    for a, b in zip(pieces, whole):
        assert np.array_equal(a, b)


def test_kernel_choice_follows_the_robot_alone_unless_tile_small(golden_dir):
    """Default: a robot the resident kernel can take is never tiled, whatever the population -- so its trajectory does not depend on
    the batch, bit for bit (test_full_size_batch_properties).  Option tile_small = 1 lets small populations of LARGE robots (the
    768- and 1024-thread variants) use the tiled kernel: faster there (scripts/dev_gpu_diag.py tilepolicy), equal to 1e-12 voxel,
    not to the bit."""
    from evosoro_amd import engine as eng_mod
    big, small = os.path.join(golden_dir, "vxa", "bench10_0.vxa"), os.path.join(golden_dir, "vxa", "rand6_col.vxa")

    def run(path, options):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 1)                                 # the automatic policy, whatever kernel the test matrix forces
            eng.set_option("tiles_per_robot", 0)                       # (conftest.py: VXH_ENGINE_OPTIONS)
            eng.set_option("wide", 1)
            for key, val in options.items():
                eng.set_option(key, val)
            eng.add_vxa_file(path)
            eng.step(600)
            return eng.state(0), eng.counters().dominant_block        # (dominant_block: 1 = the tiled kernel, else the resident variant)

    big_default, blk = run(big, {})
    assert blk == 768                                                  # a lone 10x10x10 robot: resident by default
    big_small, blk = run(big, {"tile_small": 1})
    assert blk == 1                                                    # ... tiled on request
    assert np.abs(big_small[:, :8] - big_default[:, :8]).max() < 1e-12
    small_default, blk = run(small, {})
    assert blk == 513                                                  # (the wide kernel, k_robot_wide<512>: reported as its workgroup size + 1)
    small_small, blk = run(small, {"tile_small": 1})
    assert blk == 513 and np.array_equal(small_small, small_default)  # small robots are never worth tiling: unchanged
    small_narrow, blk = run(small, {"wide": 0})
    assert blk == 256 and np.abs(small_narrow[:, :8] - small_default[:, :8]).max() < 1e-11   # resident on request: other summation order


def test_one_tiled_robot_inside_a_large_resident_batch(tmp_path):
    """A lattice of more than 1024 voxels (tiled kernel: its tiles wait for each other and must all be on the chip) among hundreds of
    robots of the one-workgroup-per-robot kernels: the tiled launches run after the launch groups, not next to them (a tile launch is
    sized for an empty chip; placed tiles would spin on CUs the other workgroups occupy).  The big robot must come out bit for bit as
    when it is evaluated alone, and so must a small one."""
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.05, fitness_eval_init_time=0.01)
    inds = [workloads.make_individual(0, workloads.full_material(11, 3))] + [workloads.random_robot(1 + i, (6, 6, 6), 50 + i) for i in range(300)]
    paths = []
    for ind in inds:
        write_voxelyze_file(sim, Env(), ind, str(tmp_path), "mix")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("mix--id_%05i.vxa" % ind.id)))

    def run(which):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0); eng.set_option("wide", 1)     # the engine's own policy
            eng.add_vxa_files([paths[i] for i in which])
            eng.step(300)
            assert all(eng.result(k).status in (eng_mod.ROBOT_PENDING, eng_mod.ROBOT_FINISHED) for k in range(len(which)))
            return [eng.state(k) for k in range(len(which))], eng.counters()

    batch, counters = run(list(range(len(paths))))
    assert counters.dominant_block == 513          # most voxel-steps are the small robots' (wide kernel); the 1331-voxel lattice can only be tiled
    big_alone, _ = run([0])
    small_alone, _ = run([17])
    assert np.array_equal(batch[0], big_alone[0])
    assert np.array_equal(batch[17], small_alone[0])


def test_a_timed_out_tiled_call_is_made_again_without_tiling(tmp_path):
    """The tiles of a robot are co-resident workgroups that wait for each other; a second process on the GPU can make them give up
    (VXH_ROBOT_SYNC_TIMEOUT).  A call that started from the imported state is then made again without the tiled kernel instead of
    failing the generation (Engine::advance); the timeout is injected here (VXH_INJECT_TILE_TIMEOUT: the first tiled call reports
    one).  The lattice above 1024 voxels must come out as an engine with tiled = 0 steps it, bit for bit, the small robot next to
    it too.  Round 4: a call in the MIDDLE of a run is repeated as well -- the state before it is gone, but the evaluation is a
    deterministic function of the imported state, so the batch is stepped again from there up to where the call was to end
    (VXH_INJECT_TILE_TIMEOUT=2: the second tiled call, i.e. steps 101-200, reports the timeout)."""
    import subprocess, sys, textwrap
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.03, fitness_eval_init_time=0.01)
    inds = [workloads.make_individual(0, workloads.full_material(11, 3)), workloads.random_robot(1, (6, 6, 6), 51)]
    paths = []
    for ind in inds:
        write_voxelyze_file(sim, Env(), ind, str(tmp_path), "to")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("to--id_%05i.vxa" % ind.id)))
    script = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        from evosoro_amd import engine as e
        paths, mode, out = sys.argv[1:3], sys.argv[3], sys.argv[4]
        with e.Engine(e.VOXCAD, 0) as eng:
            eng.set_option("tiled", 0 if mode == "untiled" else 1)
            eng.add_vxa_files(paths)
            if mode.endswith("2"):
                eng.step(100); eng.step(100)
            else:
                eng.step(200)
            np.save(out, np.concatenate([eng.state(0).ravel(), eng.state(1).ravel()]))
            print("kernel of most voxel-steps:", eng.counters().dominant_block)
    """ % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    prog = tmp_path / "run.py"
    prog.write_text(script)

    def run(mode, inject):
        env = dict(os.environ)
        env.pop("VXH_INJECT_TILE_TIMEOUT", None)
        env.pop("VXH_ENGINE_OPTIONS", None)
        if inject:
            env["VXH_INJECT_TILE_TIMEOUT"] = "2" if mode.endswith("2") else "1"
        out = str(tmp_path / (mode + ("_inj" if inject else "") + ".npy"))
        proc = subprocess.run([sys.executable, str(prog)] + paths + [mode, out], env=env, capture_output=True, timeout=600)
        return proc, (np.load(out) if os.path.exists(out) else None)

    ref_proc, ref = run("untiled", False)
    assert ref_proc.returncode == 0, ref_proc.stderr.decode()[-2000:]
    tiled_proc, tiled = run("tiled", False)
    assert tiled_proc.returncode == 0 and b"stepped again" not in tiled_proc.stderr
    assert not np.array_equal(tiled, ref) and np.abs(tiled - ref).max() < 1e-9       # (the tiled kernel really ran: same trajectory, other last bits)
    inj_proc, inj = run("tiled", True)
    assert inj_proc.returncode == 0, inj_proc.stderr.decode()[-2000:]
    assert b"stepped again without the tiled kernel" in inj_proc.stderr
    assert np.array_equal(inj, ref)
    mid_proc, mid = run("tiled2", True)           # the timeout in the second of two calls
    assert mid_proc.returncode == 0, mid_proc.stderr.decode()[-2000:]
    assert b"stepped again from its imported state without the tiled kernel" in mid_proc.stderr
    assert np.array_equal(mid, ref)


def test_one_step_of_the_full_20_cube_from_the_same_state(tmp_path):
    """BASELINE configs[4] at its full size on the tiled kernel (125 tiles of 64 voxels with the engine's own tile count): what ONE step
    of the engine and of the oracle differ by when both start from the same state (tests/test_gpu_parity.py
    test_one_step_from_the_same_state explains the instrument), over the first 300 steps of the 8000-voxel lattice settling on the floor
    with self-collision on."""
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.05, fitness_eval_init_time=0.01)
    write_voxelyze_file(sim, Env(), workloads.make_individual(0, workloads.full_material(20, 1)), str(tmp_path), "c4")
    path = str(tmp_path / "voxelyzeFiles" / "c4--id_00000.vxa")
    model = vo.parse_vxa(path, 0)
    lat = model["lattice_dim"]
    osim = vo.OracleSim(model)
    worst = [0.0, 0.0, 0.0]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0)
        eng.add_vxa_file(path)
        prev = osim.state()
        for step in range(1, 301):
            eng.step(1)
            got = eng.state(0)
            osim.set_state(prev)
            osim.step(1)
            want = osim.state()
            d = np.abs(got - want)
            worst = [max(worst[0], d[:, :3].max() / lat),
                     max(worst[1], d[:, 8:11].max() / max(1e-300, np.abs(want[:, 8:11]).max())),
                     max(worst[2], d[:, 11:14].max() / max(1e-300, np.abs(want[:, 11:14]).max()))]
            prev = got
        assert eng.counters().dominant_block == 1                 # (k_tile_steps stepped it)
    print("20^3 lattice, one step from the same state, worst over 300 steps: %.1e voxel, velocity %.1e, angular velocity %.1e" % tuple(worst))
    assert worst[0] <= 5e-14 and worst[1] <= 2e-11 and worst[2] <= 2e-11, worst


def test_whole_run_of_the_full_20_cube(tmp_path):
    """... and the whole evaluation of that lattice (781 steps, IniCM latch, stop condition, result record) against the oracle: every
    voxel within 1e-9 voxel at the end, the record's distances to 1e-12 relative."""
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.05, fitness_eval_init_time=0.01)
    write_voxelyze_file(sim, Env(), workloads.make_individual(0, workloads.full_material(20, 1)), str(tmp_path), "c4")
    path = str(tmp_path / "voxelyzeFiles" / "c4--id_00000.vxa")
    model = vo.parse_vxa(path, 0)
    lat = model["lattice_dim"]
    osim = vo.OracleSim(model)
    osim.step(-1)
    info, want_res = osim.info(), osim.result()
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0)
        eng.add_vxa_file(path)
        eng.run()
        res = eng.result(0)
        got = eng.state(0)
        assert eng.counters().dominant_block == 1
    assert res.status == eng_mod.ROBOT_FINISHED and res.steps == info.steps and res.col_rebuilds == info.col_rebuilds
    err = np.abs(got[:, :3] - osim.state()[:, :3]).max() / lat
    print("20^3 lattice, whole run of %d steps: largest voxel position error %.1e voxel" % (res.steps, err))
    assert err <= 1e-9, err
    for f in ("norm_final_dist", "final_dist", "anterior_dist", "posterior_dist"):
        a, b = getattr(res, f), getattr(want_res, f)
        assert abs(a - b) <= 1e-12 * max(1.0, abs(b)) + 1e-15, (f, a, b)


def test_a_land_water_lattice_above_1024_voxels_on_land_is_tiled(tmp_path):
    """Round 4: _voxcad_land_water robots ON LAND (no fluid: no drag mesh to average across tile boundaries) are taken by the tiled kernel;
    its tiles keep the directional strains of their voxels (SetStrainDir), which the RobotVolume tags are computed from.  A full 11^3
    lattice (1331 voxels) with a per-voxel phase offset, next to a small walker: against the oracle step by step; the whole evaluation
    against an engine with tiled = 0 (streaming kernels: the round-3 path of such a robot): every voxel within 1e-9 voxel, the volume
    tags -- functions of poses AND strains -- within 1e-9 relative, and the tiled kernel did step it."""
    from collections import OrderedDict
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.03, fitness_eval_init_time=0.005)
    big = workloads.make_individual(0, workloads.full_material(11, 1),
                                    OrderedDict([("<PhaseOffset>", np.round(np.random.RandomState(59).uniform(-1, 1, size=(11, 11, 11)), 3))]))
    small = workloads.swimmer(1, (6, 6, 6), 77)
    paths = []
    for ind in (big, small):
        write_voxelyze_file(sim, Env(), ind, str(tmp_path), "lw")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("lw--id_%05i.vxa" % ind.id)))
    sims = [vo.OracleSim.from_vxa(p, variant=1) for p in paths]
    lat = sims[0].model["lattice_dim"]
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0)      # (the engine's defaults, whatever kernel path the run is parametrised with)
        eng.add_vxa_files(paths)
        assert eng.dims(0)["nvox"] == 1331
        for upto in (1, 3, 40, 200):
            eng.step(upto - sims[0].info().steps)
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                err = np.abs(eng.state(i)[:, :3] - o.state()[:, :3]).max() / lat
                assert err < 1e-9, (i, upto, err)
        assert eng.counters().dominant_block == 1                  # k_tile_steps did most of the work (the 1331-voxel lattice)
        eng.run()
        tiled_state, tiled_res = eng.state(0), eng.result(0)
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.set_option("tiled", 0)
        eng.add_vxa_files(paths)
        eng.run()
        assert eng.counters().dominant_block == 0                  # streaming kernels
        ref_state, ref_res = eng.state(0), eng.result(0)
    assert tiled_res.status == eng_mod.ROBOT_FINISHED and tiled_res.steps == ref_res.steps
    assert np.abs(tiled_state[:, :3] - ref_state[:, :3]).max() / lat < 1e-9
    for f in ("robot_volume_start", "robot_volume_end", "norm_abs_disp"):
        a, b = getattr(tiled_res, f), getattr(ref_res, f)
        assert b > 0 and abs(a - b) <= 1e-9 * abs(b), (f, a, b)
    assert abs(tiled_res.robot_volume_end - tiled_res.robot_volume_start) > 1e-6 * tiled_res.robot_volume_start      # the strains did reach the host: a deformed mesh


def test_swimmers_on_tiles_do_not_depend_on_the_tiling(golden_dir):
    """Round 5: robots IN A FLUID on the tiled kernel.  Every tile carries the part of the drag mesh its owned voxels have facets on; a
    mesh vertex averages the corners of up to seven voxels -- the tile's own, a neighbour's, or a diagonal neighbour's that is no halo
    voxel -- whose poses AND strains (of the previous step's bonds) come through the exchange buffer.  Same arithmetic and the same
    orders of summation as the resident / wide kernels (fused_drag), so: different tile counts give the same bits; tiled vs the resident
    MESH kernel within 1e-12 voxel; launch boundaries invisible (the strains are published with the poses a launch starts from)."""
    from evosoro_amd import engine as eng_mod
    names = ["lw_swim6", "cfg3_00", "lw_swim10", "lw_hexapus"]
    paths = [os.path.join(golden_dir, "vxa", n + ".vxa") for n in names]
    checkpoints = (1, 5, 200, 700)
    ref = _states(eng_mod, paths, {"tiled": 0, "wide": 0}, checkpoints, variant=1)
    a = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 2}, checkpoints, variant=1)
    b = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 7}, checkpoints, variant=1)
    for c in range(len(checkpoints)):
        for i, name in enumerate(names):
            assert np.array_equal(a[c][i], b[c][i]), (checkpoints[c], name)
            assert np.abs(a[c][i][:, :8] - ref[c][i][:, :8]).max() < 1e-12, (checkpoints[c], name)
    pieces = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 4, "steps_per_launch": 64}, (1, 3, 256, 700), variant=1)[-1]
    whole = _states(eng_mod, paths, {"tiled": 2, "tiles_per_robot": 4, "steps_per_launch": 64}, (700,), variant=1)[-1]
    for x, y in zip(pieces, whole):
        assert np.array_equal(x, y)
    # the automatic policy with tile_small: a lone 709-voxel swimmer (768-thread class) is tiled -- in a fluid too
    small = _states(eng_mod, [paths[2]], {"tiled": 1, "tiles_per_robot": 0, "tile_small": 1}, (300,), variant=1)[0][0]
    lone = _states(eng_mod, [paths[2]], {"tiled": 0, "wide": 0}, (300,), variant=1)[0][0]
    assert np.abs(small[:, :8] - lone[:, :8]).max() < 1e-12
    with eng_mod.Engine(1, 0) as eng:
        eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0); eng.set_option("tile_small", 1)
        eng.add_vxa_file(paths[2])
        eng.step(10)
        assert eng.counters().dominant_block == 1
    with eng_mod.Engine(1, 0) as eng:          # (and the tiled kernel is what stepped them)
        eng.set_option("tiled", 2); eng.set_option("tiles_per_robot", 4)
        eng.add_vxa_file(paths[1])
        eng.step(10)
        assert eng.counters().dominant_block == 1


def test_a_tile_kernel_that_needs_scratch_is_refused_before_it_is_launched(golden_dir, monkeypatch):
    """Round 6 (the round-5 review's task 5): the round-5 abort of the FLUID tile kernel was a build with ~500 bytes of scratch per lane whose
    granule stores took their addresses from scratch slots filled under a narrower lane mask (rocgdb: a memory access fault at the first
    step).  k_tile_steps now keeps nothing in scratch -- four wavefronts, 512 registers each -- and every launch checks it
    (hipFuncGetAttributes, launch_tiled.hip): with the tolerated size forced below zero the call comes back as VXH_ERR_HIP with a message,
    nothing is launched, and the engine is still usable once the limit is back."""
    from evosoro_amd import engine as eng_mod
    path = os.path.join(golden_dir, "vxa", "rand6_col.vxa")
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 2)
        eng.set_option("tiles_per_robot", 3)
        eng.add_vxa_file(path)
        monkeypatch.setenv("VXH_TILE_SCRATCH_LIMIT", "-1")
        with pytest.raises(eng_mod.VxhError) as err:
            eng.step(10)
        assert "scratch" in str(err.value) and "status -5" in str(err.value)          # VXH_ERR_HIP
        monkeypatch.delenv("VXH_TILE_SCRATCH_LIMIT")
        eng.reset()
        eng.step(10)                            # (the product build: 0 bytes, launched)
        tiled = eng.state(0)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 0)
        eng.set_option("wide", 0)
        eng.add_vxa_file(path)
        eng.step(10)
        assert np.abs(eng.state(0)[:, :8] - tiled[:, :8]).max() < 1e-12


def test_a_refusal_behind_enqueued_group_kernels_leaves_a_usable_engine(tmp_path, monkeypatch):
    """The refused launch in a MIXED batch: small robots (launch groups on their own streams) next to a lattice above 1024 voxels (tiled).
    With the tolerated scratch size below zero the call fails with VXH_ERR_HIP when it reaches the tile launch -- the group kernels of the
    small robots are enqueued by then.  reset() frees the batch those kernels read: the engine waits for every one of its streams first
    (Device::idle), not only for the stream it frees on.  Every robot must then come out as in an engine that never failed."""
    from evosoro_amd import engine as eng_mod, workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.05, fitness_eval_init_time=0.01)
    inds = [workloads.make_individual(0, workloads.full_material(11, 3))] + [workloads.random_robot(1 + i, (6, 6, 6), 50 + i) for i in range(8)]
    paths = []
    for ind in inds:
        write_voxelyze_file(sim, Env(), ind, str(tmp_path), "mix")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("mix--id_%05i.vxa" % ind.id)))

    def engine():
        eng = eng_mod.Engine(eng_mod.VOXCAD, 0)
        eng.set_option("tiled", 1); eng.set_option("tiles_per_robot", 0); eng.set_option("wide", 1)     # the engine's own policy
        eng.add_vxa_files(paths)
        return eng

    monkeypatch.delenv("VXH_TILE_SCRATCH_LIMIT", raising=False)
    with engine() as eng:
        eng.step(10)
        want = [eng.state(k) for k in range(len(paths))]
    with engine() as eng:
        monkeypatch.setenv("VXH_TILE_SCRATCH_LIMIT", "-1")
        with pytest.raises(eng_mod.VxhError) as err:
            eng.step(10)
        assert "scratch" in str(err.value) and "status -5" in str(err.value)          # VXH_ERR_HIP
        monkeypatch.delenv("VXH_TILE_SCRATCH_LIMIT")
        eng.reset()
        eng.step(10)
        for k in range(len(paths)):
            assert np.abs(eng.state(k)[:, :8] - want[k][:, :8]).max() < 1e-12, k


def test_the_engine_keeps_the_pools_memory_between_batches(golden_dir, monkeypatch):
    """Round 6, found by looping this file on one box: the engine that had refused a launch (the test above), then reset() and stepped, came
    back with the REST state in 3 % of fresh processes -- the first two uploads of the re-uploaded batch (DRobot, DRobotState: the first
    0x290 bytes of a chunk the stream-ordered pool had just handed back to the driver and acquired again) read zero at the end of prepare()
    although they were right behind their copies.  Never with the memory kept: the engine raises the default pool's release threshold
    (engine.hip, Engine::Engine; VXH_POOL_RELEASE=1 leaves the runtime's default).  A 3-% event cannot be asserted in one run; what can is that
    the threshold is what the engine says it is, and that the refused-then-reset sequence is right ten times over in this process."""
    import ctypes
    from evosoro_amd import engine as eng_mod
    path = os.path.join(golden_dir, "vxa", "rand6_col.vxa")
    monkeypatch.delenv("VXH_POOL_RELEASE", raising=False)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 0)
        eng.set_option("wide", 0)
        eng.add_vxa_file(path)
        eng.step(10)
        want = eng.state(0).copy()
        # the HIP runtime the ENGINE is linked against: a process that has imported torch holds two copies of libamdhip64 (torch ships its
        # own), and the soname alone may resolve to the other one, which has never seen a device (hipErrorNoDevice)
        copies = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
        answers = []
        for lib_path in copies:
            hip = ctypes.CDLL(lib_path)
            pool, keep = ctypes.c_void_p(), ctypes.c_uint64(0)
            if hip.hipDeviceGetDefaultMemPool(ctypes.byref(pool), 0) == 0 and pool.value \
                    and hip.hipMemPoolGetAttribute(pool, 4, ctypes.byref(keep)) == 0:           # hipMemPoolAttrReleaseThreshold
                answers.append(keep.value)
        assert 2 ** 64 - 1 in answers, (copies, answers)
    for _ in range(10):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 2)
            eng.set_option("tiles_per_robot", 3)
            eng.add_vxa_file(path)
            monkeypatch.setenv("VXH_TILE_SCRATCH_LIMIT", "-1")
            with pytest.raises(eng_mod.VxhError):
                eng.step(10)
            monkeypatch.delenv("VXH_TILE_SCRATCH_LIMIT")
            eng.reset()
            eng.step(10)
            assert np.abs(eng.state(0)[:, :8] - want[:, :8]).max() < 1e-12
