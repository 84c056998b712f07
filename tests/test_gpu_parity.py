"""GPU parity (-m gpu): the HIP engine, called through the C ABI, against the CPU oracle (itself bit-exact with
the reference C++, tests/test_oracle_vs_reference.py) and against the reference's golden outputs.

Stated FP tolerance.  Both sides compute in FP64; the engine differs from the reference by device-libm ulps, FMA
contraction, the order of a few sums and a few algebraic rewrites (half-angle form of FromAngleToPosX, angle-addition
form of the actuation sine, the stress split folded into per-class constants; DESIGN.md "Numerics"), i.e. by
perturbations of relative size 1e-16 .. 1e-12 per operation, the upper end where the reference's own acos is
ill-conditioned to the same degree.  How far
such perturbations grow is a property of the ROBOT, not of the implementation: most robots are well conditioned
(errors stay ~1e-14 voxel over thousands of steps) but some amplify any perturbation by ~2x per step through
stick-slip contact until it saturates around 1e-3 voxel (golden case "phase4": the reference algorithm itself,
fed a gravity constant changed by ONE ulp, moves its final centre of mass by 2.5e-3 voxel).  The bar is therefore
    error(engine, oracle)  <=  max(1e-9 voxel, 20 x spread)
where `spread` is the largest deviation, over the compared horizon (plus a margin: the onset of the exponential
growth depends on the size of the first perturbation), between the oracle and the oracle with 1-ulp-perturbed
gravity, measured alongside on the CPU.  Well-conditioned robots thus get the 1e-9 voxel bar at every step.
"""
import os
import subprocess

import numpy as np
import pytest
from conftest import free_port

pytestmark = pytest.mark.gpu

CASES = ["probe6", "rand6_nocol", "rand6_col", "soft5_init0", "phase4", "stiff5", "grow5", "devo4",
         "stop1_5", "stop3_5"]                # (the last two: StopConditionType 1 and 3, VX_Sim.cpp:1398-1423)
FLOOR_VOX = 1e-9


@pytest.fixture(scope="module")
def eng_mod():
    from evosoro_amd import engine
    return engine


def _perturbed(model):
    """the same robot with ONE input changed by an ulp or two: gravity -- or, for a robot in a fluid, where gravity is off, the
    drag coefficient"""
    twin = dict(model)
    if model.get("fluid_env"):
        twin["aggregate_drag_coef"] = model["aggregate_drag_coef"] * (1 + 4e-16)
    else:
        twin["grav_acc"] = model["grav_acc"] * (1 + 4e-16)
    return twin


def _pos_err(a, b, lat):
    return np.abs(a[:, 0:3] - b[:, 0:3]).max() / lat


def _spread(model, checkpoints):
    """max position / quaternion deviation of the 1-ulp-perturbed oracle run over the given step counts"""
    from oracle import vxoracle as vo
    a, b = vo.OracleSim(model), vo.OracleSim(_perturbed(model))
    pos = quat = 0.0
    for upto in checkpoints:
        a.step(upto - a.info().steps)
        b.step(upto - b.info().steps)
        sa, sb = a.state(), b.state()
        pos = max(pos, _pos_err(sa, sb, model["lattice_dim"]))
        quat = max(quat, np.abs(sa[:, 3:7] - sb[:, 3:7]).max())
    return pos, quat


def _jitter_spread(model, upto):
    """Position deviation after `upto` steps of the oracle from a twin of itself whose first three steps start from positions moved by one
    ulp each, up or down at random (vxo_jitter): the conditioning probe for robots whose instability the one-input twin of _spread does not
    excite.  Found by a wider campaign of the land_water sweep (VXH_SWEEP_SEED=34, 120 robots): a 3 x 5 x 3 block resting on the floor
    keeps its symmetry under a change of g, and its buckling mode -- which amplifies rounding-size differences 3000-fold every 40 steps --
    only starts from a perturbation that breaks the symmetry, as any other arithmetic's roundings do.  The engine was 1e-15 voxel from
    the oracle on EVERY single step from the same state (scripts/dev_gpu_diag.py sweepcase) and 7e-4 voxel after 150 free-running steps,
    where the one-input twin had moved by 1.5e-9.  Used only for a robot that misses the bar that follows from _spread."""
    from oracle import vxoracle as vo
    a, c = vo.OracleSim(model), vo.OracleSim(model)
    c.step_jittered(min(3, upto), seed=7)
    a.step(upto)
    c.step(upto - c.info().steps)
    return _pos_err(a.state(), c.state(), model["lattice_dim"])


def test_early_steps_match_oracle(eng_mod, golden_dir):
    from oracle import vxoracle as vo
    models = [vo.parse_vxa(os.path.join(golden_dir, "vxa", n + ".vxa")) for n in CASES]
    sims = [vo.OracleSim(m) for m in models]
    spreads = [_spread(m, (50, 100, 200, 300, 400)) for m in models]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for n in CASES:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        done = 0
        for upto in (1, 2, 10, 50, 200):
            eng.step(upto - done)
            done = upto
            for i, name in enumerate(CASES):
                sims[i].step(upto - sims[i].info().steps)
                want, got = sims[i].state(), eng.state(i)
                lat = models[i]["lattice_dim"]
                tol = FLOOR_VOX if upto <= 10 else max(FLOOR_VOX, 20 * spreads[i][0])
                qtol = 1e-9 if upto <= 10 else max(1e-9, 20 * spreads[i][1])
                assert _pos_err(got, want, lat) <= tol, (name, upto, _pos_err(got, want, lat), tol)
                assert np.abs(got[:, 3:7] - want[:, 3:7]).max() <= qtol, (name, upto)
                assert np.abs(got[:, 7] - want[:, 7]).max() / lat < 1e-12, (name, upto)   # actuation: no chaos involved
        assert sum(1 for sp in spreads if sp[0] < 1e-10) >= len(CASES) - 2     # the strict 1e-9 bar really applied to almost all robots


def test_full_runs_match_reference(eng_mod, golden_dir):
    from oracle import vxoracle as vo
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for name in CASES:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", name + ".vxa"))
        eng.run()
        for i, name in enumerate(CASES):
            model = vo.parse_vxa(os.path.join(golden_dir, "vxa", name + ".vxa"))
            lat = model["lattice_dim"]
            planned = eng.dims(i)["planned_steps"]
            spread = _spread(model, sorted(set([planned // 4, planned // 2, 3 * planned // 4, planned])))[0]
            tol = max(FLOOR_VOX, 20 * spread)
            trace = vo.read_trace(os.path.join(golden_dir, "expected", name + ".final.bin"))
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", name + ".xml"))
            res = eng.result(i)
            assert res.status == eng_mod.ROBOT_FINISHED
            assert res.steps == trace["total_steps"], name
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / lat <= tol, (name, tol)
            assert np.abs(np.array(res.ini_cm) - trace["ini_cm"]).max() / lat <= tol, (name, tol)
            # result tags: 6 significant digits like the reference, up to the robot's own conditioning
            for tag, val in (("NormFinalDist", res.norm_final_dist), ("finalDistY", res.final_dist_y),
                             ("AnteriorDist", res.anterior_dist), ("PosteriorY", res.posterior_y)):
                # (the golden XML carries 6 significant digits: up to 5e-6 relative rounding)
                assert abs(val - want[tag]) <= 2 * tol + 1e-5 * abs(want[tag]), (name, tag, val, want[tag])
            assert abs(res.lifetime - want["Lifetime"]) < 1e-5, name
            if tol < 1e-6:
                assert res.num_touching_floor == want["NumTouchingFloor"], name


def test_cli_writes_reference_xml(eng_mod, golden_dir, tmp_path):
    """`voxelyze -f x.vxa` drop-in: exit code 1, result XML at <FitnessFileName>, same tags, same 6-digit numbers."""
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "golden_run" / "fitnessFiles")
    names = ["probe6", "rand6_col"]
    args = []
    for n in names:
        args += ["-f", os.path.join(golden_dir, "vxa", n + ".vxa")]
    proc = subprocess.run([eng_mod.CLI_PATH] + args, cwd=tmp_path, timeout=600)
    assert proc.returncode == 1                      # the reference's "success" code (main.cpp:132)
    ids = {"probe6": 0, "rand6_col": 2}
    for n in names:
        got_path = tmp_path / "golden_run" / "fitnessFiles" / ("softbotsOutput--id_%05i.xml" % ids[n])
        got_lines = open(got_path).read().splitlines()
        want_lines = open(os.path.join(golden_dir, "expected", n + ".xml")).read().splitlines()
        assert len(got_lines) == len(want_lines)
        got, want = vo.read_result_xml(str(got_path)), vo.read_result_xml(os.path.join(golden_dir, "expected", n + ".xml"))
        assert list(got) == list(want)
        for tag in want:
            assert abs(got[tag] - want[tag]) <= 1e-5 * max(1.0, abs(want[tag])), (n, tag)
        # well-conditioned robots: the fitness line is byte-identical
        assert [l for l in got_lines if "NormFinalDist" in l] == [l for l in want_lines if "NormFinalDist" in l]


def test_cli_progress_output_is_the_references(eng_mod, golden_dir, tmp_path):
    """`voxelyze -f x.vxa -p`, the reference CLI's only diagnostic (voxelyzeMain/main.cpp:60-63,92-104,128): the import message, then
    every 100 steps Time / |CM| / Vox[0] scale, TempAmp, TempPer, phaseOffset, then "Ended at:".  Compared line by line with what the
    reference binary printed for the same file (tests/golden/expected/soft5_init0.p.txt, written by make_golden.py): text lines equal,
    numbers equal to the six significant digits the reference prints (a last-digit difference of a printed number is allowed: the
    engine is within 1e-12 voxel, but a value may sit on a rounding boundary of the print)."""
    import subprocess
    os.makedirs(tmp_path / "golden_run" / "fitnessFiles")
    proc = subprocess.run([eng_mod.CLI_PATH, "-f", os.path.join(golden_dir, "vxa", "soft5_init0.vxa"), "-p"], cwd=tmp_path, timeout=600,
                          stdout=subprocess.PIPE)
    assert proc.returncode == 1
    got = proc.stdout.decode().splitlines()
    want = open(os.path.join(golden_dir, "expected", "soft5_init0.p.txt")).read().splitlines()
    assert len(got) == len(want), (len(got), len(want), got[:12])
    assert sum(1 for ln in want if ln.startswith("Time: ")) == 8 and want[-1].startswith("Ended at: ")
    for g, w in zip(got, want):
        if ": " in w and w.split(": ")[0] in ("Time", "CM", "Vox[0]  Scale", "Vox[0]  TempAmp", "Vox[0]  TempPer", "Vox[0]  phaseOffset", "Ended at"):
            assert g.split(": ")[0] == w.split(": ")[0], (g, w)
            a, b = float(g.split(": ")[1]), float(w.split(": ")[1])
            assert abs(a - b) <= 1.5e-6 * max(abs(b), 1e-300), (g, w)
        else:
            assert g == w, (g, w)
    assert os.path.exists(tmp_path / "golden_run" / "fitnessFiles" / "softbotsOutput--id_00003.xml") or \
        len(os.listdir(tmp_path / "golden_run" / "fitnessFiles")) == 1


def test_cli_shape_descriptor_report_is_the_references(eng_mod, golden_dir, tmp_path):
    """`voxelyze -f x.vxa -p --computeShapeDescriptors` (round 6): what the reference's _voxcad command line computes and prints of its
    deformable surface mesh (voxelyzeMain/main.cpp:65-88,113-126; CVX_MeshUtil::printAllMeshInfo, VX_MeshUtil.cpp:733-772): mesh size,
    robot volume, shape complexity, every vertex, every facet (vertex triple) and every facet normal -- right after the import and again
    after the run.  Golden: the reference binary's own stdout for the same file (tests/golden/expected/soft5_init0.pcsd.txt, make_golden.py).
    Text and integers equal; numbers to the six digits the stream prints (1.5e-6 relative, 1e-9 absolute: a normal's zero component is
    rounding noise around 1e-16 on both sides); the lines the reference's missing `qhull` produces are skipped, and where it prints
    -1 for the hull volume the engine prints the hull it computes (>= the robot's own volume)."""
    import subprocess
    for d in ("fitnessFiles", "tempFiles"):
        os.makedirs(tmp_path / "golden_run" / d)
    proc = subprocess.run([eng_mod.CLI_PATH, "-f", os.path.join(golden_dir, "vxa", "soft5_init0.vxa"), "-p", "--computeShapeDescriptors"], cwd=tmp_path,
                          timeout=600, stdout=subprocess.PIPE)
    assert proc.returncode == 1
    got = proc.stdout.decode().splitlines()
    noise = ("CVX_MeshUtil ERROR", "ERROR: CVX_MeshUtil", "[V_MeshUtil.cpp]", "WARNING: CVX_MeshUtil")
    want = [ln for ln in open(os.path.join(golden_dir, "expected", "soft5_init0.pcsd.txt")).read().splitlines() if not ln.startswith(noise)]
    assert len(got) == len(want), (len(got), len(want), got[:14])
    assert want[6].startswith("Robot mesh has 205 vertices and 444 facets") and sum(1 for ln in want if "PRINTING DEFORMABLE MESH" in ln) == 6
    volumes = {}
    for k, (g, w) in enumerate(zip(got, want)):
        if "convex hull volume: " in w:
            assert g.split(": ")[0] == w.split(": ")[0] and float(w.split(": ")[1]) == -1.0     # (no qhull on the box that made the golden file)
            volumes[g.split(" ")[0] + " hull"] = float(g.split(": ")[1])
            continue
        if ": " in w and w.split(": ")[0] in ("Time", "CM", "Vox[0]  Scale", "Vox[0]  TempAmp", "Vox[0]  TempPer", "Vox[0]  phaseOffset", "Ended at",
                                              "Init robot volume", "Final robot volume", "Init shape complexity", "Final shape complexity"):
            assert g.split(": ")[0] == w.split(": ")[0], (k, g, w)
            a, b = float(g.split(": ")[1]), float(w.split(": ")[1])
            assert abs(a - b) <= 1.5e-6 * abs(b) + 1e-12, (k, g, w)
            if "robot volume" in w:
                volumes[w.split(" ")[0] + " robot"] = a
            continue
        gt, wt = g.split(), w.split()
        if len(wt) == 3 and all(t.lstrip("-").isdigit() for t in wt):       # a facet: three vertex indices
            assert gt == wt, (k, g, w)
        elif len(wt) == 3 and not w.startswith(("|", " -")):                # a vertex or a normal
            for a, b in zip(map(float, gt), map(float, wt)):
                assert abs(a - b) <= 1.5e-6 * abs(b) + 1e-9, (k, g, w)
        else:
            assert g == w, (k, g, w)
    assert volumes["Init hull"] >= volumes["Init robot"] * (1 - 1e-9) > 0 and volumes["Final hull"] >= volumes["Final robot"] * (1 - 1e-9) > 0


def test_options_changed_between_runs_of_one_engine(eng_mod, golden_dir):
    """A captured step graph holds the kernel arguments of the moment of capture: switching the stepping kernels on ONE engine
    between runs (streaming with a graph -> resident -> streaming again) must leave nothing stale behind -- the streaming runs
    before and after equal each other and a fresh engine's, bit for bit."""
    paths = [os.path.join(golden_dir, "vxa", n + ".vxa") for n in ("probe6", "rand6_col")]

    def run(eng, fused):
        eng.reset()                         # (which kernel steps a robot is part of the assembled batch: set right after a reset)
        eng.set_option("fused", fused)
        eng.step(400)                       # > graph_steps: the streaming path replays its captured graph
        return [eng.state(i) for i in range(len(paths))]

    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 0)
        eng.set_option("graph_steps", 32)
        for p in paths:
            eng.add_vxa_file(p)
        first = run(eng, 0)
        resident = run(eng, 1)
        again = run(eng, 0)
        eng.set_option("graph_steps", 16)   # a different graph length: captured afresh as well
        shorter = run(eng, 0)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 0)
        eng.set_option("graph_steps", 32)
        for p in paths:
            eng.add_vxa_file(p)
        fresh = run(eng, 0)
    for a, b, c, d, r in zip(first, again, shorter, fresh, resident):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
        assert np.abs(a[:, :8] - r[:, :8]).max() < 1e-12          # (and the two kernels agree, as in the test below)


def test_streaming_path_matches_fused_path(eng_mod, golden_dir):
    names = ["probe6", "rand6_col", "soft5_init0"]
    states = {}
    for fused in (1, 0):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 0)
            eng.set_option("fused", fused)
            for n in names:
                eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
            eng.step(300)
            states[fused] = [eng.state(i) for i in range(len(names))]
    for a, b in zip(states[1], states[0]):
        assert np.abs(a[:, :8] - b[:, :8]).max() < 1e-12       # same kernels' math, different force-sum order
    # _voxcad_land_water, on land and in a fluid (the streaming path has its own mesh / facet kernels for the drag)
    names, states = ["lw_land6", "lw_stiff5", "lw_swim6"], {}
    for fused in (1, 0):
        with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
            eng.set_option("fused", fused)
            for n in names:
                eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
            eng.step(300)
            states[fused] = [eng.state(i) for i in range(len(names))]
    for a, b in zip(states[1], states[0]):
        assert np.abs(a[:, :8] - b[:, :8]).max() < 1e-12


def test_large_lattice_streaming_vs_oracle(eng_mod, tmp_path):
    """BASELINE configs[4]: one full 20x20x20 lattice with self-collision (more voxels than a workgroup holds)."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    ind = workloads.make_individual(0, workloads.full_material(20, 1))
    write_voxelyze_file(Sim(dt_frac=0.9, simulation_time=0.01, fitness_eval_init_time=0.002), Env(), ind, str(tmp_path), "big")
    path = str(tmp_path / "voxelyzeFiles" / "big--id_00000.vxa")
    sim = vo.OracleSim.from_vxa(path)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_file(path)
        assert eng.dims(0)["nvox"] == 8000 and eng.dims(0)["nbond"] == 22800
        for upto in (1, 20, 60):
            eng.step(upto - sim.info().steps)
            sim.step(upto - sim.info().steps)
            assert _pos_err(eng.state(0), sim.state(), 0.01) < 1e-9, upto
        eng.run()
        sim.step(-1)
        res = eng.result(0)
        assert res.status == eng_mod.ROBOT_FINISHED and res.steps == sim.info().steps == 157
        assert np.abs(np.array(res.cur_cm) - np.array(sim.info().cur_cm)).max() / 0.01 < 1e-8


def test_full_size_batch_properties(eng_mod, tmp_path):
    """BASELINE configs[1]/[2] sizes: properties that need no CPU reference at scale.
    (a) a robot's trajectory does not depend on which batch it is in or where (bitwise), (b) reruns are bitwise
    reproducible, (c) a sample of robots agrees with the oracle, (d) every robot finishes with finite state."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim, env = Sim(dt_frac=0.9, simulation_time=0.012, fitness_eval_init_time=0.004), Env()
    paths = []
    for i, shape in [(k, (6, 6, 6)) for k in range(64)] + [(64 + k, (10, 10, 10)) for k in range(128)]:
        ind = workloads.random_robot(i, shape, i)
        write_voxelyze_file(sim, env, ind, str(tmp_path), "p")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("p--id_%05i.vxa" % i)))
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for p in paths:
            eng.add_vxa_file(p)
        eng.run()
        batch = {i: eng.state(i) for i in (0, 63, 64, 100, 191)}
        results = [eng.result(i) for i in range(len(paths))]
        assert all(r.status == eng_mod.ROBOT_FINISHED for r in results)
        assert all(np.isfinite(r.cur_cm).all() and np.isfinite(r.norm_final_dist) for r in results)
        eng.reset()
        eng.run()
        for i, st in batch.items():
            assert np.array_equal(st, eng.state(i)), "rerun differs for robot %d" % i
    for i, st in batch.items():
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as solo:
            solo.add_vxa_file(paths[i])
            solo.run()
            assert np.array_equal(st, solo.state(0)), "robot %d depends on its batch" % i
    for i in (0, 64):
        o = vo.OracleSim.from_vxa(paths[i])
        o.step(-1)
        tol = max(FLOOR_VOX, 20 * _spread(o.model, (results[i].steps // 2, results[i].steps))[0])
        assert _pos_err(batch[i], o.state(), 0.01) <= tol
        assert results[i].steps == o.info().steps


LW_CASES = ["lw_land6", "lw_swim6", "lw_hexapus", "lw_quadruped_land", "lw_stiff5", "lw_stop3_5"]


def test_land_water_variant(eng_mod, golden_dir):
    """_voxcad_land_water semantics incl. BASELINE configs[3] physics: fluid environment with per-facet drag
    (lw_swim6, and lw_hexapus = a sample .vxa shipped with the reference), gravity/floor off in fluid."""
    from oracle import vxoracle as vo
    models = [vo.parse_vxa(os.path.join(golden_dir, "vxa", n + ".vxa"), 1) for n in LW_CASES]
    sims = [vo.OracleSim(m) for m in models]
    spreads = [_spread(m, (100, 300, 600)) for m in models]
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        for n in LW_CASES:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        for upto in (1, 10, 100, 400):
            eng.step(upto - sims[0].info().steps)
            for i, name in enumerate(LW_CASES):
                sims[i].step(upto - sims[i].info().steps)
                lat = models[i]["lattice_dim"]
                tol = FLOOR_VOX if upto <= 10 else max(FLOOR_VOX, 20 * spreads[i][0])
                assert _pos_err(eng.state(i), sims[i].state(), lat) <= tol, (name, upto, tol)
    # whole runs of the two generated robots against the reference's result XML
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        for n in LW_CASES[:2]:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        eng.run()
        for i, name in enumerate(LW_CASES[:2]):
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", name + ".xml"))
            trace = vo.read_trace(os.path.join(golden_dir, "expected", name + ".final.bin"))
            res = eng.result(i)
            planned = eng.dims(i)["planned_steps"]
            tol = max(FLOOR_VOX, 20 * _spread(models[i], (planned // 2, planned))[0])
            assert res.status == eng_mod.ROBOT_FINISHED and res.steps == trace["total_steps"]
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / models[i]["lattice_dim"] <= tol, name
            for tag, val in (("normAbsoluteDisplacement", res.norm_abs_disp), ("normDistZ", res.norm_dist_z)):
                assert abs(val - want[tag]) <= 2 * tol + 1e-5 * abs(want[tag]), (name, tag, val, want[tag])
            # mesh-volume tags (LW/VX_MeshUtil.cpp:908-952): rest volume exactly, deformed volume to the printed digits
            assert "%.6g" % res.robot_volume_start == "%.6g" % want["RobotVolumeStart"], name
            assert abs(res.robot_volume_end - want["RobotVolumeEnd"]) <= 2e-5 * want["RobotVolumeEnd"] + 10 * tol * 1e-6, (name, res.robot_volume_end)
            # convex hull of the surface mesh: the reference ran the qhull binary it vendors on the vertices (tests/golden/make_golden.py)
            assert "%.6g" % res.hull_volume_start == "%.6g" % want["ConvexHullVolumeStart"], name
            assert abs(res.hull_volume_end - want["ConvexHullVolumeEnd"]) <= 2e-5 * want["ConvexHullVolumeEnd"] + 10 * tol * 1e-6, (name, res.hull_volume_end)


def test_land_water_bench_size_robots_whole_run_vs_reference(eng_mod, golden_dir):
    """A 709-voxel swimmer and a full 10x10x10 lattice on land (the 768- and 1024-thread MESH variants of the fused kernel,
    strains in HBM), the whole evaluation against the reference binary's final state and result XML, incl. the
    RobotVolumeEnd tag computed from the strains of the last step."""
    from oracle import vxoracle as vo
    names = ["lw_swim10", "lw_land10"]
    models = [vo.parse_vxa(os.path.join(golden_dir, "vxa", n + ".vxa"), 1) for n in names]
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.add_vxa_files([os.path.join(golden_dir, "vxa", n + ".vxa") for n in names])
        eng.run()
        assert eng.counters().dominant_block != 0
        for i, name in enumerate(names):
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", name + ".xml"))
            trace = vo.read_trace(os.path.join(golden_dir, "expected", name + ".final.bin"))
            res = eng.result(i)
            planned = eng.dims(i)["planned_steps"]
            tol = max(FLOOR_VOX, 20 * _spread(models[i], (planned // 2, planned))[0])
            assert res.status == eng_mod.ROBOT_FINISHED and res.steps == trace["total_steps"]
            assert _pos_err(eng.state(i), trace["records"][-1]["state"], models[i]["lattice_dim"]) <= tol, (name, tol)
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / models[i]["lattice_dim"] <= tol, name
            for tag, val in (("normAbsoluteDisplacement", res.norm_abs_disp), ("normDistZ", res.norm_dist_z)):
                assert abs(val - want[tag]) <= 2 * tol + 1e-5 * abs(want[tag]), (name, tag, val, want[tag])
            assert "%.6g" % res.robot_volume_start == "%.6g" % want["RobotVolumeStart"], name
            assert abs(res.robot_volume_end - want["RobotVolumeEnd"]) <= 2e-5 * want["RobotVolumeEnd"] + 10 * tol * 1e-6, (name, res.robot_volume_end)


def _write_robot(tmp_path, ident, material, sim, env, name):
    from evosoro_amd import workloads
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles", exist_ok=True)
    write_voxelyze_file(sim, env, workloads.make_individual(ident, material), str(tmp_path), name)
    return str(tmp_path / "voxelyzeFiles" / ("%s--id_%05i.vxa" % (name, ident)))


def test_every_fused_kernel_variant_vs_oracle(eng_mod, tmp_path):
    """One robot per workgroup size of the fused kernel (256 / 512 / 768 / 1024 threads; the last one exchanges bond
    forces axis by axis through a single LDS buffer) against the oracle, self-collision on, in ONE batch."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from oracle import vxoracle as vo
    sim, env = Sim(dt_frac=0.9, simulation_time=0.02, fitness_eval_init_time=0.002), Env()
    mats = [workloads.random_material((6, 6, 6), 3), workloads.random_material((8, 8, 8), 4),
            workloads.random_material((10, 10, 10), 5), workloads.full_material(10, 2),
            workloads.full_material(11, 3)]      # and one beyond a workgroup: streaming kernels, side by side with the others
    paths = [_write_robot(tmp_path, k, m, sim, env, "v") for k, m in enumerate(mats)]
    sims = [vo.OracleSim.from_vxa(p) for p in paths]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for p in paths:
            eng.add_vxa_file(p)
        nv = [eng.dims(i)["nvox"] for i in range(5)]
        assert nv[0] <= 256 < nv[1] <= 512 < nv[2] <= 768 < nv[3] == 1000 and nv[4] == 1331
        for upto in (1, 3, 40, 120):
            eng.step(upto - sims[0].info().steps)
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                assert _pos_err(eng.state(i), o.state(), 0.01) < FLOOR_VOX, (i, upto)
                assert np.abs(eng.state(i)[:, 3:14] - o.state()[:, 3:14]).max() < 1e-7, (i, upto)   # quat, scale, vel, angvel


def test_every_mesh_kernel_variant_swims_like_the_oracle(eng_mod, tmp_path):
    """_voxcad_land_water in a fluid, one swimmer per workgroup size of the fused kernel's MESH variants (256 / 512 /
    768 / 1024 threads; the last two keep the strains in HBM and pass the voxel corners through a six-plane tile) in ONE
    batch against the oracle.  Without gravity and floor a robot only moves through actuation + drag, so a swimmer that
    silently lost its drag (e.g. by falling onto the streaming kernels, which have none) cannot pass."""
    from collections import OrderedDict
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    sim = Sim(dt_frac=0.9, simulation_time=0.02, fitness_eval_init_time=0.002)
    env = Env()
    env.add_param("fluid_environment", 1, "<FluidEnvironment>")
    env.add_param("aggregate_drag_coefficient", 750.0, "<AggregateDragCoefficient>")
    os.makedirs(tmp_path / "voxelyzeFiles")
    mats = [workloads.random_material((6, 6, 6), 3), workloads.random_material((8, 8, 8), 4),
            workloads.random_material((10, 10, 10), 5), workloads.full_material(10, 2)]
    paths = []
    for k, m in enumerate(mats):
        layers = OrderedDict([("<PhaseOffset>", np.round(np.random.RandomState(50 + k).uniform(-1, 1, size=m.shape), 3))])
        write_voxelyze_file(sim, env, workloads.make_individual(k, m, layers), str(tmp_path), "s")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("s--id_%05i.vxa" % k)))
    sims = [vo.OracleSim.from_vxa(p, variant=1) for p in paths]
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.add_vxa_files(paths)
        nv = [eng.dims(i)["nvox"] for i in range(4)]
        assert nv[0] <= 256 < nv[1] <= 512 < nv[2] <= 768 < nv[3] == 1000
        for upto in (1, 3, 40, 120):
            eng.step(upto - sims[0].info().steps)
            assert eng.counters().dominant_block != 0              # the fused kernels ran (0 = streaming path)
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                assert _pos_err(eng.state(i), o.state(), 0.01) < FLOOR_VOX, (i, upto)
                assert np.abs(eng.state(i)[:, 3:14] - o.state()[:, 3:14]).max() < 1e-7, (i, upto)
        moved = [np.abs(o.state()[:, 7:10]).max() for o in sims]       # the swimmers do move (velocities)
        assert min(moved) > 0
    # a swimmer of more than 1024 voxels (full 11x11x11) next to a small one (wide kernel, side by side in the same call): both against
    # the oracle, and the volume tag is still produced.  Round 5: the large one is TILED -- every tile carries its part of the drag mesh,
    # pose and strains of the voxels around a vertex come through the exchange buffer (k_tile_steps "fluid") -- unless the test's kernel
    # path switches tiling off (then: streaming kernels with the mesh in HBM, as until round 4)
    big = workloads.make_individual(9, workloads.full_material(11, 1),
                                    OrderedDict([("<PhaseOffset>", np.round(np.random.RandomState(59).uniform(-1, 1, size=(11, 11, 11)), 3))]))
    write_voxelyze_file(sim, env, big, str(tmp_path), "s")
    both = [paths[0], str(tmp_path / "voxelyzeFiles" / "s--id_00009.vxa")]
    sims = [vo.OracleSim.from_vxa(p, variant=1) for p in both]
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.add_vxa_files(both)
        assert eng.dims(1)["nvox"] == 1331
        for upto in (1, 3, 40, 120):
            eng.step(upto - sims[0].info().steps)
            assert eng.counters().dominant_block == (0 if "tiled=0" in os.environ.get("VXH_ENGINE_OPTIONS", "") else 1)      # streaming kernels / k_tile_steps
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                assert _pos_err(eng.state(i), o.state(), 0.01) < FLOOR_VOX, (i, upto)
                assert np.abs(eng.state(i)[:, 3:14] - o.state()[:, 3:14]).max() < 1e-7, (i, upto)
        eng.run()
        assert all(eng.result(i).robot_volume_end > 0 for i in range(2))


def test_evolved_stiffness_on_large_robots_vs_oracle(eng_mod, tmp_path):
    """Per-voxel evolved <Stiffness> makes nearly every bond (and voxel) a class of its own; from a few hundred voxels on
    the class tables outgrow the LDS and the fused kernel reads them from HBM instead (TABG variants).  Both simulators,
    small (tables in LDS) and large robots in one batch each, against the oracle; the swimmers must not lose their drag."""
    from collections import OrderedDict
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    sim = Sim(dt_frac=0.9, simulation_time=0.02, fitness_eval_init_time=0.002)
    os.makedirs(tmp_path / "voxelyzeFiles")
    env_w = Env()
    env_w.add_param("fluid_environment", 1, "<FluidEnvironment>")
    env_w.add_param("aggregate_drag_coefficient", 750.0, "<AggregateDragCoefficient>")
    for variant, env, tag, shapes in ((eng_mod.VOXCAD, Env(), "e", [(5, 5, 5), (8, 8, 8), (10, 10, 10)]),
                                      (eng_mod.VOXCAD_LAND_WATER, env_w, "f", [(4, 4, 4), (6, 6, 6), (8, 8, 8), (10, 10, 10)])):
        paths = []
        for k, shape in enumerate(shapes):
            rng = np.random.RandomState(900 + k)
            layers = OrderedDict([("<PhaseOffset>", np.round(rng.uniform(-1, 1, size=shape), 3)),
                                  ("<Stiffness>", np.round(10 ** rng.uniform(6.0, 7.7, size=shape), 0))])
            write_voxelyze_file(sim, env, workloads.make_individual(k, workloads.random_material(shape, 40 + k), layers), str(tmp_path), tag)
            paths.append(str(tmp_path / "voxelyzeFiles" / ("%s--id_%05i.vxa" % (tag, k))))
        sims = [vo.OracleSim.from_vxa(p, variant=1 if variant == eng_mod.VOXCAD_LAND_WATER else 0) for p in paths]
        with eng_mod.Engine(variant, 0) as eng:
            eng.add_vxa_files(paths)
            assert eng.dims(len(shapes) - 1)["nvox"] > 512
            for upto in (1, 3, 40, 120):
                eng.step(upto - sims[0].info().steps)
                assert eng.counters().dominant_block != 0                  # fused kernels, not the streaming path
                for i, o in enumerate(sims):
                    o.step(upto - o.info().steps)
                    assert _pos_err(eng.state(i), o.state(), 0.01) < FLOOR_VOX, (tag, i, upto)
                    assert np.abs(eng.state(i)[:, 3:14] - o.state()[:, 3:14]).max() < 1e-7, (tag, i, upto)


def test_diverging_robot_is_reported_like_the_reference(eng_mod, tmp_path):
    """DtFrac far above the stability limit: the reference's Integrate() stops at the first bond stretched past 100x
    (VX_Sim.cpp:1775) and the run ends 'diverged'; same step, same verdict, and the rest of the batch is unaffected."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from oracle import vxoracle as vo
    env = Env()
    bad = _write_robot(tmp_path, 0, workloads.random_material((6, 6, 6), 9), Sim(dt_frac=6.0, simulation_time=0.05, fitness_eval_init_time=0.0), env, "d")
    good = _write_robot(tmp_path, 1, workloads.random_material((6, 6, 6), 9), Sim(dt_frac=0.9, simulation_time=0.01, fitness_eval_init_time=0.0), env, "d")
    o = vo.OracleSim.from_vxa(bad)
    o.step(-1)
    assert o.info().status == 2
    for fused in (1, 0):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("fused", fused)
            eng.add_vxa_file(bad)
            eng.add_vxa_file(good)
            eng.run()
            assert eng.result(0).status == eng_mod.ROBOT_DIVERGED
            assert eng.result(0).steps == o.info().steps
            assert eng.result(1).status == eng_mod.ROBOT_FINISHED and np.isfinite(eng.result(1).cur_cm).all()


def test_batch_import_matches_sequential_import(eng_mod, golden_dir, tmp_path):
    """vxh_add_vxa_files (whole generation, parsed on all host cores) == vxh_add_vxa_file one by one: same order, same
    robots, bitwise the same trajectories; a bad path fails the call and appends nothing."""
    names = ["probe6", "rand6_col", "soft5_init0", "phase4", "stiff5", "grow5"] * 3
    paths = [os.path.join(golden_dir, "vxa", n + ".vxa") for n in names]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as a, eng_mod.Engine(eng_mod.VOXCAD, 0) as b:
        assert a.add_vxa_files(paths) == 0
        for p in paths:
            b.add_vxa_file(p)
        assert a.num_robots() == b.num_robots() == len(paths)
        assert [a.dims(i) for i in range(len(paths))] == [b.dims(i) for i in range(len(paths))]
        a.step(150)
        b.step(150)
        for i in range(len(paths)):
            assert np.array_equal(a.state(i), b.state(i)), i
        with pytest.raises(Exception):
            a.add_vxa_files(paths[:2] + [str(tmp_path / "missing.vxa")])
        assert a.num_robots() == len(paths)


def test_edge_sizes_in_one_batch(eng_mod, tmp_path):
    """Empty lattice, single voxel, two voxels, a one-voxel-wide tower and a lattice of exactly 1024 voxels (every
    thread of the largest workgroup owns a voxel) side by side: the empty one is reported EMPTY (the reference would
    never return), the others follow the oracle.
    (A rod lying FLAT on the floor is deliberately not used: its whole motion is a 2e-8-voxel stick-slip of the prenatal
    size change against friction, and the reference algorithm itself moves by 5e-10 voxel there when the lattice
    constant changes by one ulp.)"""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    sim, env = Sim(dt_frac=0.9, simulation_time=0.02, fitness_eval_init_time=0.004), Env()
    mats = [np.zeros((3, 3, 3), dtype=int), np.zeros((3, 3, 3), dtype=int), np.zeros((3, 3, 3), dtype=int),
            np.zeros((1, 1, 12), dtype=int), np.full((16, 8, 8), 3, dtype=int)]
    mats[1][1, 1, 0] = 3
    mats[2][1, 1, 0] = 3; mats[2][1, 1, 1] = 4
    mats[3][0, 0, :] = [1, 3, 4, 3, 1, 2, 3, 4, 3, 1, 3, 4]
    mats[4][::3, ::2, ::2] = 1
    mats[4][1::4, 1::3, :] = 4
    os.makedirs(tmp_path / "voxelyzeFiles", exist_ok=True)
    paths = []
    for k, m in enumerate(mats):
        write_voxelyze_file(sim, env, workloads.make_individual(k, m), str(tmp_path), "e")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("e--id_%05i.vxa" % k)))
    sims = [None] + [vo.OracleSim.from_vxa(p) for p in paths[1:]]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_files(paths)
        assert [eng.dims(i)["nvox"] for i in range(5)] == [0, 1, 2, 12, 1024]
        for upto in (1, 5, 60):
            eng.step(upto - sims[1].info().steps)
            for i in range(1, 5):
                sims[i].step(upto - sims[i].info().steps)
                assert _pos_err(eng.state(i), sims[i].state(), 0.01) < FLOOR_VOX, (i, upto)
        eng.run()
        assert eng.result(0).status == eng_mod.ROBOT_EMPTY
        for i in range(1, 5):
            sims[i].step(-1)
            assert eng.result(i).status == eng_mod.ROBOT_FINISHED and eng.result(i).steps == sims[i].info().steps
            assert np.abs(np.array(eng.result(i).cur_cm) - np.array(sims[i].info().cur_cm)).max() / 0.01 < 1e-7, i


def test_bench_size_robots_whole_evaluation(eng_mod, golden_dir):
    """BASELINE configs[2] size against the REFERENCE itself: the first two robots of the bench population, the whole
    0.5 s evaluation with self-collision (7806 steps), final centre of mass and result tags vs the reference binary's
    trace / XML; tolerance from the robots' own conditioning as everywhere."""
    from oracle import vxoracle as vo
    names = ["bench10_0", "bench10_1"]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_files([os.path.join(golden_dir, "vxa", n + ".vxa") for n in names])
        eng.run()
        for i, name in enumerate(names):
            model = vo.parse_vxa(os.path.join(golden_dir, "vxa", name + ".vxa"))
            lat = model["lattice_dim"]
            trace = vo.read_trace(os.path.join(golden_dir, "expected", name + ".final.bin"))
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", name + ".xml"))
            res = eng.result(i)
            planned = eng.dims(i)["planned_steps"]
            tol = max(FLOOR_VOX, 20 * _spread(model, (planned // 2, planned))[0])
            assert res.status == eng_mod.ROBOT_FINISHED and res.steps == trace["total_steps"] == 7806
            assert np.abs(np.array(res.ini_cm) - trace["ini_cm"]).max() / lat <= tol, (name, tol)
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / lat <= tol, (name, tol)
            for tag, val in (("NormFinalDist", res.norm_final_dist), ("finalDistY", res.final_dist_y)):
                assert abs(val - want[tag]) <= 2 * tol + 1e-5 * abs(want[tag]), (name, tag, val, want[tag])
            print(name, "tolerance (voxel)", tol, "CoM error (voxel)", np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / lat)


def test_free_floating_population_conserves_momentum(eng_mod, tmp_path):
    """Size-independent property at BASELINE configs[2] size (512 robots of 10x10x10): without gravity, floor and the
    velocity-proportional "slow" damping (whose coefficient depends on the material) the only forces are internal
    (bonds, self-collision, actuation), so the total linear momentum of every robot stays at its initial value, zero.
    All voxels have the same mass (one density in the evosoro palette), so sum(velocity) is the momentum up to a
    factor.  Checked against the scale of the individual voxel velocities after the actuation has run for a while."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.06, fitness_eval_init_time=0.01)
    env = Env(gravity_enabled=0, floor_enabled=0)
    paths = []
    for i in range(512):
        write_voxelyze_file(sim, env, workloads.random_robot(i, (10, 10, 10), i), str(tmp_path), "f")
        path = str(tmp_path / "voxelyzeFiles" / ("f--id_%05i.vxa" % i))
        text = open(path).read()
        assert "<SlowDampingZ>0.01</SlowDampingZ>" in text       # hard-wired in the writer, like in the reference
        open(path, "w").write(text.replace("<SlowDampingZ>0.01</SlowDampingZ>", "<SlowDampingZ>0</SlowDampingZ>"))
        paths.append(path)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_files(paths)
        eng.step(600)
        worst = 0.0
        for i in range(0, 512, 7):
            vel = eng.state(i)[:, 8:11]
            speed = np.abs(vel).max()
            assert speed > 1e-4                       # the robots do move (actuation started at t = 0.01 s)
            worst = max(worst, np.abs(vel.sum(axis=0)).max() / (speed * len(vel)))
        assert worst < 1e-9, worst


def test_two_ranks_share_the_gpu(eng_mod, golden_dir, tmp_path):
    """The multi-rank path end to end with the real engine: two processes (gloo; RCCL does not allow two ranks on one
    device) shard a generation by cost, each steps its shard on cuda:0, one gather gives both the whole table; it
    equals what a single process computes (bitwise: a robot's trajectory does not depend on its batch)."""
    import sys
    from evosoro_amd import parallel
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(os.path.dirname(__file__), "dist_worker_gpu.py"), str(tmp_path),
           os.path.join(golden_dir, "vxa")]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    t0, t1 = np.load(tmp_path / "table_rank0.npy"), np.load(tmp_path / "table_rank1.npy")
    assert np.array_equal(t0, t1)
    names = ["phase4", "soft5_init0", "rand6_nocol", "probe6", "stiff5", "grow5", "rand6_col"]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_files([os.path.join(golden_dir, "vxa", n + ".vxa") for n in names])
        eng.run()
        solo = np.stack([parallel.result_to_record(eng.result(i)) for i in range(len(names))])
    assert np.array_equal(t0, solo)


def test_parameter_sweep_vs_oracle(eng_mod, tmp_path):
    """Every switch the evosoro writer exposes, in seeded random combinations (gravity / floor / temperature / sticky
    floor / self-collision on and off, DtFrac, frequency, amplitude, lattice size, stiffnesses, shapes), plus text-level
    edits of the constants it hard-wires (damping ratios, collision system and horizon): 24 robots in one batch against
    the oracle, strict bar on the first steps, conditioning-calibrated bar afterwards."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    # (VXH_SWEEP_SEED / _COUNT / _MAXDIM: wider one-off campaigns with the same generator)
    count, maxdim = int(os.environ.get("VXH_SWEEP_COUNT", "24")), int(os.environ.get("VXH_SWEEP_MAXDIM", "7"))
    rng = np.random.RandomState(int(os.environ.get("VXH_SWEEP_SEED", "2024")))
    os.makedirs(tmp_path / "voxelyzeFiles")
    paths = []
    for k in range(count):
        shape = tuple(int(n) for n in rng.randint(2, maxdim, size=3))
        sim = Sim(dt_frac=float(np.round(rng.uniform(0.3, 0.95), 2)), simulation_time=0.05,
                  fitness_eval_init_time=float(np.round(rng.uniform(0.0, 0.01), 3)),
                  self_collisions_enabled=bool(rng.randint(2)), min_temp_fact=float(np.round(rng.uniform(0.1, 0.6), 2)))
        env = Env(frequency=float(np.round(rng.uniform(2, 8), 1)), gravity_enabled=int(rng.randint(2)), temp_enabled=int(rng.randint(2)),
                  floor_enabled=int(rng.randint(2)), sticky_floor=int(rng.randint(2)), temp_amp=float(np.round(rng.uniform(26, 45), 0)),
                  lattice_dimension=float(rng.choice([0.005, 0.01, 0.02])), fat_stiffness=float(rng.choice([1e6, 5e6])),
                  bone_stiffness=float(rng.choice([5e7, 5e8])), muscle_stiffness=float(rng.choice([5e6, 1e7])))
        if rng.randint(2):
            env.add_param("growth_amplitude", float(np.round(rng.uniform(0.05, 0.4), 2)), "<GrowthAmplitude>")
        per_voxel = None
        if rng.randint(2):
            from collections import OrderedDict
            per_voxel = OrderedDict([("<PhaseOffset>", np.round(rng.uniform(-1, 1, size=shape), 3))])
        ind = workloads.make_individual(k, workloads.random_material(shape, 100 + k, 0.2), per_voxel)
        write_voxelyze_file(sim, env, ind, str(tmp_path), "s")
        path = str(tmp_path / "voxelyzeFiles" / ("s--id_%05i.vxa" % k))
        text = open(path).read()
        for tag, choices in (("BondDampingZ", ["1", "0.5", "0.1"]), ("ColDampingZ", ["0.8", "0.2"]), ("SlowDampingZ", ["0.01", "0.001", "0"]),
                             ("ColSystem", ["3", "1"]), ("CollisionHorizon", ["2", "3"])):
            old = text[text.index("<" + tag + ">"):text.index("</" + tag + ">")]
            text = text.replace(old, "<" + tag + ">" + str(rng.choice(choices)), 1)
        open(path, "w").write(text)
        paths.append(path)
    models = [vo.parse_vxa(p) for p in paths]
    sims = [vo.OracleSim(m) for m in models]
    spreads = [_spread(m, (60, 150))[0] for m in models]
    jittered = set()
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_files(paths)
        for upto in (1, 3, 20, 150):
            eng.step(upto - sims[0].info().steps)
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                lat = models[i]["lattice_dim"]
                tol = FLOOR_VOX if upto <= 20 else max(FLOOR_VOX, 20 * spreads[i])
                err = _pos_err(eng.state(i), o.state(), lat)
                if err > tol and upto > 20:        # (a robot whose instability the one-input twin does not excite: _jitter_spread)
                    tol = max(tol, 20 * _jitter_spread(models[i], upto))
                    jittered.add(i)
                assert err <= tol, (i, upto, err, tol, paths[i])
    assert sum(1 for sp in spreads if sp < 1e-10) >= 0.75 * count      # the strict bar applied to most of them
    assert len(jittered) <= max(1, count // 40)                        # ... and the symmetry-breaking probe was needed for next to none


def test_land_water_parameter_sweep_vs_oracle(eng_mod, tmp_path):
    """The same idea for _voxcad_land_water: fluid on/off, drag coefficient, gravity/floor/temperature switches, phase
    offsets and evolved stiffness, 16 robots in one batch against the oracle."""
    from collections import OrderedDict
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    count, maxdim = int(os.environ.get("VXH_SWEEP_COUNT", "16")), int(os.environ.get("VXH_SWEEP_MAXDIM", "7"))
    rng = np.random.RandomState(int(os.environ.get("VXH_SWEEP_SEED", "777")))
    os.makedirs(tmp_path / "voxelyzeFiles")
    paths = []
    for k in range(count):
        shape = tuple(int(n) for n in rng.randint(2, maxdim, size=3))
        sim = Sim(dt_frac=float(np.round(rng.uniform(0.3, 0.95), 2)), simulation_time=0.05,
                  fitness_eval_init_time=float(np.round(rng.uniform(0.0, 0.01), 3)), self_collisions_enabled=bool(rng.randint(2)))
        env = Env(frequency=float(np.round(rng.uniform(2, 8), 1)), gravity_enabled=int(rng.randint(2)), temp_enabled=int(rng.randint(2)),
                  floor_enabled=int(rng.randint(2)), temp_amp=float(np.round(rng.uniform(26, 45), 0)))
        if rng.randint(3) > 0:
            env.add_param("fluid_environment", 1, "<FluidEnvironment>")
            env.add_param("aggregate_drag_coefficient", float(rng.choice([50.0, 750.0, 3000.0])), "<AggregateDragCoefficient>")
        layers = OrderedDict()
        if rng.randint(2):
            layers["<PhaseOffset>"] = np.round(rng.uniform(-1, 1, size=shape), 3)
        if rng.randint(2):
            layers["<Stiffness>"] = np.round(10 ** rng.uniform(6.0, 8.0, size=shape), 0)
        ind = workloads.make_individual(k, workloads.random_material(shape, 300 + k, 0.2), layers or None)
        write_voxelyze_file(sim, env, ind, str(tmp_path), "w")
        paths.append(str(tmp_path / "voxelyzeFiles" / ("w--id_%05i.vxa" % k)))
    models = [vo.parse_vxa(p, 1) for p in paths]
    sims = [vo.OracleSim(m) for m in models]
    spreads = [_spread(m, (60, 150))[0] for m in models]
    jittered = set()
    with eng_mod.Engine(eng_mod.VOXCAD_LAND_WATER, 0) as eng:
        eng.add_vxa_files(paths)
        for upto in (1, 3, 20, 150):
            eng.step(upto - sims[0].info().steps)
            for i, o in enumerate(sims):
                o.step(upto - o.info().steps)
                tol = FLOOR_VOX if upto <= 20 else max(FLOOR_VOX, 20 * spreads[i])
                err = _pos_err(eng.state(i), o.state(), models[i]["lattice_dim"])
                if err > tol and upto > 20:
                    tol = max(tol, 20 * _jitter_spread(models[i], upto))
                    jittered.add(i)
                assert err <= tol, (i, upto, err, tol, paths[i])
    assert sum(1 for sp in spreads if sp < 1e-10) >= 0.75 * count
    assert len(jittered) <= max(1, count // 40)


def test_in_memory_hand_off_builds_the_same_robots(eng_mod, tmp_path):
    """vxh_add_robots (arrays + one template) against the file route: same counts, same time step, and the same trajectory bit for
    bit -- including per-voxel layers whose values the .vxa text carries with 12 significant digits only"""
    from collections import OrderedDict
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import phenotype_arrays, write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim, env = Sim(dt_frac=0.9, simulation_time=0.3, fitness_eval_init_time=0.02), Env()
    rs = np.random.RandomState(5)
    inds = [workloads.random_robot(i, (6, 6, 6), 30 + i, phase_offset=True) for i in range(6)]        # unrounded random phases
    inds.append(workloads.make_individual(6, workloads.random_material((5, 5, 5), 77),
                                          OrderedDict([("<Stiffness>", 10 ** rs.uniform(6.0, 8.0, size=(5, 5, 5))),
                                                       ("<PhaseOffset>", rs.uniform(-1, 1, size=(5, 5, 5)))])))
    inds.append(workloads.make_individual(7, workloads.random_material((7, 4, 5), 78)))                 # no layer at all, not a cube
    texts = []
    for ind in inds:
        texts.append(write_voxelyze_file(sim, env, ind, str(tmp_path), "m", want_text=True)[1])
    paths = [str(tmp_path / "voxelyzeFiles" / ("m--id_%05i.vxa" % ind.id)) for ind in inds]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as by_file, eng_mod.Engine(eng_mod.VOXCAD, 0) as by_array:
        by_file.add_vxa_files(paths)
        first = by_array.add_robots(texts[3], [phenotype_arrays(ind) + ("fitnessFiles/softbotsOutput--id_%05i.xml" % ind.id,) for ind in inds])
        assert first == 0 and by_array.num_robots() == len(inds)
        for i in range(len(inds)):
            assert by_file.dims(i) == by_array.dims(i), i
            assert by_array.fitness_file_name(i) == "fitnessFiles/softbotsOutput--id_%05i.xml" % inds[i].id
        by_file.step(400)
        by_array.step(400)
        for i in range(len(inds)):
            assert np.array_equal(by_file.state(i), by_array.state(i)), i
    # refusals: a layer the engine does not model, a material outside the palette
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as bad:
        with pytest.raises(eng_mod.VxhError) as err:
            bad.add_robots(texts[0], [(np.ones((2, 2, 2), dtype=int), OrderedDict([("<VestigialLimbs>", np.zeros((2, 2, 2)))]), None)])
        assert err.value.status == -7
        with pytest.raises(eng_mod.VxhError):
            bad.add_robots(texts[0], [(np.full((2, 2, 2), 9), OrderedDict(), None)])
        assert bad.num_robots() == 0
        # all or nothing: a bad robot after good ones adds none of the call's robots, and the engine stays usable
        good = (np.ones((2, 2, 2), dtype=int), OrderedDict(), None)
        with pytest.raises(eng_mod.VxhError):
            bad.add_robots(texts[0], [good, good, (np.full((2, 2, 2), 9), OrderedDict(), None)])
        assert bad.num_robots() == 0
        assert bad.add_robots(texts[0], [good, good]) == 0 and bad.num_robots() == 2
        with pytest.raises(eng_mod.VxhError):
            bad.add_robots(texts[0], [good, (np.ones((2, 2, 2), dtype=int), OrderedDict([("<VestigialLimbs>", np.zeros((2, 2, 2)))]), None)])
        assert bad.num_robots() == 2
        bad.step(10)
        assert all(bad.result(i).steps == 10 for i in range(2))


@pytest.mark.parametrize("in_memory", [False, True])
def test_evaluate_all_with_the_real_engine(eng_mod, golden_dir, manifest, tmp_path, in_memory):
    """BASELINE configs[0] end to end through the recommended route: evaluate_all -> run_population ->
    libvxhip, NOT the stub engine of the CPU suite.  The basic.py-style 6x6x6 locomotor (0.5 s) and a second generation with
    another golden robot; objective values must equal what the reference's read_voxlyze_results parsed out of the reference
    binary's result XML (tests/golden/manifest.json), six digits; md5 keys, cache and file housekeeping as evaluation.py:18-219."""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env, ObjectiveDict
    from evosoro_amd.tools.evaluation import evaluate_all

    class Log(object):
        lines = []

        def message(self, text):
            self.lines.append(str(text))

    class Pop(list):
        pass

    def make_pop(inds, gen):
        pop = Pop(inds)
        pop.objective_dict = ObjectiveDict()
        pop.objective_dict.add_objective(name="fitness", maximize=True, tag="<NormFinalDist>")
        pop.objective_dict.add_objective(name="age", maximize=False, tag=None)
        pop.objective_dict.add_objective(name="y", maximize=True, tag="<finalDistY>")
        pop.objective_dict.add_objective(name="touch", maximize=True, tag="<NumTouchingFloor>")
        pop.gen, pop.pop_size, pop.total_evaluations, pop.best_fit_so_far = gen, len(inds), 0, -1e9
        pop.already_evaluated, pop.all_evaluated_individuals_ids = {}, []
        for ind in pop:
            ind.fitness, ind.age, ind.y, ind.touch = -10e6, 0, -10e6, -10e6
        return pop

    run = str(tmp_path / "run")
    for d in ("voxelyzeFiles", "fitnessFiles", "tempFiles", "bestSoFar/fitOnly", "ancestors", "Gen_0000", "Gen_0001"):
        os.makedirs(os.path.join(run, d))
    env, log = Env(), Log()
    probe = workloads.make_individual(0, workloads.probe_material())
    clone = workloads.make_individual(7, workloads.probe_material())
    pop = make_pop([probe, clone], 0)
    # the clone differs in id only: with zero actuation variance the reference evaluates both (the cache is filled after the
    # generation) and both get the same value
    evaluate_all(Sim(dt_frac=0.9, simulation_time=0.5, fitness_eval_init_time=0.1), env, pop, log, save_vxa_every=1,
                 run_directory=run, run_name="E", in_memory=in_memory)
    want = manifest["probe6"]
    assert probe.md5 == clone.md5 == want["md5"]
    for ind in (probe, clone):
        assert (ind.fitness, ind.y, ind.touch) == (want["read_results"]["0"], want["read_results"]["2"], want["read_results"]["3"])
    assert pop.total_evaluations == 2 and pop.all_evaluated_individuals_ids == [0, 7] and pop.best_fit_so_far == probe.fitness
    assert os.listdir(os.path.join(run, "fitnessFiles")) == [] and os.listdir(os.path.join(run, "voxelyzeFiles")) == []
    assert len(os.listdir(os.path.join(run, "Gen_0000"))) == 2 and len(os.listdir(os.path.join(run, "bestSoFar/fitOnly"))) == 1

    other = workloads.random_robot(2, (6, 6, 6), 7)           # = golden case rand6_col
    again = workloads.make_individual(9, workloads.probe_material())
    pop2 = make_pop([other, again], 1)
    pop2.already_evaluated, pop2.best_fit_so_far = pop.already_evaluated, pop.best_fit_so_far
    evaluate_all(Sim(dt_frac=0.9, simulation_time=0.25, fitness_eval_init_time=0.1), env, pop2, log, save_vxa_every=0,
                 run_directory=run, run_name="E", save_lineages=True, in_memory=in_memory)
    want2 = manifest["rand6_col"]
    assert other.md5 == want2["md5"]
    assert (other.fitness, other.y, other.touch) == (want2["read_results"]["0"], want2["read_results"]["2"], want2["read_results"]["3"])
    assert again.fitness == probe.fitness and pop2.total_evaluations == 1     # served from the md5 cache
    assert pop2.best_fit_so_far == other.fitness and len(os.listdir(os.path.join(run, "bestSoFar/fitOnly"))) == 2
    assert os.listdir(os.path.join(run, "ancestors")) == ["E--id_00002.vxa"]
    assert not any("WARNING" in l for l in log.lines)


def _full_batch_vs_reference(eng_mod, golden_dir, tmp_path, variant, prefix, make_ind, sim, env, tags):
    """64 robots stepped through their whole evaluation in one batch; robots 0, 21, 42 and 63 of the batch are golden cases whose final
    state and result XML come from the reference binary"""
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    from oracle import vxoracle as vo
    os.makedirs(tmp_path / "voxelyzeFiles")
    golden = {0: "%s_00" % prefix, 21: "%s_21" % prefix, 42: "%s_42" % prefix, 63: "%s_63" % prefix}
    paths = []
    for i in range(64):
        if i in golden:
            paths.append(os.path.join(golden_dir, "vxa", golden[i] + ".vxa"))
        else:
            ind = make_ind(i)
            write_voxelyze_file(sim, env, ind, str(tmp_path), "full")
            paths.append(str(tmp_path / "voxelyzeFiles" / ("full--id_%05i.vxa" % ind.id)))
    with eng_mod.Engine(variant, 0) as eng:
        eng.add_vxa_files(paths)
        eng.run()
        statuses = [eng.result(i).status for i in range(64)]
        assert statuses == [eng_mod.ROBOT_FINISHED] * 64
        steps = {eng.result(i).steps for i in range(64)}
        assert all(np.isfinite(eng.state(i)).all() for i in range(0, 64, 7))
        worst = 0.0
        for i, name in golden.items():
            model = vo.parse_vxa(paths[i], variant)
            lat = model["lattice_dim"]
            planned = eng.dims(i)["planned_steps"]
            tol = max(FLOOR_VOX, 20 * _spread(model, (planned // 4, planned // 2, planned))[0])
            trace = vo.read_trace(os.path.join(golden_dir, "expected", name + ".final.bin"))
            want = vo.read_result_xml(os.path.join(golden_dir, "expected", name + ".xml"))
            res = eng.result(i)
            assert res.steps == trace["total_steps"] == planned, name
            err = _pos_err(eng.state(i), trace["records"][-1]["state"], lat)
            worst = max(worst, err / tol)
            assert err <= tol, (name, err, tol)
            assert np.abs(np.array(res.cur_cm) - trace["cur_cm"]).max() / lat <= tol, name
            assert np.abs(np.array(res.ini_cm) - trace["ini_cm"]).max() / lat <= tol, name
            for tag, field in tags:
                val = getattr(res, field)
                assert abs(val - want[tag]) <= 2 * tol + 1e-5 * abs(want[tag]), (name, tag, val, want[tag])
        print("%s: 64 robots, step counts %s, worst error / bar over the four golden robots %.3g" % (prefix, sorted(steps)[:3], worst))


def test_configs1_whole_batch_full_duration_vs_reference(eng_mod, golden_dir, tmp_path):
    """BASELINE configs[1] at its stated size and duration: 64 random 6x6x6 walkers, 0.5 s (7806 steps each)"""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    _full_batch_vs_reference(eng_mod, golden_dir, tmp_path, eng_mod.VOXCAD, "cfg1", lambda i: workloads.random_robot(100 + i, (6, 6, 6), i),
                             Sim(dt_frac=0.9, simulation_time=0.5, fitness_eval_init_time=0.1), Env(),
                             [("NormFinalDist", "norm_final_dist"), ("finalDistY", "final_dist_y"), ("AnteriorDist", "anterior_dist"),
                              ("PosteriorY", "posterior_y")])


def test_configs3_whole_batch_full_duration_vs_reference(eng_mod, golden_dir, tmp_path):
    """BASELINE configs[3] at its stated size and duration: 64 random 8x8x8 swimmers of _voxcad_land_water in a fluid (per-facet drag,
    gravity and floor off), 0.5 s each"""
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    env_w = Env()
    env_w.add_param("fluid_environment", 1, "<FluidEnvironment>")
    env_w.add_param("aggregate_drag_coefficient", 750.0, "<AggregateDragCoefficient>")
    _full_batch_vs_reference(eng_mod, golden_dir, tmp_path, eng_mod.VOXCAD_LAND_WATER, "cfg3", lambda i: workloads.swimmer(200 + i, (8, 8, 8), i),
                             Sim(dt_frac=0.9, simulation_time=0.5, fitness_eval_init_time=0.05), env_w,
                             [("normAbsoluteDisplacement", "norm_abs_disp"), ("normDistX", "norm_dist_x"), ("normDistY", "norm_dist_y"),
                              ("normDistZ", "norm_dist_z")])


def test_cm_trace_in_the_result_file(eng_mod, golden_dir, tmp_path):
    """<TimeBetweenTraces> + <SaveTraces> (VX_Sim.cpp:1537-1547, VX_SimGA.cpp:170-184): the trace points are recorded on the device at the
    end of the step in which they fall due; times equal the reference's, centres of mass within the parity bar; the result XML carries
    them like the reference's; a robot without the tags in the same batch has none"""
    import re
    from oracle import vxoracle as vo
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("steps_per_launch", 100)          # launch boundaries inside the run, also right at trace steps
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "trace4.vxa"))
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "phase4.vxa"))
        eng.run()
        got = eng.cm_trace(0)
        assert eng.cm_trace(1).shape == (0, 4)
        sim = vo.OracleSim.from_vxa(os.path.join(golden_dir, "vxa", "trace4.vxa"))
        sim.step(-1)
        want = sim.cm_trace()
        assert got.shape == want.shape == (13, 4)
        assert np.array_equal(got[:, 0], want[:, 0])                         # the times: CurTime is a sum of identical dt's, bitwise
        model = vo.parse_vxa(os.path.join(golden_dir, "vxa", "trace4.vxa"))
        tol = max(FLOOR_VOX, 20 * _spread(model, (1000, 2000, eng.dims(0)["planned_steps"]))[0])
        assert np.abs(got[:, 1:] - want[:, 1:]).max() / model["lattice_dim"] <= tol
        out = str(tmp_path / "trace.xml")
        eng.write_result_xml(0, out)
        text, ref = open(out).read(), open(os.path.join(golden_dir, "expected", "trace4.xml")).read()
        assert text.count("<TraceStep>") == ref.count("<TraceStep>") == 13
        for tag in ("Time", "TraceX", "TraceY", "TraceZ"):
            a = [float(v) for v in re.findall(r"<%s>(.*?)</%s>" % (tag, tag), text)]
            b = [float(v) for v in re.findall(r"<%s>(.*?)</%s>" % (tag, tag), ref)]
            assert np.allclose(a, b, rtol=2e-6, atol=2 * tol * model["lattice_dim"])
        # same structure as the reference file: <Fitness> block, then <CMTrace>
        assert re.sub(r">[^<>\n]+<", "><", text) == re.sub(r">[^<>\n]+<", "><", ref)
        eng.write_result_xml(1, out)
        assert "<CMTrace>" not in open(out).read()
    # the streaming kernels record the same trace (k_step_begin, also in the call that only finishes the last step)
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.set_option("tiled", 0)
        eng.set_option("fused", 0)
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "trace4.vxa"))
        eng.run()
        streamed = eng.cm_trace(0)
        assert streamed.shape == (13, 4) and np.array_equal(streamed[:, 0], want[:, 0])
        assert np.abs(streamed[:, 1:] - want[:, 1:]).max() / model["lattice_dim"] <= tol


def test_device_side_result_reductions_equal_the_host_path(eng_mod, golden_dir):
    """vxh_get_result of a _voxcad robot comes from reductions done on the device (k_results: centre of mass summed in voxel order,
    extrema, floor-contact counts) -- every field must equal, bit for bit, what the host computes from the downloaded voxel state
    (option host_results = 1), after the first step, mid-run and at the end"""
    names = CASES + ["bench10_0"]
    seen = {}
    for host in (0, 1):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("host_results", host)
            for n in names:
                eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
            eng.step(1)
            out = [[eng.result(i).as_dict() for i in range(len(names))]]
            eng.step(332)
            out.append([eng.result(i).as_dict() for i in range(len(names))])
            eng.run()
            out.append([eng.result(i).as_dict() for i in range(len(names))])
            seen[host] = out
    assert seen[0] == seen[1]
    assert all(r["status"] == eng_mod.ROBOT_FINISHED and r["num_touching_floor"] > 0 for r in seen[0][2])


def test_collision_rows_longer_than_64_partners(eng_mod, tmp_path):
    """The reference's collision lists have no cap (CVX_Sim::CreateColBond, VX_Sim.cpp:753-769).  A folded sheet with
    <CollisionHorizon> 5 gives the voxels of its inner plates rows of far more than 64 partners (rounds 1-2 ended such a robot with
    VXH_ROBOT_COL_OVERFLOW): the engine must follow the oracle through the flapping, contacts included; with the option col_cap = 64
    the same robot must be reported as overflowed while the other robot of the batch is untouched, bit for bit."""
    import re
    from oracle import vxoracle as vo
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    os.makedirs(tmp_path / "voxelyzeFiles")
    sim = Sim(dt_frac=0.9, simulation_time=0.6, fitness_eval_init_time=0.02)
    env = Env(temp_amp=39, frequency=8.0)
    paths = []
    for i, mat in enumerate((workloads.folded_material(), workloads.random_material((6, 6, 6), 7))):
        write_voxelyze_file(sim, env, workloads.make_individual(i, mat), str(tmp_path), "fold")
        p = str(tmp_path / "voxelyzeFiles" / ("fold--id_%05i.vxa" % i))
        text, n = re.subn(r"<CollisionHorizon>[^<]*</CollisionHorizon>", "<CollisionHorizon>5</CollisionHorizon>", open(p).read())
        assert n == 1
        open(p, "w").write(text)
        paths.append(p)
    models = [vo.parse_vxa(p) for p in paths]
    sims = [vo.OracleSim(m) for m in models]
    checkpoints = (1, 10, 100, 400, 900)
    spreads = [_spread(m, checkpoints) for m in models]
    # the folded sheet flaps through hundreds of contacts: next to the twin with one constant changed by an ulp, two twins that get
    # one-ulp noise in every position and quaternion before every step (what an implementation with other roundings amounts to;
    # measured: one step of engine and oracle from the same state differ by 2e-15 voxel, one step of the oracle under this noise
    # by 3e-15, scripts/dev_gpu_diag.py drift7) -- the largest of the three spreads counts
    for i, m in enumerate(models):
        worst = spreads[i][0]
        for seed in (1, 100003):
            a, b = vo.OracleSim(m), vo.OracleSim(m)
            for upto in checkpoints:
                a.step(upto - a.info().steps)
                b.step_jittered(upto - b.info().steps, seed=seed)
                worst = max(worst, _pos_err(a.state(), b.state(), m["lattice_dim"]))
        spreads[i] = (worst, spreads[i][1])
    states = {}
    for cap in (0, 64):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("col_cap", cap)
            for p in paths:
                eng.add_vxa_file(p)
            done = 0
            for upto in checkpoints:
                eng.step(upto - done)
                done = upto
                if cap == 0:
                    for i in range(2):
                        sims[i].step(upto - sims[i].info().steps)
                        want, got = sims[i].state(), eng.state(i)
                        tol = FLOOR_VOX if upto <= 10 else max(FLOOR_VOX, 20 * spreads[i][0])
                        assert _pos_err(got, want, models[i]["lattice_dim"]) <= tol, (i, upto, _pos_err(got, want, models[i]["lattice_dim"]), tol)
            states[cap] = [eng.state(i) for i in range(2)]
            status = [eng.result(i).status for i in range(2)]
            rebuilds = eng.result(0).col_rebuilds
        if cap == 0:
            assert status == [eng_mod.ROBOT_PENDING, eng_mod.ROBOT_PENDING]
            info = sims[0].info()
            assert rebuilds == info.col_rebuilds and rebuilds >= 2
            assert 2 * info.ncol > 64 * info.nsurf                      # a collision bond sits in two rows: more than 64 partners per row ON AVERAGE
        else:
            assert status[0] == eng_mod.ROBOT_COL_OVERFLOW and status[1] == eng_mod.ROBOT_PENDING
    assert np.array_equal(states[0][1], states[64][1])                    # the neighbour in the batch: the same bits either way


def test_one_step_from_the_same_state(eng_mod, golden_dir, manifest, kernel_path):
    """What ONE step of the engine and of the oracle differ by when both start from the same state (the oracle is put on the engine's
    state before every step: oracle instrument vxo_set_state).  Differences of earlier steps cannot hide or feed anything here, so the
    bar can sit at the rounding level: 5e-14 voxel and 2e-11 of the largest velocity / angular velocity, step after step (measured
    2e-15 voxel, 3e-13, 1e-12; one-ulp noise on the oracle's own inputs gives 3e-15, 4e-13, 1.4e-12).  Round 3's systematic creep
    was a formula difference of 1.2e-12 voxel per step in exactly this number (kernels_math.hpp RotInv) that 7806-step trajectories within
    1e-10 voxel had not shown.
    Round 5: EVERY case of the parity ledger (tests/golden/manifest.json, 31 robots: all BASELINE configs at full size, both simulators,
    the 1000-voxel lattice of the 1024-thread variant, the shipped .vxa files), on each of the three kernel paths -- so that the
    ill-conditioned robots (phase4 / trace4: whole runs only held to 20 x their own spread, 0.06 voxel) are pinned at the rounding level
    per step like everything else.  300 steps each (the whole run where it is shorter; phase4's whole 742)."""
    from oracle import vxoracle as vo
    longer = {"phase4": 742, "trace4": 742, "lw_hexapus": 400, "bench10_0": 400}
    report = []
    for name, entry in manifest.items():
        variant = 1 if entry["variant"] == "lw" else 0
        path = os.path.join(golden_dir, "vxa", name + ".vxa")
        model = vo.parse_vxa(path, variant)
        lat = model["lattice_dim"]
        sim, twin = vo.OracleSim(model), vo.OracleSim(model)
        worst = [0.0, 0.0, 0.0]
        flips = taken = noisy = 0
        with eng_mod.Engine(variant, 0) as eng:
            eng.add_vxa_file(path)
            nsteps = min(longer.get(name, 300), eng.dims(0)["planned_steps"])
            prev = sim.state()
            for step in range(1, nsteps + 1):
                eng.step(1)
                got = eng.state(0)
                sim.set_state(prev)
                sim.step(1)
                want = sim.state()
                # the reference algorithm's OWN one-step noise: the same step from the same state with every position and quaternion
                # component moved by one ulp.  Mostly 3e-15 voxel -- but at the ONSET of a bond's rotation (relative rotations of 1e-8 ..
                # 1e-5 rad, e.g. when the compression wave of a landing robot reaches the bond) ToRotationVector's 1 - w * w
                # (Vec3D.h:270-285) is a difference of numbers an ulp apart, and the reference's step moves by up to 3e-9 voxel under
                # that noise (found by this test on the reference's own example_phaseoffset.vxa, steps 8-29; scripts/dev_gpu_diag.py
                # onestep).  Such steps are held to 4 x that noise instead of to 5e-14.
                twin.set_state(prev)
                twin.step_jittered(1, seed=step)
                own = np.abs(twin.state() - want)
                own_p = own[:, :3].max() / lat
                own_v = own[:, 8:11].max() / max(1e-300, np.abs(want[:, 8:11]).max())
                own_w = own[:, 11:14].max() / max(1e-300, np.abs(want[:, 11:14]).max())
                d = np.abs(got - want)
                dp = d[:, :3].max() / lat
                dv = d[:, 8:11].max() / max(1e-300, np.abs(want[:, 8:11]).max())
                dw = d[:, 11:14].max() / max(1e-300, np.abs(want[:, 11:14]).max())
                if own_p > 1e-14:
                    noisy += 1
                    assert dp <= max(5e-14, 4 * own_p) and dv <= max(2e-11, 4 * own_v) and dw <= max(2e-11, 4 * own_w), (name, step, dp, own_p, dv, own_v, dw, own_w)
                elif dp > 5e-14:        # a bond whose small- / large-angle test sits within an ulp of its threshold may flip on one side only
                    flips += 1
                else:
                    worst = [max(worst[0], dp), max(worst[1], dv), max(worst[2], dw)]
                prev = got
                taken += 1
            kernel = eng.counters().dominant_block
        report.append((name, taken, kernel, worst, flips))
        print("%s [%s, kernel %d]: one step from the same state, worst over %d steps: %.1e voxel, velocity %.1e, angular velocity %.1e; steps set aside: %d; "
              "steps on which the reference's own one-ulp noise exceeds 1e-14 voxel (held to 4 x it): %d" % (
                  name, kernel_path, kernel, taken, worst[0], worst[1], worst[2], flips, noisy))
        assert taken >= min(10, nsteps), (name, taken)
        assert flips <= 2, (name, flips)
        assert worst[1] <= 2e-11 and worst[2] <= 2e-11, (name, worst)
    assert len(report) >= 31


def test_the_second_pose_tile_of_the_wide_kernel_changes_no_bit(eng_mod, golden_dir):
    """Option wide_two_tiles: the wide kernel writes a step's new poses into a second LDS tile and steps with two workgroup barriers
    instead of three; the collision-horizon update is then evaluated by every thread from ping-pong control words.  Scheduling only:
    every voxel of walkers, colliding robots, swimmers and growing robots must come out bit for bit as with one tile, at a checkpoint
    inside the run (launch boundaries in between) and at the end."""
    names = [("cfg1_00", 0), ("rand6_col", 0), ("grow5", 0), ("stiff5", 0), ("lw_swim6", 1), ("lw_land6", 1)]
    for variant in (0, 1):
        mine = [n for n, v in names if v == variant]
        runs = []
        for two in (1, 0):
            with eng_mod.Engine(variant, 0) as eng:
                eng.set_option("wide", 1)
                eng.set_option("tiled", 0)
                eng.set_option("wide_two_tiles", two)
                eng.set_option("steps_per_launch", 37)
                for n in mine:
                    eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
                eng.step(300)
                mid = [eng.state(i) for i in range(len(mine))]
                eng.run()
                runs.append((mid, [eng.state(i) for i in range(len(mine))], [eng.result(i).as_dict() for i in range(len(mine))], eng.counters().dominant_block))
        assert runs[0][3] == 513                       # (the wide kernel stepped them)
        for i, n in enumerate(mine):
            assert np.array_equal(runs[0][0][i], runs[1][0][i]), n
            assert np.array_equal(runs[0][1][i], runs[1][1][i]), n
            a, b = runs[0][2][i], runs[1][2][i]
            assert all(a[k] == b[k] for k in a if k != "reserved"), n


def test_large_resident_robots_step_the_same_in_two_calls_as_in_one(eng_mod, tmp_path, kernel_path):
    """Robots of 513-1024 voxels on the resident kernels (k_robot_steps<768> and <1024>; tiled = 0), self-collision, broad-phase runs and the
    IniCM latch included: 300 steps taken as 120 + 180 -- the second call reads back the saved image of the contact rows and the bond
    history the first one left -- must give every voxel of every robot BIT FOR BIT as one call of 300 steps in a fresh engine, one robot
    of exactly 1024 voxels (the last slot of the largest size class) among them.  Also against the oracle."""
    if kernel_path != "auto":
        pytest.skip("the test sets the kernel options itself")
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from oracle import vxoracle as vo
    sim, env = Sim(dt_frac=0.9, simulation_time=0.05, fitness_eval_init_time=0.004), Env()
    mats = [workloads.full_material(10, 2), workloads.random_material((10, 10, 10), 5001, p_empty=0.15),
            np.pad(workloads.full_material(10, 3), ((0, 0), (0, 0), (0, 1)), constant_values=0),          # (a lattice one layer short of a second size class)
            workloads.random_material((10, 10, 10), 5)]
    mats[2][:5, :5, 10] = 1
    mats[2][0, 0, 10] = 0                                    # 1024 voxels exactly
    paths = [_write_robot(tmp_path, k, m, sim, env, "pr") for k, m in enumerate(mats)]
    runs = []
    for pieces in ((120, 180), (300,)):                      # (past InitCmTime; two launches: the saved image of the contact rows is read back)
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 0)
            for p in paths:
                eng.add_vxa_file(p)
            assert [eng.dims(i)["nvox"] for i in range(4)][2] == 1024
            for n in pieces:
                eng.step(n)
            runs.append(([eng.state(i) for i in range(4)], [eng.result(i).col_rebuilds for i in range(4)], [eng.result(i).as_dict() for i in range(4)]))
    for i in range(4):
        assert np.array_equal(runs[0][0][i], runs[1][0][i]), i
        assert runs[0][2][i] == runs[1][2][i], i            # every result field, IniCM included
    assert runs[0][1] == runs[1][1] and min(runs[0][1]) >= 1
    sim_o = vo.OracleSim.from_vxa(paths[1])
    sim_o.step(300)
    assert _pos_err(runs[0][0][1], sim_o.state(), 0.01) < FLOOR_VOX


def test_option_table(eng_mod, golden_dir, kernel_path):
    """vxh_set_option, key by key: which values are refused (VXH_ERR_ARG, -1), which keys are unknown (-1 too), and what a batch that has
    stepped still accepts: an option that is part of the assembled batch only at the value it has (VXH_ERR_STATE, -6, otherwise -- judged
    BEFORE the value's range, and after the value's coercion to what would be stored), the others always; after a reset, everything."""
    if kernel_path != "auto":
        pytest.skip("the test sets the kernel options itself")

    def status(eng, key, val):
        try:
            eng.set_option(key, val)
        except eng_mod.VxhError as e:
            return e.status
        return 0

    nan = float("nan")
    refused = [("shape_descriptors", (2, -1, 0.5, nan)), ("steps_per_launch", (0, 0.5, -3, 200001, nan)), ("graph_steps", (-1, 1000001, nan)),
               ("wide", (2, -1, 0.5, nan)), ("wide_two_tiles", (2, -1, 0.5, nan)), ("fused", (2, -1, 0.5, nan)), ("tile_small", (2, -1, 0.5, nan)),
               ("col_cap", (-1, 1000001, nan)), ("tiled", (3, -1, 0.5, 1.5, nan)), ("tiles_per_robot", (-1, 4097, nan))]
    accepted = [("host_results", (1, 2, -1, 0.5, 0)), ("shape_descriptors", (1, 0)), ("steps_per_launch", (1, 1.5, 200000, 1024)), ("graph_steps", (0, 1000000, 32)),
                ("wide", (0, 1)), ("wide_two_tiles", (0, 1)), ("fused", (0, 1)), ("tile_small", (1, 0)), ("col_cap", (1000000, 7.9, 0)),
                ("tiled", (0, 2, 1)), ("tiles_per_robot", (4096, 3.7, 0))]           # (the last value of each: the default)
    batch_now = [("tiled", 1), ("tiles_per_robot", 0), ("tile_small", 0), ("wide", 1), ("wide_two_tiles", 1), ("col_cap", 0), ("fused", 1)]
    batch_other = [("tiled", 0), ("tiled", 2), ("tiles_per_robot", 3), ("tile_small", 1), ("wide", 0), ("wide_two_tiles", 0), ("col_cap", 7), ("fused", 0)]
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "rand6_col.vxa"))
        for key, vals in refused:
            for v in vals:
                assert status(eng, key, v) == -1, (key, v)
        for key in ("pair", "pair_sel", "dbg", "tile", "Wide", "wide ", ""):          # (dbg: the developer library's)
            for v in (0, 1):
                assert status(eng, key, v) == -1, (key, v)
        for key, vals in accepted:
            for v in vals:
                assert status(eng, key, v) == 0, (key, v)
        eng.step(1)
        assert eng.counters().dominant_block == 513            # (the defaults are back: the wide kernel)
        for key, v in batch_now:
            assert status(eng, key, v) == 0, (key, v)
        for key, v in batch_other:
            assert status(eng, key, v) == -6, (key, v)
        # the state is judged first, on the coerced value: flags by != 0, integers truncated
        for key, v, want in (("tiled", 5, -6), ("tiles_per_robot", 5000, -6), ("col_cap", -1, -6), ("fused", nan, -1),
                             ("wide", 2, -1), ("tile_small", 0.5, -6), ("tiled", 1.5, -1), ("col_cap", 0.9, 0), ("tiles_per_robot", 0.9, 0)):
            assert status(eng, key, v) == want, (key, v)
        for key, v in (("steps_per_launch", 7), ("graph_steps", 0), ("host_results", 1), ("host_results", 0), ("shape_descriptors", 0)):
            assert status(eng, key, v) == 0, (key, v)
        assert status(eng, "steps_per_launch", 0) == -1 and status(eng, "graph_steps", -1) == -1
        eng.step(1)
        assert eng.result(0).steps == 2 and eng.counters().dominant_block == 513      # (nothing refused took effect)
        eng.reset()
        for key, v in batch_other:
            assert status(eng, key, v) == 0, (key, v)
        for key, v in batch_now:
            if key not in ("tiled", "wide"):
                assert status(eng, key, v) == 0, (key, v)
        assert status(eng, "tiled", 0) == 0
        eng.step(1)
        assert eng.result(0).steps == 1 and eng.counters().dominant_block == 256      # (tiled = 0, wide = 0 took effect: k_robot_steps<256>)


def test_kernel_choice_options_are_part_of_the_assembled_batch(eng_mod, golden_dir, kernel_path):
    """Which kernel steps a robot decides where its bond history lives (the resident / wide kernels keep 48-byte records of their own, and a
    saved image of the contact rows; the streaming / tiled ones the planes): once a step has been taken, `fused`, `wide`, `wide_two_tiles`,
    `tiled`, `tile_small`, `tiles_per_robot` and `col_cap` are refused (VXH_ERR_STATE) instead of silently handing a robot another kernel's stale history (round-4 advisor finding for `fused`);
    right after a reset they are accepted, and an unchanged value is always fine."""
    if kernel_path != "auto":
        pytest.skip("the test sets the kernel options itself")
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        eng.add_vxa_file(os.path.join(golden_dir, "vxa", "rand6_col.vxa"))
        eng.set_option("fused", 1)
        eng.step(10)
        for key, val in (("fused", 0), ("wide_two_tiles", 0), ("wide", 0), ("tiled", 0), ("tile_small", 1), ("col_cap", 7), ("tiles_per_robot", 3)):
            with pytest.raises(eng_mod.VxhError) as refusal:
                eng.set_option(key, val)
            assert refusal.value.status == -6, key          # (VXH_ERR_STATE: for the state of the batch, not for an unknown name)
        eng.set_option("fused", 1)              # unchanged: accepted, the batch stays
        before = eng.state(0)
        eng.step(10)
        eng.reset()
        eng.set_option("fused", 0)              # right after a reset: accepted
        eng.step(20)
        streamed = eng.state(0)
        eng.reset()
        eng.set_option("fused", 1)
        eng.step(20)
        assert np.abs(eng.state(0)[:, :8] - streamed[:, :8]).max() < 1e-12 and before.shape == streamed.shape


def test_short_calls_dispatch_due_robots_first_and_change_nothing(eng_mod, tmp_path, kernel_path):
    """Launches of at most VXH_ORDER_MAX_STEPS steps hand the robots that are due for a broad-phase run to the first workgroups
    (kernels_fused.hpp fused_dispatch_slot; the bits are written by the previous launch).  The assignment must be a permutation -- every
    robot steps exactly once per launch -- and, the robots being independent, invisible: 70 colliding robots (a list that does not fill
    its last 64-bit word) stepped 24 x 25 steps come out bit for bit as stepped 600 steps in one call, broad-phase runs included."""
    if kernel_path != "auto":
        pytest.skip("resident kernels: the default path")
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    sim, env = Sim(dt_frac=0.9, simulation_time=0.2, fitness_eval_init_time=0.004), Env()
    paths = [_write_robot(tmp_path, k, workloads.random_material((10, 10, 10), 9100 + k, p_empty=0.25 + 0.002 * k), sim, env, "od") for k in range(70)]
    outs = []
    for pieces in ([25] * 24, [600]):
        with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
            eng.set_option("tiled", 0)
            for p in paths:
                eng.add_vxa_file(p)
            assert all(eng.dims(i)["nvox"] > 512 for i in range(len(paths)))        # (k_robot_steps, not the wide kernel)
            for n in pieces:
                eng.step(n)
            assert [eng.result(i).steps for i in range(len(paths))] == [600] * len(paths)
            outs.append(([eng.state(i) for i in range(len(paths))], [eng.result(i).col_rebuilds for i in range(len(paths))]))
    assert outs[0][1] == outs[1][1] and max(outs[0][1]) >= 2
    for a, b in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(a, b)
