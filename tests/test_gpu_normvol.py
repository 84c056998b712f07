"""<NormDistByVol> on the GPU (-m gpu): the three traces UpdateStats keeps under the option (VX_Sim.cpp:1537-1597) and the Norm tags
WriteResultFile sums from them (VX_SimGA.cpp:57-112), against the reference binary's own result files of four developing robots
(tests/golden/expected/normvol_*.xml, written by tests/golden/make_normvol_golden.py; kept there only because the reference prints the
identical file with gravity moved by one ulp, so every printed digit is the robot's and not the arithmetic's).

Tolerance: rtol 2e-6, one unit of the sixth printed digit (the figure of test_cm_trace_in_the_result_file), plus for the sums
atol = 2 * 1e-9 * n / Vmin^e: the 1e-9-voxel parity floor of tests/test_gpu_parity.py on both ends of each of the n intervals,
divided by the smallest volume of the trace to the exponent.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["normvol_a", "normvol_b", "normvol_c", "normvol_d"]
# the four kernel paths the suite distinguishes (conftest.py), set explicitly: wide kernel, resident kernel, tiled kernel, streaming kernels
PATHS = {"default": dict(tiled=1, tiles_per_robot=0, wide=1, fused=1), "wide_off": dict(tiled=1, tiles_per_robot=0, wide=0, fused=1),
         "tiles3": dict(tiled=2, tiles_per_robot=3, wide=1, fused=1), "streaming": dict(tiled=0, tiles_per_robot=0, wide=1, fused=0)}
RTOL, FLOOR_VOX = 2e-6, 1e-9


@pytest.fixture(scope="module")
def eng_mod():
    from evosoro_amd import engine
    return engine


def _tags(text, tag):
    return np.array([float(v) for v in re.findall(r"<%s>(.*?)</%s>" % (tag, tag), text)])


def _reference(golden_dir, name):
    """the reference file of a fixture: its text, the Norm tags, the life trace as printed, exponent and lattice constant of the .vxa"""
    text = open(os.path.join(golden_dir, "expected", name + ".xml")).read()
    vxa = open(os.path.join(golden_dir, "vxa", name + ".vxa")).read()
    cm, vol = text[:text.index("<VolumeTrace>")], text[text.index("<VolumeTrace>"):]
    return {"text": text, "final": _tags(text, "NormFinalDist")[0], "regime": _tags(text, "NormRegimeDist")[0], "frozen": _tags(text, "NormFrozenDist")[0],
            "time": _tags(cm, "Time"), "y": _tags(cm, "TraceY"), "vol_time": _tags(vol, "Time"), "vol": _tags(vol, "Volume"),
            "exponent": _tags(vxa, "NormalizationExponent")[0], "lat": _tags(vxa, "Lattice_Dim")[0],
            "afterlife": _tags(vxa, "AfterlifeTime")[0], "freeze": _tags(vxa, "MidLifeFreezeTime")[0]}


def _run(eng_mod, golden_dir, names, options, tmp_path=None, extra=()):
    """all traces, results and (with tmp_path) result files of the robots, stepped in one batch under the options"""
    out = []
    with eng_mod.Engine(eng_mod.VOXCAD, 0) as eng:
        for key, value in options.items():
            eng.set_option(key, value)
        eng.set_option("steps_per_launch", 100)               # launch boundaries inside the run, also right at trace steps
        for n in list(names) + list(extra):
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        eng.run()
        for i, n in enumerate(names):
            rec = {"cm": [eng.cm_trace(i, w) for w in range(3)], "vol": [eng.volume_trace(i, w) for w in range(3)], "result": eng.result(i).as_dict(),
                   "cm_plain": eng.cm_trace(i)}
            if tmp_path is not None:
                path = str(tmp_path / (n + ".xml"))
                eng.write_result_xml(i, path)
                rec["xml"] = open(path).read()
            out.append(rec)
        for i in range(len(names), len(names) + len(extra)):
            out.append({"state": eng.state(i), "vol": [eng.volume_trace(i, w) for w in range(3)], "cm": [eng.cm_trace(i, w) for w in range(3)]})
    return out


@pytest.fixture(scope="module")
def runs(eng_mod, golden_dir, tmp_path_factory):
    """the four fixtures as one batch, once per kernel path (shared by the tests below, never changed)"""
    tmp = tmp_path_factory.mktemp("normvol")
    out = {}
    for path, options in PATHS.items():
        sub = tmp / path
        sub.mkdir()
        out[path] = _run(eng_mod, golden_dir, NAMES, options, sub)
    return out


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("k", range(4), ids=NAMES)
def test_traces_and_norm_tags_are_the_reference_files(runs, golden_dir, path, k):
    """point counts and times of the life trace equal the file's; volumes and the three Norm tags within a unit of the sixth digit (plus the
    parity floor carried through the sum); the XML has the reference's structure, <VolumeTrace> included"""
    ref, got = _reference(golden_dir, NAMES[k]), runs[path][k]
    life_cm, life_vol = got["cm"][0], got["vol"][0]
    print("%s %s: %d life / %d after-life / %d frozen points" % (NAMES[k], path, len(life_cm), len(got["cm"][1]), len(got["cm"][2])))
    assert len(life_cm) == len(life_vol) == len(ref["time"]) == len(ref["vol"]) >= 30
    assert np.array_equal(life_cm[:, 0], life_vol[:, 0])
    printed = lambda values: np.array([float("%g" % v) for v in values])
    assert np.array_equal(printed(life_cm[:, 0]), ref["time"]) and np.array_equal(printed(life_vol[:, 0]), ref["vol_time"])
    print("  volume: largest relative difference %.3g" % np.abs(life_vol[:, 1] / ref["vol"] - 1).max())
    assert np.allclose(life_vol[:, 1], ref["vol"], rtol=RTOL, atol=0)
    assert np.ptp(life_vol[:, 1]) > 0.01 * life_vol[0, 1]                 # the robot really changes size
    # the other two traces exist exactly where their windows do
    # A window of length w holds w / TimeBetweenTraces points, give or take the one at either end (the first falls on the first step
    # inside, the rest at least 0.01 apart).  After-life: (0.4, 0.5 + a step], w = 0.1.  Frozen: DevelopmentFrozen holds for step starts in
    # (0.175, 0.225) (VX_Sim.cpp:1090-1104 with InitCmTime 0.05, MidLifeFreezeTime 0.1), w = 0.05.
    for w, window in ((1, ref["afterlife"]), (2, 0.05 if ref["freeze"] > 0 else 0.0)):
        if window > 0:
            assert round(window / 0.01) - 1 <= len(got["cm"][w]) <= round(window / 0.01) + 1, (w, len(got["cm"][w]))
        else:
            assert len(got["cm"][w]) == 0
    for w in (1, 2):
        assert len(got["cm"][w]) == len(got["vol"][w]) and np.array_equal(got["cm"][w][:, 0], got["vol"][w][:, 0])
        if len(got["cm"][w]):
            assert np.all(np.diff(got["cm"][w][:, 0]) >= 0.01 - 1e-12)   # its own cadence: TimeBetweenTraces apart
    if ref["afterlife"] > 0:
        assert got["cm"][1][0, 0] > 0.4                                    # CurTime > StopConditionValue
    if ref["freeze"] > 0:                                                  # the window of VX_Sim.cpp:1090-1104: (0.175 - 0.05 + 0.05, 0.175 + 0.05)
        assert 0.175 < got["cm"][2][0, 0] < 0.19 and got["cm"][2][-1, 0] < 0.225 + 1e-3

    def atol(vols):
        return 2 * FLOOR_VOX * len(vols) / vols.min() ** ref["exponent"] if len(vols) else 0.0
    r = got["result"]
    final_printed = r["norm_final_dist"] - r["norm_frozen_dist"]
    tol_final = atol(life_vol[:, 1]) + atol(got["vol"][2][:, 1])
    print("  NormFinalDist %.9g (file %.9g), NormRegimeDist %.9g (file %.9g), NormFrozenDist %.9g (file %.9g)"
          % (final_printed, ref["final"], r["norm_regime_dist"], ref["regime"], r["norm_frozen_dist"], ref["frozen"]))
    # the TAGS are compared: the engine's value as the result file prints it (%g) against the reference's printed one.  (The raw double
    # cannot be held to rtol 2e-6 of a six-digit print: the print alone is off by up to 4e-6 of a value whose digits start with 1.2.)
    as_tag = lambda v: float("%g" % v)
    assert np.isclose(as_tag(final_printed), ref["final"], rtol=RTOL, atol=tol_final)
    assert np.isclose(as_tag(r["norm_frozen_dist"]), ref["frozen"], rtol=RTOL, atol=atol(got["vol"][2][:, 1]))
    assert np.isclose(as_tag(r["norm_regime_dist"]), ref["regime"], rtol=RTOL, atol=atol(got["vol"][1][:, 1]) if ref["afterlife"] > 0 else FLOOR_VOX)
    # the result file: the printed tags, and the reference's structure tag for tag
    text = got["xml"]
    for tag, a in (("NormFinalDist", tol_final), ("NormFrozenDist", atol(got["vol"][2][:, 1])),
                   ("NormRegimeDist", atol(got["vol"][1][:, 1]) if ref["afterlife"] > 0 else FLOOR_VOX), ("Volume", 0.0)):
        assert np.allclose(_tags(text, tag), _tags(ref["text"], tag), rtol=RTOL, atol=a), tag
    assert np.array_equal(_tags(text, "Time"), _tags(ref["text"], "Time"))
    assert "<VolumeTrace>" in text and re.sub(r">[^<>\n]+<", "><", text) == re.sub(r">[^<>\n]+<", "><", ref["text"])


def test_every_kernel_path_records_the_same_points(runs):
    """counts and times bitwise equal across the four paths, for all three traces of all four robots"""
    for k in range(4):
        for w in range(3):
            base = runs["default"][k]["cm"][w][:, 0]
            for path in PATHS:
                assert np.array_equal(runs[path][k]["cm"][w][:, 0], base), (NAMES[k], w, path)
                assert np.array_equal(runs[path][k]["vol"][w][:, 0], base), (NAMES[k], w, path)


def test_get_cm_trace_is_trace_zero(runs):
    for path in PATHS:
        got = runs[path][0]
        assert got["cm_plain"].shape[0] >= 30 and np.array_equal(got["cm_plain"], got["cm"][0])


def test_a_robot_without_the_option_is_untouched_by_one_with_it(eng_mod, golden_dir):
    """normvol_a + phase4 in one batch: phase4 ends bitwise where it ends in a batch of its own, and has no volume or extra traces"""
    for options in PATHS.values():
        alone = _run(eng_mod, golden_dir, [], options, extra=["phase4"])[0]
        mixed = _run(eng_mod, golden_dir, ["normvol_a"], options, extra=["phase4"])[1]
        assert np.array_equal(alone["state"], mixed["state"])
        for w in range(3):
            assert mixed["vol"][w].shape == (0, 2)
        assert mixed["cm"][1].shape == (0, 4) and mixed["cm"][2].shape == (0, 4)


def test_a_handle_over_two_engines_returns_the_same_traces(eng_mod, golden_dir, runs):
    with eng_mod.Engine(eng_mod.VOXCAD, (0, 0)) as two:
        for key, value in PATHS["default"].items():           # (the same kernel as the run it is compared with, bit for bit)
            two.set_option(key, value)
        two.set_option("steps_per_launch", 100)
        for n in NAMES:
            two.add_vxa_file(os.path.join(golden_dir, "vxa", n + ".vxa"))
        two.run()
        for k in range(4):
            for w in range(3):
                assert np.array_equal(two.cm_trace(k, w), runs["default"][k]["cm"][w]), (NAMES[k], w)
                assert np.array_equal(two.volume_trace(k, w), runs["default"][k]["vol"][w]), (NAMES[k], w)
            assert two.result(k).as_dict() == runs["default"][k]["result"]


def test_evaluate_all_returns_the_reference_fitness(eng_mod, golden_dir, tmp_path):
    """add_param("norm_dist_by_vol", 1, "<NormDistByVol>") through evaluate_all with <NormFinalDist> as the objective: the fitness of the four
    robots is what the reference binary printed, within a unit of the sixth digit plus the floor of the sum"""
    from evosoro_amd.base import ObjectiveDict
    from evosoro_amd.tools.evaluation import evaluate_all
    spec = importlib.util.spec_from_file_location("make_normvol_golden", os.path.join(golden_dir, "make_normvol_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)

    class Log(object):
        def message(self, text):
            pass

    class Pop(list):
        pass

    for name in NAMES:
        sim, env, ind = gen.inputs(gen.CASES[name])
        run = str(tmp_path / name)
        for d in ("voxelyzeFiles", "fitnessFiles", "tempFiles", "bestSoFar/fitOnly", "ancestors", "Gen_0000"):
            os.makedirs(os.path.join(run, d))
        pop = Pop([ind])
        pop.objective_dict = ObjectiveDict()
        pop.objective_dict.add_objective(name="fitness", maximize=True, tag="<NormFinalDist>")
        pop.objective_dict.add_objective(name="age", maximize=False, tag=None)
        pop.gen, pop.pop_size, pop.total_evaluations, pop.best_fit_so_far = 0, 1, 0, -1e9
        pop.already_evaluated, pop.all_evaluated_individuals_ids = {}, []
        ind.fitness, ind.age = -10e6, 0
        evaluate_all(sim, env, pop, Log(), save_vxa_every=0, run_directory=run, run_name="N")
        ref = _reference(golden_dir, name)
        n, vmin = len(ref["vol"]) + (10 if ref["freeze"] > 0 else 0), ref["vol"].min() * (1 - RTOL)
        print("%s: fitness %.9g, file %.9g" % (name, ind.fitness, ref["final"]))
        assert np.isclose(ind.fitness, ref["final"], rtol=RTOL, atol=2 * FLOOR_VOX * n / vmin ** ref["exponent"])
