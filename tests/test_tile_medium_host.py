"""The MEDIUM size class of the tiled kernel (engine option tile_medium) in the launch plan, on the host: `batch_check --medium`
(evosoro_amd/csrc/batch_check.cpp check_medium), built with the plain C++ compiler under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch_check(tmp_path_factory):
    out = tmp_path_factory.mktemp("batch_check_san")
    subprocess.check_call(["make", "-C", os.path.join(REPO, "evosoro_amd", "csrc"), "batch_check", "CHECK_OUT=%s" % out, "SAN=-fsanitize=address,undefined"], stdout=subprocess.DEVNULL)
    return str(out / "batch_check")


@pytest.mark.parametrize("population", ["four 20^3 lattices", "10x10x5 block in four tiles"])
def test_tiles_of_125_voxels_plan_into_the_medium_class(batch_check, population, tmp_path):
    from evosoro_amd import workloads
    from evosoro_amd.base import Sim, Env
    from evosoro_amd.tools.read_write_voxelyze import write_voxelyze_file
    paths, tiles = [os.path.join(REPO, "tests", "golden", "vxa", "cfg4_full20.vxa")] * 4, 0      # 4 x 125 wavefront tiles exceed 256 CUs: 64 tiles of 5x5x5 each
    if population != "four 20^3 lattices":
        os.makedirs(tmp_path / "voxelyzeFiles")
        write_voxelyze_file(Sim(dt_frac=0.9), Env(), workloads.make_individual(0, workloads.full_material(10, 1)[:, :, :5]), str(tmp_path), "m")
        paths, tiles = [str(tmp_path / "voxelyzeFiles" / "m--id_00000.vxa")], 4
    run = subprocess.run([batch_check, "--medium", "0", "256", str(tiles), "0"] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(paths) and all("own 125-125" in l and ": MEDIUM, " in l and l.endswith(": ok") for l in lines), run.stdout
