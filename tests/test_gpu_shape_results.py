"""Engine option device_shape: the RobotVolume / ConvexHullVolume tags of land_water robots from k_shape_results (kernels_shape.hpp) instead
of from the downloaded voxel state.  References, both from an engine WITHOUT the option stepped alike: the hull by the host routine
engine.convex_hull_volume over the vertices of vxh_get_mesh rounded with float("%g" % x); the robot volume as math.fsum of the signed
tetrahedra over that mesh.  Tolerances: the device builds the host's face set, so the hull differs by the order of a sum of <= 2 nmv
positive terms (relative 1e-11; beyond that the face sets differ); the robot volume's terms cancel, so its bound scales with them,
64 * 2^-53 * sum |term|."""
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import pytest

from evosoro_amd import engine

pytestmark = pytest.mark.gpu

TAGS = ("robot_volume_start", "hull_volume_start", "robot_volume_end", "hull_volume_end")
FIXTURES = ["lw_swim6", "lw_quadruped_land", "lw_stiff5"]


def _block_missing_corner_and_centre():
    m = np.ones((3, 3, 3), dtype=np.int64)
    m[0, 0, 0] = m[1, 1, 1] = 0
    return m


# the smallest shapes at which the hull can go wrong; the plate has 2 * 23^2 = 1058 mesh vertices, just above VXH_SHAPE_MAX_VERT = 1024
SHAPES = OrderedDict([("voxel", np.ones((1, 1, 1), dtype=np.int64)), ("two", np.ones((2, 1, 1), dtype=np.int64)),
                      ("plate4", np.ones((4, 4, 1), dtype=np.int64)), ("block_holes", _block_missing_corner_and_centre()),
                      ("plate22", np.ones((22, 22, 1), dtype=np.int64))])


def _synthetic(material):
    """muscles 3 / 4 in a checkerboard (they actuate in antiphase) with a phase gradient: 200 steps leave the mesh in general position"""
    x, y, z = np.indices(material.shape)
    mat = np.where(material > 0, 3 + (x + y + z) % 2, 0)
    return mat, OrderedDict([("<PhaseOffset>", np.round(0.37 * x - 0.23 * y + 0.11 * z, 3))]), None


def _expected(eng, robot):
    """(robot volume, sum |term|, hull volume) of the rest state and of the current state of an engine without the option"""
    out = {}
    for when, at_end in (("start", False), ("end", True)):
        verts, facets = eng.mesh(robot, at_end)
        a, b, c = verts[facets[:, 0]], verts[facets[:, 1]], verts[facets[:, 2]]
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        terms = (1.0 / 6.0) * (cx * c[:, 0] + cy * c[:, 1] + cz * c[:, 2])
        rounded = np.array([float("%g" % v) for v in verts.ravel()]).reshape(-1, 3)
        out[when] = (math.fsum(terms), math.fsum(np.abs(terms)), engine.convex_hull_volume(rounded))
    return out


def _check(res, want, who):
    for when in ("start", "end"):
        vol, sum_abs, hull = want[when]
        got_vol, got_hull = getattr(res, "robot_volume_" + when), getattr(res, "hull_volume_" + when)
        print(who, when, "robot volume", got_vol, vol, abs(got_vol - vol), 64 * 2.0 ** -53 * sum_abs, "hull", got_hull, hull, abs(got_hull - hull) / hull)
        assert abs(got_vol - vol) <= 64 * 2.0 ** -53 * sum_abs, (who, when, got_vol, vol)
        assert hull > 0 and abs(got_hull - hull) <= 1e-11 * hull, (who, when, got_hull, hull)


def _run(golden_dir, device_shape, files, arrays, steps):
    with engine.Engine(engine.VOXCAD_LAND_WATER, 0) as eng:
        eng.set_option("device_shape", device_shape)
        for name in files:
            eng.add_vxa_file(os.path.join(golden_dir, "vxa", name + ".vxa"))
        if arrays:
            with open(os.path.join(golden_dir, "vxa", "lw_swim6.vxa")) as handle:
                eng.add_robots(handle.read(), arrays)
        eng.step(steps)
        n = eng.num_robots()
        return [eng.result(i) for i in range(n)], ([_expected(eng, i) for i in range(n)] if not device_shape else None)


@functools.lru_cache(maxsize=None)
def _batch(golden_dir, kernel_path):
    """lw_swim6 and the synthetic shapes in one engine, 200 steps: results with the option, results and references without"""
    arrays = [_synthetic(m) for m in SHAPES.values()]
    on, _ = _run(golden_dir, 1, ["lw_swim6"], arrays, 200)
    off, want = _run(golden_dir, 0, ["lw_swim6"], arrays, 200)
    return on, off, want


@pytest.mark.parametrize("name", FIXTURES)
def test_shipped_land_water_robots(golden_dir, name):
    on, _ = _run(golden_dir, 1, [name], [], 300)
    off, want = _run(golden_dir, 0, [name], [], 300)
    assert on[0].steps == off[0].steps > 0 and on[0].reserved == 0
    _check(on[0], want[0], name)


@pytest.mark.parametrize("index, name", list(enumerate(SHAPES, 1)))
def test_smallest_shapes(golden_dir, kernel_path, index, name):
    on, off, want = _batch(golden_dir, kernel_path)
    assert on[index].steps == off[index].steps == 200
    if name == "plate22":        # above the vertex cap: evaluated on the host, like without the option
        assert on[index].reserved == 1
        assert [getattr(on[index], t) for t in TAGS] == [getattr(off[index], t) for t in TAGS]
    else:
        assert on[index].reserved == 0
        _check(on[index], want[index], name)


def test_a_function_of_the_robot_alone(golden_dir, kernel_path):
    on, _, _ = _batch(golden_dir, kernel_path)
    alone, _ = _run(golden_dir, 1, ["lw_swim6"], [], 200)
    assert alone[0].reserved == 0
    assert [getattr(alone[0], t) for t in TAGS] == [getattr(on[0], t) for t in TAGS]
