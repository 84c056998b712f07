"""Engine option device_curvature: the per-vertex angle excesses of land_water robots from k_shape_curvature (kernels_curvature.hpp) instead
of from the downloaded voxel state.  Reference: an engine WITHOUT device_shape / device_shape_large / device_curvature stepped alike in the
same process -- the host path, mesh_angle_excess, the reference's arithmetic in FP64.

Tolerance for a vertex of m corners: m * ((K + 1) * 2^-51 + 2^-49).  2^-51 is one ulp of an angle in [2, 4) (no angle is larger); the
device's vertices and its order of summation are the host's, so a term differs only by acos: one ulp for glibc's plus K for the device
library's, K = 4, the OpenCL full-profile bound that library is built to (the ROCm installation states no figure of its own); 2^-49 covers
the roundings of the partial sums, which now see different terms.  NaNs (a dot product an ulp above 1) must sit in the same places."""
import functools
import os
import re
import tempfile

import numpy as np
import pytest

from evosoro_amd import engine
from test_gpu_shape_results import _synthetic

pytestmark = pytest.mark.gpu

K = 4
LDS_MAX_VERT = 6784          # VXH_CURV_LDS_MAX_VERT (device_types.hpp): (163840 - 1024) / 24
PLATE = 58                   # the smallest k x k x 1 plate with 2 (k + 1)^2 = 6962 > LDS_MAX_VERT vertices: the HBM-point instance
SHAPES = {"cube14": np.ones((14, 14, 14), dtype=np.int64), "plate58": np.ones((PLATE, PLATE, 1), dtype=np.int64)}
ON, OFF = 1, 0


def _engine(options):
    eng = engine.Engine(engine.VOXCAD_LAND_WATER, 0)
    for key in ("device_shape", "device_shape_large", "device_curvature"):
        eng.set_option(key, options)
    return eng


def _vectors(eng, with_corners):
    """per robot (rest vector, final vector, corners per vertex or None)"""
    out = []
    for i in range(eng.num_robots()):
        start, end = eng.angle_excess(i, False), eng.angle_excess(i, True)
        out.append((start, end, np.bincount(eng.mesh(i, True)[1].ravel(), minlength=len(end)) if with_corners else None))
    return out


@functools.lru_cache(maxsize=None)
def _batch(golden_dir, kernel_path, options, with_swim6, names):
    """lw_swim6 (if asked for) and the named shapes in one engine, 200 steps"""
    with open(os.path.join(golden_dir, "vxa", "lw_swim6.vxa")) as handle:
        text = handle.read()
    with _engine(options) as eng:
        if with_swim6:
            eng.add_vxa_text(text)
        eng.add_robots(text, [_synthetic(SHAPES[name]) for name in names])
        eng.step(200)
        return _vectors(eng, options == OFF)


@functools.lru_cache(maxsize=None)
def _swim6(golden_dir, kernel_path, options):
    """lw_swim6 alone, run to completion: its vectors, the result file and the curvatures file it leaves, its final shape descriptors"""
    tmp = tempfile.mkdtemp()
    curv = os.path.join(tmp, "curvatures.txt")
    text = open(os.path.join(golden_dir, "vxa", "lw_swim6.vxa")).read()
    text = re.sub(r"<CurvaturesTmpFile>.*?</CurvaturesTmpFile>", "<CurvaturesTmpFile>%s</CurvaturesTmpFile>" % curv, text)
    with _engine(options) as eng:
        eng.add_vxa_text(text)
        eng.run()
        eng.write_result_xml(0, os.path.join(tmp, "out.xml"))
        return _vectors(eng, options == OFF)[0], open(os.path.join(tmp, "out.xml")).read(), open(curv).read(), eng.shape_descriptors(0, True)


@pytest.mark.parametrize("name", ["lw_swim6", "cube14", "plate58"])
def test_device_angle_excess_against_the_host(golden_dir, kernel_path, name):
    if name == "lw_swim6":
        on, off = _swim6(golden_dir, kernel_path, ON)[0], _swim6(golden_dir, kernel_path, OFF)[0]
    else:
        index = 1 + list(SHAPES).index(name)
        on, off = _batch(golden_dir, kernel_path, ON, True, tuple(SHAPES))[index], _batch(golden_dir, kernel_path, OFF, True, tuple(SHAPES))[index]
    corners = off[2]
    assert (len(corners) > LDS_MAX_VERT) == (name == "plate58")
    bound = corners * ((K + 1) * 2.0 ** -51 + 2.0 ** -49)
    for when, got, want in (("start", on[0], off[0]), ("end", on[1], off[1])):
        assert got.shape == want.shape == corners.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, when)
        diff = np.nan_to_num(np.abs(got - want))
        print(name, when, "vertices", len(want), "NaNs", int(np.isnan(want).sum()), "largest difference %.3g x 2^-51" % (diff.max() * 2.0 ** 51),
              "largest share of the bound %.3g" % (diff / bound).max())
        assert (diff <= bound).all(), (name, when, int(np.argmax(diff / bound)), diff.max())
    assert np.nanmax(np.abs(off[1] - off[0])) > 1e-3          # (the mesh did deform)


def test_lw_swim6_against_the_reference_files(golden_dir, kernel_path):
    (start, end, _), xml, written, descriptors = _swim6(golden_dir, kernel_path, ON)
    want_end = np.array([float(t) for t in open(os.path.join(golden_dir, "expected", "lw_swim6.curv_end.txt")).read().split()])
    assert end.shape == want_end.shape
    assert np.allclose(end, want_end, rtol=6e-6, atol=2e-7), np.abs(end - want_end).max()
    assert written.endswith("\t") and written.split() == ["%g" % v for v in end]
    ref_xml = open(os.path.join(golden_dir, "expected", "lw_swim6.xml")).read()
    got_text, ref_text = [{tag: re.search(r"<%s>(.*?)</%s>" % (tag, tag), x).group(1) for tag in ("ShapeComplexityStart", "ShapeComplexityEnd")} for x in (xml, ref_xml)]
    assert got_text["ShapeComplexityStart"] == ref_text["ShapeComplexityStart"] == "%g" % start[0]
    ref_end = float(ref_text["ShapeComplexityEnd"])
    sixth_digit = 10.0 ** (np.floor(np.log10(abs(ref_end))) - 5)
    assert abs(float(got_text["ShapeComplexityEnd"]) - ref_end) <= sixth_digit * (1 + 1e-9), (got_text, ref_text)
    # vxh_get_shape_descriptors: the complexity from the device vector, the volumes those of the result file
    assert descriptors[2] == float(got_text["ShapeComplexityEnd"]) == float("%g" % end[0])
    assert ["%g" % v for v in descriptors[:2]] == [re.search(r"<%s>(.*?)</%s>" % (tag, tag), xml).group(1) for tag in ("RobotVolumeEnd", "ConvexHullVolumeEnd")]


def test_a_function_of_the_robot_alone(golden_dir, kernel_path):
    together = _batch(golden_dir, kernel_path, ON, True, tuple(SHAPES))[1]
    alone = _batch(golden_dir, kernel_path, ON, False, ("cube14",))[0]
    for k in range(2):
        assert np.array_equal(alone[k].view(np.int64), together[k].view(np.int64))
