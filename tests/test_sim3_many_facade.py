"""The many-key-frame forms of the facade's Sim3 projection search - SearchByProjection(vpKFs, vScw, vpPoints, vvpMatched, th, ratioHamming) and the overload with
vpPointsKFs / vvpMatchedKF of include/orb_slam3_amd/ORBmatcher.h - against the single-key-frame forms called once per key frame: tests/cpp/sim3_many_test.cpp
builds two identical mock worlds (4 key frames, one set of 200 points with several points per feature, bad points, descriptors at the edge of the threshold,
keypoints that hold a point on entry; one key frame marked as a rig), runs the loop on one and the single call on the other, and requires identical return
values, vpMatched and vpMatchedKF.  The same program compiled with the map point's mfMinDistance / mfMaxDistance hidden runs the single calls throughout (the
fallback): both builds must print the same results."""
import os
import subprocess

import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import _lib

ROOT = ol.ROOT


def _build(tmp_path, libdir, libname, hidden):
    exe = tmp_path / ("sim3_many_test_hidden" if hidden else "sim3_many_test")
    subprocess.run(["g++", "-std=c++14", "-O1", "-w"] + (["-DHIDE_DISTANCE_LIMITS"] if hidden else []) +
                   ["-I" + ol.facade_include(), "-I" + os.path.join(ROOT, "oracle", "opencv_shim"),
                    os.path.join(ROOT, "tests", "cpp", "sim3_many_test.cpp"), "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-lpthread", "-o", str(exe)], check=True)
    return exe


def _run(tmp_path, libdir, libname):
    batched, fallback = _build(tmp_path, libdir, libname, False), _build(tmp_path, libdir, libname, True)
    for form in ("plain", "kfs"):
        out = []
        for exe in (batched, fallback):
            r = subprocess.run([str(exe), form], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "identical 1" in r.stdout, form + ": " + r.stdout[:2000] + r.stderr
            out.append(r.stdout)
        assert out[0] == out[1], form + ": the batched call and the single-call fallback differ"
        assert out[0].count("\nkf ") == 4 and out[0].count("count ") == 4


def test_sim3_many_equals_the_loop_emulated(tmp_path, emu_lib):
    _run(tmp_path, *ol.emu_link())


@pytest.mark.gpu
def test_sim3_many_equals_the_loop_gpu(tmp_path, hip_lib):
    _run(tmp_path, os.path.dirname(_lib.HIP_LIB_PATH), "orbx_hip")
