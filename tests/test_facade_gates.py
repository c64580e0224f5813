"""Decisions of the drop-in ORBmatcher.h that the reference has no counterpart for, on mock types (tests/cpp/facade_gates_test.cpp, compiled from include/ and the
product library alone): the resident key-frame cache - each field of its tag, the uncached entry of a key frame without BoW, the change of device, Trim at the
capacities 1, 8, 9 and 16, the implicit cache's capacity - read off the device objects and the library's count of live allocations; and Fuse over several key
frames when one-camera key frames are mixed with a two-camera rig and a point stands twice in the set: a hand-built world of five key frames of eight key points
and ten set entries (`small`), in which every key frame's held points and every count are written at the check and required of the loop of the reference's call
site and of the one call; the same world through the Sim3 Fuse over many key frames with LoopClosing's hook (`smallsim3`: held points, counts and every
vpReplacePoint written) and through the Sim3 projection search over many key frames (`smallproj`: every vvpMatched / vvpMatchedKF written, two key points holding a
set point on entry); then, more broadly, the one call against the loop on the random world of fuse_many_test.cpp (`rig`, `rigsim3`, `sim3proj`).  These are the survivors of the facade block of tools/emu_mutants.py (profiles/emu_mutants_facade)."""
import os
import subprocess

import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import _lib

ROOT = ol.ROOT


def build_driver(tmp_path, libdir, libname):
    exe = tmp_path / "facade_gates_test"
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-I" + ol.facade_include(), "-I" + os.path.join(ROOT, "oracle", "opencv_shim"),
                    os.path.join(ROOT, "tests", "cpp", "facade_gates_test.cpp"), "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-lpthread", "-o", str(exe)], check=True)
    return exe


def run(exe, env=None):
    for what in ("cache", "small", "smallsim3", "smallproj", "rig", "rigsim3", "sim3proj"):
        r = subprocess.run([str(exe), what], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "GATES OK" in r.stdout, what + ":\n" + r.stdout + r.stderr


# (the cache's change of device needs two devices: the emulated form has two emulated ones; the device form skips that one check on a machine with one GPU visible)
def test_facade_gates_emulated(tmp_path, emu_lib):
    run(build_driver(tmp_path, *ol.emu_link()), dict(os.environ, ORBX_EMU_DEVICES="2"))       # two emulated devices: the cache's change of device


@pytest.mark.gpu
def test_facade_gates_gpu(tmp_path, hip_lib):
    run(build_driver(tmp_path, os.path.dirname(_lib.HIP_LIB_PATH), "orbx_hip"))
