"""The drop-in KeyFrameDatabase.h (include/orb_slam3_amd) against a host restatement of the reference's KeyFrameDatabase on twin worlds of
mock key frames (tests/cpp/kfdb_facade_test.cpp): candidate vectors and every key frame's query fields after every call, over sequences
of relocalisation and loop / merge queries with repeat query ids, stale scores, erasures, a clearMap after a key frame changed maps and
bad key frames.  Scores of the restatement come from the reference's own DBoW2 (oracle/_ref/libref_dbow2.so)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import vocab_scenes as vs
from orb_slam3_detailed_comments_amd import _lib

ROOT = ol.ROOT
REF = os.path.join(ROOT, "oracle", "_ref")


def build_driver(tmp_path, libdir, libname):
    if ol.reference_dbow2() is None:
        pytest.skip("oracle/_ref/libref_dbow2.so not built")
    exe = tmp_path / "kfdb_facade_test"
    subprocess.run(["g++", "-std=c++14", "-O1", "-w", "-I" + ol.facade_include(), "-I" + os.path.join(ROOT, "oracle", "opencv_shim"),
                    os.path.join(ROOT, "tests", "cpp", "kfdb_facade_test.cpp"), "-L" + libdir, "-l" + libname, os.path.join(REF, "libref_dbow2.so"),
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + REF, "-lpthread", "-o", str(exe)], check=True)
    return exe


def vocabulary(tmp_path, scoring, seed=4):
    rng = np.random.default_rng(seed)
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 8, 3, scoring, 0)
    path = tmp_path / ("voc_%d.txt" % scoring)
    vs.write_text(path, header, parent, leaf, desc, weight)
    return path


def run(exe, path, seed):
    r = subprocess.run([str(exe), str(path), str(seed)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout + r.stderr
    assert "nonempty=0" not in r.stdout


@pytest.mark.parametrize("scoring,seed", [(0, 1), (1, 2), (2, 3), (4, 5)])
def test_kfdb_facade_emulated(emu_lib, tmp_path, scoring, seed):
    exe = build_driver(tmp_path, *ol.emu_link())
    run(exe, vocabulary(tmp_path, scoring), seed)


@pytest.mark.gpu
def test_kfdb_facade_gpu(hip_lib, tmp_path):
    exe = build_driver(tmp_path, os.path.dirname(_lib.HIP_LIB_PATH), "orbx_hip")
    for scoring, seed in ((0, 1), (2, 3)):
        run(exe, vocabulary(tmp_path, scoring), seed)
