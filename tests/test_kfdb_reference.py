"""The database's restatement pinned on the reference: oracle/_ref/libkfdb_ref.so is the reference's own src/KeyFrameDatabase.cc + include/KeyFrameDatabase.h,
compiled unmodified and in place over its own KeyFrame class (oracle/Makefile, oracle/ref_kfdb_driver.cpp; -DORBX_REFERENCE_KFDB lets them take the place of the
stand-in of slam_shim/full_world.h).  tests/cpp/kfdb_gates_test.cpp mirrors every operation to it: on the eleven constructed scenarios the facade, RestatedDB and
the reference must all give the written candidate lists and equal query fields; on two seeds of the random twin worlds of kfdb_facade_test.cpp (60 key frames:
repeat query ids, a duplicate add, erasures, a key frame that changes maps, clearMap) the three must agree.  Scenarios with a bad key frame in the candidate loop
of DetectNBestCandidates are left out: the reference does not advance there and spins.  CPU only: the reference does not exist beside a device."""
import os
import re

import pytest

import oracle_lib as ol
from test_kfdb_facade import REF, vocabulary
from test_kfdb_gates import build_driver, run

LIB = os.path.join(REF, "libkfdb_ref.so")


@pytest.mark.skipif(not os.path.exists(LIB), reason="oracle/_ref/libkfdb_ref.so not built (needs the reference)")
def test_restatement_reference_and_facade_agree(emu_lib, tmp_path):
    out = run(build_driver(tmp_path, *ol.emu_link()), vocabulary(tmp_path, 0), LIB, 1, 2)
    calls = int(re.search(r"reference_calls=(\d+)", out).group(1))
    assert calls == 100, out            # 16 queries of the constructed scenarios + 42 of each random world, every one answered by the reference too
