"""MapPoint::SetBadFlag on a slot of the resident map that holds no point (csrc/k_search.hip: k_map_scatter without fields) - a survivor of the mutation pass recorded
in profiles/emu_mutants/README.md.  orbm_map_set_bad takes any slot of the store; `bad = 1` on an empty slot is covered by tests/test_local_map_build.py (the slot then
reads as bad either way), `bad = 0` is not: the flag alone must not turn an empty slot into a point.  Expected: Tracking::UpdateLocalPoints (src/Tracking.cc:4088-4120)
restated by hand for one key frame row - its matches in order, without the entries that hold no map point (`if (!pMP) continue`) and without the bad ones."""
import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor
from orb_slam3_detailed_comments_amd import matcher as M

f32 = np.float32


def _check(lib):
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    mp = M.ResidentMap(ex, 8, 1, 6, 1)
    try:
        rng = np.random.default_rng(3)
        ids = np.array([0, 1, 4], np.int32)
        pos = rng.normal(0, 1, (3, 3)).astype(f32)
        mp.update(ids, pos, pos, np.ones(3, f32), np.full(3, 5, f32), rng.integers(0, 256, (3, 32), dtype=np.uint8), np.array([0, 0, 1], np.uint8))
        # slot 2 was never updated, slot 4 is bad; the flag alone on both, and on slot 1 as the case that does change something
        mp.set_bad(np.array([2, 5], np.int32), np.array([0, 0], np.uint8))
        mp.set_keyframe(0, np.array([0, 2, -1, 1, 4, 5], np.int32))
        assert mp.local_points([[0]]).tolist() == [2], "slots 2 and 5 hold no point: SetBadFlag(false) must not create one"
        assert mp.fetch(0)[0].tolist() == [0, 1]
        mp.set_bad(np.array([4, 1], np.int32), np.array([0, 1], np.uint8))                # the bad point becomes good, a good one bad
        assert mp.local_points([[0]]).tolist() == [2] and mp.fetch(0)[0].tolist() == [0, 4]
    finally:
        mp.close(); ex.close()


def test_set_bad_on_an_empty_slot_emulated(emu_lib):
    _check(emu_lib)


@pytest.mark.gpu
def test_set_bad_on_an_empty_slot_gpu(hip_lib):
    _check(hip_lib)
