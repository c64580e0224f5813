"""The rotation-consistency check of the host replays (csrc/orbm_search.cpp: RotHist - rot_bin, three_maxima, prune - and what each entry point does with a reset match) on
histograms built bin by bin - survivors of the mutation pass recorded in profiles/emu_mutants_host/README.md.  The device twins of these lines (csrc/k_search.hip: rot_bin,
three_maxima) got their tests from the first pass (tests/test_lastframe_gates.py, test_branch_edges_rotation.py); the host form decides every non-batched call.

A match per lattice spot (tests/replay_scenes.py): one keypoint and one point with the same descriptor, whose two angles are chosen - so every histogram entry is known, and
which matches the check resets follows from the bin counts written in SCENES: (angle of the first view, angle of the second, matches, bin, kept).
  rot_bin       src/ORBmatcher.cc:2118-2123  `rot = a1 - a2; if (rot < 0.0) rot += 360; bin = round(rot * factor)` with the reference's factor 1 / HISTO_LENGTH = 1 / 30:
                rot == 0 stays in bin 0, a rot just below 0 goes to bin 12 (359.5 / 30), the largest bin there is; 15 degrees is bin 1 (0.5f rounds away from zero), 14 is bin 0
  three_maxima  :2335-2377  strict `>` three times: of equal bins the first keeps its rank; a new first or second pushes the others down; the `< 0.1f * max1` cuts keep a bin of
                exactly a tenth (max1 = 10 and 20: 0.1f * 10 is 1.0f, 0.1f * 20 is 2.0f in float) and drop one entry fewer
  the resets    SearchByProjection(Frame, LastFrame / KeyFrame) and its rig form write -2 and count down; SearchForInitialization counts a match down once, not again when
                the rotation check meets a match that was displaced before; the resident BoW search (prune_by_rotation) takes a1 from key frame 1
Expected: written down per scene, and equal to the oracle's function for the entry (tests/oracle_lib.py)."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, views
from orb_slam3_detailed_comments_amd import matcher as M
from replay_scenes import Keys, f32, flip, same, spots

B = (60.0, 120.0, 180.0, 240.0)                                             # four rotations in the bins 2, 4, 6 and 8
SCENES = {
    # rot_bin
    "rot_is_0":        ((90.0, 0.0, 6, 3, True), (180.0, 0.0, 5, 6, True), (10.0, 10.0, 4, 0, True), (355.0, 0.0, 3, 12, False)),
    "rot_just_below_0": ((90.0, 0.0, 6, 3, True), (180.0, 0.0, 5, 6, True), (10.0, 10.5, 4, 12, True), (5.0, 0.0, 3, 0, False)),
    "rot_15_and_14":   ((90.0, 0.0, 7, 3, True), (180.0, 0.0, 6, 6, True), (15.0, 0.0, 5, 1, True), (14.0, 0.0, 4, 0, False)),
    # three_maxima: the tie order of each `>` and the push-downs
    "tie_5_5_5_5":     ((B[0], 0.0, 5, 2, True), (B[1], 0.0, 5, 4, True), (B[2], 0.0, 5, 6, True), (B[3], 0.0, 5, 8, False)),
    "tie_6_5_5_5":     ((B[0], 0.0, 6, 2, True), (B[1], 0.0, 5, 4, True), (B[2], 0.0, 5, 6, True), (B[3], 0.0, 5, 8, False)),
    "tie_7_6_5_5":     ((B[0], 0.0, 7, 2, True), (B[1], 0.0, 6, 4, True), (B[2], 0.0, 5, 6, True), (B[3], 0.0, 5, 8, False)),
    "rising_3_4_5_6":  ((B[0], 0.0, 3, 2, False), (B[1], 0.0, 4, 4, True), (B[2], 0.0, 5, 6, True), (B[3], 0.0, 6, 8, True)),
    "second_late_6_4_5_3": ((B[0], 0.0, 6, 2, True), (B[1], 0.0, 4, 4, True), (B[2], 0.0, 5, 6, True), (B[3], 0.0, 3, 8, False)),
    # the two cuts at a tenth of the strongest bin
    "tenth_10_1_1":    ((B[0], 0.0, 10, 2, True), (B[1], 0.0, 1, 4, True), (B[2], 0.0, 1, 6, True)),
    "tenth_20_2_1":    ((B[0], 0.0, 20, 2, True), (B[1], 0.0, 2, 4, True), (B[2], 0.0, 1, 6, False)),
    "tenth_20_1_1":    ((B[0], 0.0, 20, 2, True), (B[1], 0.0, 1, 4, False), (B[2], 0.0, 1, 6, False)),
    "tenth_20_2_2":    ((B[0], 0.0, 20, 2, True), (B[1], 0.0, 2, 4, True), (B[2], 0.0, 2, 6, True)),
}


def _written_bins():
    """the bins written in SCENES are the reference's formula in float arithmetic"""
    factor = f32(1.0) / f32(30)
    for name, groups in SCENES.items():
        for a1, a2, count, b, kept in groups:
            rot = f32(a1) - f32(a2)
            if rot < 0:
                rot = f32(rot + f32(360))
            x = float(f32(rot * factor))
            assert int(np.floor(x + 0.5)) == b, (name, a1, a2, x, b)              # (round half away from zero; x >= 0)
    assert float(f32(15) * factor) == 0.5 and float(f32(0.1) * f32(10)) == 1.0 and float(f32(0.1) * f32(20)) == 2.0


_DONE = {}


def _pairs(name):
    """one match per spot: (x, y, descriptor, angle 1, angle 2, kept) in the order of SCENES[name]"""
    if name not in _DONE:
        rng = np.random.default_rng(sum(map(ord, name)))
        sp, out = spots(), []
        for a1, a2, count, b, kept in SCENES[name]:
            for _ in range(count):
                x, y = next(sp)
                out.append((x, y, rng.integers(0, 256, 32, dtype=np.uint8), a1, a2, kept))
        _DONE[name] = out
    return _DONE[name]


def _frame_form(name):
    """a current frame (angle 2) and the last frame's / key frame's points (angle 1); expected: the match index, -2 where the check resets"""
    pairs = _pairs(name)
    K = Keys()
    for x, y, D, a1, a2, kept in pairs:
        K.add(x, y, 0, D, angle=a2)
    n = len(pairs)
    x, y, D, a1 = [np.array([p[i] for p in pairs]) for i in range(4)]
    last = views.last_frame_view(np.ones(n, np.uint8), x, y, np.ones(n, f32), np.zeros(n, np.int32), a1, np.ones(n, np.uint8), D)
    proj = views.projected_point_view(np.ones(n, np.uint8), x, y, np.zeros(n, np.int32), D, ur=x, angle=a1)
    exp = np.array([i if p[5] else -2 for i, p in enumerate(pairs)], np.int32)
    return K, last, proj, exp, int((exp >= 0).sum())


def _check_frame_forms(lib):
    _written_bins()
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    try:
        m = M.ORBmatcher(0.9, True)
        for name in SCENES:
            K, last, proj, exp, exp_n = _frame_form(name)
            fv = K.frame_view(occupied=False)
            n, a = ol.oracle_search_by_projection_frame(fv, last, 3.0, False, False, True)
            same(n, a, exp_n, exp, "%s: the oracle's SearchByProjection(Frame, LastFrame) against the written bins" % name)
            n, a = m.SearchByProjectionFrame(ex, fv, last, 3.0)
            same(n, a, exp_n, exp, "%s: SearchByProjection(Frame, LastFrame)" % name)
        # the other entries that write -2: one histogram each
        name = "rot_is_0"
        K, last, proj, exp, exp_n = _frame_form(name)
        fv = K.frame_view(occupied=False)
        n, a = ol.oracle_search_by_projection_keyframe(fv, proj, 3.0, 100, True)
        same(n, a, exp_n, exp, "%s: the oracle's SearchByProjection(Frame, KeyFrame) against the written bins" % name)
        n, a = m.SearchByProjectionKeyFrame(ex, fv, proj, 3.0, 100)
        same(n, a, exp_n, exp, "%s: SearchByProjection(Frame, KeyFrame)" % name)
        # the rig form: the same matches in both cameras (every bin twice as full: the same bins are kept), camera 2's slots behind Nleft
        f2 = views.fisheye_frame_view(fv, K.frame_view(occupied=False))
        x, y = [np.array([p[i] for p in _pairs(name)], f32) for i in range(2)]
        e2 = np.concatenate([exp, exp]); n2 = 2 * exp_n
        n, a = ol.oracle_search_by_projection_frame_fisheye(f2, last, x, y, 3.0, False, False, True)
        same(n, a, n2, e2, "%s: the oracle's SearchByProjection(rig Frame, LastFrame) against the written bins" % name)
        n, a = m.SearchByProjectionFrameFisheye(ex, f2, last, x, y, 3.0)
        same(n, a, n2, e2, "%s: SearchByProjection(rig Frame, LastFrame)" % name)
    finally:
        ex.close()


def test_rotation_histogram_of_the_frame_searches_emulated(emu_lib):
    _check_frame_forms(emu_lib)


@pytest.mark.gpu
def test_rotation_histogram_of_the_frame_searches_gpu(hip_lib):
    _check_frame_forms(hip_lib)


def _init_form():
    """SearchForInitialization on the histogram "rot_is_0" plus one spot where frame 1's keypoint A matches the frame-2 keypoint at 20 bits with a rotation of 270 (alone in
    bin 9) and B, right after it, takes the keypoint over at 10 bits with a rotation of 90.  A has been counted down when it was displaced (:817-821); the rotation check finds
    its index in the weak bin 9 and must not count it down again (:853 `if (vnMatches12[idx1] >= 0)`)."""
    pairs = _pairs("rot_is_0")
    K1, K2 = Keys(), Keys()
    for x, y, D, a1, a2, kept in pairs:
        K1.add(x, y, 0, D, angle=a1); K2.add(x, y, 0, D, angle=a2)
    exp = [i if p[5] else -1 for i, p in enumerate(pairs)]
    x, y = 24.0 + 24 * 13, 24.0 + 24 * 8                                     # the lattice's last spot: the histogram's matches fill it from the first
    A = np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8); Kd = flip(A, 0, 20); Bd = flip(Kd, 100, 110)
    K1.add(x, y, 0, A, angle=270.0); K1.add(x, y, 0, Bd, angle=90.0); k = K2.add(x + 1, y, 0, Kd, angle=0.0)
    exp += [-1, k]
    exp = np.array(exp, np.int32)
    k1, _ = K1.arrays()
    return K1, K2, np.stack([k1["x"], k1["y"]], 1).astype(f32), exp, int((exp >= 0).sum())


def _check_init_form(lib):
    K1, K2, prev, exp, exp_n = _init_form()
    f1, f2 = K1.frame_view(occupied=False), K2.frame_view(occupied=False)
    n, a = ol.oracle_search_for_initialization(f1, f2, prev.copy(), 4, 0.9, True)
    same(n, a, exp_n, exp, "the oracle's SearchForInitialization against the written bins")
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    try:
        n, a = M.ORBmatcher(0.9, True).SearchForInitialization(ex, f1, f2, prev.copy(), 4)
        same(n, a, exp_n, exp, "SearchForInitialization with the rotation check")
    finally:
        ex.close()


def test_rotation_check_meets_a_displaced_match_emulated(emu_lib):
    _check_init_form(emu_lib)


@pytest.mark.gpu
def test_rotation_check_meets_a_displaced_match_gpu(hip_lib):
    _check_init_form(hip_lib)


def _check_bow_forms(lib):
    """SearchByBoW on "rot_is_0", one vocabulary node per match: the host replay (orbm_search_by_bow) and the resident form (prune_by_rotation), whose a1 must be key frame 1's
    angle - taken the other way round, 90 becomes bin 9, 355 becomes bin 0 beside the four matches with rot == 0, and nothing is reset"""
    pairs = _pairs("rot_is_0")
    K1, K2 = Keys(), Keys()
    for x, y, D, a1, a2, kept in pairs:
        K1.add(x, y, 0, D, angle=a1); K2.add(x, y, 0, D, angle=a2)
    nodes = np.arange(len(pairs))
    exp = np.array([i if p[5] else -1 for i, p in enumerate(pairs)], np.int32)
    exp_n = int((exp >= 0).sum())
    ones = np.ones(len(pairs), np.uint8)
    kv1, kv2 = K1.key_frame_view(nodes, ones), K2.key_frame_view(nodes, ones)
    n, a = ol.oracle_search_by_bow(kv1, kv2, 0.9, True, True)
    same(n, a, exp_n, exp, "the oracle's SearchByBoW against the written bins")
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    try:
        m = M.ORBmatcher(0.9, True)
        n, a = m.SearchByBoW(ex, kv1, kv2, True)
        same(n, a, exp_n, exp, "SearchByBoW with the rotation check")
        r1, r2 = M.ResidentKeyFrame(ex, kv1), M.ResidentKeyFrame(ex, kv2)
        try:
            (n, a), = m.SearchByBoWResident(ex, [r1], [ones], [r2], [None], True)
            same(n, a, exp_n, exp, "SearchByBoW over resident key frames with the rotation check")
        finally:
            r1.close(); r2.close()
    finally:
        ex.close()


def test_rotation_histogram_of_the_bow_searches_emulated(emu_lib):
    _check_bow_forms(emu_lib)


@pytest.mark.gpu
def test_rotation_histogram_of_the_bow_searches_gpu(hip_lib):
    _check_bow_forms(hip_lib)
