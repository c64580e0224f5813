"""The resident key-frame searches with their call-time flags read from the map (orbm_search_for_triangulation_resident_map / _kb8_map,
orbm_search_by_bow_resident_map, orbm_search_by_bow_rig_batch_map): every flag array of the host-fed call is named by its key frame's row in an
orbm_map, and one launch of k_map_row_flags fills all of them under one of two rules -
  holds a point       slot >= 0 and present, the bad flag NOT read (src/ORBmatcher.cc:1123-1127, :1159-1163: SearchForTriangulation tests the pointer)
  holds a good point  slot >= 0, present and not bad (`!pMP || pMP->isBad()`, :938-941, :959-965, :306-312: the SearchByBoW forms).

Rows mix the entry kinds NONE, GOOD, EMPTY, BAD of tests/test_map_rows_projection.py, each in every row.  Each call equals its host-fed form given
flags this file computes in numpy from its mirror of rows and states; the host-fed form given the OTHER rule's flags has to differ, or the test
could not tell the rules apart.  One triangulation case and one key-frame BoW case are anchored to the reference's own ORBmatcher.cc through
matcher_world.Driver, with map points that are bad where the row says BAD."""
import ctypes as C
import os

import numpy as np
import pytest

import matcher_world as mw
import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor
from orb_slam3_detailed_comments_amd import matcher as M
from test_map_rows_projection import NONE, GOOD, EMPTY, BAD, SLOTS, E_ARG, Store, _live
from test_resident_keyframes import make_kf, near

REF_MW = os.path.join(ol.ROOT, "oracle", "_ref", "libmw_ref.so")
needs_world = pytest.mark.skipif(not os.path.exists(REF_MW), reason="oracle/_ref/libmw_ref.so not built")
SIZES = (63, 64, 65, 257)                          # a wave less one, a wave, one more, a block of k_map_row_flags and one more
F_X = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32); EP_FAR = np.array([1e6, 240.0], np.float32)       # a pure x translation, the epipole far outside


def _kinds(rng, N):
    kinds = rng.choice([NONE, GOOD, EMPTY, BAD], N, p=[0.3, 0.4, 0.1, 0.2])
    kinds[rng.choice(N, 4, replace=False)] = [NONE, GOOD, EMPTY, BAD]            # each kind in every row
    return kinds


def _fill_row(store, rng, free, row, kinds):
    """a row of len(kinds) entries of the given kinds at fresh slots, uploaded; returns the row"""
    N = len(kinds)
    s = np.full(N, -1, np.int32)
    for i in np.flatnonzero(kinds != NONE):
        s[i] = free.pop()
    pts = np.flatnonzero((kinds == GOOD) | (kinds == BAD))
    store.update(s[pts], rng.normal(0, 1, (len(pts), 3)) + [0, 0, 4], np.full(len(pts), 0.5, np.float32), np.full(len(pts), 30.0, np.float32),
                 rng.integers(0, 256, (len(pts), 32), dtype=np.uint8), np.zeros(len(pts), np.uint8))
    bad = np.flatnonzero(kinds == BAD)
    store.set_bad(s[bad], np.ones(len(bad), np.uint8))
    store.set_keyframe(int(row), s)
    return s


def _flags(store, row, rule):
    """the rule on this file's copy of the map"""
    s = store.rows[int(row)]; z = np.where(s >= 0, s, 0)
    holds = (s >= 0) & store.present[z]
    return (holds if rule == "point" else holds & ~store.bad[z]).astype(np.uint8)


def _small_world(lib, rng):
    """key frames of SIZES features that see the same descriptors in the same vocabulary nodes (feature i of one matches feature i of another), resident,
    their rows in a map at permuted row numbers"""
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    base = rng.integers(0, 256, (max(SIZES), 32), dtype=np.uint8)
    views_ = [make_kf(rng, N, np.arange(N) % 5, near(base[:N], rng, 6)) for N in SIZES]
    kfs = [M.ResidentKeyFrame(ex, v) for v in views_]
    store = Store(ex, kf_rows=len(SIZES) + 3, kf_row_cap=max(SIZES) + 1)
    free = list(rng.permutation(SLOTS))
    rows = rng.permutation(len(SIZES) + 3)[:len(SIZES)].astype(np.int32)
    kinds = [_kinds(rng, N) for N in SIZES]
    for k, N in enumerate(SIZES):
        _fill_row(store, rng, free, rows[k], kinds[k])
        assert np.array_equal(_flags(store, rows[k], "point"), np.isin(kinds[k], (GOOD, BAD)).astype(np.uint8))
        assert np.array_equal(_flags(store, rows[k], "good"), (kinds[k] == GOOD).astype(np.uint8))
    return ex, kfs, store, rows


# ---- SearchForTriangulation: "holds a point" ---------------------------------------------------------------------------------------------------

def _triangulation(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(31)
    ex, kfs, store, rows = _small_world(lib, rng)
    point = [_flags(store, r, "point") for r in rows]; good = [_flags(store, r, "good") for r in rows]
    total, differ = 0, 0
    for k1, k2s in ((3, [0, 1, 2]), (1, [2]), (0, [3, 1, 2]), (2, [0])):             # n2 = 3 and 1, every size as K1
        n2 = len(k2s)
        Fs = np.stack([F_X] * n2); eps = np.stack([EP_FAR] * n2)
        for only_stereo, coarse, ori in ((0, 1, 0), (1, 1, 1), (0, 0, 1)):
            m = M.ORBmatcher(0.6, bool(ori))
            host = m.SearchForTriangulationResident(ex, kfs[k1], point[k1], [kfs[j] for j in k2s], [point[j] for j in k2s], Fs, eps, only_stereo, coarse)
            got = m.SearchForTriangulationResidentMap(ex, kfs[k1], rows[k1], [kfs[j] for j in k2s], rows[k2s], store.map, Fs, eps, only_stereo, coarse)
            assert got == host, "K1 of %d features against %s, flags %s" % (SIZES[k1], [SIZES[j] for j in k2s], (only_stereo, coarse, ori))
            wrong = m.SearchForTriangulationResident(ex, kfs[k1], good[k1], [kfs[j] for j in k2s], [good[j] for j in k2s], Fs, eps, only_stereo, coarse)
            if (only_stereo, coarse) == (0, 1):
                # feature i of K1 meets feature i of a neighbour; 0.4 of a row's entries are NONE or EMPTY, so 0.16 of the pairs are free on both sides:
                # half of that expectation is asked for (bCoarse skips the epipolar test, and the orientation check is off)
                expect = 0.16 * sum(min(SIZES[k1], SIZES[j]) for j in k2s)
                print("K1 of %d features: %d matches, %.0f expected" % (SIZES[k1], sum(n for n, _ in host), expect))
                assert sum(n for n, _ in host) >= expect / 2, "the scene matches"
                assert wrong != host, "reading the bad flag would change nothing: the test cannot tell the rules apart"
                differ += 1
            total += sum(n for n, _ in host)
    assert total > 0 and differ == 4                 # (each coarse case has checked its own match count above)
    # no neighbour, and an update of the map that the next call sees: every point of K1's row taken away
    m = M.ORBmatcher(0.6, True)
    assert m.SearchForTriangulationResidentMap(ex, kfs[0], rows[0], [], np.zeros(0, np.int32), store.map, np.zeros((0, 9), np.float32), np.zeros((0, 2), np.float32)) == []
    before = m.SearchForTriangulationResidentMap(ex, kfs[3], rows[3], [kfs[2]], rows[[2]], store.map, [F_X], [EP_FAR], 0, 1)
    store.set_keyframe(int(rows[3]), np.full(SIZES[3], -1, np.int32))
    after = m.SearchForTriangulationResidentMap(ex, kfs[3], rows[3], [kfs[2]], rows[[2]], store.map, [F_X], [EP_FAR], 0, 1)
    none = m.SearchForTriangulationResident(ex, kfs[3], None, [kfs[2]], [point[2]], [F_X], [EP_FAR], 0, 1)
    assert after == none and after[0][0] > before[0][0]
    for k in kfs:
        k.close()
    store.close(); ex.close()
    assert _live(lib) == live0


def test_triangulation_rows_emulated(emu_lib):
    _triangulation(emu_lib)


@pytest.mark.gpu
def test_triangulation_rows_gpu(hip_lib):
    _triangulation(hip_lib)


# ---- SearchByBoW(KeyFrame, KeyFrame): "holds a good point" -------------------------------------------------------------------------------------

def _bow(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(32)
    ex, kfs, store, rows = _small_world(lib, rng)
    point = [_flags(store, r, "point") for r in rows]; good = [_flags(store, r, "good") for r in rows]
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
    K1s = [kfs[a] for a, _ in pairs]; K2s = [kfs[b] for _, b in pairs]
    rows1 = rows[[a for a, _ in pairs]]
    total, differ = 0, 0
    for rows2, elig in ((np.array([rows[1], -1, rows[3], rows[0]], np.int32), [good[1], None, good[3], good[0]]), (None, [None] * 4)):     # a pair with rows2 = -1; no rows2 at all
        for frame_version, ratio, ori in ((False, 0.7, True), (True, 0.9, False)):
            m = M.ORBmatcher(ratio, ori)
            host = m.SearchByBoWResident(ex, K1s, [good[a] for a, _ in pairs], K2s, elig, frame_version)
            got = m.SearchByBoWResidentMap(ex, K1s, rows1, K2s, rows2, store.map, frame_version)
            for p in range(len(pairs)):
                assert got[p][0] == host[p][0] and np.array_equal(got[p][1], host[p][1]), "pair %d, rows2 %s, %s" % (p, rows2, (frame_version, ratio, ori))
            wrong = m.SearchByBoWResident(ex, K1s, [point[a] for a, _ in pairs], K2s, [None if e is None else point[b] for e, (_, b) in zip(elig, pairs)], frame_version)
            assert any(w[0] != h[0] or not np.array_equal(w[1], h[1]) for w, h in zip(wrong, host)), "ignoring the bad flag would change nothing"
            differ += 1
            total += sum(h[0] for h in host)
    assert total > 60 and differ == 4
    for k in kfs:
        k.close()
    store.close(); ex.close()
    assert _live(lib) == live0


def test_bow_rows_emulated(emu_lib):
    _bow(emu_lib)


@pytest.mark.gpu
def test_bow_rows_gpu(hip_lib):
    _bow(hip_lib)


# ---- both, anchored to the reference --------------------------------------------------------------------------------------------------------------

def _reference_world(k1, k2, kinds1, kinds2):
    """the reference's SearchForTriangulation and SearchByBoW(KF, KF) on a world holding the two key frames of tests/test_branch_edges_triangulation.py with a
    map point where the row says GOOD or BAD (bad: SetBadFlag'ed) and none where it says NONE or EMPTY.
    ({(bOnlyStereo, bCoarse, ori): (n, matches12)}, {(ratio, ori): (n, matches12 as features of key frame 2)})"""
    from test_branch_edges_triangulation import P1
    drv = mw.Driver(REF_MW)
    drv.L.mw_add_camera_kb8.restype = C.c_int
    c1 = drv.L.mw_add_camera_kb8(drv.w, mw._p(P1))
    ids, mps = [], []
    for k, kinds in ((k1, kinds1), (k2, kinds2)):
        kid = drv.frame(True, k["keys"].astype(mw.KP), k["desc"], k["ur"], k["R"], k["t"], c1)
        drv.set_feat_vec(True, kid, k["node"])
        mp = np.full(len(kinds), -1, np.int32)
        for i in np.flatnonzero(np.isin(kinds, (GOOD, BAD))):
            mp[i] = drv.mappoint(np.array([0, 0, 3.0]), np.array([0, 0, 1.0]), 0.5, 30.0, k["desc"][i], bad=int(kinds[i] == BAD))
        drv.set_map_points(True, kid, mp)
        ids.append(kid); mps.append(mp)
    N1 = len(kinds1)
    tri, bow = {}, {}
    for flags in TRI_FLAGS:
        pairs = np.full((N1, 2), -1, np.int32); npairs = C.c_int(0)
        n = drv.L.mw_search_for_triangulation(drv.w, ids[0], ids[1], flags[0], flags[1], mw._p(pairs), len(pairs), C.byref(npairs), C.c_float(0.6), flags[2])
        m12 = np.full(N1, -1, np.int32); m12[pairs[:npairs.value, 0]] = pairs[:npairs.value, 1]
        tri[flags] = (n, m12)
    feature_of = {int(m): i for i, m in enumerate(mps[1]) if m >= 0}
    for ratio, ori in BOW_PARAMS:
        o = np.full(N1, -1, np.int32)
        n = drv.L.mw_search_by_bow_keyframes(drv.w, ids[0], ids[1], mw._p(o), C.c_float(ratio), int(ori))
        bow[(ratio, ori)] = (n, np.array([feature_of[int(v)] if v >= 0 else -1 for v in o], np.int32))
    drv.close()
    return tri, bow


TRI_FLAGS = ((0, 0, 1), (0, 1, 0), (1, 0, 1))
BOW_PARAMS = ((0.8, True), (0.55, False))


def _anchored(lib):
    from test_branch_edges_triangulation import _world, _pair
    live0 = _live(lib)
    rng = np.random.default_rng(33)
    k1, k2 = _world()["mono"]
    N1, N2 = len(k1["keys"]), len(k2["keys"])
    kinds1, kinds2 = _kinds(rng, N1), _kinds(rng, N2)
    ref_tri, ref_bow = _reference_world(k1, k2, kinds1, kinds2)
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    r1, r2 = M.ResidentKeyFrame(ex, k1["view"]), M.ResidentKeyFrame(ex, k2["view"])
    store = Store(ex, kf_rows=2, kf_row_cap=max(N1, N2))
    free = list(rng.permutation(SLOTS))
    _fill_row(store, rng, free, 1, kinds1); _fill_row(store, rng, free, 0, kinds2)
    kb, ep = _pair(k1, k2)
    for only_stereo, coarse, ori in TRI_FLAGS:
        (n, pairs), = M.ORBmatcher(0.6, bool(ori)).SearchForTriangulationResidentMap(ex, r1, 1, [r2], [0], store.map, None, [ep], only_stereo, coarse, cams=kb)
        m12 = np.full(N1, -1, np.int32)
        for a, b in pairs:
            m12[a] = b
        rn, rm = ref_tri[(only_stereo, coarse, ori)]
        print("triangulation %s: %d matches (reference %d)" % ((only_stereo, coarse, ori), n, rn))
        assert n == rn and np.array_equal(m12, rm), "triangulation %s: %d vs the reference's %d" % ((only_stereo, coarse, ori), n, rn)
        matched = np.flatnonzero(m12 >= 0)
        assert not np.isin(kinds1[matched], (GOOD, BAD)).any() and not np.isin(kinds2[m12[matched]], (GOOD, BAD)).any()
    assert ref_tri[(0, 0, 1)][0] >= 20 and ref_tri[(0, 1, 0)][0] >= 20
    for ratio, ori in BOW_PARAMS:
        (n, m12), = M.ORBmatcher(ratio, ori).SearchByBoWResidentMap(ex, [r1], [1], [r2], [0], store.map, frame_version=False)
        rn, rm = ref_bow[(ratio, ori)]
        print("key-frame BoW %s: %d matches (reference %d)" % ((ratio, ori), n, rn))
        assert n == rn and np.array_equal(m12, rm), "key-frame BoW %s: %d vs the reference's %d" % ((ratio, ori), n, rn)
        matched = np.flatnonzero(m12 >= 0)
        assert (kinds1[matched] == GOOD).all() and (kinds2[m12[matched]] == GOOD).all()
    assert ref_bow[BOW_PARAMS[0]][0] >= 20
    r1.close(); r2.close(); store.close(); ex.close()
    assert _live(lib) == live0


@needs_world
def test_rows_against_the_reference_emulated(emu_lib):
    _anchored(emu_lib)


@needs_world
@pytest.mark.gpu
def test_rows_against_the_reference_gpu(hip_lib):
    _anchored(hip_lib)


# ---- SearchByBoW(pKF, F) for rig frames ----------------------------------------------------------------------------------------------------------------

needs_rig = pytest.mark.skipif(ol.reference_frame_lib() is None or ol.reference_dbow2() is None or not os.path.exists(REF_MW),
                               reason="oracle/_ref (libref_frame.so, libref_dbow2.so, libmw_ref.so) not built (needs the reference sources)")


def _rig_bow(lib, tmp_path):
    """at the emulator shape of tests/test_rig_bow_batch.py: TrackReferenceKeyFrame pairs (rig and one-camera key frames) and a fan-out of one frame"""
    import test_rig_bow_batch as RB
    W = RB.World(lib, 376, 376, 500, (0, 375), 3, 2, two_handles=False, seed=0)
    rng = np.random.default_rng(34)
    store = None
    try:
        voc, ref = RB._vocabulary(W.exL, tmp_path, 31, 6, 3, 0, 0)
        voc.transform_rig_extracted(W.exL, W.lf, W.exR, W.rf, W.B, 1)
        pairs = [(b, RB._KF(W, W.exL, ref, 1, rng, b, rig=(b % 2 == 0))) for b in range(W.B)] + [(1, RB._KF(W, W.exL, ref, 1, rng, 1, rig=True, frac=0.6)),
                                                                                                   (1, RB._KF(W, W.exL, ref, 1, rng, 0, rig=False))]
        frames = [b for b, _ in pairs]; kfs = [k for _, k in pairs]
        store = Store(W.exL, kf_rows=len(kfs) + 2, kf_row_cap=max(k.N for k in kfs))
        free = list(rng.permutation(SLOTS))
        rows = rng.permutation(len(kfs) + 2)[:len(kfs)].astype(np.int32)
        for p, k in enumerate(kfs):
            _fill_row(store, rng, free, rows[p], _kinds(rng, k.N))
        good = [_flags(store, r, "good") for r in rows]; point = [_flags(store, r, "point") for r in rows]
        n_frame = [sum(W.n(b)) for b in range(W.B)]
        total = 0
        for ratio, ori in RB.PARAM_SETS:
            m = M.ORBmatcher(ratio, ori)
            args = (W.exL, W.lf, W.exR, W.rf, voc, frames, [k.res for k in kfs])
            host = m.SearchByBoWRigBatch(*args, good, n_frame)
            got = m.SearchByBoWRigBatch(*args, None, n_frame, resident_map=store.map, rows=rows)
            wrong = m.SearchByBoWRigBatch(*args, point, n_frame)
            for p in range(len(kfs)):
                assert got[p][0] == host[p][0] and np.array_equal(got[p][1], host[p][1]), "pair %d (ratio %g)" % (p, ratio)
            assert any(w[0] != h[0] or not np.array_equal(w[1], h[1]) for w, h in zip(wrong, host)), "ignoring the bad flag would change nothing"
            total += sum(h[0] for h in host)
        assert total > 20 * len(kfs)
        for k in kfs:
            k.close()
        voc.close()
    finally:
        if store is not None:
            store.close()
        W.close()


@needs_rig
def test_rig_bow_rows_emulated(emu_lib, tmp_path):
    _rig_bow(emu_lib, tmp_path)


@needs_rig
@pytest.mark.gpu
def test_rig_bow_rows_gpu(hip_lib, tmp_path):
    _rig_bow(hip_lib, tmp_path)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------

def _refusals(lib):
    L = lib.L
    live0 = _live(lib)
    rng = np.random.default_rng(35)
    ex, kfs, store, rows = _small_world(lib, rng)
    spare = [r for r in range(len(SIZES) + 3) if r not in rows]
    unset, short = spare[0], spare[1]
    store.set_keyframe(short, store.rows[int(rows[0])][:-1])                         # one entry less than key frame 0 has features
    m12 = np.full((3, max(SIZES)), -1, np.int32); nm = np.zeros(3, np.int32)
    K2 = (C.c_void_p * 1)(kfs[1]._kf); r2 = np.array([rows[1]], np.int32)
    err = lambda: L.orbx_last_error() or b""

    def tri(K1=kfs[0]._kf, row1=int(rows[0]), K2s=K2, rows2=r2, mp=store.map._m, F=F_X.ctypes.data):
        return L.orbm_search_for_triangulation_resident_map(ex._h, K1, row1, 1, K2s, None if rows2 is None else rows2.ctypes.data, mp, F, EP_FAR.ctypes.data, 0, 1, 1,
                                                            m12.ctypes.data, nm.ctypes.data)
    assert tri() == 0
    assert tri(mp=None) == E_ARG and tri(rows2=None) == E_ARG and tri(K1=None) == E_ARG and tri(K2s=None) == E_ARG and tri(F=None) == E_ARG
    for kw, text in ((dict(row1=-1), b"row -1"), (dict(row1=len(SIZES) + 3), b"outside"), (dict(row1=unset), b"never set"), (dict(row1=short), b"holds"),
                     (dict(rows2=np.array([unset], np.int32)), b"never set"), (dict(rows2=np.array([rows[2]], np.int32)), b"holds")):
        assert tri(**kw) == E_ARG and text in err(), (kw, err())
    assert L.orbm_search_for_triangulation_resident_kb8_map(ex._h, kfs[0]._kf, int(rows[0]), 1, K2, r2.ctypes.data, store.map._m, None, EP_FAR.ctypes.data, 0, 1, 1,
                                                            m12.ctypes.data, nm.ctypes.data) == E_ARG
    K1 = (C.c_void_p * 1)(kfs[0]._kf); r1 = np.array([rows[0]], np.int32)
    out = (C.c_void_p * 1)(m12.ctypes.data)

    def bow(K1s=K1, rows1=r1, rows2=r2, mp=store.map._m, outs=out):
        return L.orbm_search_by_bow_resident_map(ex._h, 1, K1s, None if rows1 is None else rows1.ctypes.data, K2, None if rows2 is None else rows2.ctypes.data, mp, 0.7, 1, 1,
                                                 outs, nm.ctypes.data)
    assert bow() == 0 and bow(rows2=None) == 0 and bow(rows2=np.array([-1], np.int32)) == 0
    assert bow(mp=None) == E_ARG and bow(rows1=None) == E_ARG and bow(K1s=None) == E_ARG and bow(outs=None) == E_ARG
    for kw, text in ((dict(rows1=np.array([unset], np.int32)), b"never set"), (dict(rows1=np.array([short], np.int32)), b"holds"), (dict(rows2=np.array([-2], np.int32)), b"row -2"),
                     (dict(rows2=np.array([rows[0]], np.int32)), b"holds")):
        assert bow(**kw) == E_ARG and text in err(), (kw, err())
    # the rig BoW form refuses its map arguments before it looks at the vocabulary's last transform
    fr = np.zeros(1, np.int32)
    rig = lambda mp=store.map._m, rws=r1: L.orbm_search_by_bow_rig_batch_map(ex._h, 0, ex._h, 1, 1, None, 1, fr.ctypes.data, K1, mp, None if rws is None else rws.ctypes.data, 0.7, 1, out, nm.ctypes.data)
    assert rig() == E_ARG and rig(mp=None) == E_ARG and rig(rws=None) == E_ARG       # (no vocabulary)
    for k in kfs:
        k.close()
    store.close(); ex.close()
    assert _live(lib) == live0


def test_row_refusals_emulated(emu_lib):
    _refusals(emu_lib)


@pytest.mark.gpu
def test_row_refusals_gpu(hip_lib):
    _refusals(hip_lib)
