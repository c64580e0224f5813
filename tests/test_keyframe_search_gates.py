"""The gates of ORBmatcher::SearchForTriangulation and SearchByBoW between key frames (csrc/k_search.hip: bow_search_core, sft_resident_body, bow_match_node, rot_bin) on
hand-built key frames whose features sit ON the values where the lines decide - survivors of the mutation pass recorded in profiles/emu_mutants/README.md.  Every
situation has a vocabulary node of its own (one feature of KF1, one or two of KF2), so that no situation meets another; the fundamental matrix is that of a pure x
translation (epipolar line y2 == y1, squared distance (y2 - y1)^2 exactly), the epipole is (500, 300).  Expected pairs: the oracle's restatement of
src/ORBmatcher.cc:1045-1323 / :259-493 (ol.oracle_search_for_triangulation, ol.oracle_search_by_bow), and the test asserts on the ORACLE's answer that each situation came
out as it was aimed.

SearchForTriangulation (host-fed and resident form):
  line_in / line_out   y2 - y1 = 1.5 / 2.2 at octave 0 (sigma2 = 1): 2.25 < 3.84 matches, 4.84 does not (and would under the 2-dof bound 5.99)
  line_zero            KF2's level-7 sigma2 is 0 and y2 == y1: `dsqr < 3.84 * sigma2` is 0 < 0, refused - the one input where the strict comparison shows, the literal
                       3.84 being no float
  epipole_on / _in     a monocular pair whose KF2 keypoint is exactly 10 px (6, 8) from the epipole at octave 0: `distex * distex + distey * distey < 100 * scale` is
                       100 < 100, kept; at (6, 7.5) it is inside the circle and skipped
  epipole_stereo2      a KF2 keypoint with a right coordinate 5 px from the epipole: the circle is not tested for stereo keypoints
  ur2_zero             the same with a right coordinate of exactly 0: `mvuRight[idx2] >= 0` makes it stereo
  ur1_zero             bOnlyStereo with a KF1 keypoint whose right coordinate is exactly 0: stereo, searched
SearchByBoW (host-fed and resident form), mfNNratio = 0.5, orientation check on:
  ratio_on / ratio_in  best and second best at 20 and 40: `bestDist1 < mfNNratio * bestDist2` is 20 < 20, no match; at 19 and 40 a match
  rotation             16 matches: three with equal angles (rot == 0 exactly: bin 0), three with rot = 355 (bin 12), six in bin 3, four in bin 6.  ComputeThreeMaxima keeps
                       bins 3, 6 and - the first of the two with three entries - bin 0; the three of bin 12 are erased.  (A rot of exactly 0 that took the `+ 360` branch
                       would fall into bin 12, make it the fullest and save those three.)"""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, views
from orb_slam3_detailed_comments_amd import matcher as M
from orb_slam3_detailed_comments_amd.extractor import KP_DTYPE
from resident_inject import at_distance

f32 = np.float32
SF = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
SIGMA2 = (SF * SF).astype(f32)
F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32)
EP = np.array([500.0, 300.0], f32)


class _Builder:
    """two key frames, one vocabulary node per situation"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.k = ([], []); self.d = ([], []); self.ur = ([], []); self.nodes = ([], [])
        self.where = {}

    def add(self, name, f1, f2s):
        """f1 / each of f2s: (x, y, octave, angle, ur, distance of its descriptor from the node's).  Remembers name -> (index in KF1, indices in KF2)."""
        D = self.rng.integers(0, 256, 32, dtype=np.uint8)
        idx = []
        for side, feats in ((0, [f1]), (1, f2s)):
            mine = []
            for (x, y, octave, angle, ur, dist) in feats:
                rec = np.zeros(1, KP_DTYPE); rec["x"], rec["y"], rec["octave"], rec["angle"] = x, y, octave, angle
                mine.append(len(self.k[side]))
                self.k[side].append(rec); self.d[side].append(at_distance(self.rng, D, dist)); self.ur[side].append(ur)
            self.nodes[side].append(mine); idx.append(mine)
        self.where[name] = (idx[0][0], idx[1])

    def views(self, mp1, mp2, sigma2_2=SIGMA2):
        out = []
        for side, mp, s2 in ((0, mp1, SIGMA2), (1, mp2, sigma2_2)):
            k = np.concatenate(self.k[side]); d = np.stack(self.d[side]); ur = np.array(self.ur[side], f32)
            nid = np.arange(len(self.nodes[side]), dtype=np.uint32)
            st = np.cumsum([0] + [len(n) for n in self.nodes[side]]).astype(np.int32)
            ft = np.array([i for n in self.nodes[side] for i in n], np.uint32)
            out.append(views.key_frame_view(k, d, SF, s2, nid, st, ft, ur, np.full(len(k), mp, np.uint8)))
        return out


_DONE = {}


def _triangulation_case():
    if "tri" not in _DONE:
        b = _Builder(21)
        mono = -1.0
        b.add("line_in", (100, 50, 0, 0, mono, 0), [(120, 51.5, 0, 0, mono, 0)])
        b.add("line_out", (100, 80, 0, 0, mono, 0), [(120, 82.2, 0, 0, mono, 0)])
        b.add("line_zero", (100, 110, 0, 0, mono, 0), [(120, 110, 7, 0, mono, 0)])
        b.add("epipole_on", (100, 292, 0, 0, mono, 0), [(494, 292, 0, 0, mono, 0)])
        b.add("epipole_in", (100, 292.5, 0, 0, mono, 0), [(494, 292.5, 0, 0, mono, 0)])
        b.add("epipole_stereo2", (100, 296, 0, 0, mono, 0), [(497, 296, 0, 0, 100.0, 0)])
        b.add("ur2_zero", (100, 297, 0, 0, mono, 0), [(496, 297, 0, 0, 0.0, 0)])
        b.add("ur1_zero", (100, 20, 0, 0, 0.0, 0), [(120, 20, 0, 0, 50.0, 0)])
        s2 = SIGMA2.copy(); s2[7] = 0
        kf1, kf2 = b.views(0, 0, s2)
        exp = {}
        for only_stereo in (False, True):
            n, pairs = ol.oracle_search_for_triangulation(kf1, kf2, F12, EP, only_stereo, False, False)
            got = dict(pairs)
            hit = {name: got.get(i1) == i2[0] for name, (i1, i2) in b.where.items()}
            if only_stereo:
                assert hit["ur1_zero"] and n == 1, (hit, pairs)
            else:
                want = dict(line_in=True, line_out=False, line_zero=False, epipole_on=True, epipole_in=False, epipole_stereo2=True, ur2_zero=True, ur1_zero=True)
                assert hit == want, hit
            exp[only_stereo] = (n, pairs)
        _DONE["tri"] = (kf1, kf2, exp)
    return _DONE["tri"]


def _check_triangulation(lib):
    kf1, kf2, exp = _triangulation_case()
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    rk1, rk2 = M.ResidentKeyFrame(ex, kf1), M.ResidentKeyFrame(ex, kf2)
    try:
        for only_stereo, want in exp.items():
            got = M.ORBmatcher(0.6, False).SearchForTriangulation(ex, kf1, kf2, F12, EP, only_stereo, False)
            assert got == want, "SearchForTriangulation(only_stereo=%s): %r, expected %r" % (only_stereo, got, want)
            res = M.ORBmatcher(0.6, False).SearchForTriangulationResident(ex, rk1, kf1.keep[8], [rk2], [kf2.keep[8]], F12[None], EP[None], only_stereo, False)
            assert res[0] == want, "resident SearchForTriangulation(only_stereo=%s): %r, expected %r" % (only_stereo, res[0], want)
    finally:
        rk1.close(); rk2.close(); ex.close()


def _bow_case():
    if "bow" not in _DONE:
        b = _Builder(22)
        b.add("ratio_on", (50, 50, 0, 100, -1.0, 0), [(60, 50, 0, 10, -1.0, 20), (70, 50, 0, 10, -1.0, 40)])
        b.add("ratio_in", (50, 60, 0, 100, -1.0, 0), [(60, 60, 0, 10, -1.0, 19), (70, 60, 0, 10, -1.0, 40)])
        for name, count, a1, a2 in (("zero", 3, 10.0, 10.0), ("r355", 3, 355.0, 0.0), ("r90", 5, 100.0, 10.0), ("r180", 4, 200.0, 20.0)):
            for i in range(count):
                b.add("%s_%d" % (name, i), (100 + 7 * i, 100, 0, a1, -1.0, 0), [(100 + 7 * i, 120, 0, a2, -1.0, 0)])
        kf1, kf2 = b.views(1, 1)
        exp = {}
        for frame_version in (True, False):
            n, m = ol.oracle_search_by_bow(kf1, kf2, 0.5, frame_version, True)
            hit = {name: m[i1] == i2[0] for name, (i1, i2) in b.where.items()}
            assert not hit["ratio_on"] and hit["ratio_in"], hit
            for name in hit:
                if name[0] in "zr" and "_" in name and not name.startswith("ratio"):
                    assert hit[name] == (not name.startswith("r355")), (name, hit)
            assert n == 13
            exp[frame_version] = (n, m)
        _DONE["bow"] = (kf1, kf2, exp)
    return _DONE["bow"]


def _check_bow(lib):
    kf1, kf2, exp = _bow_case()
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    rk1, rk2 = M.ResidentKeyFrame(ex, kf1), M.ResidentKeyFrame(ex, kf2)
    try:
        for frame_version, (n, m) in exp.items():
            n1, m1 = M.ORBmatcher(0.5, True).SearchByBoW(ex, kf1, kf2, frame_version)
            assert n1 == n and np.array_equal(m1, m), "SearchByBoW(frame_version=%s): %d matches, expected %d; differs at %s" % (frame_version, n1, n, np.flatnonzero(m1 != m))
            got = M.ORBmatcher(0.5, True).SearchByBoWResident(ex, [rk1], [kf1.keep[8]], [rk2], [kf2.keep[8]], frame_version)
            assert got[0][0] == n and np.array_equal(got[0][1], m), "resident SearchByBoW(frame_version=%s): %d matches, expected %d; differs at %s" % (
                frame_version, got[0][0], n, np.flatnonzero(got[0][1] != m))
    finally:
        rk1.close(); rk2.close(); ex.close()


def test_triangulation_search_gates_emulated(emu_lib):
    _check_triangulation(emu_lib)


@pytest.mark.gpu
def test_triangulation_search_gates_gpu(hip_lib):
    _check_triangulation(hip_lib)


def test_bow_ratio_and_rotation_gates_emulated(emu_lib):
    _check_bow(emu_lib)


@pytest.mark.gpu
def test_bow_ratio_and_rotation_gates_gpu(hip_lib):
    _check_bow(hip_lib)


# ---- the Kannala-Brandt form: KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:322-328) accepts `TriangulateMatches(..) > 0.0001f` -----------------
def _kb8_case():
    """Pairs of the 2 mm rig of tests/test_kb8_stereo_constructed.py whose triangulated depth lies either side of 1e-4, on it and one float beside it, each in a vocabulary
    node of its own with equal descriptors: a pair is matched iff the depth of csrc/kb8_model.h built for the HOST (that file's checker, bit for bit) is above float(1e-4).
    A gate of 0 instead of 1e-4 would match the pairs with 0 < z <= 1e-4 as well."""
    if "kb8" not in _DONE:
        import test_kb8_stereo_constructed as K
        rig = K.RIG_SMALL
        zs = np.array([0.5e-4, 0.8e-4, 0.95e-4, 0.999e-4, 1.001e-4, 1.05e-4, 1.2e-4, 2e-4, 1e-3], np.float64)
        X = np.stack([np.full(len(zs), 0.001) * zs / 1e-4, 0.003 * zs / 1e-4, zs], 1)
        uv1 = [K._project64(rig["cam1"], X).astype(f32)]; uv2 = [K._right_pixels(rig, X)]
        th = f32(0.0001)
        for a, b2 in K._pairs_at_depth(rig, SIGMA2, (th, np.nextafter(th, f32(1)), np.nextafter(th, f32(0)))).values():
            uv1.append(a); uv2.append(b2)
        uv1 = np.concatenate(uv1); uv2 = np.concatenate(uv2)
        z, _ = K.triangulate(rig, uv1, uv2, np.full(len(uv1), SIGMA2[0]), np.full(len(uv1), SIGMA2[0]))
        assert ((z > 0) & (z <= th)).sum() >= 5 and (z == th).sum() >= 2 and (z == np.nextafter(th, f32(1))).sum() >= 2 and (z > th).sum() >= 5, z
        b = _Builder(23)
        for i in range(len(uv1)):
            b.add("p%d" % i, (uv1[i, 0], uv1[i, 1], 0, 0, -1.0, 0), [(uv2[i, 0], uv2[i, 1], 0, 0, -1.0, 0)])
        kf1, kf2 = b.views(0, 0)
        m12 = np.where(z > th, np.arange(len(uv1)), -1).astype(np.int32)               # node i holds feature i of either key frame
        _DONE["kb8"] = (rig, kf1, kf2, m12)
    return _DONE["kb8"]


def _check_kb8(lib):
    import ctypes as C
    from test_branch_edges_triangulation import _KB8Pair
    rig, kf1, kf2, exp = _kb8_case()
    kb = _KB8Pair()
    kb.nleft1 = kb.nleft2 = -1                                                         # two one-camera key frames: pair 0 of the relative poses, camera 0 of either side
    kb.cam1[:] = list(rig["cam1"]) * 2; kb.cam2[:] = list(rig["cam2"]) * 2
    kb.R[:] = [float(v) for v in np.asarray(rig["R12"], f32).ravel()] * 4; kb.t[:] = [float(v) for v in rig["t12"]] * 4
    ep = np.array([1.0e6, 0.0], f32)                                                  # far from every keypoint: the epipole circle (:1189-1198) rejects nothing
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    rk1, rk2 = M.ResidentKeyFrame(ex, kf1), M.ResidentKeyFrame(ex, kf2)
    try:
        N1 = len(exp)
        m12 = np.full(N1, -1, np.int32); nm = C.c_int(-1)
        lib.check(lib.L.orbm_search_for_triangulation_kb8(ex._h, kf1.ref(), kf2.ref(), C.byref(kb), ep.ctypes.data, 0, 0, 0, m12.ctypes.data, C.byref(nm)))
        assert np.array_equal(m12, exp) and nm.value == int((exp >= 0).sum()), "KB8 triangulation search: %s, expected %s" % (m12, exp)
        res = np.full(N1, -1, np.int32); nres = np.zeros(1, np.int32)
        p2 = (C.c_void_p * 1)(rk2._kf); pm2 = (C.c_void_p * 1)(kf2.keep[8].ctypes.data)
        lib.check(lib.L.orbm_search_for_triangulation_resident_kb8(ex._h, rk1._kf, kf1.keep[8].ctypes.data, 1, p2, pm2, C.byref(kb), ep.ctypes.data, 0, 0, 0,
                                                                   res.ctypes.data, nres.ctypes.data))
        assert np.array_equal(res, exp) and nres[0] == int((exp >= 0).sum()), "resident KB8 triangulation search: %s, expected %s" % (res, exp)
    finally:
        rk1.close(); rk2.close(); ex.close()


def test_triangulation_search_kb8_depth_gate_emulated(emu_lib):
    _check_kb8(emu_lib)


@pytest.mark.gpu
def test_triangulation_search_kb8_depth_gate_gpu(hip_lib):
    _check_kb8(hip_lib)
