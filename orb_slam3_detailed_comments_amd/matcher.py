"""Host-side mirror of the reference's descriptor matchers on top of the HIP library:
``ORBmatcher::DescriptorDistance`` (src/ORBmatcher.cc:2383-2403), ``Frame::ComputeStereoMatches``
(src/Frame.cc:1102-1358) and the kNN + ratio part of ``Frame::ComputeStereoFishEyeMatches`` (:1553-1562)."""
import ctypes as C

import numpy as np

from ._lib import OrbxError
from .sophus import SE3f, Sim3f, as_se3
from .views import FuseTarget, Sim3Target, Projection as _Projection


def _ptrs(items, n=None):
    """A C array of n pointers (default: one per item), never of length 0, that starts with the items (None: a null pointer)."""
    items = list(items)
    return (C.c_void_p * max(len(items) if n is None else n, 1))(*items)


def _flag_ptrs(flags, n, optional=False):
    """The call-time flag arrays of n key frames as (uint8 arrays - to be kept alive over the call -, their C array of pointers); optional: None passes as a
    null pointer."""
    arrays = [None if optional and m is None else np.ascontiguousarray(m, np.uint8) for m in flags]
    return arrays, _ptrs((None if m is None else m.ctypes.data for m in arrays), n)


def _match_rows(kfs):
    """One row of matches per key frame, pre-set to -1, the rows' C array of pointers and the match counts."""
    outs = [np.full(max(k.N, 1), -1, np.int32) for k in kfs]
    return outs, _ptrs(o.ctypes.data for o in outs), np.zeros(max(len(kfs), 1), np.int32)


def _matched_rows(nm, outs, kfs):
    """[(nmatches, matches12[N1])] per key frame from what _match_rows laid out."""
    return [(int(nm[p]), outs[p][:k.N]) for p, k in enumerate(kfs)]


def _neighbour_pairs(nm, m12, n2, N1):
    """[(nmatches, [(i1, i2)...])] per neighbour from the (n2, N1) block a resident triangulation search filled."""
    m12 = m12.reshape(-1)[:n2 * N1].reshape(n2, N1) if N1 > 0 else m12[:n2, :0]
    return [(int(nm[j]), [(int(i), int(m12[j, i])) for i in np.nonzero(m12[j] >= 0)[0]]) for j in range(n2)]


class ORBmatcher:
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30   # src/ORBmatcher.cc:35-37

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio, self.mbCheckOrientation = float(nnratio), bool(checkOri)

    def SearchByProjection(self, ext, frame, map_points, th=1.0, bFarPoints=False, thFarPoints=50.0):
        """ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints), src/ORBmatcher.cc:45.
        frame / map_points: views.frame_view(...) / views.map_point_view(...).  Returns (nmatches, assigned[N]) where
        assigned[i] is the index of the map point written to F.mvpMapPoints[i] (-1: untouched)."""
        N = frame.view.N
        assigned = np.full(N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_mappoints(ext._h, frame.ref(), map_points.ref(), float(th), int(bFarPoints),
                                                                    float(thFarPoints), self.mfNNratio, assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def SearchByProjectionFrame(self, ext, cur, last, th, bForward=False, bBackward=False):
        """ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono), src/ORBmatcher.cc:1950.
        Returns (nmatches, assigned[N]): index into the last frame, -1 untouched, -2 reset by the rotation check."""
        N = cur.view.N
        assigned = np.full(N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_frame(ext._h, cur.ref(), last.ref(), float(th), int(bForward), int(bBackward),
                                                                int(self.mbCheckOrientation), assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def SearchForTriangulation(self, ext, kf1, kf2, F12, ep, bOnlyStereo=False, bCoarse=False):
        """ORBmatcher::SearchForTriangulation, src/ORBmatcher.cc:1045 (pinhole).  Returns (nmatches, vMatchedPairs [(i1,i2)...])."""
        F12 = np.ascontiguousarray(F12, np.float32).reshape(9); ep = np.ascontiguousarray(ep, np.float32).reshape(2)
        m12 = np.full(kf1.view.N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_for_triangulation(ext._h, kf1.ref(), kf2.ref(), F12.ctypes.data, ep.ctypes.data, int(bOnlyStereo),
                                                              int(bCoarse), int(self.mbCheckOrientation), m12.ctypes.data, C.byref(nm)))
        idx = np.nonzero(m12 >= 0)[0]
        return nm.value, [(int(i), int(m12[i])) for i in idx]

    def SearchForTriangulationBatch(self, ext, kf1, kf2s, F12s, eps, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation of kf1 against every key frame of kf2s in one launch.  Returns a list of (nmatches, pairs) like
        SearchForTriangulation."""
        n2 = len(kf2s)
        F = np.ascontiguousarray(F12s, np.float32).reshape(n2, 9); E = np.ascontiguousarray(eps, np.float32).reshape(n2, 2)
        ptrs = (C.c_void_p * max(n2, 1))(*[C.cast(k.ref(), C.c_void_p) for k in kf2s])
        N1 = kf1.view.N
        m12 = np.full((max(n2, 1), max(N1, 1)), -1, np.int32); nm = np.zeros(max(n2, 1), np.int32)
        ext._lib.check(ext._lib.L.orbm_search_for_triangulation_batch(ext._h, kf1.ref(), n2, ptrs, F.ctypes.data, E.ctypes.data, int(bOnlyStereo), int(bCoarse),
                                                                    int(self.mbCheckOrientation), m12.ctypes.data, nm.ctypes.data))
        return [(int(nm[j]), [(int(i), int(m12[j, i])) for i in np.nonzero(m12[j, :N1] >= 0)[0]]) for j in range(n2)]

    def SearchByBoW(self, ext, kf1, kf2, frame_version=True):
        """ORBmatcher::SearchByBoW: frame_version=True is (KeyFrame*, Frame&, vpMapPointMatches), src/ORBmatcher.cc:259;
        False is (KeyFrame*, KeyFrame*, vpMatches12), :892.  Returns (nmatches, matches12[N1])."""
        m12 = np.full(kf1.view.N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_bow(ext._h, kf1.ref(), kf2.ref(), self.mfNNratio, int(frame_version), int(self.mbCheckOrientation),
                                                   m12.ctypes.data, C.byref(nm)))
        return nm.value, m12

    def SearchByBoWBatch(self, ext, kf1s, kf2s, frame_version=True):
        """SearchByBoW for the pairs (kf1s[p], kf2s[p]) in one launch (relocalisation candidates vs the current frame, a key frame vs its loop
        candidates).  Returns a list of (nmatches, matches12) like SearchByBoW."""
        n = len(kf1s)
        p1 = (C.c_void_p * max(n, 1))(*[C.cast(k.ref(), C.c_void_p) for k in kf1s]); p2 = (C.c_void_p * max(n, 1))(*[C.cast(k.ref(), C.c_void_p) for k in kf2s])
        outs = [np.full(max(k.view.N, 1), -1, np.int32) for k in kf1s]
        po = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs]); nm = np.zeros(max(n, 1), np.int32)
        ext._lib.check(ext._lib.L.orbm_search_by_bow_batch(ext._h, n, p1, p2, self.mfNNratio, int(frame_version), int(self.mbCheckOrientation), po, nm.ctypes.data))
        return [(int(nm[p]), outs[p][:kf1s[p].view.N]) for p in range(n)]

    def SearchForTriangulationResident(self, ext, kf1, mp1, kf2s, mp2s, F12s, eps, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulationBatch over ResidentKeyFrame objects: mp1 / mp2s[j] = uint8 flags "feature has a map point" at call time (None =
        none).  Returns the same list of (nmatches, pairs)."""
        n2 = len(kf2s)
        F = np.ascontiguousarray(F12s, np.float32).reshape(n2, 9); E = np.ascontiguousarray(eps, np.float32).reshape(n2, 2)
        ptrs = _ptrs(k._kf for k in kf2s)
        m1 = None if mp1 is None else np.ascontiguousarray(mp1, np.uint8)
        m2, pm2 = _flag_ptrs(mp2s, n2, optional=True)
        N1 = kf1.N
        m12 = np.full((max(n2, 1), max(N1, 1)), -1, np.int32); nm = np.zeros(max(n2, 1), np.int32)
        ext._lib.check(ext._lib.L.orbm_search_for_triangulation_resident(ext._h, kf1._kf, None if m1 is None else m1.ctypes.data, n2, ptrs, pm2, F.ctypes.data,
                                                                       E.ctypes.data, int(bOnlyStereo), int(bCoarse), int(self.mbCheckOrientation), m12.ctypes.data,
                                                                       nm.ctypes.data))
        return _neighbour_pairs(nm, m12, n2, N1)

    def SearchByBoWResident(self, ext, kf1s, mp1s, kf2s, elig2s, frame_version=True):
        """SearchByBoWBatch over ResidentKeyFrame objects: mp1s[p] = uint8 flags "feature of kf1s[p] has a good map point", elig2s[p] = flags of the
        features of kf2s[p] that may be matched (None = all).  Returns the same list of (nmatches, matches12)."""
        n = len(kf1s)
        p1 = _ptrs(k._kf for k in kf1s); p2 = _ptrs(k._kf for k in kf2s)
        a1, q1 = _flag_ptrs(mp1s, n, optional=True); a2, q2 = _flag_ptrs(elig2s, n, optional=True)
        outs, po, nm = _match_rows(kf1s)
        ext._lib.check(ext._lib.L.orbm_search_by_bow_resident(ext._h, n, p1, q1, p2, q2, self.mfNNratio, int(frame_version), int(self.mbCheckOrientation), po, nm.ctypes.data))
        return _matched_rows(nm, outs, kf1s)

    def SearchForTriangulationResidentMap(self, ext, kf1, row1, kf2s, rows2, resident_map, F12s, eps, bOnlyStereo=False, bCoarse=False, cams=None):
        """SearchForTriangulationResident with the flags read on the device from the key frames' rows in a ResidentMap
        (orbm_search_for_triangulation_resident_map): row1 / rows2[j] = the rows of kf1 / kf2s[j]; a feature has a map point iff its slot is >= 0 and
        holds a point - the bad flag is not read (src/ORBmatcher.cc:1123-1127, :1159-1163).  cams: a ctypes array of n2 OrbmKB8Pair in place of F12s
        (orbm_search_for_triangulation_resident_kb8_map).  Returns the same list of (nmatches, pairs)."""
        n2 = len(kf2s)
        E = np.ascontiguousarray(eps, np.float32).reshape(n2, 2)
        ptrs = _ptrs(k._kf for k in kf2s)
        r2 = np.ascontiguousarray(rows2, np.int32)
        if len(r2) != n2:
            raise ValueError("%d rows for %d neighbours" % (len(r2), n2))
        N1 = kf1.N
        m12 = np.full((max(n2, 1), max(N1, 1)), -1, np.int32); nm = np.zeros(max(n2, 1), np.int32)
        tail = (E.ctypes.data, int(bOnlyStereo), int(bCoarse), int(self.mbCheckOrientation), m12.ctypes.data, nm.ctypes.data)
        if cams is None:
            F = np.ascontiguousarray(F12s, np.float32).reshape(n2, 9)
            ext._lib.check(ext._lib.L.orbm_search_for_triangulation_resident_map(ext._h, kf1._kf, int(row1), n2, ptrs, r2.ctypes.data, resident_map._m, F.ctypes.data, *tail))
        else:
            ext._lib.check(ext._lib.L.orbm_search_for_triangulation_resident_kb8_map(ext._h, kf1._kf, int(row1), n2, ptrs, r2.ctypes.data, resident_map._m, C.addressof(cams), *tail))
        return _neighbour_pairs(nm, m12, n2, N1)

    def SearchByBoWResidentMap(self, ext, kf1s, rows1, kf2s, rows2, resident_map, frame_version=True):
        """SearchByBoWResident with the flags read on the device from the key frames' rows in a ResidentMap (orbm_search_by_bow_resident_map):
        rows1[p] = the row of kf1s[p], rows2 = None or rows2[p] = the row of kf2s[p] or -1 (every feature of kf2s[p] is eligible); an entry counts iff
        its slot is >= 0 and holds a point that is not bad.  Returns the same list of (nmatches, matches12)."""
        n = len(kf1s)
        p1 = _ptrs(k._kf for k in kf1s); p2 = _ptrs(k._kf for k in kf2s)
        r1 = np.ascontiguousarray(rows1, np.int32); r2 = None if rows2 is None else np.ascontiguousarray(rows2, np.int32)
        if len(r1) != n or (r2 is not None and len(r2) != n):
            raise ValueError("the row lists need %d entries" % n)
        outs, po, nm = _match_rows(kf1s)
        ext._lib.check(ext._lib.L.orbm_search_by_bow_resident_map(ext._h, n, p1, r1.ctypes.data, p2, None if r2 is None else r2.ctypes.data, resident_map._m, self.mfNNratio,
                                                                  int(frame_version), int(self.mbCheckOrientation), po, nm.ctypes.data))
        return _matched_rows(nm, outs, kf1s)

    def SearchByBoWFramesBatch(self, ext, voc, kfs, mps, first=0, resident_map=None, rows=None):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) for the frames [first, first + len(kfs)) of ext's last extraction on the device
        (orbm_search_by_bow_frames_batch): voc = the ORBVocabulary whose transform_extracted(ext, first, B, levelsup) has run on these frames, kfs[b] = the
        ResidentKeyFrame frame b is searched against, mps[b] = uint8 flags "feature of kfs[b] has a good map point".  Returns [(nmatches, matches12)]
        with matches12[i] = frame feature matched to key-frame feature i or -1.
        resident_map, rows (mps = None): the flags are read on the device from rows[b], the row of kfs[b] in the ResidentMap - an entry counts iff its
        slot is >= 0 and holds a point that is not bad (orbm_search_by_bow_frames_batch_map)."""
        B = len(kfs)
        p1 = _ptrs(k._kf for k in kfs)
        outs, po, nm = _match_rows(kfs)
        if resident_map is not None or rows is not None:
            if resident_map is None or rows is None or mps is not None:
                raise ValueError("the map-fed form takes resident_map and rows, and mps = None")
            r = np.ascontiguousarray(rows, np.int32)
            if len(r) != B:
                raise ValueError("%d rows for %d key frames" % (len(r), B))
            ext._lib.check(ext._lib.L.orbm_search_by_bow_frames_batch_map(ext._h, voc._v, int(first), B, p1, resident_map._m, r.ctypes.data, self.mfNNratio,
                                                                          int(self.mbCheckOrientation), po, nm.ctypes.data))
        else:
            a1, q1 = _flag_ptrs(mps, B)
            ext._lib.check(ext._lib.L.orbm_search_by_bow_frames_batch(ext._h, voc._v, int(first), B, p1, q1, self.mfNNratio, int(self.mbCheckOrientation), po, nm.ctypes.data))
        return _matched_rows(nm, outs, kfs)

    def SearchByBoWRigBatch(self, exL, lf, exR, rf, voc, frames, kfs, mps, n_frame=None, resident_map=None, rows=None):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) for fisheye-rig frames on the device (orbm_search_by_bow_rig_batch): voc = the
        ORBVocabulary whose transform_rig_extracted(exL, lf, exR, rf, B, levelsup) ran last; pair p = rig frame frames[p] of that transform against the
        ResidentKeyFrame kfs[p] (rig or one camera), mps[p] = uint8 flags "feature of kfs[p] has a good map point".  Returns [(nmatches, assigned)]
        with assigned[j] = key-frame feature whose map point goes to vpMapPointMatches[j] or -1: Nleft + Nright entries when n_frame[b] gives them
        per frame, else the whole row of 2 x max_keypoints.
        resident_map, rows (mps = None): the flags are read on the device from rows[p], the row of kfs[p] in the ResidentMap, as SearchByBoWFramesBatch
        (orbm_search_by_bow_rig_batch_map)."""
        P = len(kfs)
        fr = np.ascontiguousarray(frames, np.int32)
        S = 2 * exL.max_keypoints()
        p1 = _ptrs(k._kf for k in kfs)
        outs = [np.full(S, -1, np.int32) for _ in range(P)]
        po = _ptrs(o.ctypes.data for o in outs); nm = np.zeros(max(P, 1), np.int32)

        def search(entry, *flags):                   # the two entry points differ in their flag arguments alone
            exL._lib.check(entry(exL._h, int(lf), exR._h, int(rf), int(getattr(voc, "_rig_B", 0)), voc._v, P, fr.ctypes.data, p1, *flags, self.mfNNratio,
                                 int(self.mbCheckOrientation), po, nm.ctypes.data))
        if resident_map is not None or rows is not None:
            if resident_map is None or rows is None or mps is not None:
                raise ValueError("the map-fed form takes resident_map and rows, and mps = None")
            r = np.ascontiguousarray(rows, np.int32)
            assert len(fr) == P and len(r) == P
            search(exL._lib.L.orbm_search_by_bow_rig_batch_map, resident_map._m, r.ctypes.data)
        else:
            assert len(fr) == P and len(mps) == P
            a1, q1 = _flag_ptrs(mps, P)
            search(exL._lib.L.orbm_search_by_bow_rig_batch, q1)
        return [(int(nm[p]), outs[p] if n_frame is None else outs[p][:int(n_frame[fr[p]])]) for p in range(P)]

    def SearchByBoWFisheye(self, ext, kf, frame, nleft):
        """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) for a fisheye-rig frame (F.Nleft = nleft != -1), src/ORBmatcher.cc:259-493.
        Both views list all features by index (camera 1 first).  Returns (nmatches, assigned[N_frame] = key-frame feature or -1)."""
        a2 = np.full(max(frame.view.N, 1), -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_bow_fisheye(ext._h, kf.ref(), frame.ref(), int(nleft), self.mfNNratio, int(self.mbCheckOrientation),
                                                           a2.ctypes.data, C.byref(nm)))
        return nm.value, a2[:frame.view.N]

    def SearchForInitialization(self, ext, f1, f2, vbPrevMatched, windowSize=10):
        """ORBmatcher::SearchForInitialization, src/ORBmatcher.cc:734.  vbPrevMatched [N1,2] float32 is updated in place.
        Returns (nmatches, vnMatches12)."""
        assert vbPrevMatched.dtype == np.float32 and vbPrevMatched.flags["C_CONTIGUOUS"]
        m12 = np.full(f1.view.N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_for_initialization(ext._h, f1.ref(), f2.ref(), vbPrevMatched.ctypes.data, int(windowSize), self.mfNNratio,
                                                               int(self.mbCheckOrientation), m12.ctypes.data, C.byref(nm)))
        return nm.value, m12

    def SearchByProjectionFisheye(self, ext, frame2, map_points, map_points_r, th=1.0, bFarPoints=False, thFarPoints=50.0):
        """SearchByProjection(Frame&, vector<MapPoint*>&, ...) for a two-camera frame (Nleft != -1), src/ORBmatcher.cc:45-239.
        frame2: views.fisheye_frame_view; map_points_r: views.map_point_right_view.  Returns (nmatches, assigned[Nleft + Nright])."""
        N = frame2.view.left.N + frame2.view.right.N
        assigned = np.full(N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_mappoints_fisheye(ext._h, frame2.ref(), map_points.ref(), map_points_r.ref(), float(th),
                                                                            int(bFarPoints), float(thFarPoints), self.mfNNratio, assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def SearchByProjectionFrameFisheye(self, ext, cur2, last, proj_ur, proj_vr, th, bForward=False, bBackward=False):
        """SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) for a two-camera current frame, src/ORBmatcher.cc:1950-2184."""
        N = cur2.view.left.N + cur2.view.right.N
        ur = np.ascontiguousarray(proj_ur, np.float32); vr = np.ascontiguousarray(proj_vr, np.float32)
        assigned = np.full(N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_frame_fisheye(ext._h, cur2.ref(), last.ref(), ur.ctypes.data, vr.ctypes.data, float(th),
                                                                        int(bForward), int(bBackward), int(self.mbCheckOrientation), assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def SearchByProjectionSim3(self, ext, kf, points, th, ratioHamming=1.0):
        """ORBmatcher::SearchByProjection(KeyFrame*, Sim3f&, vpPoints, [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratioHamming),
        src/ORBmatcher.cc:495 and :608.  kf: views.frame_view with occupied = (vpMatched[idx] != NULL); points:
        views.projected_point_view.  Returns (nmatches, assigned[N]) with assigned[idx] = index of the point put in vpMatched[idx]."""
        assigned = np.full(kf.view.N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_sim3(ext._h, kf.ref(), points.ref(), float(th), float(ratioHamming),
                                                               assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def SearchByProjectionKeyFrame(self, ext, cur, points, th, ORBdist):
        """ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:2196.
        cur.occupied = (CurrentFrame.mvpMapPoints[i] != NULL).  Returns (nmatches, assigned[N]) (-2: reset by the rotation check)."""
        assigned = np.full(cur.view.N, -1, np.int32); nm = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_projection_keyframe(ext._h, cur.ref(), points.ref(), float(th), int(ORBdist),
                                                                   int(self.mbCheckOrientation), assigned.ctypes.data, C.byref(nm)))
        return nm.value, assigned

    def FuseCandidates(self, ext, kf, points, th, invLevelSigma2=None):
        """Candidate search of both ORBmatcher::Fuse overloads (src/ORBmatcher.cc:1325 with the chi-square gate when invLevelSigma2 is
        given, :1543 without).  Returns (bestIdx[M], bestDist[M]); -1 where the reference would not fuse."""
        M = points.view.M
        bi = np.full(M, -1, np.int32); bd = np.full(M, -1, np.int32)
        s2 = None if invLevelSigma2 is None else np.ascontiguousarray(invLevelSigma2, np.float32)
        ext._lib.check(ext._lib.L.orbm_fuse_candidates(ext._h, kf.ref(), points.ref(), float(th), int(s2 is not None),
                                                     None if s2 is None else s2.ctypes.data, bi.ctypes.data, bd.ctypes.data))
        return bi, bd

    @staticmethod
    def FuseCandidatesBatch(ext, kfs, specs, points, th, invLevelSigma2=None, skip=None):
        """The candidate search of ORBmatcher::Fuse for one resident point set against K resident key frames in one call (orbm_fuse_candidates_batch).
        kfs[k] = ResidentKeyFrame of target k (one camera), specs[k] = fuse_spec(...) of that key frame, points = ResidentPoints; invLevelSigma2 = one
        array for every target or a list of K arrays (pKF->mvInvLevelSigma2): given, the chi-square gate of Fuse(pKF, vpMapPoints, th) runs, None = the Sim3
        overload; skip = [K, M] uint8, pairs the caller already excludes.  Returns (best_idx, best_dist) as [K, M] int32 arrays, -1 where the reference
        would not fuse."""
        K, Mp = len(kfs), points.M
        assert len(specs) == K
        T = (FuseTarget * max(K, 1))()
        if invLevelSigma2 is None:
            s2 = [None] * K
        elif isinstance(invLevelSigma2, (list, tuple)) and len(invLevelSigma2) == K and np.ndim(invLevelSigma2[0]) == 1:
            s2 = [np.ascontiguousarray(a, np.float32) for a in invLevelSigma2]
        else:
            s2 = [np.ascontiguousarray(invLevelSigma2, np.float32)] * K
        for k in range(K):
            T[k].kf = kfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]
            T[k].inv_level_sigma2 = None if s2[k] is None else s2[k].ctypes.data
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert sk is None or sk.shape == (K, Mp)
        bi = np.full((K, Mp), -1, np.int32); bd = np.full((K, Mp), -1, np.int32)
        ext._lib.check(ext._lib.L.orbm_fuse_candidates_batch(ext._h, K, T, points._p, None if sk is None else sk.ctypes.data, float(th), int(invLevelSigma2 is not None),
                                                           bi.ctypes.data, bd.ctypes.data))
        return bi, bd

    @staticmethod
    def SearchByProjectionSim3Batch(ext, kfs, specs, points, th, ratio_hamming=1.0, occupied=None, skip=None):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratioHamming) for one resident point set searched
        from K resident key frames in one call (orbm_search_by_projection_sim3_batch).  kfs[k] = ResidentKeyFrame of target k, specs[k] = sim3_spec(...) of its
        Sim3, points = ResidentPoints; occupied = None or K arrays (or None) of kfs[k].N uint8, vpMatched[idx] != NULL on entry; skip = [K, M] uint8, pairs the
        caller excludes (isBad, spAlreadyFound).  Returns (assigned [K, cap], nmatches [K]), cap = the largest N: assigned[k, idx] = the point written to
        vpMatched[idx] of target k, -1 untouched and beyond kfs[k].N."""
        K, Mp = len(kfs), points.M
        assert len(specs) == K and (occupied is None or len(occupied) == K)
        cap = max([kf.N for kf in kfs] + [0])
        T = (Sim3Target * max(K, 1))()
        occ = [None if occupied is None or o is None else np.ascontiguousarray(o, np.uint8) for o in (occupied if occupied is not None else [None] * K)]
        for k in range(K):
            assert occ[k] is None or occ[k].shape == (kfs[k].N,)
            T[k].kf = kfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]
            T[k].occupied = None if occ[k] is None else occ[k].ctypes.data
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert sk is None or sk.shape == (K, Mp)
        assigned = np.full((K, cap), -1, np.int32); nm = np.zeros(max(K, 1), np.int32)
        ext._lib.check(ext._lib.L.orbm_search_by_projection_sim3_batch(ext._h, K, T, points._p, None if sk is None else sk.ctypes.data, float(th), float(ratio_hamming),
                                                                     cap, assigned.ctypes.data, nm.ctypes.data))
        return assigned, nm[:K]

    @staticmethod
    def FuseCandidatesBatchMap(ext, kfs, specs, resident_map, set, rows, th, invLevelSigma2=None, feat0=None, want_kf_slot=False):
        """FuseCandidatesBatch on set `set` of a ResidentMap (orbm_fuse_candidates_batch_map): the pairs `pMP->isBad() || pMP->IsInKeyFrame(pKF)` excludes
        are found on the device from row rows[k] of target k and the slots' states at the moment of the call.  feat0 = None or K row entries of the
        targets' feature 0 (NLeft for a rig's right camera).  Returns (best_idx, best_dist) as [K, M] int32 arrays and, with want_kf_slot, kf_slot [K, M]:
        pKF->GetMapPoint(bestIdx) as a slot, -2 for a bad point, -1 for none."""
        K, Mp = len(kfs), resident_map.set(set, ext).M
        assert len(specs) == K and len(rows) == K and (feat0 is None or len(feat0) == K)
        T = (FuseTarget * max(K, 1))()
        if invLevelSigma2 is None:
            s2 = [None] * K
        elif isinstance(invLevelSigma2, (list, tuple)) and len(invLevelSigma2) == K and np.ndim(invLevelSigma2[0]) == 1:
            s2 = [np.ascontiguousarray(a, np.float32) for a in invLevelSigma2]
        else:
            s2 = [np.ascontiguousarray(invLevelSigma2, np.float32)] * K
        for k in range(K):
            T[k].kf = kfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]
            T[k].inv_level_sigma2 = None if s2[k] is None else s2[k].ctypes.data
        r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1), np.int32) if K else np.zeros(1, np.int32)
        f0 = None if feat0 is None else np.ascontiguousarray(np.asarray(feat0, np.int32).reshape(-1), np.int32)
        bi = np.full((K, Mp), -1, np.int32); bd = np.full((K, Mp), -1, np.int32); ks = np.full((K, Mp), -1, np.int32) if want_kf_slot else None
        ext._lib.check(ext._lib.L.orbm_fuse_candidates_batch_map(ext._h, K, T, r.ctypes.data, None if f0 is None or K == 0 else f0.ctypes.data, resident_map._m, int(set),
                                                               float(th), int(invLevelSigma2 is not None), bi.ctypes.data, bd.ctypes.data,
                                                               None if ks is None else ks.ctypes.data))
        return (bi, bd, ks) if want_kf_slot else (bi, bd)

    @staticmethod
    def _fuse_targets(kfs, specs, invLevelSigma2):
        """the OrbmFuseTarget table of the pair-list calls (and what keeps its arrays alive), as FuseCandidatesBatch fills it"""
        K = len(kfs)
        assert len(specs) == K
        T = (FuseTarget * max(K, 1))()
        if invLevelSigma2 is None:
            s2 = [None] * K
        elif isinstance(invLevelSigma2, (list, tuple)) and len(invLevelSigma2) == K and np.ndim(invLevelSigma2[0]) == 1:
            s2 = [np.ascontiguousarray(a, np.float32) for a in invLevelSigma2]
        else:
            s2 = [np.ascontiguousarray(invLevelSigma2, np.float32)] * K
        for k in range(K):
            T[k].kf = kfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]
            T[k].inv_level_sigma2 = None if s2[k] is None else s2[k].ctypes.data
        return T, s2

    @staticmethod
    def _fuse_pairs(lib, K, Mp, cap, wanted, call):
        """call(cap, start, pointers) -> rc with a guessed capacity (an eighth of the pairs, at least 1024) unless the caller names one; ORBX_E_CAPACITY with
        start[K] > cap is answered by ONE more call with cap = start[K].  wanted[j]: array j is asked for (None in its place otherwise).  Returns
        (start, *arrays) trimmed to start[K]."""
        start = np.zeros(K + 1, np.int32)
        guess = min(K * Mp, max(1024, K * Mp // 8)) if cap is None else int(cap)
        for attempt in range(2):
            arrays = [np.full(max(guess, 1), -1, np.int32) if w else None for w in wanted]
            rc = call(guess, start, [None if a is None else a.ctypes.data for a in arrays])
            if rc != -4 or attempt == 1 or guess < 0 or int(start[K]) <= guess:      # -4 = ORBX_E_CAPACITY (past a limit of the call: start stays zero, no retry)
                break
            guess = int(start[K])
        lib.check(rc)
        n = int(start[K])
        return (start,) + tuple(None if a is None else a[:n] for a in arrays)

    @staticmethod
    def FuseCandidatesPairsBatch(ext, kfs, specs, points, th, invLevelSigma2=None, skip=None, cap=None, want_dist=True):
        """FuseCandidatesBatch answered with the matched pairs alone (orbm_fuse_pairs_batch): the pairs with best_idx >= 0, ordered by target, then by
        position.  Returns (start [K + 1], point, feat, dist): target k owns entries start[k] .. start[k + 1] - 1, entry e fuses set position point[e] with
        feature feat[e] at distance dist[e] (None without want_dist).  cap = None: the wrapper guesses a capacity; either way it calls once more with
        start[K] if the list is longer."""
        K, Mp = len(kfs), points.M
        T, keep = ORBmatcher._fuse_targets(kfs, specs, invLevelSigma2)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert sk is None or sk.shape == (K, Mp)
        L = ext._lib.L
        return ORBmatcher._fuse_pairs(ext._lib, K, Mp, cap, (True, True, want_dist), lambda c, start, a: L.orbm_fuse_pairs_batch(
            ext._h, K, T, points._p, None if sk is None else sk.ctypes.data, float(th), int(invLevelSigma2 is not None), c, start.ctypes.data, *a))

    @staticmethod
    def FuseCandidatesPairsBatchMap(ext, kfs, specs, resident_map, set, rows, th, invLevelSigma2=None, feat0=None, cap=None, want_dist=True, want_slots=True):
        """FuseCandidatesBatchMap answered with the matched pairs alone (orbm_fuse_pairs_batch_map).  Returns (start, point, feat, dist, point_slot, kf_slot):
        as FuseCandidatesPairsBatch, with point_slot[e] = the map slot of set position point[e] and kf_slot[e] = pKF->GetMapPoint(feat[e]) as a slot, -2
        for a bad point, -1 for none (both None without want_slots)."""
        K, Mp = len(kfs), resident_map.set(set, ext).M
        assert len(rows) == K and (feat0 is None or len(feat0) == K)
        T, keep = ORBmatcher._fuse_targets(kfs, specs, invLevelSigma2)
        r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1), np.int32) if K else np.zeros(1, np.int32)
        f0 = None if feat0 is None else np.ascontiguousarray(np.asarray(feat0, np.int32).reshape(-1), np.int32)
        L = ext._lib.L
        return ORBmatcher._fuse_pairs(ext._lib, K, Mp, cap, (True, True, want_dist, want_slots, want_slots), lambda c, start, a: L.orbm_fuse_pairs_batch_map(
            ext._h, K, T, r.ctypes.data, None if f0 is None or K == 0 else f0.ctypes.data, resident_map._m, int(set), float(th), int(invLevelSigma2 is not None), c,
            start.ctypes.data, *a))

    @staticmethod
    def SearchByProjectionSim3BatchMap(ext, kfs, specs, resident_map, set, th, ratio_hamming=1.0, occupied=None, found=None, want_slots=False):
        """SearchByProjectionSim3Batch on set `set` of a ResidentMap (orbm_search_by_projection_sim3_batch_map): a point is skipped for target k iff its
        slot is bad at the moment of the call or listed in found[k] (spAlreadyFound as slots; found = None or K arrays, duplicates / -1 / slots outside the
        set are fine).  Returns (assigned [K, cap], nmatches [K]) and, with want_slots, assigned_slot [K, cap]: the map slot of every assigned point."""
        K, Mp = len(kfs), resident_map.set(set, ext).M
        assert len(specs) == K and (occupied is None or len(occupied) == K) and (found is None or len(found) == K)
        cap = max([kf.N for kf in kfs] + [0])
        T = (Sim3Target * max(K, 1))()
        occ = [None if occupied is None or o is None else np.ascontiguousarray(o, np.uint8) for o in (occupied if occupied is not None else [None] * K)]
        for k in range(K):
            assert occ[k] is None or occ[k].shape == (kfs[k].N,)
            T[k].kf = kfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]
            T[k].occupied = None if occ[k] is None else occ[k].ctypes.data
        fs = fl = None
        if found is not None:
            lists = [np.zeros(0, np.int32) if a is None else np.asarray(a, np.int32).reshape(-1) for a in found]
            fs = np.cumsum([0] + [len(a) for a in lists]).astype(np.int32)
            fl = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]), np.int32)
        assigned = np.full((K, cap), -1, np.int32); nm = np.zeros(max(K, 1), np.int32); aslot = np.full((K, cap), -1, np.int32) if want_slots else None
        ext._lib.check(ext._lib.L.orbm_search_by_projection_sim3_batch_map(ext._h, K, T, resident_map._m, int(set), None if fs is None else fs.ctypes.data,
                                                                         None if fl is None else fl.ctypes.data, float(th), float(ratio_hamming), cap,
                                                                         assigned.ctypes.data, nm.ctypes.data, None if aslot is None else aslot.ctypes.data))
        return (assigned, nm[:K], aslot) if want_slots else (assigned, nm[:K])

    def SearchBySim3(self, ext, kf1, kf2, p1in2, p2in1, th):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th), src/ORBmatcher.cc:1689.  Returns (nFound, matches12[N1])."""
        m12 = np.full(kf1.view.N, -1, np.int32); nf = C.c_int()
        ext._lib.check(ext._lib.L.orbm_search_by_sim3(ext._h, kf1.ref(), kf2.ref(), p1in2.ref(), p2in1.ref(), float(th), m12.ctypes.data, C.byref(nf)))
        return nf.value, m12

    @staticmethod
    def DescriptorDistance(ext, a, b):
        """All-pairs Hamming distance matrix [len(a), len(b)] of 32-byte descriptors, computed on `ext`'s GPU."""
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32); b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        out = np.zeros((len(a), len(b)), np.int32)
        ext._lib.check(ext._lib.L.orbm_hamming_matrix(ext._h, a.ctypes.data, len(a), b.ctypes.data, len(b), out.ctypes.data))
        return out


class ResidentKeyFrame:
    """orbm_keyframe: the parts of a key frame / frame the vocabulary-bucket searches read (keys, descriptors, mvuRight, mFeatVec), uploaded
    once from a views.key_frame_view.  Usable with every extractor handle of the same device."""

    def __init__(self, ext, kf_view):
        self._lib = ext._lib; self.N = kf_view.view.N
        h = C.c_void_p()
        self._lib.check(self._lib.L.orbm_keyframe_create(ext._h, kf_view.ref(), C.byref(h)))
        self._kf = h

    @classmethod
    def _adopt(cls, lib, handle, ext):
        kf = cls.__new__(cls)
        kf._lib = lib; kf._kf = C.c_void_p(handle)
        n = C.c_int()
        try:
            lib.check(lib.L.orbm_keyframe_fetch(ext._h, kf._kf, C.byref(n), None, None, None, None, None, None, None, None))
        except Exception:
            kf.close()
            raise
        kf.N = n.value
        return kf

    @classmethod
    def from_extracted(cls, ext, voc, frames, use_u_right=False):
        """orbm_keyframe_create_extracted: resident key frames made on the device from images `frames` of ext's last extraction - mvKeysUn, descriptor rows,
        mvuRight of the last stereo matcher / depth call (use_u_right; else -1) and the FeatureVector where the last voc.transform_extracted left it
        (voc = None: key frames without a FeatureVector).  Returns a list, one object per entry of `frames`."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        out = (C.c_void_p * max(len(fr), 1))()
        ext._lib.check(ext._lib.L.orbm_keyframe_create_extracted(ext._h, voc._v if voc is not None else None, len(fr), fr.ctypes.data, int(bool(use_u_right)), out))
        return cls._adopt_all(ext, out, len(fr))

    @classmethod
    def from_rig_extracted(cls, exL, lf, exR, rf, voc, frames):
        """orbm_keyframe_create_rig_extracted: rig key frames (mvKeys followed by mvKeysRight, the joined rows, no mvuRight) of rig frames `frames` of the
        last voc.transform_rig_extracted(exL, lf, exR, rf, B, levelsup).  Returns a list."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        out = (C.c_void_p * max(len(fr), 1))()
        exL._lib.check(exL._lib.L.orbm_keyframe_create_rig_extracted(exL._h, int(lf), exR._h, int(rf), voc._v if voc is not None else None, len(fr), fr.ctypes.data, out))
        return cls._adopt_all(exL, out, len(fr))

    @classmethod
    def _adopt_all(cls, ext, out, n):
        kfs = []
        try:
            for j in range(n):
                kfs.append(cls._adopt(ext._lib, out[j], ext))
        except Exception:
            for j in range(len(kfs) + 1, n):
                ext._lib.L.orbm_keyframe_destroy(C.c_void_p(out[j]))
            raise
        return kfs

    def fetch(self, ext):
        """orbm_keyframe_fetch: dict of numpy arrays - keys_un [N] (views.KP_DTYPE), desc [N, 32], u_right [N], fv_node [nodes], fv_start [nodes + 1],
        fv_feat [fv_start[-1]], node_of_feat [N]."""
        from .views import KP_DTYPE
        L = self._lib
        n, nn = C.c_int(), C.c_int()
        L.check(L.L.orbm_keyframe_fetch(ext._h, self._kf, C.byref(n), C.byref(nn), None, None, None, None, None, None, None))
        N, nodes = n.value, nn.value
        r = dict(keys_un=np.zeros(N, KP_DTYPE), desc=np.zeros((N, 32), np.uint8), u_right=np.zeros(N, np.float32), fv_node=np.zeros(nodes, np.uint32),
                 fv_start=np.zeros(nodes + 1, np.int32), node_of_feat=np.zeros(N, np.int32))
        L.check(L.L.orbm_keyframe_fetch(ext._h, self._kf, None, None, r["keys_un"].ctypes.data, r["desc"].ctypes.data, r["u_right"].ctypes.data, r["fv_node"].ctypes.data,
                                        r["fv_start"].ctypes.data, None, r["node_of_feat"].ctypes.data))
        r["fv_feat"] = np.zeros(int(r["fv_start"][nodes]), np.uint32)
        L.check(L.L.orbm_keyframe_fetch(ext._h, self._kf, None, None, None, None, None, None, None, r["fv_feat"].ctypes.data, None))
        return r

    def close(self):
        if self._kf:
            self._lib.L.orbm_keyframe_destroy(self._kf); self._kf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ComputeStereoMatches(left, right, bf, b, left_first=0, right_first=0, B=None):
    """Frame::ComputeStereoMatches on the last batches of two extractors (or two halves of one).
    Returns (mvuRight [B,cap], mvDepth [B,cap], n_matches [B]); rows beyond each image's N are -1."""
    B = B or min(left._B - left_first, right._B - right_first)
    L = left._lib
    L.check(L.L.orbm_stereo_match(left._h, left_first, right._h, right_first, B, float(bf), float(b)))
    cap = left.max_keypoints()
    u = np.zeros((B, cap), np.float32); d = np.zeros((B, cap), np.float32); n = np.zeros(B, np.int32)
    L.check(L.L.orbm_stereo_fetch(left._h, B, u.ctypes.data, d.ctypes.data, cap, n.ctypes.data))
    return u, d, n


def StereoFishEyeKnn(left, right, left_first=0, right_first=0, B=None):
    """BFMatcher(NORM_HAMMING).knnMatch(k=2) of left[monoLeft:] vs right[monoRight:] + Lowe ratio 0.7.
    Returns dict of [B,cap] arrays idx0, dist0, idx1, dist1, ratio_ok (rows beyond the query count are -1/0)."""
    B = B or min(left._B - left_first, right._B - right_first)
    L = left._lib
    L.check(L.L.orbm_knn2(left._h, left_first, right._h, right_first, B))
    cap = left.max_keypoints()
    out = {k: np.zeros((B, cap), np.int32) for k in ("idx0", "dist0", "idx1", "dist1")}
    out["ratio_ok"] = np.zeros((B, cap), np.uint8)
    L.check(L.L.orbm_knn2_fetch(left._h, B, out["idx0"].ctypes.data, out["dist0"].ctypes.data, out["idx1"].ctypes.data,
                                out["dist1"].ctypes.data, out["ratio_ok"].ctypes.data, cap))
    return out


class KB8Stereo(C.Structure):
    """OrbmKB8Stereo (include/orbx.h): the two cameras' Kannala-Brandt parameters, Frame::mRlr (row-major), mtlr"""
    _fields_ = [("cam1", C.c_float * 8), ("cam2", C.c_float * 8), ("R12", C.c_float * 9), ("t12", C.c_float * 3)]


def ComputeStereoFishEyeMatches(left, right, cam1, cam2, R12, t12, left_first=0, right_first=0, B=None):
    """Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1530-1587) for B fisheye pairs extracted with the cameras' lapping areas: 2-NN + ratio
    test, then KannalaBrandt8::TriangulateMatches on the device.  cam1 / cam2 = the 8 Kannala-Brandt parameters, (R12, t12) = mRlr, mtlr.
    Returns dict(l2r [B,cap], r2l [B,cap], depth [B,cap], p3d [B,cap,3], n [B])."""
    B = B or min(left._B - left_first, right._B - right_first)
    c = KB8Stereo()
    c.cam1[:] = [float(v) for v in cam1]; c.cam2[:] = [float(v) for v in cam2]
    c.R12[:] = [float(v) for v in np.asarray(R12, np.float32).ravel()]; c.t12[:] = [float(v) for v in np.asarray(t12, np.float32).ravel()]
    L = left._lib
    L.check(L.L.orbm_stereo_fisheye(left._h, left_first, right._h, right_first, B, C.byref(c)))
    cap = left.max_keypoints()
    out = dict(l2r=np.zeros((B, cap), np.int32), r2l=np.zeros((B, cap), np.int32), depth=np.zeros((B, cap), np.float32),
               p3d=np.zeros((B, cap, 3), np.float32), n=np.zeros(B, np.int32))
    L.check(L.L.orbm_stereo_fisheye_fetch(left._h, B, out["l2r"].ctypes.data, out["r2l"].ctypes.data, out["depth"].ctypes.data, out["p3d"].ctypes.data,
                                          out["n"].ctypes.data, cap))
    return out


class _FrustumView(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("qcw", C.c_float * 4), ("camera_type", C.c_int), ("cam", C.c_float * 8),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("mbf", C.c_float), ("log_scale_factor", C.c_float),
                ("nlevels", C.c_int), ("scale_factors", C.c_void_p)]


class _WorldPointView(C.Structure):
    _fields_ = [("M", C.c_int), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("is_bad", C.c_void_p),
                ("has_obs", C.c_void_p), ("desc", C.c_void_p)]


class _TrackOut(C.Structure):
    _fields_ = [("in_view", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p), ("depth", C.c_void_p), ("view_cos", C.c_void_p),
                ("scale_level", C.c_void_p)]


class _FrustumRigView(C.Structure):
    _fields_ = [("left", _FrustumView), ("Rrl", C.c_float * 9), ("trl", C.c_float * 3), ("tlr", C.c_float * 3), ("Rwc", C.c_float * 9), ("camera2_type", C.c_int),
                ("cam2", C.c_float * 8)]


class _TrackOutRight(C.Structure):
    _fields_ = [("in_view_r", C.c_void_p), ("proj_xr", C.c_void_p), ("proj_yr", C.c_void_p), ("depth_r", C.c_void_p), ("view_cos_r", C.c_void_p), ("scale_level_r", C.c_void_p)]


def rig_frustum_view(pose, cam1, cam2, bounds, scale_factors, into=None):
    """OrbmFrustumRigView of one rig frame: pose = dict(Rcw, tcw, Ow, Rwc, Rrl, trl, tlr) exactly as the Frame holds them (camera 1 takes Rcw / tcw /
    Ow untouched; camera 2 is derived on the device), cam1 / cam2 = the two cameras' parameters.  Returns (view, the float32 scale-factor array the
    view points into - keep it alive)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    sf = f32(scale_factors)
    V = into if into is not None else _FrustumRigView()
    frustum_view(SE3f(), None, cam1, bounds, 0.0, sf, into=V.left)
    V.left.Rcw[:] = f32(pose["Rcw"]).ravel().tolist(); V.left.tcw[:] = f32(pose["tcw"]).tolist()       # the Frame's own members, untouched
    V.left.Ow[:] = [float(v) for v in f32(pose["Ow"])]
    V.left.scale_factors = sf.ctypes.data
    V.Rrl[:] = f32(pose["Rrl"]).ravel().tolist(); V.trl[:] = f32(pose["trl"]).tolist(); V.tlr[:] = f32(pose["tlr"]).tolist(); V.Rwc[:] = f32(pose["Rwc"]).ravel().tolist()
    cam2 = [float(v) for v in cam2]
    V.camera2_type = 1 if len(cam2) == 8 else 0
    V.cam2[:] = cam2 + [0.0] * (8 - len(cam2))
    return V, sf


def SearchLocalPointsRig(ext, frame2, pose, cam1, cam2, bounds, scale_factors, pos, normal, min_distance, max_distance, is_bad=None, has_obs=None, desc=None,
                         viewing_cos_limit=0.5, th=1.0, far_points=False, th_far=50.0, nnratio=0.8, search=True):
    """Tracking::SearchLocalPoints for a two-camera (fisheye rig) frame: Frame::isInFrustum with Nleft != -1 (src/Frame.cc:754-766 ->
    isInFrustumChecks :1592-1650 per camera) on the device and, with search=True, ORBmatcher::SearchByProjection including its right-camera
    branch (src/ORBmatcher.cc:45-239).  pose = dict(Rcw, tcw, Ow, Rwc, Rrl, trl, tlr) exactly as the Frame holds them; frame2 =
    views.fisheye_frame_view(...) (None with search=False).  Returns (left dict, right dict, assigned [Nleft + Nright] or None, nmatches)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    pos, normal, mn, mx, sf = f32(pos).reshape(-1, 3), f32(normal).reshape(-1, 3), f32(min_distance), f32(max_distance), f32(scale_factors)
    M = len(pos)
    V, sf = rig_frustum_view(pose, cam1, cam2, bounds, sf)
    P = _WorldPointView()
    bad = None if is_bad is None else np.ascontiguousarray(is_bad, np.uint8); obs = None if has_obs is None else np.ascontiguousarray(has_obs, np.uint8)
    d = None if desc is None else np.ascontiguousarray(desc, np.uint8)
    P.M = M; P.pos = pos.ctypes.data; P.normal = normal.ctypes.data; P.min_distance = mn.ctypes.data; P.max_distance = mx.ctypes.data
    P.is_bad = None if bad is None else bad.ctypes.data; P.has_obs = None if obs is None else obs.ctypes.data; P.desc = None if d is None else d.ctypes.data
    M1 = max(M, 1)
    tl = dict(in_view=np.zeros(M1, np.uint8), proj_x=np.zeros(M1, np.float32), proj_y=np.zeros(M1, np.float32), proj_xr=np.zeros(M1, np.float32), depth=np.zeros(M1, np.float32),
              view_cos=np.zeros(M1, np.float32), scale_level=np.zeros(M1, np.int32))
    tr = dict(in_view_r=np.zeros(M1, np.uint8), proj_xr=np.zeros(M1, np.float32), proj_yr=np.zeros(M1, np.float32), depth_r=np.zeros(M1, np.float32),
              view_cos_r=np.zeros(M1, np.float32), scale_level_r=np.zeros(M1, np.int32))
    TL = _TrackOut(*[tl[k].ctypes.data for k in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "scale_level")])
    TR = _TrackOutRight(*[tr[k].ctypes.data for k in ("in_view_r", "proj_xr", "proj_yr", "depth_r", "view_cos_r", "scale_level_r")])
    L = ext._lib
    cut = lambda dct: {k: v[:M] for k, v in dct.items()}
    if not search:
        L.check(L.L.orbm_is_in_frustum_rig(ext._h, C.byref(V), C.byref(P), float(viewing_cos_limit), C.byref(TL), C.byref(TR)))
        return cut(tl), cut(tr), None, 0
    N = frame2.view.left.N + frame2.view.right.N
    assigned = np.full(max(N, 1), -1, np.int32); n = C.c_int(0)
    L.check(L.L.orbm_search_local_points_fisheye(ext._h, frame2.ref(), C.byref(V), C.byref(P), float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio),
                                                 C.byref(TL), C.byref(TR), assigned.ctypes.data, C.byref(n)))
    return cut(tl), cut(tr), assigned[:N], n.value


class _ProjectIn(C.Structure):
    _fields_ = [("M", C.c_int), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_inv", C.c_void_p), ("max_inv", C.c_void_p), ("skip", C.c_void_p)]


class _ProjectOut(C.Structure):
    _fields_ = [("valid", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("ur", C.c_void_p), ("inv_z", C.c_void_p), ("dist", C.c_void_p)]


def projection_spec(pose, cam, bounds, Ow=None, second=None, depth_test=1, bounds_mode=0, inline_pinhole=False, dist_mode=0, distance_test=False, angle_test=False, bf=0.0):
    """OrbmProjection (views.Projection) from a pose (sophus.SE3f or (R, t)), the camera's 4 or 8 parameters and the image bounds; the arguments as ProjectPoints."""
    S = _Projection()
    T = as_se3(pose)
    S.q[:] = [float(v) for v in T.unit_quaternion()]; S.t[:] = [float(v) for v in T.translation()]
    if isinstance(second, Sim3f):
        S.second = 1; S.q2[:] = [float(v) for v in second.quaternion()]; S.t2[:] = [float(v) for v in second.translation()]; S.s2 = float(second.scale())
    elif second is not None:
        X = as_se3(second)
        S.second = 2; S.q2[:] = [float(v) for v in X.unit_quaternion()]; S.t2[:] = [float(v) for v in X.translation()]; S.s2 = 1.0
    if Ow is not None:
        S.Ow[:] = np.ascontiguousarray(Ow, np.float32).tolist()
    cam = [float(v) for v in cam]
    S.camera_type = 1 if len(cam) == 8 else 0; S.cam[:] = cam + [0.0] * (8 - len(cam)); S.inline_pinhole = int(inline_pinhole)
    S.min_x, S.max_x, S.min_y, S.max_y = [float(v) for v in bounds]
    S.dist_mode, S.depth_test, S.bounds_mode, S.angle_test, S.bf = int(dist_mode), int(depth_test), int(bounds_mode), int(angle_test), float(bf)
    S.distance_test = int(bool(distance_test))
    return S


def fuse_spec(pose, cam, bounds, bf, log_scale_factor, Ow=None):
    """What ORBmatcher::Fuse projects with into one key frame, as FuseCandidatesBatch takes it: (OrbmProjection, mfLogScaleFactor).  pose = pKF->GetPose() (or
    the rigid part of Scw), Ow = pKF->GetCameraCenter() (default: pose.inverse().translation()), bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), KeyFrame::IsInImage,
    depth, distance-range and viewing-angle tests on, ur = u - bf / z."""
    T = as_se3(pose)
    Ow = T.inverse().translation() if Ow is None else Ow
    return projection_spec(T, cam, bounds, Ow, depth_test=1, bounds_mode=1, distance_test=True, angle_test=True, bf=bf), float(log_scale_factor)


def sim3_spec(pose, cam, bounds, log_scale_factor, Ow=None, inline_pinhole=False):
    """What ORBmatcher::SearchByProjection(pKF, Scw, ...) projects with, as SearchByProjectionSim3Batch takes it: (OrbmProjection, mfLogScaleFactor).  pose = the
    rigid part [R | t / s] of Scw, Ow = its inverse's translation (the default), bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), KeyFrame::IsInImage, depth,
    distance-range and viewing-angle tests on, bf = 0; inline_pinhole: the overload that also returns the points' key frames (src/ORBmatcher.cc:656-660)."""
    T = as_se3(pose)
    Ow = T.inverse().translation() if Ow is None else Ow
    return projection_spec(T, cam, bounds, Ow, depth_test=1, bounds_mode=1, inline_pinhole=inline_pinhole, distance_test=True, angle_test=True, bf=0.0), float(log_scale_factor)


def ProjectPoints(ext, pose, cam, bounds, pos, normal=None, min_inv=None, max_inv=None, skip=None, Ow=None, second=None, depth_test=1, bounds_mode=0, inline_pinhole=False,
                  dist_mode=0, angle_test=False, bf=0.0):
    """orbm_project_points: the geometry in front of the projection-type searches (transform, depth test, projection, image test, distance
    range, viewing angle) for M map points on the device.  pose = sophus.SE3f (or (R, t), taken through the SE3(R, t) constructor): the device
    evaluates `pose * p` as Sophus does, on the unit quaternion.  second = a sophus.Sim3f (SearchBySim3's S21 / S12) or SE3f (the rig's Trl)
    applied behind the pose.  Returns dict(valid, u, v, ur, inv_z, dist)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    pos = f32(pos).reshape(-1, 3); M = len(pos)
    S = projection_spec(pose, cam, bounds, Ow, second, depth_test, bounds_mode, inline_pinhole, dist_mode, min_inv is not None and max_inv is not None, angle_test, bf)
    keep = [pos] + [None if a is None else (f32(a) if i < 3 else np.ascontiguousarray(a, np.uint8)) for i, a in enumerate((normal, min_inv, max_inv, skip))]
    ptr = lambda a: None if a is None else a.ctypes.data
    I = _ProjectIn(M, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]))
    M1 = max(M, 1)
    out = dict(valid=np.zeros(M1, np.uint8), u=np.zeros(M1, np.float32), v=np.zeros(M1, np.float32), ur=np.zeros(M1, np.float32), inv_z=np.zeros(M1, np.float32),
               dist=np.zeros(M1, np.float32))
    O = _ProjectOut(*[out[k].ctypes.data for k in ("valid", "u", "v", "ur", "inv_z", "dist")])
    ext._lib.check(ext._lib.L.orbm_project_points(ext._h, C.byref(S), C.byref(I), C.byref(O)))
    return {k: v[:M] for k, v in out.items()}


class _LastFrameBatch(C.Structure):
    _fields_ = [("cap_last", C.c_int), ("n", C.c_void_p), ("pos", C.c_void_p), ("valid", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p), ("has_obs", C.c_void_p),
                ("desc", C.c_void_p)]


class LastFrameBatch:
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a batch of frames on the device
    (orbm_search_by_projection_lastframe_batch): current frames = images [first, first + B) of ext's last extraction; per frame the map points
    of its last frame.  enqueue() is asynchronous, fetch() returns (assigned [B, cap], nmatches [B])."""

    def __init__(self, ext, B, cam, bounds, mbf, scale_factors):
        self.ext, self.B = ext, B
        self.cam, self.bounds, self.mbf = cam, bounds, mbf
        self.sf = np.ascontiguousarray(scale_factors, np.float32)
        self.views = (_FrustumView * B)()
        self.cap = ext.max_keypoints()
        self.assigned = np.full((B, self.cap), -1, np.int32); self.nm = np.zeros(B, np.int32)

    def set_poses(self, poses):
        for b, pose in enumerate(poses):
            frustum_view(as_se3(pose), None, self.cam, self.bounds, self.mbf, self.sf, into=self.views[b])
            self.views[b].scale_factors = self.sf.ctypes.data

    def enqueue(self, n, pos, valid, octave, angle, has_obs, desc, th, forward=None, backward=None, check_orientation=True, occupied=None, use_u_right=True, first=0):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        self._again = lambda: self.enqueue(n, pos, valid, octave, angle, has_obs, desc, th, forward, backward, check_orientation, occupied, use_u_right, first)
        pos = f32(pos); capL = pos.shape[1]
        self._keep = (np.ascontiguousarray(n, np.int32), pos, u8(valid), np.ascontiguousarray(octave, np.int32), f32(angle), u8(has_obs), u8(desc), u8(forward), u8(backward), u8(occupied))
        k = self._keep
        ptr = lambda a: None if a is None else a.ctypes.data
        lb = _LastFrameBatch(capL, ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(k[3]), ptr(k[4]), ptr(k[5]), ptr(k[6]))
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_lastframe_batch(self.ext._h, int(first), self.B, self.views, C.byref(lb), float(th), ptr(k[7]), ptr(k[8]), int(bool(check_orientation)),
                                                              ptr(k[9]), int(bool(use_u_right))))

    def enqueue_slots(self, resident_map, n, slots, outlier, octave, angle, has_obs, th, forward=None, backward=None, check_orientation=True, occupied=None, use_u_right=True,
                      first=0):
        """The same search with the last frame's map points named by slot of a ResidentMap (orbm_search_by_projection_lastframe_batch_map): slots
        [B, cap_last] (-1 = no map point), outlier [B, cap_last] or None; position and descriptor are gathered from the map on the device (a slot's bad
        flag is not read).  octave, angle, has_obs and everything else as enqueue()."""
        self._again = lambda: self.enqueue_slots(resident_map, n, slots, outlier, octave, angle, has_obs, th, forward, backward, check_orientation, occupied, use_u_right, first)
        lb, k = _last_frame_slots(n, slots, outlier, octave, angle, has_obs, forward, backward, occupied)
        self._keep = k
        ptr = lambda a: None if a is None else a.ctypes.data
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_lastframe_batch_map(self.ext._h, int(first), self.B, self.views, resident_map._m, C.byref(lb), float(th), ptr(k[6]), ptr(k[7]),
                                                                  int(bool(check_orientation)), ptr(k[8]), int(bool(use_u_right))))

    def fetch(self):
        L = self.ext._lib
        rc = L.L.orbm_search_local_points_fetch(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, None)
        if rc == -4:                 # ORBX_E_CAPACITY: pool enlarged, run the batch again
            self._again()
            rc = L.L.orbm_search_local_points_fetch(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, None)
        L.check(rc)
        return self.assigned, self.nm


class _LastFrameSlots(C.Structure):
    _fields_ = [("cap_last", C.c_int), ("n", C.c_void_p), ("slots", C.c_void_p), ("outlier", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p), ("has_obs", C.c_void_p)]


class _KeyFrameRows(C.Structure):
    _fields_ = [("row", C.c_void_p), ("kfs", C.c_void_p), ("cap_found", C.c_int), ("found", C.c_void_p)]


def _last_frame_slots(n, slots, outlier, octave, angle, has_obs, forward, backward, occupied):
    """(OrbmLastFrameSlots, the arrays it points into followed by forward, backward, occupied)"""
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data
    slots = np.ascontiguousarray(slots, np.int32)
    k = (np.ascontiguousarray(n, np.int32), slots, u8(outlier), np.ascontiguousarray(octave, np.int32), np.ascontiguousarray(angle, np.float32), u8(has_obs), u8(forward), u8(backward),
         u8(occupied))
    return _LastFrameSlots(slots.shape[1], ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(k[3]), ptr(k[4]), ptr(k[5])), k


class _KeyFramePointBatch(C.Structure):
    _fields_ = [("cap_kf", C.c_int), ("n", C.c_void_p), ("pos", C.c_void_p), ("valid", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p),
                ("angle", C.c_void_p), ("desc", C.c_void_p)]


class KeyFrameBatch(LastFrameBatch):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) - relocalisation - for a batch of frames on the device
    (orbm_search_by_projection_keyframe_batch): current frames = images [first, first + B) of ext's last extraction, per frame the map points of
    its candidate key frame.  set_poses() as LastFrameBatch; enqueue() is asynchronous, fetch() returns (assigned [B, cap], nmatches [B])."""

    def enqueue(self, n, pos, valid, min_distance, max_distance, angle, desc, th, orb_dist, check_orientation=True, occupied=None, first=0):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        self._again = lambda: self.enqueue(n, pos, valid, min_distance, max_distance, angle, desc, th, orb_dist, check_orientation, occupied, first)
        pos = f32(pos); capK = pos.shape[1]
        self._keep = (np.ascontiguousarray(n, np.int32), pos, u8(valid), f32(min_distance), f32(max_distance), f32(angle), u8(desc), u8(occupied))
        k = self._keep
        ptr = lambda a: None if a is None else a.ctypes.data
        kb = _KeyFramePointBatch(capK, ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(k[3]), ptr(k[4]), ptr(k[5]), ptr(k[6]))
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_keyframe_batch(self.ext._h, int(first), self.B, self.views, C.byref(kb), float(th), int(orb_dist), int(bool(check_orientation)), ptr(k[7])))

    def enqueue_rows(self, resident_map, rows, kfs, found, th, orb_dist, check_orientation=True, occupied=None, first=0):
        """The same search with each frame's candidate key frame named by its row in a ResidentMap (orbm_search_by_projection_keyframe_batch_map): rows [B],
        kfs[b] = the same key frame as a ResidentKeyFrame (its keypoint angles are read), found [B, cap_found] uint8 (sAlreadyFound) or None.  Position,
        distance limits and descriptor are gathered from the map on the device; an entry counts iff its slot holds a point that is not bad and is not
        found.  assigned indexes the row."""
        self._again = lambda: self.enqueue_rows(resident_map, rows, kfs, found, th, orb_dist, check_orientation, occupied, first)
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        r, fnd, occ = np.ascontiguousarray(rows, np.int32), u8(found), u8(occupied)
        if len(r) != self.B or len(kfs) != self.B:
            raise ValueError("%d rows and %d key frames for %d frames" % (len(r), len(kfs), self.B))
        pk = (C.c_void_p * self.B)(*[k._kf for k in kfs])
        self._keep = (r, pk, fnd, occ)
        kr = _KeyFrameRows(ptr(r), C.cast(pk, C.c_void_p), 0 if fnd is None else fnd.shape[1], ptr(fnd))
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_keyframe_batch_map(self.ext._h, int(first), self.B, self.views, resident_map._m, C.byref(kr), float(th), int(orb_dist),
                                                                 int(bool(check_orientation)), ptr(occ)))


class ResidentPoints:
    """orbm_points: position, normal, distance limits and descriptor of a set of map points, uploaded once (the local map)."""

    def __init__(self, ext, pos, normal, min_distance, max_distance, desc):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        self._lib = ext._lib
        pos, normal, mn, mx, d = f32(pos).reshape(-1, 3), f32(normal).reshape(-1, 3), f32(min_distance), f32(max_distance), np.ascontiguousarray(desc, np.uint8)
        P = _WorldPointView(); P.M = len(pos)
        P.pos, P.normal, P.min_distance, P.max_distance, P.desc = pos.ctypes.data, normal.ctypes.data, mn.ctypes.data, mx.ctypes.data, d.ctypes.data
        h = C.c_void_p()
        self._lib.check(self._lib.L.orbm_points_create(ext._h, C.byref(P), C.byref(h)))
        self._p, self.M = h, len(pos)

    def close(self):
        if self._p:
            self._lib.L.orbm_points_destroy(self._p); self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def PointsFetch(ext, points):
    """(pos [M, 3], normal [M, 3], min_distance [M], max_distance [M], desc [M, 32]) of any resident point set (orbm_points_fetch)."""
    m = points.M
    pos = np.zeros((m, 3), np.float32); normal = np.zeros((m, 3), np.float32); mn = np.zeros(m, np.float32); mx = np.zeros(m, np.float32); desc = np.zeros((m, 32), np.uint8)
    ext._lib.check(ext._lib.L.orbm_points_fetch(ext._h, points._p, pos.ctypes.data, normal.ctypes.data, mn.ctypes.data, mx.ctypes.data, desc.ctypes.data))
    return pos, normal, mn, mx, desc


class _MapSet:
    """A point set a ResidentMap built: usable wherever a ResidentPoints is (LocalPointsBatch, LocalPointsRigBatch, FuseCandidatesBatch).  It belongs to
    the map: close() does nothing, and it is valid until the map rebuilds that set."""

    def __init__(self, p, M):
        self._p, self.M = C.c_void_p(p), M

    def close(self):
        pass


class _StereoPointsFrame(C.Structure):      # OrbmStereoPointsFrame
    _fields_ = [("frame", C.c_int), ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3), ("keeps", C.c_void_p), ("free_slots", C.c_void_p), ("nfree", C.c_int),
                ("row", C.c_int)]


class ResidentMap:
    """orbm_map: the map on the device.  The fields the searches read live in a store addressed by slot (update / set_bad), the map-point matches of
    key frames are rows of slots (set_keyframe), and local_points builds Tracking::UpdateLocalPoints (src/Tracking.cc:4088-4120) of B frames on the
    device into point sets that set(b) hands to the batched searches.  ext: any extractor on the map's device; every method takes `ext=` to run
    through another handle (LocalMapping's thread updates, Tracking's thread builds)."""

    def __init__(self, ext, slots, kf_rows, kf_row_cap, max_sets):
        self._lib, self._ext = ext._lib, ext
        self.slots, self.kf_rows, self.kf_row_cap, self.max_sets = slots, kf_rows, kf_row_cap, max_sets
        h = C.c_void_p()
        self._lib.check(self._lib.L.orbm_map_create(ext._h, int(slots), int(kf_rows), int(kf_row_cap), int(max_sets), C.byref(h)))
        self._m = h

    def _h(self, ext):
        return (ext or self._ext)._h

    def update(self, slots, pos, normal, min_distance, max_distance, desc, is_bad=None, ext=None):
        """SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors of the points at `slots` (distinct): every field the searches read"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        s = np.ascontiguousarray(slots, np.int32)
        pos, normal, mn, mx, d = f32(pos).reshape(-1, 3), f32(normal).reshape(-1, 3), f32(min_distance), f32(max_distance), np.ascontiguousarray(desc, np.uint8)
        bad = None if is_bad is None else np.ascontiguousarray(is_bad, np.uint8)
        P = _WorldPointView(); P.M = len(pos)
        P.pos, P.normal, P.min_distance, P.max_distance, P.desc = pos.ctypes.data, normal.ctypes.data, mn.ctypes.data, mx.ctypes.data, d.ctypes.data
        P.is_bad = None if bad is None else bad.ctypes.data
        self._lib.check(self._lib.L.orbm_map_update(self._h(ext), self._m, len(s), s.ctypes.data, C.byref(P)))

    def set_bad(self, slots, bad, ext=None):
        """MapPoint::SetBadFlag for the points at `slots` (distinct)"""
        s = np.ascontiguousarray(slots, np.int32); b = np.ascontiguousarray(bad, np.uint8)
        if len(b) != len(s):
            raise ValueError("%d flags for %d slots" % (len(b), len(s)))
        self._lib.check(self._lib.L.orbm_map_set_bad(self._h(ext), self._m, len(s), s.ctypes.data, b.ctypes.data))

    def set_keyframe(self, row, slots, ext=None):
        """GetMapPointMatches() of the key frame kept in `row`: the slot of feature i, or -1"""
        s = np.ascontiguousarray(slots, np.int32)
        self._lib.check(self._lib.L.orbm_map_set_keyframe(self._h(ext), self._m, int(row), len(s), s.ctypes.data))

    def edit_keyframes(self, rows, feats, slots, ext=None):
        """entry feats[j] of row rows[j] becomes slots[j] (-1 = EraseMapPointMatch): AddMapPoint / ReplaceMapPointMatch / MapPoint::Replace of a whole Fuse
        replay in one call (orbm_map_edit_keyframes); no (row, feat) twice"""
        r, f, s = (np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1), np.int32) for a in (rows, feats, slots))
        if not len(r) == len(f) == len(s):
            raise ValueError("%d rows, %d features, %d slots" % (len(r), len(f), len(s)))
        self._lib.check(self._lib.L.orbm_map_edit_keyframes(self._h(ext), self._m, len(r), r.ctypes.data, f.ctypes.data, s.ctypes.data))

    def local_points(self, rows, seen=None, ext=None):
        """Tracking::UpdateLocalPoints for B = len(rows) frames: rows[b] = the rows frame b visits, in visiting order (mvpLocalKeyFrames reversed);
        seen[b] = the slots frame b already holds (or None).  Builds sets 0 .. B - 1, returns M [B]."""
        B = len(rows)
        cat = lambda lists: (np.cumsum([0] + [len(r) for r in lists]).astype(np.int32), np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).ravel() for r in lists] + [np.zeros(0, np.int32)]), np.int32))
        ks, kr = cat(rows)
        ss = sl = None
        if seen is not None:
            if len(seen) != B:
                raise ValueError("%d seen lists for %d frames" % (len(seen), B))
            ss, sl = cat([[] if s is None else s for s in seen])
        M = np.zeros(max(B, 1), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._lib.check(self._lib.L.orbm_map_local_points(self._h(ext), self._m, B, ks.ctypes.data, kr.ctypes.data, ptr(ss), ptr(sl), M.ctypes.data))
        return M[:B]

    def select(self, b, slots, ext=None):
        """an explicit list of slots (the point set of a Fuse) into set b"""
        s = np.ascontiguousarray(slots, np.int32)
        self._lib.check(self._lib.L.orbm_map_select(self._h(ext), self._m, int(b), len(s), s.ctypes.data))

    def set(self, b, ext=None):
        """set b as the searches take it (valid until the map rebuilds it)"""
        p = self._lib.L.orbm_map_set(self._h(ext), self._m, int(b))
        if not p:
            raise OrbxError(-2, (self._lib.L.orbx_last_error() or b"").decode())
        return _MapSet(p, self._lib.L.orbm_points_count(C.c_void_p(p)))

    def fetch(self, b, ext=None):
        """(slots [M_b] int32: the slot of local point j, seen [M_b] uint8: 1 = frame b already holds it - the searches' is_bad)"""
        m = self.set(b, ext).M
        slots = np.zeros(m, np.int32); seen = np.zeros(m, np.uint8)
        self._lib.check(self._lib.L.orbm_map_set_fetch(self._h(ext), self._m, int(b), slots.ctypes.data, seen.ctypes.data))
        return slots, seen

    def set_sizes(self, set0, B, ext=None):
        """M of sets set0 .. set0 + B - 1 (0 for a set that was never built)"""
        L = self._lib.L
        return [L.orbm_points_count(C.c_void_p(L.orbm_map_set(self._h(ext), self._m, int(set0) + b))) for b in range(B)]

    def fetch_sets(self, set0, B, ext=None):
        """what fetch(set0) .. fetch(set0 + B - 1) return, with one host wait (orbm_map_sets_fetch): (start [B + 1], slots [start[B]], seen [start[B]]);
        set set0 + b's entries are [start[b], start[b + 1])"""
        start = np.cumsum([0] + self.set_sizes(set0, B, ext)).astype(np.int32)
        slots = np.zeros(int(start[-1]), np.int32); seen = np.zeros(int(start[-1]), np.uint8)
        self._lib.check(self._lib.L.orbm_map_sets_fetch(self._h(ext), self._m, int(set0), int(B), start.ctypes.data, slots.ctypes.data, seen.ctypes.data))
        return start, slots, seen

    def stereo_points(self, frames, cam, th_depth, max_points=100, mode=0, cap=None, ext=None):
        """The stereo map points of Tracking::CreateNewKeyFrame (mode 0) / Tracking::UpdateLastFrame (mode 1) for B frames of ext's last extraction
        (orbm_map_stereo_points).  frames: B dicts {frame, Rwc [3, 3], Ow [3], free_slots, keeps (N bytes or None), row (-1 = none)}; cam = (cx, cy,
        invfx, invfy).  Returns (created [B], processed [B], feat [B, cap], slot [B, cap]); a refusal raises OrbxError with .created / .processed set
        (what ORBX_E_CAPACITY reports so that the caller can size a second call)."""
        B = len(frames)
        tab = (_StereoPointsFrame * max(B, 1))()
        keep = []
        for b, f in enumerate(frames):
            t = tab[b]
            t.frame = int(f["frame"])
            t.Rwc[:] = [float(x) for x in np.asarray(f["Rwc"], np.float32).reshape(9)]
            t.Ow[:] = [float(x) for x in np.asarray(f["Ow"], np.float32).reshape(3)]
            fs = np.ascontiguousarray(f["free_slots"], np.int32).reshape(-1)
            k = None if f.get("keeps") is None else np.ascontiguousarray(f["keeps"], np.uint8).reshape(-1)
            keep += [fs, k]
            t.keeps = None if k is None else k.ctypes.data
            t.free_slots = fs.ctypes.data; t.nfree = len(fs)
            t.row = int(f.get("row", -1))
        if cap is None:
            cap = max([len(keep[2 * b]) for b in range(B)] + [0])
        c = np.zeros(6, np.float32); c[:4] = np.asarray(cam, np.float32).reshape(-1)[:4]
        created = np.zeros(max(B, 1), np.int32); processed = np.zeros(max(B, 1), np.int32)
        feat = np.full((max(B, 1), max(cap, 1)), -1, np.int32); slot = np.full((max(B, 1), max(cap, 1)), -1, np.int32)
        rc = self._lib.L.orbm_map_stereo_points(self._h(ext), self._m, B, tab, c.ctypes.data, float(th_depth), int(max_points), int(mode), created.ctypes.data,
                                                processed.ctypes.data, int(cap), feat.ctypes.data, slot.ctypes.data)
        if rc != 0:
            e = OrbxError(rc, (self._lib.L.orbx_last_error() or b"").decode())
            e.created, e.processed = created[:B].copy(), processed[:B].copy()
            raise e
        return created[:B], processed[:B], feat[:B, :cap], slot[:B, :cap]

    def close(self):
        if self._m:
            self._lib.L.orbm_map_destroy(self._ext._h, self._m); self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FrameMap(C.Structure):
    _fields_ = [("points", C.c_void_p), ("is_bad", C.c_void_p), ("has_obs", C.c_void_p)]


class _FrameMaps:
    """The OrbmFrameMap table of B frames with their own local maps: residents = B ResidentPoints (or None = empty map).  table(is_bad, has_obs)
    fills it for one enqueue: None or B arrays (or None) over the points of each frame's set.  The table is a [B, 3] array of addresses laid
    out as B _FrameMap records; each kind of flag is gathered into ONE array first, so that the table takes two base addresses plus offsets
    (asking 2 B arrays for their addresses costs more than the search itself at B = 64)."""

    def __init__(self, residents):
        assert C.sizeof(_FrameMap) == 24
        self.B = len(residents)
        self.sizes = [r.M if r is not None else 0 for r in residents]
        sz = np.array(self.sizes, np.int64)
        self.offsets = np.cumsum(sz) - sz
        self.points = np.array([(r._p.value or 0) if r is not None else 0 for r in residents], np.uint64)
        self.width = max(self.sizes + [1])

    def table(self, is_bad, has_obs):
        B, sizes = self.B, self.sizes
        table = np.zeros((B, 3), np.uint64); keep = []
        table[:, 0] = self.points
        for col, name, flags, default in ((1, "is_bad", is_bad, 0), (2, "has_obs", has_obs, 1)):
            if flags is None:
                continue
            if len(flags) != B:
                raise ValueError("%s: %d arrays for %d frames" % (name, len(flags), B))
            parts = [np.full(sizes[b], default, np.uint8) if a is None else (a if type(a) is np.ndarray else np.asarray(a)) for b, a in enumerate(flags)]
            if [a.size for a in parts] != sizes:
                raise ValueError("%s: %s flags for maps of %s points" % (name, [a.size for a in parts], sizes))
            buf = np.ascontiguousarray(np.concatenate(parts, axis=None), np.uint8)
            keep.append(buf)
            table[:, col] = buf.ctypes.data + self.offsets
        return table, keep


def _maps_of(resident, B):
    """the per-frame form of a batch's `resident` argument (None: it is ONE ResidentPoints), and the width of its in_view rows"""
    if isinstance(resident, ResidentMap):        # the map's own sets: their sizes are read at enqueue time
        return None, 1
    if not isinstance(resident, (list, tuple)):
        return None, max(resident.M, 1)
    if len(resident) != B:
        raise ValueError("%d local maps for %d frames" % (len(resident), B))
    fm = _FrameMaps(list(resident))
    return fm, fm.width


def frustum_view(Rcw, tcw, cam, bounds, mbf, scale_factors, into=None):
    """OrbmFrustumView of one frame.  The pose is a sophus.SE3f (pass it as Rcw, tcw = None) or (Rcw, tcw), which enters through Sophus' SE3(R, t)
    constructor as in Frame::SetPose(Sophus::SE3f(R, t)); the view then holds what Frame::UpdatePoseMatrices derives (src/Frame.cc:594-598):
    mRcw = mTcw.rotationMatrix(), mtcw, mOw = mTcw.inverse().translation(), plus the unit quaternion for the searches that evaluate Tcw * p.
    Camera (4 pinhole or 8 Kannala-Brandt parameters), image bounds (min_x, max_x, min_y, max_y), mbf, the scale factors.
    Returns (view, the float32 scale-factor array the view points into - keep it alive)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    T = Rcw if isinstance(Rcw, SE3f) else SE3f(Rcw, tcw)
    sf = f32(scale_factors)
    V = into if into is not None else _FrustumView()
    V.Rcw[:] = [float(v) for v in T.rotationMatrix().ravel()]; V.tcw[:] = [float(v) for v in T.translation()]
    V.Ow[:] = [float(v) for v in T.inverse().translation()]
    V.qcw[:] = [float(v) for v in T.unit_quaternion()]
    cam = [float(v) for v in cam]
    V.camera_type = 1 if len(cam) == 8 else 0
    V.cam[:] = cam + [0.0] * (8 - len(cam))
    V.min_x, V.max_x, V.min_y, V.max_y = [float(v) for v in bounds]
    V.mbf = float(mbf); V.log_scale_factor = float(np.float32(np.log(np.float64(sf[1])))) if len(sf) > 1 else 1.0
    V.nlevels = len(sf); V.scale_factors = sf.ctypes.data
    return V, sf


def ComputeStereoFromRGBD(ext, depth, mbf, first=0, device_ptr=None, shape=None):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:1361-1391) for the frames [first, first + B) of ext's last batch: depth [B, H, W] float32 (CV_32F,
    already multiplied by the depth map factor), host array or (device_ptr, shape).  Asynchronous; fetch with StereoFetch(ext, B) or keep on the
    device for SearchLocalPointsBatch."""
    L = ext._lib
    if device_ptr is None:
        depth = np.ascontiguousarray(depth, np.float32)
        B, H, W = depth.shape
        ext._keep_depth = depth
        L.check(L.L.orbm_stereo_from_depth(ext._h, int(first), B, depth.ctypes.data, W, H * W, 0, float(mbf)))
    else:
        B, H, W = shape
        L.check(L.L.orbm_stereo_from_depth(ext._h, int(first), B, device_ptr, W, H * W, 1, float(mbf)))
    return B


def StereoFetch(ext, B):
    """(mvuRight [B, cap], mvDepth [B, cap], matches [B]) of the last orbm_stereo_match / orbm_stereo_from_depth of `ext`."""
    cap = ext.max_keypoints()
    u = np.zeros((B, cap), np.float32); d = np.zeros((B, cap), np.float32); n = np.zeros(B, np.int32)
    ext._lib.check(ext._lib.L.orbm_stereo_fetch(ext._h, B, u.ctypes.data, d.ctypes.data, cap, n.ctypes.data))
    return u, d, n


class LocalPointsBatch:
    """Tracking::SearchLocalPoints for a batch of frames that stay on the device (orbm_search_local_points_batch): the frames are images
    [first, first + B) of ext's last extraction, the local map is a ResidentPoints, poses = B x (Rcw, tcw).  enqueue() is asynchronous, fetch()
    returns (assigned [B, cap], nmatches [B], in_view [B, M] or None).
    Independent streams: `resident` = a list of B ResidentPoints (or None = empty map), frame b is searched against its own
    (orbm_search_local_points_batch_maps); is_bad / has_obs of enqueue() are then lists of B arrays (or None), assigned[b] indexes frame b's set and
    in_view is [B, M_max], zero beyond M_b.
    On a resident map: `resident` = a ResidentMap, frame b is searched against the map's set set0 + b as its last build left it
    (orbm_search_local_points_batch_map): the seen bytes of the set are its is_bad, every point counts as observed, enqueue() takes neither, and
    fetch_slots() returns assigned as map SLOTS (fetch() still returns positions in the sets' lists)."""

    def __init__(self, ext, resident, B, cam, bounds, mbf, scale_factors, set0=0):
        self.ext, self.res, self.B = ext, resident, B
        self.map, self.set0 = (resident if isinstance(resident, ResidentMap) else None), int(set0)
        self.cam, self.bounds, self.mbf = cam, bounds, mbf
        self.sf = np.ascontiguousarray(scale_factors, np.float32)
        self.views = (_FrustumView * B)()
        self.cap = ext.max_keypoints()
        self.assigned = np.full((B, self.cap), -1, np.int32); self.nm = np.zeros(B, np.int32)
        self.maps, width = _maps_of(resident, B)
        self.in_view = np.zeros((B, width), np.uint8)

    def set_poses(self, poses):
        for b, pose in enumerate(poses):
            frustum_view(as_se3(pose), None, self.cam, self.bounds, self.mbf, self.sf, into=self.views[b])
            self.views[b].scale_factors = self.sf.ctypes.data

    def enqueue(self, first=0, is_bad=None, has_obs=None, occupied=None, use_u_right=True, viewing_cos_limit=0.5, th=1.0, far_points=False, th_far=50.0, nnratio=0.8,
                want_in_view=False):
        L = self.ext._lib
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        self._again = lambda: self.enqueue(first, is_bad, has_obs, occupied, use_u_right, viewing_cos_limit, th, far_points, th_far, nnratio, want_in_view)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._want = bool(want_in_view)
        if self.map is not None:
            if is_bad is not None or has_obs is not None:
                raise ValueError("a batch on a ResidentMap reads its flags from the map's sets: is_bad / has_obs cannot be given")
            if self._want:
                self.in_view = np.zeros((self.B, max(self.map.set_sizes(self.set0, self.B, self.ext) + [1])), np.uint8)
            self._keep = (None, None, u8(occupied))
            L.check(L.L.orbm_search_local_points_batch_map(self.ext._h, int(first), self.B, self.views, self.map._m, self.set0, ptr(self._keep[2]), int(bool(use_u_right)),
                                                           float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio), int(self._want)))
            return
        if self.maps is not None:
            table, flags = self.maps.table(is_bad, has_obs)
            self._keep = (table, flags, u8(occupied))
            L.check(L.L.orbm_search_local_points_batch_maps(self.ext._h, int(first), self.B, self.views, table.ctypes.data, ptr(self._keep[2]), int(bool(use_u_right)),
                                                            float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio), int(self._want)))
            return
        self._keep = (u8(is_bad), u8(has_obs), u8(occupied))
        L.check(L.L.orbm_search_local_points_batch(self.ext._h, int(first), self.B, self.views, self.res._p, ptr(self._keep[0]), ptr(self._keep[1]), ptr(self._keep[2]),
                                                   int(bool(use_u_right)), float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio), int(self._want)))

    def fetch(self, _call="orbm_search_local_points_fetch"):
        L = self.ext._lib
        fetch = lambda: getattr(L.L, _call)(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, self.in_view.ctypes.data if self._want else None)
        rc = fetch()
        if rc == -4:                 # ORBX_E_CAPACITY: the candidate pool was too small for this scene and has been enlarged - run the batch again
            self._again()
            rc = fetch()
        L.check(rc)
        return self.assigned, self.nm, (self.in_view if self._want else None)

    def fetch_slots(self):
        """fetch() of a batch on a ResidentMap with assigned[b, i] = the map slot of the point written to keypoint i (negative entries as in fetch())"""
        return self.fetch("orbm_search_local_points_fetch_slots")


class LocalPointsRigBatch:
    """Tracking::SearchLocalPoints for a batch of rig frames that stay on the device (orbm_search_local_points_rig_batch): frame b = left image
    left_first + b of `left`'s last extraction and right image right_first + b of `right`'s (right_first defaults to B when both are one handle,
    the layout [L0 .. L(B-1), R0 .. R(B-1)], else to 0), linked by the last ComputeStereoFishEyeMatches over exactly these frames; the local map is a
    ResidentPoints.  set_poses() takes B pose dicts as SearchLocalPointsRig does.  enqueue() is asynchronous, fetch() returns (assigned [B, 2 cap]
    in the slot layout of F.mvpMapPoints, nmatches [B], in_view [B, M] or None, in_view_r [B, M] or None).
    Independent streams: `resident` = a list of B ResidentPoints (or None), is_bad / has_obs lists of B arrays (or None), as LocalPointsBatch
    (orbm_search_local_points_rig_batch_maps); in_view / in_view_r are then [B, M_max].
    On a resident map: `resident` = a ResidentMap, frame b against the map's set set0 + b (orbm_search_local_points_rig_batch_map), as LocalPointsBatch;
    fetch_slots() returns both cameras' halves of assigned as map slots."""

    def __init__(self, left, right, resident, B, cam1, cam2, bounds, scale_factors, left_first=0, right_first=None, set0=0):
        self.ext, self.right, self.res, self.B = left, right, resident, B
        self.map, self.set0 = (resident if isinstance(resident, ResidentMap) else None), int(set0)
        self.lf, self.rf = int(left_first), int((B if right is left else 0) if right_first is None else right_first)
        self.cam1, self.cam2, self.bounds = cam1, cam2, bounds
        self.sf = np.ascontiguousarray(scale_factors, np.float32)
        self.views = (_FrustumRigView * B)()
        self.cap = 2 * left.max_keypoints()
        self.assigned = np.full((B, self.cap), -1, np.int32); self.nm = np.zeros(B, np.int32)
        self.maps, width = _maps_of(resident, B)
        self.in_view = np.zeros((B, width), np.uint8); self.in_view_r = np.zeros((B, width), np.uint8)

    def set_poses(self, poses):
        for b, pose in enumerate(poses):
            rig_frustum_view(pose, self.cam1, self.cam2, self.bounds, self.sf, into=self.views[b])

    def enqueue(self, is_bad=None, has_obs=None, occupied=None, viewing_cos_limit=0.5, th=1.0, far_points=False, th_far=50.0, nnratio=0.8, want_in_view=False):
        L = self.ext._lib
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        self._again = lambda: self.enqueue(is_bad, has_obs, occupied, viewing_cos_limit, th, far_points, th_far, nnratio, want_in_view)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._want = bool(want_in_view)
        if self.map is not None:
            if is_bad is not None or has_obs is not None:
                raise ValueError("a batch on a ResidentMap reads its flags from the map's sets: is_bad / has_obs cannot be given")
            if self._want:
                width = max(self.map.set_sizes(self.set0, self.B, self.ext) + [1])
                self.in_view = np.zeros((self.B, width), np.uint8); self.in_view_r = np.zeros((self.B, width), np.uint8)
            self._keep = (None, None, u8(occupied))
            L.check(L.L.orbm_search_local_points_rig_batch_map(self.ext._h, self.lf, self.right._h, self.rf, self.B, self.views, self.map._m, self.set0, ptr(self._keep[2]),
                                                               float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio), int(self._want)))
            return
        if self.maps is not None:
            table, flags = self.maps.table(is_bad, has_obs)
            self._keep = (table, flags, u8(occupied))
            L.check(L.L.orbm_search_local_points_rig_batch_maps(self.ext._h, self.lf, self.right._h, self.rf, self.B, self.views, table.ctypes.data, ptr(self._keep[2]),
                                                                float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio), int(self._want)))
            return
        self._keep = (u8(is_bad), u8(has_obs), u8(occupied))
        L.check(L.L.orbm_search_local_points_rig_batch(self.ext._h, self.lf, self.right._h, self.rf, self.B, self.views, self.res._p, ptr(self._keep[0]),
                                                       ptr(self._keep[1]), ptr(self._keep[2]), float(viewing_cos_limit), float(th), int(far_points), float(th_far),
                                                       float(nnratio), int(self._want)))

    def _fetch(self, call="orbm_search_rig_batch_fetch"):
        iv = lambda a: a.ctypes.data if self._want else None
        return getattr(self.ext._lib.L, call)(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, iv(self.in_view), iv(self.in_view_r))

    def fetch(self, _call="orbm_search_rig_batch_fetch"):
        rc = self._fetch(_call)
        if rc == -4:                 # ORBX_E_CAPACITY: the candidate pool was too small for this scene and has been enlarged - run the batch again
            self._again()
            rc = self._fetch(_call)
        self.ext._lib.check(rc)
        return self.assigned, self.nm, (self.in_view if self._want else None), (self.in_view_r if self._want else None)

    def fetch_slots(self):
        """fetch() of a batch on a ResidentMap with both halves of assigned as map slots (orbm_search_rig_batch_fetch_slots)"""
        return self.fetch("orbm_search_rig_batch_fetch_slots")


class LastFrameRigBatch:
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) for a batch of rig frames on the device (orbm_search_by_projection_lastframe_rig_batch):
    frames as LocalPointsRigBatch, per frame the map points of its last frame (rows indexed like LastFrame.mvpMapPoints).  set_poses(poses, Trl): B
    camera-1 poses (SE3f or (R, t)) and the rig's mTrl; camera 2's projections are made on the device.  enqueue() is asynchronous, fetch() returns
    (assigned [B, 2 cap], nmatches [B])."""

    def __init__(self, left, right, B, cam1, bounds, scale_factors, left_first=0, right_first=None):
        self.ext, self.right, self.B = left, right, B
        self.lf, self.rf = int(left_first), int((B if right is left else 0) if right_first is None else right_first)
        self.cam1, self.bounds = cam1, bounds
        self.sf = np.ascontiguousarray(scale_factors, np.float32)
        self.views = (_FrustumRigView * B)()
        self.cap = 2 * left.max_keypoints()
        self.assigned = np.full((B, self.cap), -1, np.int32); self.nm = np.zeros(B, np.int32)
        self.trl = np.zeros(7, np.float32)

    def set_poses(self, poses, Trl):
        for b, pose in enumerate(poses):
            frustum_view(as_se3(pose), None, self.cam1, self.bounds, 0.0, self.sf, into=self.views[b].left)
            self.views[b].left.scale_factors = self.sf.ctypes.data
        T = as_se3(Trl)
        self.trl[:] = [float(v) for v in T.unit_quaternion()] + [float(v) for v in T.translation()]

    def enqueue(self, n, pos, valid, octave, angle, has_obs, desc, th, forward=None, backward=None, check_orientation=True, occupied=None):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)
        self._again = lambda: self.enqueue(n, pos, valid, octave, angle, has_obs, desc, th, forward, backward, check_orientation, occupied)
        pos = f32(pos); capL = pos.shape[1]
        self._keep = (np.ascontiguousarray(n, np.int32), pos, u8(valid), np.ascontiguousarray(octave, np.int32), f32(angle), u8(has_obs), u8(desc), u8(forward), u8(backward), u8(occupied))
        k = self._keep
        ptr = lambda a: None if a is None else a.ctypes.data
        lb = _LastFrameBatch(capL, ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(k[3]), ptr(k[4]), ptr(k[5]), ptr(k[6]))
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_lastframe_rig_batch(self.ext._h, self.lf, self.right._h, self.rf, self.B, self.views, self.trl.ctypes.data, C.byref(lb),
                                                                  float(th), ptr(k[7]), ptr(k[8]), int(bool(check_orientation)), ptr(k[9])))

    def enqueue_slots(self, resident_map, n, slots, outlier, octave, angle, has_obs, th, forward=None, backward=None, check_orientation=True, occupied=None):
        """The same search with the last frame's map points named by slot of a ResidentMap (orbm_search_by_projection_lastframe_rig_batch_map); the
        arguments as LastFrameBatch.enqueue_slots."""
        self._again = lambda: self.enqueue_slots(resident_map, n, slots, outlier, octave, angle, has_obs, th, forward, backward, check_orientation, occupied)
        lb, k = _last_frame_slots(n, slots, outlier, octave, angle, has_obs, forward, backward, occupied)
        self._keep = k
        ptr = lambda a: None if a is None else a.ctypes.data
        L = self.ext._lib
        L.check(L.L.orbm_search_by_projection_lastframe_rig_batch_map(self.ext._h, self.lf, self.right._h, self.rf, self.B, self.views, self.trl.ctypes.data, resident_map._m,
                                                                      C.byref(lb), float(th), ptr(k[6]), ptr(k[7]), int(bool(check_orientation)), ptr(k[8])))

    def fetch(self):
        L = self.ext._lib
        rc = L.L.orbm_search_rig_batch_fetch(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, None, None)
        if rc == -4:                 # ORBX_E_CAPACITY: pool enlarged, run the batch again
            self._again()
            rc = L.L.orbm_search_rig_batch_fetch(self.ext._h, self.assigned.ctypes.data, self.cap, self.nm.ctypes.data, None, None)
        L.check(rc)
        return self.assigned, self.nm


def SearchLocalPoints(ext, frame, Rcw, tcw, cam, bounds, mbf, scale_factors, pos, normal, min_distance, max_distance, is_bad=None, has_obs=None, desc=None,
                      viewing_cos_limit=0.5, th=1.0, far_points=False, th_far=50.0, nnratio=0.8, search=True, prepared=False, resident=None):
    """Frame::isInFrustum (src/Frame.cc:667-773) for M map points and, with search=True, ORBmatcher::SearchByProjection(F, points, th, ...)
    (src/ORBmatcher.cc:45-167) on those in view - Tracking::SearchLocalPoints (src/Tracking.cc:4009-4067) on the device.
    cam: (fx, fy, cx, cy) or the 8 Kannala-Brandt parameters; bounds = (min_x, max_x, min_y, max_y); frame: views.frame_view(...).
    Returns (track dict, assigned[N] or None, nmatches)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    pos, normal, mn, mx = f32(pos).reshape(-1, 3), f32(normal).reshape(-1, 3), f32(min_distance), f32(max_distance)
    M = len(pos)
    V, sf = frustum_view(Rcw, tcw, cam, bounds, mbf, scale_factors)
    P = _WorldPointView()
    bad = None if is_bad is None else np.ascontiguousarray(is_bad, np.uint8); obs = None if has_obs is None else np.ascontiguousarray(has_obs, np.uint8)
    d = None if desc is None else np.ascontiguousarray(desc, np.uint8)
    P.M = M; P.pos = pos.ctypes.data; P.normal = normal.ctypes.data; P.min_distance = mn.ctypes.data; P.max_distance = mx.ctypes.data
    P.is_bad = None if bad is None else bad.ctypes.data; P.has_obs = None if obs is None else obs.ctypes.data; P.desc = None if d is None else d.ctypes.data
    tr = dict(in_view=np.zeros(max(M, 1), np.uint8), proj_x=np.zeros(max(M, 1), np.float32), proj_y=np.zeros(max(M, 1), np.float32), proj_xr=np.zeros(max(M, 1), np.float32),
              depth=np.zeros(max(M, 1), np.float32), view_cos=np.zeros(max(M, 1), np.float32), scale_level=np.zeros(max(M, 1), np.int32))
    T = _TrackOut(*[tr[k].ctypes.data for k in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "scale_level")])
    L = ext._lib
    if not search:
        L.check(L.L.orbm_is_in_frustum(ext._h, C.byref(V), C.byref(P), float(viewing_cos_limit), C.byref(T)))
        return {k: v[:M] for k, v in tr.items()}, None, 0
    assigned = np.full(max(frame.view.N, 1), -1, np.int32); n = C.c_int(0)
    keep = (V, P, T, sf, pos, normal, mn, mx, bad, obs, d, tr)

    def call(_keep=keep):
        """the C ABI call alone (arguments prebuilt): what a C++ caller pays.  resident: a ResidentPoints made from the same points"""
        if resident is not None:
            return L.L.orbm_search_local_points_resident(ext._h, frame.ref(), C.byref(V), resident._p, P.is_bad, P.has_obs, float(viewing_cos_limit), float(th), int(far_points),
                                                         float(th_far), float(nnratio), C.byref(T), assigned.ctypes.data, C.byref(n))
        return L.L.orbm_search_local_points(ext._h, frame.ref(), C.byref(V), C.byref(P), float(viewing_cos_limit), float(th), int(far_points), float(th_far), float(nnratio),
                                            C.byref(T), assigned.ctypes.data, C.byref(n))
    if prepared:
        return call
    L.check(call())
    return {k: v[:M] for k, v in tr.items()}, assigned[:frame.view.N], n.value


def GetFeaturesInArea(ext, frame, x, y, r, minLevel=-1, maxLevel=-1):
    """Frame::GetFeaturesInArea (src/Frame.cc:859): keypoint indices in the reference's order."""
    cap = max(frame.view.N, 1)
    out = np.zeros(cap, np.int32)
    n = ext._lib.L.orbm_get_features_in_area(ext._h, frame.ref(), float(x), float(y), float(r), int(minLevel), int(maxLevel), out.ctypes.data, cap)
    if n < 0:
        ext._lib.check(n)
    return out[:n].copy()


def AreaSearchBatch(ext, frame, queries, query_desc):
    """Batched GetFeaturesInArea + Hamming distances (orbm_area_search_batch).  queries: [Q,5] float array (x, y, r, minLevel,
    maxLevel); returns per query a list of (idx, dist, level) in the reference's GetFeaturesInArea order."""
    q = np.zeros(len(queries), np.dtype([("x", "<f4"), ("y", "<f4"), ("r", "<f4"), ("mn", "<i4"), ("mx", "<i4")]))
    qa = np.asarray(queries, np.float64).reshape(-1, 5)
    q["x"], q["y"], q["r"], q["mn"], q["mx"] = qa[:, 0], qa[:, 1], qa[:, 2], qa[:, 3].astype(np.int32), qa[:, 4].astype(np.int32)
    d = np.ascontiguousarray(query_desc, np.uint8).reshape(len(q), 32)
    Q = len(q)
    start = np.zeros(Q, np.int32); count = np.zeros(Q, np.int32)
    cap = max(64 * Q, 1024)
    for _ in range(2):
        idx = np.zeros(cap, np.int32); dist = np.zeros(cap, np.int32); lvl = np.zeros(cap, np.int32)
        tot = ext._lib.L.orbm_area_search_batch(ext._h, frame.ref(), q.ctypes.data, d.ctypes.data, Q, start.ctypes.data, count.ctypes.data,
                                                idx.ctypes.data, dist.ctypes.data, lvl.ctypes.data, cap)
        if tot < 0:
            ext._lib.check(tot)
        if tot <= cap:
            break
        cap = tot
    return [list(zip(idx[s:s + c].tolist(), dist[s:s + c].tolist(), lvl[s:s + c].tolist())) for s, c in zip(start.tolist(), count.tolist())]


def ComputeDistinctiveDescriptors(ext, desc, start):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438) for many map points: desc [total, 32] uint8, start [P+1] offsets.
    Returns best[P]: which of each point's descriptors becomes mDescriptor (-1: point without descriptors)."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); st = np.ascontiguousarray(start, np.int32)
    P = len(st) - 1
    best = np.full(max(P, 1), -1, np.int32)
    ext._lib.check(ext._lib.L.orbm_distinctive_descriptors(ext._h, d.ctypes.data if len(d) else None, st.ctypes.data, P, best.ctypes.data))
    return best[:P]


def ComputeDistinctiveDescriptorsResident(ext, kfs, obs_start, obs_kf, obs_feat, resident_map=None, slots=None, want_desc=False):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438) on observations named by (resident key frame, feature): point p owns observations
    [obs_start[p], obs_start[p+1]), observation o is row obs_feat[o] of ResidentKeyFrame kfs[obs_kf[o]].  With a ResidentMap and slots [P] the chosen
    descriptor overwrites the descriptor of slot slots[p] in the map's store on the device (-1: this point writes nothing).
    Returns best[P] (-1: point without observations), or (best, desc [P, 32]) with want_desc - rows of points without observations stay zero."""
    st = np.ascontiguousarray(obs_start, np.int32); ok = np.ascontiguousarray(obs_kf, np.int32); of = np.ascontiguousarray(obs_feat, np.int32)
    P = len(st) - 1
    if P > 0 and (len(ok) < st[-1] or len(of) < st[-1]):
        raise ValueError("obs_start names %d observations, obs_kf / obs_feat hold %d / %d" % (st[-1], len(ok), len(of)))
    table = (C.c_void_p * max(len(kfs), 1))(*[k._kf for k in kfs])
    sl = None
    if slots is not None:
        sl = np.ascontiguousarray(slots, np.int32)
        if len(sl) != P:
            raise ValueError("%d slots for %d points" % (len(sl), P))
    best = np.full(max(P, 1), -1, np.int32)
    desc = np.zeros((max(P, 1), 32), np.uint8) if want_desc else None
    ptr = lambda a: None if a is None else a.ctypes.data
    ext._lib.check(ext._lib.L.orbm_distinctive_descriptors_resident(ext._h, len(kfs), table, P, st.ctypes.data, ok.ctypes.data, of.ctypes.data,
                                                                    resident_map._m if resident_map is not None else None, ptr(sl), best.ctypes.data, ptr(desc)))
    return (best[:P], desc[:P]) if want_desc else best[:P]
