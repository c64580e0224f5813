"""k_stereo_match reads the right keypoints' search records in bucket order (k_layout gives every slot its place, k_orient_brief writes the record
there), loads the descriptors of a trip's two candidates together behind an address select, takes the winner's x out of the record its lane
read, and requests the SAD rows of all row groups at once.  The pairs here go through extraction, so the records and the row buckets are the
library's own; mvuRight, mvDepth and the match count of every pair are compared with the reference's Frame::ComputeStereoMatches (and with the
oracle), in the normal and in the reversed visiting order (orbx_debug_stereo_flags 1).

What each pair is there for is asserted from the bucket arithmetic of the kernel, restated on the fetched keypoints:
  dense   239 x 239, 2000 features: some left keypoints meet more than 128 candidates (a second trip of the search loop, whose last lanes have no
          candidate), none meets zero
  sparse  a few isolated corners: some left keypoints meet no candidate at all (the loop is not entered), some exactly one (63 + 64 lanes of the
          trip repeat that one's load and drop it)
Each case runs on the SIMT emulator and, marked gpu, on the device."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import synth
from orb_slam3_detailed_comments_amd.extractor import ORBextractor
from orb_slam3_detailed_comments_amd.matcher import ComputeStereoMatches

FX = 458.654
BF = FX * 0.110074
ROW_SHIFT = 3                # kStereoRowShift


def _sparse_pair():
    """a flat ground with single pixels 8 grey levels above it - each is one keypoint, on level 0 only: the next level's resize leaves less than the
    FAST threshold of it - and two bright squares.  Rows 30, 60 and 130 hold one such pixel in both views (a left keypoint there meets exactly one
    candidate), row 100 one in the left view only (no candidate: the nearest right keypoints are 30 rows away), rows 170 - 200 the squares in both
    views (several candidates on several levels, and matches)"""
    L = np.full((239, 239), 60, np.uint8)
    R = L.copy()
    for (y, x, both) in ((30, 120, True), (60, 90, True), (130, 100, True), (100, 150, False)):
        L[y, x] = 68
        if both:
            R[y, x - 6] = 68
    for (y, x, s) in ((170, 60, 12), (190, 160, 10)):
        L[y:y + s, x:x + s] = 200
        R[y:y + s, x - 6:x - 6 + s] = 200
    return L, R


PAIRS = {
    # name: (factory, nfeatures)
    "dense": (lambda: synth.stereo_pair(239, 239, seed=7, nrect=900), 2000),
    "sparse": (_sparse_pair, 500),
}
_expected = {}


def _expect(name):
    """the pair, the reference Frame and the oracle's stereo result: computed once, shared, never changed"""
    if name not in _expected:
        factory, nf = PAIRS[name]
        L, R = factory()
        oL, oR = ol.OracleExtractor(nf), ol.OracleExtractor(nf)
        eL, eR = oL.extract(L), oR.extract(R)
        uo, do, no = ol.oracle_stereo(oL, oR, eL[1], eL[2], eR[1], eR[2], BF, BF / FX)
        F = ol.ReferenceFrame(L, R, nf, fx=FX, bf=BF) if ol.reference() is not None else None
        _expected[name] = (L, R, nf, (eL, eR, uo, do, no), F)
    return _expected[name]


def _candidates(ex, kL, kR, height):
    """number of right keypoints each left keypoint's trips visit: the run of row buckets [rowL - lookback, rowL] of k_stereo_match"""
    sf = np.asarray(ex.GetScaleFactors(), np.float32)
    nb = (height >> ROW_SHIFT) + 2
    lookback = int(np.ceil(np.float32(4.0) * sf[-1])) + 2
    first = np.floor(kR["y"] - np.float32(2.0) * sf[kR["octave"]]).astype(np.int64)
    bucket = np.minimum(np.maximum(first, 0) >> ROW_SHIFT, nb - 1)
    per_bucket = np.bincount(bucket, minlength=nb)
    start = np.concatenate([[0], np.cumsum(per_bucket)])
    rowL = kL["y"].astype(np.int64)                      # __float2int_rz of a positive float
    lo = np.minimum(np.maximum(rowL - lookback, 0) >> ROW_SHIFT, nb - 1)
    hi = np.minimum(np.maximum(rowL, 0) >> ROW_SHIFT, nb - 1)
    return start[hi + 1] - start[lo]


def _chain(lib, name):
    L, R, nf, (eL, eR, uo, do, no), F = _expect(name)
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    (_, kL, dL), (_, kR, dR) = ex.extract_batch(np.stack([L, R]))
    assert kL.tobytes() == eL[1].tobytes() and dL.tobytes() == eL[2].tobytes() and kR.tobytes() == eR[1].tobytes() and dR.tobytes() == eR[2].tobytes()
    cand = _candidates(ex, kL, kR, L.shape[0])
    if name == "dense":
        assert (cand > 128).sum() > 20 and (cand % 128 != 0).all() and cand.min() > 0, (cand.min(), cand.max())
    else:
        assert (cand == 0).sum() >= 1 and (cand == 1).sum() >= 2 and cand.max() > 2, np.bincount(cand).tolist()
    N = len(kL)
    for flags in (0, 1):
        ex.debug_stereo_flags(flags)
        u, d, n = ComputeStereoMatches(ex, ex, BF, BF / FX, 0, 1, 1)
        tag = "%s, flags %d" % (name, flags)
        assert int(n[0]) == no and u[0, :N].tobytes() == uo.tobytes() and d[0, :N].tobytes() == do.tobytes(), tag + ": differs from the oracle"
        assert (u[0, N:] == -1).all() and (d[0, N:] == -1).all(), tag
        if F is not None:
            assert F.N == N and int(n[0]) == int((F.u_right >= 0).sum()), tag
            assert u[0, :N].tobytes() == F.u_right.tobytes() and d[0, :N].tobytes() == F.depth.tobytes(), tag + ": differs from the reference Frame"
    if name == "dense":
        assert no > 100
    ex.close()


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_stereo_chain_emu(emu_lib, name):
    _chain(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_stereo_chain_gpu(hip_lib, name):
    _chain(hip_lib, name)
