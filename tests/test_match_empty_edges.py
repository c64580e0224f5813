"""The matching kernels with nothing, or next to nothing, to match against.

Stereo: a textured left image and a flat right image - the right extractor returns no keypoint, k_stereo_match finds no candidate for any left
keypoint (`nr > 0` false) and k_stereo_median has no SAD to take the median of (`cnt == 0`).  The reference leaves mvuRight / mvDepth at -1
(src/Frame.cc:1102-1358), checked against its own Frame constructor where oracle/_ref is built and against the oracle restatement otherwise.

Fisheye 2-NN (k_knn2_mfma and the wave-per-query k_knn2): a right image without a keypoint - no nearest neighbour - and one with exactly one
keypoint - a nearest neighbour but no second one, so the ratio test (src/Frame.cc:1556 asks for two matches) can never pass.  Checked against
a numpy 2-NN.  Each handle has matched an ordinary pair first, so that a kernel that left its outputs alone would return the earlier results."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, ComputeStereoMatches, synth
from orb_slam3_detailed_comments_amd import matcher as M
from resident_inject import knn2_expected as _knn2         # the numpy 2-NN, shared with tests/test_knn2_constructed.py

W, H, NF = 376, 240, 500
FX, B = 458.654, 0.110074
BF = FX * B
LAP = (60, 300)


def _flat():
    return np.full((H, W), 90, np.uint8)


def _one_corner():
    """the corner of a slightly brighter quarter plane on a flat field: FAST fires on one pyramid level only"""
    img = _flat()
    img[100:, 150:] = 98
    return img


def _textured():
    return synth.stereo_pair(W, H, seed=20, nrect=800)


def _check_stereo(lib):
    L, R = _textured()
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    ex.extract_batch(np.stack([L, R]))
    u, d, n = ComputeStereoMatches(ex, ex, BF, B, 0, 1, 1)
    assert n[0] > 50                                             # the handle's result buffers now hold matches
    res = ex.extract_batch(np.stack([L, _flat()]))
    u, d, n = ComputeStereoMatches(ex, ex, BF, B, 0, 1, 1)
    oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
    eL, eR = oL.extract(L), oR.extract(_flat())
    N = len(eL[1])
    assert len(eR[1]) == 0 and N > 300                           # the edge, from the reference side
    assert len(res[1][1]) == 0 and res[0][1].tobytes() == eL[1].tobytes()
    if ol.reference_frame_lib() is not None:
        F = ol.ReferenceFrame(L, _flat(), NF, 1.2, 8, 20, 7, 0, fx=FX, bf=BF)
        assert len(F.keys_right) == 0 and F.N == N
        exp_u, exp_d = F.u_right, F.depth
    else:
        exp_u, exp_d, no = ol.oracle_stereo(oL, oR, eL[1], eL[2], eR[1], eR[2], BF, B)
        assert no == 0
    assert (exp_u == -1).all() and (exp_d == -1).all() and len(exp_u) == N
    assert n[0] == 0
    assert u[0, :N].tobytes() == exp_u.tobytes() and d[0, :N].tobytes() == exp_d.tobytes()
    assert (u[0, N:] == -1).all() and (d[0, N:] == -1).all()
    ex.close()


def test_stereo_right_image_without_keypoints_emulated(emu_lib):
    _check_stereo(emu_lib)


@pytest.mark.gpu
def test_stereo_right_image_without_keypoints_gpu(hip_lib):
    _check_stereo(hip_lib)


def _check_fisheye(lib):
    L, R = _textured()
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    # the right images as the reference extracts them: none / exactly one keypoint, and that one inside the lapping area
    o = ol.OracleExtractor(NF)
    assert len(o.extract(_flat(), LAP)[1]) == 0
    m1, k1, d1 = o.extract(_one_corner(), LAP)
    assert len(k1) == 1 and m1 == 0
    for flags in (0, 8):                                         # the matrix-core kernel, the wave-per-query kernel
        ex.debug_stereo_flags(flags)
        res = ex.extract_batch(np.stack([L, L, R, R]), LAP)
        out = M.StereoFishEyeKnn(ex, ex, 0, 2, 2)
        mL, dL = res[0][0], res[0][2]
        nq = len(dL) - mL
        assert nq > 100 and out["ratio_ok"][:, :nq].sum() > 40       # ordinary pairs first: the result buffers hold neighbours
        ref = _knn2(dL[mL:], res[2][2][res[2][0]:])
        for key in ref:
            assert np.array_equal(out[key][0, :nq], ref[key]), (key, flags)
        res = ex.extract_batch(np.stack([L, L, _flat(), _one_corner()]), LAP)
        out = M.StereoFishEyeKnn(ex, ex, 0, 2, 2)
        assert len(res[2][1]) == 0 and len(res[3][1]) == 1 and res[3][0] == 0 and res[3][2].tobytes() == d1.tobytes()
        for p, dT in ((0, res[2][2]), (1, res[3][2])):
            ref = _knn2(dL[mL:], dT)
            assert (ref["idx1"] == -1).all() and not ref["ratio_ok"].any() and (ref["idx0"] == (-1 if p == 0 else 0)).all()
            for key in ref:
                assert np.array_equal(out[key][p, :nq], ref[key]), (key, "pair %d" % p, flags)
            assert (out["idx0"][p, nq:] == -1).all() and not out["ratio_ok"][p, nq:].any()
    ex.debug_stereo_flags(0)
    ex.close()


def test_fisheye_right_image_with_no_and_one_keypoint_emulated(emu_lib):
    _check_fisheye(emu_lib)


@pytest.mark.gpu
def test_fisheye_right_image_with_no_and_one_keypoint_gpu(hip_lib):
    _check_fisheye(hip_lib)
