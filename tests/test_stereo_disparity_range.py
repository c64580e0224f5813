"""The two ends of Frame::ComputeStereoMatches' acceptance that the constructed-descriptor and sub-pixel tests left open (csrc/k_match.hip: k_stereo_match; found by
the mutation pass recorded in profiles/emu_mutants/README.md: `disparity < maxD` -> `<=` and `endu >= Lw` -> `>` survived every test).

1. `disparity >= minD && disparity < maxD` (src/Frame.cc:1317) at disparity == maxD EXACTLY.  The right image is the left one moved by a whole number D of pixels,
   flat rectangles without noise above row 80 (tests/test_branch_edges_stereo.py: there the SADs one pixel left and right of the best shift are often equal, deltaR == 0),
   so a level-0 keypoint at integer uL whose match sits at uL - D is refined to bestuR == uL - D and its disparity is the float D.  Below row 80 both images carry
   their own noise of +-3 grey levels: those matches keep the median SAD above 0, so that a match with SAD 0 that is wrongly accepted survives the outlier removal
   and shows in mvuRight / mvDepth.  maxD = mbf / mb with mb = mbf / fx as the reference computes them (mbf = 3: maxD == fx for the three fx used):
     at_maxd          D = 24, maxD = 24: the disparity equals maxD and the match is REFUSED (the comparison is strict)
     one_px_inside    D = 23, maxD = 24: the same keypoints one pixel inside the range are accepted
     one_float_inside D = 24, maxD = the float above 24: the same disparities, one float below maxD, are accepted
     one_float_outside D = 24, maxD = the float below 24: one float above maxD, refused
   (The boundary is moved against a fixed disparity rather than the parabola bent to land one float beside maxD: at uL ~ 300 that takes SADs of about 12500 on either
   side of the best shift that differ by exactly one, around a corner that FAST still finds at the same pixel of both images.  The comparison sees the same pair of
   neighbouring floats either way.)
   Expected mvuRight / mvDepth / count: the reference's own Frame constructor where oracle/_ref/libref_frame.so is built, and always ol.oracle_stereo and the sequential
   numpy restatement of tests/test_branch_edges_stereo.py, all three bit-equal; the restatement counts the keypoints whose disparity, where it reaches the range test,
   is maxD or a neighbour float: every case asserts at least 5 at its own value, and for at_maxd that their deltaR is 0.

2. `iniu < 0 || endu >= Lw` (src/Frame.cc:1265) at endu == Lw, i.e. a right keypoint whose x, rounded at the left keypoint's level, is Lw - 11.  No input of the library
   reaches it: orbm_stereo_match takes the right keypoints' x from the search records the right EXTRACTION wrote (tests/resident_inject.py: for this consumer only
   descriptors can be injected), and the extractor keeps keypoints at least 17 level pixels from the right border - at most Lw - 13 at a neighbouring level, which
   test_oracle_window_guard_at_the_level_border asserts for this file's extractions.  What the test pins is the checker: ol.oracle_stereo and the numpy restatement on
   hand-built keypoints answer -1 at Lw - 11 (the eleven windows would still lie inside the level: the reference refuses all the same) and a match at Lw - 12."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, ComputeStereoMatches
from orb_slam3_detailed_comments_amd.extractor import KP_DTYPE
from test_branch_edges_stereo import restated_stereo, _flat_rectangles, _noisy_below

W, H, NF = 376, 240, 500
MBF = 3.0
f32 = np.float32
# name: (shift of the right image in pixels, fx = the maxD the reference derives, the counter of the restatement that must reach 5, accepted there?)
CASES = {
    "at_maxd": (24, f32(24), "at_maxd", False),
    "one_px_inside": (23, f32(24), None, True),
    "one_float_inside": (24, np.nextafter(f32(24), f32(np.inf)), "one_float_below", True),
    "one_float_outside": (24, np.nextafter(f32(24), f32(0)), "one_float_above", False),
}


def _moved_left(img, px):
    """the content px pixels further LEFT, as a camera px * mb / mbf to the right sees it: the disparity of every point is px"""
    out = np.full_like(img, 128)
    out[:, :img.shape[1] - px] = img[:, px:]
    return out


_DONE = {}


def _case(name):
    if name not in _DONE:
        shift, fx, counter, accepted = CASES[name]
        flat = _flat_rectangles(1)
        L = _noisy_below(flat, 80, 98); R = _noisy_below(_moved_left(flat, shift), 80, 99)
        mb = f32(MBF) / fx
        assert f32(MBF) / mb == fx, "maxD as Frame.cc computes it (mbf / (mbf / fx)) is not the intended float"
        oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
        (_, kL, dL), (_, kR, dR) = oL.extract(L), oR.extract(R)
        pyrL = [oL.level_image(l) for l in range(8)]; pyrR = [oR.level_image(l) for l in range(8)]
        u, d, entered = restated_stereo(kL, dL, kR, dR, pyrL, pyrR, MBF, mb)
        uo, do, no = ol.oracle_stereo(oL, oR, kL, dL, kR, dR, MBF, float(mb))
        assert uo.tobytes() == u.tobytes() and do.tobytes() == d.tobytes() and no == int((u >= 0).sum()), "the oracle and the numpy restatement disagree"
        if ol.reference_frame_lib() is not None:
            F = ol.ReferenceFrame(L, R, NF, 1.2, 8, 20, 7, 0, fx=float(fx), bf=MBF)
            assert f32(F.mb) == mb and F.keys.tobytes() == kL.tobytes() and F.keys_right.tobytes() == kR.tobytes()
            assert F.u_right.tobytes() == u.tobytes() and F.depth.tobytes() == d.tobytes(), "the reference Frame and the numpy restatement disagree"
        print(name, "keypoints", len(kL), "matched", no, entered)
        # the input reaches the decision
        disp = (kL["x"] - u).astype(f32)
        if counter is None:
            at = (u >= 0) & (disp == f32(shift)) & (kL["octave"] == 0)
            assert shift == int(fx) - 1 and at.sum() >= 5, "level-0 matches exactly one pixel inside the range: %d" % at.sum()
        else:
            assert entered[counter] >= 5, entered
            if name == "at_maxd":
                assert entered["at_maxd_delta_zero"] == entered["at_maxd"] and entered["too_far"] >= entered["at_maxd"]
            at = (kL["octave"] == 0) & (kL["y"] < 70) & (u >= 0) & (disp == f32(shift))
            # accepted: the level-0 keypoints of the clean rows show the whole-pixel disparity; refused: none does (and the other side of the range is not in play)
            assert (at.sum() >= 5) if accepted else (at.sum() == 0), (name, int(at.sum()))
            assert entered["negative"] == 0 and entered["clamp"] == 0
        assert no > 60, "too few matches for a median"
        for a in (u, d):
            a.setflags(write=False)
        _DONE[name] = (L, R, kL, dL, kR, dR, u, d, no, float(mb))
    return _DONE[name]


def _check(lib, name):
    L, R, kL, dL, kR, dR, u_exp, d_exp, n_exp, mb = _case(name)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    try:
        (_, gkL, gdL), (_, gkR, gdR) = ex.extract_batch(np.stack([L, R]))
        assert gkL.tobytes() == kL.tobytes() and gdL.tobytes() == dL.tobytes() and gkR.tobytes() == kR.tobytes() and gdR.tobytes() == dR.tobytes()
        u, d, n = ComputeStereoMatches(ex, ex, MBF, mb, 0, 1, 1)
    finally:
        ex.close()
    N = len(kL)
    bad = np.flatnonzero(u[0, :N].view(np.uint32) != u_exp.view(np.uint32))
    assert len(bad) == 0, "%s: mvuRight differs at %d keypoints, first %d (x %r, octave %d): %r, expected %r" % (
        name, len(bad), bad[0], kL["x"][bad[0]], kL["octave"][bad[0]], u[0, bad[0]], u_exp[bad[0]])
    assert d[0, :N].tobytes() == d_exp.tobytes(), "%s: mvDepth differs" % name
    assert int(n[0]) == n_exp


@pytest.mark.parametrize("name", list(CASES))
def test_stereo_disparity_range_emulated(emu_lib, name):
    _check(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stereo_disparity_range_gpu(hip_lib, name):
    _check(hip_lib, name)


def test_oracle_window_guard_at_the_level_border():
    """src/Frame.cc:1265 on the checker, with hand-built keypoints at level 0 (level width 376): the right keypoint at x = 365 = Lw - 11 is refused although its
    windows end at column 375, the one at 364 is refined to the true match.  And the premise of the unreachability note: no right keypoint of this file's extractions,
    rounded at its own or a neighbouring level, comes nearer to that level's right border than Lw - 13."""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H, W)).astype(np.uint8)
    L = base
    R = np.clip(_moved_left(base, 4).astype(np.int32) + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8)     # (noise: a SAD of 0 would fall to the median test)
    oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
    oL.extract(L); oR.extract(R)
    pyrL = [oL.level_image(l) for l in range(8)]; pyrR = [oR.level_image(l) for l in range(8)]
    Lw = pyrL[0].shape[1]
    assert Lw == W and np.array_equal(pyrL[0], L)
    desc = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    for xr, matched in ((Lw - 11, False), (Lw - 12, True)):
        kL = np.zeros(1, KP_DTYPE); kR = np.zeros(1, KP_DTYPE)
        kL["x"], kL["y"], kL["octave"] = 368.0, 120.0, 0                   # its own window, columns 363 .. 373, lies inside the level
        kR["x"], kR["y"], kR["octave"] = float(xr), 120.0, 0
        u, d, entered = restated_stereo(kL, desc, kR, desc, pyrL, pyrR, 40.0 * 0.11, 0.11)
        uo, do, no = ol.oracle_stereo(oL, oR, kL, desc, kR, desc, 40.0 * 0.11, 0.11)
        assert uo.tobytes() == u.tobytes() and do.tobytes() == d.tobytes()
        if matched:
            assert no == 1 and abs(float(uo[0]) - 364.0) < 0.5 and do[0] > 0, (xr, uo, do)
        else:
            assert no == 0 and uo[0] == -1 and do[0] == -1, (xr, uo, do)
    sf = np.ones(8, f32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * f32(1.2)
    inv = (f32(1.0) / sf).astype(f32)
    for name in CASES:
        kR = _case(name)[4]
        for dl in (-1, 0, 1):
            lv = kR["octave"].astype(np.int64) + dl
            ok = (lv >= 0) & (lv < 8)
            cr = np.floor((kR["x"][ok] * inv[lv[ok]]).astype(f32).astype(np.float64) + 0.5)
            widths = np.array([pyrR[l].shape[1] for l in range(8)])[lv[ok]]
            assert (cr <= widths - 13).all(), (name, dl, int((cr - widths).max()))
