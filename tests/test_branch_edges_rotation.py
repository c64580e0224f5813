"""The rotation histogram of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:2118-2126, :2153-2170, ComputeThreeMaxima
:2335-2377) in the device accept loop (k_lastframe_accept, csrc/k_search.hip) with bin sizes CHOSEN by the test.  Random scenes always leave three well-filled
bins, so the 10 % rule - `(float)max2 < 0.1f * (float)max1` drops the second and third maxima, `(float)max3 < 0.1f * (float)max1` the third - was never entered.

Every frame of the batch is one case.  A case names how many accepted pairs fall into which bin; a pair is a last-frame map point placed exactly on the ray of a
keypoint of the current frame with that keypoint's descriptor (the keypoint is its best candidate at distance 0) and the last-frame angle
angle(keypoint) + 30 bin + 5 degrees.  The cases: one populated bin; the second maximum below, at and above a tenth of the first (30 / 2, 30 / 3, 30 / 4 -
0.1f * 30.0f rounds to 3.0f, so 3 is kept); the same for the third maximum with the second kept; four equal bins, of which the strict `>` keeps the three
with the lowest bin index; and a keypoint that is accepted twice - first by a point without observations (which does not occupy it) in a bin that is then
discarded, then by an observed point in a kept bin: the reference's rotHist holds the keypoint in both bins, so the discarded entry sets it to NULL.

Checked against a sequential restatement (the accepted pairs are those of the reference's run WITHOUT the orientation check; histogram, three maxima and the
reset loop are restated here in float32) and against the reference's own run with the check."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, synth
from orb_slam3_detailed_comments_amd import matcher as M
from test_local_points import _rot

needs_reference_frame = pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so not built (needs /root/reference)")
f32 = np.float32
W, H, NF = 376, 240, 500
FX, FY, CX, CY = 230.0, 230.0, 188.0, 120.0
BF = FX * 0.11

# name -> ([(bin, pairs in it), ...], bins that survive).  rot / 30 only reaches the bins 0 .. 12 of the 30.  "twice": see _scene
CASES = {
    "one_bin":          ([(4, 30)], {4}),
    "second_below":     ([(4, 30), (9, 2)], {4}),
    "second_at":        ([(4, 30), (9, 3)], {4, 9}),
    "second_above":     ([(4, 30), (9, 4)], {4, 9}),
    "third_below":      ([(4, 30), (9, 10), (11, 2)], {4, 9}),
    "third_at":         ([(4, 30), (9, 10), (11, 3)], {4, 9, 11}),
    "third_above":      ([(4, 30), (9, 10), (11, 4)], {4, 9, 11}),
    "second_drops_third": ([(4, 30), (9, 2), (11, 2)], {4}),
    "equal_bins":       ([(7, 10), (3, 10), (10, 10), (5, 10)], {3, 5, 7}),
    "wrap_around":      ([(0, 12), (11, 12), (6, 2)], {0, 6, 11}),
    "twice":            ([(4, 30), (9, 10), (11, 5), (2, 1)], {4, 9, 11}),
}


def restated_bins(last_angle, cur_angle):
    """rot = angle(last) - angle(current), < 0: + 360, bin = round(rot * (1.0f / HISTO_LENGTH)), 30 -> 0 (src/ORBmatcher.cc:2118-2125)"""
    rot = f32(last_angle) - f32(cur_angle)
    if rot < 0:
        rot = rot + f32(360.0)
    b = int(np.floor(np.float64(rot * (f32(1.0) / f32(30))) + 0.5))
    return 0 if b == 30 else b


def restated_three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:2335-2377"""
    max1 = max2 = max3 = 0; ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def restated_histogram(events, assigned_no_check, n_no_check):
    """events: (keypoint, bin) per accepted pair in acceptance order.  The reset loop (:2153-2170): every entry of a bin that is not one of the three maxima sets
    the keypoint to NULL (-2 in the product's output) and takes one match back."""
    sizes = [0] * 30
    for _, b in events:
        sizes[b] += 1
    keep = set(restated_three_maxima(sizes))
    out = assigned_no_check.copy(); n = n_no_check
    for kp, b in events:
        if b not in keep:
            out[kp] = -2; n -= 1
    return out, n, sizes, keep - {-1}


_REF = {}


def _scene():
    """one image, one reference Frame, and per case the last-frame arrays; made once, shared by the emulator and the GPU form"""
    if _REF:
        return _REF
    img = synth.corner_field(W, H, seed=71, nrect=800)
    F = ol.ReferenceFrame(img, img, NF, 1.2, 8, 20, 7, 0, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF)
    N = F.N
    R, t = _rot(0.003, -0.002, 0.004), np.array([0.01, -0.02, 0.015], f32)
    rng = np.random.default_rng(5)
    lonely = np.arange(N)                 # (any keypoint: at descriptor distance 0 it is the best candidate of the point on its ray; asserted in _expected)
    z = rng.uniform(2.0, 6.0, N)
    Xc = np.stack([(F.keys["x"] - CX) / FX * z, (F.keys["y"] - CY) / FY * z, z], 1)
    Xw = ((R.astype(np.float64).T @ (Xc - t.astype(np.float64)).T).T).astype(f32)
    cap = N + 6
    # four more points per case, in front of the camera but projecting left of, right of, above and below the image: each side of the image test of
    # k_lastframe_queries (src/ORBmatcher.cc:2003-2006) rejects one; they take no keypoint
    off_uv = np.array([(-25.0, 100.0), (W + 25.0, 120.0), (150.0, -25.0), (200.0, H + 25.0)])
    off_c = np.stack([(off_uv[:, 0] - CX) / FX * 3.0, (off_uv[:, 1] - CY) / FY * 3.0, np.full(4, 3.0)], 1)
    off_w = ((R.astype(np.float64).T @ (off_c - t.astype(np.float64)).T).T).astype(f32)
    # the input enters what it is made for: restated in float32 (Tcw * x3Dw, Pinhole::project), every one of them lies in front of the camera and fails exactly
    # one side of `u < mnMinX || u > mnMaxX || v < mnMinY || v > mnMaxY` - the first the left one, then right, above, below
    rc = (R.astype(f32) @ off_w.T).T + t.astype(f32)
    ru = f32(FX) * rc[:, 0] / rc[:, 2] + f32(CX); rv = f32(FY) * rc[:, 1] / rc[:, 2] + f32(CY)
    fails = np.stack([ru < f32(0), ru > f32(W), rv < f32(0), rv > f32(H)], 1)
    assert (rc[:, 2] > 0).all() and np.array_equal(fails, np.eye(4, dtype=bool)), (ru, rv)
    cases = {}
    for name, (bins, keep) in CASES.items():
        pos = np.zeros((cap, 3), f32); pos[:N] = Xw
        valid = np.zeros(cap, np.uint8); octave = np.zeros(cap, np.int32); octave[:N] = F.keys["octave"]
        angle = np.zeros(cap, f32); has_obs = np.ones(cap, np.uint8); desc = np.zeros((cap, 32), np.uint8); desc[:N] = F.desc
        chosen = rng.permutation(lonely)[:sum(c for _, c in bins)]
        want = {}
        at = 0
        for b, c in bins:
            for kp in chosen[at:at + c]:
                valid[kp] = 1; want[int(kp)] = b
                angle[kp] = f32((np.float64(F.keys["angle"][kp]) + 30.0 * b + 5.0) % 360.0)
            at += c
        pos[N + 1:N + 5] = off_w; valid[N + 1:N + 5] = 1; desc[N + 1:N + 5] = F.desc[:4]; angle[N + 1:N + 5] = F.keys["angle"][:4]
        n = N + 5
        if name == "twice":
            # the single pair of bin 2 comes from a point WITHOUT observations; a copy of it at the end of the list, observed, in bin 4, takes the same keypoint
            kp = int(chosen[-1]); assert want[kp] == 2
            has_obs[kp] = 0
            pos[N] = pos[kp]; desc[N] = desc[kp]; octave[N] = octave[kp]; valid[N] = 1
            angle[N] = f32((np.float64(F.keys["angle"][kp]) + 30.0 * 4 + 5.0) % 360.0)
        cases[name] = dict(n=n, pos=pos, valid=valid, octave=octave, angle=angle, has_obs=has_obs, desc=desc, want=want, keep=keep)
    _REF.update(F=F, img=img, R=R, t=t, cap=cap, cases=cases)
    return _REF


def _expected(S, name):
    """the reference without and with the orientation check, and the restatement built on the former"""
    c = S["cases"][name]; F = S["F"]; n = c["n"]
    args = (S["R"], S["t"], S["R"], S["t"], c["pos"][:n], c["valid"][:n], c["octave"][:n], c["angle"][:n], c["has_obs"][:n], c["desc"][:n], 7.0, True)
    n0, a0 = F.search_lastframe(*args, False, 0.9, None)[:2]
    n1, a1 = F.search_lastframe(*args, True, 0.9, None)[:2]
    # accepted pairs in acceptance order = ascending point index; a point's keypoint is the one it sits on (asserted through the run without the check)
    events = []
    for i in np.flatnonzero(c["valid"][:F.N + 1]):                 # (the four points beyond are the off-image ones: no pair)
        kp = int(i) if i < F.N else int(np.flatnonzero((c["pos"][:F.N] == c["pos"][i]).all(1))[0])
        events.append((kp, restated_bins(c["angle"][i], F.keys["angle"][kp])))
    assert n0 == len(events) and all(a0[kp] >= 0 for kp, _ in events) and all(a0[i] == i for i in np.flatnonzero(c["valid"][:F.N]) if c["has_obs"][i]), "a pair of the scene is not accepted by the reference"
    exp, n_exp, sizes, keep = restated_histogram(events, a0, n0)
    return (n1, a1), (n_exp, exp), sizes, keep, events


def _check(lib):
    S = _scene(); F = S["F"]; names = list(CASES); B = len(names)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([S["img"]] * B))
    assert res[0][1].tobytes() == F.keys.tobytes() and res[B - 1][2].tobytes() == F.desc.tobytes()
    stack = lambda key: np.stack([S["cases"][nm][key] for nm in names])
    n = np.array([S["cases"][nm]["n"] for nm in names], np.int32)
    lf = M.LastFrameBatch(ex, B, (FX, FY, CX, CY), (0.0, float(W), 0.0, float(H)), BF, ex.GetScaleFactors())
    lf.set_poses([(S["R"], S["t"])] * B)
    lf.enqueue(n, stack("pos"), stack("valid"), stack("octave"), stack("angle"), stack("has_obs"), stack("desc"), 7.0, None, None, True, None, use_u_right=False)
    asg, nm = lf.fetch()
    for b, name in enumerate(names):
        (ref_n, ref_a), (exp_n, exp_a), sizes, keep, events = _expected(S, name)
        c = S["cases"][name]
        print(name, "bins", {i: s for i, s in enumerate(sizes) if s}, "kept", sorted(keep), "matches", exp_n)
        # the input is what the case says, by the restated bins: the sizes, and the bins that survive
        bins, want_keep = CASES[name]
        assert {i: s for i, s in enumerate(sizes) if s} == ({2: 1, 4: 31, 9: 10, 11: 5} if name == "twice" else dict(bins)), name
        assert keep == want_keep, (name, keep)
        assert exp_n == ref_n and np.array_equal(exp_a, ref_a), "%s: the restated histogram differs from the reference's ORBmatcher.cc" % name
        if name == "twice":
            kp = events[-1][0]
            assert events[-1][1] == 4 and ref_a[kp] == -2 and ref_n == 30 + 10 + 5 + 1, "the doubly accepted keypoint: NULL although its second pair is in a kept bin"
        got = asg[b, :F.N]
        assert nm[b] == ref_n, "%s: nmatches %d vs the reference's %d" % (name, nm[b], ref_n)
        assert np.array_equal(got, ref_a), "%s: %d keypoints differ from the reference, e.g. keypoint %d: %d vs %d" % (
            name, int((got != ref_a).sum()), np.flatnonzero(got != ref_a)[0], got[np.flatnonzero(got != ref_a)[0]], ref_a[np.flatnonzero(got != ref_a)[0]])
    ex.close()


@needs_reference_frame
def test_rotation_histogram_ten_percent_rule_emulated(emu_lib):
    _check(emu_lib)


@pytest.mark.gpu
@needs_reference_frame
def test_rotation_histogram_ten_percent_rule_gpu(hip_lib):
    _check(hip_lib)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# The same bin sizes through ORBmatcher::SearchByBoW (src/ORBmatcher.cc:259-493 and :892-1043): the host replay of the single call and k_bow_rotation_prune behind
# the device-resident key frames.  Host-built key frames: a pair of features with one descriptor in one vocabulary node per wanted match (distance 0, every
# other feature of the node is a random descriptor: the ratio test passes), angles angle1 - angle2 = 30 bin + 5 degrees, and 100 unmatched features on each side.
BOW_CASES = {k: v for k, v in CASES.items() if k != "twice"}            # (SearchByBoW gives a keypoint of the second frame away once: no double entries)
SFS = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)


def _bow_pair(bins, seed):
    from orb_slam3_detailed_comments_amd import views
    rng = np.random.default_rng(seed)
    npairs = sum(c for _, c in bins); clutter = 100; N = npairs + clutter
    want = np.concatenate([[b] * c for b, c in bins])
    def frame(desc_pairs, node_pairs, angles):
        k = np.zeros(N, views.KP_DTYPE)
        k["x"] = rng.uniform(20, 350, N); k["y"] = rng.uniform(20, 220, N); k["octave"] = rng.integers(0, 8, N); k["size"] = 31.0; k["class_id"] = -1
        k["angle"][:npairs] = angles; k["angle"][npairs:] = rng.uniform(0, 360, clutter)
        d = np.concatenate([desc_pairs, rng.integers(0, 256, (clutter, 32), dtype=np.uint8)])
        node = np.concatenate([node_pairs, rng.integers(0, 8, clutter)])
        perm = rng.permutation(N)
        k, d, node = np.ascontiguousarray(k[perm]), np.ascontiguousarray(d[perm]), node[perm]
        ids = np.unique(node); order = np.argsort(node, kind="stable")
        start = np.concatenate([[0], np.cumsum([(node == n).sum() for n in ids])]).astype(np.int32)
        return views.key_frame_view(k, d, SFS, (SFS * SFS).astype(f32), ids.astype(np.uint32), start, order.astype(np.uint32), None, np.ones(N, np.uint8)), k, np.argsort(perm)
    dp = rng.integers(0, 256, (npairs, 32), dtype=np.uint8); nd = rng.integers(0, 8, npairs)
    a2 = rng.uniform(0, 360, npairs).astype(f32)
    a1 = np.mod(a2.astype(np.float64) + 30.0 * want + 5.0, 360.0).astype(f32)
    kf1, k1, where1 = frame(dp, nd, a1); kf2, k2, where2 = frame(dp, nd, a2)
    return kf1, kf2, k1, k2, where1[:npairs], where2[:npairs]


def _check_bow(lib):
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    for seed, (name, (bins, want_keep)) in enumerate(BOW_CASES.items()):
        kf1, kf2, k1, k2, i1, i2 = _bow_pair(bins, 40 + seed)
        r1, r2 = M.ResidentKeyFrame(ex, kf1), M.ResidentKeyFrame(ex, kf2)
        flags1, flags2 = kf1.keep[8], kf2.keep[8]
        for frame_version in (True, False):
            n0, m0 = ol.oracle_search_by_bow(kf1, kf2, 0.7, frame_version, False)
            assert n0 == len(i1) and np.array_equal(m0[i1], i2), "%s: the wanted pairs are not what the search accepts without the orientation check" % name
            events = [(int(a), restated_bins(k1["angle"][a], k2["angle"][b])) for a, b in sorted(zip(i1.tolist(), i2.tolist()))]
            exp, n_exp, sizes, keep = restated_histogram(events, m0, n0)
            exp[exp == -2] = -1                                   # (this search clears vpMatches12[idx1])
            assert {i: s for i, s in enumerate(sizes) if s} == dict(bins) and keep == want_keep, (name, sizes, keep)
            n1, m1 = ol.oracle_search_by_bow(kf1, kf2, 0.7, frame_version, True)
            assert n1 == n_exp and np.array_equal(m1, exp), "%s: the restated histogram differs from the oracle's SearchByBoW" % name
            n2, m2 = M.ORBmatcher(0.7, True).SearchByBoW(ex, kf1, kf2, frame_version)
            assert n2 == n_exp and np.array_equal(m2, exp), "%s (frame version %s): single call, %d vs %d matches" % (name, frame_version, n2, n_exp)
            (n3, m3), = M.ORBmatcher(0.7, True).SearchByBoWResident(ex, [r1], [flags1], [r2], [flags2], frame_version)
            assert n3 == n_exp and np.array_equal(m3, exp), "%s (frame version %s): resident key frames, %d vs %d matches" % (name, frame_version, n3, n_exp)
            (n4, m4), = M.ORBmatcher(0.7, True).SearchByBoWBatch(ex, [kf1], [kf2], frame_version)
            assert n4 == n_exp and np.array_equal(m4, exp), "%s (frame version %s): batched call" % (name, frame_version)
        r1.close(); r2.close()
    ex.close()


def test_bow_rotation_prune_ten_percent_rule_emulated(emu_lib):
    _check_bow(emu_lib)


@pytest.mark.gpu
def test_bow_rotation_prune_ten_percent_rule_gpu(hip_lib):
    _check_bow(hip_lib)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# ... and through k_bow_rotation_prune: SearchByBoW(KeyFrame*, Frame&) for the frames of a batch against device-resident key frames
# (orbm_search_by_bow_frames_batch).  One frame per case (the same image); its key frame holds copies of chosen frame features - the same descriptor, hence the
# same vocabulary word and distance 0 - with the angle of the frame's keypoint + 30 bin + 5 degrees.  Checked against the restatement and against the reference's
# own ORBmatcher.cc on a world holding the same key frame and frame (as tests/test_bow_frames_batch.py does).
def _check_bow_frames(lib):
    import os
    import ctypes as C
    import vocab_scenes as vs
    from matcher_world import Driver, KP
    from orb_slam3_detailed_comments_amd import ORBVocabulary, views
    REF = os.path.join(ol.ROOT, "oracle", "_ref", "libmw_ref.so")
    names = list(BOW_CASES); B = len(names)
    rng = np.random.default_rng(15)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    img = synth.corner_field(W, H, seed=71, nrect=800)
    res = ex.extract_batch(np.stack([img] * B))
    k, d = res[0][1], res[0][2]; N = len(k)
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 6, 3)
    voc = ORBVocabulary.from_arrays(ex, header[0], header[1], header[2], header[3], parent, leaf, desc, weight)
    sfs = ex.GetScaleFactors()
    voc.transform_extracted(ex, 0, B, 2)
    bow_f = voc.fetch(ex, 0, N)
    in_a_node = np.unique(np.asarray(bow_f.fv_feat))                              # (features of zero-weight words are in no node)
    unique = np.array([i for i in in_a_node if (d == d[i]).all(1).sum() == 1])
    kfs, mps, worlds = [], [], []
    for name in names:
        bins, _ = BOW_CASES[name]
        src = rng.permutation(unique)[:sum(c for _, c in bins)]
        want = np.concatenate([[b] * c for b, c in bins])
        kk = np.zeros(len(src), KP)
        for f in ("x", "y", "octave", "size"):
            kk[f] = k[f][src]
        kk["angle"] = np.mod(k["angle"][src].astype(np.float64) + 30.0 * want + 5.0, 360.0).astype(f32)
        dk = d[src].copy()
        bow_k = voc.transform(dk, 2)
        has_mp = np.ones(len(src), np.uint8)
        kfs.append(M.ResidentKeyFrame(ex, views.key_frame_view(kk, dk, sfs, sfs * sfs, bow_k.fv_node, bow_k.fv_start, bow_k.fv_feat, None, has_mp))); mps.append(has_mp)
        worlds.append((kk, dk, bow_k, src))
    voc.transform_extracted(ex, 0, B, 2)                                         # (again: the key frames' transforms came in between)
    plain = M.ORBmatcher(0.7, False).SearchByBoWFramesBatch(ex, voc, kfs, mps)
    got = M.ORBmatcher(0.7, True).SearchByBoWFramesBatch(ex, voc, kfs, mps)
    for b, name in enumerate(names):
        bins, want_keep = BOW_CASES[name]
        kk, dk, bow_k, src = worlds[b]
        events = [(i, restated_bins(kk["angle"][i], k["angle"][src[i]])) for i in range(len(src))]
        exp, n_exp, sizes, keep = restated_histogram(events, src.astype(np.int32), len(src))
        exp[exp == -2] = -1
        assert {i: s for i, s in enumerate(sizes) if s} == dict(bins) and keep == want_keep, (name, sizes, keep)
        # the reference's own ORBmatcher.cc, without and with the orientation check
        ref = {}
        if os.path.exists(REF):
            for ori in (0, 1):
                drv = Driver(REF)
                cam = drv.camera()
                I, z3 = np.eye(3, dtype=f32), np.zeros(3, f32)

                def set_fv(keyframe, fid, bow):
                    nodes = np.ascontiguousarray(bow.fv_node, np.uint32); st = np.ascontiguousarray(bow.fv_start, np.int32); ft = np.ascontiguousarray(bow.fv_feat, np.uint32)
                    drv.L.mw_set_feat_vec(drv.w, int(keyframe), fid, len(nodes), nodes.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), ft.ctypes.data_as(C.c_void_p))
                ids = np.array([drv.mappoint(np.array([0, 0, 3.0]), np.array([0, 0, 1.0]), 0.5, 30.0, dk[i]) for i in range(len(kk))], np.int32)
                kf = drv.frame(True, kk, dk, None, I, z3, cam); set_fv(True, kf, bow_k); drv.set_map_points(True, kf, ids)
                kfr = np.zeros(N, KP)
                for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
                    kfr[f] = k[f]
                fr = drv.frame(False, kfr, d, None, I, z3, cam); set_fv(False, fr, bow_f)
                out = np.full(N, -1, np.int32)
                n_ref = drv.L.mw_search_by_bow_frame(drv.w, kf, fr, out.ctypes.data_as(C.c_void_p), C.c_float(0.7), ori)
                drv.close()
                m = np.full(len(kk), -1, np.int32)
                for j in np.flatnonzero(out >= 0):
                    m[np.flatnonzero(ids == out[j])[0]] = j
                ref[ori] = (n_ref, m)
            assert ref[0][0] == len(src) and np.array_equal(ref[0][1], src), "%s: the reference does not accept the wanted pairs" % name
            assert ref[1][0] == n_exp and np.array_equal(ref[1][1], exp), "%s: the restated histogram differs from the reference's ORBmatcher.cc" % name
        assert plain[b][0] == len(src) and np.array_equal(plain[b][1], src), "%s: without the orientation check the wanted pairs are not what the search accepts" % name
        assert got[b][0] == n_exp and np.array_equal(got[b][1], exp), "%s: %d vs %d matches" % (name, got[b][0], n_exp)
    for kf_ in kfs:
        kf_.close()
    voc.close(); ex.close()


def test_bow_frames_rotation_prune_ten_percent_rule_emulated(emu_lib):
    _check_bow_frames(emu_lib)


@pytest.mark.gpu
def test_bow_frames_rotation_prune_ten_percent_rule_gpu(hip_lib):
    _check_bow_frames(hip_lib)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# ... and the two-camera form, k_rig_lastframe_accept (one histogram over both cameras, src/ORBmatcher.cc:2090-2150): fisheye-rig frames, the last frame's
# points on the rays of LEFT keypoints without a stereo partner.  The accepted pairs are read from the oracle restatement's run without the orientation check
# and the case's bin sizes are asserted on them.
RIG_CASES = dict(CASES)


def _check_rig(lib):
    from orb_slam3_detailed_comments_amd import views
    from test_rig_tracking_batch import World, TRL
    from test_local_points_rig import _kb8_unproject
    from test_kb8 import CAM1
    names = list(RIG_CASES); B = len(names)
    Wd = World(lib, 376, 376, 500, (0, 375), B, 1)
    try:
        F = Wd.refs[0]; nl, nr = F.nl, F.nr; N = nl + nr
        rng = np.random.default_rng(23)
        R, t = Wd.poses[0]; Wd.poses = [Wd.poses[0]] * B
        alone = np.flatnonzero(F.l2r < 0)
        capL = 2 * Wd.cap + 3
        n = np.full(B, N, np.int32); pos = np.zeros((B, capL, 3), f32); valid = np.zeros((B, capL), np.uint8); octave = np.zeros((B, capL), np.int32)
        angle = np.zeros((B, capL), f32); has_obs = np.ones((B, capL), np.uint8); desc = np.zeros((B, capL, 32), np.uint8)
        z = rng.uniform(2.0, 6.0, nl)
        Xc = _kb8_unproject(CAM1, F.keys["x"].astype(np.float64), F.keys["y"].astype(np.float64)) * z[:, None]
        Xw = (R.astype(np.float64).T @ (Xc - t.astype(np.float64)).T).T
        pos0 = np.zeros((N, 3), f32); pos0[:nl] = Xw; oct0 = np.zeros(N, np.int32); oct0[:nl] = F.keys["octave"]; d0 = np.zeros((N, 32), np.uint8); d0[:nl] = F.desc[:nl]

        def pairs_in_camera_2(points):
            """the points of `points` that, offered together, also take a keypoint of camera 2 (the oracle without the orientation check)"""
            v0 = np.zeros(N, np.uint8); v0[points] = 1
            pr = M.ProjectPoints(Wd.exL, Wd.poses[0], CAM1, Wd.bounds, pos0, skip=1 - v0, depth_test=2, bounds_mode=0)
            p2 = M.ProjectPoints(Wd.exL, Wd.poses[0], CAM1, Wd.bounds, pos0, skip=1 - v0, second=TRL, depth_test=0, bounds_mode=2)
            last0 = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], oct0, np.zeros(N, f32), np.ones(N, np.uint8), d0)
            _, a_all = ol.oracle_search_by_projection_frame_fisheye(Wd.frame2(0), last0, p2["u"], p2["v"], 7.0, 0, 0, False)
            return set(a_all[nl:][a_all[nl:] >= 0].tolist()) | {int(q) for q in points if a_all[q] != q}      # ... or do not take their own keypoint
        alone = np.setdiff1d(alone, sorted(pairs_in_camera_2(alone)))
        assert len(alone) >= 60, len(alone)
        for b, name in enumerate(names):
            bins, _ = RIG_CASES[name]
            pool = rng.permutation(alone).tolist(); need = sum(c for _, c in bins)
            chosen, pool = pool[:need], pool[need:]
            for _ in range(8):                         # a second pair in camera 2 would be an entry the case does not name: such points are exchanged
                second = pairs_in_camera_2(chosen)
                if not second:
                    break
                chosen = [pool.pop() if c in second else c for c in chosen]
            chosen = np.array(chosen)
            want = np.concatenate([[bb] * c for bb, c in bins])
            pos[b, :nl] = Xw; octave[b, :nl] = F.keys["octave"]; desc[b, :nl] = F.desc[:nl]
            valid[b, chosen] = 1
            angle[b, chosen] = np.mod(F.keys["angle"][chosen].astype(np.float64) + 30.0 * want + 5.0, 360.0).astype(f32)
            if name == "twice":                        # as in _scene: the single pair of bin 2 comes from a point without observations, an observed copy in row N (bin 4) follows
                kp = int(chosen[-1]); assert want[-1] == 2
                has_obs[b, kp] = 0
                pos[b, N] = pos[b, kp]; desc[b, N] = desc[b, kp]; octave[b, N] = octave[b, kp]; valid[b, N] = 1; n[b] = N + 1
                angle[b, N] = f32((np.float64(F.keys["angle"][kp]) + 30.0 * 4 + 5.0) % 360.0)
                twice_kp = kp
        lf = M.LastFrameRigBatch(Wd.exL, Wd.exR, B, CAM1, Wd.bounds, Wd.sfs, Wd.lf, Wd.rf)
        lf.set_poses(Wd.poses, TRL)
        lf.enqueue(n, pos, valid, octave, angle, has_obs, desc, 7.0, np.zeros(B, np.uint8), np.zeros(B, np.uint8), True, None)
        asg, nm = lf.fetch()
        kp_angle = np.concatenate([F.keys["angle"], F.keys_right["angle"]])
        for b, name in enumerate(names):
            bins, want_keep = RIG_CASES[name]
            nb = int(n[b])
            sk = 1 - valid[b, :nb]
            pr = M.ProjectPoints(Wd.exL, Wd.poses[b], CAM1, Wd.bounds, pos[b, :nb], skip=sk, depth_test=2, bounds_mode=0)
            p2 = M.ProjectPoints(Wd.exL, Wd.poses[b], CAM1, Wd.bounds, pos[b, :nb], skip=sk, second=TRL, depth_test=0, bounds_mode=2)
            last = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], octave[b, :nb], angle[b, :nb], has_obs[b, :nb], desc[b, :nb])
            cur2 = Wd.frame2(b)
            n0, a0 = ol.oracle_search_by_projection_frame_fisheye(cur2, last, p2["u"], p2["v"], 7.0, 0, 0, False)
            n1, a1 = ol.oracle_search_by_projection_frame_fisheye(cur2, last, p2["u"], p2["v"], 7.0, 0, 0, True)
            events = sorted((int(a0[kp]), int(kp)) for kp in np.flatnonzero(a0 >= 0))                     # acceptance order: by point, camera 1 before camera 2
            if name == "twice":                        # the keypoint holds the later point; the unobserved one's pair came first (the single-frame oracle's order)
                assert a0[twice_kp] == N and n0 == len(events) + 1
                events = sorted(events + [(twice_kp, twice_kp)])
            events = [(kp, restated_bins(angle[b, i], kp_angle[kp])) for i, kp in events]
            exp, n_exp, sizes, keep = restated_histogram(events, a0, n0)
            print(name, "bins", {i: s for i, s in enumerate(sizes) if s}, "kept", sorted(keep), "pairs in camera 2:", int((a0[nl:] >= 0).sum()))
            assert {i: s for i, s in enumerate(sizes) if s} == ({2: 1, 4: 31, 9: 10, 11: 5} if name == "twice" else dict(bins)) and keep == want_keep, (name, sizes, keep)
            if name == "twice":
                assert exp[twice_kp] == -2 and n_exp == 46, "the doubly accepted keypoint: NULL although its second pair is in a kept bin"
            assert n1 == n_exp and np.array_equal(a1, exp), "%s: the restated histogram differs from the oracle" % name
            assert nm[b] == n_exp and np.array_equal(asg[b, :N], exp), "%s: %d vs %d matches" % (name, nm[b], n_exp)
            one_n, one_as = M.ORBmatcher(0.9, True).SearchByProjectionFrameFisheye(Wd.exL, cur2, last, p2["u"], p2["v"], 7.0, False, False)
            assert one_n == n_exp and np.array_equal(one_as, exp), "%s: single-frame call" % name
    finally:
        Wd.close()


@needs_reference_frame
def test_rig_rotation_histogram_ten_percent_rule_emulated(emu_lib):
    _check_rig(emu_lib)


@pytest.mark.gpu
@needs_reference_frame
def test_rig_rotation_histogram_ten_percent_rule_gpu(hip_lib):
    _check_rig(hip_lib)
