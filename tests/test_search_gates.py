"""The float gates of Tracking::SearchLocalPoints on the device (csrc/k_search.hip: frustum_body, area_accept) at the values where they decide - the survivors of the
mutation pass recorded in profiles/emu_mutants/README.md in those two functions.  Random scenes never put a projection ON the image border or a viewing
cosine ON its limit; here the inputs are made for it, and every case has its neighbour one float on the other side.

frustum (expected: the reference's own Frame::isInFrustum + ORBmatcher::SearchByProjection, oracle/_ref/libref_frame.so):
  border     camera fx = cx = 188, fy = cy = 120 on a 376 x 240 image, identity pose: the points (Z, 0, Z), (-Z, 0, Z), (0, Z, Z), (0, -Z, Z) project to u = 376 = mnMaxX,
             u = 0 = mnMinX, v = 240 = mnMaxY, v = 0 = mnMinY without rounding (188 Z and 120 Z are exact for the Z used, and so are the quotients).  src/Frame.cc:700-703
             rejects `u < mnMinX || u > mnMaxX`: the border itself is inside.  Their neighbours (the coordinate a few floats larger in magnitude) are outside.
  cos        viewingCosLimit set to the viewing cosine that the reference reports for a matched point (:744 `viewCos < viewingCosLimit` keeps it), then to the float above
  far        thFarPoints set to the depth that the reference reports for a matched point (src/ORBmatcher.cc:57 `mTrackDepth > thFarPoints` keeps it), then to the float below
  radius     RadiusByViewingCos (src/ORBmatcher.cc:242-249) compares the FLOAT viewCos with the DOUBLE literal 0.998: the float nearest to 0.998 lies above it and takes
             the small radius 2.5, a float comparison would not.  A point on the optical axis at distance 1 with the "normal" (0, 0, c) has viewCos == c exactly; the camera's
             principal point is put 3.25 px beside a level-0 keypoint, whose descriptor the point carries: inside the radius 4, outside 2.5.  c = float(0.998) and the float below.
area (expected: the oracle's SearchByProjection on the tracking fields, as tests/test_branch_edges_search.py does - the reference Frame computes its own mvuRight):
  ur_zero    src/ORBmatcher.cc:107 `if (F.mvuRight[idx] > 0)`: a keypoint whose right coordinate is exactly 0 is NOT gated
  ur_on      :110 `if (er > r) continue`: a keypoint whose right coordinate is exactly r beside the projected one is kept, one float further it is not
Each case asserts on the reference's / oracle's own outputs that its input sits where it was aimed."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, ComputeStereoMatches, synth, views
from orb_slam3_detailed_comments_amd import matcher as M

pytestmark = pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so not built (needs /root/reference)")
W, H, NF = 376, 240, 500
FX, FY, CX, CY = 188.0, 120.0, 188.0, 120.0
BF = FX * 0.11
f32 = np.float32
I3, T0 = np.eye(3, dtype=f32), np.zeros(3, f32)
NGEN = 300


def _up(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


def _down(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(-np.inf))
    return x


def _generic(keys, desc, rng, n, cam):
    """n map points on the rays of random keypoints (their descriptors, their octave's distance range), normals tilted so that the viewing cosines spread"""
    fx, fy, cx, cy = cam
    src = rng.integers(0, len(keys), n); z = rng.uniform(2, 8, n)
    X = np.stack([(keys["x"][src] + rng.normal(0, 0.5, n) - cx) / fx * z, (keys["y"][src] + rng.normal(0, 0.5, n) - cy) / fy * z, z], 1).astype(f32)
    dist = np.linalg.norm(X.astype(np.float64), axis=1)
    nrm = X / dist[:, None] + rng.normal(0, 0.35, (n, 3)); nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    maxd = (dist * 1.2 ** keys["octave"][src] * rng.uniform(0.9, 1.1, n)).astype(f32)
    return X, nrm.astype(f32), (maxd / f32(1.2 ** 7)).astype(f32), maxd, desc[src].copy()


def _border_points():
    """(points, kind): on the four borders and just outside each, three depths"""
    pts, kind = [], []
    for Z in (2.0, 3.0, 5.0):
        for axis, sign, name in ((0, 1, "max_x"), (0, -1, "min_x"), (1, 1, "max_y"), (1, -1, "min_y")):
            for steps, where in ((0, "on"), (3, "outside")):
                p = [0.0, 0.0, Z]; p[axis] = float(sign * _up(Z, steps))
                pts.append(p); kind.append((name, where))
    return np.array(pts, f32), kind


_DONE = {}


def _base():
    if "base" not in _DONE:
        L, R = synth.stereo_pair(W, H, seed=31, nrect=800)
        F = ol.ReferenceFrame(L, R, NF, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF)
        assert F.N > 300
        _DONE["base"] = (L, R, F)
    return _DONE["base"]


def _frustum_case():
    """the scene and the reference's answers for (cos_limit, th_far) = defaults, both on their boundaries, both one float past them"""
    if "frustum" not in _DONE:
        L, R, F = _base()
        rng = np.random.default_rng(5)
        X, nrm, mind, maxd, desc = _generic(F.keys, F.desc, rng, NGEN, (FX, FY, CX, CY))
        B, kind = _border_points()
        bd = np.linalg.norm(B.astype(np.float64), axis=1)
        pos = np.concatenate([X, B]); normal = np.concatenate([nrm, (B / bd[:, None]).astype(f32)])
        mind = np.concatenate([mind, (0.1 * bd).astype(f32)]); maxd = np.concatenate([maxd, (2.0 * bd).astype(f32)])
        desc = np.concatenate([desc, rng.integers(0, 256, (len(B), 32), dtype=np.uint8)])
        Mp = len(pos)
        bad = np.zeros(Mp, bool); obs = np.ones(Mp, bool)
        ref = lambda cos, far: F.search_local_points(I3, T0, pos, normal, mind, maxd, bad, obs, desc, float(cos), True, 3.0, True, float(far), 0.8)
        tr0, as0, n0 = ref(0.5, 1e9)
        # the border points sit where they were aimed: on the border -> in view with the border's coordinate, outside -> rejected (mTrackProjX stays -1)
        bound = dict(max_x=("proj_x", f32(W)), min_x=("proj_x", f32(0)), max_y=("proj_y", f32(H)), min_y=("proj_y", f32(0)))
        for i, (name, where) in enumerate(kind):
            key, val = bound[name]
            if where == "on":
                assert tr0["in_view"][NGEN + i] and tr0[key][NGEN + i] == val, (name, where, tr0[key][NGEN + i])
            else:
                assert not tr0["in_view"][NGEN + i], (name, where)
        # a matched point for each of the two parameter gates
        matched = [int(p) for p in as0[as0 >= 0] if p < NGEN]
        pick = [p for p in matched if 0.55 < tr0["view_cos"][p] < 0.99 and tr0["in_view"][p]]
        assert n0 > NGEN // 4 and len(pick) >= 2, (n0, len(pick))
        i_cos, j_far = pick[0], pick[-1]
        cos_on, far_on = f32(tr0["view_cos"][i_cos]), f32(tr0["depth"][j_far])
        runs = [("defaults", 0.5, 1e9, tr0, as0, n0)]
        tr1, as1, n1 = ref(cos_on, far_on)
        assert tr1["in_view"][i_cos] and (as1 == i_cos).any() and (as1 == j_far).any(), "on their boundaries both points are still searched and matched"
        runs.append(("on", cos_on, far_on, tr1, as1, n1))
        tr2, as2, n2 = ref(_up(cos_on), _down(far_on))
        assert not tr2["in_view"][i_cos] and not (as2 == i_cos).any() and tr2["in_view"][j_far] and not (as2 == j_far).any(), "one float past them neither is matched"
        runs.append(("past", _up(cos_on), _down(far_on), tr2, as2, n2))
        _DONE["frustum"] = (pos, normal, mind, maxd, bad, obs, desc, runs)
    return _DONE["frustum"]


def _frame_of(lib, F, L, R, bf):
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    (_, kL, dL), _ = ex.extract_batch(np.stack([L, R]))
    u, _, _ = ComputeStereoMatches(ex, ex, bf, F.mb, 0, 1, 1)
    assert kL.tobytes() == F.keys.tobytes() and u[0, :F.N].tobytes() == F.u_right.tobytes()
    return ex, kL, dL, u[0, :F.N].copy()


def _same_tracks(tr, ref_tr, what):
    inv = ref_tr["in_view"]
    assert np.array_equal(tr["in_view"].astype(bool), inv), "%s: mbTrackInView differs at points %s" % (what, np.flatnonzero(tr["in_view"].astype(bool) != inv)[:8])
    for k in ("proj_x", "proj_y"):
        assert tr[k].tobytes() == ref_tr[k].tobytes(), (what, k)
    for k in ("proj_xr", "depth", "view_cos"):
        assert tr[k][inv].tobytes() == ref_tr[k][inv].tobytes(), (what, k)
    assert np.array_equal(tr["scale_level"][inv], ref_tr["scale_level"][inv]), what


def _check_frustum(lib):
    L, R, F = _base()
    pos, normal, mind, maxd, bad, obs, desc, runs = _frustum_case()
    ex, kL, dL, u = _frame_of(lib, F, L, R, BF)
    try:
        sfs = ex.GetScaleFactors()
        fv = views.frame_view(kL, dL, sfs, W, H, u_right=u, mbf=BF)
        for what, cos, far, ref_tr, ref_as, ref_n in runs:
            tr, asg, n = M.SearchLocalPoints(ex, fv, I3, T0, (FX, FY, CX, CY), (0.0, float(W), 0.0, float(H)), BF, sfs, pos, normal, mind, maxd, bad, obs, desc,
                                             float(cos), 3.0, True, float(far), 0.8)
            _same_tracks(tr, ref_tr, what)
            assert n == ref_n and np.array_equal(asg, ref_as), "%s: SearchByProjection assignment differs (%d vs %d matches) at keypoints %s" % (
                what, n, ref_n, np.flatnonzero(asg != ref_as)[:8])
    finally:
        ex.close()


def _radius_case():
    if "radius" not in _DONE:
        L, R, F0 = _base()
        # a level-0 keypoint without right coordinate (no right-coordinate gate), away from the border, with no other keypoint of levels 0 near the principal point to be
        k0 = None
        for k in np.flatnonzero((F0.keys["octave"] == 0) & (F0.u_right < 0) & (F0.keys["x"] > 40) & (F0.keys["x"] < W - 40)):
            cx, cy = F0.keys["x"][k] + f32(3.25), F0.keys["y"][k]
            near = (np.abs(F0.keys["x"] - cx) < 4.5) & (np.abs(F0.keys["y"] - cy) < 4.5) & (F0.keys["octave"] == 0)
            if near.sum() == 1 and near[k]:
                k0 = int(k); break
        assert k0 is not None
        cx, cy = float(F0.keys["x"][k0] + f32(3.25)), float(F0.keys["y"][k0])
        F = ol.ReferenceFrame(L, R, NF, fx=FX, fy=FX, cx=cx, cy=cy, bf=BF)
        assert F.keys.tobytes() == F0.keys.tobytes() and F.u_right.tobytes() == F0.u_right.tobytes()
        c_on = f32(0.998)
        assert float(c_on) > 0.998 > float(_down(c_on)), "the float nearest to 0.998 lies above the double literal"
        pos = np.array([[0, 0, 1], [0, 0, 1]], f32); normal = np.array([[0, 0, c_on], [0, 0, _down(c_on)]], f32)
        mind = np.full(2, 0.5, f32); maxd = np.ones(2, f32)
        desc = np.stack([F.desc[k0], F.desc[k0]])
        bad = np.zeros(2, bool); obs = np.ones(2, bool)
        tr, asg, n = F.search_local_points(I3, T0, pos, normal, mind, maxd, bad, obs, desc, 0.5, True, 1.0, False, 50.0, 0.8)
        assert tr["in_view"].all() and tr["view_cos"][0] == c_on and tr["view_cos"][1] == _down(c_on) and (tr["scale_level"] == 0).all()
        assert tr["proj_x"][0] == f32(cx) and tr["proj_y"][0] == f32(cy)
        assert n == 1 and asg[k0] == 1, "the point at float(0.998) searches 2.5 px and misses the keypoint 3.25 px away, the one below searches 4 px and takes it"
        _DONE["radius"] = (F, (FX, FX, cx, cy), pos, normal, mind, maxd, bad, obs, desc, tr, asg, n)
    return _DONE["radius"]


def _check_radius(lib):
    L, R, _ = _base()
    F, cam, pos, normal, mind, maxd, bad, obs, desc, ref_tr, ref_as, ref_n = _radius_case()
    ex, kL, dL, u = _frame_of(lib, F, L, R, BF)
    try:
        sfs = ex.GetScaleFactors()
        fv = views.frame_view(kL, dL, sfs, W, H, u_right=u, mbf=BF)
        tr, asg, n = M.SearchLocalPoints(ex, fv, I3, T0, cam, (0.0, float(W), 0.0, float(H)), BF, sfs, pos, normal, mind, maxd, bad, obs, desc, 0.5, 1.0, False, 50.0, 0.8)
        _same_tracks(tr, ref_tr, "radius")
        assert n == ref_n and np.array_equal(asg, ref_as), "RadiusByViewingCos at float(0.998): keypoints %s" % np.flatnonzero(asg != ref_as)
    finally:
        ex.close()


def _check_right_coordinate(lib):
    """ur_zero and ur_on: the frustum scene's matched points, the right coordinates of their keypoints rewritten in the frame view"""
    L, R, F = _base()
    pos, normal, mind, maxd, bad, obs, desc, runs = _frustum_case()
    _, _, _, tr0, as0, _ = runs[0]
    ex, kL, dL, u = _frame_of(lib, F, L, R, BF)
    try:
        sfs = np.asarray(ex.GetScaleFactors(), f32)
        pairs = [(int(k), int(as0[k])) for k in np.flatnonzero(as0 >= 0) if as0[k] < NGEN]
        assert len(pairs) >= 12
        radius = lambda p: f32((2.5 if float(tr0["view_cos"][p]) > 0.998 else 4.0)) * f32(3.0) * sfs[tr0["scale_level"][p]]

        def ur_on(p):
            """a float ur > 0 with |xr - ur| == r in float arithmetic, or None (the difference of two floats near 80 has a coarser grid than r)"""
            xr, r = f32(tr0["proj_xr"][p]), radius(p)
            for ur in (f32(xr - r), f32(xr + r)):
                for _ in range(4):
                    er = f32(abs(f32(xr - ur)))
                    if er == r:
                        return ur if ur > 0 else None
                    ur = (_up(ur) if er < r else _down(ur)) if ur > xr else (_down(ur) if er < r else _up(ur))
            return None

        hit = [(k, p, ur_on(p)) for k, p in pairs]
        exact = [(k, p, ur) for k, p, ur in hit if ur is not None]
        assert len(exact) >= 8, "points whose radius is a representable difference: %d" % len(exact)
        on, past = exact[0:4], exact[4:8]
        zero = [(k, p) for k, p, ur in hit if ur is None][:4]
        assert len(zero) >= 3
        u2 = u.copy()
        for k, p in zero:
            u2[k] = 0.0
            assert abs(tr0["proj_xr"][p]) > 50, "the projected right coordinate is far from 0: a gate on ur == 0 would refuse the keypoint"
        for k, p, ur in on:
            u2[k] = ur
        for k, p, ur in past:
            xr, r = f32(tr0["proj_xr"][p]), radius(p)
            out = _up(ur) if ur > xr else _down(ur)                       # one float further from xr: the difference is the next one on its grid, above r
            assert f32(abs(f32(xr - out))) > r and out > 0
            u2[k] = out
        on, past = [(k, p) for k, p, _ in on], [(k, p) for k, p, _ in past]
        fv = views.frame_view(kL, dL, sfs, W, H, u_right=u2, mbf=BF)
        tr, asg, n = M.SearchLocalPoints(ex, fv, I3, T0, (FX, FY, CX, CY), (0.0, float(W), 0.0, float(H)), BF, sfs, pos, normal, mind, maxd, bad, obs, desc, 0.5, 3.0, False, 50.0, 0.8)
        _same_tracks(tr, tr0, "right coordinate")
        mps = views.map_point_view(tr0["in_view"], tr0["proj_x"], tr0["proj_y"], tr0["proj_xr"], tr0["scale_level"], tr0["view_cos"], tr0["depth"], bad, obs, desc)
        n2, a2 = ol.oracle_search_by_projection_mappoints(fv, mps, 3.0, False, 50.0, 0.8)
        # the oracle keeps the keypoints at ur == 0 and at |er| == r for their points and lets go of those one float further
        assert all(a2[k] == p for k, p in zero + on), [(k, p, a2[k]) for k, p in zero + on]
        assert all(a2[k] != p for k, p in past), [(k, p, a2[k]) for k, p in past]
        assert n == n2 and np.array_equal(asg, a2), "right-coordinate gate: %d vs %d matches, keypoints %s" % (n, n2, np.flatnonzero(asg != a2)[:8])
    finally:
        ex.close()


def test_frustum_gates_on_their_boundaries_emulated(emu_lib):
    _check_frustum(emu_lib)


@pytest.mark.gpu
def test_frustum_gates_on_their_boundaries_gpu(hip_lib):
    _check_frustum(hip_lib)


def test_radius_by_viewing_cos_at_float_0998_emulated(emu_lib):
    _check_radius(emu_lib)


@pytest.mark.gpu
def test_radius_by_viewing_cos_at_float_0998_gpu(hip_lib):
    _check_radius(hip_lib)


def test_right_coordinate_gate_on_its_boundaries_emulated(emu_lib):
    _check_right_coordinate(emu_lib)


@pytest.mark.gpu
def test_right_coordinate_gate_on_its_boundaries_gpu(hip_lib):
    _check_right_coordinate(hip_lib)


def _rig_far_case():
    """the rig form of `far` (src/ORBmatcher.cc:57 with the rig's mTrackDepth): thFarPoints set to the camera-1 depth the reference reports for a matched point, then to the float below"""
    if "rig" not in _DONE:
        from test_kb8 import CAM1, CAM2, RLR, TLR, _fisheye_pair
        from test_local_points import _rot
        from test_local_points_rig import _scene
        rng = np.random.default_rng(131)
        w = h = 376
        L, R = _fisheye_pair(31, w, h)
        F = ol.ReferenceRigFrame(L, R, (0, 375), (0, 375), 500, (CAM1, CAM2, RLR, TLR))
        Rcw = _rot(0.015, -0.02, 0.01); tcw = np.array([0.2, -0.05, 0.15], f32)
        scene = _scene(F, rng, Rcw, tcw, 600)
        ref = lambda far: F.search_local_points(Rcw, tcw, *scene, 0.5, True, 3.0, True, float(far), 0.8)
        rl, rr, as0, n0, pose = ref(9.0)
        # a point that camera 2 matched (slots behind Nleft: the second pass of the search decides `far` on its own, src/ORBmatcher.cc:170-176) and camera 1 saw
        right = as0[F.nl:]
        matched = [int(p) for p in right[right >= 0] if rl["in_view"][p] and rl["depth"][p] < 9.0]
        assert len(matched) > 10
        j = matched[len(matched) // 2]
        far_on = f32(rl["depth"][j])
        runs = []
        for what, far, kept in (("on", far_on, True), ("past", _down(far_on), False)):
            r = ref(far)
            assert (r[2][F.nl:] == j).any() == kept, "thFarPoints %s the point's depth: matched by camera 2 %s" % (what, (r[2][F.nl:] == j).any())
            runs.append((what, float(far), r))
        _DONE["rig"] = (L, R, F, (CAM1, CAM2), scene, runs)
    return _DONE["rig"]


def _check_rig_far(lib):
    L, R, F, (cam1, cam2), scene, runs = _rig_far_case()
    w = h = 376
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    try:
        (mL, kL, dL), (mR, kR, dR) = ex.extract_batch(np.stack([L, R]), (0, 375))
        assert kL.tobytes() == F.keys.tobytes() and kR.tobytes() == F.keys_right.tobytes()
        sfs = ex.GetScaleFactors()
        f2 = views.fisheye_frame_view(views.frame_view(kL, dL, sfs, w, h), views.frame_view(kR, dR, sfs, w, h), F.l2r, F.r2l)
        for what, far, (rl, rr, ref_as, ref_n, pose) in runs:
            tl, tr, asg, n = M.SearchLocalPointsRig(ex, f2, pose, cam1, cam2, (0.0, float(w), 0.0, float(h)), sfs, *scene, 0.5, 3.0, True, far, 0.8)
            assert np.array_equal(tl["in_view"].astype(bool), rl["in_view"]) and np.array_equal(tr["in_view_r"].astype(bool), rr["in_view_r"])
            assert n == ref_n and np.array_equal(asg, ref_as), "rig, thFarPoints %s a point's depth: %d vs %d matches at slots %s" % (what, n, ref_n, np.flatnonzero(asg != ref_as)[:8])
        # the batched form (k_frustum_rig decides `far` on the device): one frame
        from test_rig_tracking_batch import MRLR, TLR
        M.ComputeStereoFishEyeMatches(ex, ex, cam1, cam2, MRLR, TLR, 0, 1, 1)
        pos, normal, mind, maxd, bad, obs, desc = scene
        rp = M.ResidentPoints(ex, pos, normal, mind, maxd, desc)
        lp = M.LocalPointsRigBatch(ex, ex, rp, 1, cam1, cam2, (0.0, float(w), 0.0, float(h)), sfs, 0, 1)
        for what, far, (rl, rr, ref_as, ref_n, pose) in runs:
            lp.set_poses([pose])
            lp.enqueue(is_bad=bad, has_obs=obs, th=3.0, far_points=True, th_far=far, nnratio=0.8, want_in_view=True)
            asg, nm, iv, ivr = lp.fetch()
            assert np.array_equal(iv[0].astype(bool), rl["in_view"]) and np.array_equal(ivr[0].astype(bool), rr["in_view_r"])
            assert nm[0] == ref_n and np.array_equal(asg[0, :F.nl + F.nr], ref_as), "rig batch, thFarPoints %s a point's depth: %d vs %d matches" % (what, nm[0], ref_n)
        rp.close()
    finally:
        ex.close()


def test_rig_far_points_on_the_boundary_emulated(emu_lib):
    _check_rig_far(emu_lib)


@pytest.mark.gpu
def test_rig_far_points_on_the_boundary_gpu(hip_lib):
    _check_rig_far(hip_lib)


def _rig_ratio_case():
    """camera 2's ratio test of the rig search (src/ORBmatcher.cc:206-212) ON its line: `bestDist > mfNNratio * bestDist2` with float(0.8) * 50 == 40.0f.  Two camera-2
    keypoints of one octave a few pixels apart; the point projects between them and carries a descriptor 40 bits from the first and 50 from the second (bits flipped
    where the two agree and where they differ), so the best is not above 0.8 times the second and the point is matched; at 41 / 50 it is not."""
    if "rig_ratio" not in _DONE:
        from test_kb8 import CAM1, CAM2, RLR, TLR, _fisheye_pair
        from test_local_points import _rot
        from test_local_points_rig import _scene, _kb8_unproject
        rng = np.random.default_rng(178)
        w = h = 376
        L, R = _fisheye_pair(31, w, h)
        F = ol.ReferenceRigFrame(L, R, (0, 375), (0, 375), 500, (CAM1, CAM2, RLR, TLR))
        kr, dr = F.keys_right, F.desc[F.nl:]
        Rcw = _rot(0.015, -0.02, 0.01); tcw = np.array([0.2, -0.05, 0.15], f32)
        # the pair: same octave, both inside the smaller camera-2 window (2.5 x the scale of the predicted level, octave + 1) around their midpoint, descriptors an even
        # number of bits, 10 .. 90, apart.  (That no third keypoint competes is asserted below on the distances themselves.)
        Hd = np.unpackbits(dr[:, None, :] ^ dr[None, :, :], axis=2).sum(2)
        sf = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
        pair = None
        for a in range(len(kr)):
            for b in range(a + 1, len(kr)):
                o = int(kr["octave"][a])
                if o == kr["octave"][b] and o < 7 and 10 <= Hd[a, b] <= 90 and Hd[a, b] % 2 == 0 \
                        and max(abs(kr["x"][a] - kr["x"][b]), abs(kr["y"][a] - kr["y"][b])) / 2 < 0.8 * 2.5 * sf[o + 1]:
                    pair = (a, b); break
            if pair:
                break
        assert pair is not None
        a, b = pair
        hd = int(Hd[a, b]); octv = int(kr["octave"][a])
        differ = np.flatnonzero(np.unpackbits(dr[a] ^ dr[b])); agree = np.flatnonzero(np.unpackbits(dr[a] ^ dr[b]) == 0)

        def descriptor(d1):
            """d1 bits from keypoint a, 50 from keypoint b: n_d flips where they differ, d1 - n_d where they agree, hd - n_d + d1 - n_d = 50"""
            n_d = (hd + d1 - 50) // 2
            assert (hd + d1 - 50) % 2 == 0 and 0 <= n_d <= min(hd, d1)
            bits = np.unpackbits(dr[a]).copy()
            for p in list(rng.choice(differ, n_d, replace=False)) + list(rng.choice(agree, d1 - n_d, replace=False)):
                bits[p] ^= 1
            return np.packbits(bits)
        z = 3.0
        ray = _kb8_unproject(CAM2, np.array([(kr["x"][a] + kr["x"][b]) / 2], np.float64), np.array([(kr["y"][a] + kr["y"][b]) / 2], np.float64))[0] * z
        Xc = RLR.astype(np.float64) @ ray + TLR.astype(np.float64)
        Rw = Rcw.astype(np.float64); Xw = Rw.T @ (Xc - tcw.astype(np.float64)); Ow = -(Rw.T @ tcw.astype(np.float64))
        dist = np.linalg.norm(Xw - Ow)
        runs = []
        for what, d1, kept in (("on", 40, True), ("past", 42, False)):
            D = descriptor(d1)
            da = np.unpackbits(D[None, :] ^ dr, axis=1).sum(1)
            order = np.argsort(da, kind="stable")
            assert da[a] == d1 and da[b] == 50 and set(order[:2].tolist()) == {a, b} and da[order[2]] > 60, "best and second best of the window"
            scene = list(_scene(F, np.random.default_rng(5), Rcw, tcw, 300))
            scene[0][0] = Xw; scene[1][0] = (Xw - Ow) / dist; scene[3][0] = dist * 1.2 ** (octv + 0.5); scene[2][0] = scene[3][0] / f32(1.2 ** 7)
            scene[4][0] = False; scene[5][0] = True; scene[6][0] = D
            r = F.search_local_points(Rcw, tcw, *scene, 0.5, True, 1.0, False, 50.0, 0.8)
            assert r[1]["in_view_r"][0] and r[1]["scale_level_r"][0] == octv + 1
            assert (r[2][F.nl + a] == 0) == kept, "camera 2, best %d against 0.8 * 50: matched %s" % (d1, r[2][F.nl + a] == 0)
            runs.append((what, scene, r))
        _DONE["rig_ratio"] = (L, R, F, (CAM1, CAM2), runs)
    return _DONE["rig_ratio"]


def _check_rig_ratio(lib):
    from test_rig_tracking_batch import MRLR, TLR
    L, R, F, (cam1, cam2), runs = _rig_ratio_case()
    w = h = 376
    bounds = (0.0, float(w), 0.0, float(h))
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    try:
        (mL, kL, dL), (mR, kR, dR) = ex.extract_batch(np.stack([L, R]), (0, 375))
        assert kL.tobytes() == F.keys.tobytes() and kR.tobytes() == F.keys_right.tobytes()
        sfs = ex.GetScaleFactors()
        f2 = views.fisheye_frame_view(views.frame_view(kL, dL, sfs, w, h), views.frame_view(kR, dR, sfs, w, h), F.l2r, F.r2l)
        M.ComputeStereoFishEyeMatches(ex, ex, cam1, cam2, MRLR, TLR, 0, 1, 1)
        for what, scene, (rl, rr, ref_as, ref_n, pose) in runs:
            pos, normal, mind, maxd, bad, obs, desc = scene
            tl, tr, asg, n = M.SearchLocalPointsRig(ex, f2, pose, cam1, cam2, bounds, sfs, *scene, 0.5, 1.0, False, 50.0, 0.8)
            assert n == ref_n and np.array_equal(asg, ref_as), "rig, camera-2 ratio test %s its line: %d vs %d matches at slots %s" % (what, n, ref_n, np.flatnonzero(asg != ref_as)[:8])
            rp = M.ResidentPoints(ex, pos, normal, mind, maxd, desc)
            lp = M.LocalPointsRigBatch(ex, ex, rp, 1, cam1, cam2, bounds, sfs, 0, 1)
            lp.set_poses([pose])
            lp.enqueue(is_bad=bad, has_obs=obs, th=1.0, far_points=False, th_far=50.0, nnratio=0.8, want_in_view=True)
            asg, nm, iv, ivr = lp.fetch()
            assert nm[0] == ref_n and np.array_equal(asg[0, :F.nl + F.nr], ref_as), "rig batch, camera-2 ratio test %s its line: %d vs %d matches at slots %s" % (
                what, nm[0], ref_n, np.flatnonzero(asg[0, :F.nl + F.nr] != ref_as)[:8])
            rp.close()
    finally:
        ex.close()


def test_rig_camera2_ratio_test_on_its_line_emulated(emu_lib):
    _check_rig_ratio(emu_lib)


@pytest.mark.gpu
def test_rig_camera2_ratio_test_on_its_line_gpu(hip_lib):
    _check_rig_ratio(hip_lib)
