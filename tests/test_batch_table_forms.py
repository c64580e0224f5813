"""Every batched tracking search reads its frames' points through one per-frame table (FrameMapRec: the set, M, `offset` = where the frame's
scratch rows start, `flags` = where its is_bad / has_obs rows start).  The smallest shapes at which that table can be filled or read wrongly:

* one resident set for every frame (orbm_search_local_points_batch / _rig_batch): B = 3 frames, M = 65 points - frames 1 and 2 start off a wave
  and off a 256-thread block, and `flags` (0: the flags are uploaded once) differs from `offset` (65, 130);
* the LastFrame / KeyFrame / rig-LastFrame batches: B = 3, cap_last = 65, n = (65, 0, 37) - the table says desc = the frame's uploaded rows,
  offset = flags = b * cap_last.

Expected values come from the single-frame entry points, which run another device path (k_frustum for one frame, k_area_search with a wave per
query, the accept loop replayed on the host): orbm_search_local_points_resident, orbm_search_local_points_fisheye, orbm_search_by_projection_frame,
orbm_search_by_projection_keyframe, orbm_search_by_projection_frame_fisheye.  A case is about something only if the single-frame call alone gives
every frame with points at least 10 assignments and gives another result once the call-time flags are left out; both are asserted.

Made to fail once on the emulator before it was committed: with the one-set staging writing flags = offset, frames 1 and 2 of the first case read
is_bad / has_obs beyond the one uploaded [M] array and their assignments differ from the single-frame call's."""
import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor, synth, sophus, views
from orb_slam3_detailed_comments_amd import matcher as M
from test_kb8 import CAM1, CAM2, MRLR, RLR, TLR, _fisheye_pair
from test_local_points import _rot, FX, FY, CX, CY
from test_local_points_rig import _kb8_unproject
from test_models import _predict_scale_float

B, NPTS, NF = 3, 65, 200
N_LAST = (65, 0, 37)
TRL = sophus.SE3f(RLR, TLR).inverse()
CAM = (FX, FY, CX, CY)


def _poses(rng):
    return [(_rot(*rng.normal(0, 0.01, 3)), rng.normal(0, 0.05, 3).astype(np.float32)) for _ in range(B)]


def _to_world(pose, Xc):
    R, t = pose[0].astype(np.float64), pose[1].astype(np.float64)
    return (R.T @ (Xc - t).T).T


def _flip(rng, desc, nbits):
    d = desc.copy()
    for i in range(len(d)):
        for bit in rng.choice(256, nbits, replace=False):
            d[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def _flags(rng, m, pairs):
    """is_bad on about 10 % of the points, has_obs = 0 on about 10 %; of every duplicated pair (i, i + 1) the first point is alive and has no
    observations: it takes the keypoint without occupying it and the copy behind it takes it over - with the flags left out it keeps it"""
    bad = rng.uniform(size=m) < 0.1; obs = rng.uniform(size=m) >= 0.1
    for i in pairs:
        bad[i] = bad[i + 1] = False; obs[i] = False; obs[i + 1] = True
    return bad, obs


def _local_map(rng, poses, rays, descs, octaves):
    """NPTS points, point i on the ray of a keypoint of frame i % B (its descriptor with two bits flipped) seen from that frame's pose; every
    eighth point is copied to the row behind it"""
    pos = np.zeros((NPTS, 3)); desc = np.zeros((NPTS, 32), np.uint8); octv = np.zeros(NPTS); Ow = np.zeros((NPTS, 3))
    for i in range(NPTS):
        b = i % B
        j = int(rng.integers(0, len(rays[b])))
        pos[i] = _to_world(poses[b], rays[b][j:j + 1] * rng.uniform(1.0, 6.0))[0]
        desc[i] = _flip(rng, descs[b][j:j + 1], 2)[0]; octv[i] = octaves[b][j]
        Ow[i] = -(poses[b][0].astype(np.float64).T @ poses[b][1].astype(np.float64))
    pairs = list(range(4, NPTS - 1, 8))
    for i in pairs:
        pos[i + 1] = pos[i]; desc[i + 1] = desc[i]; octv[i + 1] = octv[i]; Ow[i + 1] = Ow[i]
    d = np.linalg.norm(pos - Ow, axis=1)
    normal = (pos - Ow) / d[:, None]
    maxd = d * 1.2 ** octv; mind = maxd / 1.2 ** 7
    bad, obs = _flags(rng, NPTS, pairs)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return f32(pos), f32(normal), f32(mind), f32(maxd), bad, obs, desc


def _about_something(name, b, with_flags, without_flags):
    n, asg = with_flags
    assert n >= 10 and int((asg >= 0).sum()) >= 10, "%s, frame %d: the single-frame call assigns %d keypoints" % (name, b, int((asg >= 0).sum()))
    assert not np.array_equal(asg, without_flags[1]), "%s, frame %d: the flags change nothing" % (name, b)


# ---- one set, one camera --------------------------------------------------------------------------------------------------------------------
def _one_set(lib, seed=3):
    w, h = 320, 240
    rng = np.random.default_rng(seed)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    rp = None
    try:
        res = ex.extract_batch(np.stack([synth.corner_field(w, h, seed=700 + b, nrect=600) for b in range(B)]))
        sfs = ex.GetScaleFactors(); cap = ex.max_keypoints(); bounds = (0.0, float(w), 0.0, float(h))
        poses = _poses(rng)
        rays = [np.stack([(k["x"] - CX) / FX, (k["y"] - CY) / FY, np.ones(len(k))], 1).astype(np.float64) for _, k, _ in res]
        pos, normal, mind, maxd, bad, obs, desc = _local_map(rng, poses, rays, [r[2] for r in res], [r[1]["octave"] for r in res])
        occupied = np.zeros((B, cap), np.uint8)
        for b in range(B):
            occupied[b, rng.choice(len(res[b][1]), len(res[b][1]) // 6, replace=False)] = 1
        rp = M.ResidentPoints(ex, pos, normal, mind, maxd, desc)
        assert rp.M == NPTS
        lp = M.LocalPointsBatch(ex, rp, B, CAM, bounds, 0.0, sfs)
        lp.set_poses(poses)
        lp.enqueue(0, is_bad=bad, has_obs=obs, occupied=occupied, use_u_right=False, th=3.0, want_in_view=True)
        asg, nm, inv = lp.fetch()
        for b in range(B):
            n = len(res[b][1])
            fv = views.frame_view(res[b][1], res[b][2], sfs, w, h, occupied=occupied[b, :n])
            single = lambda bd, ob: M.SearchLocalPoints(ex, fv, poses[b][0], poses[b][1], CAM, bounds, 0.0, sfs, pos, normal, mind, maxd, bd, ob, desc, 0.5, 3.0, resident=rp)
            tr, one_as, one_n = single(bad, obs)
            _, free_as, free_n = single(None, None)
            print("one set, frame %d: %d matches (single-frame call %d, without the flags %d)" % (b, nm[b], one_n, free_n))
            _about_something("one set", b, (one_n, one_as), (free_n, free_as))
            assert nm[b] == one_n and np.array_equal(asg[b, :n], one_as) and (asg[b, n:] == -1).all(), "frame %d: %d vs %d matches" % (b, nm[b], one_n)
            assert np.array_equal(inv[b], tr["in_view"]) and tr["in_view"].any(), "mbTrackInView, frame %d" % b
    finally:
        if rp is not None:
            rp.close()
        ex.close()


def test_one_set_emulated(emu_lib):
    _one_set(emu_lib)


@pytest.mark.gpu
def test_one_set_gpu(hip_lib):
    _one_set(hip_lib)


# ---- rig frames -------------------------------------------------------------------------------------------------------------------------------
class _Rig:
    """B rig frames of one extraction [L0 .. L2, R0 .. R2] with their stereo links"""

    def __init__(self, lib, seed):
        self.w = self.h = w = 320
        self.rng = np.random.default_rng(seed)
        pairs = [_fisheye_pair(80 + b, w, w) for b in range(B)]
        self.ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
        res = self.ex.extract_batch(np.stack([p[0] for p in pairs] + [p[1] for p in pairs]), (0, w - 1))
        st = M.ComputeStereoFishEyeMatches(self.ex, self.ex, CAM1, CAM2, MRLR, TLR, 0, B, B)
        self.kL = [r[1] for r in res[:B]]; self.dL = [r[2] for r in res[:B]]; self.kR = [r[1] for r in res[B:]]; self.dR = [r[2] for r in res[B:]]
        self.l2r = [st["l2r"][b, :len(self.kL[b])].copy() for b in range(B)]; self.r2l = [st["r2l"][b, :len(self.kR[b])].copy() for b in range(B)]
        self.sfs = self.ex.GetScaleFactors(); self.cap = self.ex.max_keypoints(); self.bounds = (0.0, float(w), 0.0, float(w))
        self.poses = _poses(self.rng)
        self.occupied = np.zeros((B, 2 * self.cap), np.uint8)
        for b in range(B):
            nl, nr = len(self.kL[b]), len(self.kR[b])
            self.occupied[b, self.rng.choice(nl, nl // 8, replace=False)] = 1
            self.occupied[b, nl + self.rng.choice(nr, nr // 8, replace=False)] = 1
        # camera-1 rays of every keypoint of both cameras (Tlr maps camera 2 to camera 1), in the slot order of F.mvpMapPoints
        Tlr = sophus.SE3f(RLR, TLR)
        Rlr, tlr = Tlr.rotationMatrix().astype(np.float64), np.asarray(Tlr.translation(), np.float64)
        self.rays = []
        for b in range(B):
            rl = _kb8_unproject(CAM1, self.kL[b]["x"].astype(np.float64), self.kL[b]["y"].astype(np.float64))
            rr = _kb8_unproject(CAM2, self.kR[b]["x"].astype(np.float64), self.kR[b]["y"].astype(np.float64))
            self.rays.append((rl, rr, Rlr, tlr))

    def frame2(self, b):
        nl, nr = len(self.kL[b]), len(self.kR[b])
        left = views.frame_view(self.kL[b], self.dL[b], self.sfs, self.w, self.h, occupied=self.occupied[b, :nl])
        right = views.frame_view(self.kR[b], self.dR[b], self.sfs, self.w, self.h, occupied=self.occupied[b, nl:nl + nr])
        return views.fisheye_frame_view(left, right, self.l2r[b], self.r2l[b])

    def points_in_camera1(self, b, idx, z):
        """camera-1 coordinates of points at depth factor z in front of the slots idx of frame b"""
        rl, rr, Rlr, tlr = self.rays[b]
        nl = len(rl)
        out = np.zeros((len(idx), 3))
        for k, (s, zz) in enumerate(zip(idx, z)):
            out[k] = rl[s] * zz if s < nl else Rlr @ (rr[s - nl] * zz) + tlr
        return out

    def rig_pose(self, b):
        T = sophus.SE3f(*self.poses[b])
        Rcw = T.rotationMatrix()
        return dict(Rcw=Rcw, tcw=np.asarray(T.translation(), np.float32), Ow=np.asarray(T.inverse().translation(), np.float32), Rwc=Rcw.T.copy(),
                    Rrl=TRL.rotationMatrix(), trl=np.asarray(TRL.translation(), np.float32), tlr=TLR)

    def close(self):
        self.ex.close()


def _one_set_rig(lib, seed=5):
    W = _Rig(lib, seed)
    rp = None
    try:
        rng, ex = W.rng, W.ex
        # the rays of _local_map: every slot of a frame, camera 2's expressed in camera 1
        rays, descs, octs = [], [], []
        for b in range(B):
            n = len(W.kL[b]) + len(W.kR[b])
            rays.append(W.points_in_camera1(b, np.arange(n), np.ones(n)))
            descs.append(np.concatenate([W.dL[b], W.dR[b]])); octs.append(np.concatenate([W.kL[b]["octave"], W.kR[b]["octave"]]))
        pos, normal, mind, maxd, bad, obs, desc = _local_map(rng, W.poses, rays, descs, octs)
        rp = M.ResidentPoints(ex, pos, normal, mind, maxd, desc)
        poses = [W.rig_pose(b) for b in range(B)]
        lp = M.LocalPointsRigBatch(ex, ex, rp, B, CAM1, CAM2, W.bounds, W.sfs, 0, B)
        lp.set_poses(poses)
        lp.enqueue(is_bad=bad, has_obs=obs, occupied=W.occupied, th=3.0, want_in_view=True)
        asg, nm, iv, ivr = lp.fetch()
        for b in range(B):
            ns = len(W.kL[b]) + len(W.kR[b])
            single = lambda bd, ob: M.SearchLocalPointsRig(ex, W.frame2(b), poses[b], CAM1, CAM2, W.bounds, W.sfs, pos, normal, mind, maxd, bd, ob, desc, 0.5, 3.0)
            tl, tr, one_as, one_n = single(bad, obs)
            _, _, free_as, free_n = single(None, None)
            print("one set, rig frame %d: %d matches (single-frame call %d, without the flags %d)" % (b, nm[b], one_n, free_n))
            _about_something("one set, rig", b, (one_n, one_as), (free_n, free_as))
            assert nm[b] == one_n and np.array_equal(asg[b, :ns], one_as) and (asg[b, ns:] == -1).all(), "rig frame %d: %d vs %d matches" % (b, nm[b], one_n)
            assert np.array_equal(iv[b], tl["in_view"]) and np.array_equal(ivr[b], tr["in_view_r"]) and tl["in_view"].any() and tr["in_view_r"].any(), "mbTrackInView(R), frame %d" % b
    finally:
        if rp is not None:
            rp.close()
        W.close()


def test_one_set_rig_emulated(emu_lib):
    _one_set_rig(emu_lib)


@pytest.mark.gpu
def test_one_set_rig_gpu(hip_lib):
    _one_set_rig(hip_lib)


# ---- the projection batches ---------------------------------------------------------------------------------------------------------------------
def _last_rows(rng, poses, n_slots, camera1_points, descs, octaves, angles):
    """[B][65] rows of last-frame / key-frame points, N_LAST of them used: frame b's row i in front of a keypoint (slot) of frame b, its descriptor
    with two bits flipped, its octave and angle; every eighth row is copied to the row behind it; ~10 % invalid, ~10 % without observations"""
    cap_last = max(N_LAST)
    n = np.array(N_LAST, np.int32)
    pos = np.zeros((B, cap_last, 3), np.float32); valid = np.zeros((B, cap_last), np.uint8); octave = np.zeros((B, cap_last), np.int32)
    angle = np.zeros((B, cap_last), np.float32); has_obs = np.ones((B, cap_last), np.uint8); desc = np.zeros((B, cap_last, 32), np.uint8)
    mind = np.ones((B, cap_last), np.float32); maxd = np.ones((B, cap_last), np.float32)
    for b in range(B):
        m = int(n[b])
        if m == 0:
            continue
        idx = rng.choice(n_slots[b], m, replace=False)
        pairs = list(range(4, m - 1, 8))
        for i in pairs:
            idx[i + 1] = idx[i]
        z = rng.uniform(1.0, 6.0, m)
        for i in pairs:
            z[i + 1] = z[i]
        Xw = _to_world(poses[b], camera1_points(b, idx, z))
        pos[b, :m] = Xw
        octave[b, :m] = octaves[b][idx]; angle[b, :m] = angles[b][idx]
        d = _flip(rng, descs[b][idx], 2)
        for i in pairs:
            d[i + 1] = d[i]
        desc[b, :m] = d
        Ow = -(poses[b][0].astype(np.float64).T @ poses[b][1].astype(np.float64))
        dist = np.linalg.norm(Xw - Ow, axis=1)
        maxd[b, :m] = dist * 1.2 ** octaves[b][idx].astype(np.float64); mind[b, :m] = maxd[b, :m] / 1.2 ** 7
        bad, obs = _flags(rng, m, pairs)
        valid[b, :m] = ~bad; has_obs[b, :m] = obs
    return n, pos, valid, octave, angle, has_obs, desc, mind, maxd


def _projection(lib, seed=7):
    w, h = 320, 240
    rng = np.random.default_rng(seed)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    try:
        res = ex.extract_batch(np.stack([synth.corner_field(w, h, seed=720 + b, nrect=600) for b in range(B)]))
        sfs = ex.GetScaleFactors(); cap = ex.max_keypoints(); bounds = (0.0, float(w), 0.0, float(h))
        poses = _poses(rng)
        keys = [r[1] for r in res]
        pinhole = lambda b, idx, z: np.stack([(keys[b]["x"][idx] - CX) / FX * z, (keys[b]["y"][idx] - CY) / FY * z, z], 1).astype(np.float64)
        n, pos, valid, octave, angle, has_obs, desc, mind, maxd = _last_rows(rng, poses, [len(k) for k in keys], pinhole, [r[2] for r in res], [k["octave"] for k in keys],
                                                                             [k["angle"] for k in keys])
        assert pos.shape[1] == 65 and tuple(n) == N_LAST
        occupied = np.zeros((B, cap), np.uint8)
        for b in range(B):
            occupied[b, rng.choice(len(keys[b]), len(keys[b]) // 8, replace=False)] = 1
        matcher = M.ORBmatcher(0.9, True)
        # SearchByProjection(CurrentFrame, LastFrame)
        lf = M.LastFrameBatch(ex, B, CAM, bounds, 0.0, sfs); lf.set_poses(poses)
        lf.enqueue(n, pos, valid, octave, angle, has_obs, desc, 7.0, None, None, True, occupied, use_u_right=False)
        asg, nm = lf.fetch(); asg, nm = asg.copy(), nm.copy()
        # SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
        kb = M.KeyFrameBatch(ex, B, CAM, bounds, 0.0, sfs); kb.set_poses(poses)
        kb.enqueue(n, pos, valid, mind, maxd, angle, desc, 10.0, 100, True, occupied)
        asg_k, nm_k = kb.fetch()
        for b in range(B):
            N, m = len(keys[b]), int(n[b])
            fv = views.frame_view(keys[b], res[b][2], sfs, w, h, occupied=occupied[b, :N])
            if m == 0:
                assert nm[b] == 0 and nm_k[b] == 0 and (asg[b] == -1).all() and (asg_k[b] == -1).all(), "frame %d has no points" % b
                continue

            def last_frame(val, obs):
                pr = M.ProjectPoints(ex, poses[b], CAM, bounds, pos[b, :m], skip=1 - val, depth_test=2, bounds_mode=0)
                last = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], octave[b, :m], angle[b, :m], obs, desc[b, :m])
                return matcher.SearchByProjectionFrame(ex, fv, last, 7.0, False, False)
            one_n, one_as = last_frame(valid[b, :m], has_obs[b, :m])
            free = last_frame(np.ones(m, np.uint8), np.ones(m, np.uint8))
            print("LastFrame batch, frame %d: %d matches (single-frame call %d, without the flags %d)" % (b, nm[b], one_n, free[0]))
            _about_something("LastFrame", b, (one_n, one_as), free)
            assert nm[b] == one_n and np.array_equal(asg[b, :N], one_as) and (asg[b, N:] == -1).all(), "LastFrame batch, frame %d: %d vs %d" % (b, nm[b], one_n)

            def key_frame(val):
                T = sophus.SE3f(*poses[b])
                pk = M.ProjectPoints(ex, T, CAM, bounds, pos[b, :m], min_inv=0.8 * mind[b, :m], max_inv=1.2 * maxd[b, :m], skip=1 - val, Ow=T.inverse().translation(),
                                     depth_test=0, bounds_mode=0)
                lvl = _predict_scale_float(maxd[b, :m] / np.maximum(pk["dist"], np.float32(1e-30)), np.float32(np.log(np.float64(sfs[1]))), len(sfs))
                pts = views.projected_point_view(pk["valid"], pk["u"], pk["v"], lvl, desc[b, :m], angle=angle[b, :m])
                return matcher.SearchByProjectionKeyFrame(ex, fv, pts, 10.0, 100)
            k_n, k_as = key_frame(valid[b, :m])
            k_free = key_frame(np.ones(m, np.uint8))
            print("KeyFrame batch, frame %d: %d matches (single-frame call %d, without the flags %d)" % (b, nm_k[b], k_n, k_free[0]))
            _about_something("KeyFrame", b, (k_n, k_as), k_free)
            assert nm_k[b] == k_n and np.array_equal(asg_k[b, :N], k_as) and (asg_k[b, N:] == -1).all(), "KeyFrame batch, frame %d: %d vs %d" % (b, nm_k[b], k_n)
    finally:
        ex.close()


def test_projection_batches_emulated(emu_lib):
    _projection(emu_lib)


@pytest.mark.gpu
def test_projection_batches_gpu(hip_lib):
    _projection(hip_lib)


def _lastframe_rig(lib, seed=9):
    W = _Rig(lib, seed)
    try:
        rng, ex = W.rng, W.ex
        slots = [len(W.kL[b]) + len(W.kR[b]) for b in range(B)]
        cat = lambda name: [np.concatenate([W.kL[b][name], W.kR[b][name]]) for b in range(B)]
        n, pos, valid, octave, angle, has_obs, desc, _, _ = _last_rows(rng, W.poses, slots, W.points_in_camera1, [np.concatenate([W.dL[b], W.dR[b]]) for b in range(B)],
                                                                       cat("octave"), cat("angle"))
        lf = M.LastFrameRigBatch(ex, ex, B, CAM1, W.bounds, W.sfs, 0, B)
        lf.set_poses(W.poses, TRL)
        lf.enqueue(n, pos, valid, octave, angle, has_obs, desc, 7.0, None, None, True, W.occupied)
        asg, nm = lf.fetch()
        matcher = M.ORBmatcher(0.9, True)
        for b in range(B):
            m, ns = int(n[b]), slots[b]
            if m == 0:
                assert nm[b] == 0 and (asg[b] == -1).all(), "rig frame %d has no points" % b
                continue

            def last_frame(val, obs):
                pr = M.ProjectPoints(ex, W.poses[b], CAM1, W.bounds, pos[b, :m], skip=1 - val, depth_test=2, bounds_mode=0)
                p2 = M.ProjectPoints(ex, W.poses[b], CAM1, W.bounds, pos[b, :m], skip=1 - val, second=TRL, depth_test=0, bounds_mode=2)
                last = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], octave[b, :m], angle[b, :m], obs, desc[b, :m])
                return matcher.SearchByProjectionFrameFisheye(ex, W.frame2(b), last, p2["u"], p2["v"], 7.0, False, False)
            one_n, one_as = last_frame(valid[b, :m], has_obs[b, :m])
            free = last_frame(np.ones(m, np.uint8), np.ones(m, np.uint8))
            print("rig LastFrame batch, frame %d: %d matches (single-frame call %d, without the flags %d)" % (b, nm[b], one_n, free[0]))
            _about_something("rig LastFrame", b, (one_n, one_as), free)
            assert nm[b] == one_n and np.array_equal(asg[b, :ns], one_as) and (asg[b, ns:] == -1).all(), "rig LastFrame batch, frame %d: %d vs %d" % (b, nm[b], one_n)
    finally:
        W.close()


def test_lastframe_rig_batch_emulated(emu_lib):
    _lastframe_rig(emu_lib)


@pytest.mark.gpu
def test_lastframe_rig_batch_gpu(hip_lib):
    _lastframe_rig(hip_lib)
