"""The candidate pool of the three projection batches - LastFrame (orbm_search_by_projection_lastframe_batch), rig LastFrame
(orbm_search_by_projection_lastframe_rig_batch) and KeyFrame (orbm_search_by_projection_keyframe_batch) - driven past its size.  They share batch_fetch and
k_area_search_threads with the batched SearchLocalPoints (tests/test_local_points_batch.py::test_candidate_pool_overflow_is_retried), but size the pool for
windows of th = 7 .. 15 px: B x cap_last x 16 (32 for a rig) + 4096 entries.

Protocol under test (csrc/k_search.hip: one atomicAdd reservation per workgroup, nothing written when the span does not fit; csrc/orbm_search.cpp,
batch_fetch): the fetch of a batch that counted more candidates than the pool holds answers ORBX_E_CAPACITY, leaves the caller's buffers alone, ends the
batch (its entries were never written: a second fetch finds nothing pending) and enlarges the pool; the batch enqueued again must equal the single-frame
product calls, which the tests of each kind pin to the reference (tests/test_lastframe_batch.py, tests/test_keyframe_batch.py, tests/test_rig_tracking_batch.py).

Two routes to the overflow, each on a handle of its own because the pool belongs to the handle:
  fresh    the first batch of the handle overflows the pool sized from its rows;
  regrown  an ordinary batch (th = 7) runs first and is checked, then th = 50 overflows the pool that batch left behind, then th = 100 overflows the pool
           the th = 50 batch grew (the second growth of one handle).
Shapes: B = 2 rig frames [L0, L1, R0, R1] of 376 x 376 with 500 features per image, rows on the rays of both cameras' keypoints (about 900 per frame); the
one-camera kinds search the left images.  The smallest world the rig kind accepts, and the one tests/test_pending_batch.py uses."""
import functools
import types

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor, sophus, views
from orb_slam3_detailed_comments_amd import matcher as M
from test_kb8 import CAM1, CAM2, MRLR, TLR, _fisheye_pair
from test_local_points import _rot
from test_models import _predict_scale_float
from test_rig_tracking_batch import TRL, _last_frames

W, H, NF, LAP, B = 376, 376, 500, (0, 375), 2
BOUNDS = (0.0, float(W), 0.0, float(H))
E_ARG, E_CAPACITY = -2, -4
TH_ORDINARY, TH_WIDE, TH_WIDER = 7.0, 50.0, 100.0
KINDS = ("lastframe", "keyframe", "rig_lastframe")


@functools.lru_cache(maxsize=None)
def _images():
    pairs = [_fisheye_pair(60 + s, W, H) for s in range(B)]
    return np.stack([p[0] for p in pairs] + [p[1] for p in pairs])


class World:
    """a FRESH handle with the rig frames extracted and stereo-linked, the rows of their last frames / candidate key frames, and the three kinds of batch"""

    def __init__(self, lib, kind):
        self.lib, self.kind, self.rig = lib, kind, kind == "rig_lastframe"
        self.ex = ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
        res = ex.extract_batch(_images(), LAP)
        st = M.ComputeStereoFishEyeMatches(ex, ex, CAM1, CAM2, MRLR, TLR, 0, B, B)
        rng = np.random.default_rng(5150)
        self.sfs, cap = ex.GetScaleFactors(), ex.max_keypoints()
        self.frames = [types.SimpleNamespace(nl=len(res[b][1]), nr=len(res[B + b][1]), keys=res[b][1], keys_right=res[B + b][1], desc=np.concatenate([res[b][2], res[B + b][2]]),
                                             dl=res[b][2], dr=res[B + b][2], l2r=st["l2r"][b, :len(res[b][1])].copy(), r2l=st["r2l"][b, :len(res[B + b][1])].copy())
                       for b in range(B)]
        self.poses = [(_rot(*rng.normal(0, 0.015, 3)), rng.normal(0, 0.1, 3).astype(np.float32)) for _ in range(B)]
        world = types.SimpleNamespace(rng=rng, cap=cap, B=B, refs=self.frames, scene=list(range(B)), poses=self.poses)
        self.n, self.pos, self.valid, self.octave, self.angle, self.has_obs, self.desc = _last_frames(world)
        capL = self.pos.shape[1]
        self.maxd = np.zeros((B, capL), np.float32)
        for b in range(B):
            Ow = -(self.poses[b][0].astype(np.float64).T @ self.poses[b][1].astype(np.float64))
            self.maxd[b] = np.linalg.norm(self.pos[b].astype(np.float64) - Ow, axis=1) * 1.2 ** self.octave[b]
        self.mind = (self.maxd / 1.2 ** 7).astype(np.float32)
        self.rows, self.slots = B * capL, (2 if self.rig else 1) * cap
        if self.rig:
            self.batch = M.LastFrameRigBatch(ex, ex, B, CAM1, BOUNDS, self.sfs, 0, B); self.batch.set_poses(self.poses, TRL)
        else:
            self.batch = (M.KeyFrameBatch if kind == "keyframe" else M.LastFrameBatch)(ex, B, CAM1, BOUNDS, 0.0, self.sfs); self.batch.set_poses(self.poses)
        assert self.batch.assigned.shape == (B, self.slots)

    def first_pool(self):
        """entries of the pool that the first batch of the handle gets (csrc/orbm_search.cpp: projection_batch, lastframe_rig_batch)"""
        return self.rows * (32 if self.rig else 16) + 4096

    def enqueue(self, th):
        if self.kind == "keyframe":
            self.batch.enqueue(self.n, self.pos, self.valid, self.mind, self.maxd, self.angle, self.desc, th, 100, True, None)
        elif self.rig:
            self.batch.enqueue(self.n, self.pos, self.valid, self.octave, self.angle, self.has_obs, self.desc, th, None, None, True, None)
        else:
            self.batch.enqueue(self.n, self.pos, self.valid, self.octave, self.angle, self.has_obs, self.desc, th, None, None, True, None, use_u_right=False)

    def fetch(self):
        """the C fetch alone (the wrappers' fetch() would enqueue again by itself)"""
        a, nm, L = self.batch.assigned, self.batch.nm, self.lib.L
        if self.rig:
            return L.orbm_search_rig_batch_fetch(self.ex._h, a.ctypes.data, self.slots, nm.ctypes.data, None, None)
        return L.orbm_search_local_points_fetch(self.ex._h, a.ctypes.data, self.slots, nm.ctypes.data, None)

    def single(self, b, th):
        """(nmatches, assigned) of frame b from the single-frame product call of the kind, as the facade makes it"""
        ex, F, N = self.ex, self.frames[b], int(self.n[b])
        pos, sk, desc, angle = self.pos[b, :N], 1 - self.valid[b, :N], self.desc[b, :N], self.angle[b, :N]
        matcher = M.ORBmatcher(0.9, True)
        left = views.frame_view(F.keys, F.dl, self.sfs, W, H, u_right=None, mbf=0.0)
        if self.kind == "keyframe":
            T = sophus.SE3f(*self.poses[b])
            pk = M.ProjectPoints(ex, T, CAM1, BOUNDS, pos, min_inv=0.8 * self.mind[b, :N], max_inv=1.2 * self.maxd[b, :N], skip=sk, Ow=T.inverse().translation(), depth_test=0, bounds_mode=0)
            lvl = _predict_scale_float(self.maxd[b, :N] / np.maximum(pk["dist"], np.float32(1e-30)), np.float32(np.log(np.float64(self.sfs[1]))), len(self.sfs))
            pts = views.projected_point_view(pk["valid"], pk["u"], pk["v"], lvl, desc, angle=angle)
            return matcher.SearchByProjectionKeyFrame(ex, left, pts, th, 100)
        pr = M.ProjectPoints(ex, self.poses[b], CAM1, BOUNDS, pos, skip=sk, depth_test=2, bounds_mode=0)
        last = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], self.octave[b, :N], angle, self.has_obs[b, :N], desc)
        if not self.rig:
            return matcher.SearchByProjectionFrame(ex, left, last, th, False, False)
        p2 = M.ProjectPoints(ex, self.poses[b], CAM1, BOUNDS, pos, skip=sk, second=TRL, depth_test=0, bounds_mode=2)
        right = views.frame_view(F.keys_right, F.dr, self.sfs, W, H)
        return matcher.SearchByProjectionFrameFisheye(ex, views.fisheye_frame_view(left, right, F.l2r, F.r2l), last, p2["u"], p2["v"], th, False, False)

    def check(self, th):
        """the batch's fetched results against the single-frame calls"""
        a, nm = self.batch.assigned, self.batch.nm
        total = 0
        for b in range(B):
            F = self.frames[b]
            used = F.nl + F.nr if self.rig else F.nl
            one_n, one_as = self.single(b, th)
            print("%s, th %g, frame %d: %d matches (single-frame call: %d)" % (self.kind, th, b, nm[b], one_n))
            assert nm[b] == one_n and np.array_equal(a[b, :used], one_as), "%s, th %g, frame %d: %d vs %d matches" % (self.kind, th, b, nm[b], one_n)
            assert (a[b, used:] == -1).all()
            total += one_n
        assert total > 50 * B, "the scene is no test: %d matches" % total

    def overflow_then_again(self, th):
        """th overflows the handle's pool ONCE: the refusal, what it must leave alone, and the batch run again"""
        a, nm = self.batch.assigned, self.batch.nm
        self.enqueue(th)
        a[:] = -77; nm[:] = -77
        rc = self.fetch()
        print("%s, th %g: fetch -> %d (%s)" % (self.kind, th, rc, self.lib.L.orbx_last_error()))
        assert rc == E_CAPACITY, "th %g does not overflow the pool: %d" % (th, rc)
        assert (a == -77).all() and (nm == -77).all(), "the refused fetch wrote into the caller's buffers"
        assert self.fetch() == E_ARG, "the overflowed batch can be fetched again: its entries were never written"
        assert (a == -77).all() and (nm == -77).all()
        self.enqueue(th)
        assert self.fetch() == 0, self.lib.L.orbx_last_error()
        self.check(th)

    def close(self):
        self.ex.close()


def _fresh(lib, kind):
    Wd = World(lib, kind)
    try:
        Wd.overflow_then_again(TH_WIDER)
    finally:
        Wd.close()


def _regrown(lib, kind):
    Wd = World(lib, kind)
    try:
        Wd.enqueue(TH_ORDINARY)
        assert Wd.fetch() == 0, "an ordinary batch overflows the pool sized for it (%d entries)" % Wd.first_pool()
        Wd.check(TH_ORDINARY)
        Wd.overflow_then_again(TH_WIDE)             # past the pool the ordinary batch left behind
        Wd.overflow_then_again(TH_WIDER)            # past the pool that grew for th = 50
        Wd.enqueue(TH_ORDINARY)                     # and the grown pool serves the ordinary batch as before
        assert Wd.fetch() == 0
        Wd.check(TH_ORDINARY)
    finally:
        Wd.close()


@pytest.mark.parametrize("kind", KINDS)
def test_projection_batch_pool_overflow_emulated(emu_lib, kind):
    _fresh(emu_lib, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_projection_batch_pool_overflow_gpu(hip_lib, kind):
    _fresh(hip_lib, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_projection_batch_pool_second_growth_emulated(emu_lib, kind):
    _regrown(emu_lib, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_projection_batch_pool_second_growth_gpu(hip_lib, kind):
    _regrown(hip_lib, kind)
