"""One handle holds ONE pending batched tracking search, whatever its kind: every enqueue - accepted or refused - ends the batch before it, and the fetch of
the other family (orbm_search_local_points_fetch for one camera, orbm_search_rig_batch_fetch for rig frames) refuses.  The table KINDS names every kind of
enqueue that shares the handle's pending batch:

  local points, one set | local points, per-frame maps with want_in_view | LastFrame, host-fed | KeyFrame, host-fed | LastFrame, map-fed |
  rig local points with views | rig LastFrame

For every ordered pair (A, B), on one handle:
  A then B, both accepted: the wrong fetch refuses, the right fetch returns exactly what B returns on a FRESH handle (assignments, counts, views; nothing of
    A's frames, rows, view layout or kind shows through), and a kind without views refuses a fetch that asks for them;
  A accepted, then B refused - once for a null argument, once by a check inside the enqueue (frames with different image bounds, or n[b] > cap) -: both
    fetches refuse.
Nothing here needs a checker outside the library: what each kind computes is pinned to the reference by the tests of that kind.  The fresh results are
required to be worth comparing: every frame has matches, the views are set and end at M_b, and two kinds of one family never return the same result.

Shapes: B = 2 rig frames [L0, L1, R0, R1] of 376 x 376 with 500 features on one handle, the one-camera kinds search its left images; per-frame maps of 150
and 60 points (the accept loop runs three rounds and one), the one set has 400, the last-frame and key-frame rows about 900 per frame.
The state under test is PendingBatch (csrc/orbx_internal.h) with batch_clear / batch_finish (csrc/orbm_search.cpp)."""
import ctypes as C
import types

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor
from orb_slam3_detailed_comments_amd import matcher as M
from test_kb8 import CAM1, CAM2, MRLR, TLR, _fisheye_pair
from test_local_points import _rot
from test_local_points_rig import _scene
from test_map_rows_projection import Store
from test_rig_local_points_maps import _rig_pose
from test_rig_tracking_batch import TRL, _last_frames

W, H, NF, LAP, B = 376, 376, 500, (0, 375), 2
MAP_SIZES = (150, 60)
E_ARG, E_CAPACITY = -2, -4
BOUNDS = (0.0, float(W), 0.0, float(H))


def _handle(lib, images):
    """a handle with the rig frames extracted and stereo-linked"""
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(images, LAP)
    M.ComputeStereoFishEyeMatches(ex, ex, CAM1, CAM2, MRLR, TLR, 0, B, B)
    return ex, res


def _copy(views, edit):
    """the poses of a batch with frame 1 edited: what frames_check refuses inside every enqueue"""
    out = type(views)()
    C.memmove(out, views, C.sizeof(views))
    edit(out[1])
    return out


class Kind:
    """call(h, variant) enqueues on the handle h: variant "ok", "null" (a null argument) or "late" (refused by a check inside the enqueue, whose message
    holds `late`).  rig: the family of its fetch; views: mbTrackInView arrays it was asked for, `width` bytes per frame"""

    def __init__(self, name, call, late, rig=False, views=0, width=1):
        self.name, self.call, self.late, self.rig, self.views, self.width = name, call, late, rig, views, width


def _kinds(lib, ex, res):
    L = lib.L
    rng = np.random.default_rng(5150)
    cap, sfs = ex.max_keypoints(), ex.GetScaleFactors()
    frames = [types.SimpleNamespace(nl=len(res[b][1]), nr=len(res[B + b][1]), keys=res[b][1], keys_right=res[B + b][1], desc=np.concatenate([res[b][2], res[B + b][2]]))
              for b in range(B)]
    poses = [(_rot(*rng.normal(0, 0.015, 3)), rng.normal(0, 0.1, 3).astype(np.float32)) for _ in range(B)]
    ptr = lambda a: None if a is None else a.ctypes.data
    u8 = lambda a: np.ascontiguousarray(a, np.uint8)
    keep = []                                                            # everything the calls point into

    # the local maps: 200 points per scene; the one set holds both scenes, frame b's own map the first MAP_SIZES[b] points of its scene
    parts = [_scene(frames[b], rng, poses[b][0], poses[b][1], 200) for b in range(B)]
    pos, normal, mind, maxd, bad, obs, desc = [np.concatenate([p[k] for p in parts]) for k in range(7)]
    rp_all = M.ResidentPoints(ex, pos, normal, mind, maxd, desc)
    rp_own = [M.ResidentPoints(ex, *[parts[b][k][:MAP_SIZES[b]] for k in (0, 1, 2, 3, 6)]) for b in range(B)]
    bad_all, obs_all = u8(bad), u8(obs)
    fm = M._FrameMaps(rp_own)
    table, flags = fm.table([parts[b][4][:MAP_SIZES[b]] for b in range(B)], [parts[b][5][:MAP_SIZES[b]] for b in range(B)])
    one = M.LocalPointsBatch(ex, rp_all, B, CAM1, BOUNDS, 0.0, sfs); one.set_poses(poses)
    rig = M.LocalPointsRigBatch(ex, ex, rp_all, B, CAM1, CAM2, BOUNDS, sfs, 0, B); rig.set_poses([_rig_pose(R, t) for R, t in poses])
    v_one, v_rig = one.views, rig.views
    v_one_bad = _copy(v_one, lambda v: setattr(v, "max_x", v.max_x + 1.0))
    v_rig_bad = _copy(v_rig, lambda v: setattr(v.left, "max_x", v.left.max_x + 1.0))
    keep += [rp_all, rp_own, bad_all, obs_all, fm, table, flags, one, rig, v_one_bad, v_rig_bad]

    # the rows of the last frames (and, with distance limits, of the candidate key frames): on the rays of both cameras' keypoints
    world = types.SimpleNamespace(rng=rng, cap=cap, B=B, refs=frames, scene=list(range(B)), poses=poses)
    n, lpos, valid, octave, angle, has_obs, ldesc = _last_frames(world)
    capL = lpos.shape[1]
    n_bad = n.copy(); n_bad[1] = capL + 1
    lmax = np.zeros((B, capL), np.float32)
    for b in range(B):
        Ow = -(poses[b][0].astype(np.float64).T @ poses[b][1].astype(np.float64))
        lmax[b] = np.linalg.norm(lpos[b].astype(np.float64) - Ow, axis=1) * 1.2 ** octave[b]
    lmin = (lmax / 1.2 ** 7).astype(np.float32)
    slots = np.full((B, capL), -1, np.int32)
    used = valid.astype(bool) & (np.arange(capL)[None, :] < n[:, None])
    slots[used] = np.arange(int(used.sum()))
    store = Store(ex)
    store.update(slots[used], lpos[used], lmin[used], lmax[used], ldesc[used], np.zeros(int(used.sum()), np.uint8))
    last = M.LastFrameRigBatch(ex, ex, B, CAM1, BOUNDS, sfs, 0, B); last.set_poses(poses, TRL)
    v_last = last.views
    lb = lambda n_: M._LastFrameBatch(capL, ptr(n_), ptr(lpos), ptr(valid), ptr(octave), ptr(angle), ptr(has_obs), ptr(ldesc))
    kb = lambda n_: M._KeyFramePointBatch(capL, ptr(n_), ptr(lpos), ptr(valid), ptr(lmin), ptr(lmax), ptr(angle), ptr(ldesc))
    ls, ls_keep = M._last_frame_slots(n, slots, None, octave, angle, has_obs, None, None, None)
    keep += [n, lpos, valid, octave, angle, has_obs, ldesc, n_bad, lmin, lmax, slots, store, last, ls, ls_keep]

    def local_one(h, v):
        return L.orbm_search_local_points_batch(h, 0, B, v_one_bad if v == "late" else v_one, None if v == "null" else rp_all._p, ptr(bad_all), ptr(obs_all), None, 0, 0.5, 1.0,
                                                0, 50.0, 0.8, 0)

    def local_maps(h, v):
        return L.orbm_search_local_points_batch_maps(h, 0, B, v_one_bad if v == "late" else v_one, None if v == "null" else table.ctypes.data, None, 0, 0.5, 3.0, 0, 50.0, 0.8, 1)

    def lastframe(h, v):
        return L.orbm_search_by_projection_lastframe_batch(h, 0, B, v_one, None if v == "null" else C.byref(lb(n_bad if v == "late" else n)), 7.0, None, None, 1, None, 0)

    def keyframe(h, v):
        return L.orbm_search_by_projection_keyframe_batch(h, 0, B, v_one, None if v == "null" else C.byref(kb(n_bad if v == "late" else n)), 10.0, 100, 1, None)

    def lastframe_map(h, v):
        return L.orbm_search_by_projection_lastframe_batch_map(h, 0, B, v_one_bad if v == "late" else v_one, None if v == "null" else store.map._m, C.byref(ls), 15.0, None, None,
                                                               0, None, 0)

    def rig_local(h, v):
        return L.orbm_search_local_points_rig_batch(h, 0, h, B, B, v_rig_bad if v == "late" else v_rig, None if v == "null" else rp_all._p, ptr(bad_all), ptr(obs_all), None,
                                                    0.5, 1.0, 0, 50.0, 0.8, 1)

    def rig_lastframe(h, v):
        return L.orbm_search_by_projection_lastframe_rig_batch(h, 0, h, B, B, v_last, last.trl.ctypes.data, None if v == "null" else C.byref(lb(n_bad if v == "late" else n)), 7.0,
                                                               None, None, 1, None)

    bounds, rows = b"other image bounds", b"points in"
    kinds = [Kind("local points, one set", local_one, bounds), Kind("local points, per-frame maps with views", local_maps, bounds, views=1, width=max(MAP_SIZES)),
             Kind("LastFrame, host-fed", lastframe, rows), Kind("KeyFrame, host-fed", keyframe, rows), Kind("LastFrame, map-fed", lastframe_map, bounds),
             Kind("rig local points with views", rig_local, bounds, rig=True, views=2, width=len(pos)), Kind("rig LastFrame", rig_lastframe, rows, rig=True)]

    def close():
        store.close(); rp_all.close()
        for r in rp_own:
            r.close()
    return kinds, close, keep


def _fetch(lib, ex, rig, views=0, width=1):
    """(rc, [assigned, nmatches, views ..]) of one family's fetch into buffers no result can leave as they are"""
    slots = (2 if rig else 1) * ex.max_keypoints()
    a = np.full((B, slots), -7, np.int32); nm = np.full(B, -7, np.int32)
    iv = [np.full((B, width), 7, np.uint8) for _ in range(views)]
    p = [v.ctypes.data for v in iv] + [None] * (2 - views)
    if rig:
        rc = lib.L.orbm_search_rig_batch_fetch(ex._h, a.ctypes.data, slots, nm.ctypes.data, p[0], p[1])
    else:
        rc = lib.L.orbm_search_local_points_fetch(ex._h, a.ctypes.data, slots, nm.ctypes.data, p[0])
    return rc, [a, nm] + iv


def _fetch_right(lib, ex, kind):
    rc, got = _fetch(lib, ex, kind.rig, kind.views, kind.width)
    if rc == E_CAPACITY:                                                 # the candidate pool was too small and has grown: the batch runs again
        assert kind.call(ex._h, "ok") == 0
        rc, got = _fetch(lib, ex, kind.rig, kind.views, kind.width)
    assert rc == 0, (kind.name, rc, lib.L.orbx_last_error())
    return got


def _nothing_pending(lib, ex, what):
    for rig in (False, True):
        assert _fetch(lib, ex, rig)[0] == E_ARG, "%s: the %s fetch found a batch" % (what, "rig" if rig else "one-camera")


def _run(lib):
    pairs = [_fisheye_pair(60 + s, W, H) for s in range(B)]
    images = np.stack([p[0] for p in pairs] + [p[1] for p in pairs])
    ex, res = _handle(lib, images)
    kinds, close, keep = _kinds(lib, ex, res)
    try:
        _nothing_pending(lib, ex, "a new handle")
        fresh = []
        for k in kinds:
            f, _ = _handle(lib, images)
            assert k.call(f._h, "ok") == 0, (k.name, lib.L.orbx_last_error())
            fresh.append(_fetch_right(lib, f, k))
            f.close()
        for k, (a, nm, *iv) in zip(kinds, fresh):                       # worth comparing
            assert (nm >= 5).all() and ((a >= 0).sum(axis=1) >= 5).all(), (k.name, nm)
            for v in iv:
                sizes = MAP_SIZES if k.width == max(MAP_SIZES) else (k.width,) * B
                assert all(v[b, :sizes[b]].any() and not v[b, sizes[b]:].any() for b in range(B)), k.name
        for i, ka in enumerate(kinds):
            for j in range(i + 1, len(kinds)):
                assert ka.rig != kinds[j].rig or not np.array_equal(fresh[i][0], fresh[j][0]), "%s and %s return the same assignments" % (ka.name, kinds[j].name)
        h = ex._h
        for ka in kinds:
            for kb, want in zip(kinds, fresh):
                what = "%s, then %s" % (ka.name, kb.name)
                assert ka.call(h, "ok") == 0 and kb.call(h, "ok") == 0, (what, lib.L.orbx_last_error())
                assert _fetch(lib, ex, not kb.rig)[0] == E_ARG, "%s: the wrong fetch" % what
                got = _fetch_right(lib, ex, kb)
                assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), "%s: not what a fresh handle returns" % what
                if kb.views == 0:
                    assert _fetch(lib, ex, kb.rig, 2 if kb.rig else 1, kb.width)[0] == E_ARG, "%s: views that were never asked for" % what
                for variant in ("null", "late"):
                    assert ka.call(h, "ok") == 0, (what, lib.L.orbx_last_error())
                    assert kb.call(h, variant) == E_ARG, "%s (%s)" % (what, variant)
                    if variant == "late":
                        assert kb.late in lib.L.orbx_last_error(), (what, lib.L.orbx_last_error())
                    _nothing_pending(lib, ex, "%s refused (%s)" % (what, variant))
    finally:
        close()
        ex.close()


def test_pending_batch_emulated(emu_lib):
    _run(emu_lib)


@pytest.mark.gpu
def test_pending_batch_gpu(hip_lib):
    _run(hip_lib)
