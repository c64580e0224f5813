"""The projection searches of Tracking fed from the resident map: orbm_search_by_projection_lastframe_batch_map (TrackWithMotionModel),
orbm_search_by_projection_lastframe_rig_batch_map and orbm_search_by_projection_keyframe_batch_map (Relocalization) name their points by slot or by
key-frame row of an orbm_map, and k_map_rows_gather writes the rows the host-fed calls upload.

Checker: the REFERENCE's own Frame + ORBmatcher.cc (oracle/_ref/libref_frame.so: ref_frame_search_lastframe, ref_frame_search_keyframe), called once per
frame with arrays this file gathers on the host from ITS OWN copy of what it uploaded (class Store), `valid` computed by the rules of include/orbx.h:
  last frame  i < n[b], slot >= 0, the slot holds a point, not an outlier - the slot's bad flag is NOT read (src/ORBmatcher.cc:1981-1983)
  key frame   i below the row's length, slot >= 0, the slot holds a point that is not bad, not in sAlreadyFound (:2218-2220)
and, in addition, the host-fed product call on the same gathered arrays.  The scenes are those of tests/test_lastframe_batch.py and
tests/test_keyframe_batch.py with their PARAM_SETS, the points scattered over a store of 5000 slots at permuted slots (0 and 4999 among them); rows carry
-1 entries, slots that hold nothing, bad-flagged slots and slots duplicated at distances 1, 63, 64 and 65; one frame has n = 0 and one n = 1.  Before the
library is called the reference alone shows that the scene is a test: enough matches, rotation resets iff mbCheckOrientation, and that each rule matters
(the result changes when the bad-flagged slots of a last frame are dropped, and when any one exclusion of a key frame is lifted).
Isolation: a batch is enqueued, a second handle overwrites every used slot, flips the bad flags and rewrites the rows, and the fetch still returns the
reference's result on the original data; the next enqueue sees the new data."""
import ctypes as C
import gc

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, synth, views
from orb_slam3_detailed_comments_amd import matcher as M
from orb_slam3_detailed_comments_amd.views import KP_DTYPE
from test_keyframe_batch import PARAM_SETS as KEYFRAME_PARAM_SETS
from test_lastframe_batch import PARAM_SETS as LASTFRAME_PARAM_SETS
from test_local_points import _rot, FX, FY, CX, CY, BF
from test_struct_layout import c_layout

pytestmark = pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so not built")
BASE = 0.110074
SHAPE = (376, 240, 500, 5)             # emulator and GPU alike: width, height, features, frames
SLOTS = 5000
NONE, GOOD, EMPTY, BAD, EXCLUDED = 0, 1, 2, 3, 4     # what row i names: no map point (-1) | a point | a slot that holds nothing | a bad point | an outlier / found point
DUP_GAPS = (1, 63, 64, 65)
E_ARG, E_CAPACITY = -2, -4


class Store:
    """An orbm_map and this file's own copy of everything uploaded into it"""

    def __init__(self, ext, kf_rows=0, kf_row_cap=0):
        self.map = M.ResidentMap(ext, SLOTS, kf_rows, kf_row_cap, 1)
        self.pos = np.zeros((SLOTS, 3), np.float32); self.mind = np.zeros(SLOTS, np.float32); self.maxd = np.zeros(SLOTS, np.float32)
        self.desc = np.zeros((SLOTS, 32), np.uint8); self.present = np.zeros(SLOTS, bool); self.bad = np.zeros(SLOTS, bool)
        self.rows = {}

    def update(self, slots, pos, mind, maxd, desc, bad, ext=None):
        slots = np.asarray(slots, np.int64)
        pos = np.ascontiguousarray(pos, np.float32)
        normal = (pos / np.maximum(np.linalg.norm(pos, axis=1), 1e-6)[:, None]).astype(np.float32)
        self.map.update(slots, pos, normal, mind, maxd, desc, np.asarray(bad, np.uint8), ext=ext)
        self.pos[slots] = pos; self.mind[slots] = mind; self.maxd[slots] = maxd; self.desc[slots] = desc; self.present[slots] = True; self.bad[slots] = np.asarray(bad, bool)

    def set_bad(self, slots, bad, ext=None):
        slots = np.asarray(slots, np.int64)
        self.map.set_bad(slots, np.asarray(bad, np.uint8), ext=ext)
        assert self.present[slots].all()
        self.bad[slots] = np.asarray(bad, bool)

    def set_keyframe(self, row, slots, ext=None):
        self.map.set_keyframe(row, slots, ext=ext)
        self.rows[row] = np.array(slots, np.int32)

    def gather(self, slots, n, excluded, read_bad):
        """rows [B, cap] of slots -> valid, pos, mfMinDistance, mfMaxDistance, descriptor as the device gathers them"""
        B, cap = slots.shape
        inside = np.arange(cap)[None, :] < np.asarray(n)[:, None]
        s = np.where(slots >= 0, slots, 0)
        valid = inside & (slots >= 0) & self.present[s] & ~np.asarray(excluded, bool)
        if read_bad:
            valid &= ~self.bad[s]
        z = lambda a: np.where(valid.reshape(valid.shape + (1,) * (a.ndim - 2)), a, 0).astype(a.dtype)
        return valid.astype(np.uint8), z(self.pos[s]), z(self.mind[s]), z(self.maxd[s]), z(self.desc[s])

    def close(self):
        self.map.close()


def _assign_slots(rng, kind, n):
    """a slot for every row that names one: a permutation of the store, slot 0 and slot SLOTS - 1 given to good rows; then rows duplicated at DUP_GAPS"""
    B, cap = kind.shape
    slots = np.full((B, cap), -1, np.int32)
    free = list(rng.permutation(np.arange(1, SLOTS - 1)))
    ends = [0, SLOTS - 1]
    for b in range(B):
        for i in range(int(n[b])):
            if kind[b, i] != NONE:
                slots[b, i] = ends.pop() if (ends and kind[b, i] == GOOD) else free.pop()
    assert not ends
    return slots


def _duplicate(rng, n, slots, kind, *per_row):
    """rows that name the slot of another row of their frame (the same MapPoint twice in mvpMapPoints), at every gap of DUP_GAPS; per_row: arrays of
    the scene that belong to the point and go with it"""
    gaps = set()
    for b in range(len(n)):
        N = int(n[b])
        if N < 200:
            continue
        for i in rng.choice(N - 70, N // 5, replace=False):
            g = int(rng.choice(DUP_GAPS)); j = i + g
            if slots[b, j] in (0, SLOTS - 1):                           # (the ends of the store stay in use)
                continue
            slots[b, j] = slots[b, i]; kind[b, j] = kind[b, i]
            for a in per_row:
                a[b, j] = a[b, i]
            if slots[b, i] >= 0:
                gaps.add(g)
    assert gaps == set(DUP_GAPS)


def _fill_store(store, n, slots, kind, pos, mind, maxd, desc):
    """the points of the rows go to their slots (an EMPTY row's slot stays untouched); BAD rows' slots are flagged afterwards, as SetBadFlag does"""
    sel = [(b, i) for b in range(len(n)) for i in range(int(n[b])) if kind[b, i] in (GOOD, BAD, EXCLUDED)]
    first = {}
    for b, i in sel:
        first.setdefault(int(slots[b, i]), (b, i))
    s = np.array(sorted(first), np.int32)
    bi = np.array([first[int(k)] for k in s])
    g = lambda a: a[bi[:, 0], bi[:, 1]]
    store.update(s, g(pos), g(mind), g(maxd), g(desc), np.zeros(len(s), np.uint8))
    badslots = np.unique([slots[b, i] for b, i in sel if kind[b, i] == BAD])
    store.set_bad(badslots, np.ones(len(badslots), np.uint8))
    assert store.present[0] and store.present[SLOTS - 1]
    for b, i in sel:                                                    # every row of a slot carries that slot's point
        assert np.array_equal(store.pos[slots[b, i]], pos[b, i]) and np.array_equal(store.desc[slots[b, i]], desc[b, i])


def _flip(rng, d, most):
    for i in range(len(d)):
        for bit in rng.choice(256, int(rng.integers(0, most)), replace=False):
            d[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def _extract(lib, seed0):
    w, h, nf, B = SHAPE
    pairs = [synth.stereo_pair(w, h, seed=seed0 + b, nrect=int(3000 * w * h / (752 * 480))) for b in range(B)]
    refs = [ol.ReferenceFrame(l, r, nf, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF) for l, r in pairs]
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([l for l, _ in pairs] + [r for _, r in pairs]))
    for b in range(B):
        assert res[b][1].tobytes() == refs[b].keys.tobytes()
    return refs, ex, res


def _sizes(B, full):
    """the frames' row counts: frame B - 2 has none, frame B - 1 one"""
    n = np.array(full, np.int32); n[B - 2] = 0; n[B - 1] = 1
    return n


# ---- SearchByProjection(CurrentFrame, LastFrame) -------------------------------------------------------------------------------------------------------

def _run_lastframe(lib, mono):
    w, h, nf, B = SHAPE
    rng = np.random.default_rng(9100 + int(mono))
    refs, ex, res = _extract(lib, 120)
    lib.check(lib.L.orbm_stereo_match(ex._h, 0, ex._h, B, B, BF, BASE))
    cap = ex.max_keypoints(); sfs = ex.GetScaleFactors()
    cam, bounds = (FX, FY, CX, CY), (0.0, float(w), 0.0, float(h))
    capL = cap + 9
    assert capL % 64 != 0 and 4 * capL > 2 * 256
    n = _sizes(B, [refs[b].N for b in range(B)])
    pos = np.zeros((B, capL, 3), np.float32); kind = np.zeros((B, capL), np.uint8); octave = np.zeros((B, capL), np.int32); angle = np.zeros((B, capL), np.float32)
    has_obs = np.ones((B, capL), np.uint8); desc = np.zeros((B, capL, 32), np.uint8); unused = np.zeros((B, capL), np.float32)
    poses, last_poses = [], []
    for b in range(B):
        k, d = res[b][1], res[b][2]; N = int(n[b])
        R, t = _rot(*(rng.normal(0, 0.004, 3))), rng.normal(0, 0.02, 3).astype(np.float32)
        poses.append((R, t))
        last_poses.append((R, (t + np.array([0.0, 0.0, (0.0, 3.0, -3.0)[b % 3] * BASE], np.float32)).astype(np.float32)))
        z = rng.uniform(1.0, 10.0, N)
        Xc = np.stack([(k["x"][:N] + rng.normal(0, 1.0, N) - CX) / FX * z, (k["y"][:N] + rng.normal(0, 1.0, N) - CY) / FY * z, z], 1)
        pos[b, :N] = (R.astype(np.float64).T @ (Xc - t.astype(np.float64)).T).T.astype(np.float32)
        kind[b, :N] = rng.choice([NONE, GOOD, EMPTY, BAD, EXCLUDED], N, p=[0.06, 0.72, 0.04, 0.10, 0.08]) if N > 1 else GOOD
        octave[b, :N] = np.clip(k["octave"][:N] + rng.integers(-1, 2, N), 0, 7)
        ang = k["angle"][:N] + rng.normal(0, 4.0, N); ang[rng.uniform(size=N) < 0.15] += rng.uniform(40, 300)
        angle[b, :N] = np.mod(ang, 360.0).astype(np.float32)
        has_obs[b, :N] = rng.uniform(size=N) < 0.85
        desc[b, :N] = _flip(rng, d[:N].copy(), 30)
    slots = _assign_slots(rng, kind, n)
    _duplicate(rng, n, slots, kind, pos, desc, octave)
    store = Store(ex)
    _fill_store(store, n, slots, kind, pos, unused + 1.0, unused + 2.0, desc)
    outlier = (kind == EXCLUDED).astype(np.uint8)
    occupied = np.zeros((B, cap), np.uint8)
    for b in range(B):
        occupied[b, rng.choice(refs[b].N, refs[b].N // 8, replace=False)] = 1
    lf = M.LastFrameBatch(ex, B, cam, bounds, BF, sfs); lf.set_poses(poses)

    def reference(valid, gpos, gdesc, th, ori, occ):
        return [refs[b].search_lastframe(poses[b][0], poses[b][1], last_poses[b][0], last_poses[b][1], gpos[b, :n[b]].reshape(-1, 3), valid[b, :n[b]], octave[b, :n[b]],
                                         angle[b, :n[b]], has_obs[b, :n[b]], gdesc[b, :n[b]].reshape(-1, 32), th, mono, ori, 0.9, None if occ is None else occ[b, :refs[b].N])
                for b in range(B)]

    def check(ref, asg, nm, what):
        for b in range(B):
            assert nm[b] == ref[b][0] and np.array_equal(asg[b, :refs[b].N], ref[b][1]), "frame %d, %s: %d vs %d matches" % (b, what, nm[b], ref[b][0])
            assert (asg[b, refs[b].N:] == -1).all()

    first = True
    for th, use_occ, ori in LASTFRAME_PARAM_SETS:
        occ = occupied if use_occ else None
        valid, gpos, _, _, gdesc = store.gather(slots, n, outlier, read_bad=False)
        assert valid[kind == BAD].any() and not valid[kind == EMPTY].any()
        ref = reference(valid, gpos, gdesc, th, ori, occ)
        total = sum(r[0] for r in ref); resets = sum(int((r[1] == -2).sum()) for r in ref)
        assert total > 100 * B and (resets > 0) == ori, (total, resets)
        assert ref[B - 2][0] == 0
        if first:                                                       # the ignored bad flag matters: with those rows dropped the reference answers otherwise
            v2, p2, _, _, d2 = store.gather(slots, n, outlier, read_bad=True)
            ref2 = reference(v2, p2, d2, th, ori, occ)
            assert any(not np.array_equal(a[1], c[1]) for a, c in zip(ref, ref2))
        fwd = np.array([r[2] for r in ref], np.uint8); bwd = np.array([r[3] for r in ref], np.uint8)
        lf.enqueue_slots(store.map, n, slots, outlier, octave, angle, has_obs, th, fwd, bwd, ori, occ, use_u_right=not mono)
        asg, nm = lf.fetch()
        check(ref, asg, nm, "th %g, against the reference" % th)
        got = asg.copy(), nm.copy()
        lf.enqueue(n, gpos, valid, octave, angle, has_obs, gdesc, th, fwd, bwd, ori, occ, use_u_right=not mono)
        asg, nm = lf.fetch()
        assert np.array_equal(asg, got[0]) and np.array_equal(nm, got[1]), "th %g: the host-fed call on the gathered arrays" % th
        if first:                                                       # outlier == NULL: none
            v3, p3, _, _, d3 = store.gather(slots, n, np.zeros_like(outlier), read_bad=False)
            lf.enqueue_slots(store.map, n, slots, None, octave, angle, has_obs, th, fwd, bwd, ori, occ, use_u_right=not mono)
            asg, nm = lf.fetch()
            check(reference(v3, p3, d3, th, ori, occ), asg, nm, "no outlier array")
        first = False
    # isolation: what the batch read of the map is the map at the moment of the call
    th, _, ori = LASTFRAME_PARAM_SETS[0]
    valid, gpos, _, _, gdesc = store.gather(slots, n, outlier, read_bad=False)
    ref = reference(valid, gpos, gdesc, th, ori, None)
    fwd = np.array([r[2] for r in ref], np.uint8); bwd = np.array([r[3] for r in ref], np.uint8)
    ex2 = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    lf.enqueue_slots(store.map, n, slots, outlier, octave, angle, has_obs, th, fwd, bwd, ori, None, use_u_right=not mono)
    used = np.unique(slots[slots >= 0])
    used = used[store.present[used]]
    perm = rng.permutation(len(used))
    store.update(used, store.pos[used[perm]], store.mind[used], store.maxd[used], store.desc[used[perm]], ~store.bad[used], ext=ex2)
    asg, nm = lf.fetch()
    check(ref, asg, nm, "fetched after the map was overwritten")
    valid, gpos, _, _, gdesc = store.gather(slots, n, outlier, read_bad=False)
    ref_new = reference(valid, gpos, gdesc, th, ori, None)
    assert any(not np.array_equal(a[1], c[1]) for a, c in zip(ref, ref_new))
    lf.enqueue_slots(store.map, n, slots, outlier, octave, angle, has_obs, th, fwd, bwd, ori, None, use_u_right=not mono)
    asg, nm = lf.fetch()
    check(ref_new, asg, nm, "the next enqueue sees the new points")
    ex2.close(); store.close(); ex.close()


@pytest.mark.parametrize("mono", [False, True])
def test_lastframe_slots_emulated(emu_lib, mono):
    _run_lastframe(emu_lib, mono)


@pytest.mark.gpu
@pytest.mark.parametrize("mono", [False, True])
def test_lastframe_slots_gpu(hip_lib, mono):
    _run_lastframe(hip_lib, mono)


# ---- SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) ---------------------------------------------------------------------------------

def _resident_keyframe(ex, sfs, angle):
    """a resident key frame of len(angle) features without a FeatureVector: the search reads mvKeysUn[i].angle of it"""
    kk = np.zeros(len(angle), KP_DTYPE); kk["angle"] = angle; kk["size"] = 31.0
    z = np.zeros(0, np.uint32)
    return M.ResidentKeyFrame(ex, views.key_frame_view(kk, np.zeros((len(angle), 32), np.uint8), sfs, sfs * sfs, z, np.zeros(1, np.int32), z, None, None))


def _run_keyframe(lib):
    w, h, nf, B = SHAPE
    rng = np.random.default_rng(9200)
    refs, ex, res = _extract(lib, 520)
    cap = ex.max_keypoints(); sfs = ex.GetScaleFactors()
    cam, bounds = (FX, FY, CX, CY), (0.0, float(w), 0.0, float(h))
    capK = cap + 9
    n = _sizes(B, [refs[b].N + 7 for b in range(B)])
    pos = np.zeros((B, capK, 3), np.float32); kind = np.zeros((B, capK), np.uint8); mind = np.zeros((B, capK), np.float32); maxd = np.zeros((B, capK), np.float32)
    angle = np.zeros((B, capK), np.float32); desc = np.zeros((B, capK, 32), np.uint8)
    poses = []
    for b in range(B):
        k, d = res[b][1], res[b][2]; N = len(k); NK = int(n[b])
        R, t = _rot(*(rng.normal(0, 0.01, 3))), rng.normal(0, 0.05, 3).astype(np.float32)
        poses.append((R, t))
        src = rng.integers(0, N, NK)
        z = rng.uniform(1.0, 10.0, NK)
        Xc = np.stack([(k["x"][src] + rng.normal(0, 1.5, NK) - CX) / FX * z, (k["y"][src] + rng.normal(0, 1.5, NK) - CY) / FY * z, z], 1)
        Xc[rng.uniform(size=NK) < 0.03, 2] *= -1.0
        Xw = (R.astype(np.float64).T @ (Xc - t.astype(np.float64)).T).T
        pos[b, :NK] = Xw.astype(np.float32)
        Ow = -(R.astype(np.float64).T @ t.astype(np.float64))
        dist = np.linalg.norm(Xw - Ow, axis=1)
        mx = dist * 1.2 ** k["octave"][src].astype(np.int64) * rng.uniform(0.9, 1.1, NK)
        mn = mx / 1.2 ** 7
        out = rng.uniform(size=NK) < 0.08
        mx[out] = dist[out] / 1.2 * rng.choice([0.5, 0.99999, 1.00001], out.sum())
        far = rng.uniform(size=NK) < 0.05
        mn[far] = dist[far] / 0.8 * rng.choice([2.0, 1.00001, 0.99999], far.sum())
        mind[b, :NK] = mn.astype(np.float32); maxd[b, :NK] = mx.astype(np.float32)
        kind[b, :NK] = rng.choice([NONE, GOOD, EMPTY, BAD, EXCLUDED], NK, p=[0.07, 0.73, 0.05, 0.05, 0.10]) if NK > 1 else GOOD
        ang = k["angle"][src] + rng.normal(0, 4.0, NK); ang[rng.uniform(size=NK) < 0.15] += rng.uniform(40, 300)
        angle[b, :NK] = np.mod(ang, 360.0).astype(np.float32)
        desc[b, :NK] = _flip(rng, d[src].copy(), 60)
    slots = _assign_slots(rng, kind, n)
    _duplicate(rng, n, slots, kind, pos, desc, mind, maxd)
    store = Store(ex, kf_rows=B + 3, kf_row_cap=capK)
    _fill_store(store, n, slots, kind, pos, mind, maxd, desc)
    rows = rng.permutation(B + 3)[:B].astype(np.int32)
    for b in range(B):
        store.set_keyframe(int(rows[b]), slots[b, :n[b]])
    kfs = [_resident_keyframe(ex, sfs, angle[b, :n[b]]) for b in range(B)]
    found = (kind == EXCLUDED).astype(np.uint8)
    occupied = np.zeros((B, cap), np.uint8)
    for b in range(B):
        occupied[b, rng.choice(refs[b].N, refs[b].N // 8, replace=False)] = 1
    kb = M.KeyFrameBatch(ex, B, cam, bounds, BF, sfs); kb.set_poses(poses)

    def reference(valid, gpos, gmin, gmax, gdesc, th, orb_dist, ori, occ, ang=angle):
        return [refs[b].search_keyframe(poses[b][0], poses[b][1], gpos[b, :n[b]].reshape(-1, 3), valid[b, :n[b]], gmin[b, :n[b]], gmax[b, :n[b]], ang[b, :n[b]],
                                        gdesc[b, :n[b]].reshape(-1, 32), th, orb_dist, ori, 0.9, None if occ is None else occ[b, :refs[b].N]) for b in range(B)]

    def check(ref, asg, nm, what):
        for b in range(B):
            assert nm[b] == ref[b][0] and np.array_equal(asg[b, :refs[b].N], ref[b][1]), "frame %d, %s: %d vs %d matches" % (b, what, nm[b], ref[b][0])
            assert (asg[b, refs[b].N:] == -1).all()

    def slot_rows():
        s = np.full((B, capK), -1, np.int32)
        for b in range(B):
            s[b, :n[b]] = store.rows[int(rows[b])]
        return s

    first = True
    for th, orb_dist, use_occ, ori in KEYFRAME_PARAM_SETS:
        occ = occupied if use_occ else None
        valid, gpos, gmin, gmax, gdesc = store.gather(slot_rows(), n, found, read_bad=True)
        ref = reference(valid, gpos, gmin, gmax, gdesc, th, orb_dist, ori, occ)
        total = sum(r[0] for r in ref); resets = sum(int((r[1] == -2).sum()) for r in ref)
        assert total > 60 * B and (resets > 0) == ori, (total, resets)
        if first:                                                       # each exclusion matters: lifted alone, the reference answers otherwise
            inside = np.arange(capK)[None, :] < n[:, None]
            for lifted in (NONE, EMPTY, BAD, EXCLUDED):
                v2 = (valid.astype(bool) | ((kind == lifted) & inside)).astype(np.uint8)
                ref2 = reference(v2, pos, mind, maxd, desc, th, orb_dist, ori, occ)
                assert any(not np.array_equal(a[1], c[1]) for a, c in zip(ref, ref2)), "exclusion %d changes nothing" % lifted
        kb.enqueue_rows(store.map, rows, kfs, found, th, orb_dist, ori, occ)
        asg, nm = kb.fetch()
        check(ref, asg, nm, "th %g, against the reference" % th)
        got = asg.copy(), nm.copy()
        kb.enqueue(n, gpos, valid, gmin, gmax, angle, gdesc, th, orb_dist, ori, occ)
        asg, nm = kb.fetch()
        assert np.array_equal(asg, got[0]) and np.array_equal(nm, got[1]), "th %g: the host-fed call on the gathered arrays" % th
        if first:                                                       # found == NULL: none found
            v3, p3, mn3, mx3, d3 = store.gather(slot_rows(), n, np.zeros_like(found), read_bad=True)
            kb.enqueue_rows(store.map, rows, kfs, None, th, orb_dist, ori, occ)
            asg, nm = kb.fetch()
            check(reference(v3, p3, mn3, mx3, d3, th, orb_dist, ori, occ), asg, nm, "no found array")
        first = False
    # isolation
    th, orb_dist, _, ori = KEYFRAME_PARAM_SETS[0]
    valid, gpos, gmin, gmax, gdesc = store.gather(slot_rows(), n, found, read_bad=True)
    ref = reference(valid, gpos, gmin, gmax, gdesc, th, orb_dist, ori, None)
    ex2 = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    kb.enqueue_rows(store.map, rows, kfs, found, th, orb_dist, ori, None)
    used = np.unique(slots[slots >= 0]); used = used[store.present[used]]
    perm = rng.permutation(len(used))
    store.update(used, store.pos[used[perm]], store.mind[used[perm]], store.maxd[used[perm]], store.desc[used[perm]], ~store.bad[used], ext=ex2)
    for b in range(B):                                                  # every row reversed: entry i names the point of entry n - 1 - i now
        store.set_keyframe(int(rows[b]), store.rows[int(rows[b])][::-1].copy(), ext=ex2)
    asg, nm = kb.fetch()
    check(ref, asg, nm, "fetched after the map was overwritten")
    valid, gpos, gmin, gmax, gdesc = store.gather(slot_rows(), n, found, read_bad=True)
    ref_new = reference(valid, gpos, gmin, gmax, gdesc, th, orb_dist, ori, None)
    assert any(not np.array_equal(a[1], c[1]) for a, c in zip(ref, ref_new))
    kb.enqueue_rows(store.map, rows, kfs, found, th, orb_dist, ori, None)
    asg, nm = kb.fetch()
    check(ref_new, asg, nm, "the next enqueue sees the new rows and points")
    for k in kfs:
        k.close()
    ex2.close(); store.close(); ex.close()


def test_keyframe_rows_emulated(emu_lib):
    _run_keyframe(emu_lib)


@pytest.mark.gpu
def test_keyframe_rows_gpu(hip_lib):
    _run_keyframe(hip_lib)


# ---- rig frames ----------------------------------------------------------------------------------------------------------------------------------------

def _run_rig(lib):
    """The scene of tests/test_rig_tracking_batch.py at its emulator shape; the checkers are that file's: the single-frame product call
    (orbm_search_by_projection_frame_fisheye behind orbm_project_points) and the oracle's restatement, plus the host-fed batch on the gathered arrays."""
    import test_rig_tracking_batch as RT
    from test_kb8 import CAM1
    W = RT.World(lib, 376, 376, 500, (0, 375), 3, 2)
    try:
        ex, B = W.exL, W.B
        n, pos, valid0, octave, angle, has_obs, desc = RT._last_frames(W)
        capL = pos.shape[1]
        rng = np.random.default_rng(9300)
        kind = np.zeros((B, capL), np.uint8)
        for b in range(B):
            kind[b, :n[b]] = rng.choice([NONE, GOOD, EMPTY, BAD, EXCLUDED], int(n[b]), p=[0.06, 0.72, 0.04, 0.10, 0.08])
        slots = _assign_slots(rng, kind, n)
        _duplicate(rng, n, slots, kind, pos, desc, octave)
        store = Store(ex)
        unused = np.zeros((B, capL), np.float32)
        _fill_store(store, n, slots, kind, pos, unused + 1.0, unused + 2.0, desc)
        outlier = (kind == EXCLUDED).astype(np.uint8)
        valid, gpos, _, _, gdesc = store.gather(slots, n, outlier, read_bad=False)
        lf = M.LastFrameRigBatch(W.exL, W.exR, B, CAM1, W.bounds, W.sfs, W.lf, W.rf)
        lf.set_poses(W.poses, RT.TRL)
        occ = W.occupied()
        total = resets = 0
        for fw, bw, ori in ((1, 0, True), (0, 0, True), (0, 0, False)):
            fwd = np.full(B, fw, np.uint8); bwd = np.full(B, bw, np.uint8)
            use_occ = not (fw or bw) and ori
            lf.enqueue_slots(store.map, n, slots, outlier, octave, angle, has_obs, 7.0, fwd, bwd, ori, occ if use_occ else None)
            asg, nm = lf.fetch()
            got = asg.copy(), nm.copy()
            matcher = M.ORBmatcher(0.9, ori)
            for b in range(B):
                N = int(n[b]); nl, nr = W.n(b)
                sk = 1 - valid[b, :N]
                pr = M.ProjectPoints(ex, W.poses[b], CAM1, W.bounds, gpos[b, :N], skip=sk, depth_test=2, bounds_mode=0)
                p2 = M.ProjectPoints(ex, W.poses[b], CAM1, W.bounds, gpos[b, :N], skip=sk, second=RT.TRL, depth_test=0, bounds_mode=2)
                last = views.last_frame_view(pr["valid"], pr["u"], pr["v"], pr["inv_z"], octave[b, :N], angle[b, :N], has_obs[b, :N], gdesc[b, :N])
                cur2 = W.frame2(b, occ if use_occ else None)
                one_n, one_as = matcher.SearchByProjectionFrameFisheye(ex, cur2, last, p2["u"], p2["v"], 7.0, bool(fw), bool(bw))
                assert nm[b] == one_n and np.array_equal(asg[b, :nl + nr], one_as), "frame %d (fw %d bw %d ori %d): %d vs %d" % (b, fw, bw, ori, nm[b], one_n)
                assert (asg[b, nl + nr:] == -1).all()
                o_n, o_as = ol.oracle_search_by_projection_frame_fisheye(cur2, last, p2["u"], p2["v"], 7.0, fw, bw, ori)
                assert o_n == one_n and np.array_equal(o_as, one_as), "frame %d: oracle" % b
                total += one_n; resets += int((one_as == -2).sum())
            lf.enqueue(n, gpos, valid, octave, angle, has_obs, gdesc, 7.0, fwd, bwd, ori, occ if use_occ else None)
            asg, nm = lf.fetch()
            assert np.array_equal(asg, got[0]) and np.array_equal(nm, got[1]), "the host-fed rig call on the gathered arrays"
        assert total > 50 * B * 3 and resets > 0
        # refusals of the rig form: nothing to fetch afterwards
        L = lib.L
        a = np.zeros((B, 2 * W.cap), np.int32); m = np.zeros(B, np.int32)
        fetch = lambda: L.orbm_search_rig_batch_fetch(ex._h, a.ctypes.data, 2 * W.cap, m.ctypes.data, None, None)
        lb, keep = M._last_frame_slots(n, slots, outlier, octave, angle, has_obs, None, None, None)
        call = lambda mp, last: L.orbm_search_by_projection_lastframe_rig_batch_map(W.exL._h, W.lf, W.exR._h, W.rf, B, lf.views, lf.trl.ctypes.data, mp, last, 7.0, None, None, 1, None)
        assert call(store.map._m, C.byref(lb)) == 0 and fetch() == 0
        assert call(None, C.byref(lb)) == E_ARG and fetch() == E_ARG
        assert call(store.map._m, None) == E_ARG and fetch() == E_ARG
        s2 = slots.copy(); s2[1, 5] = SLOTS
        lb2, keep2 = M._last_frame_slots(n, s2, outlier, octave, angle, has_obs, None, None, None)
        assert call(store.map._m, C.byref(lb2)) == E_ARG and b"frame 1, entry 5" in L.orbx_last_error()
        assert fetch() == E_ARG
        store.close()
    finally:
        W.close()


def test_lastframe_rig_slots_emulated(emu_lib):
    _run_rig(emu_lib)


@pytest.mark.gpu
def test_lastframe_rig_slots_gpu(hip_lib):
    _run_rig(hip_lib)


# ---- refusals, resources, mirrors ----------------------------------------------------------------------------------------------------------------------

def _live(lib):
    gc.collect()                        # handles of earlier tests that only a collection frees (a caught exception's traceback keeps its frame) are not this test's
    a = (C.c_longlong * 4)()
    lib.check(lib.L.orbx_debug_live_resources(a))
    return list(a)


def _refusals(lib):
    L = lib.L
    live0 = _live(lib)
    w, h, nf, B = 376, 240, 300, 2
    rng = np.random.default_rng(77)
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    ex.extract_batch(np.stack([synth.corner_field(w, h, seed=5 + b, nrect=600) for b in range(B)]))
    cap = ex.max_keypoints(); sfs = ex.GetScaleFactors()
    store = Store(ex, kf_rows=4, kf_row_cap=64)
    P = 40
    store.update(np.arange(P), rng.normal(0, 1, (P, 3)) + [0, 0, 4], np.full(P, 0.5, np.float32), np.full(P, 30.0, np.float32), rng.integers(0, 256, (P, 32), dtype=np.uint8),
                 np.zeros(P, np.uint8))
    fv = (M._FrustumView * B)()
    for b in range(B):
        M.frustum_view(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), (FX, FY, CX, CY), (0.0, float(w), 0.0, float(h)), BF, sfs, into=fv[b])
    a = np.zeros((B, cap), np.int32); nm = np.zeros(B, np.int32)
    fetch = lambda: L.orbm_search_local_points_fetch(ex._h, a.ctypes.data, cap, nm.ctypes.data, None)

    def refused(rc, text=None):
        assert rc == E_ARG, rc
        if text is not None:
            assert text in (L.orbx_last_error() or b"").decode(), (text, L.orbx_last_error())
        assert fetch() == E_ARG                                          # nothing was enqueued: nothing to fetch

    # last frame
    capL = 50
    n = np.array([30, 20], np.int32); slots = rng.integers(-1, P, (B, capL)).astype(np.int32); octave = np.zeros((B, capL), np.int32); angle = np.zeros((B, capL), np.float32)

    def last(n_=n, slots_=slots, first=0, mp=store.map._m, null_last=False, octave_=octave, frames=B):
        lb, keep = M._last_frame_slots(n_, slots_, None, octave_, angle, None, None, None, None)
        return L.orbm_search_by_projection_lastframe_batch_map(ex._h, first, frames, fv, mp, None if null_last else C.byref(lb), 7.0, None, None, 1, None, 0)
    assert fetch() == E_ARG
    assert last() == 0 and fetch() == 0
    refused(last(mp=None)); refused(last(null_last=True))
    refused(last(n_=np.array([30, -1], np.int32)), "frame 1"); refused(last(n_=np.array([capL + 1, 20], np.int32)), "frame 0")
    for bad_slot in (-2, SLOTS):
        s2 = slots.copy(); s2[1, 7] = bad_slot
        refused(last(slots_=s2), "frame 1, entry 7")
    s2 = slots.copy(); s2[1, 25] = SLOTS                              # beyond n[1]: not an entry of the frame
    assert last(slots_=s2) == 0 and fetch() == 0
    refused(last(first=1)); refused(last(frames=0))                    # what the host-fed call refuses: frames beyond the extraction, no frames
    lb, keep = M._last_frame_slots(n, slots, None, octave, angle, None, None, None, None); lb.octave = None
    refused(L.orbm_search_by_projection_lastframe_batch_map(ex._h, 0, B, fv, store.map._m, C.byref(lb), 7.0, None, None, 1, None, 0))
    # key frame
    store.set_keyframe(0, rng.integers(-1, P, 33)); store.set_keyframe(2, rng.integers(-1, P, 10)); store.set_keyframe(3, np.zeros(0, np.int32))
    kf33, kf10, kf0 = (_resident_keyframe(ex, sfs, np.zeros(k, np.float32)) for k in (33, 10, 0))

    def keyframe(rows=(0, 2), kfs=(kf33, kf10), mp=store.map._m, null_kf=False, found=None, cap_found=0, orb_dist=100, null_field=None):
        r = np.array(rows, np.int32); pk = (C.c_void_p * B)(*[None if k is None else k._kf for k in kfs])
        kr = M._KeyFrameRows(r.ctypes.data, C.cast(pk, C.c_void_p), cap_found, None if found is None else found.ctypes.data)
        if null_field:
            setattr(kr, null_field, None)
        return L.orbm_search_by_projection_keyframe_batch_map(ex._h, 0, B, fv, mp, None if null_kf else C.byref(kr), 10.0, orb_dist, 1, None)
    assert keyframe() == 0 and fetch() == 0
    assert keyframe(rows=(3, 3), kfs=(kf0, kf0)) == 0 and fetch() == 0 and (nm == 0).all() and (a == -1).all()       # empty rows
    refused(keyframe(mp=None)); refused(keyframe(null_kf=True)); refused(keyframe(null_field="row")); refused(keyframe(null_field="kfs"))
    refused(keyframe(rows=(0, -1)), "frame 1"); refused(keyframe(rows=(4, 2)), "frame 0")
    refused(keyframe(rows=(0, 1)), "never set")
    refused(keyframe(rows=(2, 2)), "frame 0"); refused(keyframe(kfs=(kf33, None)), "frame 1")
    fnd = np.zeros((B, 32), np.uint8)
    refused(keyframe(found=fnd, cap_found=32), "cap_found")
    fnd = np.zeros((B, 33), np.uint8)
    assert keyframe(found=fnd, cap_found=33) == 0 and fetch() == 0
    refused(keyframe(orb_dist=300))
    if L.orbx_device_count() >= 2:                                      # the map on another device than the handle
        other = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib, device_id=1)
        far = M.ResidentMap(other, 8, 1, 8, 1)
        refused(last(mp=far._m), "device"); refused(keyframe(mp=far._m), "device")
        far.close(); other.close()
    # ORBX_E_CAPACITY as the host-fed call: the accept kernel's LDS grows with cap_last
    big = 1 << 16
    nb = np.zeros(B, np.int32); sb = np.full((B, big), -1, np.int32); ob = np.zeros((B, big), np.int32)
    lbb = M._LastFrameSlots(big, nb.ctypes.data, sb.ctypes.data, None, ob.ctypes.data, ob.view(np.float32).ctypes.data, None)
    rc = L.orbm_search_by_projection_lastframe_batch_map(ex._h, 0, B, fv, store.map._m, C.byref(lbb), 7.0, None, None, 1, None, 0)
    lbh = M._LastFrameBatch(big, nb.ctypes.data, np.zeros((B, big, 3), np.float32).ctypes.data, np.zeros((B, big), np.uint8).ctypes.data, ob.ctypes.data, ob.view(np.float32).ctypes.data, None,
                            np.zeros((B, big, 32), np.uint8).ctypes.data)
    assert rc == L.orbm_search_by_projection_lastframe_batch(ex._h, 0, B, fv, C.byref(lbh), 7.0, None, None, 1, None, 0)
    assert rc in (0, E_CAPACITY) and fetch() == (E_ARG if rc else 0)
    for k in (kf33, kf10, kf0):
        k.close()
    store.close(); ex.close()
    assert _live(lib) == live0


def test_refusals_and_resources_emulated(emu_lib):
    _refusals(emu_lib)


@pytest.mark.gpu
def test_refusals_and_resources_gpu(hip_lib):
    _refusals(hip_lib)


def test_mirrors_have_the_header_layout(tmp_path):
    """OrbmLastFrameSlots and OrbmKeyFrameRows of include/orbx.h against their ctypes mirrors: fields, offsets, sizes"""
    mirrors = {"OrbmLastFrameSlots": M._LastFrameSlots, "OrbmKeyFrameRows": M._KeyFrameRows}
    fields = {"OrbmLastFrameSlots": ["cap_last", "n", "slots", "outlier", "octave", "angle", "has_obs"], "OrbmKeyFrameRows": ["row", "kfs", "cap_found", "found"]}
    lay = c_layout(tmp_path, fields)
    for name, cls in mirrors.items():
        assert [f[0] for f in cls._fields_] == fields[name]
        assert C.sizeof(cls) == lay[name]["."][0]
        for f in fields[name]:
            d = getattr(cls, f)
            assert (d.offset, d.size) == lay[name][f], "%s.%s" % (name, f)
