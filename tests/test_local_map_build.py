"""The map on the device (orbm_map): a store of map-point fields by slot, key-frame rows of slots, and Tracking::UpdateLocalPoints for a batch of
frames built by the kernels k_map_* into point sets that the batched searches take unchanged.

1. The list: `slots` / `seen` / M of every frame against _restate(), a restatement of src/Tracking.cc:4088-4120 and :3983-4019, on one world that holds
   the edge cases together, and on seeded random worlds.
2. The fields: orbm_points_fetch of every built set = the host's gather of the uploaded arrays, byte for byte; updates show in the next build.
3. The searches: the streams of tests/test_local_points_maps.py with all their maps in ONE store at permuted slots; the batched search on the map's
   sets against the reference's own Frame.cc + ORBmatcher.cc (oracle/_ref/libref_frame.so) called with the arrays gathered in the restated order.
4. Refusals and lifetime.

The world of 1. has frames that visit 0, 1, 63, 64, 65, 255, 256, 257 and more than 4096 positions.  Before the library is called the restatement alone
has to show, for every frame, that a quarter of the visited positions are repeats, one is bad, one is -1 and M_b > 0 - for every frame that visits at
least 4 positions: fewer cannot hold a first occurrence, a repeat, a bad point and a hole at once, so the frame of ONE position (a single good point)
is the one non-empty frame outside these four conditions."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor
from orb_slam3_detailed_comments_amd import matcher as M
from test_local_points import FX, FY, CX, CY, BF
from test_local_points_batch import PARAM_SETS
from test_local_points_maps import _streams, World, EMU_SHAPE, CAM, _live, E_ARG, E_CAPACITY

GPU_SHAPE = (640, 480, 1000, (5000, 0, 37, 1300, 64, 65))
needs_reference = pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so is not built")


def _restate(frame_rows, row_slots, present, bad, seen):
    """mvpLocalMapPoints of one frame as Tracking::UpdateLocalPoints builds it (src/Tracking.cc:4088-4120), and for each of its points whether
    SearchLocalPoints' first loop (:3983-4003) has stamped it with mnLastFrameSeen (what :4015 then skips).  frame_rows: the key frames in the order
    the reference walks them; row_slots[r]: GetMapPointMatches() of key frame r as slots, -1 = no map point"""
    out, stamped = [], set()
    for r in frame_rows:                                # :4096 for(vector<KeyFrame*>::const_reverse_iterator itKF ..)
        for s in row_slots[r]:                          # :4102 for(.. itMP = vpMPs.begin() ..)
            s = int(s)
            if s < 0:                                   # :4106 if(!pMP) continue
                continue
            if s in stamped:                            # :4110 if(pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue
                continue
            if present[s] and not bad[s]:               # :4112 if(!pMP->isBad())   (a slot that holds nothing is no map point at all)
                out.append(s); stamped.add(s)           # :4115-4116
    held = set(int(s) for s in seen) if seen is not None else set()
    return np.array(out, np.int32), np.array([s in held for s in out], np.uint8)


def _mixed_row(rng, n, pool, bads, absent):
    """n >= 4 entries: a first occurrence at the front, then in random order more first occurrences, repeats of them (30 %; a quarter below 20 entries),
    bad points, holes (-1) and slots that hold nothing"""
    n_rep = -(-3 * n // 10) if n >= 20 else -(-n // 4)
    n_bad, n_neg, n_abs = max(1, n // 15), max(1, n // 15), n // 20
    n_new = n - n_rep - n_bad - n_neg - n_abs
    assert n_new >= 1
    kinds = np.array(["new"] * (n_new - 1) + ["rep"] * n_rep + ["bad"] * n_bad + ["neg"] * n_neg + ["abs"] * n_abs)
    rng.shuffle(kinds)
    fresh = list(rng.choice(pool, n_new, replace=False))
    row, used = [], []
    for k in ["new"] + list(kinds):
        if k == "new":
            used.append(int(fresh.pop())); row.append(used[-1])
        elif k == "rep":
            row.append(used[int(rng.integers(0, len(used)))])
        else:
            row.append(-1 if k == "neg" else int(rng.choice(bads if k == "bad" else absent)))
    return np.array(row, np.int32)


S_SLOTS, ROW_CAP, N_ROWS, N_SETS = 5000, 1400, 24, 16
REPEAT_GAPS = ((1, 10), (63, 20), (64, 100), (65, 30), (1023, 40), (1024, 50), (1025, 60))        # (distance, position of the first of the pair) inside row 3


@functools.lru_cache(maxsize=None)
def _edge_world():
    """One world with the edge cases of the list together; plain arrays, built once, read-only"""
    rng = np.random.default_rng(11)
    S = S_SLOTS
    present = np.ones(S, bool); present[np.arange(S) % 17 == 5] = False; present[[0, S - 1]] = True
    bad = np.zeros(S, bool); bad[np.arange(S) % 11 == 3] = True; bad[[0, S - 1]] = False; bad &= present
    good = np.flatnonzero(present & ~bad); bads = np.flatnonzero(bad); absent = np.flatnonzero(~present)
    pool = np.unique(np.concatenate([[0, S - 1], rng.choice(good, 1500, replace=False)])).astype(np.int32)
    apart = np.setdiff1d(good, pool)                     # good slots that no generated row holds
    rows = [None] * N_ROWS
    rows[0] = np.zeros(0, np.int32)                      # a key frame without features
    rows[1] = np.full(50, -1, np.int32)                  # one without map points
    rows[2] = rng.choice(bads, 40).astype(np.int32)      # one whose points are all bad
    special = _mixed_row(rng, 1300, pool, bads, absent)
    for k, (gap, p) in enumerate(REPEAT_GAPS):           # pairs of one slot at the given distances; the slot occurs nowhere else
        special[p] = special[p + gap] = apart[k]
    special[5] = 0; special[7] = S - 1
    rows[3] = special
    rows[4] = np.array([apart[20]], np.int32)            # one good point
    for k, n in enumerate((63, 64, 65, 255, 256, 257)):
        rows[5 + k] = _mixed_row(rng, n, pool, bads, absent)
    for r, n in zip(range(11, N_ROWS), (1400, 900, 700, 800, 333, 1001, 1200) + tuple(int(v) for v in rng.integers(100, 1400, N_ROWS - 18))):
        rows[r] = _mixed_row(rng, n, pool, bads, absent)
    frames = [[], [0], [4], [5], [6], [7], [8], [9], [10],
              [3, 11, 12, 13, 11],                       # a row listed twice; more than 4096 positions
              [14, 15, 16], [16, 15, 14],                # the same rows in two orders
              [0, 1, 2, 17],                             # the empty row, the row of holes and the row of bad points in front of an ordinary one
              [18, 3]]
    other = [list(reversed(frames[(b + 3) % len(frames)])) for b in range(len(frames))]          # the second build: every set gets another frame's rows, reversed
    row_of = lambda fr: [np.concatenate([rows[r] for r in f] + [np.zeros(0, np.int32)]) for f in fr]

    def seen_lists(fr):
        out = []
        for b, f in enumerate(fr):
            ls, _ = _restate(f, rows, present, bad, None)
            if b % 4 == 3 or len(ls) == 0:
                out.append(None if b % 2 else np.array([1, 2, 3], np.int32))        # no list / a list although the frame has no local map
                continue
            inside = rng.choice(ls, max(1, len(ls) // 3))                           # with duplicates
            out.append(np.concatenate([inside, inside[:5], rng.choice(absent, 4), rng.choice(bads, 4), apart[30:40]]).astype(np.int32))
        return out
    fields = dict(pos=rng.normal(0, 3, (S, 3)).astype(np.float32), normal=rng.normal(0, 1, (S, 3)).astype(np.float32), mind=rng.uniform(0.1, 1, S).astype(np.float32),
                  maxd=rng.uniform(5, 50, S).astype(np.float32), desc=rng.integers(0, 256, (S, 32), dtype=np.uint8))
    W = dict(S=S, present=present, bad=bad, rows=rows, frames=frames, other=other, seen=seen_lists(frames), seen_other=seen_lists(other), fields=fields,
             positions=[len(p) for p in row_of(frames)], apart=apart, good=good)
    for a in [present, bad] + rows + list(fields.values()):
        a.setflags(write=False)
    return W


def test_the_edge_world_holds_its_cases():
    """from the restatement alone: the position counts are there, and equality on this world cannot pass on trivial input"""
    W = _edge_world()
    rows, present, bad = W["rows"], W["present"], W["bad"]
    assert {1, 63, 64, 65, 255, 256, 257} <= set(W["positions"]) and W["positions"].count(0) == 2 and max(W["positions"]) > 4096
    assert len(rows[0]) == 0 and (rows[1] == -1).all() and bad[rows[2]].all() and max(len(r) for r in rows) == ROW_CAP
    for fr, seen in ((W["frames"], W["seen"]), (W["other"], W["seen_other"])):
        for b, f in enumerate(fr):
            walk = np.concatenate([rows[r] for r in f] + [np.zeros(0, np.int32)])
            ls, sn = _restate(f, rows, present, bad, seen[b])
            if len(walk) < 4:
                assert len(walk) in (0, 1) and len(ls) == len(walk)
                continue
            valid = walk >= 0
            kept_again, met = 0, set()
            for s in walk.tolist():                      # repeats: positions whose good point an earlier position of this frame holds
                if s >= 0 and present[s] and not bad[s]:
                    kept_again += s in met
                    met.add(s)
            assert 4 * kept_again >= len(walk), "frame %d: %d repeats in %d positions" % (b, kept_again, len(walk))
            assert bad[walk[valid]].any() and (~valid).any() and len(ls) > 0, "frame %d" % b
            assert len(ls) + kept_again == (valid & present[np.maximum(walk, 0)] & ~bad[np.maximum(walk, 0)]).sum()
            if seen[b] is not None and len(seen[b]) > 3:
                assert sn.any() and not sn.all() and len(np.setdiff1d(seen[b], ls)) > 0 and len(seen[b]) > len(np.unique(seen[b]))
    special = rows[3]
    ls, _ = _restate([3], rows, present, bad, None)
    for gap, p in REPEAT_GAPS:                           # the planted pairs: the first of each is kept, the second is a repeat at exactly that distance
        assert special[p] == special[p + gap] and (special == special[p]).sum() == 2 and special[p] in ls
    assert 0 in ls and W["S"] - 1 in ls and (~present[np.concatenate(rows)[np.concatenate(rows) >= 0]]).any()
    a, b = (_restate(W["frames"][k], rows, present, bad, None)[0] for k in (10, 11))
    assert sorted(a) == sorted(b) and not np.array_equal(a, b)                  # two orders of the same rows give two orders of the same points
    assert all(len(np.unique(r[r >= 0])) < (r >= 0).sum() for r in rows[5:])          # the same slot inside one row twice


class _Store:
    """a ResidentMap filled from host arrays by slot, which it keeps for the gathers of the tests"""

    def __init__(self, lib, slots, kf_rows, row_cap, sets, fields, present, bad):
        self.lib = lib
        self.ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
        self.map = M.ResidentMap(self.ex, slots, kf_rows, row_cap, sets)
        self.f = {k: v.copy() for k, v in fields.items()}
        self.present, self.bad = present.copy(), bad.copy()
        ids = np.flatnonzero(present).astype(np.int32)
        rng = np.random.default_rng(3); rng.shuffle(ids)
        for part in np.array_split(ids, 3):                                     # several calls, slots in no order
            if len(part):
                self.update(part, self.bad[part])

    def update(self, slots, is_bad=None):
        f = self.f
        self.map.update(slots, f["pos"][slots], f["normal"][slots], f["mind"][slots], f["maxd"][slots], f["desc"][slots], is_bad)
        self.present[slots] = True; self.bad[slots] = False if is_bad is None else np.asarray(is_bad, bool)

    def check_set(self, b, slots):
        """the fields of set b are the host's gather by `slots`, byte for byte"""
        got = M.PointsFetch(self.ex, self.map.set(b))
        for g, name in zip(got, ("pos", "normal", "mind", "maxd", "desc")):
            assert g.tobytes() == self.f[name][slots].tobytes(), "%s of set %d" % (name, b)

    def build_and_check(self, frames, rows, seen, fields=True):
        """one orbm_map_local_points; every frame against the restatement.  Returns what was fetched"""
        Ms = self.map.local_points(frames, seen)
        out = []
        for b, f in enumerate(frames):
            ls, sn = _restate(f, rows, self.present, self.bad, None if seen is None else seen[b])
            got_s, got_n = self.map.fetch(b)
            assert Ms[b] == len(ls) and self.map.set(b).M == len(ls), "frame %d: %d points, the reference lists %d" % (b, Ms[b], len(ls))
            assert np.array_equal(got_s, ls), "frame %d: the list differs at %s" % (b, np.flatnonzero(got_s != ls)[:5])
            assert np.array_equal(got_n, sn), "frame %d: seen flags" % b
            if fields:
                self.check_set(b, ls)
            out.append((got_s, got_n))
        return out

    def close(self):
        self.map.close(); self.ex.close()


def _edge_store(lib):
    W = _edge_world()
    st = _Store(lib, W["S"], N_ROWS, ROW_CAP, N_SETS, W["fields"], W["present"], W["bad"])
    for r, row in enumerate(W["rows"]):
        st.map.set_keyframe(r, row)
    return W, st


def _list(lib):
    W, st = _edge_store(lib)
    try:
        first = st.build_and_check(W["frames"], W["rows"], W["seen"])
        raw = [M.PointsFetch(st.ex, st.map.set(b)) for b in range(len(W["frames"]))]
        # other lists on the same map: the stamps of the first build must not be seen; then the first lists again, byte for byte what they were
        st.build_and_check(W["other"], W["rows"], W["seen_other"])
        again = st.build_and_check(W["frames"], W["rows"], W["seen"])
        for b in range(len(W["frames"])):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first[b], again[b]))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(raw[b], M.PointsFetch(st.ex, st.map.set(b))))
        st.build_and_check(W["frames"], W["rows"], None, fields=False)              # without seen lists nothing is seen, whatever earlier builds marked
        # an epoch of 12 000 stamps holds two builds of this world (its longest walk is 5 700 positions): the third clears and starts over
        lib.check(lib.L.orbm_map_debug_epoch(st.ex._h, st.map._m, 12000))
        for k in range(7):
            fr, sn = ((W["frames"], W["seen"]), (W["other"], W["seen_other"]))[k % 2]
            st.build_and_check(fr, W["rows"], sn, fields=False)
        # an epoch shorter than the longest walk cannot hold it: refused, and the map goes on working once it is long enough again
        lib.check(lib.L.orbm_map_debug_epoch(st.ex._h, st.map._m, 5000))
        with pytest.raises(M.OrbxError) as e:
            st.map.local_points(W["frames"])
        assert e.value.code == E_CAPACITY and "frame 9" in str(e.value)
        lib.check(lib.L.orbm_map_debug_epoch(st.ex._h, st.map._m, 5700))             # exactly the longest walk: every build wraps
        for k in range(3):
            st.build_and_check(W["other"] if k % 2 else W["frames"], W["rows"], W["seen_other"] if k % 2 else W["seen"], fields=False)
    finally:
        st.close()


def test_list_emulated(emu_lib):
    _list(emu_lib)


@pytest.mark.gpu
def test_list_gpu(hip_lib):
    _list(hip_lib)


def _fuzz(lib, seeds):
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    try:
        for seed in seeds:
            rng = np.random.default_rng(1000 + seed)
            S = int(rng.integers(1, 301)); R = int(rng.integers(1, 13)); cap = int(rng.integers(1, 151)); B = int(rng.integers(1, 5))
            present = rng.uniform(size=S) < rng.uniform(0.3, 1.0); bad = (rng.uniform(size=S) < rng.uniform(0.0, 0.5)) & present
            rows = []
            for r in range(R):
                n = int(rng.integers(0, cap + 1))
                row = rng.integers(0, S, n).astype(np.int32)
                row[rng.uniform(size=n) < rng.uniform(0.0, 0.4)] = -1
                rows.append(row)
            mp = M.ResidentMap(ex, S, R, cap, 4)
            ids = np.flatnonzero(present).astype(np.int32)
            f = rng.integers(0, 256, (S, 32), dtype=np.uint8); z = np.zeros((S, 3), np.float32); o = np.ones(S, np.float32)
            if len(ids):
                mp.update(ids, z[ids], z[ids], o[ids], o[ids], f[ids], bad[ids])
            for r, row in enumerate(rows):
                mp.set_keyframe(r, row)
            for build in range(2):                         # twice on one map: other frames, the stamps of the first build still in place
                frames = [list(rng.integers(0, R, int(rng.integers(0, 7)))) for _ in range(B)]
                seen = None if rng.uniform() < 0.2 else [None if rng.uniform() < 0.2 else rng.integers(0, S, int(rng.integers(0, 40))).astype(np.int32) for _ in range(B)]
                Ms = mp.local_points(frames, seen)
                for b in range(B):
                    ls, sn = _restate(frames[b], rows, present, bad, None if seen is None else seen[b])
                    gs, gn = mp.fetch(b)
                    assert Ms[b] == len(ls) and np.array_equal(gs, ls) and np.array_equal(gn, sn), "seed %d, build %d, frame %d" % (seed, build, b)
                    assert M.PointsFetch(ex, mp.set(b))[4].tobytes() == f[ls].tobytes()
            mp.close()
    finally:
        ex.close()


def test_fuzz_emulated(emu_lib):
    _fuzz(emu_lib, range(200))


@pytest.mark.gpu
def test_fuzz_gpu(hip_lib):
    _fuzz(hip_lib, range(20))


def _fields(lib):
    W, st = _edge_store(lib)
    try:
        rows, frames = W["rows"], W["frames"]
        before = st.build_and_check(frames, rows, W["seen"])              # (every set against the host gather)
        # an explicit list with duplicates, bad points included, into a set of its own
        rng = np.random.default_rng(5)
        pick = np.concatenate([rng.choice(np.flatnonzero(st.present), 700), [0, 0, W["S"] - 1]]).astype(np.int32)
        st.map.select(15, pick)
        assert st.map.set(15).M == len(pick)
        st.check_set(15, pick)
        got_s, got_n = st.map.fetch(15)
        assert np.array_equal(got_s, pick) and not got_n.any()
        st.check_set(9, before[9][0])                                      # the other sets are what they were
        # new positions and descriptors for some points of the longest list, the bad flag for others (one absent slot among them: it stays absent)
        ls = before[9][0]
        moved, dropped = ls[10:400:3].copy(), ls[11:400:3].copy()
        st.f["pos"][moved] += np.float32(0.25); st.f["desc"][moved] ^= np.uint8(0x5A); st.f["normal"][moved] *= np.float32(-1); st.f["maxd"][moved] += np.float32(1)
        st.update(moved)
        absent = int(np.flatnonzero(~st.present)[0])
        st.map.set_bad(np.concatenate([dropped, [absent]]).astype(np.int32), np.ones(len(dropped) + 1, np.uint8))
        st.bad[dropped] = True
        after = st.build_and_check(frames, rows, W["seen"])
        assert not np.isin(dropped, after[9][0]).any() and np.isin(moved, after[9][0]).all() and len(after[9][0]) < len(ls)
        kept = np.setdiff1d(ls, np.concatenate([moved, dropped]))
        assert len(kept) > 500 and np.isin(kept, after[9][0]).all()       # untouched points are still listed, with the fields they had (build_and_check)
        # a point that was bad comes back: MapPoint flags are stored, not latched
        st.map.set_bad(dropped[:5], np.zeros(5, np.uint8)); st.bad[dropped[:5]] = False
        back = st.build_and_check(frames, rows, None)
        assert np.isin(dropped[:5], back[9][0]).all()
        # a set made by orbm_points_create gives back what was uploaded
        f = W["fields"]
        rp = M.ResidentPoints(st.ex, f["pos"][:301], f["normal"][:301], f["mind"][:301], f["maxd"][:301], f["desc"][:301])
        for g, name in zip(M.PointsFetch(st.ex, rp), ("pos", "normal", "mind", "maxd", "desc")):
            assert g.tobytes() == f[name][:301].tobytes()
        rp.close()
    finally:
        st.close()


def test_fields_emulated(emu_lib):
    _fields(emu_lib)


@pytest.mark.gpu
def test_fields_gpu(hip_lib):
    _fields(hip_lib)


# ---- 3. the searches on map-owned sets, against the reference ------------------------------------------------------------------------------

def _stream_layout(maps, seed):
    """every stream's map in ONE store at permuted slots; stream b's key-frame rows cover its map with repeats and holes, and its frame visits all of
    them (the first one twice).  Host arrays only: fields by slot, rows, frames, seen lists, present, bad"""
    rng = np.random.default_rng(seed)
    sizes = [0 if m is None else len(m["pos"]) for m in maps]
    total = sum(sizes)
    S = total + 97
    perm = rng.permutation(S)[:total].astype(np.int32)
    slot_of = np.split(perm, np.cumsum(sizes)[:-1])
    fields = dict(pos=np.zeros((S, 3), np.float32), normal=np.zeros((S, 3), np.float32), mind=np.zeros(S, np.float32), maxd=np.zeros(S, np.float32), desc=np.zeros((S, 32), np.uint8))
    present = np.zeros(S, bool); bad = np.zeros(S, bool)
    rows, frames, seen = [], [], []
    for b, m in enumerate(maps):
        if m is None:
            frames.append([]); seen.append(None)
            continue
        sl = slot_of[b]
        for k in fields:
            fields[k][sl] = m[k]
        present[sl] = True; bad[sl] = m["bad"].astype(bool)
        order = rng.permutation(sl)
        mine = []
        for part in np.array_split(order, max(2, min(6, len(sl) // 20))):
            again = rng.choice(order, max(1, len(part) // 3))                      # repeats: points other rows (or this one) hold as well
            row = np.concatenate([part, again, np.full(max(1, len(part) // 8), -1)]).astype(np.int32)
            rng.shuffle(row)
            mine.append(len(rows)); rows.append(row)
        frames.append(mine[::-1] + mine[:1])
        seen.append(np.concatenate([rng.choice(sl, max(1, len(sl) // 10)), perm[:3]]).astype(np.int32))
    return dict(S=S, fields=fields, rows=rows, frames=frames, seen=seen, present=present, bad=bad)


def _stream_store(ex, Y):
    """the ResidentMap of a _stream_layout()"""
    mp = M.ResidentMap(ex, Y["S"], len(Y["rows"]), max(len(r) for r in Y["rows"]), len(Y["frames"]))
    ids = np.flatnonzero(Y["present"]).astype(np.int32)
    f = Y["fields"]
    mp.update(ids, f["pos"][ids], f["normal"][ids], f["mind"][ids], f["maxd"][ids], f["desc"][ids], Y["bad"][ids])
    for r, row in enumerate(Y["rows"]):
        mp.set_keyframe(r, row)
    return mp


@functools.lru_cache(maxsize=None)
def _reference_on_lists(shape, seed):
    """What the reference finds for every stream of _streams(shape) against ITS list in the restated order (_stream_layout of that seed): per frame (slots, seen, mbTrackInView, assigned, nmatches) under PARAM_SETS[0].  The reference frames are built
    here and used at once (Frame keeps image bounds in static members)."""
    w, h, nf, sizes = shape
    pairs, _, poses, maps, _, _ = _streams(w, h, nf, sizes)
    layout = _stream_layout(maps, seed)
    th, far, _, cosl, thfar, ratio = PARAM_SETS[0]
    refs = [ol.ReferenceFrame(l, r, nf, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF) for l, r in pairs]
    out = []
    for b, m in enumerate(maps):
        ls, sn = _restate(layout["frames"][b], layout["rows"], layout["present"], layout["bad"], layout["seen"][b])
        if len(ls) == 0:
            out.append((ls, sn, None, None, 0))
            continue
        f = layout["fields"]
        tr, asg, n = refs[b].search_local_points(poses[b][0], poses[b][1], f["pos"][ls], f["normal"][ls], f["mind"][ls], f["maxd"][ls], sn, np.ones(len(ls), np.uint8), f["desc"][ls],
                                                 cosl, True, th, far, thfar, ratio)
        out.append((ls, sn, tr["in_view"].copy(), asg.copy(), n))
    return out


def _searches(lib, shape):
    W = World(lib, shape)
    mp = None
    try:
        expect = _reference_on_lists(shape, 77)
        Y = _stream_layout(W.maps, 77)
        mp = _stream_store(W.ex, Y)
        Ms = mp.local_points(Y["frames"], Y["seen"])
        sets, flags, lists = [], [], []
        for b in range(W.B):
            ls, sn = mp.fetch(b)
            assert Ms[b] == len(expect[b][0]) and np.array_equal(ls, expect[b][0]) and np.array_equal(sn, expect[b][1]), "frame %d: the list" % b
            sets.append(mp.set(b)); flags.append(sn); lists.append(ls)
        th, far, _, cosl, thfar, ratio = PARAM_SETS[0]
        lp = M.LocalPointsBatch(W.ex, sets, W.B, CAM, W.bounds, BF, W.sfs)
        lp.set_poses(W.poses)
        lp.enqueue(0, is_bad=flags, has_obs=None, viewing_cos_limit=cosl, th=th, far_points=far, th_far=thfar, nnratio=ratio, want_in_view=True)
        asg, nm, inv = lp.fetch()
        for b in range(W.B):
            ls, sn, ref_inv, ref_as, ref_n = expect[b]
            N = W.refs[b].N
            print("frame %d: %d points of a map of %d, %d seen, %d matches (reference %d)" % (b, len(ls), W.sizes[b], sn.sum(), nm[b], ref_n))
            if len(ls) == 0:
                assert W.sizes[b] == 0 and nm[b] == 0 and (asg[b] == -1).all() and not inv[b].any()
                continue
            assert ref_n >= len(ls) / 8.0, "frame %d: the reference finds %d of %d points" % (b, ref_n, len(ls))
            to_slot = lambda a, l: np.where(a >= 0, l[np.maximum(a, 0)], -1)            # the MapPoint behind a local index
            assert nm[b] == ref_n and np.array_equal(to_slot(asg[b, :N], lists[b]), to_slot(ref_as, ls)), "frame %d: %d vs %d matches" % (b, nm[b], ref_n)
            assert (asg[b, N:] == -1).all()
            assert np.array_equal(inv[b, :len(ls)].astype(bool), ref_inv) and not inv[b, len(ls):].any(), "mbTrackInView, frame %d" % b
        # the sets are the map's: destroying one through the points call changes nothing
        lib.L.orbm_points_destroy(sets[0]._p)
        lp.enqueue(0, is_bad=flags, has_obs=None, viewing_cos_limit=cosl, th=th, far_points=far, th_far=thfar, nnratio=ratio)
        asg2, nm2, _ = lp.fetch()
        assert np.array_equal(nm2, nm) and np.array_equal(asg2, asg)
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_searches_emulated(emu_lib):
    _searches(emu_lib, EMU_SHAPE)


@needs_reference
@pytest.mark.gpu
def test_searches_gpu(hip_lib):
    _searches(hip_lib, GPU_SHAPE)


def _rig_batch(lib):
    """LocalPointsRigBatch on map-owned sets = the same call on ResidentPoints made from the gathered arrays"""
    import test_rig_local_points_maps as RG
    W = RG.World(lib, RG.EMU_SHAPE)
    mp = None
    try:
        Y = _stream_layout(W.maps, 78)
        fields = Y["fields"]
        mp = _stream_store(W.ex, Y)
        Ms = mp.local_points(Y["frames"], Y["seen"])
        lists = [mp.fetch(b) for b in range(W.B)]
        assert sum(Ms > 0) >= 3 and min(Ms) == 0
        rps = [M.ResidentPoints(W.ex, fields["pos"][ls], fields["normal"][ls], fields["mind"][ls], fields["maxd"][ls], fields["desc"][ls]) if len(ls) else None for ls, _ in lists]
        flags = [sn for _, sn in lists]
        res = []
        for sets in ([mp.set(b) for b in range(W.B)], rps):
            lp = W.batch(sets)
            lp.enqueue(is_bad=flags, has_obs=None, th=3.0, far_points=True, th_far=9.0, nnratio=0.8, want_in_view=True)
            res.append([x.copy() for x in lp.fetch()])
        for x, y in zip(*res):
            assert np.array_equal(x, y)
        assert res[0][1].sum() > 50
        for r in rps:
            if r is not None:
                r.close()
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_rig_batch_on_map_sets_emulated(emu_lib):
    _rig_batch(emu_lib)


@needs_reference
@pytest.mark.gpu
def test_rig_batch_on_map_sets_gpu(hip_lib):
    _rig_batch(hip_lib)


def _fuse_batch(lib):
    """FuseCandidatesBatch with the point set selected from the map = the same call on a ResidentPoints of the same arrays"""
    import test_fuse_batch as FB
    Sc = FB.scene()
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    mp = None
    try:
        rng = np.random.default_rng(8)
        slots = rng.permutation(Sc.M + 50)[:Sc.M].astype(np.int32)
        mp = M.ResidentMap(ex, Sc.M + 50, 1, 8, 2)
        mp.update(slots, Sc.pos, Sc.normal, Sc.mind, Sc.maxd, Sc.desc)
        mp.select(1, slots)
        kfs, specs = Sc.resident(ex)
        rp = Sc.points(ex)
        for th, chi2 in ((3.0, True), (6.0, False)):
            s2 = Sc.inv_sigma2 if chi2 else None
            bi, bd = M.ORBmatcher.FuseCandidatesBatch(ex, kfs, specs, mp.set(1), th, s2)
            ri, rd = M.ORBmatcher.FuseCandidatesBatch(ex, kfs, specs, rp, th, s2)
            assert np.array_equal(bi, ri) and np.array_equal(bd, rd) and (ri >= 0).sum() > 100
        rp.close()
        for k in kfs:
            k.close()
    finally:
        if mp is not None:
            mp.close()
        ex.close()


def test_fuse_batch_on_a_selected_set_emulated(emu_lib):
    _fuse_batch(emu_lib)


@pytest.mark.gpu
def test_fuse_batch_on_a_selected_set_gpu(hip_lib):
    _fuse_batch(hip_lib)


# ---- 4. refusals and lifetime -----------------------------------------------------------------------------------------------------------------

def _refusals(lib, two_devices):
    L = lib.L
    live0 = _live(lib)
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    h = ex._h
    err = lambda: L.orbx_last_error()
    i32 = lambda *v: np.array(v, np.int32)
    mh = C.c_void_p()
    live_ex = _live(lib)
    for args, code in (((0, 4, 8, 2), E_ARG), ((10, -1, 8, 2), E_ARG), ((10, 4, -8, 2), E_ARG), ((10, 4, 8, 0), E_ARG), ((1 << 29, 4, 8, 2), E_CAPACITY), ((10, 4, 8, 70000), E_CAPACITY)):
        assert L.orbm_map_create(h, *args, C.byref(mh)) == code and not mh.value
    assert L.orbm_map_create(None, 10, 4, 8, 2, C.byref(mh)) == E_ARG and L.orbm_map_create(h, 10, 4, 8, 2, None) == E_ARG
    assert _live(lib) == live_ex                                           # a refused map holds nothing
    S, R, CAP, SETS = 40, 4, 8, 2
    mp = M.ResidentMap(ex, S, R, CAP, SETS)
    m = mp._m
    assert _live(lib)[0] > live_ex[0]                                      # the map's allocations are counted
    rng = np.random.default_rng(2)
    pos = rng.normal(0, 1, (S, 3)).astype(np.float32); one = np.ones(S, np.float32); desc = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    ids = np.arange(0, 30, dtype=np.int32)
    mp.update(ids, pos[ids], pos[ids], one[ids], one[ids], desc[ids])
    mp.set_keyframe(0, i32(3, 4, -1, 5, 3)); mp.set_keyframe(1, i32(5, 6, 35, 7))

    def usable():
        assert np.array_equal(mp.local_points([[0, 1], [1]]), [5, 3])
        assert np.array_equal(mp.fetch(0)[0], [3, 4, 5, 6, 7]) and np.array_equal(mp.fetch(1)[0], [5, 6, 7])
    usable()
    V = M._WorldPointView(); V.M = 2
    V.pos = V.normal = pos.ctypes.data; V.min_distance = V.max_distance = one.ctypes.data; V.desc = desc.ctypes.data
    keep = []

    def ptr(a):
        keep.append(a)                                                     # (the array outlives the call it is an argument of)
        return a.ctypes.data
    two = i32(1, 2)
    Mo = np.zeros(4, np.int32)
    cases = [
        (lambda: L.orbm_map_update(h, m, 2, ptr(two), None), E_ARG, None),
        (lambda: L.orbm_map_update(h, m, 2, None, C.byref(V)), E_ARG, None),
        (lambda: L.orbm_map_update(h, None, 2, ptr(two), C.byref(V)), E_ARG, None),
        (lambda: L.orbm_map_update(None, m, 2, ptr(two), C.byref(V)), E_ARG, None),
        (lambda: L.orbm_map_update(h, m, -1, ptr(two), C.byref(V)), E_ARG, None),
        (lambda: L.orbm_map_update(h, m, 3, ptr(i32(1, 2, 3)), C.byref(V)), E_ARG, None),                    # view->M != n
        (lambda: L.orbm_map_update(h, m, 2, ptr(i32(1, S)), C.byref(V)), E_ARG, b"entry 1"),
        (lambda: L.orbm_map_update(h, m, 2, ptr(i32(-1, 2)), C.byref(V)), E_ARG, b"entry 0"),
        (lambda: L.orbm_map_update(h, m, 2, ptr(i32(7, 7)), C.byref(V)), E_ARG, b"twice"),
        (lambda: L.orbm_map_set_bad(h, m, 2, ptr(i32(7, 7)), ptr(np.ones(2, np.uint8))), E_ARG, b"twice"),
        (lambda: L.orbm_map_set_bad(h, m, 2, ptr(two), None), E_ARG, None),
        (lambda: L.orbm_map_set_bad(h, m, 2, ptr(i32(1, S + 3)), ptr(np.ones(2, np.uint8))), E_ARG, b"entry 1"),
        (lambda: L.orbm_map_set_keyframe(h, m, R, 2, ptr(two)), E_ARG, b"row 4"),
        (lambda: L.orbm_map_set_keyframe(h, m, -1, 2, ptr(two)), E_ARG, b"row -1"),
        (lambda: L.orbm_map_set_keyframe(h, m, 2, CAP + 1, ptr(np.zeros(CAP + 1, np.int32))), E_CAPACITY, b"row 2"),
        (lambda: L.orbm_map_set_keyframe(h, m, 2, 2, None), E_ARG, b"row 2"),
        (lambda: L.orbm_map_set_keyframe(h, m, 2, -2, ptr(two)), E_ARG, b"row 2"),
        (lambda: L.orbm_map_set_keyframe(h, m, 2, 2, ptr(i32(1, S))), E_ARG, b"row 2"),
        (lambda: L.orbm_map_set_keyframe(h, m, 2, 2, ptr(i32(1, -2))), E_ARG, b"row 2"),
        (lambda: L.orbm_map_local_points(h, m, SETS + 1, ptr(i32(0, 1, 2, 3)), ptr(i32(0, 1, 0)), None, None, ptr(Mo)), E_CAPACITY, None),
        (lambda: L.orbm_map_local_points(h, m, -1, ptr(i32(0, 1)), ptr(i32(0)), None, None, ptr(Mo)), E_ARG, None),
        (lambda: L.orbm_map_local_points(h, m, 2, None, ptr(i32(0)), None, None, ptr(Mo)), E_ARG, None),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), ptr(i32(0, 1)), None, None, None), E_ARG, None),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), None, None, None, ptr(Mo)), E_ARG, b"frame 0"),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), ptr(i32(0, R)), None, None, ptr(Mo)), E_ARG, b"frame 1"),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), ptr(i32(-1, 0)), None, None, ptr(Mo)), E_ARG, b"frame 0"),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 2, 1)), ptr(i32(0, 1)), None, None, ptr(Mo)), E_ARG, b"frame 1"),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), ptr(i32(0, 1)), ptr(i32(0, 1, 2)), ptr(i32(3, S)), ptr(Mo)), E_ARG, b"frame 1"),
        (lambda: L.orbm_map_local_points(h, m, 2, ptr(i32(0, 1, 2)), ptr(i32(0, 1)), ptr(i32(0, 1, 2)), None, ptr(Mo)), E_ARG, b"frame 0"),
        (lambda: L.orbm_map_select(h, m, SETS, 2, ptr(two)), E_ARG, b"set 2"),
        (lambda: L.orbm_map_select(h, m, -1, 2, ptr(two)), E_ARG, None),
        (lambda: L.orbm_map_select(h, m, 1, 2, None), E_ARG, None),
        (lambda: L.orbm_map_select(h, m, 1, -2, ptr(two)), E_ARG, None),
        (lambda: L.orbm_map_select(h, m, 1, 2, ptr(i32(1, S))), E_ARG, b"entry 1"),
        (lambda: L.orbm_map_select(h, m, 1, 2, ptr(i32(1, 35))), E_ARG, b"entry 1"),                          # a slot that holds nothing
        (lambda: L.orbm_map_set_fetch(h, m, SETS, ptr(Mo), None), E_ARG, None),
        (lambda: L.orbm_map_set_fetch(h, None, 0, ptr(Mo), None), E_ARG, None),
        (lambda: L.orbm_points_fetch(h, None, None, None, None, None, None), E_ARG, None),
        (lambda: L.orbm_points_fetch(None, mp.set(0)._p, None, None, None, None, None), E_ARG, None),
        (lambda: L.orbm_map_debug_epoch(h, None, 0), E_ARG, None),
    ]
    for k, (call, code, word) in enumerate(cases):
        assert call() == code, "case %d" % k
        assert word is None or word in err(), "case %d: %s" % (k, err())
        usable()
    assert not L.orbm_map_set(h, m, SETS) and not L.orbm_map_set(h, m, -1) and not L.orbm_map_set(None, m, 0) and not L.orbm_map_set(h, None, 0)
    m2 = M.ResidentMap(ex, S, R, CAP, 3)
    assert not L.orbm_map_set(h, m2._m, 1)                                  # a set that was never built
    m2.select(1, i32()); assert m2.set(1).M == 0 and len(m2.fetch(1)[0]) == 0
    m2.close()
    # B = 0, n = 0 and empty frames are not errors
    assert L.orbm_map_local_points(h, m, 0, None, None, None, None, None) == 0 and L.orbm_map_update(h, m, 0, None, None) == 0 and L.orbm_map_set_bad(h, m, 0, None, None) == 0
    assert np.array_equal(mp.local_points([[], []]), [0, 0]) and mp.set(0).M == 0 and mp.set(1).M == 0
    usable()
    # destroying a map-owned set changes nothing
    p0 = mp.set(0)
    live1 = _live(lib)
    L.orbm_points_destroy(p0._p)
    assert _live(lib) == live1 and np.array_equal(M.PointsFetch(ex, mp.set(0))[4], desc[[3, 4, 5, 6, 7]])
    # buffers are reused: the same builds again allocate nothing
    usable()
    assert _live(lib) == live1
    other = None
    if two_devices:
        other = ORBextractor(300, 1.2, 8, 20, 7, lib=lib, device_id=1)
        for call in (lambda: L.orbm_map_update(other._h, m, 2, ptr(two), C.byref(V)), lambda: L.orbm_map_set_bad(other._h, m, 2, ptr(two), ptr(np.ones(2, np.uint8))),
                     lambda: L.orbm_map_set_keyframe(other._h, m, 0, 2, ptr(two)), lambda: L.orbm_map_local_points(other._h, m, 1, ptr(i32(0, 1)), ptr(i32(0)), None, None, ptr(Mo)),
                     lambda: L.orbm_map_select(other._h, m, 0, 2, ptr(two)), lambda: L.orbm_map_set_fetch(other._h, m, 0, ptr(Mo), None),
                     lambda: L.orbm_points_fetch(other._h, mp.set(0)._p, None, None, None, None, None)):
            assert call() == E_ARG and b"device" in err()
        assert not L.orbm_map_set(other._h, m, 0)
        usable()
    # a second handle on the map's device may use it
    ex2 = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    mp.set_bad(i32(4), np.ones(1, np.uint8), ext=ex2)
    assert np.array_equal(mp.local_points([[0, 1]], ext=ex2), [4]) and np.array_equal(mp.fetch(0, ext=ex2)[0], [3, 5, 6, 7])
    for o in (mp, ex2, other, ex):
        if o is not None:
            o.close()
    assert _live(lib) == live0


def test_refusals_and_lifetime_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("ORBX_EMU_DEVICES", "2")
    assert emu_lib.L.orbx_device_count() == 2
    _refusals(emu_lib, True)


@pytest.mark.gpu
def test_refusals_and_lifetime_gpu(hip_lib):
    _refusals(hip_lib, False)


def test_map_calls_take_the_extractor_first():
    """tests/null_argument_runner.py hands a live extractor to the first pointer of every orbm_ symbol: the map calls have to take one there"""
    import os
    import re
    hdr = open(os.path.join(ol.ROOT, "include", "orbx.h")).read()
    decls = re.findall(r"\b(orbm_map_[a-z_]+|orbm_points_fetch)\s*\(([^)]*)\)\s*;", hdr)
    assert len(decls) == 11
    for name, args in decls:
        assert args.split(",")[0].strip() == "orbx_extractor* h", name
