"""Tracking::SearchLocalPoints on the map's own sets (orbm_search_local_points_batch_map / _rig_batch_map, the .._fetch_slots calls,
orbm_map_sets_fetch): frame b is searched against set set0 + b of an orbm_map where the build left it - k_map_set_flags writes the set's seen bytes
as the search's is_bad at the unaligned prefix-sum offsets of the batch, k_assigned_slots turns `assigned` into map slots behind the accept loop -
so neither a flag array nor a list crosses the bus.

1. Reference parity, one camera: the streams of tests/test_local_points_maps.py in one store (tests/test_local_map_build.py), the map form and
   fetch_slots against the reference's own search on the restated lists.
2. The plain fetch of a map batch = orbm_search_local_points_batch_maps with fetched flags; after a rebuild with other seen lists the flags follow.
3. What the equalities rest on (no library): another frame's list changes the slots, ignoring `seen` changes the match counts.
4. Rig frames against orbm_search_local_points_rig_batch_maps, both halves of `assigned` translated.
5. set0 > 0, sets made by orbm_map_select, orbm_map_sets_fetch against single fetches.
6. Pool overflow through fetch_slots.
7. Refusals, the three handle states, resources."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, synth
from orb_slam3_detailed_comments_amd import matcher as M
from test_local_points import FX, FY, CX, CY, BF
from test_local_points_batch import PARAM_SETS
from test_local_points_maps import _streams, World, EMU_SHAPE, CAM, _live, E_ARG, E_CAPACITY
from test_local_map_build import _restate, _stream_layout, _stream_store, _reference_on_lists

needs_reference = pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so is not built")
# maps of the wave and the block edge and one past each, an empty one, one below a wave (the lists are what is left of them without the bad points;
# _parity checks that their prefix sums put flag rows at dword multiples and off them)
EDGE_SHAPE = (EMU_SHAPE[0], EMU_SHAPE[1], EMU_SHAPE[2], (0, 37, 64, 65, 256, 257, 300))
SEED = 77
TH, FAR, _, COSL, THFAR, RATIO = PARAM_SETS[0]
KW = dict(viewing_cos_limit=COSL, th=TH, far_points=FAR, th_far=THFAR, nnratio=RATIO)


def to_slot(a, l):
    """the MapPoint (slot) behind a local index; negative entries pass through"""
    a = np.asarray(a)
    return np.where(a >= 0, l[np.maximum(a, 0)] if len(l) else -1, a)


def _other_seen(layout, b):
    """the seen list of stream b for the SECOND build: other slots of its map than the layout's own list"""
    if layout["seen"][b] is None:
        return None
    rng = np.random.default_rng(500 + b)
    ls, _ = _restate(layout["frames"][b], layout["rows"], layout["present"], layout["bad"], None)
    return rng.choice(ls, max(1, len(ls) // 4)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference_variant(shape, seed, variant):
    """_reference_on_lists under other flags: variant "other" = the seen lists of _other_seen (the rebuild of test 2), "ignored" = no point seen.
    Per frame (slots, seen, mbTrackInView, assigned, nmatches).  The reference frames are built here and used at once."""
    w, h, nf, sizes = shape
    pairs, _, poses, maps, _, _ = _streams(w, h, nf, sizes)
    layout = _stream_layout(maps, seed)
    refs = [ol.ReferenceFrame(l, r, nf, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF) for l, r in pairs]
    out = []
    for b in range(len(maps)):
        ls, sn = _restate(layout["frames"][b], layout["rows"], layout["present"], layout["bad"], _other_seen(layout, b) if variant == "other" else None)
        if len(ls) == 0:
            out.append((ls, sn, None, None, 0))
            continue
        f = layout["fields"]
        tr, asg, n = refs[b].search_local_points(poses[b][0], poses[b][1], f["pos"][ls], f["normal"][ls], f["mind"][ls], f["maxd"][ls], sn, np.ones(len(ls), np.uint8), f["desc"][ls],
                                                 COSL, True, TH, FAR, THFAR, RATIO)
        out.append((ls, sn, tr["in_view"].copy(), asg.copy(), n))
    return out


def _map_batch(W, mp, set0=0, B=None):
    lp = M.LocalPointsBatch(W.ex, mp, W.B if B is None else B, CAM, W.bounds, BF, W.sfs, set0=set0)
    lp.set_poses(W.poses)
    return lp


def _against_reference(W, expect, asg_slots, nm, inv, what):
    for b in range(W.B):
        ls, sn, ref_inv, ref_as, ref_n = expect[b]
        N = W.refs[b].N
        print("%s, frame %d: %d points of a map of %d, %d seen, %d matches (reference %d)" % (what, b, len(ls), W.sizes[b], sn.sum(), nm[b], ref_n))
        if len(ls) == 0:
            assert nm[b] == 0 and (asg_slots[b] == -1).all() and not inv[b].any(), "%s, frame %d has an empty set" % (what, b)
            continue
        assert ref_n >= len(ls) / 8.0, "frame %d: the reference finds %d of %d points" % (b, ref_n, len(ls))
        assert nm[b] == ref_n and np.array_equal(asg_slots[b, :N], to_slot(ref_as, ls)), "%s, frame %d: %d vs %d matches" % (what, b, nm[b], ref_n)
        assert (asg_slots[b, N:] == -1).all()
        assert np.array_equal(inv[b, :len(ls)].astype(bool), ref_inv) and not inv[b, len(ls):].any(), "%s: mbTrackInView, frame %d" % (what, b)


# ---- 1. the map form and fetch_slots against the reference ---------------------------------------------------------------------------------

def _parity(lib, shape):
    W = World(lib, shape)
    mp = None
    try:
        expect = _reference_on_lists(shape, SEED)
        Y = _stream_layout(W.maps, SEED)
        mp = _stream_store(W.ex, Y)
        Ms = mp.local_points(Y["frames"], Y["seen"])
        assert list(Ms) == [len(e[0]) for e in expect]
        assert min(Ms) == 0 and sum(e[1].sum() > 0 for e in expect) >= 2, "an empty set, and sets that hold seen points"
        offs = [int(o) for o, m in zip(np.cumsum(Ms) - Ms, Ms) if m >= 8]
        print("set sizes %s, flag offsets %s" % (list(Ms), offs))
        assert any(o % 4 == 0 for o in offs) and any(o % 4 for o in offs), "the flag kernel's dword form and its byte form both have rows to copy"
        lp = _map_batch(W, mp)
        lp.enqueue(0, want_in_view=True, **KW)
        asg, nm, inv = lp.fetch_slots()
        assert inv.shape == (W.B, max(max(Ms), 1))
        _against_reference(W, expect, asg, nm, inv, "map form")
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_parity_emulated(emu_lib):
    _parity(emu_lib, EMU_SHAPE)


@needs_reference
@pytest.mark.gpu
def test_parity_gpu(hip_lib):
    _parity(hip_lib, EMU_SHAPE)


@needs_reference
def test_parity_wave_and_block_edges_emulated(emu_lib):
    _parity(emu_lib, EDGE_SHAPE)


@needs_reference
@pytest.mark.gpu
def test_parity_wave_and_block_edges_gpu(hip_lib):
    _parity(hip_lib, EDGE_SHAPE)


# ---- 2. the plain fetch, and flags that follow a rebuild ------------------------------------------------------------------------------------

def _plain_fetch_and_rebuild(lib):
    W = World(lib, EMU_SHAPE)
    mp = None
    try:
        Y = _stream_layout(W.maps, SEED)
        mp = _stream_store(W.ex, Y)
        first = None
        for variant, seen in (("first", Y["seen"]), ("other", [_other_seen(Y, b) for b in range(W.B)])):
            mp.local_points(Y["frames"], seen)
            lists = [mp.fetch(b) for b in range(W.B)]
            host = W.batch([mp.set(b) for b in range(W.B)])
            host.enqueue(0, is_bad=[sn for _, sn in lists], has_obs=None, want_in_view=True, **KW)
            a0, n0, v0 = [x.copy() for x in host.fetch()]
            lp = _map_batch(W, mp)
            lp.enqueue(0, want_in_view=True, **KW)
            a1, n1, v1 = [x.copy() for x in lp.fetch()]            # list positions
            assert np.array_equal(a1, a0) and np.array_equal(n1, n0) and np.array_equal(v1, v0), "%s build: the plain fetch of the map batch" % variant
            a2, n2, v2 = lp.fetch_slots()                          # the same pending batch, as slots
            assert np.array_equal(n2, n0) and np.array_equal(v2, v0)
            for b in range(W.B):
                assert np.array_equal(a2[b], to_slot(a0[b], lists[b][0])), "%s build, frame %d: slots of the plain fetch's positions" % (variant, b)
            expect = _reference_on_lists(EMU_SHAPE, SEED) if variant == "first" else _reference_variant(EMU_SHAPE, SEED, "other")
            for b in range(W.B):
                assert np.array_equal(lists[b][1], expect[b][1]), "%s build, frame %d: the seen bytes" % (variant, b)
            _against_reference(W, expect, a2, n2, v2, "%s build" % variant)
            if first is None:
                first = (a2.copy(), n2.copy())
        assert not np.array_equal(first[1], n2) and not np.array_equal(first[0], a2), "the rebuild with other seen lists changed nothing"
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_plain_fetch_and_rebuild_emulated(emu_lib):
    _plain_fetch_and_rebuild(emu_lib)


@needs_reference
@pytest.mark.gpu
def test_plain_fetch_and_rebuild_gpu(hip_lib):
    _plain_fetch_and_rebuild(hip_lib)


# ---- 3. what the equalities rest on ------------------------------------------------------------------------------------------------------------

@needs_reference
def test_wrong_list_or_ignored_seen_would_be_noticed():
    """translating with ANOTHER frame's list changes assigned slots, and a search that ignores `seen` finds other match counts - in the fixture of
    test 1, on the reference alone"""
    for shape in (EMU_SHAPE, EDGE_SHAPE):
        expect = _reference_on_lists(shape, SEED)
        full = [b for b, e in enumerate(expect) if len(e[0])]
        assert len(full) >= 3
        for b, o in zip(full, full[1:] + full[:1]):
            ls, _, _, ref_as, ref_n = expect[b]
            other = expect[o][0]
            wrong = to_slot(np.where(ref_as >= 0, np.minimum(ref_as, len(other) - 1), ref_as), other)
            assert ref_n > 0 and (wrong != to_slot(ref_as, ls)).any(), "frame %d translated with frame %d's list" % (b, o)
        ignored = _reference_variant(shape, SEED, "ignored")
        changed = [b for b in full if ignored[b][4] != expect[b][4]]
        print("%s: nmatches with seen %s, ignored %s" % (shape[3], [e[4] for e in expect], [e[4] for e in ignored]))
        assert changed, "ignoring the seen bytes changes no match count"
    other = _reference_variant(EMU_SHAPE, SEED, "other")
    assert any(o[4] != e[4] for o, e in zip(other, _reference_on_lists(EMU_SHAPE, SEED)))


# ---- 4. rig frames -----------------------------------------------------------------------------------------------------------------------------------

def _rig(lib):
    import test_rig_local_points_maps as RG
    W = RG.World(lib, RG.EMU_SHAPE)
    mp = None
    try:
        Y = _stream_layout(W.maps, 78)
        mp = _stream_store(W.ex, Y)
        Ms = mp.local_points(Y["frames"], Y["seen"])
        start, slots, seen = mp.fetch_sets(0, W.B)
        lists = [(slots[start[b]:start[b + 1]], seen[start[b]:start[b + 1]]) for b in range(W.B)]
        assert sum(Ms > 0) >= 3 and min(Ms) == 0 and seen.sum() > 0
        kw = dict(th=3.0, far_points=True, th_far=9.0, nnratio=0.8, want_in_view=True)
        host = W.batch([mp.set(b) for b in range(W.B)])
        host.enqueue(is_bad=[sn for _, sn in lists], has_obs=None, **kw)
        a0, n0, v0, r0 = [x.copy() for x in host.fetch()]
        lp = M.LocalPointsRigBatch(W.ex, W.ex, mp, W.B, RG.CAM1, RG.CAM2, W.bounds, W.sfs, 0, W.B)
        lp.set_poses(W.rig_poses)
        lp.enqueue(**kw)
        a1, n1, v1, r1 = [x.copy() for x in lp.fetch()]
        assert np.array_equal(a1, a0) and np.array_equal(n1, n0) and np.array_equal(v1, v0) and np.array_equal(r1, r0)
        a2, n2, v2, r2 = lp.fetch_slots()
        assert np.array_equal(n2, n0) and np.array_equal(v2, v0) and np.array_equal(r2, r0) and n0.sum() > 50
        for b, F in enumerate(W.refs):
            assert np.array_equal(a2[b], to_slot(a0[b], lists[b][0])), "frame %d" % b
            if Ms[b] >= 45:             # both cameras' halves hold translated entries
                assert (a2[b, :F.nl] >= 0).any() and (a2[b, F.nl:F.nl + F.nr] >= 0).any(), "frame %d: a camera without matches" % b
        # the one-camera fetches refuse a rig batch and leave it pending
        assert lib.L.orbm_search_local_points_fetch_slots(W.ex._h, a2.ctypes.data, 2 * W.cap, n2.ctypes.data, None) == E_ARG
        assert lp.fetch_slots()[1].sum() == n0.sum()
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_rig_emulated(emu_lib):
    _rig(emu_lib)


@needs_reference
@pytest.mark.gpu
def test_rig_gpu(hip_lib):
    _rig(hip_lib)


# ---- 5. set0 > 0, selected sets, orbm_map_sets_fetch ----------------------------------------------------------------------------------------------

def _set0_select_and_sets_fetch(lib):
    W = World(lib, EMU_SHAPE)
    mp = None
    try:
        Y = _stream_layout(W.maps, SEED)
        B, SHIFT, SEL = W.B, 2, W.B + 3
        mp = M.ResidentMap(W.ex, Y["S"], len(Y["rows"]), max(len(r) for r in Y["rows"]), SEL + B + 1)
        ids = np.flatnonzero(Y["present"]).astype(np.int32)
        f = Y["fields"]
        mp.update(ids, f["pos"][ids], f["normal"][ids], f["mind"][ids], f["maxd"][ids], f["desc"][ids], Y["bad"][ids])
        for r, row in enumerate(Y["rows"]):
            mp.set_keyframe(r, row)
        # built sets SHIFT .. SHIFT + B - 1 hold the streams (sets 0, 1 hold other walks); selected sets SEL .. hold the same lists without seen flags
        Ms = mp.local_points([Y["frames"][2], []] + list(Y["frames"]), [None, None] + list(Y["seen"]))
        assert list(Ms[SHIFT:]) == [len(e[0]) for e in _reference_on_lists(EMU_SHAPE, SEED)]
        lists = [mp.fetch(SHIFT + b) for b in range(B)]
        for b in range(B):
            mp.select(SEL + b, lists[b][0])
        first_n = None
        for set0, flags in ((SHIFT, [sn for _, sn in lists]), (SEL, None)):
            host = W.batch([mp.set(set0 + b) for b in range(B)])
            host.enqueue(0, is_bad=flags, has_obs=None, want_in_view=True, **KW)
            a0, n0, v0 = [x.copy() for x in host.fetch()]
            lp = _map_batch(W, mp, set0)
            lp.enqueue(0, want_in_view=True, **KW)
            a1, n1, v1 = lp.fetch_slots()
            assert np.array_equal(n1, n0) and np.array_equal(v1, v0) and n0.sum() > 100, "set0 = %d" % set0
            for b in range(B):
                assert np.array_equal(a1[b], to_slot(a0[b], lists[b][0])), "set0 = %d, frame %d" % (set0, b)
            if first_n is not None:
                assert not np.array_equal(n0, first_n), "a selected set has seen = 0: the seen points match again"
            first_n = n0
        # a set that was never built inside the range: an empty map for its frame (set SEL + B exists and is unbuilt)
        lp = _map_batch(W, mp, SEL + 1)
        lp.enqueue(0, **KW)
        a, n, _ = lp.fetch_slots()
        assert n[B - 1] == 0 and (a[B - 1] == -1).all() and n[:B - 1].sum() > 0
        # orbm_map_sets_fetch: B single fetches in one call, spans with slack, NULL outputs, an empty set in the middle
        start, slots, seen = mp.fetch_sets(SHIFT, B)
        assert list(np.diff(start)) == [len(l) for l, _ in lists] and 0 in np.diff(start)[1:-1]
        for b in range(B):
            assert np.array_equal(slots[start[b]:start[b + 1]], lists[b][0]) and np.array_equal(seen[start[b]:start[b + 1]], lists[b][1])
        L = lib.L
        wide = (np.cumsum([0] + [len(l) + 5 for l, _ in lists]) + 3).astype(np.int32)
        s2 = np.full(wide[-1], -7, np.int32); f2 = np.full(wide[-1], 9, np.uint8)
        lib.check(L.orbm_map_sets_fetch(W.ex._h, mp._m, SHIFT, B, wide.ctypes.data, s2.ctypes.data, None))
        lib.check(L.orbm_map_sets_fetch(W.ex._h, mp._m, SHIFT, B, wide.ctypes.data, None, f2.ctypes.data))
        lib.check(L.orbm_map_sets_fetch(W.ex._h, mp._m, SHIFT, B, wide.ctypes.data, None, None))
        for b in range(B):
            m = len(lists[b][0])
            assert np.array_equal(s2[wide[b]:wide[b] + m], lists[b][0]) and (s2[wide[b] + m:wide[b + 1]] == -7).all()
            assert np.array_equal(f2[wide[b]:wide[b] + m], lists[b][1]) and (f2[wide[b] + m:wide[b + 1]] == 9).all()
        assert (s2[:3] == -7).all()
        short = start.copy(); short[3:] -= 1                         # set SHIFT + 2 gets one entry too few
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, SHIFT, B, short.ctypes.data, slots.ctypes.data, None) == E_ARG and b"set %d" % (SHIFT + 2) in L.orbx_last_error()
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, SEL, B + 1, wide.ctypes.data, None, None) == E_ARG and b"set %d" % (SEL + B) in L.orbx_last_error()     # never built
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, SEL, B + 2, wide.ctypes.data, None, None) == E_ARG                       # beyond the map
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, -1, 1, wide.ctypes.data, None, None) == E_ARG
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, 0, 1, None, None, None) == E_ARG
        assert L.orbm_map_sets_fetch(W.ex._h, None, 0, 1, wide.ctypes.data, None, None) == E_ARG
        assert L.orbm_map_sets_fetch(W.ex._h, mp._m, 0, 0, None, None, None) == 0
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_set0_selected_sets_and_sets_fetch_emulated(emu_lib):
    _set0_select_and_sets_fetch(emu_lib)


@needs_reference
@pytest.mark.gpu
def test_set0_selected_sets_and_sets_fetch_gpu(hip_lib):
    _set0_select_and_sets_fetch(hip_lib)


# ---- 6. pool overflow ------------------------------------------------------------------------------------------------------------------------------

def _pool_overflow(lib):
    """windows so wide that the candidate pool of a fresh handle overflows: one ORBX_E_CAPACITY from fetch_slots, nothing written, nothing left to
    fetch; the re-enqueued batch equals the host-fed call (which has overflowed and been enqueued again by then, too)"""
    W = World(lib, EMU_SHAPE)
    mp = None
    try:
        Y = _stream_layout(W.maps, SEED)
        mp = _stream_store(W.ex, Y)
        mp.local_points(Y["frames"], Y["seen"])
        lists = [mp.fetch(b) for b in range(W.B)]
        L = lib.L
        lp = _map_batch(W, mp)
        lp.enqueue(0, use_u_right=False, th=30.0)
        lp.assigned[:] = -77; lp.nm[:] = -77
        fetch = lambda: L.orbm_search_local_points_fetch_slots(W.ex._h, lp.assigned.ctypes.data, lp.cap, lp.nm.ctypes.data, None)
        assert fetch() == E_CAPACITY
        assert (lp.assigned == -77).all() and (lp.nm == -77).all(), "the refused fetch wrote into the caller's buffers"
        assert fetch() == E_ARG and (lp.assigned == -77).all(), "the overflowed batch can be fetched again: its entries were never written"
        lp.enqueue(0, use_u_right=False, th=30.0)
        assert fetch() == 0
        host = W.batch([mp.set(b) for b in range(W.B)])
        host.enqueue(0, is_bad=[sn for _, sn in lists], has_obs=None, use_u_right=False, th=30.0)
        a0, n0, _ = host.fetch()
        assert np.array_equal(lp.nm, n0) and n0[0] > 50
        for b in range(W.B):
            assert np.array_equal(lp.assigned[b], to_slot(a0[b], lists[b][0])), "frame %d" % b
    finally:
        if mp is not None:
            mp.close()
        W.close()


@needs_reference
def test_pool_overflow_emulated(emu_lib):
    _pool_overflow(emu_lib)


@needs_reference
@pytest.mark.gpu
def test_pool_overflow_gpu(hip_lib):
    _pool_overflow(hip_lib)


# ---- 7. refusals, handle states, resources -----------------------------------------------------------------------------------------------------------

NEW_CALLS = ("orbm_search_local_points_batch_map", "orbm_search_local_points_rig_batch_map", "orbm_search_local_points_fetch_slots",
             "orbm_search_rig_batch_fetch_slots", "orbm_map_sets_fetch",
             # (the row-fed key-frame searches of tests/test_map_rows_resident.py: the same three handle states)
             "orbm_search_for_triangulation_resident_map", "orbm_search_for_triangulation_resident_kb8_map", "orbm_search_by_bow_resident_map",
             "orbm_search_by_bow_rig_batch_map")


def test_new_calls_take_the_extractor_first():
    """tests/null_argument_runner.py hands a live extractor to the first pointer of every orbm_ symbol: the new calls take one there"""
    import os
    import re
    hdr = open(os.path.join(ol.ROOT, "include", "orbx.h")).read()
    for name in NEW_CALLS:
        first = re.findall(r"\b%s\s*\(\s*([^,]*)," % name, hdr)
        assert len(first) == 1 and first[0].split() == ["orbx_extractor*", "L" if "rig" in name else "h"], (name, first)


def _null_calls(lib, handle, fill):
    """the new entry points with null pointers and `fill` for every integer, as tests/null_argument_runner.py calls the others: refuse, do not dereference"""
    for name in NEW_CALLS:
        f = getattr(lib.L, name)
        args, first = [], True
        for t in f.argtypes:
            if t is C.c_float: args.append(0.0)
            elif t is C.c_int: args.append(fill)
            elif first and handle is not None: args.append(handle); first = False
            else: args.append(None)
        assert f(*args) < 0, name


def _refusals(lib, two_devices):
    L = lib.L
    live0 = _live(lib)
    _null_calls(lib, None, 0)
    w, h, nf, B = 320, 240, 300, 2
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    _null_calls(lib, ex._h, 0)                                                       # a live handle that has not extracted anything
    ex.extract_batch(np.stack([synth.corner_field(w, h, seed=40 + b, nrect=700) for b in range(B)]))
    _null_calls(lib, ex._h, 1)                                                       # after an extraction
    cap = ex.max_keypoints(); sfs = ex.GetScaleFactors(); bounds = (0.0, float(w), 0.0, float(h))
    rng = np.random.default_rng(5)
    pos = rng.uniform(-2, 2, (50, 3)).astype(np.float32); pos[:, 2] += 4
    dist = np.linalg.norm(pos, axis=1).astype(np.float32)
    fields = (pos, (pos / dist[:, None]).astype(np.float32), dist / 3, dist * 2, rng.integers(0, 256, (50, 32), dtype=np.uint8))
    SETS = 4
    mp = M.ResidentMap(ex, 60, 1, 8, SETS)
    mp.update(np.arange(50, dtype=np.int32), *fields)
    mp.select(0, np.arange(50)); mp.select(1, np.arange(49, 9, -1)); mp.select(2, [])           # set 3 is never built
    rp = M.ResidentPoints(ex, *fields)
    fv = (M._FrustumView * B)()
    for b in range(B):
        M.frustum_view(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), CAM, bounds, 0.0, sfs, into=fv[b])
    a = np.zeros((B, 2 * cap), np.int32); nm = np.zeros(B, np.int32)
    slots = lambda: L.orbm_search_local_points_fetch_slots(ex._h, a.ctypes.data, 2 * cap, nm.ctypes.data, None)
    plain = lambda: L.orbm_search_local_points_fetch(ex._h, a.ctypes.data, 2 * cap, nm.ctypes.data, None)
    enqueue = lambda m=mp._m, set0=0, first=0, n=B, frames=fv, hh=ex._h: L.orbm_search_local_points_batch_map(hh, first, n, frames, m, set0, None, 0, 0.5, 1.0, 0, 0.0, 0.8, 0)
    err = lambda: L.orbx_last_error()
    assert slots() == E_ARG                                                          # nothing yet
    assert enqueue() == 0 and slots() == 0 and nm.sum() >= 0
    assert enqueue() == 0 and plain() == 0 and slots() == 0                          # both fetches serve a map batch
    for refused, code, names in ((lambda: enqueue(m=None), E_ARG, b"map"), (lambda: enqueue(set0=-1), E_ARG, b"set0"), (lambda: enqueue(set0=SETS - 1), E_CAPACITY, b"sets ["),
                                 (lambda: enqueue(set0=SETS), E_CAPACITY, b"sets ["), (lambda: enqueue(first=1), E_ARG, b""), (lambda: enqueue(n=0), E_ARG, b""),
                                 (lambda: enqueue(n=-1), E_ARG, b""), (lambda: enqueue(frames=None), E_ARG, b"")):
        assert enqueue() == 0                                                        # a pending batch, which the refused call ends
        assert refused() == code and names in err(), err()
        assert slots() == E_ARG and plain() == E_ARG, "a refused enqueue leaves nothing to fetch"
    assert enqueue(hh=None) == E_ARG                                                 # (no handle: nobody's batch to end)
    fv[1].nlevels = 0                                                                # what the .._batch_maps calls refuse: the message names the frame
    assert enqueue() == E_ARG and b"frame 1" in err() and slots() == E_ARG
    fv[1].nlevels = len(sfs)
    assert enqueue(set0=2) == 0 and slots() == 0 and (nm == 0).all() and (a[:, :cap] == -1).all()     # an empty set and one that was never built
    # fetch_slots on a batch that was not enqueued on a map's sets: refused, and the batch stays
    table = (M._FrameMap * B)()
    table[0].points = rp._p; table[1].points = rp._p
    assert L.orbm_search_local_points_batch_maps(ex._h, 0, B, fv, table, None, 0, 0.5, 1.0, 0, 0.0, 0.8, 0) == 0
    assert slots() == E_ARG and b"map" in err() and plain() == 0
    assert L.orbm_search_local_points_batch(ex._h, 0, B, fv, rp._p, None, None, None, 0, 0.5, 1.0, 0, 0.0, 0.8, 0) == 0
    assert slots() == E_ARG and plain() == 0
    # the rig fetch refuses a one-camera map batch and leaves it pending; short rows; in_view that was not requested
    assert enqueue() == 0
    assert L.orbm_search_rig_batch_fetch_slots(ex._h, a.ctypes.data, 2 * cap, nm.ctypes.data, None, None) == E_ARG
    assert L.orbm_search_local_points_fetch_slots(ex._h, a.ctypes.data, cap - 1, nm.ctypes.data, None) == E_CAPACITY
    iv = np.zeros((B, 50), np.uint8)
    assert L.orbm_search_local_points_fetch_slots(ex._h, a.ctypes.data, 2 * cap, nm.ctypes.data, iv.ctypes.data) == E_ARG
    assert slots() == 0
    # the rig enqueue: its own refusals come before anything is enqueued
    rv = (M._FrustumRigView * B)()
    rig = lambda m=mp._m, set0=0, right=ex._h: L.orbm_search_local_points_rig_batch_map(ex._h, 0, right, 1, 1, rv, m, set0, None, 0.5, 1.0, 0, 0.0, 0.8, 0)
    for refused, code in ((lambda: rig(m=None), E_ARG), (lambda: rig(set0=-1), E_ARG), (lambda: rig(set0=SETS), E_CAPACITY), (lambda: rig(right=None), E_ARG),
                          (lambda: rig(), E_ARG)):                                   # (the last: no orbm_stereo_fisheye has linked the frames)
        assert enqueue() == 0
        assert refused() == code and slots() == E_ARG
        assert L.orbm_search_rig_batch_fetch_slots(ex._h, a.ctypes.data, 2 * cap, nm.ctypes.data, None, None) == E_ARG
    other = mp2 = None
    if two_devices:
        other = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib, device_id=1)
        mp2 = M.ResidentMap(other, 60, 1, 8, SETS)
        assert enqueue() == 0
        assert enqueue(m=mp2._m) == E_ARG and b"device" in err() and slots() == E_ARG
        assert rig(m=mp2._m) == E_ARG
        one = np.zeros(2, np.int32)
        assert L.orbm_map_sets_fetch(ex._h, mp2._m, 0, 1, one.ctypes.data, None, None) == E_ARG
    assert enqueue() == 0 and slots() == 0
    for o in (mp2, other, mp, rp, ex):
        if o is not None:
            o.close()
    assert _live(lib) == live0


def test_refusals_and_resources_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("ORBX_EMU_DEVICES", "2")
    assert emu_lib.L.orbx_device_count() == 2
    _refusals(emu_lib, True)


@pytest.mark.gpu
def test_refusals_and_resources_gpu(hip_lib):
    _refusals(hip_lib, False)
