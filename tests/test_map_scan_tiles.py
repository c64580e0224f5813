"""Tracking::UpdateLocalPoints on the resident map (orbm_map_local_points) where one frame's walk is longer than ONE TILE of k_map_scan - the scan of a
frame's chunk counts runs over 64 chunks of kMapChunk = 256 positions at a time and carries the sum of the earlier tiles -, and where the stamps' epoch
ends exactly at the limit.  Survivors of the mutation pass recorded in profiles/emu_mutants_map/README.md: no other test builds a local map of more than
64 chunks, so neither the carry between tiles nor the loop's second trip had ever run.

Expected: tests/test_local_map_build.py::_restate, the statements of src/Tracking.cc:4088-4120 and :3983-4003 on plain arrays.  Nothing is read from the
library under test; before it is called the restatement alone has to show that the world holds what it is built for (_tile_world)."""
import functools

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor
from orb_slam3_detailed_comments_amd import matcher as M
from test_local_map_build import _restate, _mixed_row

E_CAPACITY = -4
CHUNK, TILE = 256, 64                                   # kMapChunk; the chunks one trip of k_map_scan's loop covers
S_SLOTS, ROW_CAP = 12000, 512
# rows 0 .. 31: 512 entries (two chunks each); then a row of one chunk, one that ends inside a wave of its first chunk (100 = 64 + 36), one that ends
# inside a wave of its SECOND chunk (300 = 256 + 44), an empty one, one of 37
ROW_LEN = (512,) * 32 + (256, 100, 300, 0, 37)
R256, R100, R300, R0, R37 = 32, 33, 34, 35, 36
FRAMES = ([R100] + list(range(32)) + [R256, R300],      # 1 + 64 + 1 + 2 = 68 chunks, 17 040 positions: the tile edge lies inside the run of long rows
          [R300, R100, R0],                             # 3 chunks, behind frame 0's 68: frame_chunk0 is not 0 and not a multiple of the tile
          list(range(32)),                              # exactly 64 chunks: one full tile, no second trip
          list(range(31, -1, -1)) + [R37],              # 65 chunks: the second tile holds one chunk
          [])


def _chunk_of_positions(frame):
    """the chunk (counted inside the frame) of every position of the walk: a visited row of n entries is ceil(n / 256) chunks, the last one ragged"""
    out, c = [], 0
    for r in frame:
        n = ROW_LEN[r]
        out.append(c + np.arange(n) // CHUNK)
        c += -(-n // CHUNK)
    return np.concatenate(out + [np.zeros(0, np.int64)]), c


@functools.lru_cache(maxsize=None)
def _tile_world():
    rng = np.random.default_rng(64)
    S = S_SLOTS
    present = np.ones(S, bool); present[np.arange(S) % 17 == 5] = False
    bad = np.zeros(S, bool); bad[np.arange(S) % 11 == 3] = True; bad &= present
    good, bads, absent = np.flatnonzero(present & ~bad), np.flatnonzero(bad), np.flatnonzero(~present)
    rows = [_mixed_row(rng, n, good, bads, absent) if n >= 4 else np.zeros(0, np.int32) for n in ROW_LEN]
    seen = []
    for b, f in enumerate(FRAMES):
        ls, _ = _restate(f, rows, present, bad, None)
        seen.append(None if len(ls) == 0 else np.concatenate([rng.choice(ls, max(1, len(ls) // 3)), rng.choice(absent, 3), rng.choice(bads, 3)]).astype(np.int32))
    for a in [present, bad] + rows:
        a.setflags(write=False)
    return dict(present=present, bad=bad, rows=rows, seen=seen)


def _kept_per_chunk(W, frame):
    """from the restatement alone: how many positions of every chunk of the frame's walk keep their point"""
    walk = np.concatenate([W["rows"][r] for r in frame] + [np.zeros(0, np.int32)])
    chunk, nchunks = _chunk_of_positions(frame)
    ls, _ = _restate(frame, W["rows"], W["present"], W["bad"], None)
    first = {}
    for p, s in enumerate(walk.tolist()):
        if s >= 0 and s not in first:
            first[s] = p
    kept = np.zeros(nchunks, np.int64)
    for s in ls.tolist():
        kept[chunk[first[s]]] += 1
    assert kept.sum() == len(ls)
    return kept


def test_the_tile_world_holds_its_cases():
    """no library call: the chunk counts the issue of the pass asks for, on the restatement"""
    W = _tile_world()
    nch = [_chunk_of_positions(f)[1] for f in FRAMES]
    assert nch == [68, 3, 64, 65, 0] and sum(ROW_LEN[r] for r in FRAMES[0]) > TILE * CHUNK
    k0 = _kept_per_chunk(W, FRAMES[0])
    assert k0[0] > 0 and k0[63] > 0 and k0[64] > 0 and k0[-1] > 0, k0
    assert len(set(k0.tolist())) > 10 and k0[:TILE].sum() != k0.sum() and k0[63] != k0[64] and k0[64] != k0[-1]
    k3 = _kept_per_chunk(W, FRAMES[3])
    assert k3[64] > 0 and k3[:TILE].sum() > 0                  # the one chunk of the second tile keeps points, and needs the first tile's sum in front of it
    k1 = _kept_per_chunk(W, FRAMES[1])
    assert (k1 > 0).all() and ROW_LEN[R100] % 64 and (ROW_LEN[R300] - CHUNK) % 64
    for b, f in enumerate(FRAMES[:4]):
        sn = _restate(f, W["rows"], W["present"], W["bad"], W["seen"][b])[1]
        assert sn.any() and not sn.all()


def _build(lib):
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    W = _tile_world()
    mp = M.ResidentMap(ex, S_SLOTS, len(ROW_LEN), ROW_CAP, len(FRAMES))
    ids = np.flatnonzero(W["present"]).astype(np.int32)
    z3 = np.zeros((len(ids), 3), np.float32); o = np.ones(len(ids), np.float32)
    desc = (ids[:, None] * 7 + np.arange(32)[None, :]).astype(np.uint8)              # a descriptor that names its slot
    mp.update(ids, z3, z3, o, o, desc, W["bad"][ids])
    for r, row in enumerate(W["rows"]):
        mp.set_keyframe(r, row)
    return ex, mp, W


def _check(mp, ex, W, frames, seen, what):
    Ms = mp.local_points(frames, seen)
    for b, f in enumerate(frames):
        ls, sn = _restate(f, W["rows"], W["present"], W["bad"], None if seen is None else seen[b])
        got_s, got_n = mp.fetch(b)
        assert Ms[b] == len(ls), "%s, frame %d: M_out = %d, the reference lists %d points" % (what, b, Ms[b], len(ls))
        assert np.array_equal(got_s, ls), "%s, frame %d: the list differs first at %s" % (what, b, np.flatnonzero(got_s != ls)[:3])
        assert np.array_equal(got_n, sn), "%s, frame %d: seen bytes" % (what, b)
    return Ms


def _tiles(lib):
    ex, mp, W = _build(lib)
    try:
        _check(mp, ex, W, list(FRAMES), W["seen"], "five frames")
        ls = _restate(FRAMES[0], W["rows"], W["present"], W["bad"], None)[0]
        want = (ls[:, None] * 7 + np.arange(32)[None, :]).astype(np.uint8)
        assert M.PointsFetch(ex, mp.set(0))[4].tobytes() == want.tobytes(), "the gathered descriptors of the longest list"
        # the frames in another order: other chunk numbers in front of every frame, and the long frame last
        order = [1, 3, 4, 2, 0]
        _check(mp, ex, W, [FRAMES[b] for b in order], [W["seen"][b] for b in order], "reordered")
        _check(mp, ex, W, [FRAMES[0]], None, "the long frame alone, nothing seen")
    finally:
        mp.close(); ex.close()


def test_tiles_emulated(emu_lib):
    _tiles(emu_lib)


@pytest.mark.gpu
def test_tiles_gpu(hip_lib):
    _tiles(hip_lib)


# ---- the stamps' epoch at the line -----------------------------------------------------------------------------------------------------------------
# A build whose longest walk is L moves `base` up by L; a build that would move it past the limit clears the stamps and starts over.  Two frame sets of the
# same L = 656 alternate, so a stamp that survives a clear, or a clear that does not happen, shows as a point missing from the other set's list.
EPOCH_A = ([R300, R256, R100], [R37, R100], [R100, R100])
EPOCH_B = ([R100, R256, R300], [R100, R37, R300], [R256])
EPOCH_L = 656


def _epochs(lib):
    ex, mp, W = _build(lib)
    L = lib.L
    try:
        assert max(sum(ROW_LEN[r] for r in f) for f in EPOCH_A) == EPOCH_L == max(sum(ROW_LEN[r] for r in f) for f in EPOCH_B)
        a_lists = [_restate(f, W["rows"], W["present"], W["bad"], None)[0] for f in EPOCH_A]
        b_lists = [_restate(f, W["rows"], W["present"], W["bad"], None)[0] for f in EPOCH_B]
        assert all(not np.array_equal(a, b) for a, b in zip(a_lists, b_lists)), "the two frame sets list other points in every set"
        seen_a = [W["seen"][1], None, W["seen"][1][:5]]
        # limit = 3 L: builds 1 .. 3 end at base = L, 2 L and 3 L = the limit itself (no clear), build 4 is the first that clears, 5 and 6 follow it, 7 clears
        # again.  limit = 3 L - 1 clears one build earlier, 3 L + 1 leaves one stamp value unused: the lists are the restatement's under all three
        for limit in (3 * EPOCH_L, 3 * EPOCH_L - 1, 3 * EPOCH_L + 1):
            lib.check(L.orbm_map_debug_epoch(ex._h, mp._m, limit))
            for k in range(8):
                fr, sn = ((EPOCH_A, seen_a), (EPOCH_B, None))[k % 2]
                _check(mp, ex, W, list(fr), sn, "limit %d, build %d" % (limit, k + 1))
        # a walk of exactly the limit fits an epoch (every build clears); one position more is refused, and nothing is written
        lib.check(L.orbm_map_debug_epoch(ex._h, mp._m, EPOCH_L))
        for k in range(3):
            _check(mp, ex, W, list((EPOCH_A, EPOCH_B)[k % 2]), None, "limit = L, build %d" % (k + 1))
        before = [mp.fetch(b) for b in range(3)]
        lib.check(L.orbm_map_debug_epoch(ex._h, mp._m, EPOCH_L - 1))
        with pytest.raises(M.OrbxError) as e:
            mp.local_points(list(EPOCH_A))
        assert e.value.code == E_CAPACITY and "frame 0" in str(e.value)
        for b in range(3):
            assert all(np.array_equal(x, y) for x, y in zip(before[b], mp.fetch(b))), "a refused build changed set %d" % b
        _check(mp, ex, W, [EPOCH_A[1], EPOCH_A[2]], None, "walks below the limit after the refusal")       # 137 and 200 positions
    finally:
        mp.close(); ex.close()


def test_epoch_at_the_limit_emulated(emu_lib):
    _epochs(emu_lib)


@pytest.mark.gpu
def test_epoch_at_the_limit_gpu(hip_lib):
    _epochs(hip_lib)
