"""A point set of orbm_map_select that holds one slot at several positions, through the Fuse and the Sim3 projection batches on the resident map
(k_map_set_table, k_map_skip_listed, k_map_skip_dups), and the table's epoch at the line (map_skip_table).  Survivors of the mutation pass recorded in
profiles/emu_mutants_map/README.md: the sets of tests/test_fuse_map.py and tests/test_sim3_map.py repeat slots, but never the slot of POSITION 0 - the one
position whose offer to the table equals `top` -, never with more than kSkipTargets = 16 targets, and their short epochs never end exactly at the limit.

Expected values as in those two files: the oracle's rows pair by pair (tests/test_fuse_batch.py / tests/test_sim3_projection_batch.py) masked with the
numpy restatement of the exclusion rule (test_fuse_map.skip_rule) on a host mirror of rows, found lists, slot states and the set's slot list."""
import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import matcher as M
import test_fuse_map as FM
import test_sim3_map as SM
from test_fuse_map import BAD, skip_rule

i32, u8 = np.int32, np.uint8
SPARE = FM.SPARE_ROW
# targets 0 .. 8 as tests/test_fuse_map.py names them, then nine more on the largest key frame: odd ones read its own row, even ones a copy of that row
# which ALSO lists the two repeated slots.  Targets 16 and 17 are the second group of kSkipTargets = 16: one of each kind
TARGETS = FM.TARGETS + (4,) * 9
ROWS = FM.ROWS + tuple(SPARE if j % 2 == 0 else 4 for j in range(9))
FEAT0 = FM.FEAT0 + (0,) * 9


def _fuse_layout(S, W, ei):
    """(idx, rows, p0, p1, pb): the set's points in order - p0 at positions 0 and 203, p1 at 102 and 276 (behind the first workgroup of 256), the bad point
    pb at 1 and 275, every other point once - and the map's rows with SPARE_ROW = row 4 whose first and last entries name p0 and p1"""
    state, row4 = W.state, W.rows[4]
    good = (state[W.set_slots] & BAD) == 0
    free = good & (ei[4] >= 0) & ~np.isin(W.set_slots, row4)             # matched by key frame 4, not in its row: target (4, row 4) keeps the pair
    cand = np.flatnonzero(free)
    assert len(cand) >= 2, "the scene holds %d points that key frame 4 matches and its row does not list" % len(cand)
    p0, p1 = int(cand[0]), int(cand[-1])
    pb = int(np.flatnonzero(~good & (ei[4] >= 0))[0])                   # bad by the time of the call, and a match otherwise
    rest = np.setdiff1d(np.arange(S.M), [p0, p1, pb])
    idx = np.concatenate([[p0, pb], rest[:100], [p1], rest[100:200], [p0], rest[200:271], [pb, p1], rest[271:]]).astype(np.int64)
    spare = row4.copy(); spare[0] = W.set_slots[p0]; spare[-1] = W.set_slots[p1]
    rows = list(W.rows) + [spare]
    assert idx[0] == p0 == idx[203] and idx[102] == p1 == idx[276] and idx[1] == pb == idx[275] and len(idx) == S.M + 3 > 256
    return idx, rows, p0, p1, pb


def _fuse(lib):
    S, W = FM.scene(), FM.world()
    D = FM.Device(lib, S, W)
    try:
        th, chi2 = 3.0, True
        ei = S.expect(D.ex, th, chi2)[0]
        idx, rows, p0, p1, pb = _fuse_layout(S, W, ei)
        D.mp.set_keyframe(SPARE, rows[SPARE])
        D.mp.select(2, W.set_slots[idx])
        want = FM.expected(S, D.ex, W.state, W.set_slots[idx], idx, rows, th, chi2, TARGETS, ROWS, FEAT0)
        bi, sk = want[0], want[3]
        # what the layout is for, on the oracle and the restated rule alone
        listed = [k for k in range(len(TARGETS)) if ROWS[k] == SPARE]
        unlisted = [k for k in range(9, len(TARGETS)) if ROWS[k] == 4]
        assert 17 in listed and 16 in unlisted and 9 in listed and 10 in unlisted
        for pos in (0, 203, 102, 276):
            assert sk[listed, pos].all() and not sk[unlisted, pos].any() and (bi[unlisted, pos] >= 0).all() and (bi[listed, pos] == -1).all(), pos
        assert sk[:, 1].all() and sk[:, 275].all() and (bi[:, [1, 275]] == -1).all()                  # the bad point, at its first and at its later position
        assert (bi >= 0).sum() >= 100 and sk.any(axis=1).all()
        for n in range(2):                                                # (twice: the second call finds the first one's offers in the table)
            got = D.fuse(S, th, chi2, set=2, targets=TARGETS, rows=ROWS, feat0=FEAT0)
            assert got[0].shape == (len(TARGETS), len(idx))
            FM._same(got, want[:3], "18 targets on a set with repeated slots, call %d" % n)
        # the same set without chi2 gate and at another radius
        FM._same(D.fuse(S, 6.0, False, set=2, targets=TARGETS, rows=ROWS, feat0=FEAT0),
                 FM.expected(S, D.ex, W.state, W.set_slots[idx], idx, rows, 6.0, False, TARGETS, ROWS, FEAT0)[:3], "th 6, no chi2 gate")
    finally:
        D.close()


def test_fuse_repeated_slot_at_position_0_and_18_targets_emulated(emu_lib):
    _fuse(emu_lib)


@pytest.mark.gpu
def test_fuse_repeated_slot_at_position_0_and_18_targets_gpu(hip_lib):
    _fuse(hip_lib)


def _sim3(lib):
    S, W = SM.scene(), SM.world()
    D = SM.Device(lib, S, W)
    try:
        th, ratio = 5.0, 1.0
        plain = S.expect(D.ex, th, ratio)[0]                             # the oracle without exclusions: the point every keypoint takes
        good = (W.state[W.set_slots] & BAD) == 0
        times = np.array([sum(int((plain[k] == p).any()) for k in range(S.K)) for p in range(S.M)])
        cand = np.flatnonzero(good & (times >= 2))
        assert len(cand) >= 2, "points that at least two targets match"
        p0, p1 = int(cand[0]), int(cand[-1])
        pb = int(np.flatnonzero(~good & (times >= 1))[0])
        rest = np.setdiff1d(np.arange(S.M), [p0, p1, pb])
        idx = np.concatenate([[p0, pb], rest[:100], [p1], rest[100:200], [p0], rest[200:271], [pb, p1], rest[271:]]).astype(np.int64)
        slots = W.set_slots[idx]
        takers = [[k for k in range(S.K) if (plain[k] == p).any()] for p in (p0, p1)]
        # found list of target k: the world's, without the two slots - and with p0's slot in the first target that matches p0, p1's in the LAST that matches p1
        lists = []
        for k in range(S.K):
            l = W.found[k][~np.isin(W.found[k], W.set_slots[[p0, p1]])]
            extra = [W.set_slots[p0]] * (k == takers[0][0]) + [W.set_slots[p1]] * (k == takers[1][-1])
            lists.append(np.concatenate([l, np.array(extra, i32)]).astype(i32))
        sk = skip_rule(W.state, slots, lists)
        for p, pos, k_in, k_out in ((p0, (0, 203), takers[0][0], takers[0][-1]), (p1, (102, 276), takers[1][-1], takers[1][0])):
            assert k_in != k_out and sk[k_in, list(pos)].all() and not sk[k_out, list(pos)].any()
        assert sk[:, [1, 275]].all()
        S2 = SM.subscene(S, idx, sk)
        want = SM.expected(S2, D.ex, slots, th, ratio, False)
        # the pair is matched where it is not listed (by its first position: the sequential accept), and not where it is
        for p, pos, k_in, k_out in ((p0, (0, 203), takers[0][0], takers[0][-1]), (p1, (102, 276), takers[1][-1], takers[1][0])):
            assert (want[0][k_out] == pos[0]).any() and not np.isin(want[0][k_in], pos).any()
        D.mp.select(2, slots)
        for n in range(2):
            SM._same(D.search(S, th, ratio, False, lists, set=2), want, "a set with repeated slots, call %d" % n)
        SM._same(D.search(S, 8.0, 1.5, True, lists, set=2), SM.expected(S2, D.ex, slots, 8.0, 1.5, True), "th 8, ratio 1.5, occupied")
    finally:
        D.close()


def test_sim3_repeated_slot_at_position_0_emulated(emu_lib):
    _sim3(emu_lib)


@pytest.mark.gpu
def test_sim3_repeated_slot_at_position_0_gpu(hip_lib):
    _sim3(hip_lib)


# ---- the table's epoch at the line -----------------------------------------------------------------------------------------------------------------
def _table_epoch(lib):
    """Two disjoint sets of 150 points alternate; a row full of set A's slots excludes most of A and nothing of B.  Every call moves `tbase` up by 150; with a
    limit of 450 the third call ends exactly at the limit and the fourth is the first that clears the table.  449 clears one call earlier, 451 one value later."""
    S, W = FM.scene(), FM.world()
    D = FM.Device(lib, S, W)
    try:
        rng = np.random.default_rng(5)
        ia, ib = np.arange(150), np.arange(150, S.M)
        A, B = W.set_slots[ia], W.set_slots[ib]
        rows = list(W.rows) + [rng.choice(A, FM.ROW_CAP).astype(i32)]
        D.mp.set_keyframe(SPARE, rows[SPARE])
        tg, rw, f0 = (4, 3, 4), (SPARE, 3, 4), (0, 0, 0)
        D.mp.select(2, A); D.mp.select(3, B)
        call = lambda s: D.fuse(S, 3.0, True, set=s, targets=tg, rows=rw, feat0=f0)
        want = {2: FM.expected(S, D.ex, W.state, A, ia, rows, 3.0, True, tg, rw, f0), 3: FM.expected(S, D.ex, W.state, B, ib, rows, 3.0, True, tg, rw, f0)}
        assert want[2][3][0].sum() > 100 and np.array_equal(want[3][3][0], (W.state[B] & BAD) != 0) and (want[3][0][0] >= 0).sum() >= 20
        call(2)                                                          # (the first call allocates the table; the limits below start from a cleared one)
        for limit in (450, 449, 451, 150):
            lib.check(lib.L.orbm_map_debug_epoch(D.ex._h, D.mp._m, limit))
            for n in range(8):
                s = 2 + n % 2
                FM._same(call(s), want[s][:3], "limit %d, call %d" % (limit, n + 1))
    finally:
        D.close()


def test_table_epoch_at_the_limit_emulated(emu_lib):
    _table_epoch(emu_lib)


@pytest.mark.gpu
def test_table_epoch_at_the_limit_gpu(hip_lib):
    _table_epoch(hip_lib)
