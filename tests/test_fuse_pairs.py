"""orbm_fuse_pairs_batch and orbm_fuse_pairs_batch_map: the Fuse batches answered with the matched pairs alone - the pairs (k, i) with best_idx[k][i] >= 0,
ordered by target and then by position, target k's at [start[k], start[k + 1]) - compacted on the device behind the dense search (k_fuse_pairs: ballots per
chunk of 256 positions; k_fuse_pair_scan_tiles: one wave per 64 chunks; k_fuse_pair_scan_sums: one workgroup over the tiles; k_fuse_pairs again to scatter).

Expected values never come from the new calls or from the dense ones: they are the oracle rows of tests/test_fuse_batch.py::scene().expect(ex, th, chi2), for
the map form through tests/test_fuse_map.py::expected(..) (the numpy restatement of the exclusion and kf_slot rules on the host mirror), compacted with
numpy in row-major order (compact()).

The world is test_fuse_map's.  In set order the points 256-299 match almost nothing, so the set is the 300 points PERMUTED (PERM): every target with keypoints
then has pairs in both chunks.  Larger sets tile the permutation (orbm_map_select and orbm_points_create allow duplicates).  One wave of the scan handles 64
chunks and a target of the 16 800-position set has 66, so that set crosses a tile inside a target; the workgroup that scans the tile sums gives each of its
256 threads a run of ceil(tiles / 256) tiles, and 16 500 targets x 1 or 2 positions (16 500 chunks, 258 tiles) make that run 2."""
import ctypes as C

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor, views
from orb_slam3_detailed_comments_amd import matcher as M
import test_fuse_map as fm
from test_fuse_batch import NLEVELS, THS, _live, scene
from test_fuse_map import FEAT0, KF_ROWS, MAX_SETS, ROWS, TARGETS, UNSET_ROW, Device, expected, world

f32, i32, u8 = np.float32, np.int32, np.uint8
E_ARG, E_CAPACITY = -2, -4
PERM = np.random.default_rng(11).permutation(300)
PERM.setflags(write=False)
SET = 2                                               # the set the cases select into (test_fuse_map's PSET keeps the points in set order)
CHUNK = 256
MANY = tuple((1, 2, 0)[k % 3] for k in range(130))    # 130 targets: more than two waves hold, every third one without keypoints
NAMES = ("start", "point", "feat", "dist", "point_slot", "kf_slot")
SENTINEL = -7


def compact(bi, bd, ks=None, slots=None):
    """the pairs of dense [K][M] results in row-major order, as (start, point, feat, dist[, point_slot, kf_slot])"""
    keep = bi >= 0
    k, i = np.nonzero(keep)                                          # (row-major: by k, then by i)
    start = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(i32)
    out = (start, i.astype(i32), bi[k, i].astype(i32), bd[k, i].astype(i32))
    return out if ks is None else out + (np.asarray(slots, i32)[i], ks[k, i].astype(i32))


def _same(got, want, what):
    assert len(got) == len(want), what
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, "%s: %s has %s entries, expected %s" % (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s: %s differs in %d of %d entries, first at %d: %d, expected %d" % (what, name, len(bad), g.size, bad[0], g[bad[0]], w[bad[0]])


def _chunks(bi):
    """pairs per (target, chunk of 256 positions)"""
    n = (bi.shape[1] + CHUNK - 1) // CHUNK
    return np.array([[(bi[k, c * CHUNK:(c + 1) * CHUNK] >= 0).sum() for c in range(n)] for k in range(bi.shape[0])]).reshape(bi.shape[0], n)


def map_want(S, ex, idx, th, chi2, targets=TARGETS, rows=ROWS, feat0=FEAT0):
    W = world()
    bi, bd, ks, _ = expected(S, ex, W.state, W.set_slots[idx], idx, W.rows, th, chi2, targets, rows, feat0)
    return compact(bi, bd, ks, W.set_slots[idx])


def map_pairs(D, S, th, chi2, targets=TARGETS, rows=ROWS, feat0=FEAT0, cap=None, set=SET):
    kfs, specs = D.targets(targets)
    return M.ORBmatcher.FuseCandidatesPairsBatchMap(D.ex, kfs, specs, D.mp, set, rows, th, S.inv_sigma2 if chi2 else None, feat0=feat0, cap=cap)


def table(kf_list, spec_list, s2):
    T = (views.FuseTarget * max(len(kf_list), 1))()
    for k, (kf, sp) in enumerate(zip(kf_list, spec_list)):
        T[k].kf = kf._kf if kf is not None else None; T[k].spec = sp[0]; T[k].log_scale_factor = sp[1]; T[k].inv_level_sigma2 = None if s2 is None else s2.ctypes.data
    return T


class Raw:
    """the C calls on arrays full of SENTINEL, any output left out: what a call writes and what it leaves alone"""

    def __init__(self, n):
        self.a = {name: np.full(max(n, 1), SENTINEL, i32) for name in NAMES[1:]}

    def ptrs(self, without=()):
        return [None if name in without else self.a[name].ctypes.data for name in NAMES[1:]]

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.a.values())


# ---- what the cases are built for, counted on the oracle's rows and numpy alone ----
def _conditions(lib):
    S, W = scene(), world()
    ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib)
    # (set, th, chi-square) -> pairs, chunks per target, fewest pairs in a chunk of targets 1 - 8
    for reps, chunks, fewest, counts in ((1, 2, 1, (282, 300)), (3, 4, 4, (846, 900)), (56, 66, 5, (15792, 16800))):
        idx = np.tile(PERM, reps)
        for (th, chi2), pairs in zip(((3.0, True), (6.0, False)), counts):
            bi, bd, ks, _ = expected(S, ex, W.state, W.set_slots[idx], idx, W.rows, th, chi2)
            per = _chunks(bi)
            assert (bi >= 0).sum() == pairs >= 250 and per.shape[1] == chunks and per[1:].min() == fewest, (reps, th, int((bi >= 0).sum()), per.shape, int(per[1:].min()))
            assert per[0].sum() == 0 and ((per[1:] > 0).sum(1) >= 2).all(), "every target with keypoints has pairs in at least two chunks"
            left = ks[bi >= 0]
            assert (left >= 0).any() and (left == -1).any() and (left == -2).any()
    assert 66 > 64, "a target of the largest set spans more chunks than one wave of k_fuse_pair_scan_tiles scans"
    idx = np.arange(S.M)
    bi, bd, ks, _ = expected(S, ex, W.state, W.set_slots, idx, W.rows, 3.0, True)
    left = ks[bi >= 0]
    assert ((left >= 0).sum(), (left == -1).sum(), (left == -2).sum()) == (115, 123, 44)
    # 130 targets x 65 points: an empty span between two that are not, again and again
    idx = PERM[:65]
    for th, chi2 in ((3.0, True), (6.0, False)):
        bi = expected(S, ex, W.state, W.set_slots[idx], idx, W.rows, th, chi2, MANY, MANY, (0,) * len(MANY))[0]
        n = (bi >= 0).sum(1)
        assert n.sum() == 872 and (n[2::3] == 0).all() and (n[0::3] > 0).all() and (n[1::3] > 0).all(), (int(n.sum()), n[:6])
    # key frame 4 alone: enough matched points to fill a chunk with pairs only
    ei = S.expect(ex, 3.0, True)[0]
    assert (ei[4] >= 0).sum() == 70
    ex.close()


def test_conditions_hold_on_the_oracle_emulated(emu_lib):
    _conditions(emu_lib)


@pytest.mark.gpu
def test_conditions_hold_on_the_oracle_gpu(hip_lib):
    _conditions(hip_lib)


# ---- 1: the map form equals the compacted oracle rows; every optional output may be left out ----
def _parity_map(lib):
    S, W = scene(), world()
    D = Device(lib, S, W)
    D.mp.select(SET, W.set_slots[PERM])
    for chi2 in (True, False):
        for th in THS:
            _same(map_pairs(D, S, th, chi2), map_want(S, D.ex, PERM, th, chi2), "th %g chi2 %d" % (th, chi2))
    kfs, specs = D.targets()
    s2 = np.ascontiguousarray(S.inv_sigma2, f32)
    T = table(kfs, specs, s2)
    rows, feat0 = np.array(ROWS, i32), np.array(FEAT0, i32)
    want = dict(zip(NAMES, map_want(S, D.ex, PERM, 3.0, True)))
    n = int(want["start"][-1])
    for without in ((), ("dist",), ("point_slot",), ("kf_slot",), ("dist", "point_slot", "kf_slot"), ("dist", "kf_slot")):
        R = Raw(n); start = np.full(len(TARGETS) + 1, SENTINEL, i32)
        assert lib.L.orbm_fuse_pairs_batch_map(D.ex._h, len(TARGETS), T, rows.ctypes.data, feat0.ctypes.data, D.mp._m, SET, 3.0, 1, n, start.ctypes.data,
                                               *R.ptrs(without)) == 0, lib.L.orbx_last_error()
        assert np.array_equal(start, want["start"])
        for name in NAMES[1:]:
            assert (R.a[name] == SENTINEL).all() if name in without else np.array_equal(R.a[name], want[name]), (without, name)
    D.close()


def test_map_parity_emulated(emu_lib):
    _parity_map(emu_lib)


@pytest.mark.gpu
def test_map_parity_gpu(hip_lib):
    _parity_map(hip_lib)


# ---- 2: the host-fed form, without skip and with a third of the pairs skipped ----
def _points(ex, S, idx):
    return M.ResidentPoints(ex, S.pos[idx], S.normal[idx], S.mind[idx], S.maxd[idx], S.desc[idx])


def _parity_host(lib):
    S = scene()
    ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib)
    kfs, specs = S.resident(ex); rp = _points(ex, S, PERM)
    for chi2 in (True, False):
        for th in THS:
            ei, ed, _ = S.expect(ex, th, chi2)
            assert (ei >= 0).sum() >= 200
            got = M.ORBmatcher.FuseCandidatesPairsBatch(ex, kfs, specs, rp, th, S.inv_sigma2 if chi2 else None)
            _same(got, compact(ei[:, PERM], ed[:, PERM]), "no skip, th %g chi2 %d" % (th, chi2))
    skip = (np.random.default_rng(30).random((S.K, S.M)) < 0.3).astype(u8)
    for th, chi2 in ((3.0, True), (6.0, False)):
        ei, ed, _ = S.expect(ex, th, chi2)
        ei, ed = np.where(skip == 1, -1, ei[:, PERM]), np.where(skip == 1, -1, ed[:, PERM])
        assert (ei >= 0).sum() >= 100 and ((S.expect(ex, th, chi2)[0][:, PERM] >= 0) & (skip == 1)).sum() >= 40
        got = M.ORBmatcher.FuseCandidatesPairsBatch(ex, kfs, specs, rp, th, S.inv_sigma2 if chi2 else None, skip=skip)
        _same(got, compact(ei, ed), "30 %% skipped, th %g" % th)
    for o in kfs + [rp, ex]:
        o.close()


def test_host_fed_parity_emulated(emu_lib):
    _parity_host(emu_lib)


@pytest.mark.gpu
def test_host_fed_parity_gpu(hip_lib):
    _parity_host(hip_lib)


# ---- 3: set sizes around a wave, a chunk and a tile of the scan; duplicates ----
def _sets(lib):
    S, W = scene(), world()
    D = Device(lib, S, W)
    dup = np.concatenate([np.arange(100), np.arange(50, 150), [7, 7, 7], np.arange(299, 280, -1)])      # (test_fuse_map's duplicate list)
    for idx in [PERM[:n] for n in (0, 1, 63, 64, 65, 256, 257)] + [np.tile(PERM, 3), np.tile(PERM, 56), dup]:
        D.mp.select(SET, W.set_slots[idx])
        for th, chi2 in ((3.0, True), (6.0, False)):
            want = map_want(S, D.ex, idx, th, chi2)
            _same(map_pairs(D, S, th, chi2), want, "a set of %d points, th %g" % (len(idx), th))
            assert len(idx) < 63 or want[0][-1] >= 40
    D.close()


def test_set_sizes_and_duplicates_emulated(emu_lib):
    _sets(emu_lib)


@pytest.mark.gpu
def test_set_sizes_and_duplicates_gpu(hip_lib):
    _sets(hip_lib)


def _many_chunks(lib):
    """16 500 targets x 1 or 2 positions: more tiles than the workgroup of k_fuse_pair_scan_sums has threads, so every thread scans a run of two"""
    S = scene()
    ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib)
    ei, ed, _ = S.expect(ex, 3.0, True)
    p1, p2 = np.flatnonzero(ei[1] >= 0)[0], np.flatnonzero(ei[2] >= 0)[0]       # (a point matched in key frame 1, one matched in key frame 2)
    kfs, specs = S.resident(ex)
    order = [(1, 2, 0, 2)[k % 4] for k in range(16500)]
    assert (len(order) + 63) // 64 > 256
    for idx in (np.array([p1, p2]), np.array([p2])):
        rp = _points(ex, S, idx)
        got = M.ORBmatcher.FuseCandidatesPairsBatch(ex, [kfs[k] for k in order], [specs[k] for k in order], rp, 3.0, S.inv_sigma2, cap=len(order))
        want = compact(ei[order][:, idx], ed[order][:, idx])
        assert want[0][-1] >= 4000
        _same(got, want, "16 500 targets")
        rp.close()
    for o in kfs + [ex]:
        o.close()


def test_more_tiles_than_one_scan_pass_emulated(emu_lib):
    _many_chunks(emu_lib)


@pytest.mark.gpu
def test_more_tiles_than_one_scan_pass_gpu(hip_lib):
    _many_chunks(hip_lib)


# ---- 4: 130 targets, every third span empty ----
def _many_targets(lib):
    S, W = scene(), world()
    D = Device(lib, S, W)
    idx = PERM[:65]
    D.mp.select(SET, W.set_slots[idx])
    f0 = (0,) * len(MANY)
    for th, chi2 in ((3.0, True), (6.0, False)):
        want = map_want(S, D.ex, idx, th, chi2, MANY, MANY, f0)
        got = map_pairs(D, S, th, chi2, MANY, MANY, f0)
        _same(got, want, "130 targets, th %g" % th)
        n = np.diff(got[0])
        assert (n[2::3] == 0).all() and (n[0::3] > 0).all() and (n[1::3] > 0).all()
    D.close()


def test_130_targets_with_empty_spans_emulated(emu_lib):
    _many_targets(emu_lib)


@pytest.mark.gpu
def test_130_targets_with_empty_spans_gpu(hip_lib):
    _many_targets(hip_lib)


# ---- 5: a chunk in which every lane keeps its pair ----
def _full_chunk(lib):
    S = scene()
    ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib)
    ei, ed, _ = S.expect(ex, 3.0, True)
    matched = np.flatnonzero(ei[4] >= 0)
    idx = np.resize(matched, CHUNK)
    kfs, specs = S.resident(ex, [4]); rp = _points(ex, S, idx)
    got = M.ORBmatcher.FuseCandidatesPairsBatch(ex, kfs, specs, rp, 3.0, S.inv_sigma2)
    assert np.array_equal(got[0], [0, CHUNK]) and np.array_equal(got[1], np.arange(CHUNK))
    _same(got, compact(ei[4:5][:, idx], ed[4:5][:, idx]), "a full chunk")
    for o in kfs + [rp, ex]:
        o.close()


def test_a_chunk_of_pairs_only_emulated(emu_lib):
    _full_chunk(emu_lib)


@pytest.mark.gpu
def test_a_chunk_of_pairs_only_gpu(hip_lib):
    _full_chunk(hip_lib)


# ---- 6: capacity ----
def _capacity(lib):
    L = lib.L
    S, W = scene(), world()
    D = Device(lib, S, W)
    D.mp.select(SET, W.set_slots[PERM])
    kfs, specs = D.targets()
    s2 = np.ascontiguousarray(S.inv_sigma2, f32)
    T = table(kfs, specs, s2)
    K = len(TARGETS)
    rows, feat0 = np.array(ROWS, i32), np.array(FEAT0, i32)
    want = map_want(S, D.ex, PERM, 3.0, True)
    n = int(want[0][-1])
    hw = compact(*[a[list(TARGETS)][:, PERM] for a in S.expect(D.ex, 3.0, True)[:2]])
    pts = L.orbm_map_set(D.ex._h, D.mp._m, SET)

    def call_map(cap, R, start, k=K, T=T):
        return L.orbm_fuse_pairs_batch_map(D.ex._h, k, T, rows.ctypes.data, feat0.ctypes.data, D.mp._m, SET, 3.0, 1, cap, start.ctypes.data, *R.ptrs())

    def call_host(cap, R, start, k=K, T=T):
        return L.orbm_fuse_pairs_batch(D.ex._h, k, T, pts, None, 3.0, 1, cap, start.ctypes.data, *R.ptrs()[:3])
    for call, w in ((call_map, want), (call_host, hw)):
        n = int(w[0][-1])
        assert n >= 250
        for cap in (n, n + 1, K * len(PERM)):
            R = Raw(cap); start = np.full(K + 1, SENTINEL, i32)
            assert call(cap, R, start) == 0
            _same((start,) + tuple(R.a[name][:n] for name in NAMES[1:len(w)]), w, "cap %d" % cap)
            assert all((R.a[name][n:] == SENTINEL).all() for name in NAMES[1:]), "nothing is written behind the list"
        for cap in (n - 1, 1, 0):
            R = Raw(n); start = np.full(K + 1, SENTINEL, i32)
            assert call(cap, R, start) == E_CAPACITY and b"cap" in L.orbx_last_error()
            assert np.array_equal(start, w[0]) and R.untouched(), "cap %d: start is written, nothing else" % cap
        # no pairs: the target without keypoints; cap = 0 is enough, and point / feat may be null then
        start = np.full(2, SENTINEL, i32)
        R = Raw(0)
        assert call(0, R, start, k=1) == 0 and np.array_equal(start, [0, 0]) and R.untouched()
    start = np.full(2, SENTINEL, i32)
    assert L.orbm_fuse_pairs_batch_map(D.ex._h, 1, T, rows.ctypes.data, feat0.ctypes.data, D.mp._m, SET, 3.0, 1, 0, start.ctypes.data, None, None, None, None, None) == 0
    assert np.array_equal(start, [0, 0])
    # the wrappers: one more call with start[K] when the guess (or the caller's cap) was too small
    for cap in (None, 1, n, 0):
        _same(map_pairs(D, S, 3.0, True, cap=cap), want, "the wrapper with cap = %s" % cap)
    rp = _points(D.ex, S, PERM)
    k5, s5 = D.kfs5, D.specs5
    e5 = compact(*[a[:, PERM] for a in S.expect(D.ex, 3.0, True)[:2]])
    for cap in (None, 1):
        _same(M.ORBmatcher.FuseCandidatesPairsBatch(D.ex, k5, s5, rp, 3.0, S.inv_sigma2, cap=cap), e5, "the host-fed wrapper with cap = %s" % cap)
    rp.close()
    D.close()


def test_capacity_emulated(emu_lib):
    _capacity(emu_lib)


@pytest.mark.gpu
def test_capacity_gpu(hip_lib):
    _capacity(hip_lib)


# ---- 7: one handle: a large call, a small one, the large one again ----
def _reuse(lib):
    live0 = _live(lib)
    S, W = scene(), world()
    D = Device(lib, S, W)
    large, small = np.tile(PERM, 56), PERM[:65]
    D.mp.select(SET, W.set_slots[large]); D.mp.select(SET + 1, W.set_slots[small])
    want = {SET: map_want(S, D.ex, large, 3.0, True), SET + 1: map_want(S, D.ex, small, 3.0, True)}
    live = None
    for n, s in enumerate((SET, SET + 1, SET, SET + 1, SET)):
        _same(map_pairs(D, S, 3.0, True, set=s), want[s], "call %d, set %d" % (n, s))
        if n == 0:
            live = _live(lib)
        elif n > 2:
            assert _live(lib)[0] == live[0], "the handle's scratch has its size after the first large call"
    D.close()
    assert _live(lib) == live0, "device allocations, pinned allocations, streams, events: %s before, %s after" % (live0, _live(lib))


def test_scratch_growth_and_reuse_emulated(emu_lib):
    _reuse(emu_lib)


@pytest.mark.gpu
def test_scratch_growth_and_reuse_gpu(hip_lib):
    _reuse(hip_lib)


# ---- 8: refusals ----
def _rows_read_back(D, W):
    """the rows as an existing reader sees them (the local map built from one row: the first occurrence of every good point, in row order) equal the mirror"""
    for r in range(KF_ROWS - 2):
        good = W.rows[r][W.rows[r] >= 0]; good = good[W.state[good] == fm.PRESENT]
        first = good[np.sort(np.unique(good, return_index=True)[1])]
        assert np.array_equal(fm._row_points(D, r), first), "row %d" % r


def _refusals(lib, two_devices):
    L = lib.L
    S, W = scene(), world()
    live_start = _live(lib)
    D = Device(lib, S, W)
    ex, mp = D.ex, D.mp
    mp.select(SET, W.set_slots[PERM])
    K, Mp = len(TARGETS), len(PERM)
    kfs, specs = D.targets()
    s2 = np.ascontiguousarray(S.inv_sigma2, f32)
    T = table(kfs, specs, s2)
    rows = np.array(ROWS, i32); feat0 = np.array(FEAT0, i32)
    want = map_want(S, ex, PERM, 3.0, True)
    hw = compact(*[a[list(TARGETS)][:, PERM] for a in S.expect(ex, 3.0, True)[:2]])
    cap = K * Mp
    R = Raw(cap); start = np.full(K + 1, SENTINEL, i32)
    err = lambda: L.orbx_last_error() or b""
    ptr = lambda a: None if a is None else a.ctypes.data
    pts = L.orbm_map_set(ex._h, mp._m, SET)
    fetch_a, fetch_n = np.zeros(4096, i32), np.zeros(64, i32)

    def fmap(h=ex._h, n=K, T=T, rows=rows, feat0=feat0, m=mp._m, set=SET, chi2=1, cap=cap, start=start, without=()):
        return L.orbm_fuse_pairs_batch_map(h, n, T, ptr(rows), ptr(feat0), m, set, 3.0, chi2, cap, ptr(start), *R.ptrs(without))

    def fhost(h=ex._h, n=K, T=T, p=pts, chi2=1, cap=cap, start=start, without=()):
        return L.orbm_fuse_pairs_batch(h, n, T, p, None, 3.0, chi2, cap, ptr(start), *R.ptrs(without)[:3])
    assert fmap() == 0 and fhost() == 0                             # (the table by slot and the scratch exist from here on)
    R = Raw(cap)
    _rows_read_back(D, W)                                           # (the first local-map build allocates the map's staging)
    live1 = _live(lib)

    def refused(rc, code, *names):
        assert rc == code, (rc, err())
        for n in names:
            assert n in err(), (n, err())
        assert _live(lib) == live1, "a refusal holds nothing"
        assert R.untouched() and (start == SENTINEL).all(), "a refusal writes nothing"
        assert L.orbm_search_local_points_fetch(ex._h, fetch_a.ctypes.data, 64, fetch_n.ctypes.data, None) != 0, "nothing is pending"
        assert L.orbm_search_rig_batch_fetch(ex._h, fetch_a.ctypes.data, 64, fetch_n.ctypes.data, None, None) != 0, "nothing is pending"
        _rows_read_back(D, W)
    start[:] = SENTINEL
    # the new ones, both forms
    for f in (fmap, fhost):
        refused(f(cap=-1), E_ARG, b"cap")
        refused(f(start=None), E_ARG, b"start")
        refused(f(without=("point",)), E_ARG, b"point")
        refused(f(without=("feat",)), E_ARG, b"feat")
        refused(f(cap=1, without=("point", "feat")), E_ARG)
        # what both dense forms refuse
        refused(f(h=None), E_ARG)
        refused(f(n=-1), E_ARG)
        refused(f(T=None), E_ARG)
        refused(f(T=table(kfs[:2] + [None] + kfs[3:], specs, s2)), E_ARG, b"target 2")
        nos = table(kfs, specs, None); nos[0].inv_level_sigma2 = s2.ctypes.data
        refused(f(T=nos), E_ARG, b"target 1")
        e32, e1 = np.zeros(0, np.uint32), np.zeros(1, i32)
        flat = M.ResidentKeyFrame(ex, views.key_frame_view(S.targets[2].keys, S.targets[2].desc, np.zeros(0, f32), np.zeros(0, f32), e32, e1, e32, S.targets[2].u_right))
        live1 = _live(lib)
        refused(f(T=table(kfs[:3] + [flat] + kfs[4:], specs, s2), **({"rows": np.array(ROWS[:3] + (2,) + ROWS[4:], i32)} if f is fmap else {})), E_ARG, b"target 3")
        flat.close()
        live1 = _live(lib)
    refused(fhost(p=None), E_ARG)
    big = (views.FuseTarget * 65536)()
    for k in range(65536):
        big[k] = T[4]
    big_start = np.full(65537, SENTINEL, i32)
    refused(fhost(n=65536, T=big, start=big_start), E_CAPACITY)
    refused(fmap(n=65536, T=big, rows=np.full(65536, 4, i32), feat0=None, start=big_start), E_CAPACITY)
    assert (big_start == SENTINEL).all()
    # what the dense map form refuses
    refused(fmap(m=None), E_ARG, b"null map")
    refused(fmap(rows=None), E_ARG, b"row list")
    refused(fmap(set=-1), E_ARG, b"set -1"); refused(fmap(set=MAX_SETS), E_ARG, b"set %d" % MAX_SETS); refused(fmap(set=3), E_ARG, b"set 3")       # (set 3 was never built)
    r = rows.copy(); r[4] = KF_ROWS
    refused(fmap(rows=r), E_ARG, b"target 4", b"row %d" % KF_ROWS)
    r[4] = -1
    refused(fmap(rows=r), E_ARG, b"target 4")
    r = rows.copy(); r[7] = UNSET_ROW
    refused(fmap(rows=r), E_ARG, b"target 7", b"never set")
    f = feat0.copy(); f[6] = 71                                       # 71 + 1 100 is one more than the rig row holds
    refused(fmap(feat0=f), E_ARG, b"target 6")
    f[6] = -1
    refused(fmap(feat0=f), E_ARG, b"target 6")
    r = rows.copy(); r[3] = 2                                         # key frame 3 (1 100 keypoints) on the row of 70 entries
    refused(fmap(rows=r), E_ARG, b"target 3")
    other = None
    if two_devices:
        other = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib, device_id=1)
        live1 = _live(lib)
        refused(fmap(h=other._h), E_ARG, b"device")
        refused(fhost(h=other._h), E_ARG, b"device")
    # nothing to do: no targets (a null table is fine then), an empty set: start is all zero, nothing else is written
    s1 = np.full(1, SENTINEL, i32)
    assert fmap(n=0, T=None, start=s1) == 0 and s1[0] == 0 and fhost(n=0, T=None, start=s1) == 0 and s1[0] == 0
    mp.select(3, np.zeros(0, i32))
    assert fmap(set=3) == 0 and (start == 0).all() and R.untouched()
    start[:] = SENTINEL
    assert fhost(p=L.orbm_map_set(ex._h, mp._m, 3)) == 0 and (start == 0).all() and R.untouched()
    # after all of that both calls work
    assert fmap() == 0
    _same((start,) + tuple(R.a[name][:want[0][-1]] for name in NAMES[1:]), want, "after the refusals")
    R = Raw(cap)
    assert fhost() == 0
    _same((start,) + tuple(R.a[name][:hw[0][-1]] for name in NAMES[1:4]), hw, "the host-fed call after the refusals")
    if other is not None:
        other.close()
    D.close()
    assert _live(lib) == live_start, "device allocations, pinned allocations, streams, events: %s before, %s after" % (live_start, _live(lib))


def test_refusals_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("ORBX_EMU_DEVICES", "2")
    assert emu_lib.L.orbx_device_count() == 2
    _refusals(emu_lib, True)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    _refusals(hip_lib, False)


def _null_arguments(lib):
    """null pointers and zero sizes behind no handle and behind a live one: an error code, nothing dereferenced"""
    L = lib.L
    ex = ORBextractor(500, 1.2, NLEVELS, 20, 7, lib=lib)
    for h in (None, ex._h):
        for n in (0, 1):
            assert L.orbm_fuse_pairs_batch(h, n, None, None, None, 0.0, n, n, None, None, None, None) == E_ARG
            assert L.orbm_fuse_pairs_batch_map(h, n, None, None, None, None, n, 0.0, n, n, None, None, None, None, None, None) == E_ARG
    ex.close()


def test_null_arguments_emulated(emu_lib):
    _null_arguments(emu_lib)


@pytest.mark.gpu
def test_null_arguments_gpu(hip_lib):
    _null_arguments(hip_lib)
