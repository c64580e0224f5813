"""orbm_search_by_projection_sim3_batch_map: the Sim3 projection batch on a set of the resident map.  A point is skipped for target k iff its slot is bad
at the moment of the call or listed in the target's found list (spAlreadyFound(vpMatched..), src/ORBmatcher.cc:512-525 and :633-645), both decided on the
device (k_map_set_table, k_map_skip_listed, k_map_skip_dups); `assigned` also comes back as map slots (k_assigned_slots).

Expected values never come from the new call: they are tests/test_sim3_projection_batch.py::scene().expect(.., skip=True) - the oracle's sequential accept
loop, target by target - on a copy of that scene whose skip mask is the NUMPY RESTATEMENT OF THE RULE (test_fuse_map.skip_rule) on a host mirror of the slot
states, the set's slot list and the found lists; assigned_slot is the mirror's slot of every assigned point.

The world: the scene's 300 points at permuted slots of a store of 1 000; a tenth of them set bad AFTER orbm_map_select; found lists that hold slots of the
set, duplicates, -1, slots outside the set and slots never updated - one list is empty - and the found_start = NULL form."""
import copy

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import ORBextractor, views
from orb_slam3_detailed_comments_amd import matcher as M
from test_fuse_batch import NLEVELS, _live
from test_fuse_map import BAD, E_ARG, E_CAPACITY, PRESENT, skip_rule
from test_sim3_projection_batch import RATIOS, THS, _taken_by, scene

f32, i32, u8 = np.float32, np.int32, np.uint8
SLOTS, MAX_SETS, PSET = 1000, 4, 1


class World:
    def __init__(self, S):
        rng = np.random.default_rng(4711)
        perm = rng.permutation(SLOTS).astype(i32)
        self.set_slots = perm[:S.M].copy()
        self.other, self.never = perm[S.M:700].copy(), perm[700:].copy()
        self.late_bad = rng.choice(self.set_slots, S.M // 10, replace=False).astype(i32)
        n = len(self.other)
        self.other_fields = (rng.normal(0, 3, (n, 3)).astype(f32), rng.normal(0, 1, (n, 3)).astype(f32), rng.uniform(0.5, 1, n).astype(f32),
                             rng.uniform(5, 9, n).astype(f32), rng.integers(0, 256, (n, 32), dtype=u8))
        self.state = np.zeros(SLOTS, u8)
        self.state[self.set_slots] = PRESENT; self.state[self.other] = PRESENT; self.state[self.late_bad] |= BAD
        # found list of target k: about 30 % of the set's slots, 20 of them twice, slots outside the set, slots never updated, -1, shuffled; target 2's is empty
        self.found = []
        for k in range(S.K):
            a = rng.choice(self.set_slots, int(0.3 * S.M), replace=False)
            l = np.concatenate([a, a[:20], rng.choice(self.other, 40), rng.choice(self.never, 10), np.full(15, -1)]).astype(i32)
            self.found.append(rng.permutation(l).astype(i32) if k != 2 else np.zeros(0, i32))
        for a in [self.set_slots, self.other, self.never, self.late_bad, self.state] + self.found:
            a.setflags(write=False)


_WORLD = {}


def world():
    if "w" not in _WORLD:
        _WORLD["w"] = World(scene())
    return _WORLD["w"]


def subscene(S, idx, skip):
    """the scene with the points idx (in that order; duplicates allowed) and `skip` as its skip mask: expect(.., skip=True) is the oracle under that mask"""
    S2 = copy.copy(S)
    S2.pos, S2.normal, S2.mind, S2.maxd, S2.desc, S2.tag = S.pos[idx], S.normal[idx], S.mind[idx], S.maxd[idx], S.desc[idx], S.tag[idx]
    S2.M = len(idx); S2.skip = np.ascontiguousarray(skip, u8); S2.expected = {}; S2.free = {}
    return S2


_MASKED = {}


def masked(S, W, found):
    """the whole point set under the rule, with the found lists or without (found_start = NULL); one copy per form, so its oracle rows are computed once"""
    if found not in _MASKED:
        lists = W.found if found else [np.zeros(0, i32)] * S.K
        _MASKED[found] = subscene(S, np.arange(S.M), skip_rule(W.state, W.set_slots, lists))
    return _MASKED[found]


def expected(S2, ex, set_slots, th, ratio, occupied):
    """(assigned, nmatches, assigned_slot) of the oracle under S2's mask"""
    rows, nm = S2.expect(ex, th, ratio, occupied, skip=True)
    aslot = np.where(rows >= 0, np.asarray(set_slots, i32)[np.maximum(rows, 0)], rows).astype(i32)
    return rows, nm, aslot


class Device:
    def __init__(self, lib, S, W, device_id=0):
        self.ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib, device_id=device_id)
        self.kfs, self.specs = S.resident(self.ex)
        self.mp = mp = M.ResidentMap(self.ex, SLOTS, 1, 16, MAX_SETS)
        mp.update(W.set_slots, S.pos, S.normal, S.mind, S.maxd, S.desc)
        mp.update(W.other, *W.other_fields)
        mp.select(PSET, W.set_slots)
        mp.set_bad(W.late_bad, np.ones(len(W.late_bad), u8))

    def search(self, S, th, ratio, occupied, found, set=PSET):
        return M.ORBmatcher.SearchByProjectionSim3BatchMap(self.ex, self.kfs, self.specs, self.mp, set, th, ratio, occupied=list(S.occ) if occupied else None,
                                                           found=found, want_slots=True)

    def close(self):
        self.mp.close()
        for o in self.kfs + [self.ex]:
            o.close()


def _same(got, want, what):
    for name, g, w in zip(("assigned", "nmatches", "assigned_slot"), got, want):
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and len(bad) == 0, "%s: %s differs in %d entries, first %s: %d, expected %d" % (
            what, name, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


# ---- what the world is built for, on the oracle's rows and numpy alone ----
def _conditions(lib):
    """No result of the new call is read here.  Matched points excluded by a found list and by the bad flag alone, matches left, and the sequential accept
    order: a keypoint whose winner is excluded goes to a LATER point (>= 3 times).  The expectation changes when the rule ignores the bad flag and when it
    ignores the found lists, so equality on this world cannot pass on trivial input."""
    S, W = scene(), world()
    ex = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib)
    S2, S0 = masked(S, W, True), masked(S, W, False)
    member = skip_rule(W.state, W.set_slots, W.found, ignore_bad=True)
    bad = np.broadcast_to((W.state[W.set_slots] & BAD) != 0, member.shape)
    assert np.array_equal(S2.skip.astype(bool), member | bad) and np.array_equal(S0.skip.astype(bool), bad) and not member[2].any()
    S_nobad = subscene(S, np.arange(S.M), member)
    freed = 0
    for th in THS:
        plain = S.expect(ex, th, 1.0)[0]
        rows = S2.expect(ex, th, 1.0, skip=True)[0]
        by_list = by_bad = 0
        for k, T in enumerate(S.targets):
            took, took2 = _taken_by(plain[k], S.M), _taken_by(rows[k], S.M)
            by_list += int(((took >= 0) & member[k]).sum()); by_bad += int(((took >= 0) & bad[k] & ~member[k]).sum())
            assert (took2[S2.skip[k] == 1] == -1).all()
            for kp in np.flatnonzero(plain[k] >= 0):
                if S2.skip[k][plain[k, kp]] and rows[k, kp] > plain[k, kp]:
                    freed += 1
        assert by_list >= 50 and by_bad >= 10 and (rows >= 0).sum() >= 50, (by_list, by_bad, int((rows >= 0).sum()))
        assert (S0.expect(ex, th, 1.0, skip=True)[0] != rows).sum() >= 5 and (S_nobad.expect(ex, th, 1.0, skip=True)[0] != rows).sum() >= 5
    assert freed >= 3, freed
    ex.close()
    cat = np.concatenate(W.found)
    assert (cat == -1).any() and np.isin(cat, W.other).any() and np.isin(cat, W.never).any() and len(W.found[2]) == 0
    assert all(len(np.unique(l)) < len(l) for k, l in enumerate(W.found) if k != 2)


def test_world_conditions_hold_on_the_oracle_emulated(emu_lib):
    _conditions(emu_lib)


@pytest.mark.gpu
def test_world_conditions_hold_on_the_oracle_gpu(hip_lib):
    _conditions(hip_lib)


# ---- equality with the oracle under the rule ----
def _parity(lib):
    S, W = scene(), world()
    D = Device(lib, S, W)
    for found in (True, False):
        S2 = masked(S, W, found)
        for th in THS:
            for ratio in RATIOS:
                for occupied in (False, True):
                    got = D.search(S, th, ratio, occupied, W.found if found else None)
                    assert got[0].shape == (S.K, S.cap) and got[2].shape == (S.K, S.cap)
                    for k, T in enumerate(S.targets):
                        assert (got[0][k, T.N:] == -1).all() and (got[2][k, T.N:] == -1).all()
                    _same(got, expected(S2, D.ex, W.set_slots, th, ratio, occupied), "th %g ratio %g occupied %d found lists %d" % (th, ratio, occupied, found))
    # assigned_slot is optional; a list of K None is K empty lists
    a, nm = M.ORBmatcher.SearchByProjectionSim3BatchMap(D.ex, D.kfs, D.specs, D.mp, PSET, 5.0, 1.0, found=[None] * S.K)
    want = expected(masked(S, W, False), D.ex, W.set_slots, 5.0, 1.0, False)
    assert np.array_equal(a, want[0]) and np.array_equal(nm, want[1])
    D.close()


def test_parity_emulated(emu_lib):
    _parity(emu_lib)


@pytest.mark.gpu
def test_parity_gpu(hip_lib):
    _parity(hip_lib)


# ---- set sizes around a group of the accept loop and a block, duplicates in the set, and what an earlier call left in the table ----
def _sets(lib):
    S, W = scene(), world()
    D = Device(lib, S, W)
    dup = np.concatenate([np.arange(230, 300), np.arange(100), np.arange(250, 300), [7, 7, 7]])
    for idx in [np.arange(n) for n in (0, 1, 63, 64, 65, 256, 257)] + [dup]:
        slots = W.set_slots[idx]
        D.mp.select(2, slots)
        S2 = subscene(S, idx, skip_rule(W.state, slots, W.found))
        for th, ratio, occupied in ((5.0, 1.0, False), (8.0, 1.5, True)):
            got = D.search(S, th, ratio, occupied, W.found, set=2)
            if len(idx) == 0:
                assert (got[0] == -1).all() and (got[1] == 0).all() and (got[2] == -1).all()      # (nothing is written: the wrapper's initial values)
                continue
            _same(got, expected(S2, D.ex, slots, th, ratio, occupied), "a set of %d points, th %g" % (len(idx), th))
    # set A, then the disjoint set B with found lists that hold nothing but A's slots: they exclude nothing of B
    ia, ib = np.arange(150), np.arange(150, S.M)
    A, B = W.set_slots[ia], W.set_slots[ib]
    lists = [np.random.default_rng(k).permutation(A).astype(i32) for k in range(S.K)]
    D.mp.select(2, A); D.mp.select(3, B)
    SA, SB = subscene(S, ia, skip_rule(W.state, A, lists)), subscene(S, ib, skip_rule(W.state, B, lists))
    assert SA.skip.all() and np.array_equal(SB.skip.astype(bool), np.broadcast_to((W.state[B] & BAD) != 0, SB.skip.shape))
    for n in range(2):
        got = D.search(S, 5.0, 1.0, False, lists, set=2)
        assert (got[0] == -1).all() and (got[1] == 0).all()
        _same(D.search(S, 5.0, 1.0, False, lists, set=3), expected(SB, D.ex, B, 5.0, 1.0, False), "set B after set A (%d)" % n)
    assert (SB.expect(D.ex, 5.0, 1.0, False, skip=True)[1] > 0).sum() >= 2
    D.close()


def test_set_sizes_duplicates_and_stale_table_emulated(emu_lib):
    _sets(emu_lib)


@pytest.mark.gpu
def test_set_sizes_duplicates_and_stale_table_gpu(hip_lib):
    _sets(hip_lib)


# ---- refusals ----
def _refusals(lib, two_devices):
    L = lib.L
    S, W = scene(), world()
    live_start = _live(lib)
    D = Device(lib, S, W)
    ex, mp, K, cap = D.ex, D.mp, S.K, S.cap

    def table(kf_list, spec_list):
        T = (views.Sim3Target * max(len(kf_list), 1))()
        for k, (kf, sp) in enumerate(zip(kf_list, spec_list)):
            T[k].kf = kf._kf if kf is not None else None; T[k].spec = sp[0]; T[k].log_scale_factor = sp[1]; T[k].occupied = None
        return T
    T = table(D.kfs, D.specs)
    fs = np.cumsum([0] + [len(l) for l in W.found]).astype(i32); fl = np.concatenate(W.found).astype(i32)
    a = np.full((K, cap), -7, i32); nm = np.full(K, -7, i32); sl = np.full((K, cap), -7, i32)
    err = lambda: L.orbx_last_error() or b""
    ptr = lambda x: None if x is None else x.ctypes.data

    def search(h=ex._h, n=K, T=T, m=mp._m, set=PSET, fs=fs, fl=fl, cap=cap, out=a):
        return L.orbm_search_by_projection_sim3_batch_map(h, n, T, m, set, ptr(fs), ptr(fl), 5.0, 1.0, cap, ptr(out), nm.ctypes.data, sl.ctypes.data)
    want = expected(masked(S, W, True), ex, W.set_slots, 5.0, 1.0, False)
    assert search() == 0
    _same((a, nm, sl), want, "the first call")
    live1 = _live(lib)
    a[:] = -7; nm[:] = -7; sl[:] = -7

    def refused(rc, code, *names):
        assert rc == code, (rc, err())
        for n in names:
            assert n in err(), (n, err())
        assert _live(lib) == live1, "a refusal holds nothing"
        assert (a == -7).all() and (nm == -7).all() and (sl == -7).all(), "a refusal writes nothing"
    refused(search(h=None), E_ARG)
    refused(search(m=None), E_ARG, b"null map")
    refused(search(n=-1), E_ARG)
    refused(search(T=None), E_ARG)
    refused(search(out=None), E_ARG)
    refused(search(set=-1), E_ARG, b"set -1"); refused(search(set=MAX_SETS), E_ARG, b"set %d" % MAX_SETS); refused(search(set=3), E_ARG, b"set 3")
    refused(search(fl=None), E_ARG, b"found_slots")
    bad = fs.copy(); bad[4] = bad[3] - 1
    refused(search(fs=bad), E_ARG, b"target 3", b"decreases")
    bad = fs.copy(); bad[0] = -1
    refused(search(fs=bad), E_ARG, b"target 0")
    for v in (-2, SLOTS):
        bad = fl.copy(); bad[fs[4] + 5] = v
        refused(search(fl=bad), E_ARG, b"target 4", b"entry 5", b"slot %d" % v)
    # what the host-fed call refuses
    refused(search(T=table(D.kfs[:2] + [None] + D.kfs[3:], D.specs)), E_ARG, b"target 2")
    refused(search(cap=cap - 1), E_ARG, b"cap")
    big = (views.Sim3Target * 65536)()
    for k in range(65536):
        big[k] = T[1]
    refused(search(n=65536, T=big, fs=None, fl=None), E_CAPACITY)
    other = None
    if two_devices:
        other = ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib, device_id=1)
        live1 = _live(lib)
        refused(search(h=other._h), E_ARG, b"device")
    assert search(n=0, T=None) == 0
    mp.select(2, np.zeros(0, i32))
    assert search(set=2) == 0 and (a == -7).all()
    assert search() == 0
    _same((a, nm, sl), want, "after the refusals")
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
