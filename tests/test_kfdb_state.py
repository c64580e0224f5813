"""The key frame database as a thing with a history (csrc/orbv_api.cpp: db_add_host, db_compact, db_sync, db_run, orbv_db_erase, orbv_db_erase_keys,
orbv_db_clear): it erases, compacts its arena and brings its device mirror up to date BETWEEN queries, and every query has to answer as
KeyFrameDatabase's inverted file would after the same history.  The mutation pass recorded in profiles/emu_mutants_map/README.md found no mutant in that
code; this file walks the states it decides on:

  - db_sync compacts when the erased words outnumber the live ones (`dead_words > live_words`): queries with exactly as many erased as live words, and with
    one record more erased; and when the arena would have to grow while it holds erased words (`ids.size() > d_ids.n`, an arena of 4 096 words to begin
    with): queries at exactly 4 096 words and at 4 097;
  - a key added twice with other keys in between, erased once (the EARLIEST add goes: the key moves to its second add's place in the walk), excluded, erased
    by erase_keys (every add goes, size() counts both);
  - a key erased to its last add and added again with ANOTHER BowVector; clear, then fewer words than before;
  - a result of exactly `cap` keys, and one key more than cap;
  - check_capacity (the limit of run() on the features per image, which is the extractor's capacity orbx_max_keypoints): an extractor of 16 384 is the last
    accepted by orbv_transform_extracted and one of 16 385 the first refused; a rig of 2 x 8 192 the last accepted by orbv_transform_rig_extracted and one of
    2 x 8 193 the first refused - before the gather, so the earlier run's results fetch as they were; and its neighbour in orbv_transform_descriptors:
    16 384 descriptors accepted, 16 385 refused.

Expected: tests/kfdb_world.py::RestatedDB, the inverted file as lists, and - in the emulated form, where oracle/_ref/libkfdb_ref.so is built - THE REFERENCE'S OWN
src/KeyFrameDatabase.cc driven through the same history (RefDB below: add, erase, clearMap and DetectRelocalizationCandidates of oracle/ref_kfdb_driver.cpp):
after every query without exclusions the key frames the reference stamped with the query's id, their mnRelocWords, which of them it scored, the scores and the
order of its candidates must be what the model AND the library say.  Scores: the reference's score() (oracle/_ref/libref_dbow2.so); the transforms: the
reference's own DBoW2 transform (emulated form; the device form checks what is accepted and refused, the vector's invariants and that a refusal leaves the
earlier results as they were)."""
import ctypes as C
import os

import numpy as np
import pytest

import kfdb_world as kw
import oracle_lib as ol
import vocab_scenes as vs
from orb_slam3_detailed_comments_amd._lib import OrbxError

E_CAPACITY = -4
KFDB_REF = os.path.join(ol.ROOT, "oracle", "_ref", "libkfdb_ref.so")


class RefDB:
    """the reference's KeyFrameDatabase over its own KeyFrame objects (oracle/ref_kfdb_driver.cpp), keys as key frames: add / erase as they are, erase_keys as
    clearMap of a map the keys are moved into first, clear as clearMap of everything, a query as DetectRelocalizationCandidates of a Frame with a fresh id"""
    NONE = -7.0

    def __init__(self, voc_path, n=400):
        self.L = C.CDLL(KFDB_REF)
        self.L.kr_create.restype = C.c_void_p
        self.L.kr_create.argtypes = [C.c_char_p, C.c_int]
        self.L.kr_sync.argtypes = [C.c_void_p, C.c_int, C.c_ulong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.kr_fields.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for f in (self.L.kr_add, self.L.kr_erase, self.L.kr_clear_map):
            f.argtypes = [C.c_void_p, C.c_int]
        self.L.kr_reloc.argtypes = [C.c_void_p, C.c_ulong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self.w = self.L.kr_create(str(voc_path).encode(), n)
        assert self.w, "the reference does not load %s" % voc_path
        self.index, self.bow, self.n, self.qid = {}, {}, n, 1000000

    def _sync(self, key, map_=0):
        ids, vals = self.bow[key]
        i = np.ascontiguousarray(ids, np.uint32); v = np.ascontiguousarray(vals, np.float64)
        q = np.array([-1, 0, -1, 0], np.int64); sc = np.array([self.NONE, self.NONE], np.float32)
        self.L.kr_sync(self.w, self.index[key], key, map_, 0, len(i), i.ctypes.data, v.ctypes.data, 0, None, q.ctypes.data, sc.ctypes.data)

    def add(self, key, ids, vals):
        if key not in self.index:
            assert len(self.index) < self.n
            self.index[key] = len(self.index)
        self.bow[key] = (np.asarray(ids), np.asarray(vals))
        self._sync(key)
        self.L.kr_add(self.w, self.index[key])

    def erase(self, key):
        if key in self.index:
            self.L.kr_erase(self.w, self.index[key])             # (with the vector the key frame holds: the one of its latest add)

    def erase_keys(self, keys):
        mine = [k for k in set(keys) if k in self.index]
        for k in mine:
            self._sync(k, 1)
        self.L.kr_clear_map(self.w, 1)                           # KeyFrameDatabase::clearMap: every entry of every key frame of the map

    def clear(self):
        for k in self.index:
            self._sync(k, 0)
        self.L.kr_clear_map(self.w, 0)

    def query(self, qids, qvals):
        """({key: mnRelocWords} of the key frames stamped with this query, {key: mRelocScore} of those the reference scored, its candidates in its order)"""
        for k in self.index:
            self._sync(k, 0)                                     # (the fields back to `never queried`; vector and map as they are)
        self.qid += 1
        i = np.ascontiguousarray(qids, np.uint32); v = np.ascontiguousarray(qvals, np.float64)
        out = np.full(self.n, -1, np.int32)
        n = self.L.kr_reloc(self.w, self.qid, len(i), i.ctypes.data, v.ctypes.data, 0, out.ctypes.data, self.n)
        key_of = {x: k for k, x in self.index.items()}
        words, scores = {}, {}
        for k, x in self.index.items():
            q = np.zeros(4, np.int64); sc = np.zeros(2, np.float32)
            self.L.kr_fields(self.w, x, q.ctypes.data, sc.ctypes.data)
            if q[0] == self.qid:
                words[k] = int(q[1])
                if sc[0] != np.float32(self.NONE):
                    scores[k] = sc[0]
        return words, scores, [key_of[int(x)] for x in out[:n]]


class Both:
    """the database and the model side by side"""

    def __init__(self, lib, tmp_path, reference=False):
        self.ex, self.voc, self.db, self.score, self.desc, self.rng = kw.make(lib, tmp_path, 0)
        self.nw = self.voc.size()
        self.ref = kw.RestatedDB(self.nw)
        self.bow_of, self.adds = {}, 0
        self.refdb = RefDB(tmp_path / "voc_s0.txt") if reference else None        # (the emulated form: the reference does not exist beside a device)
        self.ref_queries = 0

    def bow(self, n, lo, hi):
        """n distinct words of [lo, hi), L1-normalised values"""
        ids = np.sort(self.rng.choice(np.arange(lo, hi), n, replace=False)).astype(np.uint32)
        v = self.rng.uniform(0.05, 3.0, n)
        return ids, (v / v.sum()).astype(np.float64)

    def add(self, key, b):
        self.db.add(key, *b); self.ref.add(key, *b); self.bow_of[key] = b; self.adds += 1
        if self.refdb:
            self.refdb.add(key, *b)

    def erase(self, key):
        if any(key in l for l in self.ref.inv):
            self.adds -= 1
        self.db.erase(key); self.ref.erase(key)
        if self.refdb:
            self.refdb.erase(key)

    def erase_keys(self, keys):
        for k in set(keys):
            self.adds -= max([l.count(k) for l in self.ref.inv] + [0])
        self.db.erase_keys(keys); self.ref.erase_keys(keys)
        if self.refdb:
            self.refdb.erase_keys(keys)

    def clear(self):
        self.db.clear(); self.ref.clear(); self.adds = 0
        if self.refdb:
            self.refdb.clear()

    def check(self, queries, what, exclude=None):
        res = self.db.query(queries, exclude=exclude)
        for q, (qb, r) in enumerate(zip(queries, res)):
            exp = self.ref.query(qb[0], () if exclude is None else exclude[q])
            kw.check_query(r, exp, self.bow_of, qb, self.score, "%s, query %d" % (what, q))
            if self.refdb and exclude is None:                       # (DetectRelocalizationCandidates has no exclusions)
                self._against_reference(qb, r, exp, "%s, query %d" % (what, q))
        assert self.db.size() == self.adds, "%s: size() = %d after %d surviving adds" % (what, self.db.size(), self.adds)
        return res

    def _against_reference(self, qb, r, exp, what):
        """the reference's own walk of its inverted file after the same history: who shares words and how many, minCommonWords through who is scored, the scores
        as the floats it keeps, and its candidates - the scored key frames above 0.75 of the best score, in the order the walk first met them"""
        words, scores, cand = self.refdb.query(*qb)
        order, ewords, minc, escored = exp
        assert words == dict(zip(order, ewords)), "%s: the reference counts %s, the model %s" % (what, words, dict(zip(order, ewords)))
        assert set(scores) == {k for k, s in zip(order, escored) if s}, "%s: the reference scores %s (the model's minCommonWords is %d)" % (what, sorted(scores), minc)
        got = dict(zip(r["keys"].tolist(), r["score"].tolist()))
        for k, s in scores.items():
            assert np.float32(got[k]) == s, "%s: key %d scored %r, the reference keeps %r" % (what, k, got[k], s)
        if scores:
            best = max(scores.values())
            want = [k for k in r["keys"].tolist() if k in scores and scores[k] > np.float32(0.75) * best]
            assert cand == want, "%s: the reference's candidates %s, from the library's order %s" % (what, cand, want)
        else:
            assert cand == []
        self.ref_queries += 1

    def close(self):
        self.db.close(); self.voc.close(); self.ex.close()


def _compaction(lib, tmp_path, reference=False):
    W = Both(lib, tmp_path, reference)
    try:
        assert W.nw >= 900
        # 12 records of 8 words out of 40: every pair of keys shares words.  Key 103 is added twice, with two other keys in between
        keys = [100, 101, 102, 103, 104, 105, 103, 106, 107, 108, 109, 110]
        bows = {k: W.bow(8, 0, 40) for k in set(keys)}
        for k in keys:
            W.add(k, bows[k])
        queries = [(np.arange(0, 40, dtype=np.uint32), np.full(40, 1.0 / 40)), bows[103], W.bow(10, 20, 60)]
        r = W.check(queries, "12 records")
        assert r[0]["keys"].tolist().count(103) == 1 and W.db.size() == 12
        before = r[0]["keys"].tolist()
        # exactly as many keys as cap, and one more than cap
        n = len(r[0]["keys"])
        assert n == 11 and len(W.db.query(queries[:1], cap=n)[0]["keys"]) == n
        with pytest.raises(OrbxError) as e:
            W.db.query(queries[:1], cap=n - 1)
        assert e.value.code == E_CAPACITY and e.value.n_out[0] == n
        # an exclusion of the key that was added twice
        W.check(queries, "103 excluded", exclude=[[103], [], [103, 100]])
        # the earliest add of 103 goes: it is met where its SECOND add stands (behind 104 and 105 wherever they share the word)
        W.erase(103)
        r = W.check(queries, "103 erased once")
        order = r[0]["keys"].tolist()
        assert 103 in order and order.index(103) > before.index(103), (before, order)
        # five more single erases: 6 records = 48 words erased, 6 records = 48 words live - the threshold itself, no compaction yet
        for k in (100, 102, 104, 106, 108):
            W.erase(k)
        assert W.adds == 6
        W.check(queries, "erased words == live words")
        W.check(queries, "the same again")                          # (nothing changed: the mirror is current)
        # one record more: 56 erased words against 40 live ones - the next query compacts first
        W.erase(110)
        r = W.check(queries, "erased words > live words")
        assert sorted(r[0]["keys"].tolist()) == [101, 103, 105, 107, 109]
        # behind a compaction: a new record (the appended tail goes up), a key that was erased comes back with ANOTHER vector, then twice more
        W.add(111, W.bow(8, 0, 40))
        W.check(queries, "a record behind the compaction")
        other = W.bow(8, 0, 40)                                      # (as many words as its first vector had: only the contents tell them apart)
        W.add(100, other); W.add(112, W.bow(8, 0, 40)); W.add(100, other)
        with pytest.raises(OrbxError):
            W.db.add(100, *bows[100])                                # (its first vector is another one now)
        with pytest.raises(OrbxError):
            W.db.add(112, other[0], other[1])                        # a live key, another vector of the SAME size
        for ids in ([3, 3, 9], [3, 9, 9], [4, 3]):                   # a BowVector is a map: a word id twice, or out of order, is no BowVector
            with pytest.raises(OrbxError):
                W.db.add(300, np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids)))
        W.check(queries, "an erased key added again with another vector")
        # erase_keys takes every add of a key; an absent key and a key twice in the list are fine
        W.erase_keys([100, 999, 101, 100])
        r = W.check(queries, "erase_keys")
        assert 100 not in r[0]["keys"].tolist() and W.db.size() == W.adds == 6
        W.check(queries, "erase_keys, excluded", exclude=[[105], [105, 111], []])
        # clear, then fewer words than the mirror held
        W.clear()
        assert all(len(x["keys"]) == 0 for x in W.check(queries, "cleared"))
        W.add(200, W.bow(5, 0, 40)); W.add(201, W.bow(3, 10, 30))
        r = W.check(queries, "two small records after the clear")
        assert len(r[0]["keys"]) == 2
        assert not reference or W.ref_queries == 30, "every query without exclusions was answered by the reference too: %d" % W.ref_queries
    finally:
        W.close()


def test_compaction_threshold_and_history_emulated(emu_lib, tmp_path):
    _compaction(emu_lib, tmp_path)


@pytest.mark.skipif(not os.path.exists(KFDB_REF), reason="oracle/_ref/libkfdb_ref.so not built (needs the reference)")
def test_compaction_threshold_and_history_against_the_reference(emu_lib, tmp_path):
    _compaction(emu_lib, tmp_path, reference=True)


@pytest.mark.gpu
def test_compaction_threshold_and_history_gpu(hip_lib, tmp_path):
    _compaction(hip_lib, tmp_path)


def _arena(lib, tmp_path, reference=False):
    """the arena's first size is 4 096 words: 64 records of 64 words fill it exactly (a quarter of them erased: fewer than the live ones, so that rule does not
    compact); the 65th record would make it grow, and is the one that compacts instead"""
    W = Both(lib, tmp_path, reference)
    try:
        W.add(1, W.bow(64, 0, 300))
        queries = [W.bow(80, 0, 300), W.bow(64, 100, 400)]
        W.check(queries, "one record")                               # (the first synchronisation allocates the arena)
        for k in range(2, 65):
            W.add(k, W.bow(64, 0, 300))
        for k in range(4, 65, 4):
            W.erase(k)
        assert sum(len(b[0]) for b in W.bow_of.values()) == 4096 and W.adds == 48
        W.check(queries, "4 096 words in the arena, 1 024 of them erased")
        W.add(65, (np.array([7], np.uint32), np.array([1.0])))
        W.check(queries, "4 097 words: compacted instead of grown")
        W.add(66, W.bow(64, 0, 300))
        for k in (1, 65, 3):
            W.erase(k)
        W.check(queries, "behind the compaction")
    finally:
        W.close()


def test_arena_edge_emulated(emu_lib, tmp_path):
    _arena(emu_lib, tmp_path)


@pytest.mark.skipif(not os.path.exists(KFDB_REF), reason="oracle/_ref/libkfdb_ref.so not built (needs the reference)")
def test_arena_edge_against_the_reference(emu_lib, tmp_path):
    _arena(emu_lib, tmp_path, reference=True)


@pytest.mark.gpu
def test_arena_edge_gpu(hip_lib, tmp_path):
    _arena(hip_lib, tmp_path)


def _transform_limit(lib, tmp_path, reference):
    ex, voc, db, score, desc, rng = kw.make(lib, tmp_path, 0)
    try:
        q = vs.descriptors_near(rng, desc, 16385)
        r = voc.transform(q[:16384], 2)                              # the last accepted size
        assert len(r.word_id) == 16384 and len(r.bow_id) == len(np.unique(r.bow_id)) > 100 and (np.diff(r.bow_id.astype(np.int64)) > 0).all()
        assert abs(r.bow_val.sum() - 1.0) < 1e-9 and r.fv_start[-1] <= 16384 and sorted(r.fv_feat.tolist()) == sorted(set(r.fv_feat.tolist()))
        if reference:
            ref = ol.RefVocabulary(tmp_path / "voc_s0.txt")
            bi, bv, fn, fs, ff = ref.transform(q[:16384], 2)
            assert np.array_equal(r.bow_id, bi) and r.bow_val.tobytes() == bv.tobytes()
            assert np.array_equal(r.fv_node, fn) and np.array_equal(r.fv_start, fs) and np.array_equal(r.fv_feat, ff)
        with pytest.raises(OrbxError) as e:
            voc.transform(q, 2)                                      # the first refused one
        assert e.value.code == E_CAPACITY and "16384" in str(e.value)
        again = voc.transform(q[:700], 2)                            # the refusal leaves the vocabulary usable
        assert len(again.word_id) == 700 and np.array_equal(again.word_id, r.word_id[:700])
    finally:
        db.close(); voc.close(); ex.close()


def test_transform_16384_descriptors_emulated(emu_lib, tmp_path):
    if ol.reference_dbow2() is None:
        pytest.skip("oracle/_ref/libref_dbow2.so not built")
    _transform_limit(emu_lib, tmp_path, True)


@pytest.mark.gpu
def test_transform_16384_descriptors_gpu(hip_lib, tmp_path):
    _transform_limit(hip_lib, tmp_path, False)


# ---- check_capacity: the extractor's capacity at the line, for the plain and the rig transform of extracted frames --------------------------------------
# orbx_max_keypoints() of an extractor is nFeatures + 3 per level on an image this small (csrc/orbx_api.cpp: the sum of quota + 3 over the levels), and that
# capacity - not what an image yields - is what check_capacity is given: 16 360 features in 8 levels are 16 384, 8 168 are 8 192.
def _bow(r):
    return [np.asarray(a).copy() for a in (r.bow_id, r.bow_val, r.fv_node, r.fv_start, r.fv_feat)]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _capacity_line(lib, tmp_path, reference):
    from orb_slam3_detailed_comments_amd import synth
    from orb_slam3_detailed_comments_amd.extractor import ORBextractor
    ex0, voc, db, score, desc, rng = kw.make(lib, tmp_path, 0)
    ref = ol.RefVocabulary(tmp_path / "voc_s0.txt") if reference else None
    imgs = np.stack([synth.corner_field(320, 240, seed=s, nrect=500) for s in (4, 5)])
    made = []

    def extractor(nf, want_cap):
        ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib); made.append(ex)
        res = ex.extract_batch(imgs)
        assert ex.max_keypoints() == want_cap, "an extractor of %d features holds %d key points" % (nf, ex.max_keypoints())
        return ex, [np.ascontiguousarray(r[2], np.uint8).reshape(-1, 32) for r in res]

    def check(got, rows, what):
        assert len(got[0]) > 20 and (np.diff(got[0].astype(np.int64)) > 0).all() and abs(got[1].sum() - 1.0) < 1e-9 and got[3][-1] == len(got[4]) <= len(rows), what
        if ref is not None:
            assert _same(got, [np.asarray(a) for a in ref.transform(rows, 2)]), "%s: not the reference's transform" % what
    try:
        # one camera: 16 384 is the last capacity accepted, 16 385 the first refused - on the host, before anything of the earlier run is touched
        ex, d = extractor(16360, 16384)
        voc.transform_extracted(ex, 0, 2, 2)
        first = [_bow(voc.fetch(ex, b, len(d[b]))) for b in range(2)]
        for b in range(2):
            check(first[b], d[b], "capacity 16 384, image %d" % b)
        over, _ = extractor(16361, 16385)
        with pytest.raises(OrbxError) as e:
            voc.transform_extracted(over, 0, 2, 2)
        assert e.value.code == E_CAPACITY and "16384" in str(e.value)
        for b in range(2):
            assert _same(_bow(voc.fetch(ex, b, len(d[b]))), first[b]), "the refused transform changed the results of image %d of the run before it" % b
        # a rig: 2 x 8 192 accepted, 2 x 8 193 refused before the gather of its rows
        exL, dl = extractor(8168, 8192); exR, dr = extractor(8168, 8192)
        voc.transform_rig_extracted(exL, 0, exR, 1, 1, 2)               # left image 0 with right image 1
        rows = np.concatenate([dl[0], dr[1]])
        rig = _bow(voc.fetch(exL, 0, len(rows)))
        check(rig, rows, "rig of 2 x 8 192")
        assert not _same(rig[:2], first[0][:2])
        oL, _ = extractor(8169, 8193); oR, _ = extractor(8169, 8193)
        with pytest.raises(OrbxError) as e:
            voc.transform_rig_extracted(oL, 0, oR, 1, 1, 2)
        assert e.value.code == E_CAPACITY and "16384" in str(e.value)
        assert _same(_bow(voc.fetch(exL, 0, len(rows))), rig), "the refused rig transform changed the results of the rig run before it"
        # and the database still reads that run where it lies
        db.add_extracted(7, exL, 0)
        r = db.query([(rig[0], rig[1])])[0]
        assert r["keys"].tolist() == [7] and r["words"].tolist() == [len(rig[0])]
    finally:
        db.close(); voc.close()
        for x in made + [ex0]:
            x.close()


def test_extractor_capacity_at_the_line_emulated(emu_lib, tmp_path):
    if ol.reference_dbow2() is None:
        pytest.skip("oracle/_ref/libref_dbow2.so not built")
    _capacity_line(emu_lib, tmp_path, True)


@pytest.mark.gpu
def test_extractor_capacity_at_the_line_gpu(hip_lib, tmp_path):
    _capacity_line(hip_lib, tmp_path, False)
