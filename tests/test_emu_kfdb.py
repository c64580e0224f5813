"""Key frame database (KeyFrameDatabase -> orbv_db_*, the kernels of k_vocab.hip) on the CPU SIMT emulator: candidate order, word counts,
minCommonWords and the scored set against a restatement of the reference's inverted-file walk, every score bit-equal to the reference's
own DBoW2 score() (oracle/_ref/libref_dbow2.so), and the edge cases of add / erase / clear / clearMap.  The same on the GPU:
test_gpu_kfdb.py."""
import numpy as np
import pytest

import kfdb_world as kw
import vocab_scenes as vs
from kfdb_world import make, run_world
from orb_slam3_detailed_comments_amd._lib import OrbxError, ORBX_E_ARG, ORBX_E_CAPACITY
from orb_slam3_detailed_comments_amd.extractor import ORBextractor
from orb_slam3_detailed_comments_amd.vocabulary import ORBVocabulary, KeyFrameDatabase

SCORINGS = [0, 1, 2, 4, 5]          # L1, L2, chi-square, Bhattacharyya, dot product (KL is refused)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_kfdb_world_emulated(emu_lib, tmp_path, scoring):
    run_world(emu_lib, tmp_path, scoring)


@pytest.mark.parametrize("scoring", [2, 0, 1])
def test_kfdb_raw_vectors_with_zeros_emulated(emu_lib, tmp_path, scoring):
    """raw values with zeros in both vectors: the chi-square `vi + wi == 0` branch, and sums that are not normalised"""
    run_world(emu_lib, tmp_path, scoring, n_kf=60, zeros=0.3, normalise=False)


def test_kfdb_scores_need_the_oracle(emu_lib, tmp_path):
    _, _, _, score, _, _ = make(emu_lib, tmp_path, 0)
    if score is None:
        pytest.skip("oracle/_ref/libref_dbow2.so not built")
    assert score(([1, 2], [0.5, 0.5]), ([2, 3], [0.5, 0.5])) == 0.5


def test_kfdb_kl_refused(emu_lib, tmp_path):
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=emu_lib)
    rng = np.random.default_rng(1)
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 5, 2, 3, 0)
    voc = ORBVocabulary.from_arrays(ex, *header, parent, leaf, desc, weight)
    with pytest.raises(OrbxError) as e:
        KeyFrameDatabase(voc, ex)
    assert e.value.code == ORBX_E_ARG and "KL" in str(e.value)
    voc.close(); ex.close()                 # (the caught exception keeps this frame, and with it the handles, until the next collection)


def kfdb_edge_cases(lib, tmp_path):
    """duplicate adds, erases of middle / absent / last keys, exclusions, an empty query and one that shares nothing, capacity overflow, clearMap, clear"""
    ex, voc, db, score, desc, rng = make(lib, tmp_path, 0)
    nw = voc.size()
    ref = kw.RestatedDB(nw)
    a = (np.array([1, 5, 9, 20], np.uint32), np.array([0.1, 0.2, 0.3, 0.4]))
    b = (np.array([5, 9, 30], np.uint32), np.array([0.3, 0.3, 0.4]))
    c = (np.array([1, 2, 3], np.uint32), np.array([0.2, 0.3, 0.5]))
    bow_of = {1: a, 2: b, 3: c}
    q = (np.array([1, 5, 9, 30], np.uint32), np.array([0.25, 0.25, 0.25, 0.25]))

    def both(op, *args):
        getattr(db, op)(*args); getattr(ref, op)(*args)

    def check(what, exclude=()):
        r = db.query([q], exclude=[list(exclude)])[0]
        kw.check_query(r, ref.query(q[0], exclude), bow_of, q, score, what)
        return r
    # duplicate adds: counted twice, listed once (at the earliest add)
    for k, v in ((1, a), (2, b), (1, a), (3, c), (2, b)):
        both("add", k, *v)
    assert db.size() == 5
    r = check("duplicates")
    assert r["keys"].tolist() == [1, 3, 2] and r["words"].tolist() == [6, 1, 6]
    # a key added again with another vector is refused
    with pytest.raises(OrbxError):
        db.add(1, *b)
    # erase: a middle key once (one add survives), an absent key, the duplicate again
    both("erase", 2); check("erase middle duplicate")
    both("erase", 77); check("erase absent")
    both("erase", 2); r = check("erase last add")
    assert 2 not in r["keys"].tolist()
    # exclusions, ties in first position (1 and 3 both first meet word 1: add order decides)
    check("exclude", exclude=[1])
    # an empty query and one that shares nothing
    r0 = db.query([(np.zeros(0, np.uint32), np.zeros(0)), (np.array([nw - 1], np.uint32), np.array([1.0]))])
    assert all(len(x["keys"]) == 0 and x["min_common"] == 0 for x in r0)
    # capacity overflow reports the size needed
    with pytest.raises(OrbxError) as e:
        db.query([q], cap=1)
    assert e.value.code == ORBX_E_CAPACITY and e.value.n_out[0] == 2
    # clearMap, clear
    both("erase_keys", [1]); check("erase_keys")
    both("clear"); r = check("clear")
    assert len(r["keys"]) == 0 and db.size() == 0
    both("add", 3, *c); check("after clear")
    # bad input is refused
    with pytest.raises(OrbxError):
        db.add(9, np.array([3, 2], np.uint32), np.array([0.5, 0.5]))
    with pytest.raises(OrbxError):
        db.add(9, np.array([nw], np.uint32), np.array([0.5]))
    db.close(); voc.close(); ex.close()     # (the caught exceptions keep this frame, and with it the handles, until the next collection)


def test_kfdb_edge_cases_emulated(emu_lib, tmp_path):
    kfdb_edge_cases(emu_lib, tmp_path)


def kfdb_min_common_every_max(lib, tmp_path):
    """minCommonWords = (int)(maxCommonWords * 0.8f) for every maximum 1 .. 5000: a key added m times shares m words with a one-word query"""
    ex, voc, db, score, desc, rng = make(lib, tmp_path, 0)
    # one key per m would need 12.5 M adds; instead a key with m words and a query of those m words
    ids = np.arange(min(voc.size(), 5000), dtype=np.uint32)
    assert len(ids) >= 900
    bows = []
    for m in range(1, len(ids) + 1):
        bows.append((ids[:m], np.full(m, 1.0 / m)))
    db.add(1, ids, np.full(len(ids), 1.0 / len(ids)))
    res = db.query(bows)
    for m, r in zip(range(1, len(ids) + 1), res):
        assert r["words"].tolist() == [m] and r["min_common"] == int(np.float32(m) * np.float32(0.8)), m
    # the larger maxima through duplicate adds of a one-word key
    db.clear()
    one = (np.array([7], np.uint32), np.array([1.0]))
    added = 0
    for m in list(range(len(ids) + 1, 5001, 97)) + [5000]:
        while added < m:
            db.add(2, *one); added += 1
        r = db.query([one])[0]
        assert r["words"].tolist() == [m] and r["min_common"] == int(np.float32(m) * np.float32(0.8)), m


def test_kfdb_min_common_every_max_emulated(emu_lib, tmp_path):
    kfdb_min_common_every_max(emu_lib, tmp_path)


def test_kfdb_extracted_emulated(emu_lib, tmp_path):
    """queries and adds read from the vocabulary transform of an extracted batch = the same vectors from the host"""
    from orb_slam3_detailed_comments_amd import synth
    ex, voc, db, score, desc, rng = make(emu_lib, tmp_path, 0, k=8, L=3)
    imgs = np.stack([synth.corner_field(320, 240, seed=s, nrect=700) for s in (1, 2, 3, 4)])
    ex.enqueue(imgs)
    voc.transform_extracted(ex, 0, 4, 2)
    res = ex.fetch()
    fetched = [voc.fetch(ex, b, len(res[b][2])) for b in range(4)]
    bows = [(f.bow_id, f.bow_val) for f in fetched]
    ref = kw.RestatedDB(voc.size())
    for b in range(3):
        db.add_extracted(50 + b, ex, b); ref.add(50 + b, *bows[b])
    for b in range(3):
        db.add(60 + b, *bows[b]); ref.add(60 + b, *bows[b])
    bow_of = {50 + b: bows[b] for b in range(3)}; bow_of.update({60 + b: bows[b] for b in range(3)})
    got = db.query_extracted(ex, 1, 3, exclude=[[51], [], [60]])
    host = db.query(bows[1:4], exclude=[[51], [], [60]])
    for q in range(3):
        kw.check_query(got[q], ref.query(bows[1 + q][0], [[51], [], [60]][q]), bow_of, bows[1 + q], score, q)
        for f in ("keys", "words", "scored"):
            assert got[q][f].tolist() == host[q][f].tolist()
        assert got[q]["score"].tobytes() == host[q]["score"].tobytes()
    with pytest.raises(OrbxError):
        db.query_extracted(ex, 2, 3)
    db.close(); voc.close(); ex.close()


def test_kfdb_numpy_restatement_emulated(emu_lib, tmp_path):
    """the vectorised restatement the GPU scale test uses agrees with the list walk, and the device with both, on a mid-sized map"""
    ex, voc, db, score, desc, rng = make(emu_lib, tmp_path, 0)
    bows = kw.scale_bows(rng, voc.size(), 600, per_kf=120)
    keys = [5000 + i for i in range(len(bows))]
    ref = kw.RestatedDB(voc.size())
    for k, b in zip(keys, bows):
        db.add(k, *b); ref.add(k, *b)
    npr = kw.NumpyRestatement(keys, bows, voc.size())
    qs = [bows[i] for i in (0, 299, 599)]
    res = db.query(qs)
    for q, r in zip(qs, res):
        assert npr.query(q[0]) == ref.query(q[0])
        kw.check_query(r, ref.query(q[0]), dict(zip(keys, bows)), q, score)


def test_kfdb_lifetime_emulated(emu_lib, tmp_path):
    import ctypes as C
    live = (C.c_longlong * 4)()
    emu_lib.L.orbx_debug_live_resources(live)
    before = list(live)
    ex, voc, db, score, desc, rng = make(emu_lib, tmp_path, 0)
    bows = kw.trajectory_bows(rng, voc.size(), 50)
    for i, b in enumerate(bows):
        db.add(i, *b)
    db.query(bows[:4])
    for i in range(0, 50, 2):
        db.erase(i)
    db.query(bows[:4])
    db.close(); voc.close(); ex.close()
    emu_lib.L.orbx_debug_live_resources(live)
    assert list(live) == before
