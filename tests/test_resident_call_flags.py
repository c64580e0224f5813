"""The layout of a MIXED call-time flag block of the resident searches (CallFlags in orbm_search.cpp): the flag arrays of one call lie one behind the
other, each rounded up to 16 bytes, and an array that is not passed - or whose key frame has no features - takes no room in the BoW forms.  An offset
that is one array or one byte off crashes nothing: a feature reads another feature's flag.

One call of each search on key frames of 0, 1, 15, 16, 17 and 33 features (the edges of the rounding), neighbouring arrays deliberately different:
all ones, all zeros, a single one at the LAST index; a null array, a second row of -1 and a key frame without features between two others.
  * triangulation (4 neighbours) and key-frame BoW (5 pairs): host-fed == map-fed == the view forms orbm_search_for_triangulation_batch /
    orbm_search_by_bow_batch, which take the flags inside their views and stage them through code of their own;
  * frames batch (B = 3) and rig batch (P = 3): host-fed == map-fed == the single-frame view forms orbm_search_by_bow / orbm_search_by_bow_fisheye.
All comparisons are exact.  The test shows of its own inputs that they can tell: every pair with a non-empty first key frame matches, and the view
form given any ONE of the call's flag arrays inverted answers differently."""
import numpy as np
import pytest

import vocab_scenes as vs
from orb_slam3_detailed_comments_amd import ORBextractor, ORBVocabulary, synth, views
from orb_slam3_detailed_comments_amd import matcher as M
from test_map_rows_projection import SLOTS, Store, _live
from test_map_rows_resident import F_X, EP_FAR

KP = views.KP_DTYPE
SC = (1.2 ** np.arange(8)).astype(np.float32)
NODES = 3                                             # feature i of every hand-built key frame lies in vocabulary node i % NODES


def ones(N):
    return np.ones(N, np.uint8)


def zeros(N):
    return np.zeros(N, np.uint8)


def last(N):
    f = np.zeros(N, np.uint8); f[N - 1] = 1
    return f


class KF:
    """a key frame (or a frame with its FeatureVector): keypoints, descriptors, FeatureVector (node ids, starts, features), resident on the device where
    ex is given; view(flags) = the same as a view that carries flags"""

    def __init__(self, ex, keys, desc, fv):
        self.keys, self.desc, self.fv, self.N = keys, desc, fv, len(keys)
        self.res = M.ResidentKeyFrame(ex, self.view(None)) if ex is not None else None

    def view(self, flags):
        return views.key_frame_view(self.keys, self.desc, SC, SC * SC, self.fv[0], self.fv[1], self.fv[2], None, flags)


def hand_built(ex, base, N):
    """feature i = descriptor base[i] (every key frame sees the same ones: feature i of one matches feature i of another at distance 0, every other
    descriptor is a random one ~128 bits away), the same angle in all of them, in node i % NODES"""
    k = np.zeros(N, KP)
    k["x"] = 40.0 + 13.0 * np.arange(N); k["y"] = 50.0 + 7.0 * np.arange(N); k["size"] = 31.0; k["angle"] = (11.0 * np.arange(N)) % 360.0
    node_of = np.arange(N) % NODES
    nodes = np.unique(node_of)
    ft = np.concatenate([np.flatnonzero(node_of == n) for n in nodes]) if N else np.zeros(0, np.int64)
    st = np.concatenate([[0], np.cumsum([(node_of == n).sum() for n in nodes])])
    return KF(ex, k, base[:N].copy(), (nodes.astype(np.uint32), st.astype(np.int32), ft.astype(np.uint32)))


class Rows:
    """a map in which row(flags) is a fresh key-frame row that yields exactly these flags under both rules: a slot that holds a good point where the
    flag is set, -1 where it is not.  The rows are handed out in a permuted order, so that neighbouring arrays of a call come from rows far apart."""

    def __init__(self, ex, rng, n_rows, cap):
        self.store = Store(ex, kf_rows=n_rows, kf_row_cap=cap)
        self.rng = rng
        self.free = list(rng.permutation(SLOTS)); self.order = list(rng.permutation(n_rows))

    def row(self, flags):
        flags = np.asarray(flags, np.uint8)
        s = np.full(len(flags), -1, np.int32)
        pts = np.flatnonzero(flags)
        for i in pts:
            s[i] = self.free.pop()
        if len(pts):
            self.store.update(s[pts], self.rng.normal(0, 1, (len(pts), 3)) + [0, 0, 4], np.full(len(pts), 0.5, np.float32), np.full(len(pts), 30.0, np.float32),
                              self.rng.integers(0, 256, (len(pts), 32), dtype=np.uint8), np.zeros(len(pts), np.uint8))
        r = int(self.order.pop())
        self.store.set_keyframe(r, s)
        return r


def same(a, b):
    """two answers [(nmatches, matches)] of a search, exactly"""
    return len(a) == len(b) and all(x[0] == y[0] and np.array_equal(np.asarray(x[1]), np.asarray(y[1])) for x, y in zip(a, b))


def inversions(arrays):
    """the call's flag arrays with ONE non-empty array inverted, for each of them; None entries (arrays that are not passed) stay"""
    for j, f in enumerate(arrays):
        if f is not None and len(f):
            yield j, [(1 - g).astype(np.uint8) if i == j else g for i, g in enumerate(arrays)]


# ---- triangulation: KF1 at 0, then neighbour j; a set flag EXCLUDES the feature ------------------------------------------------------------------------

def _triangulation(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(51)
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    base = rng.integers(0, 256, (33, 32), dtype=np.uint8)
    kf = {N: hand_built(ex, base, N) for N in (33, 17, 0, 16, 15)}
    K1, K2s = kf[33], [kf[17], kf[0], kf[16], kf[15]]
    # block: [33: one at the last index | 17: ones | 0 features | 16: one at the last index | 15: not passed]
    mp1, mp2 = last(33), [ones(17), zeros(0), last(16), None]
    n2 = len(K2s)
    Fs = np.stack([F_X] * n2); eps = np.stack([EP_FAR] * n2)
    m = M.ORBmatcher(0.6, True)
    z = lambda f, K: zeros(K.N) if f is None else f                      # a view without flags reads as "no feature has a map point": as the null array

    def view_form(f1, f2):
        return m.SearchForTriangulationBatch(ex, K1.view(f1), [K.view(z(f, K)) for f, K in zip(f2, K2s)], Fs, eps, False, True)
    expect = view_form(mp1, mp2)
    print("triangulation:", [n for n, _ in expect])
    assert [n for n, _ in expect] == [0, 0, 15, 15]                     # all of 17 excluded | nothing to match | features 0 .. 14 | all 15
    host = m.SearchForTriangulationResident(ex, K1.res, mp1, [K.res for K in K2s], mp2, Fs, eps, False, True)
    maps = Rows(ex, rng, 2 * (1 + n2), 34)
    row1 = maps.row(mp1); rows2 = np.array([maps.row(z(f, K)) for f, K in zip(mp2, K2s)], np.int32)
    got = m.SearchForTriangulationResidentMap(ex, K1.res, row1, [K.res for K in K2s], rows2, maps.store.map, Fs, eps, False, True)
    assert host == expect, "host-fed flags vs the view form"
    assert got == expect, "flags from the map's rows vs the view form"
    told = 0
    for j, arrays in inversions([mp1] + mp2):
        assert view_form(arrays[0], arrays[1:]) != expect, "array %d inverted changes nothing: the inputs cannot tell" % j
        told += 1
    assert told == 3
    for K in kf.values():
        K.res.close()
    maps.store.close(); ex.close()
    assert _live(lib) == live0


def test_triangulation_block_emulated(emu_lib):
    _triangulation(emu_lib)


@pytest.mark.gpu
def test_triangulation_block_gpu(hip_lib):
    _triangulation(hip_lib)


# ---- key-frame BoW: per pair mp1 then elig2; a set flag ADMITS the feature --------------------------------------------------------------------------------

def _bow(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(52)
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    base = rng.integers(0, 256, (33, 32), dtype=np.uint8)
    kf = {N: hand_built(ex, base, N) for N in (0, 1, 15, 16, 17, 33)}
    sizes = [(33, 17), (0, 16), (17, 33), (1, 15), (16, 1)]
    K1s = [kf[a] for a, _ in sizes]; K2s = [kf[b] for _, b in sizes]
    # block: [33: ones | 17: one at the last index] [0 features | not passed] [17: one at the last index | 33: ones] [1: one | not passed] [16: ones | 1: one]
    mp1 = [ones(33), zeros(0), last(17), ones(1), ones(16)]
    el2 = [last(17), None, ones(33), None, ones(1)]
    for frame_version, ratio, ori in ((False, 0.7, True), (True, 0.9, False)):
        m = M.ORBmatcher(ratio, ori)

        def view_form(f1, f2):
            return m.SearchByBoWBatch(ex, [K.view(f) for K, f in zip(K1s, f1)], [K.view(f) for K, f in zip(K2s, f2)], frame_version)
        expect = view_form(mp1, el2)
        print("key-frame BoW:", [n for n, _ in expect])
        assert [n for n, _ in expect] == [1, 0, 1, 1, 1]               # feature 16 | no K1 | feature 16 | feature 0 | feature 0
        assert all(n > 0 for (n, _), K in zip(expect, K1s) if K.N > 0)
        host = m.SearchByBoWResident(ex, [K.res for K in K1s], mp1, [K.res for K in K2s], el2, frame_version)
        maps = Rows(ex, rng, 12, 34)
        rows1 = np.array([maps.row(f) for f in mp1], np.int32)
        rows2 = np.array([-1 if f is None else maps.row(f) for f in el2], np.int32)
        got = m.SearchByBoWResidentMap(ex, [K.res for K in K1s], rows1, [K.res for K in K2s], rows2, maps.store.map, frame_version)
        assert same(host, expect), "host-fed flags vs the view form"
        assert same(got, expect), "flags from the map's rows vs the view form"
        told = 0
        for j, arrays in inversions(mp1 + el2):
            assert not same(view_form(arrays[:5], arrays[5:]), expect), "array %d inverted changes nothing: the inputs cannot tell" % j
            told += 1
        assert told == 7
        maps.store.close()
    for K in kf.values():
        K.res.close()
    ex.close()
    assert _live(lib) == live0


def test_bow_block_emulated(emu_lib):
    _bow(emu_lib)


@pytest.mark.gpu
def test_bow_block_gpu(hip_lib):
    _bow(hip_lib)


# ---- the batch forms: frame b of an extraction (of a rig transform) against a key frame cut from it ---------------------------------------------------

def _vocabulary(ex, rng):
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 6, 3)
    return ORBVocabulary.from_arrays(ex, header[0], header[1], header[2], header[3], parent, leaf, desc, weight)


def _as_kp(k):
    out = np.zeros(len(k), KP)
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        out[f] = k[f]
    return out


def _cut(ex, voc, levelsup, F, pool, N):
    """a key frame of N of the features of frame F, descriptors and angles as the frame has them: those of `pool` that lie in a vocabulary node and whose
    descriptor is farthest from every other descriptor of the frame - each matches its own frame feature at distance 0 and passes any ratio test"""
    if N == 0:
        return KF(ex, np.zeros(0, KP), np.zeros((0, 32), np.uint8), (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)))
    keys, desc = F.keys, F.desc
    bits = np.unpackbits(desc, axis=1).astype(np.int32)
    dist = bits @ (1 - bits).T + (1 - bits) @ bits.T
    np.fill_diagonal(dist, 999)
    in_node = np.isin(pool, np.asarray(F.fv[2], np.int64))
    cand = pool[in_node]
    src = np.sort(cand[np.argsort(-dist[cand].min(axis=1), kind="stable")[:N]])
    assert len(src) == N and dist[src].min() > 40
    dk = desc[src].copy()
    bow_k = voc.transform(dk, levelsup)
    return KF(ex, _as_kp(keys[src]), dk, (bow_k.fv_node, bow_k.fv_start, bow_k.fv_feat))


def _frames_batch(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(53)
    B, levelsup, w, h = 3, 2, 376, 240
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([synth.corner_field(w, h, seed=810 + b, nrect=900) for b in range(B)]))
    voc = _vocabulary(ex, rng)
    frames, kfs = [], []
    for b, N in enumerate((17, 0, 33)):                                  # the key frame without features between the two others
        k, d = _as_kp(res[b][1]), res[b][2]
        bow_f = voc.transform(d, levelsup)
        frames.append(KF(None, k, d, (bow_f.fv_node, bow_f.fv_start, bow_f.fv_feat)))
        kfs.append(_cut(ex, voc, levelsup, frames[b], np.arange(len(k)), N))
    mps = [last(17), zeros(0), ones(33)]                                 # block: [17: one at the last index | 0 features | 33: ones]
    voc.transform_extracted(ex, 0, B, levelsup)                          # (after the host transforms above: they replace the vocabulary's last run)
    m = M.ORBmatcher(0.7, True)

    def view_form(flags):
        return [m.SearchByBoW(ex, K.view(f), F.view(None), True) for K, F, f in zip(kfs, frames, flags)]
    expect = view_form(mps)
    print("frames batch:", [n for n, _ in expect])
    assert [n for n, _ in expect] == [1, 0, 33]
    host = m.SearchByBoWFramesBatch(ex, voc, [K.res for K in kfs], mps)
    maps = Rows(ex, rng, B + 2, 34)
    rows = np.array([maps.row(f) for f in mps], np.int32)
    got = m.SearchByBoWFramesBatch(ex, voc, [K.res for K in kfs], None, resident_map=maps.store.map, rows=rows)
    assert same(host, expect), "host-fed flags vs the view form"
    assert same(got, expect), "flags from the map's rows vs the view form"
    assert sum(not same(view_form(arrays), expect) for _, arrays in inversions(mps)) == 2, "an inverted array changes nothing: the inputs cannot tell"
    for K in kfs:
        K.res.close()
    maps.store.close(); voc.close(); ex.close()
    assert _live(lib) == live0


def test_frames_batch_block_emulated(emu_lib):
    _frames_batch(emu_lib)


@pytest.mark.gpu
def test_frames_batch_block_gpu(hip_lib):
    _frames_batch(hip_lib)


def _rig_batch(lib):
    live0 = _live(lib)
    rng = np.random.default_rng(54)
    B, levelsup, w, h = 2, 2, 376, 240
    ex = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)                       # one handle: [L0, L1, R0, R1]
    res = ex.extract_batch(np.stack([synth.corner_field(w, h, seed=820 + b, nrect=900) for b in range(2 * B)]))
    voc = _vocabulary(ex, rng)
    frames, nleft = [], []
    for b in range(B):
        k = _as_kp(np.concatenate([res[b][1], res[B + b][1]])); d = np.concatenate([res[b][2], res[B + b][2]])
        bow_f = voc.transform(d, levelsup)
        frames.append(KF(None, k, d, (bow_f.fv_node, bow_f.fv_start, bow_f.fv_feat))); nleft.append(len(res[b][1]))
    frame_of = [0, 1, 0]                                                 # P = 3 pairs; one-camera key frames cut from camera 1 of their frame
    kfs = []
    for p, N in enumerate((16, 0, 33)):
        kfs.append(_cut(ex, voc, levelsup, frames[frame_of[p]], np.arange(nleft[frame_of[p]]), N))
    mps = [ones(16), zeros(0), last(33)]                                 # block: [16: ones | 0 features | 33: one at the last index]
    voc.transform_rig_extracted(ex, 0, ex, B, B, levelsup)
    n_frame = [len(F.keys) for F in frames]
    m = M.ORBmatcher(0.7, True)

    def view_form(flags):
        return [m.SearchByBoWFisheye(ex, K.view(f), frames[b].view(None), nleft[b]) for K, b, f in zip(kfs, frame_of, flags)]
    expect = view_form(mps)
    print("rig batch:", [n for n, _ in expect])
    assert expect[0][0] >= 16 and expect[1][0] == 0 and expect[2][0] >= 1    # (camera 2 may add a match of its own to a feature's camera-1 match)
    args = (ex, 0, ex, B, voc, frame_of, [K.res for K in kfs])
    host = m.SearchByBoWRigBatch(*args, mps, n_frame)
    maps = Rows(ex, rng, 5, 34)
    rows = np.array([maps.row(f) for f in mps], np.int32)
    got = m.SearchByBoWRigBatch(*args, None, n_frame, resident_map=maps.store.map, rows=rows)
    assert same(host, expect), "host-fed flags vs the view form"
    assert same(got, expect), "flags from the map's rows vs the view form"
    assert sum(not same(view_form(arrays), expect) for _, arrays in inversions(mps)) == 2, "an inverted array changes nothing: the inputs cannot tell"
    for K in kfs:
        K.res.close()
    maps.store.close(); voc.close(); ex.close()
    assert _live(lib) == live0


def test_rig_batch_block_emulated(emu_lib):
    _rig_batch(emu_lib)


@pytest.mark.gpu
def test_rig_batch_block_gpu(hip_lib):
    _rig_batch(hip_lib)
