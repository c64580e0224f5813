"""orbx_fetch beside a queued matcher.

After a large batch (more than ORBX_QT_WIDE_BATCH = 32 images) the extraction sends its counts to the host and records ev_done directly behind
k_orient_brief, and orbx_fetch downloads records and descriptors on the handle's second stream while the kernels the caller queued on the first
one (k_stereo_match) are still running; small batches and replayed graphs download on the first stream behind everything (csrc/orbx_api.cpp).
Whatever the order of the calls, the bytes are the same and equal the oracle's.  The tests run at 2 stereo pairs (4 images: the small forms) and at
17 or 33 pairs (34 / 33 images per handle: the large forms), 376 x 240 pixels, 300 features, on the CPU build of the kernels and - the `gpu` twins -
on the device.  The emulator's streams are synchronous, so there the large size only walks the host code of the large forms, and only where that
takes one or two extractions (a 34-image batch is seconds of emulation); the device runs every test at both sizes.
"""
import math

import numpy as np
import pytest

import oracle_lib as ol
from cases import EUROC_BF, EUROC_B
from orb_slam3_detailed_comments_amd import ORBextractor, KP_DTYPE, synth, _lib

W, H, NF = 376, 240, 300
NSCENES = 3


@pytest.fixture(scope="module")
def scenes():
    """three stereo pairs and what the oracle makes of each: ((mono, keys, desc) left, (...) right, uRight, depth, matches)"""
    out = []
    for s in range(NSCENES):
        l, r = synth.stereo_pair(W, H, seed=4100 + s, nrect=800)
        oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
        eL, eR = oL.extract(l), oR.extract(r)
        u, z, nm = ol.oracle_stereo(oL, oR, eL[1], eL[2], eR[1], eR[2], EUROC_BF, EUROC_B)
        assert len(eL[1]) > 100 and nm > 20
        out.append(dict(l=l, r=r, L=eL, R=eR, u=u, z=z, nm=nm))
    return out


def _batch(scenes, P, first=0):
    """P pairs, lefts then rights; pair p shows scene (first + p) % NSCENES"""
    ids = [(first + p) % NSCENES for p in range(P)]
    return np.stack([scenes[i]["l"] for i in ids] + [scenes[i]["r"] for i in ids]), ids


class Out:
    """page-locked output blocks in the device layout [images][cap] (cap = orbx_max_keypoints: orbx_fetch copies straight into them)"""

    def __init__(self, h, nimg, P, cap):
        self.k = h.pinned_empty((nimg, cap), KP_DTYPE); self.d = h.pinned_empty((nimg, cap, 32), np.uint8)
        self.n = np.zeros(nimg, np.int32); self.m = np.zeros(nimg, np.int32)
        self.u = h.pinned_empty((P, cap), np.float32); self.z = h.pinned_empty((P, cap), np.float32); self.nm = np.zeros(P, np.int32)
        self.clear()

    def clear(self):
        self.k.view(np.uint8)[...] = 0xEE; self.d[...] = 0xEE; self.u[...] = -7; self.z[...] = -7
        self.n[...] = -1; self.m[...] = -1; self.nm[...] = -1


def _fetch(lib, h, o, cap, kps=True, desc=True):
    return lib.L.orbx_fetch(h._h, o.k.ctypes.data if kps else None, o.d.ctypes.data if desc else None, cap, o.n.ctypes.data, o.m.ctypes.data)


def _match(lib, L, R, P, rf):
    lib.check(lib.L.orbm_stereo_match(L._h, 0, R._h, rf, P, EUROC_BF, EUROC_B))


def _stereo_fetch(lib, h, o, P, cap):
    lib.check(lib.L.orbm_stereo_fetch(h._h, P, o.u.ctypes.data, o.z.ctypes.data, cap, o.nm.ctypes.data))


def _extraction_bytes(o, images):
    """what the extraction returned for `images`, the valid entries only (rows past an image's count are unspecified)"""
    return [(int(o.n[b]), int(o.m[b]), o.k[b, :o.n[b]].tobytes(), o.d[b, :o.n[b]].tobytes()) for b in images]


def _stereo_bytes(o, P):
    return [(int(o.nm[p]), o.u[p, :o.n[p]].tobytes(), o.z[p, :o.n[p]].tobytes()) for p in range(P)]


def _assert_oracle(o, scenes, ids, P, right_at=None, stereo=True):
    """images [0, P) are the lefts of scenes `ids`; the rights sit at [right_at, right_at + P) of the same block (None: not in it)"""
    for p, s in enumerate(ids):
        e = scenes[s]
        sides = [(p, e["L"], "left")] + ([(right_at + p, e["R"], "right")] if right_at is not None else [])
        for b, (mono, keys, desc), side in sides:
            assert o.n[b] == len(keys) and o.m[b] == mono, "pair %d %s: counts" % (p, side)
            assert o.k[b, :o.n[b]].tobytes() == keys.tobytes(), "pair %d %s: keypoints differ from the oracle" % (p, side)
            assert o.d[b, :o.n[b]].tobytes() == desc.tobytes(), "pair %d %s: descriptors differ from the oracle" % (p, side)
        if stereo:
            assert o.nm[p] == e["nm"], "pair %d: match count" % p
            assert o.u[p, :o.n[p]].tobytes() == e["u"].tobytes() and o.z[p, :o.n[p]].tobytes() == e["z"].tobytes(), "pair %d: uRight / depth differ from the oracle" % p


# ---- fetch before and after the matcher -----------------------------------------------------------------------------------------------------------

def _order(lib, scenes, P, profile=False):
    batch, ids = _batch(scenes, P)
    h = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    h.profile(profile)
    cap = None
    got = []
    for fetch_first in (True, False):
        h.enqueue(batch)
        cap = h.max_keypoints()
        o = Out(h, 2 * P, P, cap)
        if fetch_first:
            lib.check(_fetch(lib, h, o, cap)); _match(lib, h, h, P, P)
        else:
            _match(lib, h, h, P, P); lib.check(_fetch(lib, h, o, cap))
        _stereo_fetch(lib, h, o, P, cap)
        _assert_oracle(o, scenes, ids, P, right_at=P)
        got.append((_extraction_bytes(o, range(2 * P)), _stereo_bytes(o, P)))
    assert got[0] == got[1]
    ms = h.stage_ms()
    h.close()
    return ms


@pytest.mark.parametrize("P", [2, 17])
def test_fetch_before_and_after_the_matcher(emu_lib, scenes, P):
    _order(emu_lib, scenes, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 17])
def test_fetch_before_and_after_the_matcher_gpu(hip_lib, scenes, P):
    _order(hip_lib, scenes, P)


# ---- two handles: the matcher of L waits for R's ev_done ------------------------------------------------------------------------------------------

def _two_handles(lib, scenes, P):
    batch, ids = _batch(scenes, P)
    L, R = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib), ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    L.enqueue(batch[:P]); R.enqueue(batch[P:])
    cap = L.max_keypoints()
    oL, oR = Out(L, P, P, cap), Out(R, P, P, cap)
    _match(lib, L, R, P, 0)
    lib.check(_fetch(lib, R, oR, cap)); lib.check(_fetch(lib, L, oL, cap))
    _stereo_fetch(lib, L, oL, P, cap)
    _assert_oracle(oL, scenes, ids, P)
    for p, s in enumerate(ids):
        mono, keys, desc = scenes[s]["R"]
        assert oR.n[p] == len(keys) and oR.m[p] == mono and oR.k[p, :oR.n[p]].tobytes() == keys.tobytes() and oR.d[p, :oR.n[p]].tobytes() == desc.tobytes()
    # the single-handle run on the same images
    S = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    S.enqueue(batch)
    oS = Out(S, 2 * P, P, cap)
    _match(lib, S, S, P, P); lib.check(_fetch(lib, S, oS, cap)); _stereo_fetch(lib, S, oS, P, cap)
    assert _extraction_bytes(oL, range(P)) == _extraction_bytes(oS, range(P)) and _extraction_bytes(oR, range(P)) == _extraction_bytes(oS, range(P, 2 * P))
    assert _stereo_bytes(oL, P) == _stereo_bytes(oS, P)
    for x in (L, R, S):
        x.close()


@pytest.mark.parametrize("P", [2])
def test_two_handles(emu_lib, scenes, P):
    _two_handles(emu_lib, scenes, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 33])
def test_two_handles_gpu(hip_lib, scenes, P):
    _two_handles(hip_lib, scenes, P)


# ---- the staged layout (cap != orbx_max_keypoints) and the forms without records or descriptors, behind a queued matcher -------------------------------

def _staged(lib, scenes, P):
    batch, ids = _batch(scenes, P)
    h = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    h.enqueue(batch)
    tc = h.max_keypoints()
    _match(lib, h, h, P, P)
    ref = Out(h, 2 * P, P, tc)
    lib.check(_fetch(lib, h, ref, tc))
    _assert_oracle(ref, scenes, ids, P, right_at=P, stereo=False)
    want = _extraction_bytes(ref, range(2 * P))
    nmax = int(ref.n.max())
    assert nmax < tc
    for cap in (tc + 7, nmax):                                   # wider rows than the device's, and the narrowest that still hold every image
        o = Out(h, 2 * P, P, cap)
        lib.check(_fetch(lib, h, o, cap))
        assert _extraction_bytes(o, range(2 * P)) == want, "cap %d" % cap
    for kps, desc in ((False, True), (True, False), (False, False)):
        for cap in (tc, tc + 7):
            o = Out(h, 2 * P, P, cap)
            lib.check(_fetch(lib, h, o, cap, kps=kps, desc=desc))
            assert o.n.tolist() == ref.n.tolist() and o.m.tolist() == ref.m.tolist()
            for b in range(2 * P):
                n = o.n[b]
                assert (o.k[b, :n].tobytes() == ref.k[b, :n].tobytes()) if kps else bool((o.k.view(np.uint8) == 0xEE).all())
                assert (o.d[b, :n].tobytes() == ref.d[b, :n].tobytes()) if desc else bool((o.d == 0xEE).all())
    o = Out(h, 2 * P, P, nmax - 1)                               # too narrow for the fullest image: refused, the counts still reported
    assert _fetch(lib, h, o, nmax - 1) == _lib.ORBX_E_CAPACITY
    assert o.n.tolist() == ref.n.tolist() and o.m.tolist() == ref.m.tolist()
    for b in range(2 * P):
        if o.n[b] < nmax:
            assert o.k[b, :o.n[b]].tobytes() == ref.k[b, :o.n[b]].tobytes() and o.d[b, :o.n[b]].tobytes() == ref.d[b, :o.n[b]].tobytes()
    _stereo_fetch(lib, h, ref, P, tc)                            # the matcher queued in front of all these fetches
    _assert_oracle(ref, scenes, ids, P, right_at=P)
    h.close()


@pytest.mark.parametrize("P", [2, 17])
def test_staged_layout_behind_a_matcher(emu_lib, scenes, P):
    _staged(emu_lib, scenes, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 17])
def test_staged_layout_behind_a_matcher_gpu(hip_lib, scenes, P):
    _staged(hip_lib, scenes, P)


# ---- fetch twice; an extraction without a fetch in front of it; then other images -----------------------------------------------------------------------

def _twice_then_other_images(lib, scenes, P):
    batch, ids = _batch(scenes, P)
    other, ids2 = _batch(scenes, P, first=1)
    assert all(a != b for a, b in zip(ids, ids2))
    h = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    h.enqueue(batch)
    cap = h.max_keypoints()
    _match(lib, h, h, P, P)
    a, b = Out(h, 2 * P, P, cap), Out(h, 2 * P, P, cap)
    lib.check(_fetch(lib, h, a, cap)); lib.check(_fetch(lib, h, b, cap))
    assert _extraction_bytes(a, range(2 * P)) == _extraction_bytes(b, range(2 * P))
    _stereo_fetch(lib, h, a, P, cap)
    _assert_oracle(a, scenes, ids, P, right_at=P)
    # the next batch rewrites what the downloads above read: its results, and nothing of the first batch
    h.enqueue(other)
    _match(lib, h, h, P, P)
    c = Out(h, 2 * P, P, cap)
    lib.check(_fetch(lib, h, c, cap)); _stereo_fetch(lib, h, c, P, cap)
    _assert_oracle(c, scenes, ids2, P, right_at=P)
    # two extractions with no fetch between them: the fetch returns the second
    h.enqueue(other); _match(lib, h, h, P, P)
    h.enqueue(batch); _match(lib, h, h, P, P)
    d = Out(h, 2 * P, P, cap)
    lib.check(_fetch(lib, h, d, cap)); _stereo_fetch(lib, h, d, P, cap)
    _assert_oracle(d, scenes, ids, P, right_at=P)
    h.close()


@pytest.mark.parametrize("P", [2])
def test_fetch_twice_then_other_images(emu_lib, scenes, P):
    _twice_then_other_images(emu_lib, scenes, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 17])
def test_fetch_twice_then_other_images_gpu(hip_lib, scenes, P):
    _twice_then_other_images(hip_lib, scenes, P)


# ---- one image per call: graph replay, and blur + FAST in one launch (the second stream carries nothing) ----------------------------------------------------

def _single_image(lib, scenes, graph, small_forms):
    e = scenes[0]
    oL = ol.OracleExtractor(NF)
    mono, keys, desc = oL.extract(e["l"])
    u, z, nm = ol.oracle_stereo(oL, oL, keys, desc, keys, desc, EUROC_BF, EUROC_B)      # the image against itself
    h = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    h.graph_replay(graph); h.set_small_batch_forms(small_forms)
    got = []
    for rep in range(2):                                          # (the second round replays the graph the first one captured)
        for fetch_first in (True, False):
            h.enqueue(e["l"][None])
            cap = h.max_keypoints()
            o = Out(h, 1, 1, cap)
            if fetch_first:
                lib.check(_fetch(lib, h, o, cap)); _match(lib, h, h, 1, 0)
            else:
                _match(lib, h, h, 1, 0); lib.check(_fetch(lib, h, o, cap))
            _stereo_fetch(lib, h, o, 1, cap)
            assert o.n[0] == len(keys) and o.m[0] == mono and o.k[0, :o.n[0]].tobytes() == keys.tobytes() and o.d[0, :o.n[0]].tobytes() == desc.tobytes()
            assert o.nm[0] == nm and o.u[0, :o.n[0]].tobytes() == u.tobytes() and o.z[0, :o.n[0]].tobytes() == z.tobytes()
            got.append((_extraction_bytes(o, [0]), _stereo_bytes(o, 1)))
    assert all(g == got[0] for g in got)
    h.close()


@pytest.mark.parametrize("graph,small_forms", [(True, True), (True, False), (False, True), (False, False)])
def test_single_image_forms(emu_lib, scenes, graph, small_forms):
    _single_image(emu_lib, scenes, graph, small_forms)


@pytest.mark.gpu
@pytest.mark.parametrize("graph,small_forms", [(True, True), (True, False), (False, True)])
def test_single_image_forms_gpu(hip_lib, scenes, graph, small_forms):
    _single_image(hip_lib, scenes, graph, small_forms)


@pytest.mark.gpu
def test_large_batch_graph_replay_gpu(hip_lib, scenes):
    """34 images through a captured graph: ev_done is not recorded inside the capture, the fetch behind the matcher takes the first stream"""
    lib, P = hip_lib, 17
    batch, ids = _batch(scenes, P)
    h = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    h.graph_replay(True)
    p, shape, st, ist = h.input_upload(batch)
    cap = h.max_keypoints()
    for rep in range(3):                                          # capture, then two replays
        h.enqueue(None, (0, 0), device_ptr=p, shape=shape, stride=st, image_stride=ist)
        _match(lib, h, h, P, P)
        o = Out(h, 2 * P, P, cap)
        lib.check(_fetch(lib, h, o, cap)); _stereo_fetch(lib, h, o, P, cap)
        _assert_oracle(o, scenes, ids, P, right_at=P)
    h.close()


# ---- stage timers -------------------------------------------------------------------------------------------------------------------------------------------

def _timers(lib, scenes, P):
    ms = _order(lib, scenes, P, profile=True)
    assert len(ms) == _lib.NSTAGES
    for name, v in ms.items():
        assert math.isfinite(v) and v >= 0.0, "stage %s: %r" % (name, v)


@pytest.mark.parametrize("P", [2])
def test_stage_timers_after_both_fetches(emu_lib, scenes, P):
    _timers(emu_lib, scenes, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 17])
def test_stage_timers_after_both_fetches_gpu(hip_lib, scenes, P):
    _timers(hip_lib, scenes, P)
