"""k_orient_brief requests everything its prologue needs in one round trip (level layouts and counts lane-parallel, picked by shuffle), walks the
valid keypoints of a wave by the set bits of its mask with the patch loads of a group of keypoints in flight together, and loads the next
keypoint's window while this one is sampled.  What can go wrong is in the waves that are not full: a shuffle that an inactive lane skips, a
"next keypoint" that does not exist, a pitch or level that changes inside a wave.  Keypoints (angle bits included), descriptors and the zeroed
descriptor rows past the count are compared with the oracle and, where it is built, with the reference's own source, at B = 1 (k_orient_brief_small,
2 keypoints per wave) and B = 33 (k_orient_brief, 8 per wave; just past the small-batch limit of 32).

The wave shapes are asserted from the level counts the extractor reports (debug_level_keys) and the slot layout (level l owns
max(quota + 3, 4) slots from the sum of the lower levels' on; checked against max_keypoints()).  313 features put level 1 at slot 71 and level 4
at slot 223 (both 7 mod 8, and every level above 0 at an odd slot), so that
  * a dense image has a wave that straddles two levels with keypoints on both sides of the three unused slots between them (8 per wave; with 2 per
    wave a wave holds slots of two levels only where the lower one fills its last slot, which needs a level 3 over its quota: not constructed);
  * an image with one corner (one keypoint on each of the upper levels, none on the lower: levels without a keypoint) has waves whose only valid
    keypoint is the last (slot 223 of 216 .. 223; any odd first slot with 2 per wave);
  * an image with one weak pixel (one keypoint, on level 0) has a wave whose only valid keypoint is the first;
  * a flat image has no keypoint at all.
test_extremes_*: noise images at 3000 features whose keypoints reach the detectable minimum and maximum x and y (19 and size - 20 in level
coordinates) of level 0 and of the top level - the windows nearest both ends of an image's pyramid block - with the one that reaches the maxima
as the last image of the batch.
Each case runs on the SIMT emulator and, marked gpu, on the device."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import synth
from orb_slam3_detailed_comments_amd.extractor import ORBextractor

NF = 313
SIZES = {"239x239": (239, 239), "320x240": (320, 240)}


def _flat(w, h, v=60):
    return np.full((h, w), v, np.uint8)


def _one_corner(w, h):
    img = _flat(w, h)
    img[h // 2:, w // 2:] = 200
    return img


def _weak_pixel(w, h):
    img = _flat(w, h)
    img[h // 3, w // 3] = 68          # 8 grey levels: a corner at the fallback threshold on level 0, below it after the first resize
    return img


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


_expected = {}


def _expect(key, factory, nf):
    """image, oracle result, oracle level counts and reference result: computed once, shared, never changed"""
    if key not in _expected:
        img = factory()
        o = ol.OracleExtractor(nf)
        exp = o.extract(img)
        counts = [len(o.level_keypoints(l)) for l in range(8)]
        ref = ol.ReferenceExtractor(nf).extract(img) if ol.reference() is not None else None
        _expected[key] = (img, exp, counts, ref)
    return _expected[key]


def _same(a, b):
    return a[0] == b[0] and ol.kps_equal(a[1], b[1]) and a[1]["angle"].tobytes() == b[1]["angle"].tobytes() and np.array_equal(a[2], b[2])


def _layout(ex):
    quota = [int(q) for q in ex.features_per_level()]
    cap = [max(q + 3, 4) for q in quota]                       # (one quadtree root at these aspect ratios)
    off = [int(x) for x in np.concatenate([[0], np.cumsum(cap)])]
    assert off[-1] == ex.max_keypoints(), "the slot layout of this test is not the extractor's"
    return off, cap


def _wave_masks(counts, off, cap, kpw):
    """(valid bits, set of levels with a valid slot) of every wave of kpw consecutive slots"""
    total = off[-1]
    valid = np.zeros(-(-total // kpw) * kpw, bool)
    level = np.full(valid.shape, -1)
    for l, c in enumerate(counts):
        assert c <= cap[l]
        valid[off[l]:off[l] + c] = True
        level[off[l]:off[l] + cap[l]] = l
    out = []
    for w0 in range(0, len(valid), kpw):
        v = valid[w0:w0 + kpw]
        out.append((int(sum(1 << i for i in range(kpw) if v[i])), set(level[w0:w0 + kpw][v].tolist())))
    return out


def _shapes_seen(counts, off, cap, kpw):
    seen = set()
    for mask, levels in _wave_masks(counts, off, cap, kpw):
        if mask == 1:
            seen.add("only_first")
        if mask == 1 << (kpw - 1):
            seen.add("only_last")
        bits = [i for i in range(kpw) if mask >> i & 1]
        if len(levels) == 2 and len(bits) < bits[-1] - bits[0] + 1:
            seen.add("straddle_with_hole")
    if 0 in counts:
        seen.add("empty_level")
    if sum(counts) == 0:
        seen.add("no_keypoint")
    return seen


def _run(lib, nf, items, kpw):
    """one batch of the given (key, factory) items; every image against its expectations, descriptor rows past the count zero"""
    exps = [_expect(k, f, nf) for k, f in items]
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    off, cap = _layout(ex)
    res = ex.extract_batch(np.stack([e[0] for e in exps]))
    rows = ex._fetch_buf[2]                                    # the fetched descriptor block [B, cap, 32]
    seen = set()
    for b, (img, exp, counts, ref) in enumerate(exps):
        tag = "%s, batch of %d, image %d" % (items[b][0], len(items), b)
        got = [len(ex.debug_level_keys(l, b)) for l in range(8)]
        assert got == counts, tag
        assert _same(res[b], exp), tag
        if ref is not None:
            assert _same(res[b], ref), tag + " against the reference"
        assert not rows[b, len(res[b][1]):].any(), tag + ": descriptor rows past the count"
        seen |= _shapes_seen(got, off, cap, kpw)
    ex.close()
    return seen


def _shapes(lib, size):
    w, h = SIZES[size]
    dense = (size + "/dense", lambda: synth.corner_field(w, h, seed=4, nrect=600))
    corner = (size + "/one_corner", lambda: _one_corner(w, h))
    pixel = (size + "/weak_pixel", lambda: _weak_pixel(w, h))
    flat = (size + "/flat", lambda: _flat(w, h))
    counts = _expect(dense[0], dense[1], NF)[2]
    assert any(c % 2 for c in counts) and any(c % 8 for c in counts) and min(counts) > 8, counts
    # 8 keypoints per wave
    seen = _run(lib, NF, [dense, corner, pixel] + [flat] * 29 + [dense], 8)
    assert seen >= {"only_first", "only_last", "empty_level", "straddle_with_hole", "no_keypoint"}, seen
    # 2 keypoints per wave
    seen = set()
    for item in (dense, corner, pixel, flat):
        seen |= _run(lib, NF, [item], 2)
    assert seen >= {"only_first", "only_last", "empty_level", "no_keypoint"}, seen


def _extremes(lib):
    w = h = 239
    nf = 3000
    low = ("239x239/noise18", lambda: _noise(w, h, 18))
    high = ("239x239/noise34", lambda: _noise(w, h, 34))
    flat = ("239x239/flat", lambda: _flat(w, h))
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    sf = np.asarray(ex.GetScaleFactors(), np.float32)
    ex.close()

    def reached(key, factory):
        """which of (x min, x max, y min, y max) the keypoints of level 0 and of the top level reach, in level coordinates"""
        k = _expect(key, factory, nf)[1][1]
        out = {}
        for l in (0, 7):
            kl = k[k["octave"] == l]
            lw, lh = int(round(w / float(sf[l]))), int(round(h / float(sf[l])))
            x, y = np.rint(kl["x"] / sf[l]).astype(int), np.rint(kl["y"] / sf[l]).astype(int)
            out[l] = ((x == 19).any(), (x == lw - 20).any(), (y == 19).any(), (y == lh - 20).any())
        return out

    lo, hi = reached(*low), reached(*high)
    assert all(hi[0]) and hi[7][1] and hi[7][3] and hi[7][2], hi       # the last image: every extreme of level 0, both maxima of the top level
    assert lo[7][0], lo                                                # the top level's minimum x
    _run(lib, nf, [low] + [flat] * 31 + [high], 8)
    _run(lib, nf, [high], 2)


@pytest.mark.parametrize("size", sorted(SIZES))
def test_wave_shapes_emu(emu_lib, size):
    _shapes(emu_lib, size)


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(SIZES))
def test_wave_shapes_gpu(hip_lib, size):
    _shapes(hip_lib, size)


def test_extremes_emu(emu_lib):
    _extremes(emu_lib)


@pytest.mark.gpu
def test_extremes_gpu(hip_lib):
    _extremes(hip_lib)
