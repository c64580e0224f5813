"""The stereo map points a key frame is born with, made on the device map (orbm_map_stereo_points: k_map_stereo_select + k_map_stereo_write): the second
half of Tracking::CreateNewKeyFrame (src/Tracking.cc:3868-3960, mode 0) and the loop of Tracking::UpdateLastFrame (:3264-3341, mode 1).

Everything is bit equality.  The checker is tests/cpp/ref_stereo_points_driver.cpp, compiled here with the flags of oracle/Makefile's libref_mappoint.so
rule and linked against that library, which holds the reference's own Frame.cc and MapPoint.cc: Frame::UnprojectStereo, both MapPoint constructors,
AddObservation, ComputeDistinctiveDescriptors and UpdateNormalAndDepth are the reference's, compiled in place.  THE SELECTION LOOP ITSELF IS A
RESTATEMENT of Tracking.cc in that driver (Tracking.cc cannot be built here); each statement names the line it follows.

The device box has no reference tree, so the driver's inputs and outputs are recorded in tests/golden/stereo_points.npz (data only):
test_fixture_is_what_the_reference_gives_today regenerates them where the tree exists and requires the committed file to hold exactly that; the
emulator and device tests read the file.  The frames are 376x240 corner fields at 700 features (and a blank image); the generator takes their keypoints
from the CPU oracle, the tests from the library, and the fixture's hash of the keypoints says at once if the two ever differ.  A depth image puts a
CHOSEN depth under each keypoint; keypoints of different levels may share a pixel, so depths are chosen per pixel and every count below is asserted
on what the reference then reports.

A component of Pos - Ow cannot be -0.0 itself: Pos = (mRwc * x3Dc) + mOw, and a sum is -0 only if both terms are -0, in which case the difference
(-0) - (-0) is +0.  What CAN be -0 is a component of the normal, when the quotient underflows: the `minus_zero` call looks through a camera with
invfx = 2^-149 at features a quarter pixel left of cx, so x = -2^-149, and x / |Pos - Ow| rounds to -0 in mode 1 and is turned into +0 by the
`0 + ..` of mode 0.  Both are pinned on the reference's own statements.

"The map on another device" is not reachable on a one-device box and is left to the check all orbm_map_* calls share (tests/test_local_map_build.py)."""
import ctypes as C
import gc
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, OrbxError, synth
from orb_slam3_detailed_comments_amd import matcher as M

FIXTURE = os.path.join(ol.ROOT, "tests", "golden", "stereo_points.npz")
DRIVER = os.path.join(ol.ROOT, "tests", "cpp", "ref_stereo_points_driver.cpp")
REFERENCE = "/root/reference"
E_ARG, E_CAPACITY = -2, -4
W, H, NFEAT = 376, 240, 700
TH, MAXP = np.float32(3.5), 100
TH_UP = np.nextafter(TH, np.float32(np.inf))
SLOTS, ROWS, ROW_CAP = 4096, 6, 1024
f32 = np.float32
# a pinhole camera as Frame holds it (cx, cy, invfx, invfy), and a pose that is no special case
CAM = (f32(187.3), f32(120.9), f32(1.0) / f32(290.0), f32(1.0) / f32(288.5))
Q_GEN = np.array([0.9, 0.1, -0.3, 0.2], np.float64)
POSE_GEN = ((Q_GEN / np.linalg.norm(Q_GEN)).astype(f32), np.array([0.3, -1.2, 0.7], f32))
POSE_ID = (np.array([1, 0, 0, 0], f32), np.zeros(3, f32))
CALLS = ("few_far", "count_100_101", "count_103_th_equal", "th_next_many_close", "equal_runs_keeps", "minus_zero", "empty")


def _images():
    return np.stack([synth.corner_field(W, H, seed=71, nrect=800), synth.corner_field(W, H, seed=72, nrect=800), np.full((H, W), 90, np.uint8)])


def _key_hash(kps):
    return hashlib.sha1(np.ascontiguousarray(kps["x"]).tobytes() + np.ascontiguousarray(kps["y"]).tobytes() + np.ascontiguousarray(kps["octave"]).tobytes()).hexdigest()


# ---- the scenarios: a depth per PIXEL (so per group of keypoints that share it), by plan -----------------------------------------------------------
def _groups(kps, rng):
    px = {}
    for i in range(len(kps)):
        px.setdefault((int(kps["x"][i]), int(kps["y"][i])), []).append(i)
    keys = sorted(px)
    return [px[keys[j]] for j in rng.permutation(len(keys))]


def _assign(kps, rng, plan, rest=0.0):
    """plan: (count, depths) in turn - `count` KEYPOINTS get the values of `depths` (a callable count -> array, one value per pixel group).  The
    keypoints the plan leaves over get `rest` (a value, or a callable)."""
    depth = np.zeros(len(kps), f32)
    groups = _groups(kps, rng)
    used = [False] * len(groups)
    for count, depths in plan:
        vals = iter(np.asarray(depths(count), f32))
        left = count
        for g, members in enumerate(groups):
            if left == 0:
                break
            if used[g] or len(members) > left:
                continue
            v = next(vals)
            used[g] = True
            for i in members:
                depth[i] = v
            left -= len(members)
        assert left == 0, "the plan asks for more keypoints than the image has"
    for g, members in enumerate(groups):
        if not used[g]:
            v = rest(g) if callable(rest) else rest
            for i in members:
                depth[i] = v
    return depth


def _distinct(lo, hi, rng):
    return lambda n: rng.permutation(np.linspace(lo, hi, n, dtype=f32))


def _scenarios(keys):
    """{call: [frame, ..]}; frame = dict(image, depth [N], holds [N], pose).  keys: the keypoints of the three images"""
    rng = np.random.default_rng(2026)
    k0, k1 = keys[0], keys[1]
    const = lambda v: (lambda n: np.full(n, v, f32))
    none = lambda k: np.zeros(len(k), np.uint8)
    out = {}
    # 1. fewer than max_points candidates, all beyond th_depth | 6. zero and negative depths beside 50 close ones
    out["few_far"] = [dict(image=0, depth=_assign(k0, rng, [(60, _distinct(4.0, 9.0, rng))]), holds=none(k0), pose=POSE_GEN),
                      dict(image=1, depth=_assign(k1, rng, [(50, _distinct(0.5, 3.0, rng))], rest=lambda g: 0.0 if g % 2 else -1.5), holds=none(k1), pose=POSE_GEN)]
    # 2. exactly max_points and max_points + 1 beyond th_depth
    out["count_100_101"] = [dict(image=0, depth=_assign(k0, rng, [(100, _distinct(4.0, 9.0, rng))]), holds=none(k0), pose=POSE_GEN),
                            dict(image=1, depth=_assign(k1, rng, [(101, _distinct(4.0, 9.0, rng))]), holds=none(k1), pose=POSE_GEN)]
    # 2. two more than that: the entry at j = 100 ends the loop | 3. 100 close, then th_depth itself (no stop), then the next float up (stop), then more
    out["count_103_th_equal"] = [dict(image=0, depth=_assign(k0, rng, [(103, _distinct(4.0, 9.0, rng))]), holds=none(k0), pose=POSE_GEN),
                                 dict(image=1, depth=_assign(k1, rng, [(100, _distinct(0.5, 3.0, rng)), (1, const(TH)), (1, const(TH_UP)), (20, _distinct(5.0, 9.0, rng))]),
                                      holds=none(k1), pose=POSE_GEN)]
    # 3. the next float up directly at j = 100 | 4. 250 close points, then 30 far ones: the first of them is processed and ends the loop
    out["th_next_many_close"] = [dict(image=0, depth=_assign(k0, rng, [(100, _distinct(0.5, 3.0, rng)), (1, const(TH_UP)), (20, _distinct(5.0, 9.0, rng))]), holds=none(k0), pose=POSE_GEN),
                                 dict(image=1, depth=_assign(k1, rng, [(250, _distinct(0.5, 3.4, rng)), (30, _distinct(4.0, 9.0, rng))]), holds=none(k1), pose=POSE_GEN)]
    # 5. a run of 12 equal far depths over the stop position, keeps alternating | 7. holds of every kind on every feature, 250 close + 30 far
    d5 = _assign(k0, rng, [(95, _distinct(0.5, 3.0, rng)), (12, const(6.25)), (10, _distinct(7.0, 9.0, rng))])
    h5 = none(k0); run = np.flatnonzero(d5 == f32(6.25)); h5[run[::2]] = 1
    d7 = _assign(k1, rng, [(250, _distinct(0.5, 3.4, rng)), (30, _distinct(4.0, 9.0, rng))])
    out["equal_runs_keeps"] = [dict(image=0, depth=d5, holds=h5, pose=POSE_GEN),
                               dict(image=1, depth=d7, holds=rng.integers(0, 3, len(k1)).astype(np.uint8), pose=POSE_GEN)]
    # 8. identity pose, cx a quarter pixel right of a column of level-0 keypoints, depth 4 everywhere (cam is replaced by _cam_minus_zero for this call)
    out["minus_zero"] = [dict(image=0, depth=_assign(k0, rng, [(120, const(4.0))]), holds=none(k0), pose=POSE_ID),
                         dict(image=1, depth=_assign(k1, rng, [(80, _distinct(0.5, 3.0, rng))]), holds=none(k1), pose=POSE_GEN)]
    # 11. no feature at a positive depth, and a frame without keypoints, beside a normal frame
    out["empty"] = [dict(image=0, depth=_assign(k0, rng, [(130, _distinct(0.5, 6.0, rng))]), holds=rng.integers(0, 2, len(k0)).astype(np.uint8), pose=POSE_GEN),
                    dict(image=1, depth=_assign(k1, rng, [], rest=lambda g: 0.0 if g % 3 else -2.0), holds=none(k1), pose=POSE_GEN),
                    dict(image=2, depth=np.zeros(len(keys[2]), f32), holds=none(keys[2]), pose=POSE_GEN)]
    return out


def _cam_of(call, keys, frames):
    if call != "minus_zero":
        return np.array(CAM, f32)
    # cx a quarter pixel right of the column that holds most level-0 keypoints at a positive depth; invfx the smallest denormal
    k, d = keys[0], frames[0]["depth"]
    cols = k["x"][(k["octave"] == 0) & (d > 0)]
    vals, cnt = np.unique(cols, return_counts=True)
    return np.array([f32(vals[np.argmax(cnt)]) + f32(0.25), CAM[1], np.float32(2.0 ** -149), CAM[3]], f32)


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
_DRIVER_LIB, _DRIVER_TMP = [], []


def _driver():
    """tests/cpp/ref_stereo_points_driver.cpp over the reference's headers, linked against oracle/_ref/libref_mappoint.so; None without the reference tree"""
    if _DRIVER_LIB:
        return _DRIVER_LIB[0]
    lib = None
    if os.path.isdir(os.path.join(REFERENCE, "src")) and ol.reference_mappoint_lib() is not None:
        tmp = tempfile.TemporaryDirectory(prefix="ref_stereo_points_")          # (kept in _DRIVER_TMP: removed when the interpreter ends)
        _DRIVER_TMP.append(tmp)
        so = os.path.join(tmp.name, "libref_stereo_points.so")
        o, dbow = ol.ORACLE_DIR, os.path.join(REFERENCE, "Thirdparty", "DBoW2")
        inc = ["-I" + os.path.join(o, "slam_shim"), "-I" + os.path.join(o, "opencv_shim"), "-I" + os.path.join(o, "boost_shim"), "-I" + REFERENCE, "-I" + dbow,
               "-I" + os.path.join(REFERENCE, "include"), "-I" + os.path.join(REFERENCE, "include", "CameraModels")]
        flags = ["-std=c++14", "-O3", "-march=x86-64-v2", "-ffp-contract=off", "-fPIC", "-w", "-shared"]
        ref = os.path.join(o, "_ref")
        cmd = ["g++"] + flags + inc + ["-include", os.path.join(o, "slam_shim", "mappoint_world.h"), DRIVER]
        r = subprocess.run(cmd + ["-L" + ref, "-lref_mappoint", "-Wl,-rpath," + ref, "-Wl,--no-undefined", "-lpthread", "-o", so], capture_output=True, text=True)
        if r.returncode != 0:
            # the library hides what the driver needs: the reference's two sources go into the test's own library, same flags
            src = [os.path.join(REFERENCE, "src", s) for s in ("MapPoint.cc", "Frame.cc", "ORBextractor.cc", "ORBmatcher.cc", "CameraModels/Pinhole.cpp", "CameraModels/KannalaBrandt8.cpp")]
            src += [os.path.join(dbow, s) for s in ("DBoW2/FORB.cpp", "DBoW2/BowVector.cpp", "DBoW2/FeatureVector.cpp", "DBoW2/ScoringObject.cpp", "DUtils/Random.cpp", "DUtils/Timestamp.cpp")]
            subprocess.run(cmd + [os.path.join(o, "ref_mappoint_driver.cpp")] + src + ["-lpthread", "-o", so], check=True)
        lib = C.CDLL(so)
        lib.ref_stereo_points.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 6
    _DRIVER_LIB.append(lib)
    return lib


def _reference_frame(lib, kps, desc, scale, cam, frame, mode):
    N = len(kps)
    n1 = max(N, 1)
    kx, ky, oc = np.ascontiguousarray(kps["x"], f32), np.ascontiguousarray(kps["y"], f32), np.ascontiguousarray(kps["octave"], np.int32)
    scale, cam, q, t = (np.ascontiguousarray(a, f32) for a in (scale, cam, frame["pose"][0], frame["pose"][1]))
    d = np.ascontiguousarray(desc, np.uint8).reshape(N, 32) if N else np.zeros((1, 32), np.uint8)
    Rwc = np.zeros(9, f32); Ow = np.zeros(3, f32); processed = C.c_int(0)
    feat = np.zeros(n1, np.int32); fields = np.zeros((n1, 8), np.uint32); dout = np.zeros((n1, 32), np.uint8)
    dep, holds = np.ascontiguousarray(frame["depth"], f32), np.ascontiguousarray(frame["holds"], np.uint8)
    p = lambda a: a.ctypes.data
    created = lib.ref_stereo_points(N, p(kx), p(ky), p(oc), p(dep) if N else None, p(d), len(scale), p(scale), p(cam), p(q), p(t),
                                    p(holds) if N else None, float(TH), MAXP, mode, p(Rwc), p(Ow), C.addressof(processed), p(feat), p(fields), p(dout))
    assert np.array_equal(dout[:created], d[feat[:created]]), "the reference's descriptor of a point with one observation is not its feature's row"
    return dict(Rwc=Rwc, Ow=Ow, processed=processed.value, created=created, feat=feat[:created].copy(), fields=fields[:created].copy())


def _generate():
    """the fixture's content from the CPU oracle's keypoints and the reference driver"""
    lib = _driver()
    imgs = _images()
    oe = ol.OracleExtractor(NFEAT, 1.2, 8, 20, 7)
    ext = [oe.extract(im) for im in imgs]
    keys = [e[1] for e in ext]
    scale = np.ascontiguousarray(oe.tables()[2][0], f32)              # mvScaleFactor as ORBextractor builds it (src/ORBextractor.cc:478-483)
    assert scale[0] == 1.0 and abs(float(scale[1]) - 1.2) < 1e-6
    out = {"scale": scale}
    for b in range(len(imgs)):
        out["keyhash_%d" % b] = np.frombuffer(_key_hash(keys[b]).encode(), np.uint8)
        out["n_%d" % b] = np.array([len(keys[b])], np.int32)
    sc = _scenarios(keys)
    for call in CALLS:
        frames = sc[call]
        cam = _cam_of(call, keys, frames)
        out["%s/cam" % call] = cam
        out["%s/images" % call] = np.array([f["image"] for f in frames], np.int32)
        for k, f in enumerate(frames):
            b = f["image"]
            pre = "%s/%d/" % (call, k)
            out[pre + "depth"], out[pre + "holds"] = f["depth"], f["holds"]
            out[pre + "q"], out[pre + "t"] = f["pose"]
            for mode in (0, 1):
                r = _reference_frame(lib, keys[b], ext[b][2], scale, cam, f, mode)
                for name in ("Rwc", "Ow", "feat", "fields"):
                    out[pre + "m%d/%s" % (mode, name)] = r[name]
                out[pre + "m%d/counts" % mode] = np.array([r["created"], r["processed"]], np.int32)
    return out


_FIX = []


def fixture():
    if not _FIX:
        z = np.load(FIXTURE)
        _FIX.append({k: z[k] for k in z.files})
    return _FIX[0]


def test_fixture_is_what_the_reference_gives_today():
    """where the reference tree is present, tests/golden/stereo_points.npz holds exactly what the driver computes now"""
    if _driver() is None:
        assert os.path.exists(FIXTURE)                 # (the device box: the fixture is all there is)
        return
    fresh, have = _generate(), fixture()
    assert sorted(fresh) == sorted(have)
    for k in fresh:
        assert fresh[k].dtype == have[k].dtype and fresh[k].shape == have[k].shape and fresh[k].tobytes() == have[k].tobytes(), k


def test_fixture_holds_the_cases_it_is_meant_to():
    """what each call was built for, read off the reference's own counts"""
    fx = fixture()
    cnt = lambda call, k, m=0: tuple(int(v) for v in fx["%s/%d/m%d/counts" % (call, k, m)])
    npos = lambda call, k: int((fx["%s/%d/depth" % (call, k)] > 0).sum())
    for call in CALLS:
        for k in range(len(fx["%s/images" % call])):
            assert cnt(call, k, 0) == cnt(call, k, 1)
            assert fx["%s/%d/m0/feat" % (call, k)].tobytes() == fx["%s/%d/m1/feat" % (call, k)].tobytes()
    assert cnt("few_far", 0) == (60, 60) and npos("few_far", 0) == 60                                  # 1. the whole list
    assert cnt("few_far", 1) == (50, 50) and (fx["few_far/1/depth"] == 0).any() and (fx["few_far/1/depth"] < 0).any()   # 6.
    assert cnt("count_100_101", 0) == (100, 100) and cnt("count_100_101", 1) == (101, 101)                 # 2. > , not >=
    assert cnt("count_103_th_equal", 0) == (101, 101) and npos("count_103_th_equal", 0) == 103
    assert cnt("count_103_th_equal", 1) == (102, 102) and npos("count_103_th_equal", 1) == 122             # 3. th itself at j = 100 does not stop
    assert cnt("th_next_many_close", 0) == (101, 101) and npos("th_next_many_close", 0) == 121             # 3. the next float up does
    assert cnt("th_next_many_close", 1) == (251, 251) and npos("th_next_many_close", 1) == 280             # 4.
    # 5. the run of equal depths lies over the stop: entries 95 .. 100 are processed in index order, every second one keeps its point
    d, h = fx["equal_runs_keeps/0/depth"], fx["equal_runs_keeps/0/holds"]
    run = np.flatnonzero(d == f32(6.25))
    assert len(run) == 12 and cnt("equal_runs_keeps", 0)[1] == 101
    first6 = run[:6]
    assert cnt("equal_runs_keeps", 0)[0] == 95 + int((h[first6] == 0).sum()) and 0 < int((h[first6] == 1).sum()) < 6
    assert list(fx["equal_runs_keeps/0/m0/feat"][95:]) == [int(i) for i in first6 if h[i] == 0]
    # 7. kept entries are counted, not created
    c7, p7 = cnt("equal_runs_keeps", 1)
    assert p7 == 251 and 0 < c7 < p7 and {0, 1, 2} == set(fx["equal_runs_keeps/1/holds"].tolist())
    # 8. the normal's -0 exists in mode 1 and is +0 in mode 0; nothing else differs between the modes anywhere
    f0, f1 = fx["minus_zero/0/m0/fields"], fx["minus_zero/0/m1/fields"]
    neg = f1[:, 3] == 0x80000000
    assert neg.any() and (f0[neg, 3] == 0).all()
    for call in CALLS:
        for k in range(len(fx["%s/images" % call])):
            a, b = fx["%s/%d/m0/fields" % (call, k)], fx["%s/%d/m1/fields" % (call, k)]
            diff = a != b
            assert not diff[:, [0, 1, 2, 6, 7]].any() and (b[diff] == 0x80000000).all() and (a[diff] == 0).all()
    assert cnt("empty", 1) == (0, 0) and cnt("empty", 2) == (0, 0) and cnt("empty", 0)[0] > 0 and int(fx["n_2"][0]) == 0       # 11.


# ---- the library -------------------------------------------------------------------------------------------------------------------------------
_SCENES = {}


class _Scene:
    """one extraction of the three images per library, its keypoints and descriptor rows, and a map"""

    def __init__(self, lib):
        fx = fixture()
        self.lib, self.ex = lib, ORBextractor(NFEAT, 1.2, 8, 20, 7, lib=lib)
        self.extract()
        for b in range(3):
            assert _key_hash(self.keys[b]) == bytes(fx["keyhash_%d" % b]).decode(), "image %d: the library's keypoints are not the oracle's the fixture was made from" % b
        assert np.array_equal(np.asarray(self.ex.GetScaleFactors(), f32), fx["scale"])

    def extract(self):
        res = self.ex.extract_batch(_images())
        self.keys = [r[1] for r in res]; self.desc = [np.ascontiguousarray(r[2], np.uint8).reshape(-1, 32) for r in res]

    def set_depth(self, call, images=None):
        fx = fixture()
        img = np.zeros((3, H, W), f32)
        for k, b in enumerate(fx["%s/images" % call]):
            kp, d = self.keys[b], fx["%s/%d/depth" % (call, k)]
            img[b, kp["y"].astype(np.int64), kp["x"].astype(np.int64)] = d
        M.ComputeStereoFromRGBD(self.ex, img if images is None else img[:images], 40.0)

    def frames(self, call, mode, free, rows=None, keeps=True):
        fx = fixture()
        out = []
        for k, b in enumerate(fx["%s/images" % call]):
            pre = "%s/%d/" % (call, k)
            holds = fx[pre + "holds"]
            out.append(dict(frame=int(b), Rwc=fx[pre + "m%d/Rwc" % mode], Ow=fx[pre + "m%d/Ow" % mode], free_slots=free[k],
                            keeps=(holds == 1).astype(np.uint8) if keeps and holds.any() else None, row=-1 if rows is None else rows[k]))
        return out


def _scene(lib):
    if id(lib) not in _SCENES:
        _SCENES[id(lib)] = _Scene(lib)
    return _SCENES[id(lib)]


def _free_lists(call, seed, base=0):
    """deliberately unsorted free slots, as many as the image has features, disjoint between the frames"""
    fx = fixture()
    rng = np.random.default_rng(seed)
    out, at = [], base
    for b in fx["%s/images" % call]:
        n = int(fx["n_%d" % b][0])
        out.append((at + rng.permutation(n + 8)).astype(np.int32))
        at += n + 8
    return out


def _stored(S, mp, slots):
    """the five fields at `slots` as the searches would read them: [n][8] bits and [n][32] descriptor bytes"""
    if len(slots) == 0:
        return np.zeros((0, 8), np.uint32), np.zeros((0, 32), np.uint8)
    mp.select(0, slots)
    pos, normal, mn, mx, desc = M.PointsFetch(S.ex, mp.set(0))
    return np.concatenate([pos, normal, mn[:, None], mx[:, None]], axis=1).astype(f32).view(np.uint32), desc


def _check_call(lib, call):
    """both modes of one call of the fixture: counts, features, slots and the stored fields, bit for bit"""
    S, fx = _scene(lib), fixture()
    S.set_depth(call)
    for mode in (1, 0):
        mp = M.ResidentMap(S.ex, SLOTS, ROWS, ROW_CAP, 2)
        free = _free_lists(call, 5 + mode)
        created, processed, feat, slot = mp.stereo_points(S.frames(call, mode, free), fx["%s/cam" % call], TH, MAXP, mode)
        for k, b in enumerate(fx["%s/images" % call]):
            pre = "%s/%d/m%d/" % (call, k, mode)
            c, p = (int(v) for v in fx[pre + "counts"])
            assert (int(created[k]), int(processed[k])) == (c, p), "%s frame %d mode %d: created, processed = %d, %d, the reference %d, %d" % (call, k, mode, created[k], processed[k], c, p)
            assert np.array_equal(feat[k, :c], fx[pre + "feat"]) and np.array_equal(slot[k, :c], free[k][:c]), "%s frame %d mode %d: features / slots" % (call, k, mode)
            bits, desc = _stored(S, mp, slot[k, :c])
            assert bits.tobytes() == fx[pre + "fields"].tobytes(), "%s frame %d mode %d: stored fields differ from the reference at point %s" % (
                call, k, mode, np.flatnonzero((bits != fx[pre + "fields"]).any(axis=1))[:5])
            assert np.array_equal(desc, S.desc[b][fx[pre + "feat"]]), "%s frame %d mode %d: descriptors" % (call, k, mode)
        mp.close()


def _case_few_far(lib):
    _check_call(lib, "few_far")


def _case_count_boundary(lib):
    _check_call(lib, "count_100_101")
    _check_call(lib, "count_103_th_equal")


def _case_th_boundary(lib):
    _check_call(lib, "count_103_th_equal")
    _check_call(lib, "th_next_many_close")


def _case_many_close(lib):
    _check_call(lib, "th_next_many_close")


def _case_equal_runs_and_keeps(lib):
    _check_call(lib, "equal_runs_keeps")


def _case_modes_and_minus_zero(lib):
    _check_call(lib, "minus_zero")


def _case_empty_frames(lib):
    _check_call(lib, "empty")


def _case_store_and_rows(lib):
    """9. what the call leaves in the store and the rows, and what it leaves alone"""
    S, fx = _scene(lib), fixture()
    call, mode = "equal_runs_keeps", 0
    S.set_depth(call)
    mp = M.ResidentMap(S.ex, SLOTS, ROWS, ROW_CAP, 3)
    rng = np.random.default_rng(9)
    free = _free_lists(call, 3, base=600)
    # the points the frames keep live in slots 0 .. 599 (a guard band around them is written too); their rows hold them at the keeping features
    guard = np.arange(0, 600, dtype=np.int32)
    g = dict(pos=rng.normal(size=(600, 3)).astype(f32), normal=rng.normal(size=(600, 3)).astype(f32), mn=rng.uniform(1, 2, 600).astype(f32), mx=rng.uniform(3, 4, 600).astype(f32),
             desc=rng.integers(0, 256, (600, 32), dtype=np.uint8))
    mp.update(guard, g["pos"], g["normal"], g["mn"], g["mx"], g["desc"])
    rows_before = []
    at = 0
    for k, b in enumerate(fx["%s/images" % call]):
        holds = fx["%s/%d/holds" % (call, k)]
        row = np.full(len(holds), -1, np.int32)
        keep = np.flatnonzero(holds == 1)
        row[keep] = at + np.arange(len(keep)); at += len(keep)
        rows_before.append(row)
    assert at <= 600
    mp.set_keyframe(1, rows_before[0])                                   # frame 0's row exists; frame 1's row 4 was never set
    before = _stored(S, mp, guard)
    created, processed, feat, slot = mp.stereo_points(S.frames(call, mode, free, rows=[1, 4]), fx["%s/cam" % call], TH, MAXP, mode)
    after = _stored(S, mp, guard)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes(), "slots the call was not given have changed"
    for k, b in enumerate(fx["%s/images" % call]):
        c = int(created[k])
        bits, desc = _stored(S, mp, slot[k, :c])
        assert bits.tobytes() == fx["%s/%d/m%d/fields" % (call, k, mode)].tobytes() and np.array_equal(desc, S.desc[b][feat[k, :c]])
        # the free slots the frame did not use stay absent: a set cannot be selected over them
        for s in (free[k][c], free[k][-1]):
            with pytest.raises(OrbxError):
                mp.select(2, np.array([s], np.int32))
    # Tracking::UpdateLocalPoints over each written row: the kept and the new points in feature order, nothing else
    M_out = mp.local_points([[1], [4]])
    for k, b in enumerate(fx["%s/images" % call]):
        exp = rows_before[k].copy() if k == 0 else np.full(len(rows_before[k]), -1, np.int32)
        exp[feat[k, :created[k]]] = slot[k, :created[k]]
        exp = exp[exp >= 0]
        got = mp.fetch(k)[0]
        assert int(M_out[k]) == len(exp) and np.array_equal(got, exp), "row of frame %d" % k
    mp.close()


def _refused(mp, code, *args, **kw):
    with pytest.raises(OrbxError) as e:
        mp.stereo_points(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return e.value


def _case_refusals(lib):
    """10. every refusal leaves the store as it was; ORBX_E_CAPACITY still reports created / processed"""
    S, fx = _scene(lib), fixture()
    call, mode = "few_far", 1
    cam = fx["%s/cam" % call]
    free = _free_lists(call, 1)
    mp = M.ResidentMap(S.ex, SLOTS, ROWS, ROW_CAP, 2)
    L = lib.L
    S.set_depth(call)
    F = lambda **kw: S.frames(call, mode, kw.pop("free", free), **kw)
    exp = [int(fx["%s/%d/m%d/counts" % (call, k, mode)][0]) for k in range(2)]

    def untouched():
        for k in range(2):
            with pytest.raises(OrbxError):
                mp.select(0, free[k][:1])

    # plain arguments
    tab = (M._StereoPointsFrame * 2)()
    c6 = np.zeros(6, f32); c6[:4] = cam
    cr = np.zeros(2, np.int32); pr = np.zeros(2, np.int32); ft = np.zeros((2, 64), np.int32); sl = np.zeros((2, 64), np.int32)
    p = lambda a: a.ctypes.data
    raw = lambda B=2, frames=tab, cam_=p(c6), maxp=MAXP, mode_=1, created=p(cr), processed=p(pr), cap=64, feat=p(ft), slot=p(sl): L.orbm_map_stereo_points(
        S.ex._h, mp._m, B, frames, cam_, float(TH), maxp, mode_, created, processed, cap, feat, slot)
    assert raw(B=0) == 0 and raw(B=0, frames=None, cam_=None) == 0
    for bad in (dict(B=-1), dict(maxp=-1), dict(cap=-1), dict(mode_=2), dict(mode_=-1), dict(frames=None), dict(cam_=None), dict(created=None), dict(processed=None),
                dict(feat=None), dict(slot=None)):
        assert raw(**bad) == E_ARG, bad
    assert L.orbm_map_stereo_points(None, mp._m, 2, tab, p(c6), float(TH), MAXP, 1, p(cr), p(pr), 64, p(ft), p(sl)) == E_ARG
    assert L.orbm_map_stereo_points(S.ex._h, None, 2, tab, p(c6), float(TH), MAXP, 1, p(cr), p(pr), 64, p(ft), p(sl)) == E_ARG
    # the frames
    fr = F(); fr[1]["frame"] = 3
    assert "frame 1" in str(_refused(mp, E_ARG, fr, cam, TH, MAXP, mode))
    fr = F(); fr[0]["frame"] = -1
    _refused(mp, E_ARG, fr, cam, TH, MAXP, mode)
    fr = F(rows=[0, ROWS]); assert "frame 1" in str(_refused(mp, E_ARG, fr, cam, TH, MAXP, mode))
    fr = F(rows=[-2, 0]); _refused(mp, E_ARG, fr, cam, TH, MAXP, mode)
    fr = F(rows=[2, 2]); assert "row 2" in str(_refused(mp, E_ARG, fr, cam, TH, MAXP, mode))
    bad = [free[0].copy(), free[1].copy()]; bad[1][5] = SLOTS
    assert "frame 1" in str(_refused(mp, E_ARG, F(free=bad), cam, TH, MAXP, mode))
    bad = [free[0].copy(), free[1].copy()]; bad[0][7] = -1
    _refused(mp, E_ARG, F(free=bad), cam, TH, MAXP, mode)
    bad = [free[0].copy(), free[1].copy()]; bad[1][3] = bad[0][9]                    # the same slot in two frames of the call
    assert "twice" in str(_refused(mp, E_ARG, F(free=bad), cam, TH, MAXP, mode))
    bad = [free[0].copy(), free[1].copy()]; bad[0][3] = bad[0][9]
    _refused(mp, E_ARG, F(free=bad), cam, TH, MAXP, mode)
    small = M.ResidentMap(S.ex, SLOTS, 2, 16, 1)                                     # an image with more features than the map's rows hold
    assert "frame 0" in str(_refused(small, E_ARG, F(rows=[0, -1]), cam, TH, MAXP, mode))
    small.close()
    untouched()
    # ORBX_E_CAPACITY: too few free slots, cap too small - nothing is written, the counts are reported
    short = [free[0][:exp[0] - 1], free[1]]
    e = _refused(mp, E_CAPACITY, F(free=short), cam, TH, MAXP, mode)
    assert "frame 0" in str(e) and list(e.created) == exp and list(e.processed) == exp
    e = _refused(mp, E_CAPACITY, F(), cam, TH, MAXP, mode, cap=exp[1] - 1)
    assert list(e.created) == exp
    untouched()
    # the same arguments with room go through (the refusals above were the arguments', not the state's)
    created = mp.stereo_points(F(), cam, TH, MAXP, mode, cap=max(exp))[0]
    assert list(created) == exp
    mp.close()
    # no depth results: on a new extraction, and for an image the depth producer did not cover
    mp = M.ResidentMap(S.ex, SLOTS, ROWS, ROW_CAP, 2)
    S.extract()
    assert "frame 0" in str(_refused(mp, E_ARG, F(), cam, TH, MAXP, mode))
    S.set_depth(call, images=1)
    assert "frame 1" in str(_refused(mp, E_ARG, F(), cam, TH, MAXP, mode))
    # depths left by the fisheye stereo matcher (a rig frame: out of scope) are not read as mvDepth
    S.set_depth(call)
    kb8 = (190.9, 190.9, 188.0, 120.0, 0.003, 0.0007, -0.0002, 0.0002)
    M.ComputeStereoFishEyeMatches(S.ex, S.ex, kb8, kb8, np.eye(3), (0.1, 0.0, 0.0), 0, 1, 1)
    assert "frame 0" in str(_refused(mp, E_ARG, F(), cam, TH, MAXP, mode))
    # orbx_set_undistort since the extraction
    S.set_depth(call)
    S.ex.set_undistort((300.0, 300.0, W / 2.0, H / 2.0), (-0.2, 0.05, 0.0, 0.0, 0.0))
    assert "undistort" in str(_refused(mp, E_ARG, F(), cam, TH, MAXP, mode))
    S.ex.set_undistort(None, None)
    untouched()
    # nothing extracted yet
    ex2 = ORBextractor(NFEAT, 1.2, 8, 20, 7, lib=lib)
    with pytest.raises(OrbxError) as e2:
        mp.stereo_points(F(), cam, TH, MAXP, mode, ext=ex2)
    assert e2.value.code == E_ARG
    ex2.close()
    mp.close()
    S.extract()                                                                       # (the scene other tests share: a valid extraction again)


def _live(lib):
    gc.collect()
    a = (C.c_longlong * 4)()
    lib.check(lib.L.orbx_debug_live_resources(a))
    return tuple(a)


def _case_lifetime(lib):
    """12. create, call, destroy: the library holds what it held before"""
    _scene(lib)                                                       # (the shared scene exists before the count is taken)
    fx = fixture()
    start = _live(lib)
    ex = ORBextractor(NFEAT, 1.2, 8, 20, 7, lib=lib)
    S = _Scene.__new__(_Scene); S.lib, S.ex = lib, ex
    S.extract()
    S.set_depth("empty")
    mp = M.ResidentMap(ex, SLOTS, ROWS, ROW_CAP, 2)
    free = _free_lists("empty", 4)
    created = mp.stereo_points(S.frames("empty", 0, free, rows=[0, 1, 2]), fx["empty/cam"], TH, MAXP, 0)[0]
    assert int(created[0]) == int(fx["empty/0/m0/counts"][0])
    with pytest.raises(OrbxError):
        mp.stereo_points(S.frames("empty", 0, [f[:1] for f in free]), fx["empty/cam"], TH, MAXP, 0)
    mp.close(); ex.close()
    assert _live(lib) == start


def test_more_candidates_than_the_lds_sort_holds_is_refused(request, monkeypatch):
    """The third ORBX_E_CAPACITY: with the emulator told that a workgroup has 3 KB of LDS (ORBX_EMU_LDS_LIMIT) the sort holds 256 keys, and the frame with
    280 features at a positive depth reports created = -1, processed = 280; nothing is written.  (The device's own bound, 16 384 keys, needs an image
    with more than 16 384 features at a positive depth: not run there.)"""
    lib = request.getfixturevalue("emu_lib")
    S, fx = _scene(lib), fixture()
    call = "th_next_many_close"
    S.set_depth(call)
    mp = M.ResidentMap(S.ex, SLOTS, ROWS, ROW_CAP, 1)
    free = _free_lists(call, 2)
    monkeypatch.setenv("ORBX_EMU_LDS_LIMIT", "3072")
    e = _refused(mp, E_CAPACITY, S.frames(call, 1, free), fx["%s/cam" % call], TH, MAXP, 1)
    assert "frame 1" in str(e) and list(e.created) == [101, -1] and list(e.processed) == [101, 280]
    for k in range(2):
        with pytest.raises(OrbxError):
            mp.select(0, free[k][:1])
    monkeypatch.delenv("ORBX_EMU_LDS_LIMIT")
    assert list(mp.stereo_points(S.frames(call, 1, free), fx["%s/cam" % call], TH, MAXP, 1)[0]) == [101, 251]
    mp.close()


def test_stereo_points_frame_mirror_has_the_header_layout(tmp_path):
    """OrbmStereoPointsFrame of include/orbx.h against its ctypes mirror: same fields, offsets and sizes"""
    fields = [f[0] for f in M._StereoPointsFrame._fields_]
    assert fields == ["frame", "Rwc", "Ow", "keeps", "free_slots", "nfree", "row"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "orbx.h"', 'int main(void) {', 'printf("%zu\\n", sizeof(OrbmStereoPointsFrame));']
    lines += ['printf("%%zu %%zu\\n", offsetof(OrbmStereoPointsFrame, %s), sizeof(((OrbmStereoPointsFrame*)0)->%s));' % (f, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ol.ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(M._StereoPointsFrame)
    for k, f in enumerate(fields):
        d = getattr(M._StereoPointsFrame, f)
        assert (d.offset, d.size) == (int(out[1 + 2 * k]), int(out[2 + 2 * k])), f


# ---- each case on the emulator and on the device -------------------------------------------------------------------------------------------------
def test_fewer_than_max_points_and_nonpositive_depths_emulated(emu_lib):
    """1. fewer than max_points candidates, all beyond th_depth: the whole list; 6. depths 0 and below are no candidates"""
    _case_few_far(emu_lib)


@pytest.mark.gpu
def test_fewer_than_max_points_and_nonpositive_depths_gpu(hip_lib):
    _case_few_far(hip_lib)


def test_stop_comes_after_max_points_emulated(emu_lib):
    """2. 100, 101 and 103 candidates beyond th_depth: the loop ends at nPoints > 100, not >="""
    _case_count_boundary(emu_lib)


@pytest.mark.gpu
def test_stop_comes_after_max_points_gpu(hip_lib):
    _case_count_boundary(hip_lib)


def test_depth_equal_to_th_depth_does_not_stop_emulated(emu_lib):
    """3. th_depth itself at j = 100 goes on, the next float up ends the loop"""
    _case_th_boundary(emu_lib)


@pytest.mark.gpu
def test_depth_equal_to_th_depth_does_not_stop_gpu(hip_lib):
    _case_th_boundary(hip_lib)


def test_many_close_points_emulated(emu_lib):
    """4. 250 close points are all processed; the first far one behind them is processed and ends the loop"""
    _case_many_close(emu_lib)


@pytest.mark.gpu
def test_many_close_points_gpu(hip_lib):
    _case_many_close(hip_lib)


def test_equal_depths_keeps_and_slot_order_emulated(emu_lib):
    """5. equal depths over the stop position are ordered by index; 7. kept entries are counted and not created, the rest take the unsorted free slots in order"""
    _case_equal_runs_and_keeps(emu_lib)


@pytest.mark.gpu
def test_equal_depths_keeps_and_slot_order_gpu(hip_lib):
    _case_equal_runs_and_keeps(hip_lib)


def test_both_modes_and_the_minus_zero_normal_emulated(emu_lib):
    """8. mode 0 and mode 1 on the same inputs, each against its own reference path, with a normal component that is -0 in mode 1 and +0 in mode 0"""
    _case_modes_and_minus_zero(emu_lib)


@pytest.mark.gpu
def test_both_modes_and_the_minus_zero_normal_gpu(hip_lib):
    _case_modes_and_minus_zero(hip_lib)


def test_store_and_rows_after_the_call_emulated(emu_lib):
    _case_store_and_rows(emu_lib)


@pytest.mark.gpu
def test_store_and_rows_after_the_call_gpu(hip_lib):
    _case_store_and_rows(hip_lib)


def test_refusals_leave_the_store_untouched_emulated(emu_lib):
    _case_refusals(emu_lib)


@pytest.mark.gpu
def test_refusals_leave_the_store_untouched_gpu(hip_lib):
    _case_refusals(hip_lib)


def test_empty_frames_in_a_batch_emulated(emu_lib):
    """11. a frame with no feature at a positive depth and a frame without keypoints beside a normal frame"""
    _case_empty_frames(emu_lib)


@pytest.mark.gpu
def test_empty_frames_in_a_batch_gpu(hip_lib):
    _case_empty_frames(hip_lib)


def test_lifetime_emulated(emu_lib):
    _case_lifetime(emu_lib)


@pytest.mark.gpu
def test_lifetime_gpu(hip_lib):
    _case_lifetime(hip_lib)
