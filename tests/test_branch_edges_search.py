"""Directed inputs for branches of csrc/k_search.hip that random scenes do not enter (found by tools/emu_coverage.sh, profiles/emu_coverage/):

* k_grid_build with more than 4 * 1024 keypoints in a frame (the tail loops behind the four register-held keypoints of a thread), on the unordered path, in
  front of the crowded-cell path, and with keypoints whose rounded cell lies outside the grid - the frames of the monocular initialisation hold 5000-10000;
* MapPoint::PredictScale's clamps (n < 0 -> 0, n >= nlevels -> nlevels - 1) in k_frustum and k_keyframe_queries, with the distance gates
  0.8 mfMinDistance / 1.2 mfMaxDistance hit exactly, one float inside and one float outside.

Every case is compared with a sequential restatement in numpy (float32 where the reference computes in float), with the C++ restatement of oracle/ and,
where oracle/_ref is built, with the reference's own Frame.cc / ORBmatcher.cc (the large frames: SearchForInitialization through the world driver), and asserts that its input enters the branch it is written for.  The emulator
and the GPU forms use the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import matcher_world as mw
import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, synth, views
from orb_slam3_detailed_comments_amd import matcher as M
from orb_slam3_detailed_comments_amd._lib import KP_DTYPE

f32 = np.float32
GRID_COLS, GRID_ROWS = 64, 48                     # FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:44-45
KEPT = 4 * 1024                                   # keypoints k_grid_build holds in registers (kKeep * kGridThreads); the tail loops take the rest
SMALL_CELL = 16                                   # kGridSmallCell: a frame with a fuller cell takes the ordered chunk placement


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:469-504, :962-978, :859-951), restated
def _c_round(v):
    """round() of <cmath>: halves away from zero (v: float32 values, exact in float64)"""
    v = np.asarray(v, np.float64)
    return np.trunc(v + np.copysign(0.5, v)).astype(np.int64)


class RestatedGrid:
    def __init__(self, keys, w, h):
        self.k = keys
        self.gw = f32(GRID_COLS) / (f32(w) - f32(0)); self.gh = f32(GRID_ROWS) / (f32(h) - f32(0))
        px = _c_round((keys["x"] - f32(0)) * self.gw); py = _c_round((keys["y"] - f32(0)) * self.gh)
        self.inside = ~((px < 0) | (px >= GRID_COLS) | (py < 0) | (py >= GRID_ROWS))
        self.cells = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in np.flatnonzero(self.inside):
            self.cells[px[i]][py[i]].append(int(i))
        self.largest_cell = max(len(c) for col in self.cells for c in col)

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1):
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        n_min_x = max(0, int(np.floor((x - f32(0) - r) * self.gw)))
        if n_min_x >= GRID_COLS:
            return out
        n_max_x = min(GRID_COLS - 1, int(np.ceil((x - f32(0) + r) * self.gw)))
        if n_max_x < 0:
            return out
        n_min_y = max(0, int(np.floor((y - f32(0) - r) * self.gh)))
        if n_min_y >= GRID_ROWS:
            return out
        n_max_y = min(GRID_ROWS - 1, int(np.ceil((y - f32(0) + r) * self.gh)))
        if n_max_y < 0:
            return out
        check = min_level > 0 or max_level >= 0
        for ix in range(n_min_x, n_max_x + 1):
            for iy in range(n_min_y, n_max_y + 1):
                for i in self.cells[ix][iy]:
                    kp = self.k[i]
                    if check:
                        if kp["octave"] < min_level:
                            continue
                        if max_level >= 0 and kp["octave"] > max_level:
                            continue
                    if abs(f32(kp["x"]) - x) < r and abs(f32(kp["y"]) - y) < r:
                        out.append(i)
        return out


W, H = 640, 480
SCALES = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
OUTSIDE = [(-6.0, 100.0), (639.9, 200.0), (300.0, -5.5), (320.0, 479.9), (-30.0, -30.0), (700.0, 500.0)]     # (639.9: round(63.99) = 64, one past the last column)


def _big_frame(N, layout, seed):
    """N host-built keypoints in a 640 x 480 image.  "sparse": spread evenly, every cell holds few; "crowded": a third of them within 40 x 30 pixels, those cells
    hold far more than kGridSmallCell.  Both: keypoints outside the grid at the front, around index 4096 and near the end (the last keypoint is inside)."""
    rng = np.random.default_rng(seed)
    k = np.zeros(N, KP_DTYPE)
    k["x"] = rng.uniform(0, W - 1, N).astype(f32); k["y"] = rng.uniform(0, H - 1, N).astype(f32)
    if layout == "crowded":
        c = rng.choice(N, N // 3, replace=False)
        k["x"][c] = rng.uniform(300, 340, len(c)).astype(f32); k["y"][c] = rng.uniform(200, 230, len(c)).astype(f32)
    where = [0, 5, 1023, 1024, N // 2, KEPT - 2, KEPT - 1, KEPT + 1, N - 2]
    for j, i in enumerate(i for i in where if 0 <= i < N):
        k["x"][i], k["y"][i] = OUTSIDE[j % len(OUTSIDE)]
    k["octave"] = rng.integers(0, 8, N); k["angle"] = rng.uniform(0, 360, N).astype(f32); k["size"] = 31.0; k["response"] = 50.0; k["class_id"] = -1
    d = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    return k, d


BIG_N = (4095, 4096, 4097, 8192, 10000)
_QUERIES = [(320, 215, 45, -1, -1), (320, 215, 12, 0, 3), (10, 10, 60, 2, -1), (635, 475, 30, -1, -1), (-50, 100, 20, -1, -1), (900, 100, 20, -1, -1),
            (100, -80, 30, -1, -1), (100, 700, 30, -1, -1), (0, 240, 25, 0, -1), (639, 0, 40, 1, 2), (200, 150, 0.5, -1, -1), (320, 240, 1000, 7, 7), (320, 240, 1000, -1, -1)]
_GRID_REF = {}


def _grid_reference(N, layout):
    """the frame, its restated grid and the expected index lists of the queries: made once, shared by the emulator and the GPU form, not written afterwards"""
    if (N, layout) not in _GRID_REF:
        k, d = _big_frame(N, layout, 1000 + N + (layout == "crowded"))
        g = RestatedGrid(k, W, H)
        exp = [g.features_in_area(*q) for q in _QUERIES]
        k.setflags(write=False); d.setflags(write=False)
        _GRID_REF[(N, layout)] = (k, d, g, exp)
    return _GRID_REF[(N, layout)]


REF_WORLD = os.path.join(ol.ROOT, "oracle", "_ref", "libmw_ref.so")          # the reference's own ORBmatcher.cc over frames that take keypoints (tests/matcher_world.py)
_INIT_REF = {}


def _reference_search_for_initialization(key, k1, d1, k2, d2, window, nnratio):
    """ORBmatcher::SearchForInitialization of the reference on two frames holding these keypoints (grid of 640 x 480 bounds); None where oracle/_ref is not built"""
    if not os.path.exists(REF_WORLD):
        return None
    if key not in _INIT_REF:
        drv = mw.Driver(REF_WORLD)
        cam = drv.camera(500.0, 500.0, 320.0, 240.0)
        bounds = np.array([0, 0, W, H], f32); I, z3 = np.eye(3, dtype=f32), np.zeros(3, f32)
        ids = []
        for k, d in ((k1, d1), (k2, d2)):
            kk = np.ascontiguousarray(k).astype(mw.KP); dd = np.ascontiguousarray(d)
            ids.append(drv.L.mw_add_frame(drv.w, 0, len(kk), mw._p(kk), mw._p(kk), -1, None, mw._p(dd), None, mw._p(I), mw._p(z3), None, None, mw._p(bounds), 8, C.c_float(1.2),
                                          cam, -1, C.c_float(0.0), C.c_float(0.0)))
        prev = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), f32); m12 = np.full(len(k1), -1, np.int32)
        n = drv.L.mw_search_for_initialization(drv.w, ids[0], ids[1], mw._p(prev), mw._p(m12), int(window), C.c_float(nnratio), 1)
        drv.close()
        _INIT_REF[key] = (n, m12, prev)
    return _INIT_REF[key]


def _check_big_grid(lib, N, layout):
    k, d, g, exp = _grid_reference(N, layout)
    # the input enters what it is made for
    assert (g.largest_cell > SMALL_CELL) == (layout == "crowded"), g.largest_cell
    assert (~g.inside[:KEPT]).sum() >= 4 and (N < 2 * KEPT or (~g.inside[KEPT:]).sum() >= 2)
    assert sorted(exp[-1]) == np.flatnonzero(g.inside).tolist() and (N <= KEPT or N - 1 in exp[-1])       # the whole-image window: every keypoint of the grid
    assert sum(len(e) for e in exp) > N // 10 and sum(len(e) == 0 for e in exp) >= 4
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    fv = views.frame_view(k, d, SCALES, W, H)
    for q, e in zip(_QUERIES, exp):
        got = M.GetFeaturesInArea(ex, fv, *q)
        assert got.tolist() == e, "GetFeaturesInArea%r of %d keypoints (%s) differs from the restated Frame.cc: %d vs %d indices" % (q, N, layout, len(got), len(e))
        assert ol.oracle_features_in_area(fv, *q).tolist() == e, q
    # ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:734-880) runs GetFeaturesInArea on the second frame for every level-0 keypoint of the first
    rng = np.random.default_rng(N)
    k2 = k.copy(); k2["x"] = k["x"] + rng.uniform(-4, 4, N).astype(f32); k2["y"] = k["y"] + rng.uniform(-4, 4, N).astype(f32)
    perm = rng.permutation(N); k2 = np.ascontiguousarray(k2[perm])
    d2 = d[perm].copy()
    flip = rng.integers(0, 256, (N, 12)); keep = rng.random((N, 12)) < 0.5
    for c in range(12):
        rows = np.flatnonzero(keep[:, c]); d2[rows, flip[rows, c] >> 3] ^= (1 << (flip[rows, c] & 7)).astype(np.uint8)
    f2 = views.frame_view(k2, d2, SCALES, W, H)
    pa = np.ascontiguousarray(np.stack([k["x"], k["y"]], 1), f32); pb = pa.copy()
    n1, m1 = M.ORBmatcher(0.9, True).SearchForInitialization(ex, fv, f2, pa, 20)
    n2, m2 = ol.oracle_search_for_initialization(fv, f2, pb, 20, 0.9, True)
    assert n1 == n2 and np.array_equal(m1, m2) and pa.tobytes() == pb.tobytes(), "SearchForInitialization, %d keypoints (%s): %d vs %d matches" % (N, layout, n1, n2)
    ref = _reference_search_for_initialization((N, layout), k, d, k2, d2, 20, 0.9)
    if ref is not None:
        assert n1 == ref[0] and np.array_equal(m1, ref[1]) and pa.tobytes() == ref[2].tobytes(), "SearchForInitialization, %d keypoints (%s): %d matches vs the reference's %d" % (N, layout, n1, ref[0])
    level0 = int((k["octave"] == 0).sum())
    assert n2 > level0 // 4 and (N <= KEPT + 1 or (m2[m2 >= 0] >= KEPT).sum() > 10), "too few matches to be a test: %d of %d level-0 keypoints" % (n2, level0)
    if N == 8192:
        _local_points_on_big_frame(ex, fv, k, d)
    ex.close()


def _local_points_on_big_frame(ex, fv, k, d):
    """one Tracking::SearchLocalPoints through the single-frame call on 8192 keypoints: the frustum fields go into the oracle's SearchByProjection(Frame, MapPoints)"""
    rng = np.random.default_rng(8)
    N = len(k); Mp = 1500
    fx, fy, cx, cy = 500.0, 500.0, 320.0, 240.0
    src = rng.integers(0, N, Mp); z = rng.uniform(2, 8, Mp)
    Xw = np.stack([(k["x"][src] + rng.normal(0, 1, Mp) - cx) / fx * z, (k["y"][src] + rng.normal(0, 1, Mp) - cy) / fy * z, z], 1).astype(f32)
    dist = np.linalg.norm(Xw.astype(np.float64), axis=1)
    normal = (Xw / dist[:, None]).astype(f32)
    maxd = (dist * 1.2 ** k["octave"][src] * rng.uniform(0.9, 1.1, Mp)).astype(f32); mind = (maxd / f32(1.2 ** 7)).astype(f32)
    desc = d[src].copy(); bad = rng.random(Mp) < 0.03; obs = rng.random(Mp) < 0.9
    I, t0 = np.eye(3, dtype=f32), np.zeros(3, f32)
    tr, asg, n = M.SearchLocalPoints(ex, fv, I, t0, (fx, fy, cx, cy), (0.0, float(W), 0.0, float(H)), 0.0, SCALES, Xw, normal, mind, maxd, bad, obs, desc, 0.5, 3.0, False, 0.0, 0.8)
    mps = views.map_point_view(tr["in_view"], tr["proj_x"], tr["proj_y"], tr["proj_xr"], tr["scale_level"], tr["view_cos"], tr["depth"], bad, obs, desc)
    n2, a2 = ol.oracle_search_by_projection_mappoints(fv, mps, 3.0, False, 0.0, 0.8)
    assert tr["in_view"].sum() > Mp // 2 and n == n2 > Mp // 10 and np.array_equal(asg, a2), "SearchLocalPoints on 8192 keypoints: %d vs %d matches" % (n, n2)
    assert (a2[KEPT:] >= 0).sum() > 20


@pytest.mark.parametrize("layout", ["sparse", "crowded"])
@pytest.mark.parametrize("N", BIG_N)
def test_grid_of_large_frames_emulated(emu_lib, N, layout):
    _check_big_grid(emu_lib, N, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["sparse", "crowded"])
@pytest.mark.parametrize("N", BIG_N)
def test_grid_of_large_frames_gpu(hip_lib, N, layout):
    _check_big_grid(hip_lib, N, layout)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# MapPoint::PredictScale (src/MapPoint.cc:714-731) behind the distance gates of Frame::isInFrustum (src/Frame.cc:722-730) and of the relocalisation search
# (src/ORBmatcher.cc:2232-2241)
PW, PH, PNF = 376, 240, 500
PFX, PFY, PCX, PCY = 230.0, 230.0, 188.0, 120.0
PBF = PFX * 0.11
_LIBM = C.CDLL("libm.so.6")
_LIBM.logf.restype = C.c_float; _LIBM.logf.argtypes = [C.c_float]
KINDS = ("min_on", "min_inside", "min_outside", "max_on", "max_inside", "max_outside", "n_is_nlevels", "n_is_last_level")


def _factor_hitting(target, factor, start):
    """a float m with float(factor * m) == target, searched from start (m -> factor * m maps neighbouring floats onto the same or neighbouring floats)"""
    m = f32(start)
    for _ in range(16):
        p = f32(factor) * m
        if p == target:
            return m
        m = np.nextafter(m, f32(np.inf) if p < target else f32(-np.inf))
    return None


def _predict_scale_scene(F, scale):
    """for 48 keypoints of the frame a point on the keypoint's ray, six times: mfMinDistance / mfMaxDistance set so that the point's distance from the camera
    centre - restated in float32 as PO.norm(), Eigen's a0 + (a1 + a2) - is exactly 0.8 mfMinDistance, one float above it (inside), one float below (outside),
    and the same around 1.2 mfMaxDistance.  Returns the keypoints, the points in camera coordinates, logf(scale) and scale^7."""
    rng = np.random.default_rng(77)
    order = np.argsort(F.keys["octave"], kind="stable")
    src = np.concatenate([order[:24], order[-24:]])                    # the clamp at 0 is visible at the finest keypoints, the clamp at nlevels - 1 at the coarsest
    z = rng.uniform(2.0, 6.0, len(src))
    Xc = np.stack([(F.keys["x"][src] - PCX) / PFX * z, (F.keys["y"][src] - PCY) / PFY * z, z], 1)
    return src, Xc, f32(_LIBM.logf(f32(scale))), f32(scale) ** 7


def _restate_points(pos, Ow, mind, maxd, log_s, nlevels=8):
    o = pos.astype(f32) - Ow.astype(f32)[None, :]
    dist = np.sqrt(o[:, 0] * o[:, 0] + (o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2]))              # float32 throughout
    in_range = ~((dist < f32(0.8) * mind) | (dist > f32(1.2) * maxd))
    ratio = maxd / dist
    n = np.array([int(np.ceil(f32(_LIBM.logf(r)) / log_s)) for r in ratio])
    return dist, in_range, n, np.clip(n, 0, nlevels - 1)


_PS_REF = {}


def _predict_scale_case(scale):
    if scale in _PS_REF:
        return _PS_REF[scale]
    from test_local_points import _rot
    L, R = synth.stereo_pair(PW, PH, seed=31, nrect=800)
    F = ol.ReferenceFrame(L, R, PNF, scale, 8, 20, 7, 0, fx=PFX, fy=PFY, cx=PCX, cy=PCY, bf=PBF)
    Rcw = _rot(0.02, -0.03, 0.01); tcw = np.array([0.05, -0.02, 0.04], f32)
    sfs = np.cumprod(np.array([1.0] + [scale] * 7, f32), dtype=f32)
    V, _ = M.frustum_view(Rcw, tcw, (PFX, PFY, PCX, PCY), (0.0, float(PW), 0.0, float(PH)), PBF, sfs)
    Ow = np.array(list(V.Ow), f32)
    src, Xc, log_s, s7 = _predict_scale_scene(F, scale)
    assert log_s == f32(V.log_scale_factor)
    Xw = ((Rcw.astype(np.float64).T @ (Xc - tcw.astype(np.float64)).T).T).astype(f32)
    dist0 = _restate_points(Xw, Ow, np.ones(len(Xw), f32), np.ones(len(Xw), f32), log_s)[0]
    pos, mind, maxd, kind, source = [], [], [], [], []
    up, down = f32(np.inf), f32(-np.inf)
    for j, s in enumerate(src):
        dj = dist0[j]
        for kd in KINDS:
            if kd.startswith("n_is"):                                    # well inside the range: n = nlevels exactly (the first clamped value) and n = nlevels - 1 (the last free one)
                m = f32(dj * f32(scale) ** f32(7.5 if kd == "n_is_nlevels" else 6.5))
                mx, mn = m, f32(m / s7)
            elif kd.startswith("min"):
                target = {"min_on": dj, "min_inside": np.nextafter(dj, down), "min_outside": np.nextafter(dj, up)}[kd]          # = 0.8 mfMinDistance
                m = _factor_hitting(target, 0.8, target / f32(0.8))
                mn, mx = m, (None if m is None else f32(m * s7))
            else:
                target = {"max_on": dj, "max_inside": np.nextafter(dj, up), "max_outside": np.nextafter(dj, down)}[kd]           # = 1.2 mfMaxDistance
                m = _factor_hitting(target, 1.2, target / f32(1.2))
                mx, mn = m, (None if m is None else f32(m / s7))
            if m is None:
                continue
            pos.append(Xw[j]); mind.append(mn); maxd.append(mx); kind.append(kd); source.append(int(s))
    pos = np.array(pos, f32); mind = np.array(mind, f32); maxd = np.array(maxd, f32); kind = np.array(kind); source = np.array(source)
    dist, in_range, n, lvl = _restate_points(pos, Ow, mind, maxd, log_s)
    normal = ((pos - Ow) / dist[:, None]).astype(f32)
    case = dict(L=L, R=R, F=F, Rcw=Rcw, tcw=tcw, sfs=sfs, pos=pos, mind=mind, maxd=maxd, kind=kind, source=source, normal=normal, in_range=in_range, n=n, lvl=lvl,
                desc=F.desc[source].copy(), angle=F.keys["angle"][source].copy())
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _PS_REF[scale] = case
    return case


def _check_predict_scale(lib, scale):
    c = _predict_scale_case(scale)
    F, pos, mind, maxd, kind, in_range, n, lvl = c["F"], c["pos"], c["mind"], c["maxd"], c["kind"], c["in_range"], c["n"], c["lvl"]
    Mp = len(pos)
    # the input enters what it is made for: every kind of point exists, the points on and inside a limit pass, those outside fail, both clamps act
    for kd in KINDS:
        sel = kind == kd
        assert sel.sum() >= 40, (kd, int(sel.sum()))
        assert (in_range[sel] == (not kd.endswith("outside"))).all(), kd
    assert (n[in_range] < 0).sum() >= (40 if scale == 1.1 else 1) and (n[in_range] >= 8).sum() >= 40, "PredictScale's clamps are not entered"
    assert (n[kind == "n_is_nlevels"] == 8).all() and (n[kind == "n_is_last_level"] == 7).all()
    assert n[in_range].min() == -1 and set(lvl[in_range & np.char.startswith(kind, "max")]) == {0} and set(lvl[in_range & np.char.startswith(kind, "min")]) == {7}
    ex = ORBextractor(PNF, scale, 8, 20, 7, lib=lib)
    (_, kL, dL), _ = ex.extract_batch(np.stack([c["L"], c["R"]]))
    assert kL.tobytes() == F.keys.tobytes() and dL.tobytes() == F.desc.tobytes()
    assert np.array_equal(np.asarray(ex.GetScaleFactors(), f32), c["sfs"])
    fv = views.frame_view(kL, dL, c["sfs"], PW, PH, u_right=F.u_right, mbf=PBF)
    bad = np.zeros(Mp, bool); obs = np.ones(Mp, bool)
    cam, bounds = (PFX, PFY, PCX, PCY), (0.0, float(PW), 0.0, float(PH))
    # Frame::isInFrustum + PredictScale + SearchByProjection(Frame, MapPoints): k_frustum
    ref_tr, ref_as, ref_n = F.search_local_points(c["Rcw"], c["tcw"], pos, c["normal"], mind, maxd, bad, obs, c["desc"], 0.5, True, 3.0, False, 0.0, 0.8)
    assert np.array_equal(ref_tr["in_view"], in_range), "the restated distance gates differ from the reference's isInFrustum at %d points" % int((ref_tr["in_view"] != in_range).sum())
    assert np.array_equal(ref_tr["scale_level"][in_range], lvl[in_range]), "the restated PredictScale differs from the reference"
    tr, asg, nm = M.SearchLocalPoints(ex, fv, c["Rcw"], c["tcw"], cam, bounds, PBF, c["sfs"], pos, c["normal"], mind, maxd, bad, obs, c["desc"], 0.5, 3.0, False, 0.0, 0.8)
    wrong = np.flatnonzero(tr["in_view"].astype(bool) != in_range)
    assert len(wrong) == 0, "mbTrackInView differs at %d points, first: %s" % (len(wrong), kind[wrong[0]])
    wrong = np.flatnonzero((tr["scale_level"] != lvl) & in_range)
    assert len(wrong) == 0, "mnTrackScaleLevel differs at %d points, first: %s, %d vs %d (before the clamp %d)" % (len(wrong), kind[wrong[0]], tr["scale_level"][wrong[0]], lvl[wrong[0]], n[wrong[0]])
    for key in ("proj_x", "proj_y"):
        assert tr[key].tobytes() == ref_tr[key].tobytes(), key
    for key in ("proj_xr", "depth", "view_cos"):
        assert tr[key][in_range].tobytes() == ref_tr[key][in_range].tobytes(), key
    assert nm == ref_n and np.array_equal(asg, ref_as), "SearchByProjection assignment differs (%d vs %d matches)" % (nm, ref_n)
    assert ref_n >= 20
    # the relocalisation search, SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): k_keyframe_queries
    ones = np.ones(Mp, np.uint8)
    for ori in (True, False):
        kn, kas = F.search_keyframe(c["Rcw"], c["tcw"], pos, ones, mind, maxd, c["angle"], c["desc"], 10.0, 100, ori, 0.9, None)
        kb = M.KeyFrameBatch(ex, 1, cam, bounds, PBF, c["sfs"]); kb.set_poses([(c["Rcw"], c["tcw"])])
        kb.enqueue(np.array([Mp], np.int32), pos[None], ones[None], mind[None], maxd[None], c["angle"][None], c["desc"][None], 10.0, 100, ori, None)
        a, m = kb.fetch()
        assert m[0] == kn and np.array_equal(a[0, :F.N], kas), "relocalisation search (orientation check %s): %d vs the reference's %d matches" % (ori, m[0], kn)
        got = kas[kas >= 0]
        assert len(got) >= 20 and in_range[got].all(), "a point outside its distance range was matched"
        # a matched keypoint lies in [level - 1, level + 1] of the CLAMPED level: at the ends that is only so because of the clamp
        octv = F.keys["octave"][np.flatnonzero(kas >= 0)]
        assert (np.abs(octv - lvl[got]) <= 1).all()
        assert (lvl[got] == 0).sum() >= 5 and (lvl[got] == 7).sum() >= 5
    ex.close()


@pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so not built (needs /root/reference)")
@pytest.mark.parametrize("scale", [1.2, 1.1])
def test_predict_scale_clamps_emulated(emu_lib, scale):
    _check_predict_scale(emu_lib, scale)


@pytest.mark.gpu
@pytest.mark.skipif(ol.reference_frame_lib() is None, reason="oracle/_ref/libref_frame.so not built (needs /root/reference)")
@pytest.mark.parametrize("scale", [1.2, 1.1])
def test_predict_scale_clamps_gpu(hip_lib, scale):
    _check_predict_scale(hip_lib, scale)
