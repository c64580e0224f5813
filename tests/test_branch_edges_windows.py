"""The image test of k_project_points (csrc/k_search.hip) in both of its forms - the Frame's inclusive one (`u < mnMinX || u > mnMaxX`, src/ORBmatcher.cc:2003-2006)
and KeyFrame::IsInImage's half-open one (`u >= mnMinX && u < mnMaxX`, src/KeyFrame.cc:803-806) - with projections exactly ON each of the four bounds, one float
outside and one float inside; and search windows that miss the 64 x 48 grid on each side (`nMinCellX >= FRAME_GRID_COLS`, `nMaxCellX < 0`, ... src/Frame.cc:877-903)
for the projection-type searches that run without an image test (bounds mode 2: SearchByProjection(KeyFrame*, Sim3, ...) and Fuse take whatever projects).

With the identity pose, fx = fy = 1, cx = cy = 0 and z = 1 every operation of the projection is exact: the point (u, v, 1) projects to (u, v) bit for bit, so the
test chooses the projections and restates the image test on them.  Random scenes put a projection exactly on a bound with probability 2^-24."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ORBextractor, views
from orb_slam3_detailed_comments_amd import matcher as M
from orb_slam3_detailed_comments_amd._lib import KP_DTYPE
from test_branch_edges_search import RestatedGrid

f32 = np.float32
BOUNDS = (10.0, 300.0, 20.0, 200.0)             # mnMinX, mnMaxX, mnMinY, mnMaxY
UP, DOWN = f32(np.inf), f32(-np.inf)
I3, T0 = np.eye(3, dtype=f32), np.zeros(3, f32)


def _edge_points():
    """(u, v, what) : 25 points per (bound, on / one float outside / one float inside), the other coordinate anywhere inside; and the four corners"""
    rng = np.random.default_rng(3)
    mnx, mxx, mny, mxy = [f32(b) for b in BOUNDS]
    pts = []
    for name, val, out_dir in (("min_x", mnx, DOWN), ("max_x", mxx, UP), ("min_y", mny, DOWN), ("max_y", mxy, UP)):
        for what, x in (("on", val), ("outside", np.nextafter(val, out_dir)), ("inside", np.nextafter(val, -out_dir))):
            for _ in range(25):
                other = f32(rng.uniform(30, 190))
                pts.append((x, other, name, what) if name.endswith("x") else (other, x, name, what))
    for x in (mnx, mxx):
        for y in (mny, mxy):
            pts.append((x, y, "corner", "on"))
    return pts


def restated_image_test(u, v, mode):
    mnx, mxx, mny, mxy = [f32(b) for b in BOUNDS]
    if mode == 0:
        return not (u < mnx or u > mxx or v < mny or v > mxy)
    if mode == 1:
        return bool(u >= mnx and u < mxx and v >= mny and v < mxy)
    return True


def _check_bounds(lib):
    pts = _edge_points()
    pos = np.array([(u, v, 1.0) for u, v, _, _ in pts], f32)
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    seen = set()
    for mode in (0, 1, 2):
        for inline in (False, True):
            pr = M.ProjectPoints(ex, (I3, T0), (1.0, 1.0, 0.0, 0.0), BOUNDS, pos, depth_test=1, bounds_mode=mode, inline_pinhole=inline)
            assert pr["u"].tobytes() == pos[:, 0].tobytes() and pr["v"].tobytes() == pos[:, 1].tobytes(), "the projection is not exact: the test cannot choose it"
            for i, (u, v, name, what) in enumerate(pts):
                exp = restated_image_test(u, v, mode)
                assert bool(pr["valid"][i]) == exp, "bounds mode %d%s: %s %s (%r, %r) is %s" % (mode, " inline" if inline else "", name, what, u, v, "valid" if pr["valid"][i] else "invalid")
                seen.add((mode, name, what, exp))
    # the input enters both sides of every comparison: on a maximum the two forms differ, on a minimum they agree, outside fails both, mode 2 takes everything
    for name in ("min_x", "max_x", "min_y", "max_y"):
        assert (0, name, "on", True) in seen and (1, name, "on", name.startswith("min")) in seen
        assert (0, name, "outside", False) in seen and (1, name, "outside", False) in seen and (2, name, "outside", True) in seen
        assert (0, name, "inside", True) in seen and (1, name, "inside", True) in seen
    ex.close()


def test_project_points_on_the_image_bounds_emulated(emu_lib):
    _check_bounds(emu_lib)


@pytest.mark.gpu
def test_project_points_on_the_image_bounds_gpu(hip_lib):
    _check_bounds(hip_lib)


W, H = 376, 240
SCALES = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)


def _check_windows(lib):
    rng = np.random.default_rng(12)
    N = 600
    k = np.zeros(N, KP_DTYPE)
    k["x"] = rng.uniform(0, W - 1, N).astype(f32); k["y"] = rng.uniform(0, H - 1, N).astype(f32); k["octave"] = rng.integers(0, 8, N)
    k["angle"] = rng.uniform(0, 360, N).astype(f32); k["size"] = 31.0; k["class_id"] = -1
    d = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    ur = np.where(rng.random(N) < 0.6, k["x"] - f32(4.0), f32(-1)).astype(f32)
    kf = views.frame_view(k, d, SCALES, W, H, ur, np.zeros(N, np.uint8), 40.0)
    g = RestatedGrid(k, W, H)
    # 60 points per side, further out than any window radius (th * scale <= 8 * 3.6), 30 whose window reaches back in over each side, 200 on keypoints
    side = {"left": lambda n: (rng.uniform(-400, -40, n), rng.uniform(0, H, n)), "right": lambda n: (rng.uniform(W + 40, W + 400, n), rng.uniform(0, H, n)),
            "above": lambda n: (rng.uniform(0, W, n), rng.uniform(-400, -40, n)), "below": lambda n: (rng.uniform(0, W, n), rng.uniform(H + 40, H + 400, n))}
    near = {"left": lambda n: (rng.uniform(-3, -0.5, n), rng.uniform(20, H - 20, n)), "right": lambda n: (rng.uniform(W + 0.5, W + 3, n), rng.uniform(20, H - 20, n)),
            "above": lambda n: (rng.uniform(20, W - 20, n), rng.uniform(-3, -0.5, n)), "below": lambda n: (rng.uniform(20, W - 20, n), rng.uniform(H + 0.5, H + 3, n))}
    side["left_above"] = lambda n: (rng.uniform(-400, -40, n), rng.uniform(-400, -40, n))          # off two sides at once: both cell ranges are empty
    side["right_below"] = lambda n: (rng.uniform(W + 40, W + 400, n), rng.uniform(H + 40, H + 400, n))
    near["left_above"] = lambda n: (rng.uniform(-3, -0.5, n), rng.uniform(-3, -0.5, n)); near["right_below"] = lambda n: (rng.uniform(W + 0.5, W + 3, n), rng.uniform(H + 0.5, H + 3, n))
    us, vs, tag = [], [], []
    for name in side:
        u, v = side[name](60); us.append(u); vs.append(v); tag += ["far_" + name] * 60
        u, v = near[name](30); us.append(u); vs.append(v); tag += ["near_" + name] * 30
    src = rng.integers(0, N, 200)
    us.append(k["x"][src] + rng.uniform(-2, 2, 200)); vs.append(k["y"][src] + rng.uniform(-2, 2, 200)); tag += ["inside"] * 200
    u = np.concatenate(us).astype(f32); v = np.concatenate(vs).astype(f32); tag = np.array(tag); Mp = len(u)
    desc = rng.integers(0, 256, (Mp, 32), dtype=np.uint8); desc[tag == "inside"] = d[src]
    lvl = rng.integers(0, 8, Mp).astype(np.int32); lvl[tag == "inside"] = k["octave"][src]
    # through the device projection without an image test: everything stays valid, wherever it lands
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=lib)
    pr = M.ProjectPoints(ex, (I3, T0), (1.0, 1.0, 0.0, 0.0), (0.0, float(W), 0.0, float(H)), np.stack([u, v, np.ones(Mp, f32)], 1), depth_test=1, bounds_mode=2)
    assert pr["valid"].all() and pr["u"].tobytes() == u.tobytes() and pr["v"].tobytes() == v.tobytes()
    pts = views.projected_point_view(pr["valid"], pr["u"], pr["v"], lvl, desc, ur=(pr["u"] - f32(4.0)).astype(f32))
    for th in (3, 8):
        # the restated windows: radius th * scale[level] (src/ORBmatcher.cc:552); the far points' windows hold nothing because they miss the grid on their side
        cand = [g.features_in_area(u[i], v[i], f32(th) * SCALES[lvl[i]]) for i in range(Mp)]
        for name in side:
            assert all(len(cand[i]) == 0 for i in np.flatnonzero(tag == "far_" + name)), name
        assert sum(len(cand[i]) > 0 for i in np.flatnonzero(np.char.startswith(tag, "near_"))) >= 20 and sum(len(cand[i]) > 0 for i in np.flatnonzero(tag == "inside")) >= 150
        n1, a1 = M.ORBmatcher().SearchByProjectionSim3(ex, kf, pts, th, 1.0)
        n2, a2 = ol.oracle_search_by_projection_sim3(kf, pts, th, 1.0)
        assert n1 == n2 and np.array_equal(a1, a2), "SearchByProjection(KeyFrame, Sim3) th %d: %d vs %d matches" % (th, n1, n2)
        matched = a2[a2 >= 0]
        assert n2 >= 100 and not np.char.startswith(tag[matched], "far_").any()
        assert all(int(kp) in cand[int(p)] for kp, p in zip(np.flatnonzero(a2 >= 0), matched)), "a match outside the point's restated window"
        inv_s2 = (f32(1.0) / (SCALES * SCALES)).astype(f32)
        for s2 in (inv_s2, None):
            b1, d1 = M.ORBmatcher().FuseCandidates(ex, kf, pts, float(th), s2)
            b2, d2 = ol.oracle_fuse_candidates(kf, pts, float(th), s2)
            assert np.array_equal(b1, b2) and np.array_equal(d1, d2), "Fuse candidates, th %d" % th
            assert (b2[np.char.startswith(tag, "far_")] == -1).all() and (b2[tag == "inside"] >= 0).sum() >= 100
            assert all(b2[i] in cand[i] for i in np.flatnonzero(b2 >= 0))
    ex.close()


def test_windows_off_the_grid_emulated(emu_lib):
    _check_windows(emu_lib)


@pytest.mark.gpu
def test_windows_off_the_grid_gpu(hip_lib):
    _check_windows(hip_lib)
