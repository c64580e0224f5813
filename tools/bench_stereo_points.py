"""The stereo map points a new key frame is born with (the second half of Tracking::CreateNewKeyFrame, src/Tracking.cc:3868-3960), for B frames that are on
the device, in milliseconds per call, blocking, the two routes alternating inside every repetition on one box in one run.
  (a) host_route     what a host with an orbm_map had to do: orbx_fetch_undistorted (mvKeysUn) and orbm_stereo_fetch (mvDepth) of the batch; per frame the
                     sort by (depth, index), the stop rule, the unprojection and the five fields in numpy float32 (a C++ host would be faster at this part:
                     host_compute gives it alone); the descriptor rows picked from rows the host already holds; one orbm_map_update of all new points
                     and B x orbm_map_set_keyframe
  (b) stereo_points  one orbm_map_stereo_points(h, map, B, ..) with a row per frame, its table built beforehand
Shape (tools/bench_local_map_build.py's): 640 x 480, 1000 features, uRight / depth from a depth image, B = 1, 8, 64; th_depth = 2.4 (about 40 % of the
depths are closer), max_points = 100, every fifth feature keeps a point; orbm_keyframe_create_extracted has run on the batch before (the first half of
CreateNewKeyFrame: not timed, both routes follow it).  Every repetition writes the same slots and rows again.  The tool asserts that both routes select
the same features and leave the same fields up to the rounding of numpy's matrix product (the bit-exact check is tests/test_stereo_points.py).
Prints one JSON line.  Usage: python tools/bench_stereo_points.py [--out profiles/stereo_points/bench.json] [--reps 20] [--lib other_build.so] [--batches 1,8,64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_detailed_comments_amd import KP_DTYPE, ORBextractor, synth  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402

W, H, NF, NSCENES, MBF = 640, 480, 1000, 8, 40.0
TH, MAXP = np.float32(2.4), 100
CAM = np.array([320.5, 239.5, 1.0 / 458.0, 1.0 / 457.0, 0, 0], np.float32)
f32 = np.float32


def stats(t):
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)))


def alternating(fns, reps, warm=3):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    t = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter(); fn(); t[name].append((time.perf_counter() - t0) * 1e3)
    return {name: stats(v) for name, v in t.items()}


def host_points(kp, depth, desc, keeps, Rwc, Ow, scale):
    """the loop of Tracking.cc:3876-3958 and the fields of the created points, in numpy float32"""
    cand = np.flatnonzero(depth > 0)
    order = cand[np.lexsort((cand, depth[cand]))]
    far = np.flatnonzero((depth[order] > TH) & (np.arange(1, len(order) + 1) > MAXP))
    order = order[:far[0] + 1] if len(far) else order
    feat = order[keeps[order] == 0]
    z = depth[feat]
    x = (kp["x"][feat] - CAM[0]) * z * CAM[2]; y = (kp["y"][feat] - CAM[1]) * z * CAM[3]
    pos = (np.stack([x, y, z], 1) @ Rwc.T + Ow).astype(f32)
    d = pos - Ow
    dist = np.sqrt((d * d).sum(1, dtype=f32))
    mx = dist * scale[kp["octave"][feat]]
    return len(order), feat, pos, d / dist[:, None], mx / scale[-1], mx, desc[feat]


def bench(lib, batches, reps):
    bmax = max(batches)
    rng = np.random.default_rng(11)
    imgs = [synth.corner_field(W, H, seed=500 + s, nrect=2500) for s in range(NSCENES)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    L = ex._lib
    cap = ex.max_keypoints()
    scale = np.asarray(ex.GetScaleFactors(), f32)
    depth_img = (2.0 + np.sin(np.arange(W)[None, :] / 50.0) + np.cos(np.arange(H)[:, None] / 40.0)).astype(f32)
    per = cap + 8
    mp = M.ResidentMap(ex, bmax * per, bmax, cap, 1)
    free = [(b * per + rng.permutation(per)).astype(np.int32) for b in range(bmax)]
    ang = rng.normal(0, 0.02, (bmax, 3))
    poses = []
    for b in range(bmax):
        a, c, e = ang[b]
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]); Ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(e), -np.sin(e)], [0, np.sin(e), np.cos(e)]])
        poses.append(((Rz @ Ry @ Rx).astype(f32), rng.normal(0, 0.5, 3).astype(f32)))
    kun = np.zeros((bmax, cap), KP_DTYPE); ur = np.zeros((bmax, cap), f32); dep = np.zeros((bmax, cap), f32); nm = np.zeros(bmax, np.int32)
    ptr = lambda a: a.ctypes.data
    out = {}
    for B in batches:
        # a batch of exactly B frames: the host route's fetches move what the extraction holds
        res = ex.extract_batch(np.stack([imgs[b % NSCENES] for b in range(B)]))
        M.ComputeStereoFromRGBD(ex, np.broadcast_to(depth_img, (B, H, W)).copy(), MBF)
        kfs = M.ResidentKeyFrame.from_extracted(ex, None, list(range(B)), use_u_right=True)
        n = [len(r[1]) for r in res]
        descs = [np.ascontiguousarray(r[2], np.uint8).reshape(-1, 32) for r in res]
        keeps = [(np.arange(k) % 5 == 0).astype(np.uint8) for k in n]
        tab = (M._StereoPointsFrame * B)()
        for b in range(B):
            t = tab[b]; t.frame = b; t.Rwc[:] = [float(v) for v in poses[b][0].reshape(9)]; t.Ow[:] = [float(v) for v in poses[b][1]]
            t.keeps = ptr(keeps[b]); t.free_slots = ptr(free[b]); t.nfree = len(free[b]); t.row = b
        created = np.zeros(B, np.int32); processed = np.zeros(B, np.int32); feat = np.zeros((B, cap), np.int32); slot = np.zeros((B, cap), np.int32)

        def new_fn():
            L.check(L.L.orbm_map_stereo_points(ex._h, mp._m, B, tab, ptr(CAM), float(TH), MAXP, 0, ptr(created), ptr(processed), cap, ptr(feat), ptr(slot)))

        last = {}

        def compute():
            pts = [host_points(kun[b, :n[b]], dep[b, :n[b]], descs[b], keeps[b], poses[b][0], poses[b][1], scale) for b in range(B)]
            last["pts"] = pts
            return pts

        def host_fn():
            L.check(L.L.orbx_fetch_undistorted(ex._h, ptr(kun), cap))
            L.check(L.L.orbm_stereo_fetch(ex._h, B, ptr(ur), ptr(dep), cap, ptr(nm)))
            pts = compute()
            slots = np.concatenate([free[b][:len(p[1])] for b, p in enumerate(pts)])
            if len(slots):
                mp.update(slots, *[np.concatenate([p[k] for p in pts]) for k in (2, 3, 4, 5, 6)])
            for b, p in enumerate(pts):
                row = np.full(n[b], -1, np.int32)
                row[p[1]] = free[b][:len(p[1])]
                L.check(L.L.orbm_map_set_keyframe(ex._h, mp._m, b, n[b], ptr(row)))

        # both routes select the same features and leave (nearly) the same fields
        host_fn()
        mp.select(0, np.concatenate([free[b][:len(p[1])] for b, p in enumerate(last["pts"])]))
        h_fields = M.PointsFetch(ex, mp.set(0))
        new_fn()
        for b, p in enumerate(last["pts"]):
            assert processed[b] == p[0] and created[b] == len(p[1]) and np.array_equal(feat[b, :created[b]], p[1]), "frame %d: the routes select different features" % b
        mp.select(0, np.concatenate([slot[b, :created[b]] for b in range(B)]))
        d_fields = M.PointsFetch(ex, mp.set(0))
        for hf, df in zip(h_fields[:4], d_fields[:4]):
            assert np.allclose(hf, df, rtol=1e-5, atol=1e-6)
        assert np.array_equal(h_fields[4], d_fields[4])
        alt = alternating(dict(host_route=host_fn, stereo_points=new_fn), reps)
        alt["new_over_host"] = alt["stereo_points"]["ms"] / alt["host_route"]["ms"]
        t = []
        for _ in range(max(3, reps // 2)):
            t0 = time.perf_counter(); compute(); t.append((time.perf_counter() - t0) * 1e3)
        alt["host_compute"] = stats(t)
        alt["created_per_frame"] = [int(v) for v in created[:4]]; alt["processed_per_frame"] = [int(v) for v in processed[:4]]
        out["B%d" % B] = alt
        for k in kfs:
            k.close()
    mp.close(); ex.close()
    return dict(shape=dict(W=W, H=H, nfeatures=NF, th_depth=float(TH), max_points=MAXP, keeps_every=5), rows=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement)")
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    lib = _lib.OrbxLib(a.lib) if a.lib else None
    out = dict(reps=a.reps, **bench(lib, [int(v) for v in a.batches.split(",")], a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
