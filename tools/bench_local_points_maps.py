"""Tracking::SearchLocalPoints for independent streams - every frame of a batch with its OWN local map - in milliseconds per call, blocking
(enqueue + fetch in the row's time), at the two shapes the project is benchmarked on: 640 x 480, 1000 features, uRight from a depth image (the rgbd
configuration) and 512 x 512, 1500 features on the Kannala-Brandt rig; 5 000 points per map; B = 1, 8, 64 frames.  Rows per shape and B:
  (a) maps_batch            orbm_search_local_points_batch_maps / _rig_batch_maps with B distinct maps
  (b) one_frame_batch_loop  what an independent-stream host could do before: B batch calls of ONE frame, each with its own map
      (uRight and the rig's stereo links of a handle cover ONE frame range, so the loop runs frame 0 against the poses and maps of the streams
      that show frame 0's scene, in turn: the same matching work per call as those streams' own frames)
      single_frame_loop     ... or B single-frame calls (orbm_search_local_points_resident; rig: orbm_search_local_points_fisheye, host points),
                            the C call alone, views prebuilt
  (c) one_map_batch         the existing one-map batch over the same frames, every frame against map 0
      maps_batch_copies     the new call with B separately uploaded COPIES of map 0 and B copies of its flags: exactly the work of (c), so
                            maps_batch_copies / one_map_batch is what the per-frame table, the per-frame flag upload and B sets instead of one cost
The frames show NSCENES scenes in turn (frame b = scene b % NSCENES), each stream under its own pose with its own map, so in (c) only the frames
of scene 0 find many matches: (a)/(c) compares calls, not equal work - the match counts are in the rows.
Warm-up, then median and p10 / p90 over the repetitions; ratios (a)/(b), (a)/(c); prints one JSON line.
Usage: python tools/bench_local_points_maps.py [--out profiles/local_points_maps/bench.json] [--reps 20] [--lib other_build.so] [--batches 1,8,64]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from orb_slam3_detailed_comments_amd import ORBextractor, sophus, synth, views  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402
from bench_rig_tracking import KB_CAM1, KB_CAM2, KB_RLR, KB_TLR, rig_pose, unproject  # noqa: E402
from test_local_points import _rot, FX, FY, CX, CY  # noqa: E402

NPTS = 5000; NSCENES = 8; MBF = 40.0


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)))


def flip_bits(rng, desc, nbits=8):
    fl = rng.integers(0, 256, (len(desc), nbits))
    for j in range(nbits):
        desc[np.arange(len(desc)), fl[:, j] >> 3] ^= (1 << (fl[:, j] & 7)).astype(np.uint8)
    return desc


def finish_map(rng, Xc, T, desc, octv):
    """camera-1 coordinates -> the fields of a local map seen from pose T"""
    R = T.rotationMatrix().astype(np.float64); t = np.asarray(T.translation(), np.float64)
    pos = (R.T @ (Xc - t).T).T
    dvec = pos - np.asarray(T.inverse().translation(), np.float64); dn = np.linalg.norm(dvec, axis=1)
    maxd = dn * 1.2 ** octv * 1.2
    return dict(pos=pos.astype(np.float32), normal=(dvec / dn[:, None]).astype(np.float32), mind=(maxd / 1.2 ** 7).astype(np.float32), maxd=maxd.astype(np.float32),
                desc=flip_bits(rng, desc), bad=(rng.uniform(size=len(pos)) < 0.03).astype(np.uint8), obs=(rng.uniform(size=len(pos)) < 0.9).astype(np.uint8))


def finish_rows(B, r):
    for k in ("maps_batch", "maps_batch_copies", "one_frame_batch_loop", "single_frame_loop", "one_map_batch"):
        r[k]["ms_per_frame"] = r[k]["ms"] / B
    r["a_over_b"] = r["maps_batch"]["ms"] / min(r["one_frame_batch_loop"]["ms"], r["single_frame_loop"]["ms"])
    r["a_over_c"] = r["maps_batch"]["ms"] / r["one_map_batch"]["ms"]
    r["copies_over_c"] = r["maps_batch_copies"]["ms"] / r["one_map_batch"]["ms"]
    r["c_spread_p90_over_p10"] = r["one_map_batch"]["p90"] / r["one_map_batch"]["p10"]
    return r


def same_scene_streams(B, bmax):
    """for the one-frame loop: B streams that show frame 0's scene (b % NSCENES == 0), in turn"""
    return [(i * NSCENES) % bmax for i in range(B)]


def bench_rgbd(lib, batches, reps):
    W, H, NF = 640, 480, 1000
    bmax = max(batches)
    rng = np.random.default_rng(5)
    imgs = [synth.corner_field(W, H, seed=500 + s, nrect=2500) for s in range(NSCENES)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([imgs[b % NSCENES] for b in range(bmax)]))
    depth = (2.0 + np.sin(np.arange(W)[None, :] / 50.0) + np.cos(np.arange(H)[:, None] / 40.0)).astype(np.float32)
    M.ComputeStereoFromRGBD(ex, np.broadcast_to(depth, (bmax, H, W)).copy(), MBF)
    u, _, _ = M.StereoFetch(ex, bmax)
    sfs = ex.GetScaleFactors(); cam = (FX, FY, CX, CY); bounds = (0.0, float(W), 0.0, float(H))
    poses = [sophus.SE3f(_rot(*rng.normal(0, 0.004, 3)), rng.normal(0, 0.01, 3).astype(np.float32)) for _ in range(bmax)]
    maps = []
    for b in range(bmax):                      # stream b's map: points on the rays of ITS frame's keypoints at the depth image's depth
        k, d = res[b][1], res[b][2]
        j = rng.integers(0, len(k), NPTS)
        z = depth[k["y"][j].astype(int), k["x"][j].astype(int)].astype(np.float64)
        Xc = np.stack([(k["x"][j] - CX) / FX * z, (k["y"][j] - CY) / FY * z, z], 1)
        maps.append(finish_map(rng, Xc, poses[b], d[j].copy(), k["octave"][j].astype(np.float64)))
    rps = [M.ResidentPoints(ex, m["pos"], m["normal"], m["mind"], m["maxd"], m["desc"]) for m in maps]
    copies = [M.ResidentPoints(ex, maps[0]["pos"], maps[0]["normal"], maps[0]["mind"], maps[0]["maxd"], maps[0]["desc"]) for _ in range(bmax)]
    L = ex._lib
    singles = []
    for b in range(bmax):
        n = len(res[b][1]); m = maps[b]
        fv = views.frame_view(res[b][1], res[b][2], sfs, W, H, u_right=u[b, :n], mbf=MBF)
        singles.append(M.SearchLocalPoints(ex, fv, poses[b], None, cam, bounds, MBF, sfs, m["pos"], m["normal"], m["mind"], m["maxd"], m["bad"], m["obs"], m["desc"], 0.5, 3.0,
                                           prepared=True, resident=rps[b]))
    out = {}
    for B in batches:
        many = M.LocalPointsBatch(ex, rps[:B], B, cam, bounds, MBF, sfs); many.set_poses(poses[:B])
        one = M.LocalPointsBatch(ex, rps[0], B, cam, bounds, MBF, sfs); one.set_poses(poses[:B])
        cop = M.LocalPointsBatch(ex, copies[:B], B, cam, bounds, MBF, sfs); cop.set_poses(poses[:B])
        ones = []
        for j in same_scene_streams(B, bmax):
            o = M.LocalPointsBatch(ex, rps[j], 1, cam, bounds, MBF, sfs); o.set_poses(poses[j:j + 1]); ones.append((o, maps[j]))
        bads = [m["bad"] for m in maps[:B]]; obss = [m["obs"] for m in maps[:B]]

        def a_fn():
            many.enqueue(0, is_bad=bads, has_obs=obss, th=3.0); many.fetch()

        def a2_fn():
            cop.enqueue(0, is_bad=[bads[0]] * B, has_obs=[obss[0]] * B, th=3.0); cop.fetch()

        def b_fn():
            for o, m in ones:
                o.enqueue(0, is_bad=m["bad"], has_obs=m["obs"], th=3.0); o.fetch()

        def single_fn():
            for call in singles[:B]:
                L.check(call())

        def c_fn():
            one.enqueue(0, is_bad=bads[0], has_obs=obss[0], th=3.0); one.fetch()
        r = finish_rows(B, dict(maps_batch=timed(a_fn, reps), maps_batch_copies=timed(a2_fn, reps), one_frame_batch_loop=timed(b_fn, reps),
                                single_frame_loop=timed(single_fn, max(3, reps // 4), warm=1), one_map_batch=timed(c_fn, reps)))
        r["matches"] = dict(maps_batch=int(many.nm.sum()), maps_batch_copies=int(cop.nm.sum()), one_map_batch=int(one.nm.sum()),
                            one_frame_batch_loop=int(sum(int(o.nm[0]) for o, _ in ones)))
        out["B%d" % B] = r
    for r in rps + copies:
        r.close()
    ex.close()
    return dict(shape=dict(W=W, H=H, nfeatures=NF, map_points=NPTS, scenes=NSCENES), rows=out)


def bench_rig(lib, batches, reps):
    W = H = 512; NF = 1500; LAP = (0, 511)
    bmax = max(batches)
    rng = np.random.default_rng(3)
    Tlr = sophus.SE3f(KB_RLR, KB_TLR); Trl = Tlr.inverse()
    Rlr, tlr = Tlr.rotationMatrix().astype(np.float64), np.asarray(KB_TLR, np.float64)
    pairs = [synth.stereo_pair(W, H, seed=60 + s, nrect=2000, max_disp=24, band=64) for s in range(NSCENES)]
    scene = [b % NSCENES for b in range(bmax)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([pairs[s][0] for s in scene] + [pairs[s][1] for s in scene]), LAP)
    link = lambda n: M.ComputeStereoFishEyeMatches(ex, ex, KB_CAM1, KB_CAM2, Tlr.rotationMatrix(), KB_TLR, 0, bmax, n)
    st = link(bmax)
    sfs = ex.GetScaleFactors(); bounds = (0.0, float(W), 0.0, float(H))
    poses = [sophus.SE3f(_rot(*rng.normal(0, 0.015, 3)), rng.normal(0, 0.1, 3).astype(np.float32)) for _ in range(bmax)]
    rposes = [rig_pose(T, Trl, Tlr) for T in poses]
    maps = []
    for b in range(bmax):                      # stream b's map: points on the rays of ITS left and right keypoints
        kl, dl, kr, dr = res[b][1], res[b][2], res[bmax + b][1], res[bmax + b][2]
        right = rng.uniform(size=NPTS) < 0.5
        jl = rng.integers(0, len(kl), NPTS); jr = rng.integers(0, len(kr), NPTS); z = rng.uniform(0.8, 10.0, NPTS)
        XcL = unproject(KB_CAM1, kl["x"][jl], kl["y"][jl]) * z[:, None]
        XcR = (Rlr @ (unproject(KB_CAM2, kr["x"][jr], kr["y"][jr]) * z[:, None]).T).T + tlr
        Xc = np.where(right[:, None], XcR, XcL)
        desc = np.where(right[:, None], dr[jr], dl[jl]).copy()
        octv = np.where(right, kr["octave"][jr], kl["octave"][jl]).astype(np.float64)
        maps.append(finish_map(rng, Xc, poses[b], desc, octv))
    rps = [M.ResidentPoints(ex, m["pos"], m["normal"], m["mind"], m["maxd"], m["desc"]) for m in maps]
    copies = [M.ResidentPoints(ex, maps[0]["pos"], maps[0]["normal"], maps[0]["mind"], maps[0]["maxd"], maps[0]["desc"]) for _ in range(bmax)]
    L = ex._lib
    singles = []
    for b in range(bmax):
        kl, dl, kr, dr = res[b][1], res[b][2], res[bmax + b][1], res[bmax + b][2]; m = maps[b]
        f2 = views.fisheye_frame_view(views.frame_view(kl, dl, sfs, W, H), views.frame_view(kr, dr, sfs, W, H), st["l2r"][b, :len(kl)], st["r2l"][b, :len(kr)])
        V, sfv = M.rig_frustum_view(rposes[b], KB_CAM1, KB_CAM2, bounds, sfs)
        P = M._WorldPointView()
        P.M = NPTS; P.pos = m["pos"].ctypes.data; P.normal = m["normal"].ctypes.data; P.min_distance = m["mind"].ctypes.data; P.max_distance = m["maxd"].ctypes.data
        P.is_bad = m["bad"].ctypes.data; P.has_obs = m["obs"].ctypes.data; P.desc = m["desc"].ctypes.data
        singles.append((f2, V, sfv, P, np.full(len(kl) + len(kr), -1, np.int32), C.c_int()))
    out = {}
    for B in batches:
        link(B)
        many = M.LocalPointsRigBatch(ex, ex, rps[:B], B, KB_CAM1, KB_CAM2, bounds, sfs, 0, bmax); many.set_poses(rposes[:B])
        one = M.LocalPointsRigBatch(ex, ex, rps[0], B, KB_CAM1, KB_CAM2, bounds, sfs, 0, bmax); one.set_poses(rposes[:B])
        cop = M.LocalPointsRigBatch(ex, ex, copies[:B], B, KB_CAM1, KB_CAM2, bounds, sfs, 0, bmax); cop.set_poses(rposes[:B])
        bads = [m["bad"] for m in maps[:B]]; obss = [m["obs"] for m in maps[:B]]

        def a_fn():
            many.enqueue(is_bad=bads, has_obs=obss, th=3.0); many.fetch()

        def a2_fn():
            cop.enqueue(is_bad=[bads[0]] * B, has_obs=[obss[0]] * B, th=3.0); cop.fetch()

        def c_fn():
            one.enqueue(is_bad=bads[0], has_obs=obss[0], th=3.0); one.fetch()

        def single_fn():
            for f2, V, _, P, asg, nmv in singles[:B]:
                L.check(L.L.orbm_search_local_points_fisheye(ex._h, f2.ref(), C.byref(V), C.byref(P), 0.5, 3.0, 0, 50.0, 0.8, None, None, asg.ctypes.data, C.byref(nmv)))
        r = dict(maps_batch=timed(a_fn, reps), maps_batch_copies=timed(a2_fn, reps), one_map_batch=timed(c_fn, reps), single_frame_loop=timed(single_fn, max(3, reps // 4), warm=1))
        matches = dict(maps_batch=int(many.nm.sum()), maps_batch_copies=int(cop.nm.sum()), one_map_batch=int(one.nm.sum()))
        link(1)                                 # the links now cover frame 0 alone
        ones = []
        for j in same_scene_streams(B, bmax):
            o = M.LocalPointsRigBatch(ex, ex, rps[j], 1, KB_CAM1, KB_CAM2, bounds, sfs, 0, bmax); o.set_poses(rposes[j:j + 1]); ones.append((o, maps[j]))

        def b_fn():
            for o, m in ones:
                o.enqueue(is_bad=m["bad"], has_obs=m["obs"], th=3.0); o.fetch()
        r["one_frame_batch_loop"] = timed(b_fn, reps)
        matches["one_frame_batch_loop"] = int(sum(int(o.nm[0]) for o, _ in ones))
        finish_rows(B, r)["matches"] = matches
        out["B%d" % B] = r
    for r in rps + copies:
        r.close()
    ex.close()
    return dict(shape=dict(W=W, H=H, nfeatures=NF, lapping=list(LAP), map_points=NPTS, scenes=NSCENES), rows=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement)")
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    lib = _lib.OrbxLib(a.lib) if a.lib else None
    batches = [int(v) for v in a.batches.split(",")]
    out = dict(reps=a.reps, rgbd=bench_rgbd(lib, batches, a.reps), rig=bench_rig(lib, batches, a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
