"""Tracking::UpdateLocalPoints on the device (orbm_map_local_points) in front of the batched SearchLocalPoints, in milliseconds per call, blocking, against
the route a host had before: a new orbm_points per frame and stream.  Shape: 640 x 480, 1000 features, uRight from a depth image; a store of 100 000
slots; per stream 80 key-frame rows of 1000 features, 60 % filled, overlapping so that the local map has about 5 000 points; 300 seen slots; B = 1, 8,
64 streams.  The store holds NMAPS = 16 distinct local maps (80 000 slots, the rest filler): stream b tracks map b % 16 from that map's pose.
Rows per B:
  (a) build                 orbm_map_local_points alone
  (b) build_search          (a) + orbm_map_set_fetch of every set (the seen flags are the search's is_bad, the slots the way back to the MapPoint)
                            + orbm_search_local_points_batch_maps on the map's sets + its fetch
  (c) create_search         B x orbm_points_create from arrays the host has gathered beforehand + the same search + B x orbm_points_destroy
      host_walk_gather      the host's own list walk and gather for (c), in numpy (first occurrence over the concatenated rows, fancy indexing of five
                            arrays): NOT part of (c)
  (d) map_search            (a) + orbm_search_local_points_batch_map on the map's sets + orbm_search_local_points_fetch_slots: no set fetch, no flag
                            array, no table, and the answer in slots
      update_200            orbm_map_update of 200 points;  set_keyframe: orbm_map_set_keyframe of one row of 1000
Both (b) and (c) build their OrbmFrameMap table inside the timed call.  Warm-up, then median and p10 / p90 over the repetitions; prints one JSON line.
"alternating": (b), (c) and (d) timed in ONE loop, one call of each inside every repetition, so that whatever drifts during the run drifts under all three;
d_over_b and d_over_c are ratios of those medians.  The routes' results are asserted equal first ((d)'s slots = the lists' slots at (b)'s positions).
Usage: python tools/bench_local_map_build.py [--out profiles/local_map_build/bench.json] [--reps 20] [--lib other_build.so] [--batches 1,8,64]"""
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
from orb_slam3_detailed_comments_amd import ORBextractor, sophus, synth  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402
from bench_local_points_maps import timed, finish_map, NPTS, NSCENES, MBF  # noqa: E402
from test_local_points import _rot, FX, FY, CX, CY  # noqa: E402

SLOTS = 100000; NMAPS = 16; KF_PER_STREAM = 80; ROW = 1000; FILLED = 600; NSEEN = 300


def host_list(rows_cat, good):
    """the host's UpdateLocalPoints over the concatenated rows: first occurrence of every good slot, in visiting order"""
    s = rows_cat[rows_cat >= 0]
    s = s[good[s]]
    _, first = np.unique(s, return_index=True)
    return s[np.sort(first)]


def alternating(fns, reps, warm=3):
    """{name: median / p10 / p90 in ms} of the routes, one call of each inside every repetition"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    t = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter(); fn(); t[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(ms=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90))) for name, v in t.items()}


def bench(lib, batches, reps):
    W, H, NF = 640, 480, 1000
    bmax = max(batches)
    rng = np.random.default_rng(5)
    imgs = [synth.corner_field(W, H, seed=500 + s, nrect=2500) for s in range(NSCENES)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    nfr = max(bmax, NSCENES)                           # (the maps are made from frames 0 .. NSCENES - 1)
    res = ex.extract_batch(np.stack([imgs[b % NSCENES] for b in range(nfr)]))
    depth = (2.0 + np.sin(np.arange(W)[None, :] / 50.0) + np.cos(np.arange(H)[:, None] / 40.0)).astype(np.float32)
    M.ComputeStereoFromRGBD(ex, np.broadcast_to(depth, (nfr, H, W)).copy(), MBF)
    sfs = ex.GetScaleFactors(); cam = (FX, FY, CX, CY); bounds = (0.0, float(W), 0.0, float(H))
    map_pose = [sophus.SE3f(_rot(*rng.normal(0, 0.004, 3)), rng.normal(0, 0.01, 3).astype(np.float32)) for _ in range(NMAPS)]
    # the store: NMAPS local maps at permuted slots (map j: points on the rays of the keypoints of a frame of scene j % NSCENES), filler in the rest
    perm = rng.permutation(SLOTS).astype(np.int32)
    f = dict(pos=rng.normal(0, 5, (SLOTS, 3)).astype(np.float32), normal=rng.normal(0, 1, (SLOTS, 3)).astype(np.float32), mind=np.full(SLOTS, 0.1, np.float32),
             maxd=np.full(SLOTS, 50.0, np.float32), desc=rng.integers(0, 256, (SLOTS, 32), dtype=np.uint8))
    bad = rng.uniform(size=SLOTS) < 0.03
    rows, map_rows, map_slots = [], [], []
    for j in range(NMAPS):
        k, d = res[j % NSCENES][1], res[j % NSCENES][2]
        i = rng.integers(0, len(k), NPTS)
        z = depth[k["y"][i].astype(int), k["x"][i].astype(int)].astype(np.float64)
        Xc = np.stack([(k["x"][i] - CX) / FX * z, (k["y"][i] - CY) / FY * z, z], 1)
        m = finish_map(rng, Xc, map_pose[j], d[i].copy(), k["octave"][i].astype(np.float64))
        sl = perm[j * NPTS:(j + 1) * NPTS]
        for name in f:
            f[name][sl] = m[name]
        map_slots.append(sl)
        mine = []
        for _ in range(KF_PER_STREAM):                 # a key frame of the map's neighbourhood: 60 % of its features hold one of the map's points
            row = np.full(ROW, -1, np.int32)
            row[rng.choice(ROW, FILLED, replace=False)] = rng.choice(sl, FILLED, replace=False)
            mine.append(len(rows)); rows.append(row)
        map_rows.append(mine[::-1])
    mp = M.ResidentMap(ex, SLOTS, len(rows), ROW, bmax)
    every = np.arange(SLOTS, dtype=np.int32)
    mp.update(every, f["pos"], f["normal"], f["mind"], f["maxd"], f["desc"], bad)
    for r, row in enumerate(rows):
        mp.set_keyframe(r, row)
    L = ex._lib
    ptr = lambda a: a.ctypes.data
    out = {}
    for B in batches:
        frames = [map_rows[b % NMAPS] for b in range(B)]
        seen = [rng.choice(map_slots[b % NMAPS], NSEEN).astype(np.int32) for b in range(B)]
        poses = [map_pose[b % NMAPS] for b in range(B)]
        ks = np.cumsum([0] + [len(r) for r in frames]).astype(np.int32); kr = np.concatenate(frames).astype(np.int32)
        ss = np.cumsum([0] + [len(s) for s in seen]).astype(np.int32); sl = np.concatenate(seen).astype(np.int32)
        Mo = np.zeros(B, np.int32)
        slots_buf = [np.zeros(NPTS + 64, np.int32) for _ in range(B)]; seen_buf = [np.zeros(NPTS + 64, np.uint8) for _ in range(B)]

        def a_fn():
            L.check(L.L.orbm_map_local_points(ex._h, mp._m, B, ptr(ks), ptr(kr), ptr(ss), ptr(sl), ptr(Mo)))

        def search(sets, flags):
            lp = M.LocalPointsBatch(ex, sets, B, cam, bounds, MBF, sfs)
            lp.views = views
            lp.enqueue(0, is_bad=flags, has_obs=None, th=3.0)
            return lp.fetch()

        proto = M.LocalPointsBatch(ex, [None] * B, B, cam, bounds, MBF, sfs); proto.set_poses(poses)
        views = proto.views                            # the poses do not change between repetitions: their views are built once, for both routes

        def b_fn():
            a_fn()
            sets, flags = [], []
            for b in range(B):
                L.check(L.L.orbm_map_set_fetch(ex._h, mp._m, b, ptr(slots_buf[b]), ptr(seen_buf[b])))
                sets.append(mp.set(b)); flags.append(seen_buf[b][:Mo[b]])
            return search(sets, flags)
        # the route without the map: what the host has walked and gathered goes up as a new set per stream
        good = ~bad
        lists = [host_list(np.concatenate([rows[r] for r in fr]), good) for fr in frames]
        gathered = [tuple(np.ascontiguousarray(f[name][ls]) for name in ("pos", "normal", "mind", "maxd", "desc")) for ls in lists]
        flags_c = [np.isin(ls, s).astype(np.uint8) for ls, s in zip(lists, seen)]

        def c_fn():
            rps = [M.ResidentPoints(ex, *g) for g in gathered]
            r = search(rps, flags_c)
            for p in rps:
                p.close()
            return r

        def host_fn():
            for fr in frames:
                ls = host_list(np.concatenate([rows[r] for r in fr]), good)
                for name in ("pos", "normal", "mind", "maxd", "desc"):
                    np.ascontiguousarray(f[name][ls])
        # the two routes search the same lists and find the same matches
        asg_b, nm_b, _ = b_fn()
        asg_b, nm_b = asg_b.copy(), nm_b.copy()
        for b in range(B):
            assert Mo[b] == len(lists[b]) and np.array_equal(slots_buf[b][:Mo[b]], lists[b]) and np.array_equal(seen_buf[b][:Mo[b]], flags_c[b]), "stream %d: the lists differ" % b
        asg_c, nm_c, _ = c_fn()
        assert np.array_equal(nm_b, nm_c) and np.array_equal(asg_b, asg_c)
        on_map = M.LocalPointsBatch(ex, mp, B, cam, bounds, MBF, sfs)
        on_map.views = views

        def d_fn():
            a_fn()
            on_map.enqueue(0, th=3.0)
            return on_map.fetch_slots()
        asg_d, nm_d, _ = d_fn()
        assert np.array_equal(nm_d, nm_b)
        for b in range(B):
            assert np.array_equal(asg_d[b], np.where(asg_b[b] >= 0, lists[b][np.maximum(asg_b[b], 0)], asg_b[b])), "stream %d: (d)'s slots are not (b)'s points" % b
        alt = alternating(dict(build_search=b_fn, create_search=c_fn, map_search=d_fn), reps)
        alt["d_over_b"] = alt["map_search"]["ms"] / alt["build_search"]["ms"]; alt["d_over_c"] = alt["map_search"]["ms"] / alt["create_search"]["ms"]
        r = dict(build=timed(a_fn, reps), build_search=timed(b_fn, reps), create_search=timed(c_fn, reps), host_walk_gather=timed(host_fn, max(3, reps // 4), warm=1))
        r["b_over_c"] = r["build_search"]["ms"] / r["create_search"]["ms"]
        r["alternating"] = alt
        r["local_map_points"] = [int(v) for v in Mo[:4]]; r["positions_per_stream"] = int(sum(len(rows[x]) for x in frames[0])); r["matches"] = int(nm_b.sum())
        out["B%d" % B] = r
    # (d) keeping the store current
    ids = rng.choice(SLOTS, 200, replace=False).astype(np.int32)
    g = [np.ascontiguousarray(f[name][ids]) for name in ("pos", "normal", "mind", "maxd", "desc")]
    upd = timed(lambda: mp.update(ids, *g), reps)
    kfr = timed(lambda: mp.set_keyframe(3, rows[3]), reps)
    mp.close(); ex.close()
    return dict(shape=dict(W=W, H=H, nfeatures=NF, slots=SLOTS, distinct_maps=NMAPS, rows_per_stream=KF_PER_STREAM, row_features=ROW, row_filled=FILLED, seen=NSEEN),
                rows=out, update_200=upd, set_keyframe=kfr)


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
