"""The three tracking searches around SearchLocalPoints with their points named by slot / key-frame row of the resident map, in milliseconds per blocking
enqueue + fetch, against the host-fed calls.  Shape: 640 x 480, 1000 features, uRight from a depth image, a store of 100 000 slots, cap_last = the
handle's keypoint capacity, B = 1, 8, 64 streams (stream b: frame b % 8 of the extraction, its own points at its own permuted slots).
Per search and B:
  last frame   (a) map        orbm_search_by_projection_lastframe_batch_map + fetch
               (b) host_fed   orbm_search_by_projection_lastframe_batch + fetch on arrays the host has ALREADY gathered
               (c) numpy_gather   the host's gather alone (valid, pos, desc by fancy indexing of its mirror), in numpy: NOT part of (b)
  key frame    the same three for orbm_search_by_projection_keyframe_batch_map / _keyframe_batch (pos, mfMinDistance, mfMaxDistance, desc, valid incl. bad)
  bow          (a) map        orbm_search_by_bow_frames_batch_map
               (b) host_flags orbm_search_by_bow_frames_batch with the flags computed in the timed call from a host mirror of rows and slot states
               (c) numpy_flags    that flag computation alone
Once per run ("resident"), the searches between resident key frames with their flags read from the key frames' rows, each against its host-fed call with
the flags computed in the timed call from the host mirror, as the bow rows above:
  triangulation   orbm_search_for_triangulation_resident_map: key frame 0 against up to 20 neighbours (rule: holds a point)
  bow_keyframes   orbm_search_by_bow_resident_map: key frame 0 paired with up to 8 others, has_map_point1 and eligible2 from rows (rule: holds a good point)
  bow_rig         orbm_search_by_bow_rig_batch_map: the extraction read as rig frames [L .. | R ..], frame p against key frame p
The routes of a search alternate inside every repetition; median and p10 / p90 over the repetitions.  (a) and (b) are asserted to return identical results.
Prints one JSON line.  Usage: python tools/bench_map_rows.py [--out profiles/map_rows/bench.json] [--reps 20] [--lib other_build.so] [--batches 1,8,64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from orb_slam3_detailed_comments_amd import ORBextractor, ORBVocabulary, sophus, synth  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402
from bench_local_points_maps import flip_bits, NSCENES, MBF  # noqa: E402
from test_local_points import _rot, FX, FY, CX, CY  # noqa: E402
import vocab_scenes as vs  # noqa: E402

SLOTS = 100000


def timed_alternating(fns, reps, warm=3):
    """{name: fn} called one after the other inside every repetition -> {name: median / p10 / p90 in ms}"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter(); fn(); t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(ms=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90))) for k, v in t.items()}


def bench(lib, batches, reps):
    W, H, NF = 640, 480, 1000
    bmax = max(batches)
    rng = np.random.default_rng(7)
    imgs = [synth.corner_field(W, H, seed=500 + s, nrect=2500) for s in range(NSCENES)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    res = ex.extract_batch(np.stack([imgs[b % NSCENES] for b in range(bmax)]))
    depth = (2.0 + np.sin(np.arange(W)[None, :] / 50.0) + np.cos(np.arange(H)[:, None] / 40.0)).astype(np.float32)
    M.ComputeStereoFromRGBD(ex, np.broadcast_to(depth, (bmax, H, W)).copy(), MBF)
    sfs = ex.GetScaleFactors(); cam = (FX, FY, CX, CY); bounds = (0.0, float(W), 0.0, float(H))
    cap = ex.max_keypoints()
    header, parent, leaf, vdesc, weight = vs.make_vocabulary(rng, 6, 3)
    voc = ORBVocabulary.from_arrays(ex, header[0], header[1], header[2], header[3], parent, leaf, vdesc, weight)
    voc.transform_extracted(ex, 0, bmax, 2)
    kfs = M.ResidentKeyFrame.from_extracted(ex, voc, np.arange(bmax))         # key frame b = frame b itself: its keypoints' angles, its FeatureVector
    # the host's mirror of the map: every slot holds a point (filler), stream b's points at its own permuted slots
    f = dict(pos=rng.normal(0, 5, (SLOTS, 3)).astype(np.float32), normal=rng.normal(0, 1, (SLOTS, 3)).astype(np.float32), mind=np.full(SLOTS, 0.1, np.float32),
             maxd=np.full(SLOTS, 50.0, np.float32), desc=rng.integers(0, 256, (SLOTS, 32), dtype=np.uint8))
    bad = rng.uniform(size=SLOTS) < 0.03
    perm = rng.permutation(SLOTS).astype(np.int32)
    n = np.zeros(bmax, np.int32); slots = np.full((bmax, cap), -1, np.int32); octave = np.zeros((bmax, cap), np.int32); angle = np.zeros((bmax, cap), np.float32)
    has_obs = np.ones((bmax, cap), np.uint8); excluded = (rng.uniform(size=(bmax, cap)) < 0.05).astype(np.uint8)
    poses = []
    at = 0
    for b in range(bmax):
        k, d = res[b][1], res[b][2]; N = len(k); n[b] = N
        T = sophus.SE3f(_rot(*rng.normal(0, 0.004, 3)), rng.normal(0, 0.01, 3).astype(np.float32)); poses.append(T)
        R = T.rotationMatrix().astype(np.float64); t = np.asarray(T.translation(), np.float64)
        z = depth[k["y"].astype(int), k["x"].astype(int)].astype(np.float64)
        Xc = np.stack([(k["x"] + rng.normal(0, 0.7, N) - CX) / FX * z, (k["y"] + rng.normal(0, 0.7, N) - CY) / FY * z, z], 1)
        pos = (R.T @ (Xc - t).T).T
        dn = np.linalg.norm(pos - np.asarray(T.inverse().translation(), np.float64), axis=1)
        maxd = dn * 1.2 ** k["octave"].astype(np.float64) * 1.1
        sl = perm[at:at + N]; at += N
        f["pos"][sl] = pos; f["maxd"][sl] = maxd; f["mind"][sl] = maxd / 1.2 ** 7; f["desc"][sl] = flip_bits(rng, d.copy())
        slots[b, :N] = np.where(rng.uniform(size=N) < 0.9, sl, -1)
        octave[b, :N] = k["octave"]; angle[b, :N] = k["angle"]
    assert at <= SLOTS
    mp = M.ResidentMap(ex, SLOTS, bmax, cap, 1)
    mp.update(np.arange(SLOTS, dtype=np.int32), f["pos"], f["normal"], f["mind"], f["maxd"], f["desc"], bad)
    for b in range(bmax):
        mp.set_keyframe(b, slots[b, :n[b]])
    rows = np.arange(bmax, dtype=np.int32)
    out = {}
    for B in batches:
        nB, sB, exB = n[:B], slots[:B], excluded[:B]
        inside = np.arange(cap)[None, :] < nB[:, None]

        def gather(read_bad, fields):
            s = np.where(sB >= 0, sB, 0)
            valid = inside & (sB >= 0) & (exB == 0)
            if read_bad:
                valid &= ~bad[s]
            return (valid.astype(np.uint8),) + tuple(np.ascontiguousarray(f[name][s]) for name in fields)
        # SearchByProjection(CurrentFrame, LastFrame)
        lf = M.LastFrameBatch(ex, B, cam, bounds, MBF, sfs); lf.set_poses(poses[:B])
        g_valid, g_pos, g_desc = gather(False, ("pos", "desc"))

        def last_map():
            lf.enqueue_slots(mp, nB, sB, exB, octave[:B], angle[:B], has_obs[:B], 7.0, None, None, True, None, use_u_right=True)
            return lf.fetch()

        def last_host():
            lf.enqueue(nB, g_pos, g_valid, octave[:B], angle[:B], has_obs[:B], g_desc, 7.0, None, None, True, None, use_u_right=True)
            return lf.fetch()
        a = [x.copy() for x in last_map()]; h = last_host()
        assert np.array_equal(a[0], h[0]) and np.array_equal(a[1], h[1]), "last frame: the routes differ"
        r_last = timed_alternating(dict(map=last_map, host_fed=last_host, numpy_gather=lambda: gather(False, ("pos", "desc"))), reps)
        r_last["matches"] = int(a[1].sum())
        # SearchByProjection(CurrentFrame, pKF, sAlreadyFound)
        kb = M.KeyFrameBatch(ex, B, cam, bounds, MBF, sfs); kb.set_poses(poses[:B])
        k_valid, k_pos, k_min, k_max, k_desc = gather(True, ("pos", "mind", "maxd", "desc"))

        def key_map():
            kb.enqueue_rows(mp, rows[:B], kfs[:B], exB, 10.0, 100, True, None)
            return kb.fetch()

        def key_host():
            kb.enqueue(nB, k_pos, k_valid, k_min, k_max, angle[:B], k_desc, 10.0, 100, True, None)
            return kb.fetch()
        a = [x.copy() for x in key_map()]; h = key_host()
        assert np.array_equal(a[0], h[0]) and np.array_equal(a[1], h[1]), "key frame: the routes differ"
        r_key = timed_alternating(dict(map=key_map, host_fed=key_host, numpy_gather=lambda: gather(True, ("pos", "mind", "maxd", "desc"))), reps)
        r_key["matches"] = int(a[1].sum())
        # SearchByBoW(pKF, F)
        voc.transform_extracted(ex, 0, B, 2)
        matcher = M.ORBmatcher(0.7, True)

        def flags():
            return [((sB[b, :nB[b]] >= 0) & ~bad[np.where(sB[b, :nB[b]] >= 0, sB[b, :nB[b]], 0)]).astype(np.uint8) for b in range(B)]
        bow_map = lambda: matcher.SearchByBoWFramesBatch(ex, voc, kfs[:B], None, resident_map=mp, rows=rows[:B])
        bow_host = lambda: matcher.SearchByBoWFramesBatch(ex, voc, kfs[:B], flags())
        a, h = bow_map(), bow_host()
        assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, h)), "bow: the routes differ"
        r_bow = timed_alternating(dict(map=bow_map, host_flags=bow_host, numpy_flags=flags), reps)
        r_bow["matches"] = int(sum(x[0] for x in a))
        for r in (r_last, r_key):
            r["map_over_host_fed"] = r["map"]["ms"] / r["host_fed"]["ms"]
            r["map_over_host_fed_plus_gather"] = r["map"]["ms"] / (r["host_fed"]["ms"] + r["numpy_gather"]["ms"])
        r_bow["map_over_host_flags"] = r_bow["map"]["ms"] / r_bow["host_flags"]["ms"]
        out["B%d" % B] = dict(lastframe=r_last, keyframe=r_key, bow=r_bow)
    resident = {}
    if bmax >= 2:
        row_of = lambda b: slots[b, :n[b]]
        holds = lambda b: (row_of(b) >= 0).astype(np.uint8)                                            # (every slot of this store holds a point)
        good = lambda b: ((row_of(b) >= 0) & ~bad[np.where(row_of(b) >= 0, row_of(b), 0)]).astype(np.uint8)
        same = lambda a, h: all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, h))
        nb = list(range(1, min(bmax, 21)))
        F = np.stack([np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)] * len(nb)); eps = np.stack([np.array([1e6, H / 2], np.float32)] * len(nb))
        m6 = M.ORBmatcher(0.6, True)
        tri_map = lambda: m6.SearchForTriangulationResidentMap(ex, kfs[0], 0, [kfs[j] for j in nb], rows[nb], mp, F, eps, False, True)
        tri_host = lambda: m6.SearchForTriangulationResident(ex, kfs[0], holds(0), [kfs[j] for j in nb], [holds(j) for j in nb], F, eps, False, True)
        assert tri_map() == tri_host(), "triangulation: the routes differ"
        r = timed_alternating(dict(map=tri_map, host_flags=tri_host, numpy_flags=lambda: [holds(j) for j in [0] + nb]), reps)
        r.update(neighbours=len(nb), matches=int(sum(x[0] for x in tri_map())), map_over_host_flags=r["map"]["ms"] / r["host_flags"]["ms"])
        resident["triangulation"] = r
        prs = list(range(1, min(bmax, 9)))
        m7 = M.ORBmatcher(0.7, True)
        kb_map = lambda: m7.SearchByBoWResidentMap(ex, [kfs[0]] * len(prs), [0] * len(prs), [kfs[j] for j in prs], rows[prs], mp, False)
        kb_host = lambda: m7.SearchByBoWResident(ex, [kfs[0]] * len(prs), [good(0)] * len(prs), [kfs[j] for j in prs], [good(j) for j in prs], False)
        assert same(kb_map(), kb_host()), "key-frame bow: the routes differ"
        r = timed_alternating(dict(map=kb_map, host_flags=kb_host, numpy_flags=lambda: [good(j) for j in [0] + prs]), reps)
        r.update(pairs=len(prs), matches=int(sum(x[0] for x in kb_map())), map_over_host_flags=r["map"]["ms"] / r["host_flags"]["ms"])
        resident["bow_keyframes"] = r
        B2 = bmax // 2                                                                                # (last: the rig transform replaces the vocabulary's run)
        voc.transform_rig_extracted(ex, 0, ex, B2, B2, 2)
        fr = np.arange(B2, dtype=np.int32)
        rig_map = lambda: m7.SearchByBoWRigBatch(ex, 0, ex, B2, voc, fr, kfs[:B2], None, resident_map=mp, rows=rows[:B2])
        rig_host = lambda: m7.SearchByBoWRigBatch(ex, 0, ex, B2, voc, fr, kfs[:B2], [good(b) for b in range(B2)])
        assert same(rig_map(), rig_host()), "rig bow: the routes differ"
        r = timed_alternating(dict(map=rig_map, host_flags=rig_host, numpy_flags=lambda: [good(b) for b in range(B2)]), reps)
        r.update(pairs=B2, matches=int(sum(x[0] for x in rig_map())), map_over_host_flags=r["map"]["ms"] / r["host_flags"]["ms"])
        resident["bow_rig"] = r
    for k in kfs:
        k.close()
    mp.close(); voc.close(); ex.close()
    return dict(shape=dict(W=W, H=H, nfeatures=NF, slots=SLOTS, cap_last=cap, keypoints_per_frame=[int(v) for v in n[:4]]), rows=out, resident=resident)


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
