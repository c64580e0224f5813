"""TrackReferenceKeyFrame / Relocalization's BoW step for fisheye-rig frames: milliseconds per frame of the batched device forms against the
single-frame route and the reference, at the TUM-VI shape (512 x 512, 1500 features, lapping {0, 511}, the rig of bench.py --config fisheye) with a
synthetic vocabulary of ORBvoc's shape (k = 10, L = 6, levelsup = 4; tests/vocab_scenes.make_vocabulary_fast).
Rows: orbv_transform_rig_extracted + orbm_search_by_bow_rig_batch at B = 1, 8, 64 (P = B, one rig key frame per frame; both calls in the row's
time, the search blocks); one frame against 20 candidate key frames (Relocalization); the single-frame route per frame (join the two descriptor
sets on the host, the blocking orbv_transform, orbm_search_by_bow_fisheye); the reference's ORBmatcher::SearchByBoW(pKF, F) alone on one host
core (oracle/_ref/libmw_ref.so, its FeatureVectors set from the device transform) when it is built.  Warm-up, then the median (min / max) over
repetitions; prints one JSON line.
Usage: python tools/bench_rig_bow.py [--out profiles/rig_bow/bench_rig_bow.json] [--reps 20]"""
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
from orb_slam3_detailed_comments_amd import ORBextractor, ORBVocabulary, synth, views  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402
import vocab_scenes as vs  # noqa: E402

W = H = 512; NF = 1500; LAP = (0, 511); BMAX = 64; NSCENES = 8; NCAND = 20
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def key_frame(rng, kl, dl, kr, dr, rot=20.0):
    """a rig key frame of the frame's place: 80 % of each camera's features re-observed (descriptor noise, a rotation), 30 clutter features each"""
    kk, dk = [], []
    for k, d in ((kl, dl), (kr, dr)):
        src = np.sort(rng.choice(len(k), int(0.8 * len(k)), replace=False))
        o = np.zeros(len(src) + 30, KP)
        for f in ("x", "y", "size", "octave"):
            o[f][:len(src)] = k[f][src]
        o["angle"][:len(src)] = np.mod(k["angle"][src] + rot + rng.normal(0, 3.0, len(src)), 360.0); o["angle"][len(src):] = rng.uniform(0, 360, 30)
        e = np.concatenate([d[src].copy(), rng.integers(0, 256, (30, 32), dtype=np.uint8)])
        for i in range(len(src)):
            bits = rng.choice(256, int(rng.integers(0, 60)), replace=False)
            e[i, bits >> 3] ^= (1 << (bits & 7)).astype(np.uint8)
        kk.append(o); dk.append(e)
    return np.concatenate(kk), np.concatenate(dk), len(kk[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement)")
    ap.add_argument("--small-vocabulary", action="store_true", help="k = 10, L = 4, levelsup = 2 instead of ORBvoc's shape (functional checks)")
    a = ap.parse_args()
    global LEVELSUP
    LEVELSUP = 2 if a.small_vocabulary else 4          # nodes at level 2 either way (Frame::ComputeBoW: levelsup = 4 on ORBvoc)
    rng = np.random.default_rng(5)
    pairs = [synth.stereo_pair(W, H, seed=160 + s, nrect=2000, max_disp=24, band=64) for s in range(NSCENES)]
    scene = [b % NSCENES for b in range(BMAX)]
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=_lib.OrbxLib(a.lib) if a.lib else None)
    res = ex.extract_batch(np.stack([pairs[s][0] for s in scene] + [pairs[s][1] for s in scene]), LAP)
    sfs = ex.GetScaleFactors()
    t0 = time.perf_counter()
    header, parent, leaf, desc, weight = vs.make_vocabulary_fast(rng, 10, 4 if a.small_vocabulary else 6)
    voc = ORBVocabulary.from_arrays(ex, *header, parent, leaf, desc, weight)
    voc_s = time.perf_counter() - t0
    # one rig key frame per frame, resident, with its FeatureVector from the (same) vocabulary
    kfs, mps, kviews = [], [], []
    for b in range(BMAX):
        kk, dk, nl_k = key_frame(rng, res[b][1], res[b][2], res[BMAX + b][1], res[BMAX + b][2])
        bow = voc.transform(dk, LEVELSUP)
        mp = (rng.uniform(size=len(kk)) < 0.85).astype(np.uint8)
        kv = views.key_frame_view(kk, dk, sfs, sfs * sfs, bow.fv_node, bow.fv_start, bow.fv_feat, None, mp)
        kfs.append(M.ResidentKeyFrame(ex, kv)); mps.append(mp); kviews.append((kv, kk, dk, bow, mp, nl_k))
    n_frame = [len(res[b][1]) + len(res[BMAX + b][1]) for b in range(BMAX)]
    m = M.ORBmatcher(0.7, True)
    out = dict(shape=dict(W=W, H=H, nfeatures=NF, lapping=list(LAP), scenes=NSCENES, vocabulary=dict(k=10, L=int(header[1]), levelsup=LEVELSUP, nodes=len(parent)),
                          features_per_frame=float(np.mean(n_frame))), reps=a.reps, rows={}, vocabulary_build_s=voc_s)
    nm_batch = {}
    for B in (1, 8, 64):
        got = [None]

        def run():
            voc.transform_rig_extracted(ex, 0, ex, BMAX, B, LEVELSUP)
            got[0] = m.SearchByBoWRigBatch(ex, 0, ex, BMAX, voc, list(range(B)), kfs[:B], mps[:B])
        med, mn, mx = timed(run, a.reps)
        nm_batch[B] = [g[0] for g in got[0]]
        out["rows"]["transform_and_bow_rig_batch_B%d" % B] = dict(ms_per_frame=med / B, ms_per_call=med, min_ms=mn, max_ms=mx, matches=int(sum(nm_batch[B])))
    # Relocalization: frame 0 against NCAND candidates (its own place's key frame and others)
    cand = [0] + list(range(1, NCAND))

    def run_reloc():
        voc.transform_rig_extracted(ex, 0, ex, BMAX, 1, LEVELSUP)
        got_r[0] = m.SearchByBoWRigBatch(ex, 0, ex, BMAX, voc, [0] * NCAND, [kfs[c] for c in cand], [mps[c] for c in cand])
    got_r = [None]
    med, mn, mx = timed(run_reloc, a.reps)
    out["rows"]["relocalization_1_frame_x%d_candidates" % NCAND] = dict(ms_per_call=med, ms_per_pair=med / NCAND, min_ms=mn, max_ms=mx,
                                                                         matches=int(sum(g[0] for g in got_r[0])))
    # the single-frame route: host join, blocking transform, single-frame search, per frame
    single = [0] * BMAX

    def run_single():
        for b in range(BMAX):
            rows = np.concatenate([res[b][2], res[BMAX + b][2]])
            keys = np.concatenate([res[b][1], res[BMAX + b][1]])
            bw = voc.transform(rows, LEVELSUP)
            fv = views.key_frame_view(keys, rows, sfs, sfs * sfs, bw.fv_node, bw.fv_start, bw.fv_feat)
            single[b] = m.SearchByBoWFisheye(ex, kviews[b][0], fv, len(res[b][1]))[0]
    med, mn, mx = timed(run_single, max(3, a.reps // 4), warm=1)
    out["rows"]["single_frame_route_loop_64"] = dict(ms_per_frame=med / BMAX, ms_per_loop=med, min_ms=mn, max_ms=mx, matches=int(sum(single)))
    out["batch_equals_single_frame_route"] = nm_batch[64] == single
    # the reference's SearchByBoW alone on one host core
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libmw_ref.so")
    if os.path.exists(ref_path):
        from matcher_world import Driver
        voc.transform_rig_extracted(ex, 0, ex, BMAX, BMAX, LEVELSUP)
        fbows = [voc.fetch(ex, b, n_frame[b]) for b in range(BMAX)]
        t, ref_nm = [], []
        I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        trl = (I3, np.array([-0.1, 0.0, 0.0], np.float32))

        def set_fv(drv, keyframe, fid, bw):
            nodes = np.ascontiguousarray(bw.fv_node, np.uint32); st = np.ascontiguousarray(bw.fv_start, np.int32); ft = np.ascontiguousarray(bw.fv_feat, np.uint32)
            drv.L.mw_set_feat_vec(drv.w, int(keyframe), fid, len(nodes), nodes.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), ft.ctypes.data_as(C.c_void_p))
        for b in range(NSCENES):
            _, kk, dk, bw, mp, nl_k = kviews[b]
            drv = Driver(ref_path)
            cam = drv.camera(); cam2 = drv.camera()
            ids = np.full(len(kk), -1, np.int32)
            for i in np.nonzero(mp)[0]:
                ids[i] = drv.mappoint(np.array([0, 0, 3.0]), np.array([0, 0, 1.0]), 0.5, 30.0, dk[i])
            kid = drv.frame(True, kk[:nl_k], dk, None, I3, Z3, cam, cam2, keys_right=kk[nl_k:], trl=trl)
            set_fv(drv, True, kid, bw); drv.set_map_points(True, kid, ids)
            fid = drv.frame(False, res[b][1], np.concatenate([res[b][2], res[BMAX + b][2]]), None, I3, Z3, cam, cam2, keys_right=res[BMAX + b][1], trl=trl)
            set_fv(drv, False, fid, fbows[b])
            o = np.full(n_frame[b], -1, np.int32)
            for rep in range(4):
                t0 = time.perf_counter()
                n = drv.L.mw_search_by_bow_frame(drv.w, kid, fid, o.ctypes.data_as(C.c_void_p), C.c_float(0.7), 1)
                t.append((time.perf_counter() - t0) * 1e3)
            ref_nm.append(n)
            drv.close()
        out["rows"]["reference_search_by_bow_one_core"] = dict(ms_per_frame=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), frames=len(t),
                                                               note="SearchByBoW alone: the reference's ComputeBoW is not in this row")
        out["reference_equals_batch"] = ref_nm == nm_batch[64][:NSCENES]
    else:
        out["rows"]["reference_search_by_bow_one_core"] = None
    for k in kfs:
        k.close()
    voc.close(); ex.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
