"""Tracking::CreateNewKeyFrame for frames that are on the device: n frames out of an extracted batch of 64 become resident key frames (orbm_keyframe),
in milliseconds per call, blocking, the routes alternating repetition by repetition on one box in one run.
  (a)  fetch_create   what the parent commit offers: orbx_fetch, orbx_fetch_undistorted and orbm_stereo_fetch of the batch, orbv_fetch of each of the n
                      frames (FeatureVector only), then n x orbm_keyframe_create from those host arrays
  (a') create         n x orbm_keyframe_create from host arrays (and views) the host already holds: the uploads alone
  (b)  extracted      one orbm_keyframe_create_extracted(h, v, n, frames, use_u_right = 1)
Shape: 752 x 480, 1200 features, an undistortion model, mvuRight from depth images, a synthetic vocabulary of ORBvoc's shape (k = 10, L = 6,
levelsup = 4; --small-vocabulary: L = 4, levelsup = 2).  The key frames of a repetition are destroyed outside the timed region (every route pays the same
n x hipFree).  The Python around the calls is part of every route: the views of (a) are built per key frame with views.key_frame_view, (b) is one call.
The tool asserts that (a) and (b) leave byte-equal key frames (orbm_keyframe_fetch).  Prints one JSON line.
Usage: python tools/bench_keyframe_promote.py [--out profiles/keyframe_promote/bench.json] [--reps 20] [--lib other_build.so] [--small-vocabulary]"""
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
import vocab_scenes as vs  # noqa: E402
from orb_slam3_detailed_comments_amd import KP_DTYPE, ORBextractor, ORBVocabulary, synth, views  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402

W, H, NF, B = 752, 480, 1200, 64
NS = (1, 8, 64)


def stats(t):
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement)")
    ap.add_argument("--small-vocabulary", action="store_true")
    a = ap.parse_args()
    lib = _lib.OrbxLib(a.lib) if a.lib else None
    rng = np.random.default_rng(7)
    levelsup = 2 if a.small_vocabulary else 4
    header, parent, leaf, desc, weight = vs.make_vocabulary_fast(rng, 10, 4 if a.small_vocabulary else 6)
    ex = ORBextractor(NF, 1.2, 8, 20, 7, lib=lib)
    L = ex._lib
    ex.set_undistort((0.8 * W, 0.8 * W, W / 2 + 1.5, H / 2 - 2.0), (-0.28, 0.07, 2e-4, 1e-4, 0.0))
    voc = ORBVocabulary.from_arrays(ex, *header, parent, leaf, desc, weight)
    scenes = [synth.corner_field(W, H, seed=700 + s, nrect=3000) for s in range(8)]
    imgs = np.stack([np.roll(scenes[b % 8], 3 * (b // 8), axis=1) for b in range(B)])
    depth = rng.uniform(0.5, 6.0, (B, H, W)).astype(np.float32)
    ex.enqueue(imgs)
    M.ComputeStereoFromRGBD(ex, depth, 40.0)
    voc.transform_extracted(ex, 0, B, levelsup)
    ex.sync()
    cap = ex.max_keypoints()
    sfs, sig = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    kps = np.zeros((B, cap), KP_DTYPE); kun = np.zeros((B, cap), KP_DTYPE); dsc = np.zeros((B, cap, 32), np.uint8)
    nk = np.zeros(B, np.int32); mono = np.zeros(B, np.int32)
    ur = np.zeros((B, cap), np.float32); dep = np.zeros((B, cap), np.float32); nst = np.zeros(B, np.int32)
    fvn = np.zeros((B, cap), np.uint32); fvs = np.zeros((B, cap + 1), np.int32); fvf = np.zeros((B, cap), np.uint32); nfv = np.zeros(B, np.int32)

    def fetch_all(frames):
        L.check(L.L.orbx_fetch(ex._h, kps.ctypes.data, dsc.ctypes.data, cap, nk.ctypes.data, mono.ctypes.data))
        L.check(L.L.orbx_fetch_undistorted(ex._h, kun.ctypes.data, cap))
        L.check(L.L.orbm_stereo_fetch(ex._h, B, ur.ctypes.data, dep.ctypes.data, cap, nst.ctypes.data))
        n = C.c_int()
        for b in frames:
            L.check(L.L.orbv_fetch(voc._v, ex._h, int(b), None, None, 0, None, None, None, fvn[b].ctypes.data, fvs[b].ctypes.data, fvf[b].ctypes.data, C.byref(n)))
            nfv[b] = n.value

    def make_views(frames):
        out = []
        for b in frames:
            N, nn = int(nk[b]), int(nfv[b])
            out.append(views.key_frame_view(kun[b, :N], dsc[b, :N], sfs, sig, fvn[b, :nn], fvs[b, :nn + 1], fvf[b, :int(fvs[b, nn])], ur[b, :N], None))
        return out

    def create(vws):
        out = []
        for v in vws:
            h = C.c_void_p()
            L.check(L.L.orbm_keyframe_create(ex._h, v.ref(), C.byref(h)))
            out.append(h)
        return out

    def extracted(fr):
        out = (C.c_void_p * len(fr))()
        L.check(L.L.orbm_keyframe_create_extracted(ex._h, voc._v, len(fr), fr.ctypes.data, 1, out))
        return [C.c_void_p(out[j]) for j in range(len(fr))]

    def destroy(hs):
        for h in hs:
            L.L.orbm_keyframe_destroy(h)

    def read(h):
        kf = M.ResidentKeyFrame._adopt(L, h.value, ex)
        r = kf.fetch(ex)
        kf._kf = None                                              # the caller destroys it
        return r
    result = dict(shape=dict(W=W, H=H, nfeatures=NF, batch=B, vocabulary=dict(k=10, L=int(header[1]), levelsup=levelsup, nodes=len(parent))), reps=a.reps, n={})
    fetch_all(range(B))
    result["features_per_frame"] = dict(min=int(nk.min()), mean=float(nk.mean()), max=int(nk.max()))
    for n in NS:
        fr = np.ascontiguousarray(rng.permutation(B)[:n], np.int32)
        # both routes leave the same key frames
        fetch_all(fr)
        ka = create(make_views(fr)); kb = extracted(fr)
        nbytes = 0
        for x, y in zip(ka, kb):
            rx, ry = read(x), read(y)
            for k in rx:
                assert rx[k].shape == ry[k].shape and rx[k].tobytes() == ry[k].tobytes(), (n, k)
                nbytes += rx[k].nbytes
            assert len(rx["fv_node"]) > 0 and (rx["u_right"] >= 0).any()
        destroy(ka); destroy(kb)
        vws = make_views(fr)
        ta, tc, tb = [], [], []
        for it in range(-3, a.reps):                               # three warm-up rounds; the routes alternate
            t0 = time.perf_counter(); fetch_all(fr); ka = create(make_views(fr)); t1 = time.perf_counter()
            kc = create(vws); t2 = time.perf_counter()
            kb = extracted(fr); t3 = time.perf_counter()
            destroy(ka); destroy(kc); destroy(kb)
            if it >= 0:
                ta.append((t1 - t0) * 1e3); tc.append((t2 - t1) * 1e3); tb.append((t3 - t2) * 1e3)
        r = dict(fetch_create=stats(ta), create=stats(tc), extracted=stats(tb), key_frame_bytes=nbytes)
        r["b_over_a"] = r["extracted"]["ms"] / r["fetch_create"]["ms"]; r["b_over_a_prime"] = r["extracted"]["ms"] / r["create"]["ms"]
        result["n"][str(n)] = r
    voc.close(); ex.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
