"""The Sim3 projection search of one map-point set from K key frames (LoopClosing::FindMatchesByProjection and the covisible-key-frame verification of
DetectCommonRegionsFromBoW): orbm_search_by_projection_sim3_batch over resident key frames and a resident point set, beside the single-key-frame route called
once per key frame - orbm_project_points, MapPoint::PredictScale on the host, orbm_search_by_projection_sim3 with the key frame uploaded again - on the same
data (the scene of tools/bench_fuse_batch.py: every key frame sees most of the points, so the accept loop commits hundreds of matches per key frame; the
scene has one point per keypoint, so at th = 3 next to no point loses its choice to an earlier one - `points_contended_keyframe0` says how many do).

Both routes are timed at the C ABI with every argument record built beforehand; PredictScale of the loop is one vectorised numpy expression per key frame.
Every call is blocking, so the time is the wall clock of the call.  The two routes alternate, round by round, on one machine: 3 warm-up rounds, then the
median (min, max) over `--reps` rounds.  `batch_cold_ms` is the first call on fresh key frames (their grids are built in it).  Before the timing the two
routes are compared on the first key frames with the exact PredictScale (glibc's logf): rows and counts must be equal.
Usage: python tools/bench_sim3_batch.py [--out profiles/sim3_batch/bench.json] [--reps 50] [--shapes 1x3000,6x3000,64x3000]"""
import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_lib as ol                                   # noqa: E402
from test_models import _predict_scale_float              # noqa: E402
from bench_fuse_batch import BOUNDS, CAM, N_KEYS, NLEVELS, SCALE, make_scene       # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, views   # noqa: E402
from orb_slam3_detailed_comments_amd import matcher as M  # noqa: E402
from orb_slam3_detailed_comments_amd.extractor import ORBextractor        # noqa: E402

f32 = np.float32
TH, RATIO = 3.0, 1.5                                      # FindMatchesByProjection: SearchByProjection(pCurrentKF, mScw, vpMapPoints, vpMatchedMapPoints, 3, 1.5) (src/LoopClosing.cc:1265)


def run_shape(lib, ex, rng, K, Mp, reps):
    L = lib.L
    S = make_scene(rng, K, Mp)
    sfs = np.cumprod(np.array([1.0] + [SCALE] * (NLEVELS - 1), f32), dtype=f32); sigma2 = (sfs * sfs).astype(f32)
    libm = C.CDLL("libm.so.6"); libm.logf.restype = C.c_float; libm.logf.argtypes = [C.c_float]
    lsf = f32(libm.logf(f32(SCALE)))
    # ---- the batch: resident key frames, resident points, one table ----
    e32, e1 = np.zeros(0, np.uint32), np.zeros(1, np.int32)
    rkfs = [M.ResidentKeyFrame(ex, views.key_frame_view(kf["keys"], kf["desc"], sfs, sigma2, e32, e1, e32, kf["ur"])) for kf in S["kfs"]]
    rp = M.ResidentPoints(ex, S["pos"], S["normal"], S["mind"], S["maxd"], S["desc"])
    specs = [M.sim3_spec(kf["T"], CAM, BOUNDS, lsf) for kf in S["kfs"]]
    T = (views.Sim3Target * K)()
    for k in range(K):
        T[k].kf = rkfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]; T[k].occupied = None          # vpMatchedMapPoints is all NULL on entry (:1263)
    ba = np.full((K, N_KEYS), -1, np.int32); bn = np.zeros(K, np.int32)
    batch = lambda: lib.check(L.orbm_search_by_projection_sim3_batch(ex._h, K, T, rp._p, None, TH, RATIO, N_KEYS, ba.ctypes.data, bn.ctypes.data))
    t0 = time.perf_counter(); batch(); cold = (time.perf_counter() - t0) * 1e3
    # ---- the loop: per key frame project, PredictScale on the host, search (the key frame goes up again) ----
    min_inv = (f32(0.8) * S["mind"]).astype(f32); max_inv = (f32(1.2) * S["maxd"]).astype(f32)
    pin = M._ProjectIn(Mp, S["pos"].ctypes.data, S["normal"].ctypes.data, min_inv.ctypes.data, max_inv.ctypes.data, None)
    out = dict(valid=np.zeros(Mp, np.uint8), u=np.zeros(Mp, f32), v=np.zeros(Mp, f32), ur=np.zeros(Mp, f32), inv_z=np.zeros(Mp, f32), dist=np.zeros(Mp, f32))
    pout = M._ProjectOut(*[out[k].ctypes.data for k in ("valid", "u", "v", "ur", "inv_z", "dist")])
    lvl = np.zeros(Mp, np.int32)
    pview = views.ProjectedPointView(Mp, out["valid"].ctypes.data, out["u"].ctypes.data, out["v"].ctypes.data, None, lvl.ctypes.data, None, S["desc"].ctypes.data)
    fvs = [views.frame_view(kf["keys"], kf["desc"], sfs, 0, 0, kf["ur"], bounds=BOUNDS) for kf in S["kfs"]]
    la = np.full((K, N_KEYS), -1, np.int32); ln = [C.c_int() for _ in range(K)]
    rows = [la[k].ctypes.data for k in range(K)]

    def loop(exact=False, upto=K):
        for k in range(upto):
            lib.check(L.orbm_project_points(ex._h, C.byref(specs[k][0]), C.byref(pin), C.byref(pout)))
            ratio = S["maxd"] / np.maximum(out["dist"], f32(1e-30))
            if exact:
                lvl[:] = _predict_scale_float(ratio, lsf, NLEVELS)
            else:
                np.clip(np.ceil(np.log(ratio) / lsf), 0, NLEVELS - 1, out=ratio); lvl[:] = ratio
            lib.check(L.orbm_search_by_projection_sim3(ex._h, fvs[k].ref(), C.byref(pview), TH, RATIO, rows[k], C.byref(ln[k])))
    check = min(K, 3)
    loop(exact=True, upto=check)
    equal = bool(np.array_equal(la[:check], ba[:check]) and [n.value for n in ln[:check]] == list(bn[:check]))
    # contention the accept loop meets: points that do not get what they would take alone (key frame 0, from the oracle's two searches)
    lib.check(L.orbm_project_points(ex._h, C.byref(specs[0][0]), C.byref(pin), C.byref(pout)))
    lvl[:] = _predict_scale_float(S["maxd"] / np.maximum(out["dist"], f32(1e-30)), lsf, NLEVELS)
    pts0 = views.projected_point_view(out["valid"], out["u"], out["v"], lvl, S["desc"])
    alone = ol.oracle_fuse_candidates(fvs[0], pts0, TH, None)[0]
    took = np.full(Mp, -1, np.int32); hit = np.flatnonzero(ba[0] >= 0); took[ba[0][hit]] = hit
    contended = int(((alone >= 0) & (took != alone)).sum())       # (of the points whose choice alone is within TH_LOW: the oracle's Fuse search knows no ratio)
    tb, tl = [], []
    for r in range(3 + reps):                                      # the routes alternate; the first 3 rounds warm up
        t0 = time.perf_counter(); batch(); t1 = time.perf_counter(); loop(); t2 = time.perf_counter()
        if r >= 3:
            tb.append((t1 - t0) * 1e3); tl.append((t2 - t1) * 1e3)
    med = lambda t: float(np.median(t))
    row = dict(K=K, M=Mp, N=N_KEYS, matches=int(bn.sum()), points_contended_keyframe0=contended, rows_equal_exact_predict_scale=equal, rows_checked=check,
               batch_ms=med(tb), batch_min_max=(min(tb), max(tb)), batch_cold_ms=cold, loop_ms=med(tl), loop_min_max=(min(tl), max(tl)), loop_ms_per_keyframe=med(tl) / K,
               loop_over_batch=med(tl) / med(tb), rounds=reps)
    for o in rkfs + [rp]:
        o.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shapes", default="1x3000,6x3000,64x3000")
    ap.add_argument("--emu", action="store_true", help="rehearsal on the CPU emulator build (tests/emu): checks the script, its times mean nothing")
    a = ap.parse_args()
    lib = _lib.OrbxLib(ol.emu_lib_path()) if a.emu else _lib.load_hip()
    ex = ORBextractor(1000, SCALE, NLEVELS, 20, 7, lib=lib)
    rng = np.random.default_rng(13)
    run_shape(lib, ex, rng, 2, 200, 3)                       # code objects, pinned buffers
    rows = []
    for sh in a.shapes.split(","):
        K, Mp = [int(x) for x in sh.split("x")]
        row = run_shape(lib, ex, rng, K, Mp, a.reps if K <= 8 else max(10, a.reps // 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(tool="tools/bench_sim3_batch.py", library="emulator (rehearsal)" if a.emu else "liborbx_hip.so", host=platform.node(), cpus=os.cpu_count(),
               timing="wall clock of blocking calls at the C ABI; batch and loop alternate round by round, median after 3 warm-up rounds; "
                      "loop = orbm_project_points + numpy PredictScale + orbm_search_by_projection_sim3 per key frame",
               th=TH, ratio_hamming=RATIO, occupied="none (vpMatched is all NULL on entry, as in FindMatchesByProjection)", rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ex.close()


if __name__ == "__main__":
    main()
