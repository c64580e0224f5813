"""Fusing one map-point set into K key frames (LocalMapping::SearchInNeighbors, LoopClosing::SearchAndFuse): orbm_fuse_candidates_batch over resident key frames
and a resident point set, beside the single-key-frame route called once per key frame - orbm_project_points, MapPoint::PredictScale on the host,
orbm_fuse_candidates with the key frame uploaded again - over the same data, and the CPU oracle's candidate search on one core (oracle_fuse_candidates per key
frame, fed with the projections: the search alone, without the geometry in front of it).

Both routes are timed at the C ABI with every argument record built beforehand (the ctypes wrappers of matcher.py cost more per call than a round trip and
would be charged to the loop K times); PredictScale of the loop is one vectorised numpy expression per key frame.  Every call is blocking, so the time is the
wall clock of the call: warm-up, then the median (min, max) of `--reps` repetitions.  `batch_cold_ms` is the first call on fresh key frames (their grids are
built in it).  Before the timing the two routes are compared on the first key frames with the exact PredictScale (glibc's logf): the rows must be equal.
Usage: python tools/bench_fuse_batch.py [--out profiles/fuse_batch/bench_fuse_batch.json] [--reps 50] [--shapes 30x1500,60x2000,200x4000,1x1500,4x1500,8x1500]"""
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
import oracle_lib as ol                                   # noqa: E402
from test_models import _predict_scale_float              # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, views, sophus           # noqa: E402
from orb_slam3_detailed_comments_amd import matcher as M                  # noqa: E402
from orb_slam3_detailed_comments_amd.extractor import ORBextractor        # noqa: E402

f32 = np.float32
CAM = (517.3, 516.5, 318.6, 255.3)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
BF, NLEVELS, SCALE, TH, N_KEYS = 40.0, 8, 1.2, 3.0, 1200


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])).astype(f32)


def make_scene(rng, K, Mp):
    """Mp map points in front of K nearby cameras; every key frame holds N_KEYS keypoints: the projections (+ noise) of the points it sees, with the point's
    descriptor a few bits off, filled up with unrelated keypoints"""
    z = rng.uniform(3.0, 8.0, Mp)
    pos = np.stack([(rng.uniform(20, 620, Mp) - CAM[2]) / CAM[0] * z, (rng.uniform(20, 460, Mp) - CAM[3]) / CAM[1] * z, z], 1)
    octave = rng.integers(0, NLEVELS, Mp)
    dist = np.linalg.norm(pos, axis=1)
    maxd = (dist * SCALE ** (octave + 0.5)).astype(f32); mind = (maxd / f32(SCALE ** (NLEVELS - 1))).astype(f32)
    normal = (pos / dist[:, None]).astype(f32)
    desc = rng.integers(0, 256, (Mp, 32), dtype=np.uint8)
    kfs = []
    for _ in range(K):
        R = rot(*rng.normal(0, 0.02, 3)); t = rng.normal(0, 0.1, 3).astype(f32)
        Xc = (R.astype(np.float64) @ pos.T).T + t
        u = CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2]; v = CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]
        seen = np.flatnonzero((u > 5) & (u < 635) & (v > 5) & (v < 475))
        seen = rng.choice(seen, min(len(seen), N_KEYS * 3 // 4), replace=False)
        k = np.zeros(N_KEYS, _lib.KP_DTYPE); d = rng.integers(0, 256, (N_KEYS, 32), dtype=np.uint8)
        k["x"] = rng.uniform(5, 635, N_KEYS); k["y"] = rng.uniform(5, 475, N_KEYS); k["octave"] = rng.integers(0, NLEVELS, N_KEYS); k["size"] = 31; k["class_id"] = -1
        n = len(seen)
        k["x"][:n] = u[seen] + rng.uniform(-0.5, 0.5, n); k["y"][:n] = v[seen] + rng.uniform(-0.5, 0.5, n); k["octave"][:n] = octave[seen]
        dd = desc[seen].copy(); fl = rng.integers(0, 256, (n, 8))
        for j in range(8):
            dd[np.arange(n), fl[:, j] >> 3] ^= (1 << (fl[:, j] & 7)).astype(np.uint8)
        d[:n] = dd
        ur = np.full(N_KEYS, -1.0, f32); st = rng.random(n) < 0.6
        ur[:n] = np.where(st, k["x"][:n] - f32(BF) / Xc[seen, 2].astype(f32), f32(-1))
        perm = rng.permutation(N_KEYS)
        kfs.append(dict(T=sophus.SE3f(R, t), keys=np.ascontiguousarray(k[perm]), desc=np.ascontiguousarray(d[perm]), ur=np.ascontiguousarray(ur[perm])))
    return dict(pos=pos.astype(f32), normal=normal, mind=mind, maxd=maxd, desc=desc, kfs=kfs)


def run_shape(lib, ex, rng, K, Mp, reps):
    L = lib.L
    S = make_scene(rng, K, Mp)
    sfs = np.cumprod(np.array([1.0] + [SCALE] * (NLEVELS - 1), f32), dtype=f32); sigma2 = (sfs * sfs).astype(f32); inv_s2 = (f32(1) / sigma2).astype(f32)
    libm = C.CDLL("libm.so.6"); libm.logf.restype = C.c_float; libm.logf.argtypes = [C.c_float]
    lsf = f32(libm.logf(f32(SCALE)))
    # ---- the batch: resident key frames, resident points, one table ----
    e32, e1 = np.zeros(0, np.uint32), np.zeros(1, np.int32)
    rkfs = [M.ResidentKeyFrame(ex, views.key_frame_view(kf["keys"], kf["desc"], sfs, sigma2, e32, e1, e32, kf["ur"])) for kf in S["kfs"]]
    rp = M.ResidentPoints(ex, S["pos"], S["normal"], S["mind"], S["maxd"], S["desc"])
    specs = [M.fuse_spec(kf["T"], CAM, BOUNDS, BF, lsf) for kf in S["kfs"]]
    T = (views.FuseTarget * K)()
    for k in range(K):
        T[k].kf = rkfs[k]._kf; T[k].spec = specs[k][0]; T[k].log_scale_factor = specs[k][1]; T[k].inv_level_sigma2 = inv_s2.ctypes.data
    bi = np.full((K, Mp), -1, np.int32)
    batch = lambda: lib.check(L.orbm_fuse_candidates_batch(ex._h, K, T, rp._p, None, TH, 1, bi.ctypes.data, None))
    t0 = time.perf_counter(); batch(); cold = (time.perf_counter() - t0) * 1e3
    # ---- the loop: per key frame project, PredictScale on the host, search (the key frame goes up again) ----
    min_inv = (f32(0.8) * S["mind"]).astype(f32); max_inv = (f32(1.2) * S["maxd"]).astype(f32)
    pin = M._ProjectIn(Mp, S["pos"].ctypes.data, S["normal"].ctypes.data, min_inv.ctypes.data, max_inv.ctypes.data, None)
    out = dict(valid=np.zeros(Mp, np.uint8), u=np.zeros(Mp, f32), v=np.zeros(Mp, f32), ur=np.zeros(Mp, f32), inv_z=np.zeros(Mp, f32), dist=np.zeros(Mp, f32))
    pout = M._ProjectOut(*[out[k].ctypes.data for k in ("valid", "u", "v", "ur", "inv_z", "dist")])
    lvl = np.zeros(Mp, np.int32)
    pview = views.ProjectedPointView(Mp, out["valid"].ctypes.data, out["u"].ctypes.data, out["v"].ctypes.data, out["ur"].ctypes.data, lvl.ctypes.data, None, S["desc"].ctypes.data)
    fvs = [views.frame_view(kf["keys"], kf["desc"], sfs, 0, 0, kf["ur"], mbf=BF, bounds=BOUNDS) for kf in S["kfs"]]
    li = np.full((K, Mp), -1, np.int32)
    rows = [li[k].ctypes.data for k in range(K)]

    def loop(exact=False, upto=K):
        for k in range(upto):
            lib.check(L.orbm_project_points(ex._h, C.byref(specs[k][0]), C.byref(pin), C.byref(pout)))
            ratio = S["maxd"] / np.maximum(out["dist"], f32(1e-30))
            if exact:
                lvl[:] = _predict_scale_float(ratio, lsf, NLEVELS)
            else:
                np.clip(np.ceil(np.log(ratio) / lsf), 0, NLEVELS - 1, out=ratio); lvl[:] = ratio
            lib.check(L.orbm_fuse_candidates(ex._h, fvs[k].ref(), C.byref(pview), TH, 1, inv_s2.ctypes.data, rows[k], None))
    check = min(K, 3)
    loop(exact=True, upto=check)
    equal = bool(np.array_equal(li[:check], bi[:check]))
    t_batch = timed(batch, reps)
    t_loop = timed(loop, max(5, reps if K <= 60 else reps // 5))
    approx_rows_differ = int((li != bi).any(1).sum())          # numpy's logf is not glibc's to the last bit: rows of the timed loop that differ from the batch
    # ---- the oracle's candidate search on one core, fed with the loop's projections ----
    t_or = 0.0
    for k in range(K):
        lib.check(L.orbm_project_points(ex._h, C.byref(specs[k][0]), C.byref(pin), C.byref(pout)))
        lv = np.clip(np.ceil(np.log(S["maxd"] / np.maximum(out["dist"], f32(1e-30))) / lsf), 0, NLEVELS - 1).astype(np.int32)
        pts = views.projected_point_view(out["valid"], out["u"], out["v"], lv, S["desc"], ur=out["ur"])
        t0 = time.perf_counter(); ol.oracle_fuse_candidates(fvs[k], pts, TH, inv_s2); t_or += (time.perf_counter() - t0) * 1e3
    row = dict(K=K, M=Mp, N=N_KEYS, pairs_fused=int((bi >= 0).sum()), rows_equal_exact_predict_scale=equal, rows_checked=check, timed_loop_rows_differing=approx_rows_differ,
               batch_ms=t_batch[0], batch_min_max=t_batch[1:], batch_cold_ms=cold, loop_ms=t_loop[0], loop_min_max=t_loop[1:], loop_ms_per_keyframe=t_loop[0] / K,
               loop_over_batch=t_loop[0] / t_batch[0], cpu_oracle_search_ms_one_core=t_or)
    for o in rkfs + [rp]:
        o.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shapes", default="30x1500,60x2000,200x4000,1x1500,4x1500,8x1500")
    ap.add_argument("--emu", action="store_true", help="rehearsal on the CPU emulator build (tests/emu): checks the script, its times mean nothing")
    a = ap.parse_args()
    lib = _lib.OrbxLib(ol.emu_lib_path()) if a.emu else _lib.load_hip()
    ex = ORBextractor(1000, SCALE, NLEVELS, 20, 7, lib=lib)
    rng = np.random.default_rng(11)
    run_shape(lib, ex, rng, 2, 200, 3)                       # code objects, pinned buffers
    rows = []
    for sh in a.shapes.split(","):
        K, Mp = [int(x) for x in sh.split("x")]
        row = run_shape(lib, ex, rng, K, Mp, a.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(tool="tools/bench_fuse_batch.py", library="emulator (rehearsal)" if a.emu else "liborbx_hip.so", host=platform.node(), cpus=os.cpu_count(),
               timing="wall clock of blocking calls at the C ABI, median after 3 warm-up calls; loop = orbm_project_points + numpy PredictScale + orbm_fuse_candidates per key frame",
               th=TH, chi2_gate=1, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ex.close()


if __name__ == "__main__":
    main()
