"""MapPoint::ComputeDistinctiveDescriptors for the points of a resident map, in milliseconds per call, blocking: the route the parent commit has against
orbm_distinctive_descriptors_resident, the two alternating repetition by repetition on one box in one run.
  (a) gather_choose_update   the host copies the 32 bytes of every observation out of the key frames' descriptor rows (numpy fancy indexing of one
                             array of all rows; a C++ loop over mObservations was NOT timed), orbm_distinctive_descriptors on them, then orbm_map_update
                             of the points with the winners and the four other fields.  `gather` is that copy alone, `choose` the call alone
  (b) resident               orbm_distinctive_descriptors_resident with the map and the slots: observations named by (key frame, feature), the winners
                             written into the store on the device; only best[] comes back
  kernels                    HIP-event times of k_distinctive_resident (both launch lists, with the store writes) and of k_distinctive on the same points,
                             from tools/distinctive_kernels_bench.hip (built into tools/bin/ when it is not there), alternating
Shapes (key frames of 1200 features; a point's rows are copies of one descriptor with 20 of 256 bits flipped, at places of their own):
  local_mapping   1 000 points in 40 key frames, 2..60 observations skewed low (2 + a geometric count, mean about 10)
  loop_closing    20 000 points with the same counts; 400 key frames, so that every observation still has a place of its own
  large           200 points of 65..300 observations in 40 key frames (all of them take the LDS form)
The tool asserts that both routes choose the same rows and leave the same descriptors in the store.  Prints one JSON line.
Usage: python tools/bench_distinctive_resident.py [--out profiles/map_descriptors/bench.json] [--reps 20] [--lib other_build.so] [--shapes local_mapping,large]
       [--points-dir DIR]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_detailed_comments_amd import ORBextractor, views  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402

KF_N = 1200
SHAPES = dict(local_mapping=(1000, 40, "low"), loop_closing=(20000, 400, "low"), large=(200, 40, "large"))
PROGRAM = os.path.join(ROOT, "tools", "bin", "distinctive_kernels_bench")
SOURCE = os.path.join(ROOT, "tools", "distinctive_kernels_bench.hip")


def stats(t):
    return dict(ms=float(np.median(t)), p10=float(np.percentile(t, 10)), p90=float(np.percentile(t, 90)))


def build_program():
    csrc = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")
    deps = [SOURCE, os.path.join(csrc, "k_match.hip"), os.path.join(csrc, "orbx_types.h")]
    if os.path.exists(PROGRAM) and all(os.path.getmtime(PROGRAM) >= os.path.getmtime(d) for d in deps):
        return
    os.makedirs(os.path.dirname(PROGRAM), exist_ok=True)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + csrc, SOURCE, "-o", PROGRAM], check=True)


def make_shape(rng, P, nkf, kind):
    counts = (2 + np.minimum(58, rng.geometric(0.12, P) - 1)) if kind == "low" else rng.integers(65, 301, P)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(start[-1])
    assert total <= nkf * KF_N
    place = rng.permutation(nkf * KF_N)[:total]                                   # observation o is row place[o] of all rows: a place of its own
    obs_kf = (place // KF_N).astype(np.int32); obs_feat = (place % KF_N).astype(np.int32)
    all_rows = rng.integers(0, 256, (nkf * KF_N, 32), dtype=np.uint8)
    rows = np.repeat(rng.integers(0, 256, (P, 32), dtype=np.uint8), counts, axis=0)
    fl = rng.integers(0, 256, (total, 20))
    for j in range(20):
        rows[np.arange(total), fl[:, j] >> 3] ^= (1 << (fl[:, j] & 7)).astype(np.uint8)
    all_rows[place] = rows
    return counts, start, obs_kf, obs_feat, all_rows


def bench_shape(lib, name, reps, kernels, points_dir=None):
    P, nkf, kind = SHAPES[name]
    rng = np.random.default_rng(31)
    counts, start, obs_kf, obs_feat, all_rows = make_shape(rng, P, nkf, kind)
    total = int(start[-1])
    ex = ORBextractor(1000, 1.2, 8, 20, 7, lib=lib)
    sfs = ex.GetScaleFactors(); e32 = np.zeros(0, np.uint32); keys = np.zeros(KF_N, views.KP_DTYPE)
    kfs = [M.ResidentKeyFrame(ex, views.key_frame_view(keys, all_rows[k * KF_N:(k + 1) * KF_N], sfs, sfs * sfs, e32, np.zeros(1, np.int32), e32)) for k in range(nkf)]
    SLOTS = 2 * P
    slots = rng.permutation(SLOTS)[:P].astype(np.int32)
    pos = rng.normal(0, 3, (P, 3)).astype(np.float32); normal = rng.normal(0, 1, (P, 3)).astype(np.float32)
    mind = rng.uniform(0.1, 1, P).astype(np.float32); maxd = rng.uniform(5, 50, P).astype(np.float32)
    mp = M.ResidentMap(ex, SLOTS, 1, 8, 1)
    mp.update(slots, pos, normal, mind, maxd, np.zeros((P, 32), np.uint8))
    L = ex._lib
    table = (C.c_void_p * nkf)(*[k._kf for k in kfs])
    best_b = np.zeros(P, np.int32)
    state = {}

    def gather():
        return all_rows[obs_kf.astype(np.int64) * KF_N + obs_feat]               # (the index arithmetic is the walk's: key frame, then row)

    def a_fn():
        rows = gather()
        best = M.ComputeDistinctiveDescriptors(ex, rows, start)
        mp.update(slots, pos, normal, mind, maxd, rows[start[:-1] + best])
        state["best_a"] = best

    def b_fn():
        L.check(L.L.orbm_distinctive_descriptors_resident(ex._h, nkf, table, P, start.ctypes.data, obs_kf.ctypes.data, obs_feat.ctypes.data, mp._m, slots.ctypes.data,
                                                          best_b.ctypes.data, None))

    def store():
        mp.select(0, slots)
        return M.PointsFetch(ex, mp.set(0))[4].copy()
    # both routes choose the same rows and leave the same descriptors in the store
    mp.update(slots, pos, normal, mind, maxd, np.zeros((P, 32), np.uint8))
    b_fn(); got_b = store()
    mp.update(slots, pos, normal, mind, maxd, np.zeros((P, 32), np.uint8))
    a_fn(); got_a = store()
    assert np.array_equal(state["best_a"], best_b) and got_a.tobytes() == got_b.tobytes() and got_a.any()
    rows0 = gather()
    ta, tb, tg, tc = [], [], [], []
    for it in range(-3, reps):                                                    # three warm-up rounds; the routes alternate
        t0 = time.perf_counter(); a_fn(); t1 = time.perf_counter(); b_fn(); t2 = time.perf_counter()
        gather(); t3 = time.perf_counter(); M.ComputeDistinctiveDescriptors(ex, rows0, start); t4 = time.perf_counter()
        if it >= 0:
            ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3); tg.append((t3 - t2) * 1e3); tc.append((t4 - t3) * 1e3)
    r = dict(points=P, key_frames=nkf, observations=total, largest=int(counts.max()), mean_observations=float(counts.mean()),
             gather_choose_update=stats(ta), resident=stats(tb), gather=stats(tg), choose=stats(tc))
    r["b_over_a"] = r["resident"]["ms"] / r["gather_choose_update"]["ms"]
    mp.close()
    for k in kfs:
        k.close()
    ex.close()
    if kernels:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(points_dir or tmp, name + ".bin")                 # (--points-dir keeps the file: the program can be run on it again)
            with open(path, "wb") as f:
                np.array([nkf, P, total] + [KF_N] * nkf, np.int32).tofile(f)
                all_rows.tofile(f); start.tofile(f); obs_kf.tofile(f); obs_feat.tofile(f)
            r["kernels"] = json.loads(subprocess.run([PROGRAM, path, str(reps)], check=True, capture_output=True, text=True, timeout=300).stdout)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement; no kernel times)")
    ap.add_argument("--shapes", default="local_mapping,loop_closing,large")
    ap.add_argument("--points-dir", default=None, help="keep the points files of the kernel timing program in this (existing) directory")
    a = ap.parse_args()
    lib = _lib.OrbxLib(a.lib) if a.lib else None
    if not a.lib:
        build_program()
    out = dict(reps=a.reps, key_frame_features=KF_N, shapes={s: bench_shape(lib, s, a.reps, not a.lib, a.points_dir) for s in a.shapes.split(",")})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
