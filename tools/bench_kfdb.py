"""Key frame database query latency (orbv_db_query, the place-recognition step of Tracking::Relocalization / LoopClosing): milliseconds per
query at Q = 1 and Q = 64 on synthetic maps of 1 k / 5 k / 20 k key frames of ~1 000 words, beside a host restatement of the reference's
std::list inverted file on one core (tests/cpp/kfdb_facade_test.cpp, bench mode: the walk, the threshold and the scores of
DetectRelocalizationCandidates - a restatement, not the reference build).  Every call is blocking (the results are back on the host when
it returns), so the time is the wall-clock time of the call: warm-up, then the median (and min / max) of repeated calls.
Usage: python tools/bench_kfdb.py [--out profiles/kfdb/bench.json] [--maps 1000,5000,20000] [--reps 30]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kfdb_world as kw           # noqa: E402
import vocab_scenes as vs         # noqa: E402
from orb_slam3_detailed_comments_amd import _lib  # noqa: E402
from orb_slam3_detailed_comments_amd.extractor import ORBextractor  # noqa: E402
from orb_slam3_detailed_comments_amd.vocabulary import ORBVocabulary, KeyFrameDatabase  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def host_restatement(vocpath, n, tmp):
    ref = os.path.join(ROOT, "oracle", "_ref", "libref_dbow2.so")
    if not os.path.exists(ref):
        return None
    exe = os.path.join(tmp, "kfdb_bench")
    libdir = os.path.dirname(_lib.HIP_LIB_PATH)
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-I" + os.path.join(ROOT, "include", "orb_slam3_amd"), "-I" + os.path.join(ROOT, "oracle", "opencv_shim"),
                    os.path.join(ROOT, "tests", "cpp", "kfdb_facade_test.cpp"), "-L" + libdir, "-lorbx_hip", ref, "-Wl,-rpath," + libdir,
                    "-Wl,-rpath," + os.path.dirname(ref), "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe, vocpath, "1", "bench", str(n), "30"], capture_output=True, text=True, timeout=900, check=True)
    return float(r.stdout.split("median_ms=")[1].split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--maps", default="1000,5000,20000")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    ex = ORBextractor(1000, 1.2, 8, 20, 7)
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp()
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 10, 4)
    vocpath = os.path.join(tmp, "voc.txt")
    vs.write_text(vocpath, header, parent, leaf, desc, weight)
    voc = ORBVocabulary.loadFromTextFile(ex, vocpath)
    rows = []
    for n in [int(x) for x in a.maps.split(",")]:
        bows = kw.scale_bows(rng, voc.size(), n)
        db = KeyFrameDatabase(voc, ex)
        for i, b in enumerate(bows):
            db.add(i, *b)
        qs = [bows[int(i)] for i in rng.integers(0, n, 64)]
        db.query(qs[:1])                                   # first query uploads the map
        q1 = timed(lambda: db.query(qs[:1]), a.reps)
        q64 = timed(lambda: db.query(qs), max(5, a.reps // 3))
        host = host_restatement(vocpath, n, tmp)
        row = dict(keyframes=n, words_per_kf=float(np.mean([len(b[0]) for b in bows])), sharing_keys_q1=len(db.query(qs[:1])[0]["keys"]),
                   device_q1_ms=q1[0], device_q1_min_max=q1[1:], device_q64_ms_per_query=q64[0] / 64, device_q64_call_ms=q64[0],
                   host_restatement_q1_ms=host)
        rows.append(row)
        print(json.dumps(row), flush=True)
        db.close()
    out = dict(tool="tools/bench_kfdb.py", timing="wall clock of blocking calls, median after 3 warm-up calls", rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
