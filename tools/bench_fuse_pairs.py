"""The Fuse batch on the resident map answered with the matched pairs alone (orbm_fuse_pairs_batch_map) against the dense call (orbm_fuse_candidates_batch_map),
in milliseconds per blocking call through the wrappers.  The world and the two shapes are tools/bench_fuse_map.py's:
  local_mapping   40 key frames of 1 200 features, the current key frame's 1 000 points, the chi-square overload
  loop_closing    400 key frames of 1 200 features, 5 000 loop points, the Sim3 overload
Per shape:
  (a)  dense               orbm_fuse_candidates_batch_map with kf_slot: three [K][M] arrays come down (the parent commit's route)
  (a') dense_without_kf_slot   the same with kf_slot = NULL: two arrays
  (a+) dense_and_nonzero   (a) and np.nonzero(best_idx >= 0) on the host: the replay needs the pairs either way
  (p)  pairs               orbm_fuse_pairs_batch_map with every output: start, point, feat, dist, point_slot, kf_slot
  (p') pairs_point_feat    the same with point and feat only
The routes alternate inside every repetition; median and p10 / p90 over the repetitions.  (p) is asserted to equal the row-major compaction of (a).
pairs_ahead: the p10 - p90 range of (p) lies wholly below that of (a).
Prints one JSON line.  Usage: python tools/bench_fuse_pairs.py [--out profiles/fuse_pairs/bench.json] [--reps 20] [--lib other_build.so] [--shapes 40x1000,400x5000]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from orb_slam3_detailed_comments_amd import ORBextractor  # noqa: E402
from orb_slam3_detailed_comments_amd import _lib, matcher as M  # noqa: E402
from bench_fuse_map import NLEVELS, World, timed_alternating  # noqa: E402

i32, u8 = np.int32, np.uint8


def bench_shape(lib, K, Mp, chi2, reps):
    rng = np.random.default_rng(17)
    ex = ORBextractor(1000, 1.2, NLEVELS, 20, 7, lib=lib)
    W = World(ex, rng, K)
    good = np.flatnonzero((W.state[W.slot_of] & 2) == 0)
    set_slots = W.slot_of[rng.choice(good, Mp, replace=False)]
    W.mp.select(0, set_slots)
    late = rng.choice(set_slots, Mp // 50, replace=False).astype(i32)
    W.mp.set_bad(late, np.ones(len(late), u8))
    rows_idx = np.arange(K, dtype=i32)
    s2 = W.inv_sigma2 if chi2 else None
    dense = lambda: M.ORBmatcher.FuseCandidatesBatchMap(ex, W.kfs, W.specs, W.mp, 0, rows_idx, 3.0, s2, want_kf_slot=True)
    dense_plain = lambda: M.ORBmatcher.FuseCandidatesBatchMap(ex, W.kfs, W.specs, W.mp, 0, rows_idx, 3.0, s2)
    pairs = lambda: M.ORBmatcher.FuseCandidatesPairsBatchMap(ex, W.kfs, W.specs, W.mp, 0, rows_idx, 3.0, s2)
    pairs_plain = lambda: M.ORBmatcher.FuseCandidatesPairsBatchMap(ex, W.kfs, W.specs, W.mp, 0, rows_idx, 3.0, s2, want_dist=False, want_slots=False)

    def dense_and_nonzero():
        bi, bd, ks = dense()
        return bi, bd, ks, np.nonzero(bi >= 0)
    bi, bd, ks, (k, i) = dense_and_nonzero()
    start = np.concatenate([[0], np.cumsum((bi >= 0).sum(1))]).astype(i32)
    want = (start, i.astype(i32), bi[k, i], bd[k, i], set_slots[i].astype(i32), ks[k, i])
    for name, got in (("pairs", pairs()), ("pairs_point_feat", pairs_plain())):
        for j, w in enumerate(want):
            assert got[j] is None and name == "pairs_point_feat" and j > 2 or np.array_equal(got[j], w), "%s: output %d differs from the compaction of the dense call" % (name, j)
    r = timed_alternating(dict(dense=dense, dense_without_kf_slot=dense_plain, dense_and_nonzero=dense_and_nonzero, pairs=pairs, pairs_point_feat=pairs_plain), reps)
    r.update(K=K, M=Mp, chi2_gate=int(chi2), fused_pairs=int(start[-1]), dense_bytes=int(12 * K * Mp), pairs_bytes=int(4 * (K + 1) + 20 * start[-1]),
             pairs_over_dense=r["pairs"]["ms"] / r["dense"]["ms"], pairs_over_dense_and_nonzero=r["pairs"]["ms"] / r["dense_and_nonzero"]["ms"],
             pairs_ahead=bool(r["pairs"]["p90"] < r["dense"]["p10"]))
    W.close(); ex.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of the library (the emulator: a functional check of this tool, not a measurement)")
    ap.add_argument("--shapes", default="40x1000,400x5000", help="KxM: the first is run with the chi-square gate (LocalMapping), the others without (loop closing)")
    a = ap.parse_args()
    lib = _lib.OrbxLib(a.lib) if a.lib else None
    names = ["local_mapping", "loop_closing"]
    out = dict(reps=a.reps)
    for n, shape in enumerate(a.shapes.split(",")):
        K, Mp = (int(v) for v in shape.split("x"))
        out[names[n] if n < 2 else "shape%d" % n] = bench_shape(lib, K, Mp, n == 0, a.reps)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
