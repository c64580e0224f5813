"""Run by tests/test_shared_objects.py in a process of its own: host threads, each with its own extractor handle, use ONE device object at the same
time (a vocabulary; resident key frames and a point set).  A defect here corrupts memory and aborts the process, so the threaded part runs in this child
and the test reads its exit status and its last line.

    shared_objects_runner.py <library> <repository root> <scratch directory> <scenario> <calls per thread>

Every expectation is computed here, serially, before the threads start, and never by the library under test: the reference's own DBoW2
(oracle/_ref/libref_dbow2.so) for the vocabulary, oracle_lib's search oracles for the match rows.  The threads start behind a barrier.  Last line:
"DONE <calls> calls, 0 mismatches" and exit status 0, or the mismatches and exit status 1."""
import os
import sys
import threading

import numpy as np

LIB, ROOT, TMP, SCENARIO, COUNT = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol                                                   # noqa: E402
import vocab_scenes as vs                                                 # noqa: E402
from orb_slam3_detailed_comments_amd import _lib                          # noqa: E402
from orb_slam3_detailed_comments_amd.extractor import ORBextractor       # noqa: E402
from orb_slam3_detailed_comments_amd.vocabulary import ORBVocabulary     # noqa: E402

NTHREADS = 3
FIELDS = ("bow_id", "bow_val", "fv_node", "fv_start", "fv_feat", "word_id", "node_id")
lib = _lib.OrbxLib(LIB)
errors, errors_lock = [], threading.Lock()
events = []                                # what a thread may wait for besides the barrier: set when another thread dies, so that nobody waits for it


def report(msg):
    with errors_lock:
        errors.append(msg)


def run_threads(bodies):
    """bodies[t](barrier): one thread each; an exception in a thread is a mismatch"""
    barrier = threading.Barrier(len(bodies))

    def guard(t):
        try:
            bodies[t](barrier)
        except BaseException as e:                     # noqa: B036 - the barrier must not be left waiting
            barrier.abort()
            for ev in events:
                ev.set()
            report("thread %d: %s: %s" % (t, type(e).__name__, e))
    ths = [threading.Thread(target=guard, args=(t,)) for t in range(len(bodies))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()


def dbow2_expectation(ref, q, levelsup):
    """the seven arrays of a BowResult from the reference's transform() and its single-feature descent"""
    bi, bv, fn, fs, ff = ref.transform(q, levelsup)
    words = np.zeros(len(q), np.uint32); nodes = np.zeros(len(q), np.uint32)
    for i in range(len(q)):
        w, _, nd = ref.transform_one(q[i], levelsup)
        words[i], nodes[i] = w, nd
    return dict(bow_id=bi.astype(np.uint32), bow_val=bv.astype(np.float64), fv_node=fn.astype(np.uint32), fv_start=fs.astype(np.int32), fv_feat=ff.astype(np.uint32),
                word_id=words, node_id=nodes)


def differs(res, exp):
    return [f for f in FIELDS if np.ascontiguousarray(getattr(res, f)).tobytes() != np.ascontiguousarray(exp[f]).tobytes()]


def vocabulary(grow):
    """One vocabulary (k = 10, L = 3, L1 / TF-IDF), three handles, three descriptor sets of 700 / 650 / 500 rows, levelsup 2, warmed at 700 rows.  grow: the
    first call of thread 2 carries 1500 rows, more than the scratch holds, and is made once both other threads have a call behind them."""
    levelsup = 2
    rng = np.random.default_rng(41)
    header, parent, leaf, desc, weight = vs.make_vocabulary(rng, 10, 3)
    path = os.path.join(TMP, "voc_shared.txt")
    vs.write_text(path, header, parent, leaf, desc, weight)
    ref = ol.RefVocabulary(path)
    sets = [vs.descriptors_near(rng, desc, n) for n in (700, 650, 500)]
    exps = [dbow2_expectation(ref, q, levelsup) for q in sets]
    big = vs.descriptors_near(rng, desc, 1500)
    exp_big = dbow2_expectation(ref, big, levelsup) if grow else None
    exs = [ORBextractor(500, 1.2, 8, 20, 7, lib=lib) for _ in range(NTHREADS)]
    voc = ORBVocabulary.from_arrays(exs[0], *header, parent, leaf, desc, weight)
    d = differs(voc.transform(sets[0], levelsup), exps[0])
    if d:
        report("the warming call differs from DBoW2 in %s" % d)
    views_ = [ORBVocabulary(exs[t], voc._v) for t in range(NTHREADS)]      # the same orbv_vocabulary through each thread's own handle
    for w in views_:
        w.close = lambda: None                                             # (voc destroys it)
    calls = [0] * NTHREADS
    started = [threading.Event() for _ in range(NTHREADS)]
    events.extend(started)

    def body(t):
        def run(barrier):
            barrier.wait()
            if grow and t == 2:
                started[0].wait(); started[1].wait()
                d = differs(views_[t].transform(big, levelsup), exp_big); calls[t] += 1
                if d:
                    report("thread 2, growing call of 1500 rows: differs from DBoW2 in %s" % d)
            for i in range(COUNT):
                d = differs(views_[t].transform(sets[t], levelsup), exps[t]); calls[t] += 1
                started[t].set()
                if d:
                    report("thread %d call %d: differs from DBoW2 in %s" % (t, i, d))
        return run
    run_threads([body(t) for t in range(NTHREADS)])
    voc.close()
    for ex in exs:
        ex.close()
    return sum(calls)


def live():
    import ctypes as C
    a = (C.c_longlong * 4)()
    lib.check(lib.L.orbx_debug_live_resources(a))
    return list(a)


def keyframes():
    """The Scene of tests/test_fuse_batch.py (5 key frames, 300 points): ONE set of resident key frames and ONE resident point set, made through handle 0,
    searched by three threads through their own handles.  Each thread alternates orbm_fuse_candidates_batch and orbm_search_by_projection_sim3_batch over
    three image-bounds variants (the scene's own, widened by 3.5, widened by 9.25), so that every key frame's grid cache (kKfGridsKept = 2) turns over while
    other threads hold grids; thread 0 also runs the resident triangulation and BoW searches on key frames 2 and 4, whose call-time flags and results are
    its own.  Every row equals the oracle's for the variant used."""
    from orb_slam3_detailed_comments_amd import matcher as M, views
    from test_fuse_batch import NLEVELS, Scene, Target, scene
    from test_sim3_projection_batch import Sim3Scene
    live0 = live()
    S = scene()
    exs = [ORBextractor(500, S.scale, NLEVELS, 20, 7, lib=lib) for _ in range(NTHREADS)]
    th, ratio = 3.0, 1.0
    variants = []
    for w in (0.0, 3.5, 9.25):
        V = Scene.__new__(Scene); V.__dict__.update(S.__dict__); V.expected = {}; V.targets = []
        for T in S.targets:
            alt = Target.__new__(Target); alt.__dict__.update(T.__dict__)
            alt.bounds = (T.bounds[0] - w, T.bounds[1] + w, T.bounds[2] - w, T.bounds[3] + w)
            V.targets.append(alt)
        Q = Sim3Scene.__new__(Sim3Scene); Q.__dict__.update(V.__dict__); Q.expected = {}; Q.free = {}      # the same targets as the Sim3 search takes them
        Q.cap = max(T.N for T in V.targets)
        fi, fd, _ = V.expect(exs[0], th, True)
        sa, sn = Q.expect(exs[0], th, ratio)
        variants.append(dict(fuse_specs=[T.spec(S.log_scale) for T in V.targets], sim3_specs=[Q.spec(k) for k in range(V.K)], fi=fi, fd=fd, sa=sa, sn=sn))
    if not all((v["fi"] >= 0).sum() > 150 and v["sn"].sum() > 60 for v in variants):
        report("the scene gives the oracle too little to match")
    if all(np.array_equal(variants[0]["fi"], v["fi"]) for v in variants[1:]):
        report("the bounds variants do not change the oracle's rows")
    # the shared objects: key frames 2 and 4 carry a FeatureVector and map-point flags as tests/test_resident_keyframes.py makes them
    rng = np.random.default_rng(8)
    kviews = []
    for k, T in enumerate(S.targets):
        node_of = rng.integers(0, 9, T.N) * 7 + 2
        nodes = np.unique(node_of) if T.N else np.zeros(0, np.int64)
        st, ft = [0], []
        for n in nodes:
            f = np.nonzero(node_of == n)[0]; ft += f.tolist(); st.append(len(ft))
        mp = (rng.random(T.N) < 0.6).astype(np.uint8)
        kviews.append(views.key_frame_view(T.keys, T.desc, S.sfs, S.sigma2, nodes.astype(np.uint32), np.asarray(st, np.int32), np.asarray(ft, np.uint32), T.u_right, mp))
    fresh = [M.ResidentKeyFrame(exs[0], kv) for kv in kviews]              # never searched: what a key frame without grids gives back
    before = live()[0]
    for kf in fresh:
        kf.close()
    per_fresh = before - live()[0]
    kfs = [M.ResidentKeyFrame(exs[0], kv) for kv in kviews]
    rp = S.points(exs[0])
    a, b = 4, 2
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32); ep = np.array([1e6, 240.0], np.float32)
    bow_pairs = [(a, a), (a, b), (b, a)]
    exp_bow = [ol.oracle_search_by_bow(kviews[i], kviews[j], 0.7, True, True) for i, j in bow_pairs]
    exp_tri = [ol.oracle_search_for_triangulation(kviews[a], kviews[j], F, ep, False, True, True) for j in (b, a)]
    if exp_bow[0][0] < 100 or exp_tri[1][0] < 1:
        report("the resident searches have nothing to find: %d BoW matches, %d triangulation pairs" % (exp_bow[0][0], exp_tri[1][0]))
    calls = [0] * NTHREADS

    def body(t):
        def run(barrier):
            ex = exs[t]
            barrier.wait()
            for i in range(COUNT):
                v = variants[(i + t) % 3]
                bi, bd = M.ORBmatcher.FuseCandidatesBatch(ex, kfs, v["fuse_specs"], rp, th, S.inv_sigma2); calls[t] += 1
                if not (np.array_equal(bi, v["fi"]) and np.array_equal(bd, v["fd"])):
                    report("thread %d call %d: orbm_fuse_candidates_batch, variant %d: %d entries differ from the oracle" % (t, i, (i + t) % 3, int((bi != v["fi"]).sum())))
                v = variants[(i + t + 1) % 3]
                ga, gn = M.ORBmatcher.SearchByProjectionSim3Batch(ex, kfs, v["sim3_specs"], rp, th, ratio); calls[t] += 1
                if not (np.array_equal(ga, v["sa"]) and np.array_equal(gn, v["sn"])):
                    report("thread %d call %d: orbm_search_by_projection_sim3_batch, variant %d: %d entries differ from the oracle" % (t, i, (i + t + 1) % 3, int((ga != v["sa"]).sum())))
                if t == 0:
                    got = M.ORBmatcher(0.7, True).SearchByBoWResident(ex, [kfs[i_] for i_, _ in bow_pairs], [kviews[i_].keep[8] for i_, _ in bow_pairs],
                                                                      [kfs[j_] for _, j_ in bow_pairs], [kviews[j_].keep[8] for _, j_ in bow_pairs], True); calls[t] += 1
                    for p, (g, e) in enumerate(zip(got, exp_bow)):
                        if g[0] != e[0] or not np.array_equal(g[1], e[1]):
                            report("thread 0 call %d: orbm_search_by_bow_resident, pair %d: %d matches, the oracle has %d" % (i, p, g[0], e[0]))
                    got = M.ORBmatcher(0.6, True).SearchForTriangulationResident(ex, kfs[a], kviews[a].keep[8], [kfs[b], kfs[a]], [kviews[b].keep[8], kviews[a].keep[8]],
                                                                                 np.stack([F, F]), np.stack([ep, ep]), False, True); calls[t] += 1
                    for p in range(2):
                        if got[p] != exp_tri[p]:
                            report("thread 0 call %d: orbm_search_for_triangulation_resident, key frame %d: %d pairs, the oracle has %d" % (i, p, got[p][0], exp_tri[p][0]))
        return run
    run_threads([body(t) for t in range(NTHREADS)])
    # every key frame kept at most kKfGridsKept = 2 grids (one device allocation each) on top of what a key frame that was never searched holds
    before = live()[0]
    for kf in kfs:
        kf.close()
    grids = (before - live()[0]) - per_fresh
    searched = sum(1 for T in S.targets if T.N > 0)
    if not (searched <= grids <= 2 * len(kfs)):
        report("the %d key frames held %d grids between them after the run (at most 2 each, at least 1 for each of the %d with keypoints)" % (len(kfs), grids, searched))
    rp.close()
    for ex in exs:
        ex.close()
    if live() != live0:
        report("orbx_debug_live_resources: %s before, %s after everything was destroyed" % (live0, live()))
    return sum(calls)


def shared_map():
    """One orbm_map (the streams of tests/test_local_map_build.py's search test, all maps in one store), a writer and two readers, each with a handle of
    its own.  Reader 0 repeats orbm_map_local_points (sets 0 .. B - 1) + orbm_map_set_fetch + a SearchLocalPoints batch on the sets.  orbm_map_local_points
    always builds sets 0 .. B - 1, so a second reader cannot run it on set indices of its own: reader 1 builds ITS sets B .. 2B - 1 with orbm_map_select from
    the restated lists, fetches them and runs the same batch.  The writer repeats orbm_map_update, orbm_map_set_bad and orbm_map_set_keyframe on slots and
    rows that no reader's list visits (asserted).  Lists = the restatement of Tracking::UpdateLocalPoints, matches = the reference's own Frame.cc +
    ORBmatcher.cc (oracle/_ref/libref_frame.so), both computed before the threads start.  At the end the writer's slots hold the last values written."""
    from orb_slam3_detailed_comments_amd import matcher as M
    import test_local_map_build as LM
    from test_local_points import BF
    from test_local_points_batch import PARAM_SETS
    from test_local_points_maps import CAM, EMU_SHAPE, World
    shape = EMU_SHAPE
    expect = LM._reference_on_lists(shape, 77)                         # per frame: (list, seen, mbTrackInView, assigned, nmatches)
    W = [World(lib, shape), World(lib, shape)]                         # the readers: the same frames extracted on a handle each
    B = W[0].B
    Y = LM._stream_layout(W[0].maps, 77)
    writer = ORBextractor(300, 1.2, 8, 20, 7, lib=lib)
    n_rows = len(Y["rows"])
    free = np.flatnonzero(~Y["present"]).astype(np.int32)              # slots that hold nothing and stand in no row
    wslots, wrows = free[:60], (n_rows, n_rows + 1)
    visited_rows = set(r for f in Y["frames"] for r in f)
    visited_slots = set(int(s) for r in visited_rows for s in Y["rows"][r]) | set(int(s) for sn in Y["seen"] if sn is not None for s in sn) | \
        set(int(s) for e in expect for s in e[0])
    assert len(wslots) == 60 and not (set(int(s) for s in wslots) & visited_slots) and not (set(wrows) & visited_rows), "the writer must stay off what the readers visit"
    mp = M.ResidentMap(writer, Y["S"], n_rows + 2, max(max(len(r) for r in Y["rows"]), 64), 2 * B + 1)
    ids = np.flatnonzero(Y["present"]).astype(np.int32)
    f = Y["fields"]
    mp.update(ids, f["pos"][ids], f["normal"][ids], f["mind"][ids], f["maxd"][ids], f["desc"][ids], Y["bad"][ids])
    for r, row in enumerate(Y["rows"]):
        mp.set_keyframe(r, row)
    th, far, _, cosl, thfar, ratio = PARAM_SETS[0]
    if sum(e[4] for e in expect) < 50:
        report("the reference finds too little: %s matches" % [e[4] for e in expect])
    to_slot = lambda a, l: np.where(a >= 0, l[np.maximum(a, 0)], -1) if len(l) else np.full(len(a), -1)
    calls = [0, 0, 0]
    done = [threading.Event(), threading.Event()]
    events.extend(done)
    last = {}

    def reader(t):
        def run(barrier):
            w = W[t]; ex = w.ex
            barrier.wait()
            for i in range(COUNT):
                if t == 0:
                    Ms = mp.local_points(Y["frames"], Y["seen"], ext=ex); first = 0
                    if [int(m) for m in Ms] != [len(e[0]) for e in expect]:
                        report("reader 0 call %d: orbm_map_local_points counts %s" % (i, list(Ms)))
                else:
                    first = B
                    for b in range(B):
                        mp.select(B + b, expect[b][0], ext=ex)
                calls[t] += 1
                sets, flags = [], []
                for b in range(B):
                    ls, sn = mp.fetch(first + b, ext=ex)
                    if not np.array_equal(ls, expect[b][0]) or (t == 0 and not np.array_equal(sn, expect[b][1])):
                        report("reader %d call %d: the list of frame %d differs from the restatement" % (t, i, b))
                    sets.append(mp.set(first + b, ext=ex)); flags.append(expect[b][1])
                lp = M.LocalPointsBatch(ex, sets, B, CAM, w.bounds, BF, w.sfs)
                lp.set_poses(w.poses)
                lp.enqueue(0, is_bad=flags, has_obs=None, viewing_cos_limit=cosl, th=th, far_points=far, th_far=thfar, nnratio=ratio, want_in_view=True)
                asg, nm, inv = lp.fetch(); calls[t] += 1
                for b in range(B):
                    ls, sn, ref_inv, ref_as, ref_n = expect[b]
                    N = w.refs[b].N
                    if len(ls) == 0:
                        if nm[b] != 0 or (asg[b] != -1).any():
                            report("reader %d call %d: matches in frame %d, whose map is empty" % (t, i, b))
                        continue
                    if nm[b] != ref_n or not np.array_equal(to_slot(asg[b, :N], ls), to_slot(ref_as, ls)) or not np.array_equal(inv[b, :len(ls)].astype(bool), ref_inv):
                        report("reader %d call %d: frame %d has %d matches, the reference %d" % (t, i, b, nm[b], ref_n))
            done[t].set()
        return run

    def write(barrier):
        rng = np.random.default_rng(5)
        barrier.wait()
        it = 0
        while it < COUNT or not (done[0].is_set() and done[1].is_set()):
            n = len(wslots)
            last.update(pos=rng.normal(0, 3, (n, 3)).astype(np.float32), normal=rng.normal(0, 1, (n, 3)).astype(np.float32), mind=rng.uniform(0.1, 1, n).astype(np.float32),
                        maxd=rng.uniform(5, 50, n).astype(np.float32), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
            mp.update(wslots, last["pos"], last["normal"], last["mind"], last["maxd"], last["desc"], (rng.random(n) < 0.3).astype(np.uint8), ext=writer)
            mp.set_bad(wslots[::2], (rng.random(len(wslots[::2])) < 0.5).astype(np.uint8), ext=writer)
            mp.set_keyframe(wrows[it % 2], rng.permutation(wslots)[:int(rng.integers(1, n))], ext=writer)
            calls[2] += 3; it += 1
    run_threads([reader(0), reader(1), write])
    mp.set_bad(wslots, np.zeros(len(wslots), np.uint8), ext=writer)
    mp.select(2 * B, wslots, ext=writer)
    got = M.PointsFetch(writer, mp.set(2 * B, ext=writer))
    for g, name in zip(got, ("pos", "normal", "mind", "maxd", "desc")):
        if not last or g.tobytes() != last[name].tobytes():
            report("the writer's slots do not hold the last %s written" % name)
    mp.close()
    for w in W:
        w.close()
    writer.close()
    return sum(calls)


SCENARIOS = {"vocabulary": lambda: vocabulary(False), "vocabulary_grow": lambda: vocabulary(True), "keyframes": keyframes, "map": shared_map}

if __name__ == "__main__":
    n = SCENARIOS[SCENARIO]()
    for e in errors[:20]:
        print(e)
    print("DONE %d calls, %d mismatches" % (n, len(errors)), flush=True)
    sys.exit(1 if errors else 0)
