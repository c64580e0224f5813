"""Resident key frames made on the device from frames of the last extraction (orbm_keyframe_create_extracted, orbm_keyframe_create_rig_extracted,
k_keyframe_counts + k_keyframe_snapshot) and their read-back (orbm_keyframe_fetch).

What a key frame holds is pinned array by array by the existing fetch routes: orbx_fetch / orbx_fetch_undistorted (keys), the descriptor rows,
orbm_stereo_fetch (mvuRight) and orbv_fetch (FeatureVector); node_of_feat by the inverse of the CSR computed here.  The same arrays given to
orbm_keyframe_create must read back byte for byte the same (which also tests the fetch), and every search that takes a resident key frame must give the
same result with either.  SearchByBoW(pKF, F) on key frames made on the device is compared with the reference's ORBmatcher.cc
(oracle/_ref/libmw_ref.so), as tests/test_bow_frames_batch.py compares it for key frames made from host arrays.
Shapes: the emulator runs 376x240, 500 features, B = 3; the GPU 752x480, 1200 features, B = 8."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import vocab_scenes as vs
from orb_slam3_detailed_comments_amd import KP_DTYPE, ORBextractor, ORBVocabulary, synth, views
from orb_slam3_detailed_comments_amd import matcher as M

REF = os.path.join(ol.ROOT, "oracle", "_ref", "libmw_ref.so")
E_ARG = -2
LEVELSUP = 2
VOC_SEED = 11              # vs.make_vocabulary(default_rng(VOC_SEED), 6, 3) has zero-weight words that features of these scenes reach (asserted below)
EMU, GPU = (376, 240, 500, 3), (752, 480, 1200, 8)
PARAM_SETS = ((0.7, True), (0.9, False))
SENTINEL = 0x5A5A5A50
f32 = np.float32


def live(lib):
    gc.collect()
    a = (C.c_longlong * 4)()
    lib.check(lib.L.orbx_debug_live_resources(a))
    return tuple(a)


def _images(w, h, B, seed0, blank=1, shift=0, nrect=3000):
    imgs = [synth.corner_field(w, h, seed=seed0 + b, nrect=int(nrect * w * h / (752 * 480))) for b in range(B)]
    if blank is not None:
        imgs[blank] = np.full((h, w), 90, np.uint8)
    a = np.stack(imgs)
    return np.ascontiguousarray(np.roll(a, shift, axis=2)) if shift else a


def _depth(w, h, B, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 6.0, (B, h, w)).astype(f32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0                   # holes: mvuRight = -1 there
    return d


def _vocabulary(ex, seed=VOC_SEED):
    header, parent, leaf, desc, weight = vs.make_vocabulary(np.random.default_rng(seed), 6, 3)
    return ORBVocabulary.from_arrays(ex, *header, parent, leaf, desc, weight)


def _undistortion(w, h):
    return (0.8 * w, 0.8 * w, w / 2 + 1.5, h / 2 - 2.0), (-0.28, 0.07, 2e-4, 1e-4, 0.0)


def _inverse(N, fv_start, fv_feat):
    nof = np.full(N, -1, np.int32)
    for a in range(len(fv_start) - 1):
        nof[np.asarray(fv_feat[fv_start[a]:fv_start[a + 1]], np.int64)] = a
    return nof


class _Batch:
    """one extraction of a handle with everything the existing routes fetch of it: keys (mvKeysUn), descriptor rows, mvuRight from depth, FeatureVectors"""

    def __init__(self, ex, voc, imgs, depth_seed=5, transform=True):
        self.ex, self.B = ex, len(imgs)
        res = ex.extract_batch(imgs)
        self.n = [len(r[1]) for r in res]
        self.raw = [r[1] for r in res]; self.desc = [r[2] for r in res]
        un = ex.fetch_undistorted()
        self.keys = [un[b, :self.n[b]].copy() for b in range(self.B)]
        M.ComputeStereoFromRGBD(ex, _depth(imgs.shape[2], imgs.shape[1], self.B, depth_seed), 40.0)
        u = M.StereoFetch(ex, self.B)[0]
        self.ur = [u[b, :self.n[b]].copy() for b in range(self.B)]
        self.bow = None
        if transform:
            voc.transform_extracted(ex, 0, self.B, LEVELSUP)
            self.bow = [voc.fetch(ex, b, self.n[b]) for b in range(self.B)]

    def expected(self, b, use_ur=True, fv=True):
        N = self.n[b]
        z = np.zeros(0, np.uint32)
        fn, fs, ff = (self.bow[b].fv_node, self.bow[b].fv_start, self.bow[b].fv_feat) if fv else (z, np.zeros(1, np.int32), z)
        fn, fs, ff = np.ascontiguousarray(fn, np.uint32), np.ascontiguousarray(fs, np.int32), np.ascontiguousarray(ff, np.uint32)
        return dict(keys_un=self.keys[b].astype(KP_DTYPE), desc=np.ascontiguousarray(self.desc[b], np.uint8).reshape(N, 32),
                    u_right=self.ur[b].astype(f32) if use_ur else np.full(N, -1.0, f32), fv_node=fn, fv_start=fs, fv_feat=ff, node_of_feat=_inverse(N, fs, ff))


def _same(got, exp, what):
    for k in ("keys_un", "desc", "u_right", "fv_node", "fv_start", "fv_feat", "node_of_feat"):
        assert got[k].shape == exp[k].shape and got[k].tobytes() == exp[k].tobytes(), "%s: %s differs" % (what, k)


def _host_made(ex, e, use_ur=True):
    """orbm_keyframe_create from host arrays `e` (a dict as fetch() gives it)"""
    view = views.key_frame_view(e["keys_un"], e["desc"], ex.GetScaleFactors(), ex.GetScaleSigmaSquares(), e["fv_node"], e["fv_start"], e["fv_feat"],
                                e["u_right"] if use_ur else None, None)
    return M.ResidentKeyFrame(ex, view)


def _close(*lists):
    for l in lists:
        for o in l:
            o.close()


def _order(B):
    return [2, 0, 2, 1] + list(range(B - 1, 2, -1))            # permuted, image 2 twice, image 1 blank


# ---- 1. contents, 2. a copy --------------------------------------------------------------------------------------------------------------------
def _contents(lib, shape, undist):
    w, h, nf, B = shape
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    if undist:
        ex.set_undistort(*_undistortion(w, h))
    voc = _vocabulary(ex)
    S = _Batch(ex, voc, _images(w, h, B, 700))
    assert S.n[1] == 0 and min(S.n[0], S.n[2]) > 100
    if undist:
        assert any(S.keys[b].tobytes() != S.raw[b].tobytes() for b in range(B))            # mvKeysUn is not mvKeys here
    else:
        assert all(S.keys[b].tobytes() == S.raw[b].tobytes() for b in range(B))            # orbx_fetch's keys
    frames = _order(B)
    kfs = M.ResidentKeyFrame.from_extracted(ex, voc, frames, use_u_right=True)
    assert len(kfs) == len(frames) and len({k._kf.value for k in kfs}) == len(frames)      # every occurrence an object of its own
    got = [k.fetch(ex) for k in kfs]
    exp = [S.expected(b) for b in frames]
    for j, b in enumerate(frames):
        assert kfs[j].N == S.n[b]
        _same(got[j], exp[j], "key frame %d (image %d)" % (j, b))
        hk = _host_made(ex, exp[j])
        _same(hk.fetch(ex), got[j], "key frame %d vs orbm_keyframe_create" % j)
        hk.close()
    # the inputs reach what the kernel can get wrong
    assert any((e["node_of_feat"] == -1).any() for e in exp), "no feature of a zero-weight word: choose another VOC_SEED"
    assert any(S.n[b] % 64 != 0 for b in frames) and any((e["u_right"] >= 0).any() for e in exp) and any((e["u_right"] < 0).any() for e in exp)
    assert all(len(e["fv_node"]) >= 3 for j, e in enumerate(exp) if S.n[frames[j]] > 0)        # levelsup = 2 of 3 levels: at most 6 nodes
    # no mvuRight; no FeatureVector (any image of the extraction)
    mono = M.ResidentKeyFrame.from_extracted(ex, voc, frames, use_u_right=False)
    bare = M.ResidentKeyFrame.from_extracted(ex, None, frames, use_u_right=True)
    for j, b in enumerate(frames):
        _same(mono[j].fetch(ex), S.expected(b, use_ur=False), "use_u_right = 0, key frame %d" % j)
        g = bare[j].fetch(ex)
        _same(g, S.expected(b, fv=False), "v = NULL, key frame %d" % j)
        assert len(g["fv_node"]) == 0 and (g["node_of_feat"] == -1).all()
    # 2. copies: another batch on the handle, other stereo results, another run of the vocabulary - the key frames keep what they held
    _Batch(ex, voc, _images(w, h, B, 900, blank=0), depth_seed=6)
    for j in range(len(frames)):
        _same(kfs[j].fetch(ex), got[j], "key frame %d after the next extraction" % j)
    voc.transform(np.random.default_rng(1).integers(0, 256, (40, 32), dtype=np.uint8), LEVELSUP)
    _same(kfs[0].fetch(ex), got[0], "key frame 0 after a host transform")
    _close(kfs, mono, bare); voc.close(); ex.close()


@pytest.mark.parametrize("undist", [True, False])
def test_contents_emulated(emu_lib, undist):
    _contents(emu_lib, EMU, undist)


@pytest.mark.gpu
@pytest.mark.parametrize("undist", [True, False])
def test_contents_gpu(hip_lib, undist):
    _contents(hip_lib, GPU, undist)


# ---- 3. the searches ---------------------------------------------------------------------------------------------------------------------------
SHIFT = 4          # batch B = batch A moved right by whole pixels: the same corners, detected again on another cell grid


def _two_batches(lib, shape):
    """batch A promoted on the device (dev_a) and made again from its fetched arrays (host_a); then batch B on the same handle, left on the device, and its key
    frames both ways (dev_b, host_b)"""
    w, h, nf, B = shape
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    voc = _vocabulary(ex)
    A = _Batch(ex, voc, _images(w, h, B, 700))
    dev_a = M.ResidentKeyFrame.from_extracted(ex, voc, list(range(B)), use_u_right=True)
    arr_a = [k.fetch(ex) for k in dev_a]
    host_a = [_host_made(ex, e) for e in arr_a]
    Bt = _Batch(ex, voc, _images(w, h, B, 700, shift=SHIFT))
    dev_b = M.ResidentKeyFrame.from_extracted(ex, voc, list(range(B)), use_u_right=True)
    arr_b = [k.fetch(ex) for k in dev_b]
    host_b = [_host_made(ex, e) for e in arr_b]
    return ex, voc, A, Bt, (dev_a, host_a, arr_a), (dev_b, host_b, arr_b)


def _against_reference(lib, shape):
    from matcher_world import Driver, KP
    ex, voc, A, Bt, (dev_a, host_a, arr_a), (dev_b, host_b, arr_b) = _two_batches(lib, shape)
    B = A.B
    rng = np.random.default_rng(97 + B)
    mps = [(rng.uniform(size=max(A.n[b], 1)) < 0.85).astype(np.uint8) for b in range(B)]
    I, z3 = np.eye(3, dtype=f32), np.zeros(3, f32)

    def set_fv(drv, keyframe, fid, nodes, st, ft):
        nodes = np.ascontiguousarray(nodes, np.uint32); st = np.ascontiguousarray(st, np.int32); ft = np.ascontiguousarray(ft, np.uint32)
        drv.L.mw_set_feat_vec(drv.w, int(keyframe), fid, len(nodes), nodes.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), ft.ctypes.data_as(C.c_void_p))
    for ratio, ori in PARAM_SETS:
        got = M.ORBmatcher(ratio, ori).SearchByBoWFramesBatch(ex, voc, dev_a, mps)
        for b in range(B):
            e, N = arr_a[b], Bt.n[b]
            kk = np.zeros(A.n[b], KP); kfr = np.zeros(N, KP)
            for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
                kk[f] = e["keys_un"][f]; kfr[f] = Bt.keys[b][f]
            drv = Driver(REF)
            cam = drv.camera()
            ids = np.full(A.n[b], -1, np.int32)
            for i in np.nonzero(mps[b][:A.n[b]])[0]:
                ids[i] = drv.mappoint(np.array([0, 0, 3.0]), np.array([0, 0, 1.0]), 0.5, 30.0, e["desc"][i])
            kf = drv.frame(True, kk, e["desc"], None, I, z3, cam); set_fv(drv, True, kf, e["fv_node"], e["fv_start"], e["fv_feat"]); drv.set_map_points(True, kf, ids)
            fr = drv.frame(False, kfr, Bt.desc[b], None, I, z3, cam); set_fv(drv, False, fr, Bt.bow[b].fv_node, Bt.bow[b].fv_start, Bt.bow[b].fv_feat)
            out = np.full(max(N, 1), -1, np.int32)
            n_ref = drv.L.mw_search_by_bow_frame(drv.w, kf, fr, out.ctypes.data_as(C.c_void_p), C.c_float(ratio), int(ori))
            drv.close()
            n_got, m12 = got[b]
            expd = np.full(max(N, 1), -1, np.int32)
            for i in np.nonzero(m12 >= 0)[0]:
                expd[m12[i]] = ids[i]
            print("frame %d ratio %g: %d matches, the reference %d" % (b, ratio, n_got, n_ref))
            assert n_got == n_ref and np.array_equal(expd[:N], out[:N]) and int((m12 >= 0).sum()) == n_ref, "frame %d ratio %g: %d vs %d matches" % (b, ratio, n_got, n_ref)
            assert A.n[b] == 0 or n_ref >= 40, "frame %d: the reference finds %d matches" % (b, n_ref)
    _close(dev_a, host_a, dev_b, host_b); voc.close(); ex.close()


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libmw_ref.so not built (needs the reference sources)")
def test_bow_frames_against_reference_emulated(emu_lib):
    _against_reference(emu_lib, EMU)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libmw_ref.so not built (needs the reference sources)")
def test_bow_frames_against_reference_gpu(hip_lib):
    _against_reference(hip_lib, GPU)


def _searches(lib, shape):
    """every other consumer of a resident key frame: the same results from key frames made on the device and from orbm_keyframe_create on the fetched arrays"""
    ex, voc, A, Bt, (dev_a, host_a, arr_a), (dev_b, host_b, arr_b) = _two_batches(lib, shape)
    w, h, nf, B = shape
    rng = np.random.default_rng(3)
    live_b = [b for b in range(B) if A.n[b] > 0 and Bt.n[b] > 0]
    mp1 = [(rng.uniform(size=max(A.n[b], 1)) < 0.85).astype(np.uint8) for b in range(B)]
    # SearchByBoW(pKF1, pKF2): key frame b of batch A against key frame b of batch B (the same scene, moved)
    for ratio, ori in PARAM_SETS:
        m = M.ORBmatcher(ratio, ori)
        rd = m.SearchByBoWResident(ex, [dev_a[b] for b in live_b], [mp1[b] for b in live_b], [dev_b[b] for b in live_b], [None] * len(live_b), frame_version=False)
        rh = m.SearchByBoWResident(ex, [host_a[b] for b in live_b], [mp1[b] for b in live_b], [host_b[b] for b in live_b], [None] * len(live_b), frame_version=False)
        for (nd, md), (nh, mh) in zip(rd, rh):
            assert nd == nh and np.array_equal(md, mh)
        assert sum(n for n, _ in rd) > 20 * len(live_b), [n for n, _ in rd]
    # SearchForTriangulation: a camera moved along x sees the scene shifted along the rows - F12 of that motion, the epipole far outside the image
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
    for only_stereo in (False, True):
        for b in live_b:
            m = M.ORBmatcher(0.6, True)
            td = m.SearchForTriangulationResident(ex, dev_a[b], None, [dev_b[b]], [None], [F12], [(-1e6, h / 2)], bOnlyStereo=only_stereo)
            th = m.SearchForTriangulationResident(ex, host_a[b], None, [host_b[b]], [None], [F12], [(-1e6, h / 2)], bOnlyStereo=only_stereo)
            assert td == th
            assert td[0][0] > 20, (b, only_stereo, td[0][0])
    # Fuse: map points in front of the features of key frame b (a third of them), searched in every key frame
    b0 = live_b[0]
    e = arr_a[b0]
    fx = fy = 0.8 * w; cx, cy = w / 2, h / 2
    pick = np.arange(0, A.n[b0], 3)
    zs = rng.uniform(2.0, 5.0, len(pick)).astype(f32)
    pos = np.stack([(e["keys_un"]["x"][pick] - cx) / fx * zs, (e["keys_un"]["y"][pick] - cy) / fy * zs, zs], axis=1).astype(f32)
    nrm = np.tile(np.array([0, 0, 1.0], f32), (len(pick), 1))
    sfs = ex.GetScaleFactors()
    max_d = (np.linalg.norm(pos, axis=1) * sfs[e["keys_un"]["octave"][pick]]).astype(f32)       # MapPoint::UpdateNormalAndDepth: the level they were seen at is predicted again
    pts = M.ResidentPoints(ex, pos, nrm, (max_d / sfs[-1]).astype(f32), max_d, e["desc"][pick])
    spec = M.fuse_spec((np.eye(3, dtype=f32), np.zeros(3, f32)), (fx, fy, cx, cy), (0.0, float(w), 0.0, float(h)), 40.0, float(np.log(sfs[1])))
    for inv_sigma2 in (ex.GetInverseScaleSigmaSquares(), None):
        bd, dd = M.ORBmatcher.FuseCandidatesBatch(ex, dev_a + dev_b, [spec] * (2 * B), pts, 3.0, inv_sigma2)
        bh, dh = M.ORBmatcher.FuseCandidatesBatch(ex, host_a + host_b, [spec] * (2 * B), pts, 3.0, inv_sigma2)
        assert np.array_equal(bd, bh) and np.array_equal(dd, dh)
        assert (bd[b0] >= 0).sum() > len(pick) // 4, int((bd[b0] >= 0).sum())
    # ComputeDistinctiveDescriptors over rows of the key frames
    P = 40
    nobs = rng.integers(1, 6, P)
    st = np.concatenate([[0], np.cumsum(nobs)]).astype(np.int32)
    okf = rng.choice(live_b, st[-1]).astype(np.int32)
    oft = np.array([rng.integers(0, A.n[k]) for k in okf], np.int32)
    cd = M.ComputeDistinctiveDescriptorsResident(ex, dev_a, st, okf, oft, want_desc=True)
    ch = M.ComputeDistinctiveDescriptorsResident(ex, host_a, st, okf, oft, want_desc=True)
    assert np.array_equal(cd[0], ch[0]) and np.array_equal(cd[1], ch[1]) and (cd[0] >= 0).all() and cd[1].any()
    pts.close(); _close(dev_a, host_a, dev_b, host_b); voc.close(); ex.close()


def test_searches_emulated(emu_lib):
    _searches(emu_lib, EMU)


@pytest.mark.gpu
def test_searches_gpu(hip_lib):
    _searches(hip_lib, GPU)


# ---- 4. rig ------------------------------------------------------------------------------------------------------------------------------------
def _rig(lib, shape):
    from test_branch_edges_triangulation import P1, P2, _KB8Pair
    w, h, nf, B = shape
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    voc = _vocabulary(ex)
    left = _images(w, h, B, 700, blank=None); right = _images(w, h, B, 800, blank=None, nrect=40)       # camera 2 sees fewer corners: Nright < Nleft
    left[1] = left[0]; right[1] = right[0]                      # rig frames 0 and 1 see the same scene: something to triangulate
    right[2] = 90                                                 # a rig frame whose camera 2 sees nothing
    res = ex.extract_batch(np.concatenate([left, right]))
    nl = [len(res[b][1]) for b in range(B)]; nr = [len(res[B + b][1]) for b in range(B)]
    assert all(a != b for a, b in zip(nl, nr)) and nr[2] == 0 and min(nr[0], nr[1]) > 50, (nl, nr)
    voc.transform_rig_extracted(ex, 0, ex, B, B, LEVELSUP)
    frames = _order(B)
    dev = M.ResidentKeyFrame.from_rig_extracted(ex, 0, ex, B, voc, frames)
    host, flags = [], []
    for j, b in enumerate(frames):
        N = nl[b] + nr[b]
        bow = voc.fetch(ex, b, N)
        fs, ff = np.ascontiguousarray(bow.fv_start, np.int32), np.ascontiguousarray(bow.fv_feat, np.uint32)
        e = dict(keys_un=np.concatenate([res[b][1], res[B + b][1]]).astype(KP_DTYPE), desc=np.concatenate([res[b][2], res[B + b][2]]).reshape(N, 32),
                 u_right=np.full(N, -1.0, f32), fv_node=np.ascontiguousarray(bow.fv_node, np.uint32), fv_start=fs, fv_feat=ff, node_of_feat=_inverse(N, fs, ff))
        assert dev[j].N == N
        _same(dev[j].fetch(ex), e, "rig key frame %d (frame %d)" % (j, b))
        host.append(_host_made(ex, e, use_ur=False))
        _same(host[j].fetch(ex), e, "rig key frame %d made by orbm_keyframe_create" % j)
        flags.append((np.random.default_rng(j).uniform(size=max(N, 1)) < 0.85).astype(np.uint8))
    n_frame = [nl[b] + nr[b] for b in range(B)]
    for ratio, ori in PARAM_SETS:
        m = M.ORBmatcher(ratio, ori)
        gd = m.SearchByBoWRigBatch(ex, 0, ex, B, voc, frames, dev, flags, n_frame)
        gh = m.SearchByBoWRigBatch(ex, 0, ex, B, voc, frames, host, flags, n_frame)
        for (a, x), (c, y) in zip(gd, gh):
            assert a == c and np.array_equal(x, y)
        assert sum(a for a, _ in gd) > 40 * len(frames), [a for a, _ in gd]
    # SearchForTriangulation with Kannala-Brandt cameras: rig key frame of frame 0 against that of frame 1
    j0, j1 = frames.index(0), frames.index(1)
    kb = _KB8Pair(); kb.nleft1 = nl[0]; kb.nleft2 = nl[1]
    kb.cam1[:] = list(P1) + list(P2); kb.cam2[:] = list(P1) + list(P2)
    kb.R[:] = [float(v) for v in np.eye(3, dtype=f32).ravel()] * 4; kb.t[:] = [0.3, 0.0, 0.0] * 4
    ep = np.array([-1e6, h / 2], f32)
    total = 0
    for only_stereo, coarse, ori in ((0, 1, 1), (0, 0, 1), (0, 1, 0)):
        outs = []
        for kfs in (dev, host):
            m12 = np.full(max(kfs[j0].N, 1), -1, np.int32); nm = np.zeros(1, np.int32)
            p2 = (C.c_void_p * 1)(kfs[j1]._kf); pm2 = (C.c_void_p * 1)(None)
            lib.check(lib.L.orbm_search_for_triangulation_resident_kb8(ex._h, kfs[j0]._kf, None, 1, p2, pm2, C.byref(kb), ep.ctypes.data, only_stereo, coarse, ori,
                                                                       m12.ctypes.data, nm.ctypes.data))
            outs.append((int(nm[0]), m12))
        assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1])
        total += outs[0][0] if coarse else 0
    assert total > 40, total
    _close(dev, host); voc.close(); ex.close()


def test_rig_emulated(emu_lib):
    _rig(emu_lib, EMU)


@pytest.mark.gpu
def test_rig_gpu(hip_lib):
    _rig(hip_lib, GPU)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def _refusals(lib, shape, second_device):
    w, h, nf, B = shape
    L = lib.L
    ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib); ex2 = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
    voc = _vocabulary(ex)
    imgs = _images(w, h, B, 700)
    fr = np.array([0, 2], np.int32)
    out = (C.c_void_p * 2)()

    def one(h_, v_, n, frames, use_ur, o, what):
        out[0] = out[1] = SENTINEL
        before = live(lib)
        rc = L.orbm_keyframe_create_extracted(h_, v_, n, None if frames is None else frames.ctypes.data, use_ur, o)
        assert rc == E_ARG, "%s: %d" % (what, rc)
        assert b"orbm_keyframe_create_extracted" in L.orbx_last_error(), what
        assert out[0] == SENTINEL and out[1] == SENTINEL and live(lib) == before, what

    def rig(hl, lf, hr, rf, v_, n, frames, o, what):
        out[0] = out[1] = SENTINEL
        before = live(lib)
        rc = L.orbm_keyframe_create_rig_extracted(hl, lf, hr, rf, v_, n, None if frames is None else frames.ctypes.data, o)
        assert rc == E_ARG, "%s: %d" % (what, rc)
        assert b"orbm_keyframe_create_rig_extracted" in L.orbx_last_error(), what
        assert out[0] == SENTINEL and out[1] == SENTINEL and live(lib) == before, what
    L.orbx_last_error.restype = C.c_char_p
    one(ex._h, None, 2, fr, 0, out, "no extraction yet")
    ex.extract_batch(imgs)
    one(ex._h, voc._v, 2, fr, 0, out, "no transform yet")
    voc.transform_extracted(ex, 0, B, LEVELSUP)
    one(ex._h, voc._v, 2, fr, 1, out, "use_u_right without stereo results")
    M.ComputeStereoFromRGBD(ex, _depth(w, h, 1, 5), 40.0, first=1)
    one(ex._h, voc._v, 2, fr, 1, out, "use_u_right, stereo results of another range")
    one(None, voc._v, 2, fr, 0, out, "null handle")
    one(ex._h, voc._v, 2, None, 0, out, "null frames")
    one(ex._h, voc._v, 2, fr, 0, None, "null out")
    one(ex._h, voc._v, -1, fr, 0, out, "n < 0")
    one(ex._h, None, 2, np.array([0, B], np.int32), 0, out, "index outside the extraction")
    one(ex._h, None, 2, np.array([-1, 0], np.int32), 0, out, "negative index")
    out[0] = out[1] = SENTINEL
    lib.check(L.orbm_keyframe_create_extracted(ex._h, voc._v, 0, fr.ctypes.data, 0, out))                     # n == 0
    lib.check(L.orbm_keyframe_create_rig_extracted(ex._h, 0, ex._h, 1, voc._v, 0, fr.ctypes.data, out))
    assert out[0] == SENTINEL and out[1] == SENTINEL
    rig(ex._h, 0, ex._h, 1, voc._v, 1, fr, out, "a one-camera transform given to the rig call")
    rig(ex._h, 0, ex._h, 1, None, 1, fr, out, "rig call without a vocabulary")
    voc.transform_extracted(ex, 1, B - 1, LEVELSUP)
    one(ex._h, voc._v, 2, fr, 0, out, "index outside the transform's range")
    ex2.extract_batch(imgs)
    voc.transform_extracted(ex2, 0, B, LEVELSUP)
    one(ex._h, voc._v, 2, fr, 0, out, "the transform ran on another handle")
    voc.transform_extracted(ex, 0, B, LEVELSUP)
    voc.transform(np.random.default_rng(1).integers(0, 256, (40, 32), dtype=np.uint8), LEVELSUP)
    one(ex._h, voc._v, 2, fr, 0, out, "the transform's results were overwritten")
    voc.transform_extracted(ex, 0, B, LEVELSUP)
    ex.extract_batch(imgs)
    one(ex._h, voc._v, 2, fr, 0, out, "another extraction since the transform")
    voc.transform_extracted(ex, 0, B, LEVELSUP)
    ex.set_undistort(*_undistortion(w, h))
    one(ex._h, voc._v, 2, fr, 0, out, "orbx_set_undistort since the extraction")
    one(ex._h, None, 2, fr, 0, out, "orbx_set_undistort since the extraction, no vocabulary")
    ex.set_undistort(None)
    ex.extract_batch(imgs)
    half = B // 2
    voc.transform_rig_extracted(ex, 0, ex, half, half, LEVELSUP)
    one(ex._h, voc._v, 2, fr, 0, out, "a rig transform given to the one-camera call")
    rig(ex._h, 0, ex._h, half, voc._v, 1, np.array([half], np.int32), out, "rig frame outside the transform")
    rig(ex._h, 0, ex._h, half - 1, voc._v, 1, fr, out, "rig call with another right range")
    rig(ex._h, 0, ex2._h, half, voc._v, 1, fr, out, "rig call with another right handle")
    ex.extract_batch(imgs)
    rig(ex._h, 0, ex._h, half, voc._v, 1, fr, out, "rig call after another extraction")
    if second_device:
        ex3 = ORBextractor(nf, 1.2, 8, 20, 7, device_id=1, lib=lib)
        ex3.extract_batch(imgs)
        voc.transform_extracted(ex, 0, B, LEVELSUP)
        one(ex3._h, voc._v, 2, fr, 0, out, "the vocabulary on another device")
        ex3.close()
    # after all that the call still works
    voc.transform_extracted(ex, 0, B, LEVELSUP)
    kfs = M.ResidentKeyFrame.from_extracted(ex, voc, fr)
    assert kfs[0].N > 100
    _close(kfs); voc.close(); ex.close(); ex2.close()


def test_refusals_emulated(emu_lib, monkeypatch):
    monkeypatch.setenv("ORBX_EMU_DEVICES", "2")
    _refusals(emu_lib, EMU, True)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib):
    _refusals(hip_lib, GPU, hip_lib.L.orbx_device_count() > 1)


# ---- 6. lifetime -------------------------------------------------------------------------------------------------------------------------------
def _lifetime(lib, shape):
    w, h, nf, B = shape
    start = live(lib)
    for handle_first in (False, True):
        ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
        voc = _vocabulary(ex)
        S = _Batch(ex, voc, _images(w, h, B, 700))
        kfs = M.ResidentKeyFrame.from_extracted(ex, voc, list(range(B)), use_u_right=True) + M.ResidentKeyFrame.from_extracted(ex, None, [0, 0])
        assert live(lib)[0] >= start[0] + len(kfs)
        got = M.ORBmatcher(0.7, True).SearchByBoWFramesBatch(ex, voc, kfs[:B], [np.ones(max(S.n[b], 1), np.uint8) for b in range(B)])
        assert got[0][0] > 100                                   # every frame against its own key frame
        half = B // 2
        ex.extract_batch(np.concatenate([_images(w, h, half, 700, blank=None), _images(w, h, half, 800, blank=None)]))
        voc.transform_rig_extracted(ex, 0, ex, half, half, LEVELSUP)
        rig = M.ResidentKeyFrame.from_rig_extracted(ex, 0, ex, half, voc, [0, 0])
        keep = rig[0].fetch(ex)
        if handle_first:                                         # the key frames outlive the handle they were made through
            ex2 = ORBextractor(nf, 1.2, 8, 20, 7, lib=lib)
            voc.close(); ex.close()
            _same(rig[1].fetch(ex2), keep, "rig key frame after its handle is gone")
            _close(kfs, rig); ex2.close()
        else:
            _close(kfs, rig); voc.close(); ex.close()
        assert live(lib) == start, (handle_first, live(lib), start)


def test_lifetime_emulated(emu_lib):
    _lifetime(emu_lib, EMU)


@pytest.mark.gpu
def test_lifetime_gpu(hip_lib):
    _lifetime(hip_lib, GPU)


# ---- 7. the C++ facade: ResidentKeyFrames::Adopt / ORBmatcher::AdoptImplicit -------------------------------------------------------------------
def _facade_adopt(tmp_path, libdir, libname):
    src = os.path.join(ol.ROOT, "tests", "cpp", "keyframe_adopt_probe.cpp")
    exe = tmp_path / "keyframe_adopt_probe"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ol.ROOT, "oracle", "opencv_shim"),
                    "-I" + ol.include_root(), src, "-o", str(exe), "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ADOPT OK" in r.stdout, r.stdout + r.stderr


def test_facade_adopt(emu_lib, tmp_path):
    _facade_adopt(tmp_path, *ol.emu_link())


@pytest.mark.gpu
def test_facade_adopt_gpu(hip_lib, tmp_path):
    from orb_slam3_detailed_comments_amd import _lib
    _facade_adopt(tmp_path, os.path.dirname(_lib.HIP_LIB_PATH), "orbx_hip")
