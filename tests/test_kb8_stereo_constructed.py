"""k_kb8_stereo (csrc/k_match.hip: the rest of Frame::ComputeStereoFishEyeMatches behind the 2-NN, KannalaBrandt8::TriangulateMatches per accepted query) on
keypoints and descriptors built for it and injected into a resident extraction (tests/resident_inject.py).  From real images the kernel only ever sees what the
2-NN hands it; here the matches are chosen: a right descriptor is a copy of its left one (0 bits flipped), everything else is unrelated random rows.

Expected depth and p3d: csrc/kb8_model.h compiled for the HOST (g++ -O2 -ffp-contract=off, tests/cpp/kb8_host_model.cpp), bit for bit.  On the emulator that
checks the kernel's bookkeeping; on the GPU it also compares the device compiler's build of the camera chain - unproject, Jacobi SVD, project with the glibc
models of tanf, atan2f, cosf, sinf - with the host's at chosen arguments.  The projection feeds only the two chi-square gates, so beside the gross outcomes the
inputs hold pairs whose shifted pixel is the LAST float the host model still accepts and its neighbour, the first it rejects: a projection that is off by an ulp
flips one of them.  Expected l2r, r2l and n are replayed in numpy from the host depths: accept when z > 1e-4, the largest left index wins a right keypoint.

Rigs: the TUM-VI pair of tests/test_kb8.py, and a 2 mm rig without rotation: with TUM-VI's tz = 1 mm and 2.7 degrees of pitch no point that both cameras see
inside the theta_d clamp has 0 < z <= 1e-4 (z2 > 0 needs 0.0469 y + z > 1.05e-3, the clamp z >= |y| / 72), so the acceptance threshold itself is exercised on the small rig:
depths either side of 1e-4, and pairs searched among neighbouring float pixels until the host model's depth is float(1e-4) EXACTLY (refused: the comparison is strict),
the float above it (accepted) and the float below.

Rejection codes of the host model: -1 parallax below the gate, -2 z1 <= 0, -3 z2 <= 0, -4 / -5 the chi-square gate in camera 1 / 2."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import matcher as M, sophus
from resident_inject import ResidentBatch, knn2_expected

ROOT = ol.ROOT
CSRC = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")
f32 = np.float32

# Examples/Stereo/TUM-VI.yaml (as tests/test_kb8.py)
CAM1 = [190.978477, 190.973307, 254.931706, 256.897442, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736]
CAM2 = [190.442369, 190.434438, 252.598711, 254.917238, 0.003400603976, 0.001766924711, -0.002663898171, 0.000329921072]
RLR = np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224],
                [-0.000823363992158, 0.998899461915674, 0.046895490788700],
                [-0.000656143613422, -0.046896036240590, 0.998899559977407]], np.float32)
TLR = np.array([0.100931237881590, 0.000570764538347, 0.001046438762054], np.float32)
RIG_TUMVI = dict(cam1=CAM1, cam2=CAM2, R12=sophus.SE3f(RLR, TLR).rotationMatrix(), t12=TLR)
RIG_SMALL = dict(cam1=CAM1, cam2=CAM2, R12=np.eye(3, dtype=np.float32), t12=np.array([0.002, 0, 0], np.float32))

_MODEL = []


def host_model():
    """csrc/kb8_model.h built for the host as the emulator library is: no FMA contraction"""
    if not _MODEL:
        _MODEL.append(_model_build(["-ffp-contract=off"]))
    return _MODEL[0]


def _model_build(flags):
    """flags = ["-march=x86-64-v3", "-ffp-contract=fast"] gives the contracted build to compare with when a device result differs: on these scenes it moves 519 of
    640 depths of frame pair 0 in their last bits and flips 16 gate decisions of frame pair 1 (profiles/resident_inject/README.md)"""
    td = tempfile.mkdtemp(prefix="kb8_host_model_")
    so = os.path.join(td, "kb8_host_model.so")
    subprocess.run(["g++", "-O2"] + flags + ["-shared", "-fPIC", "-DORBX_EMU", "-I" + os.path.join(ROOT, "tests", "emu"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "kb8_host_model.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.kb8_unproject.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_void_p]
    L.kb8_triangulate_matches.argtypes = [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 2
    return L


def triangulate(rig, uv1, uv2, s1, s2, model=None):
    """(z or rejection code [n], p3d [n, 3]) of the host model"""
    L = model or host_model()
    a = lambda x: np.ascontiguousarray(x, np.float32)
    c1, c2, R, t, uv1, uv2, s1, s2 = a(rig["cam1"]), a(rig["cam2"]), a(rig["R12"]), a(rig["t12"]), a(uv1).reshape(-1, 2), a(uv2).reshape(-1, 2), a(s1), a(s2)
    n = len(uv1)
    z = np.zeros(n, np.float32); p = np.zeros((n, 3), np.float32)
    L.kb8_triangulate_matches(c1.ctypes.data, c2.ctypes.data, R.ctypes.data, t.ctypes.data, uv1.ctypes.data, uv2.ctypes.data, s1.ctypes.data, s2.ctypes.data, n,
                              z.ctypes.data, p.ctypes.data)
    return z, p


# ---- float64 camera, only to place pixels (nothing expected comes from it) -----------------------------------------------------------------------------------
def _dir64(cam, uv):
    """unit viewing direction of a pixel: Kannala-Brandt unprojection by Newton's method in float64, theta_d clamped like the reference"""
    fx, fy, cx, cy, k1, k2, k3, k4 = [np.float64(f32(v)) for v in cam]
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    x = (uv[:, 0] - cx) / fx; y = (uv[:, 1] - cy) / fy
    td = np.minimum(np.sqrt(x * x + y * y), np.pi / 2)
    th = td.copy()
    for _ in range(30):
        t2 = th * th
        th = th - (th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td) / (1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4))))
    psi = np.arctan2(y, x)
    return np.stack([np.sin(th) * np.cos(psi), np.sin(th) * np.sin(psi), np.cos(th)], 1)


def _project64(cam, p):
    fx, fy, cx, cy, k1, k2, k3, k4 = [np.float64(f32(v)) for v in cam]
    th = np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2]); psi = np.arctan2(p[:, 1], p[:, 0])
    t2 = th * th
    r = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], 1)


def _right_pixels(rig, X, behind=False):
    """float32 pixels of the points X (camera 1 coordinates) in camera 2; behind: the pixel whose ray passes through X backwards (X lies behind camera 2)"""
    R21 = rig["R12"].astype(np.float64).T
    X2 = (X - rig["t12"].astype(np.float64)[None, :]) @ R21.T
    return _project64(rig["cam2"], -X2 if behind else X2).astype(np.float32)


def _flip_pairs(rig, uv1, uv2, oL, oR, sigma2, side):
    """For every pair (accepted as it stands) the v coordinate of the left (side 0) or right (side 1) pixel is raised until the host model rejects, then bisected down to
    two neighbouring floats: returns (uv of the last accepted, uv of the first rejected) for that side."""
    uv = (uv1, uv2)[side].copy()
    lo = uv[:, 1].copy(); hi = (lo + f32(40.0)).astype(np.float32)

    def accepted(v):
        a = uv.copy(); a[:, 1] = v
        z, _ = triangulate(rig, a if side == 0 else uv1, uv2 if side == 0 else a, sigma2[oL], sigma2[oR])
        return z > 0
    assert accepted(lo).all() and not accepted(hi).any()
    for _ in range(40):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) / 2).astype(np.float32)
        done = (mid == lo) | (mid == hi)
        ok = accepted(mid)
        lo = np.where(~done & ok, mid, lo); hi = np.where(~done & ~ok, mid, hi)
    assert (np.nextafter(lo, f32(np.inf)) == hi).all()
    a, b = uv.copy(), uv.copy()
    a[:, 1] = lo; b[:, 1] = hi
    return a, b


class Scene:
    """one (left frame, right frame) pair: keypoints, descriptors, counts, and the replayed expectation"""

    def __init__(self, rig, sigma2, mono_l, mono_r, seed):
        self.rig, self.sigma2, self.mono_l, self.mono_r = rig, sigma2, mono_l, mono_r
        self.rng = np.random.default_rng(seed)
        self.left = []          # (u, v, octave, descriptor row)
        self.right = []

    def _row(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def add_pairs(self, uv1, uv2, oL, oR):
        """matched pairs: the right descriptor is the left one; returns the left query rows"""
        first = len(self.left)
        for a, b, p, q in zip(np.asarray(uv1, np.float32).reshape(-1, 2), np.asarray(uv2, np.float32).reshape(-1, 2), np.broadcast_to(oL, len(uv1)), np.broadcast_to(oR, len(uv1))):
            d = self._row()
            self.left.append((a[0], a[1], int(p), d)); self.right.append((b[0], b[1], int(q), d))
        return np.arange(first, len(self.left))

    def add_left_on(self, right_row, uv1, oL):
        """one more left keypoint whose descriptor is that of an existing right keypoint (several left keypoints on one right keypoint)"""
        self.left.append((f32(uv1[0]), f32(uv1[1]), int(oL), self.right[right_row][3]))
        return len(self.left) - 1

    def add_unmatched(self, n_left, n_right):
        for _ in range(n_left):
            self.left.append((f32(self.rng.uniform(0, 512)), f32(self.rng.uniform(0, 512)), int(self.rng.integers(0, 8)), self._row()))
        for _ in range(n_right):
            self.right.append((f32(self.rng.uniform(0, 512)), f32(self.rng.uniform(0, 512)), int(self.rng.integers(0, 8)), self._row()))

    def shuffle(self):
        """the queries and the right keypoints in random order (matched pairs keep their descriptors, so the 2-NN finds them wherever they are)"""
        pl = self.rng.permutation(len(self.left)); pr = self.rng.permutation(len(self.right))
        self.left = [self.left[i] for i in pl]; self.right = [self.right[i] for i in pr]

    def finish(self, cap):
        """arrays for injection + the expected outputs"""
        from orb_slam3_detailed_comments_amd.extractor import KP_DTYPE
        rng = self.rng
        out = {}
        for side, rows, mono in (("L", self.left, self.mono_l), ("R", self.right, self.mono_r)):
            n = mono + len(rows)
            assert n <= cap, (side, n, cap)
            k = np.zeros(cap, KP_DTYPE); d = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
            k["x"] = rng.uniform(0, 512, cap).astype(np.float32); k["y"] = rng.uniform(0, 512, cap).astype(np.float32); k["octave"] = rng.integers(0, 8, cap)
            k["size"] = 31; k["angle"] = 0; k["response"] = 20; k["class_id"] = -1
            for i, (u, v, o, row) in enumerate(rows):
                k["x"][mono + i] = u; k["y"][mono + i] = v; k["octave"][mono + i] = o; d[mono + i] = row
            out[side] = (k, d, n)
        kL, dL, nL = out["L"]; kR, dR, nR = out["R"]
        # bait: the monocular rows of the right frame and the rows past its count repeat query descriptors - a 2-NN that read them would return them at distance 0
        nq = len(self.left)
        if nq:
            for i in list(range(self.mono_r)) + list(range(nR, min(nR + 8, cap))):
                dR[i] = dL[self.mono_l + (i * 7) % nq]
        self.kL, self.dL, self.nL, self.kR, self.dR, self.nR = kL, dL, nL, kR, dR, nR
        nn = knn2_expected(dL[self.mono_l:nL], dR[self.mono_r:nR])
        l2r = np.full(cap, -1, np.int32); r2l = np.full(cap, -1, np.int32); depth = np.full(cap, -1, np.float32); p3d = np.zeros((cap, 3), np.float32)
        q = np.flatnonzero(nn["ratio_ok"])
        i = q + self.mono_l; j = nn["idx0"][q] + self.mono_r
        z, p = triangulate(self.rig, np.stack([kL["x"][i], kL["y"][i]], 1), np.stack([kR["x"][j], kR["y"][j]], 1), self.sigma2[kL["octave"][i]], self.sigma2[kR["octave"][j]])
        self.match = np.full(cap, -1, np.int32); self.match[i] = j                 # per left keypoint: the right keypoint the ratio test hands to the triangulation
        self.code = np.full(cap, 0, np.int32)                                  # per left keypoint: 1 accepted, -1 .. -5 rejected by that gate, -6 depth <= 1e-4, 0 no ratio match
        self.model_z = np.full(cap, np.nan, np.float32); self.model_z[i] = z    # per left keypoint: what the host model returned (depth or rejection code)
        n_acc = 0
        for a, b, zz, pp in zip(i, j, z, p):                                  # ascending left index: the last writer of r2l[j] is the largest
            if zz > f32(0.0001):
                l2r[a] = b; depth[a] = zz; p3d[a] = pp; r2l[b] = a; n_acc += 1
                self.code[a] = 1
            else:
                self.code[a] = int(zz) if zz < 0 else -6
        self.exp = dict(l2r=l2r, r2l=r2l, depth=depth, p3d=p3d, n=n_acc)
        for v in (l2r, r2l, depth, p3d, self.code):
            v.setflags(write=False)
        return self


def _grid_pixels(cam):
    """left pixels for the camera chain: the principal point and its four neighbours, both axes, the four quadrants, radii up to and beyond the theta_d clamp
    (fx pi / 2 = 300 px)"""
    cx, cy = f32(cam[2]), f32(cam[3])
    px = [(cx, cy), (cx + f32(1), cy), (cx - f32(1), cy), (cx, cy + f32(1)), (cx, cy - f32(1))]
    radii = (0.25, 3.0, 20.0, 60.0, 110.0, 170.0, 230.0, 270.0, 290.0, 298.0, 299.9, 300.5, 310.0)
    for r in radii:
        px += [(cx + f32(r), cy), (cx - f32(r), cy), (cx, cy + f32(r)), (cx, cy - f32(r))]                    # the axes: psi = 0, pi, +-pi / 2
        for deg in (45.0, 135.0, 225.0, 315.0, 10.0, 100.0, 190.0, 280.0, 80.0, 170.0, 260.0, 350.0):           # every quadrant of psi, near both ends of each
            px.append((cx + f32(r * np.cos(np.radians(deg))), cy + f32(r * np.sin(np.radians(deg)))))
    return np.array(px, np.float32)


def _float_steps(v, ks):
    out = np.zeros(len(ks), np.float32)
    for n, k in enumerate(ks):
        x = f32(v)
        for _ in range(abs(int(k))):
            x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
        out[n] = x
    return out


def _pairs_at_depth(rig, sigma2, targets, want=2, seed=1):
    """Pixel pairs (octave 0 on both sides) whose depth by the host model is EXACTLY one of `targets`: points near 1e-4 on rays like those of the small-rig frame, then the
    121 x 121 neighbouring floats of (left v, right u) - some 5 000 to 9 000 distinct depths within 1e-7 of the point's - searched for the values.  {target: (uv1, uv2)}"""
    rng = np.random.default_rng(seed)
    ks = np.arange(-60, 61)
    found = {f32(t): ([], []) for t in targets}
    for _ in range(200):
        if all(len(v[0]) >= want for v in found.values()):
            break
        z0 = np.array([1e-4 * (1 + rng.uniform(-1e-3, 1e-3))])
        X = np.stack([rng.uniform(0.0005, 0.002) * z0 / 1e-4, rng.uniform(0.002, 0.004) * z0 / 1e-4, z0], 1)
        u1 = _project64(rig["cam1"], X).astype(np.float32); u2 = _right_pixels(rig, X)
        xs = _float_steps(u2[0, 0], ks); ys = _float_steps(u1[0, 1], ks)
        A = np.zeros((len(ks) ** 2, 2), np.float32); B = np.zeros_like(A)
        A[:, 0] = u1[0, 0]; A[:, 1] = np.repeat(ys, len(ks)); B[:, 0] = np.tile(xs, len(ks)); B[:, 1] = u2[0, 1]
        z, _ = triangulate(rig, A, B, np.full(len(A), sigma2[0]), np.full(len(A), sigma2[0]))
        for t, (l, r) in found.items():
            hit = np.flatnonzero(z == t)
            if len(hit) and len(l) < want:
                l.append(A[hit[0]].copy()); r.append(B[hit[0]].copy())
    assert all(len(v[0]) >= want for v in found.values()), {float(t): len(v[0]) for t, v in found.items()}
    return {t: (np.array(l), np.array(r)) for t, (l, r) in found.items()}


def build_scenes(sigma2, cap):
    """[(rig, [Scene per frame pair])] - made once, shared by the emulator and the GPU form"""
    rng = np.random.default_rng(21)
    rig = RIG_TUMVI

    def points_on(uv1, dist):
        return _dir64(rig["cam1"], uv1) * np.asarray(dist, np.float64).reshape(-1, 1)

    # ---- frame pair 0: more than two workgroups of accepted pairs, 40 right keypoints matched by 3 left keypoints each --------------------------------------
    s0 = Scene(rig, sigma2, 11, 7, 1)
    n_bulk = 560
    ang = rng.uniform(0, 2 * np.pi, n_bulk); rad = rng.uniform(2, 215, n_bulk)
    uv1 = np.stack([f32(CAM1[2]) + rad * np.cos(ang), f32(CAM1[3]) + rad * np.sin(ang)], 1).astype(np.float32)
    X = points_on(uv1, rng.uniform(0.4, 1.2, n_bulk))
    oL = np.arange(n_bulk) % 8; oR = (np.arange(n_bulk) // 8) % 8                                               # every (left octave, right octave)
    bulk = s0.add_pairs(uv1, _right_pixels(rig, X), oL, oR)
    triples = []
    for t in range(40):
        j = int(bulk[t * 13])                                                                                  # the right keypoint (the rows are parallel until shuffle())
        u, v = s0.left[j][0], s0.left[j][1]
        # two more left keypoints at the same pixel (other octaves); in every other triple the LAST one is 30 px off: rejected, the middle one must win
        a = s0.add_left_on(j, (u, v), (t + 3) % 8)
        b = s0.add_left_on(j, (u, v + f32(30.0 if t & 1 else 0.0)), (t + 5) % 8)
        triples.append((j, a, b))
    s0.add_unmatched(40, 30)
    s0.shuffle()
    s0.finish(cap)

    # ---- frame pair 1: the camera chain at chosen pixels and every outcome -------------------------------------------------------------------------------------
    s1 = Scene(rig, sigma2, 5, 9, 2)
    g = _grid_pixels(CAM1)
    s1.add_pairs(g, _right_pixels(rig, points_on(g, np.full(len(g), 0.8))), np.arange(len(g)) % 8, (np.arange(len(g)) // 3) % 8)
    m = 12
    ang = rng.uniform(0, 2 * np.pi, m); rad = rng.uniform(5, 150, m)
    base = np.stack([f32(CAM1[2]) + rad * np.cos(ang), f32(CAM1[3]) + rad * np.sin(ang)], 1).astype(np.float32)
    # parallax below the gate: far points
    s1.add_pairs(base, _right_pixels(rig, points_on(base, np.full(m, 40.0))), 2, 3)
    # z1 <= 0: the right pixel as if the disparity had the other sign - the rays meet behind both cameras
    d1 = _dir64(rig["cam1"], base)
    s1.add_pairs(base, _right_pixels(rig, 2.0 * rig["t12"].astype(np.float64)[None, :] + d1 * 1.0), 1, 1)
    # z2 <= 0: a point in front of camera 1 and, by camera 2's pitch of 2.7 degrees, behind camera 2 - rays 86.5 to 88.5 degrees above the axis (pixel radii 289.5 to 296.2; further out camera 2 clamps theta_d and the rays meet behind camera 1)
    up = np.stack([f32(CAM1[2]) + np.linspace(-12, 12, m), f32(CAM1[3]) - np.linspace(289.5, 296.2, m)], 1).astype(np.float32)
    s1.add_pairs(up, _right_pixels(rig, points_on(up, rng.uniform(0.5, 2.0, m)), behind=True), 0, 0)
    # the chi-square gates by a shifted pixel: 9 px against the level's sigma2 - the tight gate is camera 1's (octaves 0 / 7), then camera 2's (7 / 0)
    good = _right_pixels(rig, points_on(base, np.full(m, 0.7)))
    s1.add_pairs(base, good + np.array([0, 9.0], np.float32), 0, 7)
    s1.add_pairs(base, good + np.array([0, 9.0], np.float32), 7, 0)
    # .. and at the float where each gate flips
    oL0, oR0 = np.zeros(m, np.int64), np.full(m, 7)
    a, b = _flip_pairs(rig, base, good, oL0, oR0, sigma2, 0); s1.add_pairs(a, good, oL0, oR0); s1.add_pairs(b, good, oL0, oR0)
    a, b = _flip_pairs(rig, base, good, oR0, oL0, sigma2, 1); s1.add_pairs(base, a, oR0, oL0); s1.add_pairs(base, b, oR0, oL0)
    a, b = _flip_pairs(rig, base, good, np.full(m, 3), np.full(m, 3), sigma2, 1); s1.add_pairs(base, a, 3, 3); s1.add_pairs(base, b, 3, 3)
    s1.add_unmatched(20, 20)
    s1.shuffle()
    s1.finish(cap)

    # ---- frame pair 2: nothing accepted ----------------------------------------------------------------------------------------------------------------------------
    s2 = Scene(rig, sigma2, 3, 4, 3)
    s2.add_pairs(base, _right_pixels(rig, points_on(base, np.full(m, 40.0))), 2, 3)
    s2.add_pairs(base, _right_pixels(rig, 2.0 * rig["t12"].astype(np.float64)[None, :] + d1 * 1.0), 1, 1)
    s2.add_pairs(up, _right_pixels(rig, points_on(up, np.full(m, 1.0)), behind=True), 0, 0)
    s2.add_pairs(base, good + np.array([0, 9.0], np.float32), 0, 7)
    s2.add_pairs(base, good + np.array([0, 9.0], np.float32), 7, 0)
    s2.add_unmatched(300, 100)
    s2.shuffle()
    s2.finish(cap)

    # ---- the 2 mm rig: depths either side of the acceptance threshold 1e-4 -------------------------------------------------------------------------------------
    small = RIG_SMALL
    s3 = Scene(small, sigma2, 2, 1, 4)
    zs = np.array([0.5e-4, 0.8e-4, 0.95e-4, 0.999e-4, 1.0e-4, 1.001e-4, 1.05e-4, 1.2e-4, 2e-4, 1e-3, 0.9e-4, 1.1e-4], np.float64)
    X = np.stack([np.full(len(zs), 0.001) * zs / 1e-4, 0.003 * zs / 1e-4, zs], 1)                                 # rays 88.6 degrees off the axis, inside the clamp
    u1 = _project64(small["cam1"], X).astype(np.float32)
    s3.add_pairs(u1, _right_pixels(small, X), 0, 0)
    # .. and ON it: `depth > 0.0001f` (src/Frame.cc:1573) refuses float(1e-4) itself and takes the next float
    th = f32(0.0001)
    for uv1, uv2 in _pairs_at_depth(small, sigma2, (th, np.nextafter(th, f32(1)), np.nextafter(th, f32(0)))).values():
        s3.add_pairs(uv1, uv2, 0, 0)
    s3.add_unmatched(5, 5)
    s3.finish(cap)
    empty = Scene(small, sigma2, 0, 0, 5).finish(cap)
    return [(rig, [s0, s1, s2]), (small, [s3, empty, empty])], triples


_SCENES = {}
PAIRS = 3


def _scenes(rb):
    key = (rb.cap, rb.ex.GetScaleSigmaSquares().tobytes())
    if key not in _SCENES:
        _SCENES[key] = build_scenes(rb.ex.GetScaleSigmaSquares().astype(np.float32), rb.cap)
    return _SCENES[key]


def _check_construction(groups):
    (rig, (s0, s1, s2)), (_, (s3, _, _)) = groups
    count = lambda s, c: int((s.code == c).sum())
    print("pair 0:", {c: count(s0, c) for c in (1, 0, -1, -2, -3, -4, -5, -6)}, "pair 1:", {c: count(s1, c) for c in (1, 0, -1, -2, -3, -4, -5, -6)},
          "pair 2:", {c: count(s2, c) for c in (1, 0, -1, -2, -3, -4, -5, -6)}, "small rig:", {c: count(s3, c) for c in (1, -6)}, s3.exp["depth"][s3.exp["depth"] > 0])
    assert s0.exp["n"] >= 600 and s0.mono_l > 0 and s0.mono_r > 0
    # 40 right keypoints with three accepted-or-not left keypoints each; the winner is the largest ACCEPTED left index, which is not always the largest
    rows = {}
    for i in np.flatnonzero(s0.match >= 0):
        rows.setdefault(int(s0.match[i]), []).append(int(i))
    multi = {j: v for j, v in rows.items() if len(v) == 3}
    assert len(multi) == 40
    assert sum(1 for j, v in multi.items() if all(s0.code[i] == 1 for i in v)) >= 15
    assert sum(1 for j, v in multi.items() if s0.exp["r2l"][j] != max(v) and s0.exp["r2l"][j] == sorted(v)[1]) >= 5
    assert sum(1 for j, v in multi.items() if s0.exp["r2l"][j] != min(v)) == 40                                  # atomicMin would give another answer at every one
    assert sum(1 for j, v in multi.items() if (max(v) >> 8) != (min(v) >> 8)) >= 20                              # .. and the writers sit in different workgroups
    # the per-side sigma2: accepted pairs whose octaves differ, with outcomes that swapping the sides would change
    for c in (1, -1, -2, -3, -4, -5):
        assert count(s1, c) >= 8, "outcome %d occurs %d times in the constructed frame" % (c, count(s1, c))
    for c in (-1, -2, -3, -4, -5):
        assert count(s2, c) >= 8
    assert s2.exp["n"] == 0 and (s2.exp["r2l"] == -1).all() and (s2.exp["depth"] == -1).all()
    assert count(s3, -6) >= 3 and count(s3, 1) >= 3, "depths on both sides of 1e-4"
    th = f32(0.0001)
    on, above, below = s3.model_z == th, s3.model_z == np.nextafter(th, f32(1)), s3.model_z == np.nextafter(th, f32(0))
    assert on.sum() >= 2 and above.sum() >= 2 and below.sum() >= 2, "depths of exactly float(1e-4) and its two neighbours: %d, %d, %d" % (on.sum(), above.sum(), below.sum())
    assert (s3.code[on] == -6).all() and (s3.code[below] == -6).all() and (s3.code[above] == 1).all()
    acc = np.flatnonzero(s0.code == 1)
    assert {(int(a), int(b)) for a, b in zip(s0.kL["octave"][acc], s0.kR["octave"][s0.match[acc]])} >= {(a, b) for a in range(8) for b in range(8)}   # sigma2 is picked per side


def _check(lib):
    rb = ResidentBatch(lib, 2 * PAIRS)
    try:
        groups, _ = _scenes(rb)
        _check_construction(groups)
        cap = rb.cap
        for rig, scenes in groups:
            for p, s in enumerate(scenes):
                rb.keys[p] = s.kL; rb.desc[p] = s.dL; rb.n[p] = s.nL; rb.mono[p] = s.mono_l
                rb.keys[PAIRS + p] = s.kR; rb.desc[PAIRS + p] = s.dR; rb.n[PAIRS + p] = s.nR; rb.mono[PAIRS + p] = s.mono_r
            rb.put()
            for flags in (0, 8):
                rb.ex.debug_stereo_flags(flags)
                out = M.ComputeStereoFishEyeMatches(rb.ex, rb.ex, rig["cam1"], rig["cam2"], rig["R12"], rig["t12"], 0, PAIRS, PAIRS)
                for p, s in enumerate(scenes):
                    e = s.exp
                    assert np.array_equal(out["l2r"][p], e["l2r"]), "pair %d flags %d: l2r differs at left keypoints %s" % (p, flags, np.flatnonzero(out["l2r"][p] != e["l2r"])[:8])
                    bad = np.flatnonzero(out["depth"][p].view(np.uint32) != e["depth"].view(np.uint32))
                    assert len(bad) == 0, "pair %d flags %d: depth differs at %s: %r vs %r" % (p, flags, bad[:8], out["depth"][p][bad[:8]], e["depth"][bad[:8]])
                    assert out["p3d"][p].tobytes() == e["p3d"].tobytes(), "pair %d flags %d: p3d differs" % (p, flags)
                    assert np.array_equal(out["r2l"][p], e["r2l"]), "pair %d flags %d: r2l differs at right keypoints %s" % (p, flags, np.flatnonzero(out["r2l"][p] != e["r2l"])[:8])
                    assert int(out["n"][p]) == e["n"], (p, flags, int(out["n"][p]), e["n"])
    finally:
        rb.ex.debug_stereo_flags(0)
        rb.close()


def test_kb8_stereo_constructed_emulated(emu_lib):
    _check(emu_lib)


@pytest.mark.gpu
def test_kb8_stereo_constructed_gpu(hip_lib):
    _check(hip_lib)
