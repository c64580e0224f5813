"""Hand-built features for the kernels that read an extraction in place (helper, not a test).

The fisheye 2-NN (k_knn2_mfma / k_knn2), the fisheye triangulation (k_kb8_stereo) and the rectified stereo row search (k_stereo_match /
k_stereo_median) take the keypoint records, descriptor rows, counts and monoIndex of a handle's last batch straight from device memory.
ResidentBatch extracts a small batch - that sizes every buffer - and then overwrites chosen parts through the public C ABI:
orbx_device_outputs returns the device addresses, orbx_device_upload writes at a byte offset.  No product change, no new entry point.

Layout (csrc/orbx_api.cpp): keypoints [maxB][cap] KeyPointRec (extractor.KP_DTYPE, 28 bytes), descriptors [maxB][cap][32] bytes, n [maxB]
ints and, behind them in the same allocation, mono [maxB] ints - the distance between the two is taken from the two returned addresses.

What the consumers keep from the extraction and what they read again at every call (csrc/orbx_api.cpp):
  orbm_knn2            reads descriptors, n, mono at the call.  Nothing derived: all four may be injected.
  orbm_stereo_fisheye  the same plus the keypoint records (x, y, octave) of both sides at the call.  All may be injected.
  orbm_stereo_match    reads the left keypoint records, n and the descriptors at the call, but the right side through what the right
                       extraction's k_layout left behind: d_aux (band rows, x bits, octave per right keypoint) and the row buckets
                       d_rowstart / d_rowitems; the SAD windows come from the pyramids.  Injected keypoints or counts would disagree with
                       those, so for this consumer inject DESCRIPTORS ONLY.
  mvKeysUn (orbx_fetch_undistorted) is computed by the extraction: not consistent with injected keypoints either; none of the three
  consumers above reads it."""
import ctypes as C

import numpy as np

from orb_slam3_detailed_comments_amd import ORBextractor, synth
from orb_slam3_detailed_comments_amd.extractor import KP_DTYPE


def all_pairs_hamming(q, t):
    """[len(q), len(t)] popcount of the xor of 32-byte rows"""
    return np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2).astype(np.int32)


def knn2_expected(q, t):
    """BFMatcher(NORM_HAMMING).knnMatch(k = 2) + the ratio test of Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1553-1562): all-pairs popcount, neighbours
    by (distance, index) through a stable argsort, -1 where there is none, `DMatch::distance (float) < 0.7 (double) * DMatch::distance` in double"""
    nq = len(q)
    out = dict(idx0=np.full(nq, -1, np.int32), dist0=np.full(nq, -1, np.int32), idx1=np.full(nq, -1, np.int32), dist1=np.full(nq, -1, np.int32),
               ratio_ok=np.zeros(nq, np.uint8))
    if len(t) == 0:
        return out
    dist = all_pairs_hamming(q, t)
    order = np.argsort(dist, axis=1, kind="stable")
    rows = np.arange(nq)
    out["idx0"][:] = order[:, 0]; out["dist0"][:] = dist[rows, order[:, 0]]
    if len(t) > 1:
        out["idx1"][:] = order[:, 1]; out["dist1"][:] = dist[rows, order[:, 1]]
        out["ratio_ok"][:] = out["dist0"].astype(np.float32).astype(np.float64) < out["dist1"].astype(np.float32).astype(np.float64) * 0.7
    return out


def flip_bits(row, bits):
    """a copy of the 32-byte row with the given bit positions (0..255) inverted"""
    out = row.copy()
    for p in np.asarray(bits, np.int64).ravel():
        out[p >> 3] ^= np.uint8(1 << (p & 7))
    return out


def at_distance(rng, row, d):
    """a row at Hamming distance exactly d from `row`: d bit positions drawn without replacement"""
    return flip_bits(row, rng.choice(256, int(d), replace=False))


class ResidentBatch:
    """A handle whose last batch of `nimages` frames can be overwritten on the device.  keys / desc / n / mono are host mirrors ([nimages, cap] ..) that
    start as the natural extraction; change them and call put() (everything) or put_descriptors() to bring the device in line."""

    def __init__(self, lib, nimages, nfeatures=700, w=376, h=240, lap=(0, 0), images=None, seed=3):
        self.ex = ORBextractor(nfeatures, 1.2, 8, 20, 7, lib=lib)
        self._lib = lib
        if images is None:
            images = np.stack([synth.corner_field(w, h, seed=seed, nrect=600)] * nimages)
        self.natural = self.ex.extract_batch(images, lap)
        self.B = nimages
        p = [C.c_void_p() for _ in range(4)]; cap = C.c_int(); B = C.c_int()
        lib.check(lib.L.orbx_device_outputs(self.ex._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3]), C.byref(cap), C.byref(B)))
        assert B.value == nimages and cap.value == self.ex.max_keypoints()
        self.cap = cap.value
        self._kps, self._desc, self._n, self._mono = [x.value for x in p]
        self.mono_offset = self._mono - self._n                      # bytes: maxB ints, whatever maxB is
        assert self.mono_offset >= 4 * nimages and self.mono_offset % 4 == 0
        self.keys = np.zeros((nimages, self.cap), KP_DTYPE); self.desc = np.zeros((nimages, self.cap, 32), np.uint8)
        self.n = np.zeros(nimages, np.int32); self.mono = np.zeros(nimages, np.int32)
        for b, (m, k, d) in enumerate(self.natural):
            self.keys[b, :len(k)] = k; self.desc[b, :len(k)] = d; self.n[b] = len(k); self.mono[b] = m

    def _upload(self, addr, arr):
        arr = np.ascontiguousarray(arr)
        self._lib.check(self._lib.L.orbx_device_upload(self.ex._h, C.c_void_p(addr), arr.ctypes.data, arr.nbytes))

    def put_descriptors(self, b=None):
        """all descriptor rows (rows past n[b] included) of frame b, or of every frame"""
        if b is None:
            self._upload(self._desc, self.desc)
        else:
            self._upload(self._desc + b * self.cap * 32, self.desc[b])

    def put_keypoints(self, b=None):
        if b is None:
            self._upload(self._kps, self.keys)
        else:
            self._upload(self._kps + b * self.cap * KP_DTYPE.itemsize, self.keys[b])

    def put_counts(self):
        assert (self.n <= self.cap).all() and (self.mono >= 0).all() and (self.mono <= self.n).all(), "counts outside the buffers"
        self._upload(self._n, self.n)
        self._upload(self._n + self.mono_offset, self.mono)

    def put(self):
        self.put_keypoints(); self.put_descriptors(); self.put_counts()

    def close(self):
        self.ex.close()
