"""Hand-built frames, key frames and point lists for the tests of the host replays (helper, not a test: tests/test_host_replay_gates.py, tests/test_host_rotation_gates.py).

A scene is a lattice of `spots` 24 px apart on a 376 x 240 image.  Every case owns one spot: its keypoints sit within 1 px of it, its points project onto it, and no search
window used here (at most 3 * 1.2^7 = 10.8 px) reaches a neighbouring spot - so a case's outcome follows from its own few keypoints and can be written down beside it.
Candidate order: the reference's GetFeaturesInArea walks the grid cells by column, then row, then the cell's keypoints by index; the keypoints of a spot are added with
ascending x and index, so the order of the list is the order they were added in, whether they share a cell or not.
Descriptors: flip(base, lo, hi) inverts the bits lo .. hi - 1, so distances between rows made from one base over disjoint bit ranges add up exactly."""
import numpy as np

from orb_slam3_detailed_comments_amd import views
from orb_slam3_detailed_comments_amd.extractor import KP_DTYPE
from resident_inject import flip_bits

f32 = np.float32
W, H = 376, 240
SF = np.cumprod(np.array([1.0] + [1.2] * 7, f32), dtype=f32)
SIGMA2 = (SF * SF).astype(f32)
STEP = 24


def flip(base, lo, hi):
    return flip_bits(base, np.arange(lo, hi))


def spots():
    """the lattice, row by row"""
    for y in range(24, H - 23, STEP):
        for x in range(24, W - 23, STEP):
            yield float(x), float(y)


def up(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(np.inf))
    return float(x)


def down(x, n=1):
    x = f32(x)
    for _ in range(n):
        x = np.nextafter(x, f32(-np.inf))
    return float(x)


class Keys:
    """the keypoints of one hand-built frame"""

    def __init__(self):
        self.rows, self.desc, self.occupied, self.u_right = [], [], [], []

    def add(self, x, y, octave, desc, angle=0.0, occupied=0, u_right=-1.0):
        self.rows.append((x, y, 31.0 * float(SF[octave]), angle, 1.0, octave, -1)); self.desc.append(np.asarray(desc, np.uint8))
        self.occupied.append(occupied); self.u_right.append(u_right)
        return len(self.rows) - 1

    def __len__(self):
        return len(self.rows)

    def arrays(self):
        return np.array(self.rows, KP_DTYPE), np.array(self.desc, np.uint8).reshape(-1, 32)

    def frame_view(self, bounds=None, occupied=True):
        k, d = self.arrays()
        return views.frame_view(k, d, SF, W, H, u_right=np.array(self.u_right, f32), occupied=np.array(self.occupied, np.uint8) if occupied else None, mbf=0.0, bounds=bounds)

    def key_frame_view(self, node_of_feature, has_map_point):
        """mFeatVec from one vocabulary node per feature (features of a node in index order, as DBoW2 adds them)"""
        k, d = self.arrays()
        node_of_feature = np.asarray(node_of_feature)
        nodes = np.unique(node_of_feature)
        order = np.argsort(node_of_feature, kind="stable")
        start = np.concatenate([[0], np.cumsum([(node_of_feature == n).sum() for n in nodes])]).astype(np.int32)
        return views.key_frame_view(k, d, SF, SIGMA2, nodes.astype(np.uint32), start, order.astype(np.uint32), np.array(self.u_right, f32), np.asarray(has_map_point, np.uint8))


def same(got_n, got, exp_n, exp, what, names=None):
    """assert an assignment array and its match count, naming the cases (names[i]: the case that owns keypoint i) that differ"""
    got, exp = np.asarray(got), np.asarray(exp)
    bad = np.flatnonzero(got != exp)
    where = [names[i] for i in bad[:8]] if names is not None else bad[:8]
    assert len(bad) == 0 and got_n == exp_n, "%s: %s matches, expected %s; differs at %s: %s, expected %s" % (what, got_n, exp_n, where, got[bad[:8]], exp[bad[:8]])
