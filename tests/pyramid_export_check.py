"""Shared checks of the bordered pyramid export (orbx_set_pyramid_export / orbx_pyramid_exported, ORBextractor.pyramid_export) for the
emulator and GPU tests: every exported frame against a numpy restatement of cv::copyMakeBorder(BORDER_REFLECT_101 + BORDER_ISOLATED) applied
to the level planes that orbx_pyramid_level returns."""
import numpy as np


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), repeated while p is out of range (edge >= n); n == 1 gives 0."""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def framed(plane, edge):
    h, w = plane.shape
    ys = reflect101(np.arange(-edge, h + edge), h)
    xs = reflect101(np.arange(-edge, w + edge), w)
    return plane[np.ix_(ys, xs)]


def expected_frames(ex, B, edge):
    """[image][level] framed planes restated from the device pyramid of the last extraction."""
    return [[framed(ex.pyramid_level(l, image_index=b), edge) for l in range(ex.nlevels)] for b in range(B)]


def check_export(ex, B, edge):
    """The exported frames of every image of the last batch equal the restatement; returns (views, expected) for ring checks."""
    exp = expected_frames(ex, B, edge)
    views = [ex.exported_pyramid(b) for b in range(B)]
    for b in range(B):
        for l in range(ex.nlevels):
            v = views[b][l]
            assert v.shape == exp[b][l].shape, (b, l, v.shape, exp[b][l].shape)
            assert not v.flags.writeable
            assert np.array_equal(v, exp[b][l]), "image %d level %d: exported frame differs" % (b, l)
    return views, exp


def views_intact(views, exp):
    return all(np.array_equal(v, e) for vb, eb in zip(views, exp) for v, e in zip(vb, eb))


def ring_check(ex, images_seq, edge, depth, B):
    """Extractions k = 0, 1, ... on a sequence of batches: after each, the exports of the depth - 1 previous extractions are still intact
    in the views handed out for them."""
    held = []
    for imgs in images_seq:
        ex.extract_batch(imgs)
        held.append(check_export(ex, B, edge))
        for age, (v, e) in enumerate(reversed(held[:-1][-(depth - 1):] if depth > 1 else [])):
            assert views_intact(v, e), "export of %d extraction(s) ago was overwritten (depth %d)" % (age + 1, depth)
    return held


def live(lib):
    a = np.zeros(4, np.int64)
    lib.check(lib.L.orbx_debug_live_resources(a.ctypes.data))
    return a.copy()
