"""Constructed inputs that sit ON the decisions of the extraction kernels, where the parity tests on textures and noise reach them by chance only
(tools/emu_mutants.py, ids from 405; profiles/emu_mutants_extract/README.md).  Every case compares the library stage by stage and bit for bit with the
oracle and, where it is built, with the reference's own ORBextractor - never with the library itself - and runs on the emulator and on the device:
byte_ballot<J>'s SDWA compares and the v_mbcnt ranks of k_fast_cells exist on the device alone, so the FAST cases put their pixels at every byte
position of a dword (x mod 4), for both polarities."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import synth
from orb_slam3_detailed_comments_amd.extractor import ORBextractor

# FAST-9/16 ring, OpenCV's order
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
W, H = 376, 240


def _stagewise(lib, img, nf, nl, ini, mn, lap=(0, 0), setup=None):
    """the library against the oracle at every stage (tests/test_emu_parity.py::test_extractor_stagewise_and_final) and the reference at the end; returns the
    oracle.  setup(ex): test switches of the extractor that change the path and not the result"""
    ex = ORBextractor(nf, 1.2, nl, ini, mn, lib=lib)
    if setup is not None:
        setup(ex)
    got = ex(img, None, lap)
    o = ol.OracleExtractor(nf, 1.2, nl, ini, mn, 0)
    exp = o.extract(img, lap)
    for l in range(nl):
        assert np.array_equal(ex.pyramid_level(l), o.level_image(l)), "pyramid level %d" % l
        assert np.array_equal(ex.pyramid_level(l, blurred=True), o.level_image(l, blurred=True)), "blur level %d" % l
        assert np.array_equal(ex.debug_candidates(l), o.level_candidates(l)), "FAST candidates level %d" % l
        k2 = o.level_keypoints(l)
        k2a = np.stack([k2["x"] - 16, k2["y"] - 16, k2["response"]], 1).astype(np.int32) if len(k2) else np.zeros((0, 3), np.int32)
        assert np.array_equal(ex.debug_level_keys(l), k2a), "quadtree level %d" % l
    same = lambda a, b: a[0] == b[0] and ol.kps_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert same(got, exp)
    if ol.reference() is not None:
        assert same(got, ol.ReferenceExtractor(nf, 1.2, nl, ini, mn, 0).extract(img, lap))
    ex.close()
    return o


def _arc_corner_image(bg, ini, mn):
    """Isolated pixels on a flat background whose nine-arc differs from them by exactly t - 1, t, t + 1 and t + 2: in the left part of the image with t = ini,
    in the right part - whose cells hold nothing at ini and take the second FAST run - with t = mn.  The arc's rotation, its polarity and the pixel's x mod 4
    vary independently.  Returns the image and one (x, y, polarity, d - t) per pixel."""
    img = np.full((H, W), bg, np.uint8)
    made = []
    i = 0
    for y in range(23, H - 23, 9):
        for x in range(23, W - 23, 9):
            t = ini if x < W // 2 - 24 else mn if x > W // 2 + 24 else None
            if t is None:
                continue
            i += 1
            off = (-1, 0, 1, 2)[(i // 4 + i) % 4]
            dark = (i // 16) % 2 == 0
            val = bg - (t + off) if dark else bg + (t + off)
            if val < 0 or val > 255:
                continue
            rot = (i * 7 + i // 32) % 16
            for k in range(9):
                dx, dy = RING[(rot + k) % 16]
                img[y + dy, x + dx] = val
            made.append((x, y, dark, off))
    return img, made


# (background, iniThFAST, minThFAST): even and odd thresholds; backgrounds at which v - t reaches 0 and v + t reaches 255 and 256, where the quick test's
# byte arithmetic saturates (max(V - td + 1, 0), min(V + td, 128))
ARC_CASES = [(128, 20, 7), (128, 21, 8), (21, 20, 7), (22, 21, 8), (234, 20, 7), (235, 20, 7), (233, 21, 8), (8, 20, 7), (247, 20, 7)]


def _fast_threshold_boundaries_case(lib, bg, ini, mn):
    img, made = _arc_corner_image(bg, ini, mn)
    o = _stagewise(lib, img, 500, 8, ini, mn)
    # the construction sits where it says: the oracle takes a pixel whose arc differs by more than t, with score d - 1, and, at mn, none whose arc differs by
    # t or less (in the left part a cell without a corner at ini runs again at mn and then takes such a pixel, with its score d - 1)
    cand = {(int(x) + 16, int(y) + 16): int(s) for x, y, s in o.level_candidates(0)}
    seen = set()
    for x, y, dark, off in made:
        t = ini if x < W // 2 else mn
        if off > 0:
            assert cand.get((x, y)) == t + off - 1, (x, y, dark, off, cand.get((x, y)))
            seen.add((x % 4, dark, off, t))
        elif t == mn:
            assert (x, y) not in cand, (x, y, dark, off)
        else:
            assert cand.get((x, y)) in (None, t + off - 1), (x, y, dark, off, cand.get((x, y)))
    if bg == 128:
        assert len(seen) == 4 * 2 * 2 * 2, sorted(seen)             # every byte position x polarity x {t + 1, t + 2} x {ini, mn}
        at_ini = [(x, y) for x, y, dark, off in made if x < W // 2 and off <= 0]
        assert sum(p not in cand for p in at_ini) > len(at_ini) // 2    # most cells of the left part have a corner at ini: there d == t is refused at ini
    else:
        assert len(seen) >= 4 * 2 * 2, sorted(seen)                 # the polarity that fits the byte range, at least


@pytest.mark.parametrize("bg,ini,mn", ARC_CASES)
def test_fast_threshold_boundaries_emulated(emu_lib, bg, ini, mn):
    _fast_threshold_boundaries_case(emu_lib, bg, ini, mn)


@pytest.mark.gpu
@pytest.mark.parametrize("bg,ini,mn", ARC_CASES)
def test_fast_threshold_boundaries_gpu(hip_lib, bg, ini, mn):
    _fast_threshold_boundaries_case(hip_lib, bg, ini, mn)


def _borrow_image(ini):
    """The quick test of k_fast_cells compares four pixels of a dword at once, (ring | 0x80) - bound per byte.  The bright bound min(V + td, 128) is saturated so
    that no byte borrows from its neighbour; without the saturation a pixel A near 255 with a DARK ring pixel borrows from the byte of the pixel B right of it,
    and B's ring pixel at the same ring position, if it sits exactly on B's 7-bit bound (R == V + td), stops counting as bright.  B is a bright corner whose
    pair (4, 12) rests on that one ring pixel: arc = ring 0 .. 8, so ring 12 is background.  Once per byte position of A that has a right neighbour in its
    dword (x mod 4 = 0, 1, 2), and per parity of B's value."""
    img = np.full((H, W), 100, np.uint8)
    td = (ini + 1) >> 1
    made = []
    n = 0
    for y in range(30, H - 30, 12):
        for x in range(32, W - 32, 16):
            n += 1
            xa = x + (n % 3) - (x % 4)                          # A at x mod 4 = n mod 3
            vb = 100 + (n // 3) % 2
            img[y - 4:y + 5, xa - 4:xa + 7] = vb                # B's surroundings at B's own value
            r = 2 * ((vb >> 1) + td) + ((n // 6) % 2)           # ring value with R == V + td: the lowest the quick test lets through, even and odd
            if r - vb <= ini:
                r += 2
            for k in range(9):
                dx, dy = RING[k]
                img[y + dy, xa + 1 + dx] = r
            img[y, xa] = 255                                    # A, left of B
            img[y, xa + 3] = 0                                  # A's ring pixel 4 (B's ring pixel 4 is the one right of it)
            # A itself must be no corner, or its score would suppress B: the pixels of A's ring that are not on B's ring (all but 0, 1, 7, 8) and not
            # the dark one are as bright as A, which leaves A two adjacent darker ring pixels at the most
            for k in (2, 3, 5, 6, 9, 10, 11, 12, 13, 14, 15):
                dx, dy = RING[k]
                img[y + dy, xa + dx] = 255
            made.append((xa + 1, y, r - vb - 1))
    return img, made


def _quick_test_saturation_case(lib, ini):
    img, made = _borrow_image(ini)
    o = _stagewise(lib, img, 500, 8, ini, 7)
    cand = {(int(x) + 16, int(y) + 16): int(s) for x, y, s in o.level_candidates(0)}
    hit = [(x, y) for x, y, s in made if cand.get((x, y)) == s]
    assert len(hit) == len(made) and {(x - 1) % 4 for x, _ in hit} == {0, 1, 2}, (len(hit), len(made))


@pytest.mark.parametrize("ini", [20, 21])
def test_quick_test_saturation_emulated(emu_lib, ini):
    _quick_test_saturation_case(emu_lib, ini)


@pytest.mark.gpu
@pytest.mark.parametrize("ini", [20, 21])
def test_quick_test_saturation_gpu(hip_lib, ini):
    _quick_test_saturation_case(hip_lib, ini)


TABLE_CASES = [(1200, 1.2, 8), (500, 1.2, 8), (1000, 1.2, 8), (250, 1.5, 4), (800, 1.2, 11), (37, 1.3, 3)]


def _level_tables_case(lib):
    """the constructor's tables (scale factors, their inverses, sigma squares, their inverses, the feature quota per level, umax) against the oracle's and
    the reference's own, bit for bit: no kernel of the extractor reads the sigma tables; orbm_stereo_match copies sigma2 into the matcher's parameters and the callers read the others"""
    for nf, sf, nl in TABLE_CASES:
        ex = ORBextractor(nf, sf, nl, 20, 7, lib=lib)
        f, q, um = ex._tables()
        oq, oum, of = ol.OracleExtractor(nf, sf, nl, 20, 7, 0).tables()
        assert np.array_equal(q, oq) and np.array_equal(um, oum), (nf, sf, nl)
        for a, b in zip(f, of):
            assert a.tobytes() == b.tobytes(), (nf, sf, nl)
        if ol.reference() is not None:
            rq, rum, _, rf = ol.ReferenceExtractor(nf, sf, nl, 20, 7, 0).tables()
            assert np.array_equal(q, rq) and np.array_equal(um, rum), (nf, sf, nl)
            for a, b in zip(f, rf):
                assert a.tobytes() == b.tobytes(), (nf, sf, nl)
        ex.close()


def test_level_tables_emulated(emu_lib):
    _level_tables_case(emu_lib)


@pytest.mark.gpu
def test_level_tables_gpu(hip_lib):
    _level_tables_case(hip_lib)


def _equal_responses_case(lib, nf):
    """The quadtree's result is, per final node, the largest response and among equal ones the earliest in vKeys order (the reference's loop keeps the first).
    The arc pixels above have four responses in all, so with a small feature budget every final node holds several keys with the same, largest response.  A
    tree that sorted its keys holds them in bucket order, which is not vKeys order: both forms of the selection are run - the never-sorted one (bucket words)
    and, with the keys sorted right after the gather, the one that walks the node's span with several lanes and several keys per lane.
    nf = 1000: the other end, the smallest image with a texture and a budget so large that most final nodes hold two or three keys.  It is here because it is
    the one small input found on which "the first in BUFFER order of equal responses" differs from the reference's answer (a sorted span, level 2): on the arc
    image the two orders agree among the ties of every lane at every budget tried (10 .. 3000)."""
    img = synth.corner_field(239, 239, seed=4, nrect=600) if nf == 1000 else _arc_corner_image(128, 20, 7)[0]
    for eager in (False, True):
        o = _stagewise(lib, img, nf, 8, 20, 7, setup=lambda ex: ex.debug_quadtree_eager(eager))
        k0 = o.level_keypoints(0)
        cand = o.level_candidates(0)
        if nf < 1000:
            assert len(cand) > 4 * len(k0) > 0 and len(set(k0["response"].tolist())) <= 4    # several candidates per node, ties at the top


@pytest.mark.parametrize("nf", [40, 150, 1000])
def test_equal_responses_in_a_final_node_emulated(emu_lib, nf):
    _equal_responses_case(emu_lib, nf)


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [40, 150, 1000])
def test_equal_responses_in_a_final_node_gpu(hip_lib, nf):
    _equal_responses_case(hip_lib, nf)


def _cell_intervals(size):
    """interiors [a, b) of the FAST cells along one axis of level 0, in level coordinates (ComputeKeyPointsOctTree :1069-1129, csrc/orbx_api.cpp configure):
    35-pixel cells between the 16-pixel borders, a window of cell + 6, the interior 3 inside it.  (The reference skips a row that begins within 3 of the
    border and a column within 6: neither happens at these sizes.)"""
    lo, hi = 16, size - 16
    n = (hi - lo) // 35
    cell = -(-(hi - lo) // n)
    out = []
    for k in range(n):
        ini = lo + k * cell
        assert ini < hi - 6
        out.append((ini + 3, min(ini + cell + 6, hi) - 3))
    return out


def _in_cell_order(cand, cols, rows):
    """candidates (level coordinates) come cell by cell, row-major, and by y, then x inside a cell: true of the oracle's list only if the intervals are its cells"""
    idx = lambda v, iv: next(k for k, (a, b) in enumerate(iv) if a <= v < b)
    keys = [(idx(y, rows), idx(x, cols), y, x) for x, y in cand]
    return keys == sorted(keys) and len(set(keys)) == len(keys)


EDGE_KINDS = ["left", "right", "top", "bottom", "top_left", "bottom_right", "top_right", "bottom_left"]     # kind k ^ 1 is the opposite one


def _edge_pixel(kind, x0, x1, y0, y1):
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    return {"left": (x0, ym), "right": (x1 - 1, ym), "top": (xm, y0), "bottom": (xm, y1 - 1), "top_left": (x0, y0), "bottom_right": (x1 - 1, y1 - 1),
            "top_right": (x1 - 1, y0), "bottom_left": (x0, y1 - 1)}[kind]


def _cell_edge_image(t):
    """Arc pixels ON the first and last row and column of FAST cells, where the validity mask of the quick test's dwords (VM, xbase + j >= 0) and the zero frame
    of the score tile act: per cell one pixel whose arc differs by t + 1 on one edge or corner and one with t on the opposite one, and a pixel with t + 2 in
    the middle, which fixes the cell's run: with t = iniThFAST the first, with t = minThFAST (nothing in the image above it) the second."""
    img = np.full((H, W), 128, np.uint8)
    cols, rows = _cell_intervals(W), _cell_intervals(H)
    made = []
    n = {t: 0}
    for y0, y1 in rows:
        for j, (x0, x1) in enumerate(cols):
            k, dark = n[t] % 8, (n[t] // 8) % 2 == 0
            want = [(EDGE_KINDS[k], 1), (EDGE_KINDS[k ^ 1], 0), (None, 2)]
            at = [_edge_pixel(kind, x0, x1, y0, y1) if kind else ((x0 + x1) // 2, (y0 + y1) // 2) for kind, _ in want]
            # (a neighbouring cell's pixel on the other side of a shared edge would lie inside this one's ring: such a cell only gets its middle pixel)
            if any(max(abs(x - q[0]), abs(y - q[1])) < 10 for x, y in at[:2] for q in made):
                want, at = want[2:], at[2:]
            else:
                n[t] += 1
            for (kind, off), (x, y) in zip(want, at):
                rot = (5 * n[t] + 3 * off) % 16
                for a in range(9):
                    dx, dy = RING[(rot + a) % 16]
                    img[y + dy, x + dx] = 128 - (t + off) if dark else 128 + (t + off)
                made.append((x, y, kind, dark, off, t))
    return img, made, cols, rows


def _fast_cell_edges_case(lib, ini, mn, second_run):
    img, made, cols, rows = _cell_edge_image(mn if second_run else ini)
    o = _stagewise(lib, img, 500, 8, ini, mn)
    c0 = o.level_candidates(0)
    assert _in_cell_order([(int(x) + 16, int(y) + 16) for x, y, _ in c0], cols, rows)       # the intervals above are the oracle's cells
    cand = {(int(x) + 16, int(y) + 16): int(s) for x, y, s in c0}
    seen = set()
    for x, y, kind, dark, off, t in made:
        if off == 0:
            assert (x, y) not in cand, (x, y, kind, dark, t)
        else:
            assert cand.get((x, y)) == t + off - 1, (x, y, kind, dark, off, t, cand.get((x, y)))
            if kind:
                seen.add((kind, dark, t))
    assert len(seen) == 8 * 2, sorted(seen)                     # every edge and corner x polarity
    assert {x % 4 for x, _, kind, _, off, _ in made if kind and off == 1} == {0, 1, 2, 3}


EDGE_CASES = [(20, 7, False), (21, 8, False), (20, 7, True), (21, 8, True)]


@pytest.mark.parametrize("ini,mn,second_run", EDGE_CASES)
def test_fast_cell_edges_emulated(emu_lib, ini, mn, second_run):
    _fast_cell_edges_case(emu_lib, ini, mn, second_run)


@pytest.mark.gpu
@pytest.mark.parametrize("ini,mn,second_run", EDGE_CASES)
def test_fast_cell_edges_gpu(hip_lib, ini, mn, second_run):
    _fast_cell_edges_case(hip_lib, ini, mn, second_run)


def _full_ballot_image(lo, hi):
    """A two-level pattern of period 4 x 2 (rows 0 0 1 1 / 1 1 0 0) in which EVERY pixel has, in each of the four opposite ring pairs (0, 8), (2, 10), (4, 12),
    (6, 14), a pixel of the other level: every pixel passes the quick test, for the polarity of its level, so every lane of a trip of k_fast_cells lists its
    pixels and each of the four byte ballots holds more than 32 hits - the high half of the ballot counts in the v_mbcnt ranks."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((xx >> 1) + yy) % 2 == 0, lo, hi).astype(np.uint8)


def _full_ballots_case(lib, ini):
    img = _full_ballot_image(60, 180)
    v = img.astype(np.int32)
    for a, b in ((0, 8), (2, 10), (4, 12), (6, 14)):             # the pair test, restated: |ring - centre| > ini for one pixel of each pair, everywhere
        d = [np.abs(np.roll(v, (-RING[k][1], -RING[k][0]), (0, 1)) - v)[3:-3, 3:-3] for k in (a, b)]
        assert (np.maximum(d[0], d[1]) > ini).all()
    for x0, x1 in _cell_intervals(W):                              # lanes of a trip: whole rows of dword groups, 64 // groups rows (k_fast_cells, phase A)
        groups = ((x1 + 2) >> 2) - ((x0) >> 2) + 1
        assert (64 // groups) * (groups - 2) > 32, (x0, x1)        # (the first and last group of a row may hold invalid bytes)
    _stagewise(lib, img, 500, 8, ini, 7)


@pytest.mark.parametrize("ini", [20, 1])
def test_fast_full_ballots_emulated(emu_lib, ini):
    _full_ballots_case(emu_lib, ini)


@pytest.mark.gpu
@pytest.mark.parametrize("ini", [20, 1])
def test_fast_full_ballots_gpu(hip_lib, ini):
    _full_ballots_case(hip_lib, ini)
