"""k_fast_cells keeps its survivor and corner lists in pixel (row-major) order and writes the NMS survivors in list order (csrc/k_fast.hip, phases A - C):
constructed cells in which that order can break, compared ORDER-SENSITIVELY with the oracle's candidates and, for the whole extraction, with the oracle and
the reference - on the emulator and on the device, at a batch of one image (k_fast_cells_blur) and of 33 (k_fast_cells).

The images are the smallest the library accepts: one level of 67 .. 101 pixels is ONE FAST cell (csrc/orbx_api.cpp: border 16, cells of >= 35 pixels), so the
cell, its dword alignment and its number of dword groups per row (ng) follow from the image size and are asserted, not searched for.  A pixel that differs from a
flat background by more than the threshold is a corner with score |difference| - 1 (its whole ring is an arc); the constructions are made of such dots."""
import math

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import _lib
from orb_slam3_detailed_comments_amd.extractor import ORBextractor

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
INI, MIN, BORDER, PITCH = 20, 7, 16, 48


def cells_of_level(w, h):
    """the FAST cell grid of a level (src/ORBextractor.cc:1069-1129 as csrc/orbx_api.cpp restates it): interior rectangles (x0, x1, y0, y1)"""
    bw, bh = w - 2 * BORDER, h - 2 * BORDER
    ncols, nrows = int(bw / 35.0), int(bh / 35.0)
    wcell, hcell = math.ceil(bw / ncols), math.ceil(bh / nrows)
    out = []
    for i in range(nrows):
        iy = BORDER + i * hcell
        if iy >= h - BORDER - 3:
            continue
        for j in range(ncols):
            ix = BORDER + j * wcell
            if ix >= w - BORDER - 6:
                continue
            out.append((ix + 3, min(ix + wcell + 6, w - BORDER) - 3, iy + 3, min(iy + hcell + 6, h - BORDER) - 3))
    return out


def cell_shape(x0, x1):
    """(xo, ng, pitch) of k_fast_cells for a cell with interior columns [x0, x1): tile column of the window's first pixel, dword groups of an interior row,
    LDS pitch (0 = the cell's own width: fast_cell<0>)"""
    gx0, gx1 = (x0 - 3) & ~3, (x1 + 6) & ~3
    xo = x0 - 3 - gx0
    g0 = (xo + 3) >> 2
    return xo, ((xo + 3 + (x1 - x0) - 1) >> 2) - g0 + 1, PITCH if gx1 - gx0 <= PITCH else 0


def corner_mask(img, t):
    """the segment test as defined: nine contiguous ring pixels all brighter or all darker than the centre by more than t"""
    a = img.astype(np.int16)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    m = np.zeros((h, w), bool)
    for sign in (1, -1):
        ring = np.stack([sign * (a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c) > t for dx, dy in RING])
        r2 = np.concatenate([ring, ring[:8]])
        for s in range(16):
            m[3:h - 3, 3:w - 3] |= np.logical_and.reduce(r2[s:s + 9])
    return m


def pair_entries(img, t):
    """list entries per pixel of an exact pair test at threshold t (0, 1, or 2 for both polarities): each of the four opposite ring pairs (0, 8) (2, 10)
    (4, 12) (6, 14) holds a pixel darker than the centre by more than t / brighter by more than t"""
    a = img.astype(np.int16)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    n = np.zeros((h, w), np.int32)
    for sign in (1, -1):
        ok = np.ones_like(c, bool)
        for k in (0, 2, 4, 6):
            (dx, dy), (ex, ey) = RING[k], RING[k + 8]
            ok &= (sign * (a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c) > t) | (sign * (a[3 + ey:h - 3 + ey, 3 + ex:w - 3 + ex] - c) > t)
        n[3:h - 3, 3:w - 3] += ok
    return n


def _same(a, b):
    return a[0] == b[0] and ol.kps_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def run(lib, img, B, nl=1, ini=INI, mn=MIN):
    """the image as the last of a batch of B (the others: its mirror image) against the oracle: FAST candidates of every level in order, then the whole extraction
    (tests/test_emu_parity.py).  Returns the oracle's level-0 candidates as (x, y, score) rows in image coordinates."""
    ex = ORBextractor(100, 1.2, nl, ini, mn, lib=lib)
    res = ex.extract_batch(np.stack([np.ascontiguousarray(img[:, ::-1])] * (B - 1) + [img]))
    o = ol.OracleExtractor(100, 1.2, nl, ini, mn, 0)
    exp = o.extract(img)
    for l in range(nl):
        assert np.array_equal(ex.debug_candidates(l, B - 1), o.level_candidates(l)), "FAST candidates level %d, batch of %d" % (l, B)
    assert _same(res[B - 1], exp), "extraction, batch of %d" % B
    if ol.reference() is not None:
        assert _same(res[B - 1], ol.ReferenceExtractor(100, 1.2, nl, ini, mn, 0).extract(img))
    ex.close()
    c = o.level_candidates(0).copy()
    c[:, :2] += BORDER
    return [tuple(int(v) for v in r) for r in c]


def one_cell(size, bg=100):
    """a flat square image of one level and one FAST cell, and the cell"""
    img = np.full((size, size), bg, np.uint8)
    cells = cells_of_level(size, size)
    assert len(cells) == 1
    return img, cells[0]


# ---- the constructions: name -> (image, levels, check(candidates of level 0)) ----

def case_empty_at_ini():
    """no corner at iniThFAST, three at minThFAST (difference 12): the cell takes the second run"""
    img, (x0, x1, y0, y1) = one_cell(67)
    dots = [(x0 + 4, y0 + 2, 112), (x0 + 13, y0 + 9, 88), (x0 + 22, y0 + 20, 113)]
    for x, y, v in dots:
        img[y, x] = v
    assert not corner_mask(img, INI).any() and corner_mask(img, MIN).sum() == 3

    def check(c):
        assert c == [(x, y, abs(v - 100) - 1) for x, y, v in dots]
    return img, 1, check


def case_no_corner():
    """no corner at either threshold (differences of 7 and less)"""
    img, (x0, x1, y0, y1) = one_cell(67)
    img[y0 + 5, x0 + 5] = 107
    img[y0 + 15, x0 + 20] = 93
    assert not corner_mask(img, MIN).any()

    def check(c):
        assert c == []
    return img, 1, check


def case_byte_positions():
    """one corner at each byte position of a dword, in the first and last interior column and row, in two adjacent lanes (dwords), in two adjacent rows"""
    img, (x0, x1, y0, y1) = one_cell(67)
    assert (x0, x1, y0, y1) == (19, 48, 19, 48) and cell_shape(x0, x1) == (0, 8, PITCH)
    dots = [(x0, y0, 150), (x1 - 1, y0, 151), (x0 + 9, y0, 152),                          # first row: first and last column
            (24, 24, 153), (29, 25, 154), (34, 26, 155), (39, 27, 156),                     # x mod 4 = 0, 1, 2, 3
            (23, 31, 157), (27, 31, 158),                                                  # the last byte of a dword and the first of the next: adjacent lanes
            (36, 31, 159), (41, 31, 160),                                                   # dwords 9 and 10
            (24, 36, 161), (29, 37, 162),                                                   # adjacent rows
            (x0, 42, 40), (x1 - 1, 43, 41),                                                 # dark ones in the edge columns
            (x0, y1 - 1, 163), (x0 + 14, y1 - 1, 30), (x1 - 1, y1 - 1, 164)]                # last row
    for x, y, v in dots:
        img[y, x] = v
    assert {x % 4 for x, y, v in dots[3:7]} == {0, 1, 2, 3} and dots[7][0] >> 2 == (dots[8][0] >> 2) - 1 and dots[9][0] >> 2 == (dots[10][0] >> 2) - 1
    assert corner_mask(img, INI).sum() == len(dots)

    def check(c):
        assert c == sorted(((x, y, abs(v - 100) - 1) for x, y, v in dots), key=lambda r: (r[1], r[0]))
    return img, 1, check


def case_equal_scores():
    """two 8-connected corners with the same score (side by side, and diagonal): the strict maximum keeps neither; a single one beside them is kept"""
    img, (x0, x1, y0, y1) = one_cell(67)
    for x, y in ((24, 24), (25, 24), (33, 25), (34, 26), (42, 24), (26, 35), (27, 35), (28, 35)):
        img[y, x] = 170
    img[40, 30] = 171; img[40, 31] = 170
    assert corner_mask(img, INI).sum() == 10

    def check(c):
        assert c == [(42, 24, 69), (30, 40, 70)]
    return img, 1, check


def case_descending_scores():
    """a run of corners with descending scores in one dword, and an ascending one: the first / the last alone is a strict maximum"""
    img, (x0, x1, y0, y1) = one_cell(67)
    for j in range(4):
        img[24, 24 + j] = 180 - j
        img[32, 28 + j] = 150 + j
        img[38 + j, 36] = 190 - j                   # and down a column
    assert corner_mask(img, INI).sum() == 12

    def check(c):
        assert c == [(24, 24, 79), (31, 32, 52), (36, 38, 89)]
    return img, 1, check


def _dual(img, x, y, arc=None, bright=150, dark=106):
    """a pixel at the background value (128) that passes the quick test for both polarities: of every opposite ring pair one pixel is brighter and one darker
    by 22.  arc: first ring index of nine contiguous dark ring pixels (the pixel is then a dark corner as well, score 21)"""
    assert img[y, x] == 128
    for k in range(16):
        dx, dy = RING[k]
        if arc is None:
            v = (bright if k < 8 else dark) if k % 2 == 0 else None
        else:
            in_arc = (k - arc) % 16 < 9
            v = dark if in_arc else bright if k % 2 == 0 else None
        if v is not None:
            img[y + dy, x + dx] = v


def case_both_polarities():
    """a pixel listed twice (dark and bright candidate) that is no corner, left of, right of, above and below a true corner in the same dword column - and one that
    IS a (dark) corner, with a second corner two bytes further in its dword: its second entry has to stay directly behind its first"""
    img, (x0, x1, y0, y1) = one_cell(101, bg=128)
    assert cell_shape(x0, x1)[2] == 0
    places = [((28, 28), (29, 28)), ((45, 28), (44, 28)), ((60, 29), (60, 28)), ((28, 44), (28, 45))]      # (dual pixel, corner)
    for (dx, dy), (cx, cy) in places:
        _dual(img, dx, dy)
        img[cy, cx] = 255
        assert dx >> 2 == cx >> 2
    _dual(img, 44, 60, arc=9)                       # dark arc 9 .. 1: ring pixels 3, 4, 5 (right of it) stay free
    img[60, 46] = 255
    assert pair_entries(img, INI)[60, 44] == 2 and all(pair_entries(img, INI)[y, x] == 2 for (x, y), _ in places)
    cm = corner_mask(img, INI)
    assert cm[60, 44] and cm[60, 46] and not any(cm[y, x] for (x, y), _ in places) and all(cm[y, x] for _, (x, y) in places)

    def check(c):
        pts = {(x, y): s for x, y, s in c}
        for (dx, dy), (cx, cy) in places:
            assert (dx, dy) not in pts and pts.get((cx, cy)) == 126, (dx, dy, pts.get((cx, cy)))
        assert pts.get((44, 60)) == 21 and pts.get((46, 60)) == 126
    return img, 1, check


def _dense(img, x0, x1, y0, y1, pairs=True):
    """dots two pixels apart, columns alternately high (200) and low (100) on 0: a high dot sees the four low dots on its ring and the background, all darker: a corner of
    score 99; a low dot has the four high ones on its ring, 90 degrees apart: no corner.  Every fifth high dot of the first rows gets an equal right neighbour."""
    n = 0
    for y in range(y0 + 1, y1 - 1, 2):
        for i, x in enumerate(range(x0 + 1, x1 - 1, 2)):
            img[y, x] = 200 if i % 2 == 0 else 100
            n += i % 2 == 0
            if pairs and i % 2 == 0 and n % 5 == 0 and y < y0 + 12 and x + 1 < x1 - 1:
                img[y, x + 1] = 200


def case_dense():
    """more than 128 corners in a cell of the common pitch: phase C takes four trips and `base` carries; corners 63 | 64, 127 | 128 and 191 | 192 of the list (the last lane of a trip and
    the first of the next) survive"""
    img, (x0, x1, y0, y1) = one_cell(77, bg=0)
    assert cell_shape(x0, x1) == (0, 11, PITCH)
    _dense(img, x0, x1, y0, y1)
    cm = corner_mask(img, INI)[y0:y1, x0:x1]
    ys, xs = np.nonzero(cm)                         # row-major: the order of the corner list
    assert 192 < len(ys) <= 256

    def check(c):
        assert 128 < len(c) < len(ys)               # some corners are suppressed: rank != lane
        pts = {(x, y) for x, y, s in c}
        for i in (63, 64, 127, 128, 191, 192):
            assert (int(xs[i]) + x0, int(ys[i]) + y0) in pts, i
    return img, 1, check


def case_wide_cell():
    """a level whose single cell is wider than the common pitch (fast_cell<0>: the division by the cell's own pitch), more than 256 corners, with a second level"""
    img, (x0, x1, y0, y1) = one_cell(101, bg=0)
    assert cell_shape(x0, x1) == (0, 17, 0)
    _dense(img, x0, x1, y0, y1)

    def check(c):
        assert len(c) > 256
    return img, 2, check


def case_alignment(size, want):
    """cells of 30 interior columns: at tile column 0 their rows take nine dwords, at tile column 1 eight"""
    def build():
        img = np.full((67, size), 100, np.uint8)
        cells = cells_of_level(size, 67)
        x0, x1, y0, y1 = cells[-1]
        assert x1 - x0 == 30 and cell_shape(x0, x1) == want, cell_shape(x0, x1)
        dots = [(x0 + (5 * i) % 30, y0 + 1 + 3 * i, 140 + i) for i in range(9)] + [(x0, y1 - 1, 60), (x1 - 1, y1 - 1, 61)]
        for x, y, v in dots:
            img[y, x] = v
        assert corner_mask(img, INI)[y0:y1, x0:x1].sum() == len(dots)

        def check(c):
            mine = [r for r in c if r[0] >= x0]
            assert mine == sorted(((x, y, abs(v - 100) - 1) for x, y, v in dots), key=lambda r: (r[1], r[0]))
        return img, 1, check
    return build


CASES = {
    "empty_at_ini": case_empty_at_ini, "no_corner": case_no_corner, "byte_positions": case_byte_positions, "equal_scores": case_equal_scores,
    "descending_scores": case_descending_scores, "both_polarities": case_both_polarities, "dense": case_dense, "wide_cell": case_wide_cell,
    "ng9_tile_column_0": case_alignment(68, (0, 9, PITCH)), "ng8_tile_column_1": case_alignment(105, (1, 8, PITCH)),
}


def _case(lib, name, B):
    img, nl, check = CASES[name]()
    check(run(lib, img, B, nl))


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ordered_lists_emulated(emu_lib, name, B):
    _case(emu_lib, name, B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ordered_lists_gpu(hip_lib, name, B):
    _case(hip_lib, name, B)


# ---- a flush in the middle of a cell: emulator builds with a small list ----

def case_flush(cap):
    """One cell of the common pitch whose quick-test survivors do not fit a list of 200 entries while its corners do.  Filler: dots (160 on 128) on every third row, two
    columns apart: a dot has equal dots on its ring at the odd positions 1, 7, 9 and 15 only, which the pair test does not read and which cut every arc down to five
    pixels - listed, never a corner.  True corners: filler dots raised above their neighbours, in the first trip's rows, in the middle and in the last trip's rows; a pixel
    listed for both polarities in the first and in the last trip: whichever trip the list fills up at, corners and a double entry lie on both sides of the flush."""
    size = 77
    img, (x0, x1, y0, y1) = one_cell(size, bg=128)
    xo, ng, pitch = cell_shape(x0, x1)
    assert pitch == PITCH
    rpt, ih = 64 // ng, y1 - y0                     # rows per trip of phase A
    last = ih - (ih % rpt or rpt)                   # first row of the last trip
    for y in range(0, size, 3):
        img[y, (y // 3) % 2::2] = 160
    rows = [y for y in range(y0, y1) if y % 3 == 0]
    first_row, mid_row, last_row = rows[0], rows[len(rows) // 2], rows[-1]
    assert first_row - y0 < rpt and last_row - y0 >= last
    for y in (first_row, mid_row, last_row):
        xs = [x for x in range(x0 + 1, x1 - 12) if img[y, x] == 160][::3]
        for i, x in enumerate(xs):
            img[y, x] = 230 + i
    duals = [(x1 - 5, first_row + 1), (x1 - 5, last_row - 1)]
    for x, y in duals:
        img[y - 3:y + 4, x - 3:x + 4] = 128
        _dual(img, x, y)
    cm = corner_mask(img, INI)[y0:y1, x0:x1]
    ent = pair_entries(img, INI)[y0:y1, x0:x1]              # entries of an exact pair test: every one of them is in the kernel's list
    loose = pair_entries(img, INI - 3)[y0:y1, x0:x1]        # the 7-bit test lets through nothing that differs by less than t - 1
    assert all(ent[y - y0, x - x0] == 2 and not cm[y - y0, x - x0] for x, y in duals)
    trips = [int(loose[r:r + rpt].sum()) for r in range(0, ih, rpt)]
    assert cm[:rpt].sum() >= 4 and cm[last:].sum() >= 4, "corners in the first and in the last trip"
    return img, cm, ent, trips


@pytest.mark.parametrize("cap", [200, 600])
def test_mid_cell_flush_keeps_the_order(tmp_path, cap):
    from test_emu_variants import build_emu_variant
    so = str(tmp_path / "liborbx_emu_cap.so")
    build_emu_variant(so, ["-DORBX_FAST_LIST_CAP=%d" % cap])
    lib = _lib.OrbxLib(so)
    img, cm, ent, trips = case_flush(cap)
    if cap == 200:
        # the list overflows in the middle of the cell (more entries than it holds before the last trip), yet keeps its corners: they and a whole trip always fit
        assert ent.sum() - trips[-1] > cap and cm.sum() + max(trips) <= cap and trips[0] <= cap
    else:
        assert sum(trips) <= cap                    # the same cell without a flush
    for B in (1, 33):
        c = run(lib, img, B)
        assert len(c) >= 20
    # the dense cell: more corners than 200 entries hold (the list is given up: C', D'), fewer than 600
    img, nl, check = case_dense()
    check(run(lib, img, 1, nl))
    # low-amplitude noise (tests/test_emu_variants.py::test_fast_list_flush_path): next to no corner at iniThFAST, a crowd at minThFAST - flushes and the list-free path
    # in the second run, over eight levels
    noise = (60 + np.random.default_rng(5).integers(0, 26, (240, 376))).astype(np.uint8)
    ex = ORBextractor(500, 1.2, 8, INI, MIN, lib=lib)
    got = ex(noise)
    o = ol.OracleExtractor(500)
    exp = o.extract(noise)
    for l in range(8):
        assert np.array_equal(ex.debug_candidates(l), o.level_candidates(l)), "FAST candidates level %d" % l
    assert _same(got, exp)
