"""The fisheye 2-NN kernels (csrc/k_match.hip: k_knn2_mfma on the matrix cores, k_knn2 one wave per query, orbx_debug_stereo_flags 0 and 8) on descriptor
sets built for the places where they decide, injected into a resident extraction (tests/resident_inject.py).  Natural features reach the common paths; they
do not land on a ratio of exactly 0.7, on equal keys in chosen lanes, tiles and waves, on distances 0 and 256 or on set sizes either side of a tile boundary.

Expected values: resident_inject.knn2_expected - all-pairs popcount, stable argsort, -1 where a neighbour does not exist, the ratio in double (the reference
compares `DMatch::distance`, a float, with `0.7 *` the other one: a double product, src/Frame.cc:1556).

Every case is a (query set, train set) pair of its own.  Leaks: every descriptor row of the two frames that lies OUTSIDE [q0, q0 + nQ) / [t0, t0 + nT) - rows past n[b]
included - is a copy of one of the pair's queries unless the case puts something more specific there, so that a read outside the sets shows as a neighbour at
distance 0; output rows nQ..cap must be -1 / 0.

The accumulator of v_mfma_i32_32x32x32_i8 holds, in register i of lane l, train row (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the tile: rows r and r + 1 (r & 3 < 3) sit in
one lane, r and r + 4 (r & 4 == 0) in the two lanes of a query; wave w of the workgroup takes tiles w, w + 4, w + 8 ..."""
import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import matcher as M
from resident_inject import ResidentBatch, knn2_expected, at_distance

PAIRS = 16                                  # (query set, train set) pairs per call: frames [0, PAIRS) are the left, [PAIRS, 2 PAIRS) the right ones
KEYS = ("idx0", "dist0", "idx1", "dist1", "ratio_ok")
_BATCH = {}


def _batch(lib):
    """one resident extraction per library, shared by every test of this module (the tests overwrite all they read)"""
    if id(lib) not in _BATCH:
        _BATCH[id(lib)] = ResidentBatch(lib, 2 * PAIRS)
        assert _BATCH[id(lib)].cap >= 45 + 544 + 1
    return _BATCH[id(lib)]


def _case(q, t, q0=0, t0=0, before=None, after=None):
    """before / after: train-side rows placed just in front of t0 / just behind t0 + nT (outside the set)"""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    c = dict(q=q, t=t, q0=q0, t0=t0, before=before, after=after, exp=knn2_expected(q, t))
    for a in c["exp"].values():
        a.setflags(write=False)
    return c


def _run(lib, cases, flag_list=(0, 8)):
    """every case through both kernels, PAIRS at a time; returns the outputs of the last kernel per case (for assertions about the construction itself
    use case["exp"]: the comparison with it is made here)"""
    rb = _batch(lib)
    cap = rb.cap
    filler = _case(np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8))
    try:
        for base in range(0, len(cases), PAIRS):
            chunk = cases[base:base + PAIRS]
            chunk = chunk + [filler] * (PAIRS - len(chunk))
            for p, c in enumerate(chunk):
                nQ, nT, q0, t0 = len(c["q"]), len(c["t"]), c["q0"], c["t0"]
                assert q0 + nQ <= cap and t0 + nT <= cap
                copies = c["q"][np.arange(cap) % nQ]                 # the leak bait
                rb.desc[p] = copies; rb.desc[p, q0:q0 + nQ] = c["q"]
                rb.desc[PAIRS + p] = copies; rb.desc[PAIRS + p, t0:t0 + nT] = c["t"]
                if c["before"] is not None:
                    rb.desc[PAIRS + p, t0 - len(c["before"]):t0] = c["before"]
                if c["after"] is not None:
                    rb.desc[PAIRS + p, t0 + nT:t0 + nT + len(c["after"])] = c["after"]
                rb.n[p] = q0 + nQ; rb.mono[p] = q0; rb.n[PAIRS + p] = t0 + nT; rb.mono[PAIRS + p] = t0
            rb.put_descriptors(); rb.put_counts()
            for flags in flag_list:
                rb.ex.debug_stereo_flags(flags)
                out = M.StereoFishEyeKnn(rb.ex, rb.ex, 0, PAIRS, PAIRS)
                for p, c in enumerate(chunk):
                    nQ = len(c["q"])
                    for key in KEYS:
                        got, exp = out[key][p, :nQ], c["exp"][key]
                        assert np.array_equal(got, exp), "case %d (nQ %d, nT %d, q0 %d, t0 %d), flags %d, %s: query %d gives %d, expected %d" % (
                            base + p, nQ, len(c["t"]), c["q0"], c["t0"], flags, key, np.flatnonzero(got != exp)[0], got[np.flatnonzero(got != exp)[0]],
                            exp[np.flatnonzero(got != exp)[0]])
                    assert (out["idx0"][p, nQ:] == -1).all() and (out["idx1"][p, nQ:] == -1).all() and (out["dist0"][p, nQ:] == -1).all() and \
                        (out["dist1"][p, nQ:] == -1).all() and not out["ratio_ok"][p, nQ:].any(), "case %d flags %d: output rows past the query count were written" % (base + p, flags)
    finally:
        rb.ex.debug_stereo_flags(0)


# ---- sizes: 1 to 17 train tiles (each wave 0 to 5 tiles, the prefetch loop entered 0, 1 and 2 times), full and partial last tile ----------------------------------
NT = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 160, 161, 256, 257, 288, 289, 384, 385, 416, 417, 544)
QSETS = ((1, 0, 0), (33, 7, 45), (64, 31, 1), (32, 0, 0))


def _size_cases():
    rng = np.random.default_rng(11)
    cases = []
    for nT in NT:
        for nQ, q0, t0 in QSETS:
            q = rng.integers(0, 256, (nQ, 32), dtype=np.uint8); t = rng.integers(0, 256, (nT, 32), dtype=np.uint8)
            # a few near neighbours, so that the two best are not always two arbitrary rows around distance 100: the last row of the set and row 0 among them
            for i in range(nQ):
                t[(nT - 1 - i) % nT] = at_distance(rng, q[i], 10 + i % 50)
            cases.append(_case(q, t, q0, t0))
    return cases


def _check_sizes(lib):
    cases = _size_cases()
    assert len(cases) == len(NT) * len(QSETS)
    assert all(c["exp"]["dist0"].min() > 0 for c in cases)             # no train row equals a query: a neighbour at distance 0 can only be a leak
    _run(lib, cases)


def test_knn2_set_sizes_around_every_tile_boundary_emulated(emu_lib):
    _check_sizes(emu_lib)


@pytest.mark.gpu
def test_knn2_set_sizes_around_every_tile_boundary_gpu(hip_lib):
    _check_sizes(hip_lib)


# ---- the ratio test at its boundary --------------------------------------------------------------------------------------------------------------------------
def _ratio_pairs():
    pairs = []
    for d1 in range(1, 257):
        for d0 in sorted({int(np.floor(0.7 * d1)), int(np.ceil(0.7 * d1)), d1}):
            pairs.append((d0, d1))
    return pairs


def _ratio_cases():
    rng = np.random.default_rng(12)
    cases = []
    for k, (d0, d1) in enumerate(_ratio_pairs()):
        q = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        near, far = at_distance(rng, q[0], d0), at_distance(rng, q[0], d1)
        t = np.stack([far, near]) if k & 1 else np.stack([near, far])  # the nearer one first and second in turn
        cases.append(_case(q, t, k % 5, k % 7))
    return cases


def _check_ratio(lib):
    pairs, cases = _ratio_pairs(), _ratio_cases()
    exp = {}
    for (d0, d1), c in zip(pairs, cases):
        e = c["exp"]
        assert e["dist0"][0] == d0 and e["dist1"][0] == d1, "the construction missed its distances"
        exp[(d0, d1)] = int(e["ratio_ok"][0])
    # The all-float form `(float)d0 < (float)d1 * 0.7f` was expected to answer differently at (63, 90), (119, 170), (126, 180), where 0.7 d1 is an integer
    # and the double product lies one ulp below it (90 * 0.7 = 62.99999999999999).  It does not: the float product 90 * 0.7f = 62.9999989.. rounds to the
    # float 63.0 exactly, and `63 < 63` is as false as `63 < 62.99999999999999`.  test_ratio_forms_agree_on_every_pair_of_distances shows that for all
    # 257 x 257 pairs, so no input can tell the two forms apart; what these pairs do pin is the strictness of the comparison and the constant itself.
    assert not any(exp[k] for k in ((63, 90), (119, 170), (126, 180), (7, 10), (256, 256)))
    assert all(exp[k] for k in ((62, 90), (118, 170), (125, 180), (179, 256)))
    assert not exp[(180, 256)]                                             # 0.7 * 256 = 179.2
    assert sum(exp.values()) > 200 and sum(1 - v for v in exp.values()) > 400
    _run(lib, cases)


def test_ratio_forms_agree_on_every_pair_of_distances():
    """Hamming distances of 256-bit descriptors are the integers 0..256.  On all of them the reference's double form, an all-float form and the exact rational
    10 d0 < 7 d1 agree: rounding 0.7 or the product to float moves the right-hand side by less than half a float ulp of an integer it could cross only by
    reaching it, and at equality all three say no.  (So a kernel that evaluated the ratio in float would be right; the kernels keep the reference's double.)"""
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    dbl = d0.astype(np.float32).astype(np.float64) < d1.astype(np.float32).astype(np.float64) * 0.7
    flt = d0.astype(np.float32) < (d1.astype(np.float32) * np.float32(0.7)).astype(np.float32)
    exact = 10 * d0 < 7 * d1
    assert np.array_equal(dbl, flt) and np.array_equal(dbl, exact)
    assert not np.array_equal(dbl, 10 * d0 <= 7 * d1)                      # `<=` differs, at the pairs (7 k, 10 k), k = 1..25, which the boundary cases contain
    assert {(int(a), int(b)) for a, b in zip(*np.nonzero(dbl != (10 * d0 <= 7 * d1)))} - {(0, 0)} <= set(_ratio_pairs())


def test_knn2_ratio_decided_in_double_at_the_boundary_emulated(emu_lib):
    _check_ratio(emu_lib)


@pytest.mark.gpu
def test_knn2_ratio_decided_in_double_at_the_boundary_gpu(hip_lib):
    _check_ratio(hip_lib)


# ---- ties and extremes ---------------------------------------------------------------------------------------------------------------------------------------
def _tie_cases():
    """train sets of 300 rows (ten tiles, the last one partial) and 320 rows (ten full tiles) behind t0 = 5; query k owns the rows of scenario k: 2 or 3 rows at one
    distance below every other row's, at chosen accumulator positions.  Returns (cases, [(case, query, expected idx0, expected idx1)])."""
    rng = np.random.default_rng(13)
    T = lambda tile, row: 32 * tile + row
    scen = [
        (T(1, 8), T(1, 9)), (T(1, 12), T(1, 13), T(1, 14)),                 # one lane: accumulator registers i, i + 1 (, i + 2)
        (T(2, 0), T(2, 4)), (T(2, 1), T(2, 5), T(2, 9)),                    # the two lanes of a query (the __shfl_xor merge); the third back in the first lane
        (T(6, 19), T(6, 23)), (T(0, 27), T(0, 31)),
        (T(1, 3), T(5, 3)), (T(1, 7), T(5, 2), T(9, 7)),                    # tiles w, w + 4 (, w + 8) of wave 1: both tile buffers of the prefetch loop and its tail
        (T(0, 30), T(4, 1), T(8, 17)), (T(3, 5), T(7, 5)),
        (T(2, 10), T(3, 10)), (T(0, 2), T(2, 2), T(7, 2)),                  # tiles of different waves (the merge through LDS)
        (T(3, 31), T(4, 0)), (T(1, 20), T(2, 20), T(3, 20)), (T(0, 4), T(9, 1)),
        (T(5, 6), T(5, 6 + 4), T(6, 6)),                                    # two lanes of one wave and another wave
    ]
    cases, designed = [], []
    for nT in (300, 320):
        nQ = len(scen) + 6
        q = rng.integers(0, 256, (nQ, 32), dtype=np.uint8); t = rng.integers(0, 256, (nT, 32), dtype=np.uint8)
        want = []
        for k, rows in enumerate(scen):
            assert max(rows) < nT - 2
            for r in rows:
                t[r] = at_distance(rng, q[k], 17 + k)
            want.append((k, rows[0], rows[1]))
        k = len(scen)
        # across the end of the set: the last row and, just outside, its twin at the same distance; a runner-up further away inside
        t[nT - 1] = at_distance(rng, q[k], 30); t[150] = at_distance(rng, q[k], 31)
        after = np.stack([at_distance(rng, q[k], 30), at_distance(rng, q[k + 1], 12)])          # .. and a row outside that is NEARER than any inside (query k + 1)
        want.append((k, nT - 1, 150))
        t[200] = at_distance(rng, q[k + 1], 40); t[nT - 2] = at_distance(rng, q[k + 1], 40)
        want.append((k + 1, 200, nT - 2))
        # across the start of the set: row 0 and its twin in front of t0
        t[0] = at_distance(rng, q[k + 2], 25); t[1] = at_distance(rng, q[k + 2], 25)
        before = np.stack([at_distance(rng, q[k + 2], 25)])
        want.append((k + 2, 0, 1))
        # the query itself twice: distance 0 at two indices (every row outside the set that the case does not set is a copy of a query as well)
        t[77] = q[k + 3]; t[266] = q[k + 3]
        want.append((k + 3, 77, 266))
        # distance 0 once and a tie for the second place across waves
        t[100] = q[k + 4]; t[33] = at_distance(rng, q[k + 4], 9); t[130] = at_distance(rng, q[k + 4], 9)
        want.append((k + 4, 100, 33))
        # the complement of the query at two rows: distance 256 must lose against everything, the query's neighbours are ordinary rows
        t[212] = ~q[k + 5]; t[213] = ~q[k + 5]
        c = _case(q, t, 3, 5, before=before, after=after)
        cases.append(c)
        designed += [(c, a, b, d) for a, b, d in want]
        assert c["exp"]["idx0"][k + 5] not in (212, 213) and c["exp"]["idx1"][k + 5] not in (212, 213)
    # complements only: both distances 256 (and with a third complement outside the set)
    for nT in (2, 3, 33):
        q = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        c = _case(q, np.tile(~q, (nT, 1)), 2, 1, after=~q)
        assert c["exp"]["dist0"][0] == 256 and c["exp"]["dist1"][0] == 256
        cases.append(c); designed.append((c, 0, 0, 1))
    # duplicates only: distance 0 twice, nothing else
    q = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    c = _case(q, np.tile(q, (2, 1)), 0, 0)
    assert c["exp"]["dist0"][0] == 0 and c["exp"]["dist1"][0] == 0
    cases.append(c); designed.append((c, 0, 0, 1))
    return cases, designed


def _check_ties(lib):
    cases, designed = _tie_cases()
    for c, k, i0, i1 in designed:                                          # the construction reached its target: the lower index first, no twin from outside
        e = c["exp"]
        assert (e["idx0"][k], e["idx1"][k]) == (i0, i1), (k, i0, i1, e["idx0"][k], e["idx1"][k])
    assert sum(1 for c, k, _, _ in designed if c["exp"]["dist0"][k] == c["exp"]["dist1"][k]) >= 30
    _run(lib, cases)


def test_knn2_ties_by_lane_tile_wave_and_set_boundary_emulated(emu_lib):
    _check_ties(emu_lib)


@pytest.mark.gpu
def test_knn2_ties_by_lane_tile_wave_and_set_boundary_gpu(hip_lib):
    _check_ties(hip_lib)
