"""The rectified stereo row search (csrc/k_match.hip: k_stereo_match, k_stereo_median) on descriptors built for the values where it decides.  Keypoints, pyramids and
the right frame's row index are those of natural synth.stereo_pair images - orbm_stereo_match reads the right keypoints through what their extraction left behind
(tests/resident_inject.py), so only DESCRIPTORS are injected, on both sides.  Expected mvuRight / mvDepth / match count: ol.oracle_stereo on the same keypoints and
the same overwritten descriptors, bit for bit, for the normal candidate order, the reversed one and the every-lane walk (orbx_debug_stereo_flags 0, 1, 4).

Every chosen left keypoint gets a random descriptor of its own, and one or two right keypoints of its candidate list get rows at chosen distances from it (a
right keypoint serves one left keypoint only); every other right row, natural or built for another left keypoint, is ~128 bits away from it.  The keypoints that
are not chosen keep their natural descriptors and matches, so that the median of step 5 stays where the natural pair has it and the chosen matches survive it:
  d74 / d75     the best candidate at th_orb - 1 / th_orb: the last distance that goes on to the SAD refinement and the first that does not
  d99 / d100    the best candidate at TH_HIGH - 1 / TH_HIGH: the last distance that replaces the starting value and the first that does not
  tie           two candidates at the same best distance: the lower right index wins, whatever the visiting order
  octave+2 / -2 an exact copy of the left descriptor on a keypoint of the band two octaves above / below: it must lose against a candidate at distance 40
  outside       an exact copy on a keypoint of the band whose x lies just outside [uL - maxD, uL] (on either side, the nearest there is): it must lose
  edge          an exact copy on a candidate whose x equals uL exactly - there `x <= maxU` decides (these pairs have such candidates: bands of disparity 0)
th_orb and TH_HIGH come from matcher.ORBmatcher.  The designated candidate is the one the natural descriptors matched and refined successfully, so that a match
which wrongly goes on to the refinement changes the output.  mbf is chosen for maxD = 40 px: both ends of the disparity range lie inside the image.

The intermediate view - best distance and index per left keypoint, recomputed in numpy from the oracle's row bands - asserts that every situation occurred for at
least 5 left keypoints."""
import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd import ComputeStereoMatches, synth
from orb_slam3_detailed_comments_amd.matcher import ORBmatcher
from resident_inject import ResidentBatch, all_pairs_hamming, at_distance

W, H, NF = 376, 240, 500
B_LINE = 0.110074
BF = 40.0 * B_LINE
SEEDS = (20, 21, 22)
P = len(SEEDS)
TH_HIGH = ORBmatcher.TH_HIGH
TH_ORB = (ORBmatcher.TH_HIGH + ORBmatcher.TH_LOW) // 2
SITUATIONS = ("d74", "d75", "d99", "d100", "tie", "octave+2", "octave-2", "outside", "edge")
f32 = np.float32


def _candidates(kL, kR):
    """(band [NL, NR], valid [NL, NR]): right keypoints in the row band of each left keypoint, and those that also pass the octave and column gates
    (Frame::ComputeStereoMatches, src/Frame.cc:1135-1215; float arithmetic as there)"""
    sf = np.ones(8, f32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * f32(1.2)
    r = f32(2.0) * sf[kR["octave"]]
    lo = np.floor(kR["y"] - r).astype(np.int64); hi = np.ceil(kR["y"] + r).astype(np.int64)
    row = kL["y"].astype(np.int64)[:, None]
    band = (row >= lo[None, :]) & (row <= hi[None, :])
    maxD = f32(BF) / f32(B_LINE)
    minU = (kL["x"] - maxD).astype(f32)[:, None]; maxU = kL["x"][:, None]
    octs = np.abs(kR["octave"][None, :] - kL["octave"][:, None]) <= 1
    cols = (kR["x"][None, :] >= minU) & (kR["x"][None, :] <= maxU)
    return band, band & octs & cols, octs, cols


def _best(valid, dL, dR):
    """the view: (bestDist, bestIdxR) per left keypoint as the reference's loop leaves them - start TH_HIGH / 0, replace on a strictly smaller distance, ascending index"""
    d = all_pairs_hamming(dL, dR)
    d = np.where(valid, d, 1 << 20)
    idx = d.argmin(1); best = d.min(1)
    hit = best < TH_HIGH
    return np.where(hit, best, TH_HIGH), np.where(hit, idx, 0)


def _construct(kL, dL0, kR, dR0, u_nat, seed):
    """descriptors for one pair and the situation of every chosen left keypoint"""
    rng = np.random.default_rng(seed)
    band, valid, octs, cols = _candidates(kL, kR)
    nat_best, nat_idx = _best(valid, dL0, dR0)
    dL = dL0.copy(); dR = dR0.copy()
    claimed = np.zeros(len(kR), bool)
    chosen = {}
    special_first = ("octave+2", "octave-2", "edge", "outside")                                  # the situations that need particular keypoints take what they can get first
    order = [i for i in range(len(kL)) if u_nat[i] >= 0 and nat_best[i] < TH_ORB]
    todo = {s: [] for s in SITUATIONS}

    def free(mask):
        return np.flatnonzero(mask & ~claimed)

    def far(c, r, iL):
        """those of c that lie more than 8 pixels of the left keypoint's level from right keypoint r, the farthest first: a wrong winner then sends the SAD refinement
        (5 shifts either way at that level) somewhere else.  A corner is often found on several octaves at nearly one x; such a twin would be refined to the same mvuRight."""
        gap = np.abs(kR["x"][c] - kR["x"][r])
        c = c[gap > 8.0 * 1.2 ** int(kL["octave"][iL])]
        return c[np.argsort(-np.abs(kR["x"][c] - kR["x"][r]), kind="stable")]

    def rows_for(sit, iL, r):
        """{right keypoint: distance from the left keypoint's new descriptor} that makes situation `sit` at left keypoint iL, whose natural match is r; None: not possible here"""
        uL = kL["x"][iL]
        if sit == "edge":
            c = free(valid[iL] & (kR["x"] == uL)); c = c[c != r]
            if len(c):
                return {int(c[0]): 0, r: 40}
            return {r: 0} if kR["x"][r] == uL else None                           # the natural match itself sits at uL: the copy goes there
        if sit.startswith("octave"):
            c = far(free(band[iL] & cols[iL] & (kR["octave"] - kL["octave"][iL] == int(sit[6:]))), r, iL)
            return {int(c[0]): 0, r: 40} if len(c) else None
        if sit == "outside":
            above = free(band[iL] & octs[iL] & (kR["x"] > uL)); below = free(band[iL] & octs[iL] & (kR["x"] < (uL - f32(BF) / f32(B_LINE)).astype(f32)))
            out = {}
            if len(above):
                out[int(above[np.argmin(kR["x"][above])])] = 0
            if len(below):
                out[int(below[np.argmax(kR["x"][below])])] = 0
            if not out:
                return None
            out[r] = 40
            return out
        if sit == "tie":
            c = far(free(valid[iL]), r, iL)
            return {int(c[0]): 33, r: 33} if len(c) else None
        return {r: {"d74": TH_ORB - 1, "d75": TH_ORB, "d99": TH_HIGH - 1, "d100": TH_HIGH}[sit]}

    for sit_pass in (special_first, ("tie",), ("d74", "d75", "d99", "d100")):
        for iL in order:
            r = int(nat_idx[iL])
            if iL in chosen or claimed[r]:
                continue
            for sit in sorted((s for s in sit_pass if len(todo[s]) < 8), key=lambda s: len(todo[s])):      # the situation that has the fewest so far, if it can be made here
                rows = rows_for(sit, iL, r)
                if rows is None:
                    continue
                D = rng.integers(0, 256, 32, dtype=np.uint8)
                dL[iL] = D
                for j, dist in rows.items():
                    dR[j] = at_distance(rng, D, dist); claimed[j] = True
                chosen[iL] = sit; todo[sit].append(iL)
                break
    return dL, dR, chosen, (band, valid, octs, cols), nat_idx


_CASE = []


def _case():
    """images, oracle extractions and constructed descriptors: made once, shared by the emulator and the GPU form"""
    if _CASE:
        return _CASE[0]
    pairs = [synth.stereo_pair(W, H, seed=s, nrect=800, max_disp=30) for s in SEEDS]
    images = np.stack([p[0] for p in pairs] + [p[1] for p in pairs])
    per_pair = []
    counts = {s: 0 for s in SITUATIONS}
    went_on = 0
    for p, (L, R) in enumerate(pairs):
        oL, oR = ol.OracleExtractor(NF), ol.OracleExtractor(NF)
        (_, kL, dL0), (_, kR, dR0) = oL.extract(L), oR.extract(R)
        u_nat, _, n_nat = ol.oracle_stereo(oL, oR, kL, dL0, kR, dR0, BF, B_LINE)
        assert n_nat > 60
        dL, dR, chosen, (band, valid, octs, cols), nat_idx = _construct(kL, dL0, kR, dR0, u_nat, 100 + p)
        u, d, n = ol.oracle_stereo(oL, oR, kL, dL, kR, dR, BF, B_LINE)
        # the view: every situation is what it was built to be
        best, idx = _best(valid, dL, dR)
        dist = all_pairs_hamming(dL, dR)
        for iL, sit in chosen.items():
            r = int(nat_idx[iL])
            if sit in ("d74", "d75", "d99"):
                ok = best[iL] == {"d74": TH_ORB - 1, "d75": TH_ORB, "d99": TH_HIGH - 1}[sit] and idx[iL] == r
                ok = ok and (sit == "d74" or u[iL] < 0)                           # only th_orb - 1 goes on to the refinement
                went_on += sit == "d74" and u[iL] >= 0
            elif sit == "d100":
                ok = best[iL] == TH_HIGH and idx[iL] == 0 and dist[iL, r] == TH_HIGH and u[iL] < 0
            elif sit == "tie":
                tied = np.flatnonzero(valid[iL] & (dist[iL] == 33))
                ok = best[iL] == 33 and len(tied) == 2 and idx[iL] == tied.min()
            elif sit == "edge":
                ok = best[iL] == 0 and kR["x"][idx[iL]] == kL["x"][iL]
            else:                                                                  # octave / outside: a copy (distance 0) in the band that is no candidate; the candidate at 40 wins
                copies = np.flatnonzero(band[iL] & (dist[iL] == 0))
                ok = best[iL] == 40 and idx[iL] == r and len(copies) >= 1 and not valid[iL][copies].any()
                if sit.startswith("octave"):
                    ok = ok and cols[iL][copies].all() and (kR["octave"][copies] - kL["octave"][iL] == int(sit[6:])).all()
                else:
                    ok = ok and octs[iL][copies].all() and not cols[iL][copies].any()
            assert ok, (p, iL, sit, best[iL], idx[iL], r)
            counts[sit] += 1
        for a in (u, d, dL, dR):
            a.setflags(write=False)
        per_pair.append(dict(kL=kL, kR=kR, dL0=dL0, dR0=dR0, dL=dL, dR=dR, u=u, d=d, n=n, chosen=chosen))
    print("situations:", counts, "matches per pair:", [c["n"] for c in per_pair])
    assert all(counts[s] >= 5 for s in SITUATIONS), counts
    assert went_on >= 5, "matches at th_orb - 1 whose refinement succeeds (as it did on the natural descriptors) and survives the median test"
    _CASE.append((images, per_pair))
    return _CASE[0]


def _check(lib):
    images, per_pair = _case()
    rb = ResidentBatch(lib, 2 * P, nfeatures=NF, images=images)
    try:
        for p, c in enumerate(per_pair):
            NL, NR = len(c["kL"]), len(c["kR"])
            assert rb.natural[p][1].tobytes() == c["kL"].tobytes() and rb.natural[P + p][1].tobytes() == c["kR"].tobytes()
            assert rb.natural[p][2].tobytes() == c["dL0"].tobytes() and rb.natural[P + p][2].tobytes() == c["dR0"].tobytes()
            rb.desc[p, :NL] = c["dL"]; rb.desc[P + p, :NR] = c["dR"]
        rb.put_descriptors()
        for flags in (0, 1, 4):
            rb.ex.debug_stereo_flags(flags)
            u, d, n = ComputeStereoMatches(rb.ex, rb.ex, BF, B_LINE, 0, P, P)
            for p, c in enumerate(per_pair):
                NL = len(c["kL"])
                bad = np.flatnonzero(u[p, :NL].view(np.uint32) != c["u"].view(np.uint32))
                assert len(bad) == 0, "pair %d flags %d: mvuRight differs at left keypoints %s (situations %s): %r, expected %r" % (
                    p, flags, bad[:8], [c["chosen"].get(int(i)) for i in bad[:8]], u[p, bad[:8]], c["u"][bad[:8]])
                assert d[p, :NL].tobytes() == c["d"].tobytes(), "pair %d flags %d: mvDepth differs" % (p, flags)
                assert (u[p, NL:] == -1).all() and (d[p, NL:] == -1).all()
                assert int(n[p]) == c["n"]
        # the ties bite: with the distance-only compare (bit 1) in the walk that meets the higher index first (bit 2) the higher index wins, and the refinement starts
        # from the other right keypoint (more than 8 level pixels away)
        rb.ex.debug_stereo_flags(6)
        u, d, n = ComputeStereoMatches(rb.ex, rb.ex, BF, B_LINE, 0, P, P)
        changed = sum(int(u[p, iL].view(np.uint32) != c["u"][iL].view(np.uint32)) for p, c in enumerate(per_pair) for iL, sit in c["chosen"].items() if sit == "tie")
        assert changed >= 5, "the distance-only tie rule changed %d of the constructed ties" % changed
    finally:
        rb.ex.debug_stereo_flags(0)
        rb.close()


def test_stereo_constructed_descriptors_emulated(emu_lib):
    _check(emu_lib)


@pytest.mark.gpu
def test_stereo_constructed_descriptors_gpu(hip_lib):
    _check(hip_lib)
