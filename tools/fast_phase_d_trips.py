#!/usr/bin/env python3
"""What the back half of k_fast_cells does per cell on the bench inputs, from an emulator run (CPU only):

    python tools/fast_phase_d_trips.py [--images 2] [--workload corner_field|natural]

For every FAST cell of every level: corners at iniThFAST (numpy segment test on the emulator's pyramid level), NMS survivors (the emulator's
debug_candidates), the words of the parent kernel's row-major bitmap (32 score-tile bytes each, 64 words per wave trip) that hold a survivor,
and the trips of its bit-extraction loop: per 64-word chunk the largest popcount of a word, for all 64 lanes.  The cell grid and the LDS pitch
are restated from csrc/orbx_api.cpp (the FAST cell grid) and k_fast.hip (window, pitch)."""
import argparse
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_detailed_comments_amd import _lib, synth                      # noqa: E402
from orb_slam3_detailed_comments_amd.extractor import ORBextractor           # noqa: E402

K_BORDER, K_PITCH = 16, 48


def cells_of_level(w, h):
    minBX, minBY, maxBX, maxBY = K_BORDER, K_BORDER, w - K_BORDER, h - K_BORDER
    ncols, nrows = int((maxBX - minBX) / 35.0), int((maxBY - minBY) / 35.0)
    wcell, hcell = math.ceil((maxBX - minBX) / ncols), math.ceil((maxBY - minBY) / nrows)
    out = []
    for i in range(nrows):
        iniY = minBY + i * hcell
        if iniY >= maxBY - 3:
            continue
        maxY = min(iniY + hcell + 6, maxBY)
        for j in range(ncols):
            iniX = minBX + j * wcell
            if iniX >= maxBX - 6:
                continue
            maxX = min(iniX + wcell + 6, maxBX)
            out.append((iniX + 3, maxX - 3, iniY + 3, maxY - 3))
    return out


def corner_mask(img, t):
    a = img.astype(np.int16)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    m = np.zeros((h, w), bool)
    for sign in (1, -1):
        ring = np.stack([sign * (a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c) > t for dx, dy in synth._RING])
        r2 = np.concatenate([ring, ring[:8]])
        acc = np.zeros_like(ring[0])
        for s in range(16):
            acc |= np.logical_and.reduce(r2[s:s + 9])
        m[3:h - 3, 3:w - 3] |= acc
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--workload", default="corner_field", choices=["corner_field", "natural"])
    ap.add_argument("--ini", type=int, default=20)
    a = ap.parse_args()
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["make", "-C", d, "-s"], check=True, stdout=subprocess.DEVNULL)
    lib = _lib.OrbxLib(os.path.join(d, "liborbx_emu.so"))
    ex = ORBextractor(1200, 1.2, 8, a.ini, 7, lib=lib)
    gen = synth.stereo_pair if a.workload == "corner_field" else synth.natural_stereo_pair
    ncell = corners = surv = words = chunks = trips = c_trips = 0
    hist = {}
    for s in range(a.images):
        img = gen(752, 480, seed=s // 2)[s & 1]
        ex(img)
        for l in range(8):
            lv = ex.pyramid_level(l)
            cm = corner_mask(lv, a.ini)
            cand = ex.debug_candidates(l)
            px, py = cand[:, 0] + K_BORDER, cand[:, 1] + K_BORDER
            for (x0, x1, y0, y1) in cells_of_level(lv.shape[1], lv.shape[0]):
                if x1 <= x0 or y1 <= y0:
                    continue
                gx0, gx1 = (x0 - 3) & ~3, (x1 + 6) & ~3
                wp = K_PITCH if gx1 - gx0 <= K_PITCH else gx1 - gx0
                xo = x0 - 3 - gx0
                sel = (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
                o = (py[sel] - y0 + 1) * wp + xo + 3 + (px[sel] - x0)
                nwords = (wp * (y1 - y0 + 2) + 31) >> 5
                pop = np.bincount(o >> 5, minlength=nwords)
                nc = int(cm[y0:y1, x0:x1].sum())
                ncell += 1; corners += nc; surv += int(sel.sum()); words += int((pop > 0).sum())
                c_trips += (nc + 63) // 64
                for c0 in range(0, nwords, 64):
                    t = int(pop[c0:c0 + 64].max())
                    chunks += 1; trips += t
                    hist[t] = hist.get(t, 0) + 1
    print("workload %s, %d images, iniThFAST %d: %d cells" % (a.workload, a.images, a.ini, ncell))
    print("per cell: %.1f corners (%.2f trips of 64), %.1f survivors in %.1f bitmap words, %.2f chunks of 64 words, %.2f trips of the bit loop"
          % (corners / ncell, c_trips / ncell, surv / ncell, words / ncell, chunks / ncell, trips / ncell))
    print("bit-loop trips per chunk: " + ", ".join("%d: %d" % (k, hist[k]) for k in sorted(hist)))


if __name__ == "__main__":
    sys.exit(main())
