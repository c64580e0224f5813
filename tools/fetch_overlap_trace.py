#!/usr/bin/env python
"""Where the keypoint / descriptor downloads of orbx_fetch sit relative to the kernels of their handle, from one
`rocprofv3 --kernel-trace --memory-copy-trace --output-format csv` run of bench.py (profiles/fetch_overlap/).

usage: fetch_overlap_trace.py DIR [TIMED]   (DIR holds *_kernel_trace.csv and *_memory_copy_trace.csv; TIMED = chains of the timed region, default 12)

For every extraction chain (one k_orient_brief dispatch) it pairs the matcher kernels that follow on the same stream and the first two large
device-to-host copies (records, descriptors) that start after the end of k_orient_brief, on whichever stream they were issued, attributing a
copy to the chain whose k_orient_brief ended last before it among the chains that have not received theirs yet (fetches are in chain order).
Prints one row per chain and the medians over the last TIMED chains (the timed steps: set-up and warm-up come first), in microseconds.
"""
import csv
import glob
import os
import statistics
import sys

BIG_US = 50.0            # the two big copies take 100-250 us each; the counts, uRight / depth blocks are far shorter


def rows(d, pat):
    f = glob.glob(os.path.join(d, "**", pat), recursive=True)
    if not f:
        raise SystemExit("no %s under %s" % (pat, d))
    return list(csv.DictReader(open(f[0])))


def main(d, timed=12):
    ks = rows(d, "*kernel_trace.csv")
    cs = rows(d, "*memory_copy_trace.csv")
    t0 = min(int(r["Start_Timestamp"]) for r in ks)
    us = lambda t: (int(t) - t0) / 1e3
    chains = []
    for r in ks:
        n = r["Kernel_Name"]
        if n.startswith("k_orient_brief") or "k_orient_brief" in n.split("(")[0]:
            chains.append({"stream": r["Stream_Id"], "ob_end": us(r["End_Timestamp"]), "match": None, "median": None, "copies": []})
    chains.sort(key=lambda c: c["ob_end"])
    by_stream = {}
    for c in chains:
        by_stream.setdefault(c["stream"], []).append(c)
    for r in ks:
        n = r["Kernel_Name"].split("(")[0]
        key = "match" if "k_stereo_match" in n else "median" if "k_stereo_median" in n else None
        if not key:
            continue
        s, e = us(r["Start_Timestamp"]), us(r["End_Timestamp"])
        prev = [c for c in by_stream.get(r["Stream_Id"], []) if c["ob_end"] <= s + 1e-3]
        if prev and prev[-1][key] is None:
            prev[-1][key] = (s, e)
    big = sorted(((us(r["Start_Timestamp"]), us(r["End_Timestamp"]), r["Stream_Id"]) for r in cs
                  if r["Direction"].endswith("DEVICE_TO_HOST") and (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 >= BIG_US))
    ci = 0
    for s, e, sid in big:
        while ci < len(chains) and len(chains[ci]["copies"]) >= 2:
            ci += 1
        if ci == len(chains):
            break
        if s >= chains[ci]["ob_end"]:
            chains[ci]["copies"].append((s, e, sid))
    print("%-5s %-7s %-7s %10s %12s %12s %12s %12s %9s %s" % ("chain", "stream", "cpstrm", "ob_end", "copy_start", "copy_end", "match_start", "median_end", "copy_us", "copies vs matcher"))
    stat = {"start_after_ob": [], "start_after_median": [], "copy_us": [], "overlap_us": []}
    for i, c in enumerate(chains):
        if len(c["copies"]) < 2 or not c["match"] or not c["median"]:
            continue
        cs0, ce = c["copies"][0][0], c["copies"][1][1]
        ms, me = c["match"][0], c["median"][1]
        ov = max(0.0, min(ce, me) - max(cs0, ms))
        where = "behind the matcher" if cs0 >= me - 1e-3 else "beside the matcher" if ov > 0 else "before the matcher"
        print("%-5d %-7s %-7s %10.1f %12.1f %12.1f %12.1f %12.1f %9.1f %s" % (i, c["stream"], c["copies"][0][2], c["ob_end"], cs0, ce, ms, me, ce - cs0, where))
        if i >= len(chains) - timed:
            stat["start_after_ob"].append(cs0 - c["ob_end"]); stat["start_after_median"].append(cs0 - me)
            stat["copy_us"].append(ce - cs0); stat["overlap_us"].append(ov)
    for k, v in stat.items():
        if v:
            print("median %-20s %9.1f us  (min %.1f, max %.1f, n %d)" % (k, statistics.median(v), min(v), max(v), len(v)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else ".", int(sys.argv[2]) if len(sys.argv) > 2 else 12)
