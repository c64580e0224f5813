#!/usr/bin/env python3
"""Static instruction counts of k_fast_cells by source-line range, from the device assembly with line tables:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -gline-tables-only -S -x hip k_fast.hip -o k_fast_lines.s
    python tools/fast_phase_count.py k_fast_lines.s NAME=FIRST-LAST [NAME=FIRST-LAST ..]

Every instruction of the kernel `--kernel` (default k_fast_cells; both wide and common instantiations of fast_cell are inlined into it) is
attributed to the k_fast.hip line of the `.loc` in force; an instruction whose `.loc` names another file (an inlined helper of orbx_block.h or
orbx_types.h) goes to the last k_fast.hip line seen before it.  Counts are static (per instance in the code, not per execution): a loop body
counts once, and the scheduler may move an instruction across a range boundary.  No GPU needed."""
import argparse
import re
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("ranges", nargs="*", help="NAME=FIRST-LAST of k_fast.hip")
    ap.add_argument("--kernel", default="k_fast_cells")
    ap.add_argument("--source", default="k_fast.hip")
    ap.add_argument("--split", default="108-126", help="lines of the prologue of a run: seeing them after the late lines starts the next inlined copy")
    ap.add_argument("--late", default="300-372", help="lines of the last phases")
    a = ap.parse_args()
    a.split_lo, a.split_hi = (int(x) for x in a.split.split("-"))
    a.late_from, a.late_to = (int(x) for x in a.late.split("-"))
    ranges = []
    for r in a.ranges:
        name, span = r.split("=")
        lo, hi = span.split("-")
        ranges.append((name, int(lo), int(hi)))
    files, inside, line, seg, late = {}, False, 0, 0, False
    per_line = {}
    sym = re.compile(r"^(_ZN4orbx\d+%s[A-Z]\S*):" % re.escape(a.kernel))
    for t in open(a.asm):
        s = t.strip()
        m = re.match(r'\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', s)
        if m:
            files[int(m.group(1))] = m.group(2)
            continue
        if sym.match(s):
            inside = True
            continue
        if not inside:
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if files.get(int(m.group(1)), "").endswith(a.source):
                line = int(m.group(2))
                # fast_cell is inlined twice (common pitch, then the cell's own): the second copy starts where the lines fall back to the run's prologue
                if a.split_lo <= line <= a.split_hi and late:
                    seg += 1; late = False
                if line >= a.late_from and line <= a.late_to:
                    late = True
            continue
        m = re.match(r"([a-z][a-z0-9_]+)\b", s)
        if not m or s.startswith(".") or s.endswith(":"):
            continue
        op = m.group(1)
        if op.startswith("v_"):
            kind = "valu"
        elif op.startswith("ds_"):
            kind = "lds"
        elif op.startswith(("global_", "buffer_", "flat_")):
            kind = "vmem"
        elif op.startswith("s_"):
            kind = "salu"
        else:
            continue
        d = per_line.setdefault((seg, line), {"valu": 0, "lds": 0, "vmem": 0, "salu": 0})
        d[kind] += 1
    kinds = ("valu", "lds", "vmem", "salu")
    print("%-36s %6s %6s %6s %6s" % ("range", "valu", "lds", "vmem", "salu"))
    for sg in range(seg + 1):
        tot = {k: sum(d[k] for (g, l), d in per_line.items() if g == sg) for k in kinds}
        print("%-36s %6d %6d %6d %6d" % ("copy %d, all lines" % sg, tot["valu"], tot["lds"], tot["vmem"], tot["salu"]))
        for name, lo, hi in ranges:
            c = {k: sum(d[k] for (g, l), d in per_line.items() if g == sg and lo <= l <= hi) for k in kinds}
            print("%-36s %6d %6d %6d %6d" % ("copy %d, %s (%d-%d)" % (sg, name, lo, hi), c["valu"], c["lds"], c["vmem"], c["salu"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
