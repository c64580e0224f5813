#!/usr/bin/env python3
"""Reads the .gcda files a coverage build of the emulator library (tools/emu_coverage.sh) left behind - the main library and every library that
tests/test_emu_variants.py built - and prints, summed over all of them: line and branch figures per source file, the never-executed lines and the never-taken
branches of the kernel sources (k_*.hip and the headers of csrc/).  A template or inline function that is instantiated several times counts once per instantiation
for its branches (a branch that only bow_search_body<false> takes is still listed for bow_search_body<true>) and once per line for its lines; an instantiation
that never ran is named once.  Branches that only an exception takes are left out.  usage: emu_coverage_report.py <directory with the .gcda files> [repository root]"""
import collections
import json
import os
import subprocess
import sys

work = os.path.abspath(sys.argv[1])
root = os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), ".."))
csrc = os.path.join(root, "orb_slam3_detailed_comments_amd", "csrc")

lines = collections.defaultdict(int)             # (file, line) -> executions
branches = collections.defaultdict(int)          # (file, line, function, index) -> times taken
functions = collections.defaultdict(int)         # (file, function) -> calls
builds = 0
for d, _, files in sorted(os.walk(work)):
    for f in sorted(files):
        if not f.endswith(".gcda"):
            continue
        builds += 1
        out = subprocess.run(["gcov", "-b", "-c", "--json-format", "--stdout", f], cwd=d, capture_output=True, text=True, check=True).stdout
        for doc in out.splitlines():
            if not doc.startswith("{"):
                continue
            for src in json.loads(doc)["files"]:
                path = os.path.normpath(os.path.join(root, src["file"]))
                if os.path.dirname(path) != csrc:
                    continue
                name = os.path.basename(path)
                for fn in src.get("functions", []):
                    functions[(name, fn["name"])] += fn["execution_count"]
                for ln in src["lines"]:
                    lines[(name, ln["line_number"])] += ln["count"]
                    for i, b in enumerate(ln["branches"]):
                        if not b["throw"]:
                            branches[(name, ln["line_number"], ln.get("function_name", ""), i)] += b["count"]

demangled = {}
names = sorted({k[2] for k in branches if k[2]} | {k[1] for k in functions})
if names:
    for a, b in zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()):
        demangled[a] = b.split("(")[0]
text = {}


def source(name, line):
    if name not in text:
        with open(os.path.join(csrc, name), errors="replace") as fh:
            text[name] = fh.read().splitlines()
    return text[name][line - 1].strip()[:150] if line <= len(text[name]) else ""


kernel = lambda name: name.endswith(".hip") or name.endswith(".h") or name.endswith(".inc")
print("# emulator coverage of the CPU suite: %d translation-unit profiles (the main coverage library and the libraries of tests/test_emu_variants.py)" % builds)
print("\n## per file: lines executed, branches taken at least once")
for name in sorted({k[0] for k in lines}):
    ls = [v for k, v in lines.items() if k[0] == name]
    bs = [v for k, v in branches.items() if k[0] == name]
    print("%-28s lines %5d / %5d  %6.2f %%    branches %5d / %5d  %s" % (name, sum(v > 0 for v in ls), len(ls), 100.0 * sum(v > 0 for v in ls) / len(ls),
                                                                      sum(v > 0 for v in bs), len(bs), "%6.2f %%" % (100.0 * sum(v > 0 for v in bs) / len(bs)) if bs else "   -"))
print("\n## never-executed lines of the kernel sources")
for (name, line), v in sorted(lines.items()):
    if v == 0 and kernel(name):
        print("%s:%d: %s" % (name, line, source(name, line)))
print("\n## functions and template instantiations of the kernel sources that never ran (their branches are not listed below)")
for (name, fn), v in sorted(functions.items()):
    if v == 0 and kernel(name):
        print("%s: %s" % (name, demangled.get(fn, fn)))
print("\n## never-taken branches of the kernel sources, in functions that ran (branch index / branches of that line in that function)")
per_line = collections.Counter((k[0], k[1], k[2]) for k in branches)
for (name, line, fn, i), v in sorted(branches.items()):
    if v == 0 and kernel(name) and lines[(name, line)] > 0 and functions.get((name, fn), 1) > 0:
        print("%s:%d: [%s] branch %d/%d: %s" % (name, line, demangled.get(fn, fn), i, per_line[(name, line, fn)], source(name, line)))
