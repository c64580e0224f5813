#!/usr/bin/env python3
"""Would a test notice a kernel line deciding wrongly?  A mutation pass over the DECISIONS of the match / search / vocabulary kernels, on the CPU SIMT emulator only.

For every mutant of tools/emu_mutants_list.py: copy csrc to a temporary directory (the tree is never edited), replace the mutant's old text - which must occur exactly
once in its file, so that the list cannot rot silently when a kernel is edited - by its new text, build the emulator library from the copy with the flags of
tests/emu/Makefile (g++ only: a mutant is never built for the device and never runs on one), and run the CPU test files named for the mutant on it:
    ORBX_EMU_LIB=<mutant library> python -m pytest <files> -m "not gpu" -x -q
killed (with the first failing test), survived, timeout, build_error or refused goes into a .jsonl file, one line per mutant, written as each finishes: a rerun skips what the file
already holds (--fresh starts over).  The unmutated objects are compiled once per pass; a mutant recompiles its own translation unit and links.

    python tools/emu_mutants.py                       every mutant -> profiles/emu_mutants/results_after.jsonl
    python tools/emu_mutants.py --only k_match        the mutants of files whose name contains k_match (comma-separated list)
    python tools/emu_mutants.py --ids 3,4             by id
    python tools/emu_mutants.py --without test_x.py   leave test files out (how results_before.jsonl was made: without the tests that the pass itself added)
    python tools/emu_mutants.py --carry before.jsonl  take the kills of an earlier pass as they are and run only what survived it
    python tools/emu_mutants.py --check               only verify that every old text occurs exactly once
    python tools/emu_mutants.py --jobs 2              mutants side by side (default 1: each pytest run already spreads over the cores)
A survivor is a gap in the suite unless the list carries a note for it (`note`: why the mutant is equivalent or why no input reaches the line); the summary at the end
names the survivors without one and the exit status is 1 when there are any.  Not part of the test suite or the benchmark: a tool to run after editing a kernel's decisions."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")


def emu_sources():
    """the translation units of tests/emu/Makefile, as file names inside csrc"""
    for line in open(os.path.join(EMU, "Makefile")):
        if line.startswith("SRCS"):
            return [os.path.basename(w) for w in line.split("=", 1)[1].split()]
    raise SystemExit("tests/emu/Makefile has no SRCS line")


def emu_flags(src_dir):
    """the compile flags of tests/emu/Makefile (tests/test_emu_variants.py::build_emu_variant has the same line), for sources in src_dir"""
    return ["-O2", "-std=c++17", "-ffp-contract=off", "-fwrapv", "-fno-gnu-unique", "-DORBX_EMU", "-I" + EMU, "-I" + src_dir, "-fPIC", "-w"]


def compile_unit(src_dir, name, obj):
    return subprocess.run(["g++"] + emu_flags(src_dir) + ["-c", "-x", "c++", os.path.join(src_dir, name), "-o", obj], capture_output=True, text=True)


def edits(m):
    return [(m["old"], m["new"])] + [tuple(e) for e in m.get("more", ())]


def apply_mutant(m, src_dir):
    """rewrite m's file inside src_dir; the old text must be there exactly once"""
    path = os.path.join(src_dir, m["file"])
    text = open(path).read()
    for old, new in edits(m):
        n = text.count(old)
        if n != 1:
            raise ValueError("mutant %d: the old text occurs %d times in %s (must be exactly once): %r" % (m["id"], n, m["file"], old))
        if old == new:
            raise ValueError("mutant %d changes nothing" % m["id"])
        text = text.replace(old, new)
    open(path, "w").write(text)


def first_failure(out):
    hit = re.search(r"^(?:FAILED|ERROR) (\S+)", out, re.M)
    if hit:
        return hit.group(1)
    hit = re.search(r"^\[gw\d+\] .*?(tests/\S+::\S+)", out, re.M) or re.search(r"(tests/\S+::\S+)", out)
    return hit.group(1) if hit else None


def test_files(m, without):
    """the mutant's test files that exist and are not left out"""
    return [f for f in m["tests"] if f not in without and os.path.exists(os.path.join(ROOT, "tests", f))]


def run_mutant(m, base, work, without, timeout):
    """build and test one mutant; base: the copy of csrc with the unmutated objects in base/obj"""
    rec = dict(id=m["id"], file=m["file"], intent=m["intent"], edits=[list(e) for e in edits(m)])
    if m.get("note"):
        rec["note"] = m["note"]
    d = os.path.join(work, "m%03d" % m["id"])
    src = os.path.join(d, "csrc")
    shutil.copytree(base, src, ignore=shutil.ignore_patterns("obj"))
    t0 = time.time()
    try:
        apply_mutant(m, src)
    except ValueError as e:
        rec.update(verdict="refused", detail=str(e))
        return rec
    # what includes a mutated header is every unit; a mutated unit is itself
    units = emu_sources()
    mine = [m["file"]] if m["file"] in units else units
    objs = []
    for u in units:
        if u in mine:
            o = os.path.join(d, u + ".o")
            r = compile_unit(src, u, o)
            if r.returncode:
                rec.update(verdict="build_error", detail=r.stderr[-400:], build_s=round(time.time() - t0, 1))
                return rec
        else:
            o = os.path.join(base, "obj", u + ".o")
        objs.append(o)
    so = os.path.join(d, "liborbx_emu.so")                      # named like the default build: tests/test_bench_dist.py looks for that name
    r = subprocess.run(["g++", "-shared"] + objs + ["-o", so, "-lpthread"], capture_output=True, text=True)
    if r.returncode:
        rec.update(verdict="build_error", detail=r.stderr[-400:], build_s=round(time.time() - t0, 1))
        return rec
    rec["build_s"] = round(time.time() - t0, 1)
    files = test_files(m, without)
    rec["tests"] = files
    if not files:                                               # (pytest without a path would collect the whole tree)
        rec.update(verdict="refused", detail="none of the mutant's test files is left: %s" % m["tests"])
        shutil.rmtree(d, ignore_errors=True)
        return rec
    t1 = time.time()
    env = dict(os.environ, ORBX_EMU_LIB=so)
    cmd = [sys.executable, "-m", "pytest"] + [os.path.join("tests", f) for f in files] + ["-m", "not gpu", "-x", "-q", "-rfE", "-p", "no:cacheprovider", "--basetemp=" + os.path.join(d, "pytest")]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
        out, rc = r.stdout + r.stderr, r.returncode
    except subprocess.TimeoutExpired as e:
        out, rc = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), "timeout"
    rec["test_s"] = round(time.time() - t1, 1)
    if rc == 0:
        rec["verdict"] = "survived"
    elif rc == 5:
        rec.update(verdict="refused", detail="no test collected from %s" % files)
    elif rc == "timeout":                                       # a verdict of its own: a hang is noticed, but no test says what is wrong
        rec.update(verdict="timeout", detail="the tests did not end within %d s" % timeout)
    else:
        rec.update(verdict="killed", first_failing_test=first_failure(out))
        if rec["first_failing_test"] is None:
            rec["detail"] = out[-300:]
    shutil.rmtree(d, ignore_errors=True)
    return rec


def table(before, after, mutants):
    """the markdown table of profiles/emu_mutants/README.md from two results files"""
    load = lambda path: {json.loads(l)["id"]: json.loads(l) for l in open(path) if l.strip()}
    b, a = load(before), load(after)
    short = lambda r: "-" if r is None else r["verdict"] + (" (carried)" if r.get("carried") else "")
    killer = lambda r: (r.get("first_failing_test") or "").replace("tests/", "") if r and r["verdict"] == "killed" else ""
    print("| id | file | mutant | before | after | first killing test | s |")
    print("|---|---|---|---|---|---|---|")
    for m in mutants:
        rb, ra = b.get(m["id"]), a.get(m["id"])
        if rb is None and ra is None:
            continue
        r = ra or rb
        print("| %d | `%s` | %s: `%s` -> `%s` | %s | %s | `%s` | %.0f |" % (m["id"], m["file"].replace(".hip", ""), m["intent"], m["old"].strip().replace("|", "\\|").replace("\n", " "),
                                                                    m["new"].strip().replace("|", "\\|").replace("\n", " "), short(rb), short(ra), killer(ra) or killer(rb),
                                                                    (r.get("build_s", 0) + r.get("test_s", 0))))


def main():
    from emu_mutants_list import MUTANTS
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="comma-separated substrings of the mutated file's name")
    ap.add_argument("--ids", default="", help="comma-separated mutant ids")
    ap.add_argument("--without", default="", help="comma-separated test files to leave out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emu_mutants", "results_after.jsonl"))
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per mutant's test run")
    ap.add_argument("--fresh", action="store_true", help="forget what --out already holds")
    ap.add_argument("--carry", default="", help="results file of an earlier pass: its kills, and its survivors whose test files are the same now, are copied (marked carried) instead of "
                                                "run again - right only while the existing tests and the kernels are unchanged since, e.g. results_before.jsonl when tests were added and nothing else")
    ap.add_argument("--check", action="store_true", help="verify the list against the sources and stop")
    ap.add_argument("--table", nargs=2, metavar=("BEFORE", "AFTER"), help="print the markdown table of two results files and stop")
    a = ap.parse_args()
    if a.table:
        table(a.table[0], a.table[1], MUTANTS)
        return 0

    ids = [m["id"] for m in MUTANTS]
    assert len(set(ids)) == len(ids), "duplicate mutant ids"
    bad = 0
    for m in MUTANTS:                                           # the whole list is verified, whatever is selected
        text = open(os.path.join(CSRC, m["file"])).read()
        for old, _ in edits(m):
            if text.count(old) != 1:
                print("mutant %d (%s): the old text occurs %d times, must be exactly once: %r" % (m["id"], m["file"], text.count(old), old))
                bad += 1
        if not m["tests"]:
            print("mutant %d names no test file" % m["id"]); bad += 1
    if bad:
        return 2
    if a.check:
        print("%d mutants, every old text occurs exactly once" % len(MUTANTS))
        return 0

    chosen = MUTANTS
    if a.only:
        chosen = [m for m in chosen if any(s in m["file"] for s in a.only.split(","))]
    if a.ids:
        want = {int(x) for x in a.ids.split(",")}
        chosen = [m for m in chosen if m["id"] in want]
    without = set(filter(None, a.without.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    done = {}
    if os.path.exists(a.out) and not a.fresh:
        for line in open(a.out):
            if line.strip():
                r = json.loads(line); done[r["id"]] = r
    elif a.fresh and os.path.exists(a.out):
        os.remove(a.out)
    if a.carry:
        texts = {m["id"]: [list(e) for e in edits(m)] for m in chosen}
        by_id = {m["id"]: m for m in chosen}
        with open(a.out, "a") as f:
            for line in open(a.carry):
                r = json.loads(line) if line.strip() else None
                if not r or r["id"] not in texts or r["id"] in done or r.get("edits") != texts[r["id"]]:
                    continue
                # a kill stands; a survivor's verdict stands only if the very same test files would run now
                if r["verdict"] == "killed" or (r["verdict"] == "survived" and r.get("tests") == test_files(by_id[r["id"]], without)):
                    r["carried"] = True; done[r["id"]] = r
                    f.write(json.dumps(r) + "\n")
    todo = [m for m in chosen if m["id"] not in done]
    print("%d mutants selected, %d already in %s" % (len(chosen), len(chosen) - len(todo), a.out))

    t_pass = time.time()
    work = tempfile.mkdtemp(prefix="orbx_mutants.")
    try:
        if todo:
            subprocess.run(["make", "-C", EMU, "-s"], check=True)   # (the emu_lib fixture builds the default library before it looks at ORBX_EMU_LIB: not while the workers start)
            base = os.path.join(work, "base")
            shutil.copytree(CSRC, base)
            os.makedirs(os.path.join(base, "obj"))
            with ThreadPoolExecutor(min(8, os.cpu_count() or 2)) as ex:
                for u, r in zip(emu_sources(), ex.map(lambda u: compile_unit(base, u, os.path.join(base, "obj", u + ".o")), emu_sources())):
                    if r.returncode:
                        raise SystemExit("the unmutated %s does not build:\n%s" % (u, r.stderr[-800:]))
            print("unmutated objects: %.0f s" % (time.time() - t_pass))

        def one(m):
            r = run_mutant(m, base, work, without, a.timeout)
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
            print("%3d %-12s %-11s %5.0f s  %s%s" % (r["id"], r["file"], r["verdict"], r.get("build_s", 0) + r.get("test_s", 0), r["intent"],
                                                    "  <- " + str(r.get("first_failing_test")) if r["verdict"] == "killed" else ""), flush=True)
            return r
        with ThreadPoolExecutor(max(1, a.jobs)) as ex:
            for r in ex.map(one, todo):
                done[r["id"]] = r
    finally:
        shutil.rmtree(work, ignore_errors=True)

    rows = [done[m["id"]] for m in chosen if m["id"] in done]
    count = {v: sum(r["verdict"] == v for r in rows) for v in ("killed", "survived", "timeout", "build_error", "refused")}
    notes = {m["id"]: m.get("note") for m in MUTANTS}             # (the list's notes as they are now, not as an earlier run recorded them)
    open_ = [r for r in rows if r["verdict"] == "survived" and not notes.get(r["id"])]
    print("%d mutants: %s; survivors without a note: %s; this run %.0f s" % (len(rows), count, [r["id"] for r in open_] or "none", time.time() - t_pass))
    return 1 if open_ or count["build_error"] or count["refused"] or count["timeout"] else 0


if __name__ == "__main__":
    sys.exit(main())
