#!/usr/bin/env python3
"""Would a test notice a kernel line deciding wrongly?  A mutation pass over the DECISIONS of the kernels (match / search / vocabulary: ids below 405; extraction - FAST,
quadtree, pyramid, blur, orientation and BRIEF, input stage - and the host tables of orbx_api.cpp that feed it: ids from 405) and of the host replays of the single-frame
matcher entries in orbm_search.cpp (ids from 1000: host code is a translation unit of the emulator library like any kernel file), on the CPU SIMT emulator only - and over the
drop-in facade headers of include/orb_slam3_amd (ids from 2000), which are compiled into the test drivers, not into the library.  Ids from 3000 are the state-carrying code:
the resident map's kernels and host code (k_map_* of k_search.hip, the map and batch entries of orbm_search.cpp), the resident key frames and the key frame database of orbv_api.cpp.

For every mutant of tools/emu_mutants_list.py: copy csrc to a temporary directory (the tree is never edited), replace the mutant's old text - which must occur exactly
once in its file, so that the list cannot rot silently when a kernel is edited - by its new text, build the emulator library from the copy with the flags of
tests/emu/Makefile (g++ only: a mutant is never built for the device and never runs on one), and run the CPU test files named for the mutant on it:
    ORBX_EMU_LIB=<mutant library> python -m pytest <files> -m "not gpu" -x -q
killed (with the first failing test), survived, crashed, timeout, build_error or refused goes into a .jsonl file, one line per mutant, written as each finishes: a rerun skips what
the file already holds (--fresh starts over).  The unmutated objects are compiled once per pass; a mutant recompiles its own translation unit - for a mutated header the units
that include it, directly or through another header of csrc (a textual scan of the copy) - and links.
A mutant may carry `defines` (("-DORBX_FAST_LIST_CAP=200",): the switches of tests/test_emu_variants.py): its whole library, the unmutated objects included, is then built with
them - for decisions that the default build reaches only on very large or very dense images.  Its test files must take the `emu_lib` fixture (tests/test_emu_variants.py builds
its own libraries from the tree and would not see the mutant).  A test may be named as a file or as a pytest node id (`test_x.py::test_y`, `test_x.py::test_y[case]`) where the
whole file takes minutes on the emulator; files are run in the order given, cheapest first, and the run stops at the first failure.
A mutant whose file is named from the repository root (include/orb_slam3_amd/ORBmatcher.h) is a header's: a copy of include/ takes the edit, the emulator library stays the
unmutated one of tests/emu (built once per pass), oracle/_ref/libmw_facade.so - and libmw_facade_full.so where the mutant's group names a test that loads it - is built from the
copy into the temporary directory by the recipe of oracle/Makefile (FACADE_INC, FACADE_OUT), and the tests run with ORBX_FACADE_INCLUDE / ORBX_MW_FACADE_LIB /
ORBX_MW_FACADE_FULL_LIB naming them (tests/oracle_lib.py: facade_include, include_root, mw_facade_lib).  tests/test_callers_compile.py reads objects made from the real headers
and is refused in such a mutant's group.
crashed: pytest, or one of its workers, ended on a signal (a negative return status, "worker .. crashed").  That is no kill: a mutant that can index outside its arrays is a
defect of the LIST (it breaks the list's safety rule), and the pass fails on it.

    python tools/emu_mutants.py                       every mutant -> profiles/emu_mutants/results_after.jsonl
    python tools/emu_mutants.py --only k_match        the mutants of files whose name contains k_match (comma-separated list)
    python tools/emu_mutants.py --only orbm_search    the host replays (profiles/emu_mutants_host/: --out / --carry / --base name that directory's files)
    python tools/emu_mutants.py --only include/       the facade headers (profiles/emu_mutants_facade/)
    python tools/emu_mutants.py --ids 3000,3001,..    the resident map, key frames and database (profiles/emu_mutants_map/: its README has the whole command)
    python tools/emu_mutants.py --ids 3,4             by id
    python tools/emu_mutants.py --without test_x.py   leave test files out (how results_before.jsonl was made: without the tests that the pass itself added)
    python tools/emu_mutants.py --carry before.jsonl  take the kills of an earlier pass as they are and run only what survived it
    python tools/emu_mutants.py --base first.jsonl    the same without copying them into --out (how profiles/emu_mutants_extract/ stands next to the first pass's file)
    python tools/emu_mutants.py --check               only verify that every old text occurs exactly once
    python tools/emu_mutants.py --jobs 2              mutants side by side (default 1: each pytest run already spreads over the cores)
A survivor is a gap in the suite unless the list carries a note for it (`note`: why the mutant is equivalent or why no input reaches the line); the summary at the end
names the survivors without one and the exit status is 1 when there are any.  Not part of the test suite or the benchmark: a tool to run after editing a kernel's decisions."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
INCLUDE = os.path.join(ROOT, "include")
ORACLE = os.path.join(ROOT, "oracle")
# the tests that load oracle/_ref/libmw_facade.so (tests/oracle_lib.py::mw_facade_lib) - and, of these, what loads libmw_facade_full.so: the `real` tests of
# tests/test_matcher_reference.py (a mutant's group names them by node id, or the whole file)
MW_TESTS = ("test_matcher_reference.py", "test_lifetime.py", "test_matcher_gates.py")
MW_FULL_NODES = ("real",)


def is_facade(m):
    """a mutant of a drop-in header: its file is named from the repository root (include/orb_slam3_amd/ORBmatcher.h), not inside csrc"""
    return m["file"].startswith("include/")


def source_path(m):
    return os.path.join(ROOT, m["file"]) if is_facade(m) else os.path.join(CSRC, m["file"])


def needs_mw(files, full=False):
    """does one of the test files / node ids load the matcher-world facade library (full: the one over the reference's own Frame / KeyFrame / MapPoint)"""
    for f in files:
        name, _, node = f.partition("::")
        if name in MW_TESTS and (not full or (name == "test_matcher_reference.py" and (not node or any(w in node for w in MW_FULL_NODES)))):
            return True
    return False


def emu_sources():
    """the translation units of tests/emu/Makefile, as file names inside csrc"""
    for line in open(os.path.join(EMU, "Makefile")):
        if line.startswith("SRCS"):
            return [os.path.basename(w) for w in line.split("=", 1)[1].split()]
    raise SystemExit("tests/emu/Makefile has no SRCS line")


def emu_flags(src_dir, defines=()):
    """the compile flags of tests/emu/Makefile (tests/test_emu_variants.py::build_emu_variant has the same line), for sources in src_dir"""
    return ["-O2", "-std=c++17", "-ffp-contract=off", "-fwrapv", "-fno-gnu-unique", "-DORBX_EMU", "-I" + EMU, "-I" + src_dir, "-fPIC", "-w"] + list(defines)


def compile_unit(src_dir, name, obj, defines=()):
    return subprocess.run(["g++"] + emu_flags(src_dir, defines) + ["-c", "-x", "c++", os.path.join(src_dir, name), "-o", obj], capture_output=True, text=True)


def includers(src_dir, header, units):
    """the units of `units` that include `header` of src_dir, directly or through other files of src_dir: a textual scan of #include "..." lines"""
    direct = {}
    for name in os.listdir(src_dir):
        path = os.path.join(src_dir, name)
        if os.path.isfile(path):
            direct[name] = set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path, errors="replace").read(), re.M))
    reach = {header}
    grown = True
    while grown:
        grown = False
        for name, inc in direct.items():
            if name not in reach and inc & reach:
                reach.add(name); grown = True
    return [u for u in units if u in reach]


_base_objs = {}
_base_lock = threading.Lock()


def base_objects(base, defines):
    """the directory with the unmutated objects built with `defines` (compiled once per pass and set of defines)"""
    key = tuple(defines)
    with _base_lock:
        if key not in _base_objs:
            d = os.path.join(base, "obj" if not key else "obj_%d" % len(_base_objs))
            os.makedirs(d, exist_ok=True)
            with ThreadPoolExecutor(min(8, os.cpu_count() or 2)) as ex:
                for u, r in zip(emu_sources(), ex.map(lambda u: compile_unit(base, u, os.path.join(d, u + ".o"), key), emu_sources())):
                    if r.returncode:
                        raise SystemExit("the unmutated %s does not build with %s:\n%s" % (u, list(key), r.stderr[-800:]))
            _base_objs[key] = d
        return _base_objs[key]


def edits(m):
    return [(m["old"], m["new"])] + [tuple(e) for e in m.get("more", ())]


def edits_sha(m):
    """what a results record keeps of the mutant's texts: enough to see that the list still says the same"""
    return hashlib.sha1(json.dumps([list(e) for e in edits(m)]).encode()).hexdigest()[:12]


def same_mutant(r, m):
    return r["edits"] == [list(e) for e in edits(m)] if "edits" in r else r.get("edits_sha") == edits_sha(m)


def tests_sha(files):
    """what a survivor of a header's mutant survived: the contents of its test files and of everything they compile or run (tests/cpp, the world runner, the helpers) -
    a check strengthened INSIDE an existing driver changes it, which the list of file names alone would not show"""
    h = hashlib.sha1()
    names = sorted({f.split("::")[0] for f in files}) + ["matcher_world.py", "oracle_lib.py"] + sorted("cpp/" + n for n in os.listdir(os.path.join(ROOT, "tests", "cpp")))
    for n in names:
        h.update(n.encode()); h.update(open(os.path.join(ROOT, "tests", n), "rb").read())
    return h.hexdigest()[:12]


def stands(r, m, without):
    """a kill of an earlier run stands; a survivor's verdict stands only if the very same test files would run now - for a header's mutant (ids from 2000) with the very
    same contents (tests_sha: a record without one is run again)"""
    if not same_mutant(r, m):
        return False
    if r["verdict"] == "killed":
        return True
    files = test_files(m, without)
    return r["verdict"] == "survived" and r.get("tests") == files and (not is_facade(m) or r.get("tests_sha") == tests_sha(files))


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
    return [f for f in m["tests"] if f.split("::")[0] not in without and os.path.exists(os.path.join(ROOT, "tests", f.split("::")[0]))]


def crashed(rc, out):
    """pytest itself, or a worker of pytest-xdist, ended on a signal"""
    return (isinstance(rc, int) and (rc < 0 or rc >= 128)) or re.search(r"crashed while running|Fatal Python error|node down: Not properly terminated", out) is not None


def run_tests(rec, m, d, files, env, timeout):
    """the mutant's test files under `env`; the verdict goes into rec"""
    t1 = time.time()
    cmd = [sys.executable, "-m", "pytest"] + [os.path.join("tests", f) for f in files] + ["-m", "not gpu", "-x", "-q", "-rfE", "-p", "no:cacheprovider", "--basetemp=" + os.path.join(d, "pytest")]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
        out, rc = r.stdout + r.stderr, r.returncode
    except subprocess.TimeoutExpired as e:
        out, rc = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), "timeout"
    rec["test_s"] = round(time.time() - t1, 1)
    if rc == 0:
        rec.update(verdict="survived", tests=files)             # (what it survived: --carry runs it again when the files change)
    elif rc == 5:
        rec.update(verdict="refused", detail="no test collected from %s" % files)
    elif crashed(rc, out):                                      # no kill: the mutant broke the list's safety rule
        rec.update(verdict="crashed", first_failing_test=(first_failure(out) or "").strip("'\"") or None, detail=out[-300:])
    elif rc == "timeout":                                       # a verdict of its own: a hang is noticed, but no test says what is wrong
        rec.update(verdict="timeout", detail="the tests did not end within %d s" % timeout)
    else:
        rec.update(verdict="killed", first_failing_test=first_failure(out))
        if rec["first_failing_test"] is None:
            rec["detail"] = out[-300:]
    return rec


def run_facade_mutant(m, work, without, timeout):
    """a mutant of a header under include/orb_slam3_amd: a copy of include/ with the edit, the matcher-world facade libraries built from the copy by the recipe of
    oracle/Makefile where the mutant's tests load them, and the tests pointed at both (tests/oracle_lib.py: ORBX_FACADE_INCLUDE, ORBX_MW_FACADE_LIB,
    ORBX_MW_FACADE_FULL_LIB).  The emulator library is the unmutated one of tests/emu (built once per pass, in main)."""
    rec = dict(id=m["id"], file=m["file"], intent=m["intent"], edits_sha=edits_sha(m))
    d = os.path.join(work, "m%03d" % m["id"])
    inc = os.path.join(d, "include")
    shutil.copytree(INCLUDE, inc)
    t0 = time.time()
    try:
        apply_mutant(dict(m, file=os.path.relpath(m["file"], "include")), inc)
    except ValueError as e:
        rec.update(verdict="refused", detail=str(e))
        shutil.rmtree(d, ignore_errors=True)
        return rec
    files = test_files(m, without)
    if not files:
        rec.update(verdict="refused", detail="none of the mutant's test files is left: %s" % m["tests"])
        shutil.rmtree(d, ignore_errors=True)
        return rec
    env = dict(os.environ, ORBX_FACADE_INCLUDE=inc)
    env.pop("ORBX_EMU_LIB", None)
    targets = [("libmw_facade.so", "ORBX_MW_FACADE_LIB")] * needs_mw(files) + [("libmw_facade_full.so", "ORBX_MW_FACADE_FULL_LIB")] * needs_mw(files, full=True)
    if targets:
        r = subprocess.run(["make", "-C", ORACLE, "-j2", "FACADE_INC=" + inc, "FACADE_OUT=" + d] + [os.path.join(d, t) for t, _ in targets], capture_output=True, text=True)
        if r.returncode:
            rec.update(verdict="build_error", detail=r.stderr[-400:], build_s=round(time.time() - t0, 1))
            shutil.rmtree(d, ignore_errors=True)
            return rec
        for t, var in targets:
            env[var] = os.path.join(d, t)
    rec["build_s"] = round(time.time() - t0, 1)
    run_tests(rec, m, d, files, env, timeout)
    if rec["verdict"] == "survived":
        rec["tests_sha"] = tests_sha(files)
    shutil.rmtree(d, ignore_errors=True)
    return rec


def run_mutant(m, base, work, without, timeout):
    """build and test one mutant; base: the copy of csrc, the unmutated objects beside it (base_objects)"""
    if is_facade(m):
        return run_facade_mutant(m, work, without, timeout)
    # (a record is small: note and texts are the list's, which a record only has to be matched against - edits_sha; the first pass's records hold them in full)
    rec = dict(id=m["id"], file=m["file"], intent=m["intent"], edits_sha=edits_sha(m))
    defines = tuple(m.get("defines") or ())
    if defines:
        rec["defines"] = list(defines)
    d = os.path.join(work, "m%03d" % m["id"])
    src = os.path.join(d, "csrc")
    shutil.copytree(base, src, ignore=shutil.ignore_patterns("obj", "obj_*"))
    t0 = time.time()
    try:
        apply_mutant(m, src)
    except ValueError as e:
        rec.update(verdict="refused", detail=str(e))
        return rec
    # a mutated unit is itself; a mutated header is the units that include it
    units = emu_sources()
    mine = [m["file"]] if m["file"] in units else includers(src, m["file"], units)
    objdir = base_objects(base, defines)
    objs = []
    for u in units:
        if u in mine:
            o = os.path.join(d, u + ".o")
            r = compile_unit(src, u, o, defines)
            if r.returncode:
                rec.update(verdict="build_error", detail=r.stderr[-400:], build_s=round(time.time() - t0, 1))
                return rec
        else:
            o = os.path.join(objdir, u + ".o")
        objs.append(o)
    so = os.path.join(d, "liborbx_emu.so")                      # named like the default build: tests/test_bench_dist.py looks for that name
    r = subprocess.run(["g++", "-shared"] + objs + ["-o", so, "-lpthread"], capture_output=True, text=True)
    if r.returncode:
        rec.update(verdict="build_error", detail=r.stderr[-400:], build_s=round(time.time() - t0, 1))
        return rec
    rec["build_s"] = round(time.time() - t0, 1)
    files = test_files(m, without)
    if not files:                                               # (pytest without a path would collect the whole tree)
        rec.update(verdict="refused", detail="none of the mutant's test files is left: %s" % m["tests"])
        shutil.rmtree(d, ignore_errors=True)
        return rec
    run_tests(rec, m, d, files, dict(os.environ, ORBX_EMU_LIB=so), timeout)
    shutil.rmtree(d, ignore_errors=True)
    return rec


def table(before, after, mutants, brief=False):
    """the markdown table of profiles/emu_mutants/README.md from two results files; brief: without the texts (the list has them) and the file column"""
    load = lambda path: {json.loads(l)["id"]: json.loads(l) for l in open(path) if l.strip()}
    b, a = load(before), load(after)
    short = lambda r: "-" if r is None else r["verdict"] + (" (carried)" if r.get("carried") else "")
    killer = lambda r: (r.get("first_failing_test") or "").replace("tests/", "") if r and r["verdict"] == "killed" else ""
    print("| id | mutant | before | after | first killing test | s |\n|---|---|---|---|---|---|" if brief else
          "| id | file | mutant | before | after | first killing test | s |\n|---|---|---|---|---|---|---|")
    for m in mutants:
        rb, ra = b.get(m["id"]), a.get(m["id"])
        if rb is None and ra is None:
            continue
        if ra is None and rb["verdict"] == "killed":            # (an after file made with --base before: a kill stands and is not repeated)
            ra = dict(rb, carried=True)
        r = ra or rb
        if brief:
            print("| %d | %s | %s | %s | `%s` | %.0f |" % (m["id"], m["intent"], short(rb), short(ra), killer(ra) or killer(rb), r.get("build_s", 0) + r.get("test_s", 0)))
            continue
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
    ap.add_argument("--base", default="", help="like --carry, but what stands of the file(s, comma-separated) is only counted, not copied into --out (a second pass's record next to the first's, "
                                               "without a copy of it).  Right under the same condition as --carry: tests and kernels unchanged since.  Ignored under --fresh")
    ap.add_argument("--check", action="store_true", help="verify the list against the sources and stop")
    ap.add_argument("--table", nargs=2, metavar=("BEFORE", "AFTER"), help="print the markdown table of two results files and stop")
    ap.add_argument("--brief", action="store_true", help="--table without the mutants' texts")
    a = ap.parse_args()
    if a.table:
        table(a.table[0], a.table[1], MUTANTS, a.brief)
        return 0

    ids = [m["id"] for m in MUTANTS]
    assert len(set(ids)) == len(ids), "duplicate mutant ids"
    bad = 0
    for m in MUTANTS:                                           # the whole list is verified, whatever is selected
        text = open(source_path(m)).read()
        for old, _ in edits(m):
            if text.count(old) != 1:
                print("mutant %d (%s): the old text occurs %d times, must be exactly once: %r" % (m["id"], m["file"], text.count(old), old))
                bad += 1
        if not m["tests"]:
            print("mutant %d names no test file" % m["id"]); bad += 1
        if is_facade(m) and any(t.startswith("test_callers_compile.py") for t in m["tests"]):   # (it reads objects made from the real headers at build time)
            print("mutant %d: tests/test_callers_compile.py cannot see a mutated header" % m["id"]); bad += 1
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
    by_id = {m["id"]: m for m in chosen}
    if a.carry:
        with open(a.out, "a") as f:
            for line in open(a.carry):
                r = json.loads(line) if line.strip() else None
                if r and r["id"] in by_id and r["id"] not in done and stands(r, by_id[r["id"]], without):
                    r["carried"] = True; done[r["id"]] = r
                    f.write(json.dumps(r) + "\n")
    for path in (a.base.split(",") if a.base and not a.fresh else ()):
        for line in open(path):
            r = json.loads(line) if line.strip() else None
            if r and r["id"] in by_id and r["id"] not in done and stands(r, by_id[r["id"]], without):
                done[r["id"]] = dict(r, carried=True)
    todo = [m for m in chosen if m["id"] not in done]
    print("%d mutants selected, %d already in %s%s" % (len(chosen), len(chosen) - len(todo), a.out, " or " + a.base if a.base else ""))

    t_pass = time.time()
    work = tempfile.mkdtemp(prefix="orbx_mutants.")
    try:
        if todo:
            subprocess.run(["make", "-C", EMU, "-s"], check=True)   # (the emu_lib fixture builds the default library before it looks at ORBX_EMU_LIB: not while the workers start)
            base = os.path.join(work, "base")
            shutil.copytree(CSRC, base)
            if not all(is_facade(m) for m in todo):
                base_objects(base, ())
                print("unmutated objects: %.0f s" % (time.time() - t_pass))
            if any(is_facade(m) for m in todo):                 # the oracle's libraries (the reference builds among them) before the workers ask for them
                subprocess.run(["make", "-C", ORACLE, "-j8", "-s"], check=True, stdout=subprocess.DEVNULL)

        def one(m):
            r = run_mutant(m, base, work, without, a.timeout)
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
            print("%3d %-12s %-11s %5.0f s  %s%s" % (r["id"], r["file"], r["verdict"], r.get("build_s", 0) + r.get("test_s", 0), m["intent"],
                                                    "  <- " + str(r.get("first_failing_test")) if r["verdict"] == "killed" else ""), flush=True)
            return r
        with ThreadPoolExecutor(max(1, a.jobs)) as ex:
            for r in ex.map(one, todo):
                done[r["id"]] = r
    finally:
        shutil.rmtree(work, ignore_errors=True)

    rows = [done[m["id"]] for m in chosen if m["id"] in done]
    count = {v: sum(r["verdict"] == v for r in rows) for v in ("killed", "survived", "crashed", "timeout", "build_error", "refused")}
    notes = {m["id"]: m.get("note") for m in MUTANTS}             # (the list's notes as they are now, not as an earlier run recorded them)
    open_ = [r for r in rows if r["verdict"] == "survived" and not notes.get(r["id"])]
    print("%d mutants: %s; survivors without a note: %s; this run %.0f s" % (len(rows), count, [r["id"] for r in open_] or "none", time.time() - t_pass))
    return 1 if open_ or count["build_error"] or count["refused"] or count["timeout"] or count["crashed"] else 0


if __name__ == "__main__":
    sys.exit(main())
