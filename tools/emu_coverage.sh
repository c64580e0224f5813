#!/bin/bash
# Which lines and branches of the kernel sources does the CPU suite execute?  The kernel sources + the host side of the library are built for the CPU SIMT emulator
# with gcc's --coverage (-O1, otherwise the flags of tests/emu/Makefile), the whole CPU suite runs on that library (ORBX_EMU_LIB; the libraries that
# tests/test_emu_variants.py builds take --coverage through ORBX_EMU_EXTRA_FLAGS and leave their profiles in pytest's temporary directory), and
# tools/emu_coverage_report.py sums the profiles: per-file figures, never-executed lines, never-taken branches.  About a quarter of an hour on 8 cores.
# The emulator runs workgroups on several threads and gcc's default counter increments are plain: counts are lost under contention, and arcs that gcov derives by
# subtraction come out a few events off, below zero included - a branch taken a handful of times can read as never taken.  ORBX_COVERAGE_ATOMIC=1 builds with
# -fprofile-update=atomic (exact counts, but the suite then runs several times longer: meant for runs narrowed with -k).
# usage: tools/emu_coverage.sh [report file, default profiles/emu_coverage/after.txt] [further pytest arguments, e.g. -k search]
set -e
cd "$(dirname "$0")/.."
OUT=${1:-profiles/emu_coverage/after.txt}
shift || true
CSRC=orb_slam3_detailed_comments_amd/csrc
SRCS=$(grep "^SRCS" tests/emu/Makefile | sed "s/SRCS = //; s#\$(CSRC)#$CSRC#g")
WORK=$(mktemp -d /tmp/orbx_coverage.XXXXXX)
ATOMIC=""; [ "${ORBX_COVERAGE_ATOMIC:-0}" = 1 ] && ATOMIC="-fprofile-update=atomic"
mkdir -p "$WORK/main" "$(dirname "$OUT")"
make -C tests/emu -s                              # (the emu_lib fixture builds the -O2 library before it looks at ORBX_EMU_LIB: not while the workers start)
pids=""
for f in $SRCS; do                                # one object per translation unit: its .gcno / .gcda lie next to it
    g++ -O1 --coverage $ATOMIC -std=c++17 -ffp-contract=off -fwrapv -fno-gnu-unique -DORBX_EMU -Itests/emu -I$CSRC -fPIC -w -c -x c++ $f -o "$WORK/main/$(basename $f).o" &
    pids="$pids $!"
done
for p in $pids; do wait $p; done
# named like the default build: tests/test_bench_dist.py looks for that name in bench.py's result line
g++ -shared --coverage "$WORK"/main/*.o -o "$WORK/main/liborbx_emu.so" -lpthread
ORBX_EMU_LIB="$WORK/main/liborbx_emu.so" ORBX_EMU_EXTRA_FLAGS="-O1 --coverage $ATOMIC" python -m pytest tests -q -m "not gpu" --basetemp="$WORK/pytest" "$@" > "$WORK/suite.log" 2>&1 && RC=0 || RC=$?
tail -3 "$WORK/suite.log"
python tools/emu_coverage_report.py "$WORK" . > "$OUT"
echo "suite log: $WORK/suite.log   report: $OUT"
sed -n '/^## per file/,/^$/p' "$OUT"
# the report is written either way (what a failing run reached is worth reading), but a suite that failed or died half way gives figures that are too low
if [ $RC -ne 0 ]; then echo "WARNING: pytest ended with status $RC on the coverage build: the figures of $OUT are not those of a passing suite" >&2; exit $RC; fi
